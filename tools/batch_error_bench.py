#!/usr/bin/env python3
"""Batch quantisation-error report (NetworkBatch.error_plan) against the two ways to get the same numbers without it, on
the GPU (warm-up, alternating legs, medians of --reps), for a batch of --batch MobileNetV2
(synthetic.build('mobilenet_v2', seed=s % 4), BatchNorm folded):

  * (a) BatchErrorPlan.run() between device events for one configuration, (8, per tensor, asymmetric), and for four, and the
    TB/s they imply at 8 B per weight (every weight read twice, nothing written but the small block), alternating with
    BatchTablePlan.run() -- one read of the same bytes -- and next to the read rate tools/litmus/hbm_stream reports in the
    same job, if it has been built;
  * (b) clone + quant_plan: a copy of the batch allocation, BatchQuantPlan.run() (per tensor, no codes, no biases), then per
    network and layer a torch subtraction and the three reductions, gathered into one tensor and read once -- between device
    events, the weights restored in front of every repetition outside the measurement.  It moves at least 8 B (copy) + 12 B
    (quantise) + 12 B (subtract) per weight, before the reductions;
  * (c) the loop: ``dfq._quantize_error(w, 8, 'sum')`` and ``'mean'`` per layer and network, each with its host read, by the
    host's clock.

    python tools/batch_error_bench.py [--reps 25] [--warmup 3] [--batch 64] [--loop-reps 3] [--out profiles/batch_error_bench.json]

Kernel durations come from a separate `rocprofv3 --kernel-trace --stats -- python tools/batch_error_bench.py --reps 3 --loop-reps 1`.
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dfq_amd import _ffi, arena, dfq                                   # noqa: E402
from batch_bench_common import alternate, emit, events, wall, nets as _nets   # noqa: E402
from batch_table_bench import litmus_read                             # noqa: E402

TARG = [nn.Conv2d, nn.Linear]
ONE = ((8, False, False),)
FOUR = ((8, False, False), (8, True, False), (8, False, True), (4, True, True))


def _stat(samples):
    return {'median_us': statistics.median(samples), 'spread_us': [min(samples), max(samples)], 'reps': len(samples)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=25)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--loop-reps', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    dev = torch.device('cuda', 0)
    nets = _nets(args.batch, dev, TARG)
    batch = arena.NetworkBatch(nets, TARG)
    torch.cuda.synchronize()
    one, four, table = batch.error_plan(ONE), batch.error_plan(FOUR), batch.table_plan()
    quant = batch.quant_plan(8, 32, per_channel=False, codes=None)
    pristine = batch.storage.clone()
    keys = one.keys
    res = {'networks': args.batch, 'layers': one.n_tensors, 'weights_per_network': one.elements, 'launches': one.launches,
           'configs_one': [list(c) for c in ONE], 'configs_four': [list(c) for c in FOUR]}

    # (b) what a user does at the parent commit with the batch plans: copy, quantise in place, subtract, reduce
    base = batch.storage.data_ptr()
    where = [[((g[k].weight.data_ptr() - base) // 4, g[k].weight.numel()) for k in keys] for (g, _, _) in nets]

    def clone_quant():
        snap = batch.storage.clone().view(-1)
        quant.run()
        rows = []
        for n, (g, _, _) in enumerate(nets):
            for (off, numel), k in zip(where[n], keys):
                e = g[k].weight.detach().view(-1) - snap[off:off + numel]
                rows.append(torch.stack([e.sum(dtype=torch.float64), e.abs().sum(dtype=torch.float64), e.double().square().sum()]))
        return torch.stack(rows).cpu()

    def restore():
        batch.storage.copy_(pristine)

    def ev(fn):
        return events(fn, restore)

    # the sums of (b) against the plan's, so that the legs compute the same thing (float64 sums in another order)
    one.run()
    _ffi.synchronize()
    mine = one.block.cpu().view(args.batch, one.n_tensors, 4)[:, :, 1:].reshape(-1, 3)
    theirs = clone_quant()
    restore()
    torch.cuda.synchronize()
    scale = mine.abs()[:, 1:2].clamp_min(1e-300)
    res['max_rel_difference_to_clone_quant'] = float(((mine - theirs).abs() / scale).max())
    assert res['max_rel_difference_to_clone_quant'] < 1e-9, 'the legs do not compute the same sums'

    t = alternate({'run_one': (one.run, ev), 'run_four': (four.run, ev), 'table': (table.run, ev), 'clone_quant': (clone_quant, ev)},
                  args.reps, args.warmup, restore)
    restore()
    gb = args.batch * one.elements * 8 / 1e9
    res['run'] = {k: _stat(v) for k, v in t.items()}
    for k in ('run_one', 'run_four'):
        res['run'][k]['GB'] = gb
        res['run'][k]['TBps'] = gb / res['run'][k]['median_us'] * 1e-3 * 1e6
    res['run']['table']['GB'] = gb / 2
    res['run']['table']['TBps'] = gb / 2 / res['run']['table']['median_us'] * 1e-3 * 1e6
    res['litmus_read'] = litmus_read()
    res['clone_quant_over_run_one'] = res['run']['clone_quant']['median_us'] / res['run']['run_one']['median_us']
    res['four_over_one'] = res['run']['run_four']['median_us'] / res['run']['run_one']['median_us']

    # (c) the loop of single-tensor calls
    def loop():
        return [[(float(dfq._quantize_error(g[k].weight, 8, 'sum')), float(dfq._quantize_error(g[k].weight, 8, 'mean'))) for k in keys]
                for (g, _, _) in nets]
    t = alternate({'loop': (loop, wall), 'quantize_error': (lambda: batch.quantize_error(8, False, False), wall)}, args.loop_reps, 1)
    res['loop'] = {k: _stat(v) for k, v in t.items()}
    res['loop']['calls'] = 2 * args.batch * one.n_tensors
    res['loop_over_quantize_error'] = res['loop']['loop']['median_us'] / res['loop']['quantize_error']['median_us']
    for p in (one, four, table, quant):
        p.close()
    _ffi.synchronize()
    res['device'] = torch.cuda.get_device_name(0)
    emit(res, args.out)


if __name__ == '__main__':
    main()
