#!/usr/bin/env python3
"""Mixed-precision quantisation of a batch (NetworkBatch.mixed_plan) on the GPU (warm-up, alternating legs between device
events, median and min-max of --reps), for a batch of --batch equalised MobileNetV2 (synthetic.build('mobilenet_v2',
seed=s % 4), BatchNorm folded, le_plan run once), widths (2, 3, 4, 6, 8), avg_bits = 4, per tensor and per channel, 1-byte
codes.  The weights are restored in front of every repetition, outside the measurement.

  * BatchMixedPlan.run(): ranges, the errors at the five widths, the allocation per network, the quantisation;
  * its yardstick, the nearest thing the library offered before without leaving the device: two BatchErrorPlan.run()
    (four widths + one) and one BatchQuantPlan.run() at 4 bits (weights only: bits_bias=32) -- five reads of every weight
    where the mixed plan reads it two or three times, the same five quantisers per weight, and no allocation at all;
  * the mixed plan without ``apply`` (ranges, errors, allocation), to see what the quantisation adds;
  * the read rate tools/litmus/hbm_stream reports in the same job, if that program has been built, next to the rate the
    mixed plan's traffic (two reads and a write of 4 B, a 1 B code) implies;
  * the distribution of the chosen widths over all layers and networks, used / budget, and the sum over the layers of the sum
    of squared errors against uniform 4-bit quantisation, which has the same size (from the plan's own error block).

    python tools/batch_mixed_bench.py [--reps 25] [--warmup 3] [--batch 64] [--avg-bits 4] [--out profiles/batch_mixed_bench.json]
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dfq_amd import _ffi, arena                                        # noqa: E402
from batch_bench_common import alternate, emit, events, nets as _nets   # noqa: E402
from batch_table_bench import litmus_read                               # noqa: E402

TARG = [nn.Conv2d, nn.Linear]
WIDTHS = (2, 3, 4, 6, 8)


def _stat(samples):
    return {'median_us': statistics.median(samples), 'spread_us': [min(samples), max(samples)], 'reps': len(samples)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=25)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--avg-bits', type=float, default=4.0)
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    dev = torch.device('cuda', 0)
    nets = _nets(args.batch, dev, TARG)
    batch = arena.NetworkBatch(nets, TARG)
    le = batch.le_plan()
    le.run()
    le.close()
    torch.cuda.synchronize()
    pristine = batch.storage.clone()

    def restore():
        batch.storage.copy_(pristine)

    def ev(fn):
        return events(fn, restore)

    res = {'networks': args.batch, 'widths': list(WIDTHS), 'avg_bits': args.avg_bits, 'configs': {}}
    for per_channel in (False, True):
        mixed = batch.mixed_plan(WIDTHS, avg_bits=args.avg_bits, per_channel=per_channel, codes='int8')
        alloc = batch.mixed_plan(WIDTHS, avg_bits=args.avg_bits, per_channel=per_channel, apply=False)
        err4 = batch.error_plan([(b, per_channel, False) for b in WIDTHS[:4]])
        err1 = batch.error_plan([(b, per_channel, False) for b in WIDTHS[4:]])
        quant = batch.quant_plan(4, 32, per_channel=per_channel, codes='int8')

        def yardstick():
            err4.run()
            err1.run()
            quant.run()

        t = alternate({'mixed_plan': (mixed.run, ev), 'yardstick': (yardstick, ev), 'mixed_plan_no_apply': (alloc.run, ev)},
                      args.reps, args.warmup, restore)
        restore()
        mixed.run()
        _ffi.synchronize()
        r = {k: _stat(v) for k, v in t.items()}
        r['mixed_over_yardstick'] = r['mixed_plan']['median_us'] / r['yardstick']['median_us']
        weights = mixed.elements
        r['weights_per_s'] = args.batch * weights / r['mixed_plan']['median_us'] * 1e6
        r['implied_TBps'] = args.batch * weights * 13.0 / r['mixed_plan']['median_us'] * 1e-6        # 2 reads + 1 write of 4 B, 1 B code
        r['launches'] = {'mixed_plan': mixed.launches, 'mixed_plan_no_apply': alloc.launches,
                         'yardstick': err4.launches + err1.launches + quant.launches}
        bits = mixed.bits_block.cpu()
        r['width_share'] = {str(b): float((bits == b).double().mean()) for b in WIDTHS}
        used = mixed.used_block.cpu()
        r['used_over_budget'] = {'min': float(used[:, 0].min()) / mixed.budget, 'max': float(used[:, 0].max()) / mixed.budget}
        r['steps'] = {'min': int(used[:, 1].min()), 'max': int(used[:, 1].max())}
        errors = mixed.error_block.cpu()                                           # [n_nets, T, B]
        chosen = torch.zeros_like(bits, dtype=torch.int64)
        for j, b in enumerate(WIDTHS):
            chosen[bits == b] = j
        e_mixed = errors.gather(2, chosen.unsqueeze(2)).squeeze(2).sum(dim=1)
        e_uniform = errors[:, :, WIDTHS.index(4)].sum(dim=1)
        ratio = e_mixed / e_uniform
        r['sum_sq_error_over_uniform_4bit'] = {'median': float(ratio.median()), 'min': float(ratio.min()), 'max': float(ratio.max())}
        res['configs']['row' if per_channel else 'tensor'] = r
        res['weights_per_network'] = weights
        res['budget_bits'] = mixed.budget
        for p in (mixed, alloc, err4, err1, quant):
            p.close()
    restore()
    _ffi.synchronize()
    res['hbm_stream'] = litmus_read() or 'not measured yet'
    res['device'] = torch.cuda.get_device_name(0)
    emit(res, args.out)


if __name__ == '__main__':
    main()
