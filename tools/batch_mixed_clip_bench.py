#!/usr/bin/env python3
"""Clip-aware mixed precision of a batch (NetworkBatch.mixed_plan(clip=)) on the GPU: warm-up, alternating legs between device
events, median and min-max of --reps, for a batch of --batch equalised MobileNetV2 (synthetic.build('mobilenet_v2', seed=s % 4),
BatchNorm folded, le_plan run once), widths (2, 3, 4, 6, 8), --avg-bits per weight, K = --candidates, alpha_min = --alpha-min,
per tensor and per channel (signed).  The weights are put back from a copy in front of every timed run (outside the events):
the applying leg writes them.

  * ``clipped_no_apply``: the clipped plan with ``apply=False`` -- the search at every width, the allocation;
  * ``clipped_apply``: the clipped plan with ``apply=True`` -- the same and the clamp + quantisation at the chosen widths;
  * ``yardstick_A``: the five ``clip_plan(b_j, apply=False).run()`` searches plus one ``mixed_plan(apply=False).run()``: what a
    user would have to loop without the clipped plan (and it still cannot apply);
  * the read rate tools/litmus/hbm_stream reports in the same job, if that program has been built.

Quality, measured and not promised: sum e^2 (against the weights as they were) at the chosen allocation for the clipped plan,
for the unclipped ``mixed_plan`` at the same budget, and for uniform 4-bit ``clip_plan`` + ``quant_plan`` (the clip plan's
error at its k*); the histogram of the chosen widths and the share of (network, layer) pairs whose width differs from the
unclipped plan's.  The synthetic weights are not trained and there is no dataset: whether accuracy on a real network improves
cannot be measured here.

    python tools/batch_mixed_clip_bench.py [--reps 25] [--warmup 3] [--batch 64] [--avg-bits 4] [--candidates 32]
                                           [--alpha-min 0.5] [--out profiles/batch_mixed_clip_bench.json]
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
    ap.add_argument('--candidates', type=int, default=32)
    ap.add_argument('--alpha-min', type=float, default=0.5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    dev = torch.device('cuda', 0)
    nets = _nets(args.batch, dev, TARG)
    batch = arena.NetworkBatch(nets, TARG)
    le = batch.le_plan()
    le.run()
    le.close()
    torch.cuda.synchronize()
    saved = batch.storage.clone()

    def restore():
        batch.storage.copy_(saved)

    def timer(fn):
        return events(fn, restore)

    K, amin = args.candidates, args.alpha_min
    res = {'networks': args.batch, 'widths': list(WIDTHS), 'avg_bits': args.avg_bits, 'candidates': K, 'alpha_min': amin, 'configs': {}}
    for per_channel, signed in ((False, False), (True, True)):
        kw = dict(avg_bits=args.avg_bits, per_channel=per_channel, signed=signed)
        clipped = batch.mixed_plan(WIDTHS, apply=False, clip=K, alpha_min=amin, **kw)
        applying = batch.mixed_plan(WIDTHS, apply=True, clip=K, alpha_min=amin, **kw)
        plain = batch.mixed_plan(WIDTHS, apply=False, **kw)
        searches = [batch.clip_plan(b, per_channel, signed, candidates=K, alpha_min=amin, apply=False) for b in WIDTHS]
        uniform = batch.clip_plan(4, per_channel, signed, candidates=K, alpha_min=amin, apply=False, keep_errors=True)

        def yardstick():
            for p in searches:
                p.run()
            plain.run()

        t = alternate({'clipped_no_apply': (clipped.run, timer), 'clipped_apply': (applying.run, timer), 'yardstick_A': (yardstick, timer)},
                      args.reps, args.warmup, restore)
        r = {k: _stat(v) for k, v in t.items()}
        r['clipped_over_yardstick_A'] = r['clipped_no_apply']['median_us'] / r['yardstick_A']['median_us']
        weights = clipped.elements
        evals = args.batch * weights * len(WIDTHS) * K
        r['evaluations_per_s'] = evals / r['clipped_no_apply']['median_us'] * 1e6
        r['launches'] = {'clipped_no_apply': clipped.launches, 'clipped_apply': applying.launches,
                         'yardstick_A': sum(p.launches for p in searches) + plain.launches}
        restore()
        clipped.run()
        plain.run()
        uniform.run()
        _ffi.synchronize()
        b_clip, b_plain = clipped.bits_block.cpu(), plain.bits_block.cpu()

        def at_chosen(plan):
            idx = torch.zeros_like(plan.bits_block, dtype=torch.int64)
            for j, b in enumerate(WIDTHS):
                idx[plan.bits_block == b] = j
            return plan.error_block.gather(2, idx.unsqueeze(2)).squeeze(2).sum(dim=1).cpu()       # [n_nets]

        e_clip, e_plain = at_chosen(clipped), at_chosen(plain)
        e_uni = uniform.error_block.gather(2, uniform.chosen_block.long().unsqueeze(2)).squeeze(2).sum(dim=1).cpu()
        r['sum_e2'] = {'clipped_mixed': float(e_clip.mean()), 'unclipped_mixed': float(e_plain.mean()), 'uniform_4bit_clip': float(e_uni.mean()),
                       'mean_over': 'networks'}
        r['width_share'] = {'clipped': {str(b): float((b_clip == b).double().mean()) for b in WIDTHS},
                            'unclipped': {str(b): float((b_plain == b).double().mean()) for b in WIDTHS}}
        r['layers_with_another_width'] = float((b_clip != b_plain).double().mean())
        r['narrowed_share_at_chosen_width'] = float((clipped.range_block != plain.range_block).double().mean())
        used = clipped.used_block.cpu()
        r['used_over_budget'] = {'min': float(used[:, 0].min()) / clipped.budget, 'max': float(used[:, 0].max()) / clipped.budget}
        res['configs']['row_signed' if per_channel else 'tensor'] = r
        res['weights_per_network'] = weights
        res['budget_bits'] = clipped.budget
        for p in [clipped, applying, plain, uniform] + searches:
            p.close()
    _ffi.synchronize()
    res['hbm_stream'] = litmus_read() or 'not measured yet'
    res['device'] = torch.cuda.get_device_name(0)
    res['note'] = 'synthetic untrained weights, no dataset: sum e^2 and the allocations are measured, accuracy is not'
    emit(res, args.out)


if __name__ == '__main__':
    main()
