#!/usr/bin/env python3
"""Adaptive rounding of a batch (NetworkBatch.squant_plan) on the GPU (warm-up, alternating legs between device events,
median and min-max of --reps), for a batch of --batch equalised MobileNetV2 (synthetic.build('mobilenet_v2', seed=s % 4),
BatchNorm folded, le_plan run once), at 4 and 8 bits, per tensor and per channel, with 1-byte codes:

  * BatchSquantPlan.run() alternating with BatchQuantPlan.run() of the same configuration (weights only: bits_bias=32), the
    weights restored in front of every repetition, outside the measurement.  Both read every weight once and write it and its
    code once, so their ratio is what the selection costs;
  * the share of the codes that differ from nearest rounding (from the plan's stats).

    python tools/batch_squant_bench.py [--reps 25] [--warmup 3] [--batch 64] [--out profiles/batch_squant_bench.json]
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

TARG = [nn.Conv2d, nn.Linear]
CONFIGS = [(4, False), (4, True), (8, False), (8, True)]               # (bit_weight, per_channel)


def _stat(samples):
    return {'median_us': statistics.median(samples), 'spread_us': [min(samples), max(samples)], 'reps': len(samples)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=25)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--batch', type=int, default=64)
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

    res = {'networks': args.batch, 'configs': {}}
    for bits, per_channel in CONFIGS:
        squant = batch.squant_plan(bits, per_channel=per_channel, codes='int8')
        nearest = batch.quant_plan(bits, 32, per_channel=per_channel, codes='int8')
        t = alternate({'squant_plan': (squant.run, ev), 'quant_plan': (nearest.run, ev)}, args.reps, args.warmup, restore)
        restore()
        squant.run()
        _ffi.synchronize()
        weights = sum(numel for (_, _, numel, _) in squant._code_views)
        stats = squant.stats_block.view(args.batch, -1, 2)
        r = {k: _stat(v) for k, v in t.items()}
        r['squant_over_quant'] = r['squant_plan']['median_us'] / r['quant_plan']['median_us']
        r['weights_per_s'] = args.batch * weights / r['squant_plan']['median_us'] * 1e6
        r['flip_share'] = float(stats[:, :, 1].sum().item()) / (args.batch * weights)
        r['largest_row_sum_quanta'] = float(stats[:, :, 0].abs().max().item()) / float(1 << 30)
        r['launches'] = {'squant_plan': squant.launches, 'quant_plan': nearest.launches}
        res['configs']['{}b_{}'.format(bits, 'row' if per_channel else 'tensor')] = r
        res['weights_per_network'] = weights
        squant.close()
        nearest.close()
    restore()
    _ffi.synchronize()
    res['device'] = torch.cuda.get_device_name(0)
    emit(res, args.out)


if __name__ == '__main__':
    main()
