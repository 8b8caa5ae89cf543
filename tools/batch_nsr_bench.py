#!/usr/bin/env python3
"""Data-free layer sensitivities of a batch (NetworkBatch.nsr_plan) on the GPU (warm-up, alternating legs between device
events, median and min-max of --reps), for a batch of --batch equalised MobileNetV2 (synthetic.build('mobilenet_v2',
seed=s % 4), BatchNorm folded, le_plan run once), widths (2, 3, 4, 6, 8), per tensor and per channel.  Nothing writes a
weight, so nothing is restored between the repetitions.

  * BatchNsrPlan.run(): the input moments, per tensor the ranges, the rows (S and the five numerators of every output row),
    the fold;
  * its yardstick, BatchMixedPlan.run() with ``apply=False`` on the same widths: the same bytes read and the same five
    quantisers per weight, one float64 sum per tensor and width where the nsr plan keeps six per row and weighs every term;
  * the read rate tools/litmus/hbm_stream reports in the same job, if that program has been built, next to the rate the
    nsr plan's traffic (4 B per weight with per-channel ranges, 8 B per tensor) implies;
  * the allocation at --avg-bits under ``cost='nsr'`` (mixed_plan(costs=nsr plan)) and under ``cost='mse'``: the distribution
    of the chosen widths over all layers and networks, and the share of (network, layer) pairs whose width differs.

The BatchNorm statistics of the synthetic networks match no data and the weights are not trained: the histograms show that
the two costs allocate differently, not that either allocation is more accurate.

    python tools/batch_nsr_bench.py [--reps 25] [--warmup 3] [--batch 64] [--avg-bits 4] [--out profiles/batch_nsr_bench.json]
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

    res = {'networks': args.batch, 'widths': list(WIDTHS), 'avg_bits': args.avg_bits, 'configs': {}}
    for per_channel in (False, True):
        nsr = batch.nsr_plan(WIDTHS, per_channel=per_channel)
        mse = batch.mixed_plan(WIDTHS, avg_bits=args.avg_bits, per_channel=per_channel, apply=False)
        on_nsr = batch.mixed_plan(WIDTHS, avg_bits=args.avg_bits, per_channel=per_channel, apply=False, costs=nsr)
        t = alternate({'nsr_plan': (nsr.run, events), 'mixed_plan_no_apply': (mse.run, events)}, args.reps, args.warmup)
        r = {k: _stat(v) for k, v in t.items()}
        r['nsr_over_mixed_no_apply'] = r['nsr_plan']['median_us'] / r['mixed_plan_no_apply']['median_us']
        weights = mse.elements
        r['weights_per_s'] = args.batch * weights / r['nsr_plan']['median_us'] * 1e6
        r['implied_TBps'] = args.batch * weights * (4.0 if per_channel else 8.0) / r['nsr_plan']['median_us'] * 1e-6
        r['launches'] = {'nsr_plan': nsr.launches, 'mixed_plan_no_apply': mse.launches}
        nsr.run()
        mse.run()
        on_nsr.run()
        _ffi.synchronize()
        b_mse, b_nsr = mse.bits_block.cpu(), on_nsr.bits_block.cpu()
        r['width_share'] = {'mse': {str(b): float((b_mse == b).double().mean()) for b in WIDTHS},
                            'nsr': {str(b): float((b_nsr == b).double().mean()) for b in WIDTHS}}
        r['layers_with_another_width'] = float((b_mse != b_nsr).double().mean())
        used = on_nsr.used_block.cpu()
        r['used_over_budget_nsr'] = {'min': float(used[:, 0].min()) / on_nsr.budget, 'max': float(used[:, 0].max()) / on_nsr.budget}
        r['finite_costs'] = bool(torch.isfinite(nsr.cost_block).all())
        res['configs']['row' if per_channel else 'tensor'] = r
        res['weights_per_network'] = weights
        res['budget_bits'] = mse.budget
        for p in (nsr, mse, on_nsr):
            p.close()
    _ffi.synchronize()
    res['hbm_stream'] = litmus_read() or 'not measured yet'
    res['device'] = torch.cuda.get_device_name(0)
    emit(res, args.out)


if __name__ == '__main__':
    main()
