#!/usr/bin/env python3
"""MSE-optimal weight clipping of a batch (NetworkBatch.clip_plan) on the GPU (warm-up, alternating legs between device
events, median and min-max of --reps), for a batch of --batch equalised MobileNetV2 (synthetic.build('mobilenet_v2',
seed=s % 4), BatchNorm folded, le_plan run once), --candidates candidates down to --alpha-min, for the configurations
(8, per tensor), (4, per tensor) and (4, per channel, signed):

  * BatchClipPlan.run() without and with ``apply`` (the weights restored in front of every repetition, outside the
    measurement), and the weights x candidates per second it implies;
  * alternating with BatchErrorPlan.run() of the same single configuration: the same quantiser recipe ONCE per weight, so
    K of those are the yardstick for the arithmetic -- reported as the time of a search over K error runs, as the rate of
    quantiser evaluations of the search over that of the error plan, and as the search's rate over K times the error plan's;
  * an eager torch restatement of the search on the same allocation (per layer over all networks at once: K full passes,
    a dozen temporaries each; --eager-reps repetitions), and how many of its choices agree with the plan's (it forms the
    scale in torch's arithmetic, so a near-tie may fall the other way).

    python tools/batch_clip_bench.py [--reps 25] [--warmup 3] [--batch 64] [--candidates 32] [--alpha-min 0.5] [--eager-reps 3]
                                     [--out profiles/batch_clip_bench.json]
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
CONFIGS = [(8, False, False), (4, False, False), (4, True, True)]      # (bit_weight, per_channel, signed)


def _stat(samples):
    return {'median_us': statistics.median(samples), 'spread_us': [min(samples), max(samples)], 'reps': len(samples)}


def _name(config):
    return '{}b_{}{}'.format(config[0], 'row' if config[1] else 'tensor', '_signed' if config[2] else '')


def eager_search(store, views, config, alphas):
    """k* of every unit [n_nets, units] by plain torch operations on the batch allocation `store` [n_nets, stride]"""
    bits, per_channel, signed = config
    n_nets = store.shape[0]
    out = []
    for off, rows, row_len in views:
        w = store[:, off:off + rows * row_len].view(n_nets, rows if per_channel else 1, -1)
        mn, mx = w.amin(dim=2, keepdim=True).double(), w.amax(dim=2, keepdim=True).double()
        z = torch.minimum(mn.clamp_min(0.0), mx)
        best = ks = None
        for k, a in enumerate(alphas):
            lo, hi = (z + a * (mn - z)).float(), (z + a * (mx - z)).float()
            wc = torch.minimum(torch.maximum(w, lo), hi)               # the error is that of the clamped weight
            if signed:
                qmin, qmax = -float(1 << (bits - 1)), float((1 << (bits - 1)) - 1)
                scale = (torch.maximum(lo.abs(), hi.abs()).double() / qmax).clamp_min(1e-8).float()
                lo = torch.zeros_like(lo)
            else:
                qmin, qmax = 0.0, float(1 << bits) - 1.0
                scale = ((hi.double() - lo.double()) / qmax).clamp_min(1e-8).float()
            q = ((wc - lo) / scale).clamp_(qmin, qmax).round_()
            err = (q * scale + lo - w).double().square_().sum(dim=2)
            if best is None:
                best, ks = err, torch.zeros_like(err, dtype=torch.int32)
            else:
                better = err < best
                best = torch.where(better, err, best)
                ks = torch.where(better, torch.full_like(ks, k), ks)
        out.append(ks)
    return torch.cat(out, dim=1)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=25)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--candidates', type=int, default=32)
    ap.add_argument('--alpha-min', type=float, default=0.5)
    ap.add_argument('--eager-reps', type=int, default=3)
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
    store = batch.storage.view(args.batch, batch.stride)
    K = args.candidates
    alphas = [1.0 if K == 1 else 1.0 - k * (1.0 - args.alpha_min) / (K - 1) for k in range(K)]
    g0 = nets[0][0]
    base = batch.storage.data_ptr()
    views = [((m.weight.data_ptr() - base) // 4, int(m.weight.shape[0]), m.weight.numel() // int(m.weight.shape[0]))
             for m in g0.values() if type(m) in TARG]

    def restore():
        batch.storage.copy_(pristine)

    def ev(fn):
        return events(fn, restore)

    res = {'networks': args.batch, 'candidates': K, 'alpha_min': args.alpha_min, 'configs': {}}
    for config in CONFIGS:
        name = _name(config)
        search = batch.clip_plan(*config, candidates=K, alpha_min=args.alpha_min, apply=False)
        clamp = batch.clip_plan(*config, candidates=K, alpha_min=args.alpha_min, apply=True)
        error = batch.error_plan((config,))
        t = alternate({'search': (search.run, ev), 'search_apply': (clamp.run, ev), 'error_plan': (error.run, ev)}, args.reps, args.warmup, restore)
        restore()
        search.run()
        _ffi.synchronize()
        mine = search.chosen_block.clone()
        te = alternate({'eager': (lambda: eager_search(store, views, config, alphas), lambda fn: events(fn))}, args.eager_reps, 1)
        theirs = eager_search(store, views, config, alphas)
        r = {k: _stat(v) for k, v in t.items()}
        r['eager'] = _stat(te['eager'])
        evaluations = args.batch * search.elements * K
        t_err = r['error_plan']['median_us']
        for k in ('search', 'search_apply'):
            us = r[k]['median_us']
            r[k]['weights_x_candidates_per_s'] = evaluations / us * 1e6
            r[k]['time_over_K_error_runs'] = us / (K * t_err)
            r[k]['evaluation_rate_over_error_plan'] = K * t_err / us
            r[k]['rate_over_K_times_error_rate'] = t_err / us
        r['error_plan']['weights_per_s'] = args.batch * search.elements / t_err * 1e6
        r['eager_over_search'] = r['eager']['median_us'] / r['search']['median_us']
        r['launches'] = {'search': search.launches, 'search_apply': clamp.launches, 'error_plan': error.launches}
        r['units_per_network'] = int(mine.shape[1])
        r['ranges_narrowed'] = float((mine != 0).double().mean())
        r['eager_choices_agree'] = float((mine == theirs).double().mean())
        res['configs'][name] = r
        res['weights_per_network'] = search.elements
        for p in (search, clamp, error):
            p.close()
    _ffi.synchronize()
    res['device'] = torch.cuda.get_device_name(0)
    emit(res, args.out)


if __name__ == '__main__':
    main()
