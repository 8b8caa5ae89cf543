#!/usr/bin/env python3
"""Bias correction at each layer's own bit width (BCPlan.run(widths=)) on the GPU: ``plan.run()`` between device events after a
warm-up, the legs alternating in one job, median and min-max of --reps, for a batch of --batch equalised MobileNetV2
(synthetic.build('mobilenet_v2', seed=s % 4), BatchNorm folded, le_plan run once).  Biases and BN proxies are restored in front of
every repetition, outside the measurement.

  (a) run()                                    per tensor, 8 bits: the existing run
  (b) run(per_channel=True, bits=8)            the existing per-channel run
  (c) run(widths=8)                            the widths path per tensor, one width
  (d) run(per_channel=True, widths=mixed)      a width per (network, layer), read on the device from a mixed_plan(apply=False)
  (e) run(widths=mixed)                        the same per tensor

Yardsticks: (d) against (b) -- the same reads and the same number of launches; (c) and (e) against (a) plus one more read of the
weights (4 B per weight on top of the 8 B of the pass): the extra time is reported with the read rate it implies, next to the rate
tools/litmus/hbm_stream reports in the same job if that program has been built.

Regression check: with ``--parent-lib`` (a libdfq_hip.so built from the parent commit, e.g. by ``make BUILD=build_parent
OUT=../../variants/libdfq_hip_parent.so`` in a checkout of it) legs (a) and (b) are also measured with that library AND with this
one under the same conditions -- child processes that run these two legs only -- alternating with this process's rounds
(--rounds of each).  The noise is the spread of the parent's own round medians; ``a_within_noise`` / ``b_within_noise`` say
whether this library's child medians lie within the parent's range widened by that spread on either side.  (The five-leg
rounds of this process are not the comparison: what a leg costs depends on which legs ran in front of it.)  Without the
library the parent's legs are "not measured yet".

    python tools/bc_widths_bench.py [--reps 25] [--warmup 3] [--batch 64] [--rounds 3] [--parent-lib PATH] [--out profiles/bc_widths_bench.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TARG = [nn.Conv2d, nn.Linear]
WIDTHS = (2, 3, 4, 6, 8)


def _stat(samples):
    return {'median_us': statistics.median(samples), 'spread_us': [min(samples), max(samples)], 'reps': len(samples)}


def measure(args, legs):
    """one round: {leg: stat} (+ what describes the batch)"""
    from dfq_amd import _ffi, arena
    from batch_bench_common import alternate, events, nets as _nets
    dev = torch.device('cuda', 0)
    batch = arena.NetworkBatch(_nets(args.batch, dev, TARG), TARG)
    le = batch.le_plan()
    le.run()
    le.close()
    torch.cuda.synchronize()
    pristine = batch.storage.clone()

    def restore():
        batch.storage.copy_(pristine)

    def ev(fn):
        return events(fn, restore)

    plan = batch.bc_plan()
    info = {'one_launch': plan.one_launch, 'tagged': plan.tagged, 'weights_per_network': plan.weight_elements // args.batch}
    fns = {'a': lambda: plan.run(), 'b': lambda: plan.run(per_channel=True, bits=8)}
    mixed = {}
    if set(legs) - {'a', 'b'}:
        for per_channel in (False, True):
            m = batch.mixed_plan(WIDTHS, avg_bits=args.avg_bits, per_channel=per_channel, apply=False)
            m.run()
            mixed[per_channel] = m
        _ffi.synchronize()
        bits = mixed[True].bits_block.cpu()
        info['width_share_row'] = {str(b): float((bits == b).double().mean()) for b in WIDTHS}
        bits = mixed[False].bits_block.cpu()
        info['width_share_tensor'] = {str(b): float((bits == b).double().mean()) for b in WIDTHS}
        fns['c'] = lambda: plan.run(widths=8)
        fns['d'] = lambda: plan.run(per_channel=True, widths=mixed[True])
        fns['e'] = lambda: plan.run(widths=mixed[False])
    t = alternate({k: (fns[k], ev) for k in legs}, args.reps, args.warmup, restore)
    plan.status()
    for m in mixed.values():
        m.close()
    plan.close()
    return {k: _stat(v) for k, v in t.items()}, info


def child_round(args, lib):
    """legs (a) and (b) with the library `lib`, in a process of its own"""
    env = dict(os.environ, DFQ_HIP_LIB=os.path.abspath(lib))
    cmd = [sys.executable, os.path.abspath(__file__), '--child', '--reps', str(args.reps), '--warmup', str(args.warmup),
           '--batch', str(args.batch)]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, check=True).stdout
    return json.loads(out.strip().splitlines()[-1])


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=25)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--avg-bits', type=float, default=4.5)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--parent-lib', default=None)
    ap.add_argument('--child', action='store_true', help='(internal) legs a and b only, with whatever library DFQ_HIP_LIB names')
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    if args.child:
        from dfq_amd import _ffi
        _ffi.SIGNATURES.pop('dfq_bc_plan_run_widths', None)      # (the parent's library has no such symbol)
        stats, _ = measure(args, ['a', 'b'])
        print(json.dumps(stats))
        return
    from batch_bench_common import emit
    from batch_table_bench import litmus_read
    res = {'networks': args.batch, 'widths': list(WIDTHS), 'avg_bits': args.avg_bits, 'rounds': []}
    have_parent = bool(args.parent_lib and os.path.exists(args.parent_lib))
    for _ in range(args.rounds):
        rnd = {}
        if have_parent:
            from dfq_amd import _ffi
            rnd['parent'] = child_round(args, args.parent_lib)
            rnd['this_ab_only'] = child_round(args, _ffi.LIB_PATH)
        rnd['this'], info = measure(args, ['a', 'b', 'c', 'd', 'e'])
        res.update(info)
        res['rounds'].append(rnd)
    med = {k: statistics.median(r['this'][k]['median_us'] for r in res['rounds']) for k in 'abcde'}
    res['legs'] = {k: {'median_us': med[k], 'round_medians_us': [r['this'][k]['median_us'] for r in res['rounds']],
                       'spread_us': [min(r['this'][k]['spread_us'][0] for r in res['rounds']),
                                     max(r['this'][k]['spread_us'][1] for r in res['rounds'])]} for k in 'abcde'}
    res['d_over_b'] = med['d'] / med['b']
    res['c_over_a'] = med['c'] / med['a']
    res['e_over_a'] = med['e'] / med['a']
    extra_bytes = 4.0 * args.batch * res['weights_per_network']
    res['extra_read'] = {k: {'us': med[k] - med['a'], 'implied_TBps': extra_bytes / (med[k] - med['a']) * 1e-6 if med[k] > med['a'] else None}
                         for k in 'ce'}
    if have_parent:
        for k in 'ab':
            rounds = [r['parent'][k]['median_us'] for r in res['rounds']]
            noise = max(rounds) - min(rounds)
            res['parent_' + k] = {'median_us': statistics.median(rounds), 'round_medians_us': rounds, 'noise_us': noise}
            own = [r['this_ab_only'][k]['median_us'] for r in res['rounds']]
            res['this_' + k + '_ab_only'] = {'median_us': statistics.median(own), 'round_medians_us': own}
            res[k + '_within_noise'] = bool(min(rounds) - noise <= statistics.median(own) <= max(rounds) + noise)
    else:
        res['parent_a'] = res['parent_b'] = 'not measured yet'
    res['hbm_stream'] = litmus_read() or 'not measured yet'
    res['device'] = torch.cuda.get_device_name(0)
    emit(res, args.out)


if __name__ == '__main__':
    main()
