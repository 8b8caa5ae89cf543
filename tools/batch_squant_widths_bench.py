#!/usr/bin/env python3
"""Adaptive rounding at each layer's own width (NetworkBatch.squant_plan(widths=)) on the GPU: ``plan.run()`` between device events
after a warm-up, the legs alternating in one job, median and min-max of --reps, for a batch of --batch equalised MobileNetV2
(synthetic.build('mobilenet_v2', seed=s % 4), BatchNorm folded, le_plan run once), per tensor and per channel, 1-byte codes.  The
weights are restored in front of every repetition, outside the measurement.

  widths    squant_plan(widths=mixed).run(), the widths read on the device from mixed_plan((2, 3, 4, 6, 8), avg_bits=4, apply=False)
  uniform   squant_plan(4).run(): the same reads, writes and number of launches at one width

``widths_over_uniform`` is their ratio; nothing is asserted about it.  tools/litmus/hbm_stream's read rate is reported from the
same job if that program has been built.

Regression check of the uniform path: with ``--parent-lib`` (a libdfq_hip.so built from the parent commit, e.g. by ``make
BUILD=build_parent OUT=../../variants/libdfq_hip_parent.so`` in a checkout of it) the uniform leg is also measured with that
library AND with this one under the same conditions -- child processes that run that leg only -- alternating, --rounds of each.
The noise is the spread of the parent's own round medians; ``uniform_within_noise`` says whether this library's child medians
lie within the parent's range widened by that spread on either side, ``uniform_not_slower`` whether they lie below its upper end.
Without the library the parent is "not measured yet".

    python tools/batch_squant_widths_bench.py [--reps 25] [--warmup 3] [--batch 64] [--rounds 3] [--parent-lib PATH]
                                              [--out profiles/batch_squant_widths_bench.json]
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
CONFIGS = [('tensor', False), ('row', True)]


def _stat(samples):
    return {'median_us': statistics.median(samples), 'spread_us': [min(samples), max(samples)], 'reps': len(samples)}


def measure(args, with_widths):
    """{config: {leg: stat, ...}}"""
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

    out = {}
    for name, per_channel in CONFIGS:
        uniform = batch.squant_plan(4, per_channel=per_channel, codes='int8')
        legs = {'uniform': (uniform.run, ev)}
        r = {}
        if with_widths:
            mixed = batch.mixed_plan(WIDTHS, avg_bits=4, per_channel=per_channel, apply=False)
            mixed.run()
            _ffi.synchronize()
            bits = mixed.bits_block.cpu()
            r['width_share'] = {str(b): float((bits == b).double().mean()) for b in WIDTHS}
            widths = batch.squant_plan(per_channel=per_channel, codes='int8', widths=mixed)
            legs['widths'] = (widths.run, ev)
        t = alternate(legs, args.reps, args.warmup, restore)
        r.update({k: _stat(v) for k, v in t.items()})
        if with_widths:
            r['widths_over_uniform'] = r['widths']['median_us'] / r['uniform']['median_us']
            r['launches'] = {'widths': widths.launches, 'uniform': uniform.launches}
            r['status_all_zero'] = widths.status_block.cpu().tolist().count(0) == args.batch
            weights = sum(numel for (_, _, numel, _) in widths._code_views)
            r['weights_per_network'] = weights
            r['flip_share'] = float(widths.stats_block.view(args.batch, -1, 2)[:, :, 1].sum().item()) / (args.batch * weights)
            widths.close()
            mixed.close()
        uniform.close()
        out[name] = r
    restore()
    _ffi.synchronize()
    return out


def child_round(args, lib):
    """the uniform leg with the library `lib`, in a process of its own"""
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
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--parent-lib', default=None)
    ap.add_argument('--child', action='store_true', help='(internal) the uniform leg only, with whatever library DFQ_HIP_LIB names')
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    if args.child:
        from dfq_amd import _ffi
        _ffi.SIGNATURES.pop('dfq_batch_squant_plan_set_widths', None)      # (the parent's library has no such symbol)
        print(json.dumps(measure(args, False)))
        return
    from dfq_amd import _ffi
    from batch_bench_common import emit
    from batch_table_bench import litmus_read
    res = {'networks': args.batch, 'widths': list(WIDTHS), 'avg_bits': 4, 'rounds': []}
    have_parent = bool(args.parent_lib and os.path.exists(args.parent_lib))
    for _ in range(args.rounds):
        rnd = {}
        if have_parent:
            rnd['parent'] = child_round(args, args.parent_lib)
            rnd['this_uniform_only'] = child_round(args, _ffi.LIB_PATH)
        rnd['this'] = measure(args, True)
        res['rounds'].append(rnd)
    res['configs'] = {}
    for name, _ in CONFIGS:
        c = dict(res['rounds'][-1]['this'][name])
        for leg in ('widths', 'uniform'):
            c[leg] = {'median_us': statistics.median(r['this'][name][leg]['median_us'] for r in res['rounds']),
                      'round_medians_us': [r['this'][name][leg]['median_us'] for r in res['rounds']],
                      'spread_us': [min(r['this'][name][leg]['spread_us'][0] for r in res['rounds']),
                                    max(r['this'][name][leg]['spread_us'][1] for r in res['rounds'])]}
        c['widths_over_uniform'] = c['widths']['median_us'] / c['uniform']['median_us']
        if have_parent:
            rounds = [r['parent'][name]['uniform']['median_us'] for r in res['rounds']]
            noise = max(rounds) - min(rounds)
            own = [r['this_uniform_only'][name]['uniform']['median_us'] for r in res['rounds']]
            c['parent_uniform'] = {'median_us': statistics.median(rounds), 'round_medians_us': rounds, 'noise_us': noise}
            c['this_uniform_only'] = {'median_us': statistics.median(own), 'round_medians_us': own}
            c['uniform_within_noise'] = bool(min(rounds) - noise <= statistics.median(own) <= max(rounds) + noise)
            c['uniform_not_slower'] = bool(statistics.median(own) <= max(rounds) + noise)
        else:
            c['parent_uniform'] = 'not measured yet'
        res['configs'][name] = c
    res['hbm_stream'] = litmus_read() or 'not measured yet'
    res['device'] = torch.cuda.get_device_name(0)
    emit(res, args.out)


if __name__ == '__main__':
    main()
