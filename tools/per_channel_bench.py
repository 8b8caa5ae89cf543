#!/usr/bin/env python3
"""Per-channel against per-tensor weight mode, on the GPU (device events, warm-up, alternating A/B, median of --reps):

  * bias correction of one MobileNetV2 and of a batch of --batch MobileNetV2s (one plan each; BCPlan.run with and without
    per_channel) -- the per-channel run adds the row-range launch in front of the chain;
  * quantize_targ_layer of one MobileNetV2, per tensor (two launches) and per channel (one launch), the whole call.

    python tools/per_channel_bench.py [--reps 25] [--warmup 5] [--batch 64] [--out profiles/per_channel_bench.json]

Kernel durations come from a separate `rocprofv3 --kernel-trace --stats -- python tools/per_channel_bench.py --reps 5`.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dfq_amd import dfq, synthetic                                    # noqa: E402
from dfq_amd.utils import layer_transform as lt                        # noqa: E402

TARG = [torch.nn.Conv2d, torch.nn.Linear]


def _nets(n, dev):
    out = []
    for s in range(n):
        model, graph, bottoms = synthetic.build('mobilenet_v2', seed=s % 4)
        model.to(dev)
        lt.merge_batchnorm(model, graph, bottoms, TARG)
        for k in graph:
            if type(graph[k]) in TARG:
                dfq._ensure_bias(graph[k])
        out.append((model, graph, bottoms))
    return out


def _time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3                     # us


def ab(fa, fb, reps, warmup):
    for _ in range(warmup):
        fa()
        fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for i in range(reps):
        if i % 2 == 0:
            ta.append(_time(fa))
            tb.append(_time(fb))
        else:
            tb.append(_time(fb))
            ta.append(_time(fa))
    ma, mb = statistics.median(ta), statistics.median(tb)
    return {'per_tensor_us': ma, 'per_channel_us': mb, 'ratio': mb / ma,
            'per_tensor_spread_us': [min(ta), max(ta)], 'per_channel_spread_us': [min(tb), max(tb)], 'reps': reps}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=25)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    dev = torch.device('cuda', 0)
    res = {}

    (_, g1, b1), = _nets(1, dev)
    plan, _ = dfq.build_bc_plan(g1, b1, TARG)
    res['bc_single'] = ab(lambda: plan.run(), lambda: plan.run(per_channel=True, bits=8), args.reps, args.warmup)
    res['bc_single']['one_launch'] = plan.one_launch
    plan.close()

    nets = _nets(args.batch, dev)
    plan = dfq.build_bc_plan_batch([(g, b) for (_, g, b) in nets], TARG)
    res['bc_batch'] = ab(lambda: plan.run(), lambda: plan.run(per_channel=True, bits=8), args.reps, args.warmup)
    res['bc_batch']['one_launch'] = plan.one_launch
    res['bc_batch']['networks'] = args.batch
    plan.close()
    del nets

    import contextlib
    import io
    quiet = contextlib.redirect_stdout(io.StringIO())
    with quiet:
        res['quantize_targ_layer'] = ab(lambda: lt.quantize_targ_layer(g1, 8, 16, TARG),
                                        lambda: lt.quantize_targ_layer(g1, 8, 16, TARG, per_channel=True), args.reps, args.warmup)
    res['device'] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or '.', exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
