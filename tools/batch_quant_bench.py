#!/usr/bin/env python3
"""Batch weight quantisation (NetworkBatch.quant_plan) against the loop of per-network quantize_targ_layer calls, on the GPU
(device events, warm-up, alternating A/B, median of --reps), for a batch of --batch MobileNetV2
(synthetic.build('mobilenet_v2', seed=s % 4)):

  * (a) the loop of quantize_targ_layer calls over the batch's networks, per tensor and per channel, against
    BatchQuantPlan.run() with int8 codes in the same mode;
  * (b) BatchQuantPlan.run() with int32 against int8 codes, in both modes; achieved TB/s counting 13 B per weight per tensor
    (min/max read, read, write, code) and 9 B per channel (read, write, code), plus 3 B more per weight for int32 codes;
  * (c) plan creation on its own (host wall clock: creation synchronises), and plan destruction.

    python tools/batch_quant_bench.py [--reps 25] [--warmup 5] [--batch 64] [--out profiles/batch_quant_bench.json]

Kernel durations come from a separate `rocprofv3 --kernel-trace --stats -- python tools/batch_quant_bench.py --reps 5`.
"""
import argparse
import contextlib
import io
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dfq_amd import arena                                            # noqa: E402
from dfq_amd.utils import layer_transform as lt                        # noqa: E402
from batch_bench_common import ab, emit, nets as _nets               # noqa: E402

TARG = [torch.nn.Conv2d, torch.nn.Linear]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=25)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    dev = torch.device('cuda', 0)
    nets = _nets(args.batch, dev, TARG)
    batch = arena.NetworkBatch(nets, TARG)
    weights = sum(m.weight.numel() for m in nets[0][0].values() if type(m) in TARG)
    res = {'networks': args.batch, 'weights_per_network': weights}

    plans = {}
    for mode, pc in (('per_tensor', False), ('per_channel', True)):
        for codes in ('int32', 'int8'):
            plans[mode, codes] = batch.quant_plan(8, 16, per_channel=pc, codes=codes)
    res['launches'] = {mode: plans[mode, 'int8'].launches for mode in ('per_tensor', 'per_channel')}

    quiet = contextlib.redirect_stdout(io.StringIO())
    with quiet:
        for mode, pc in (('per_tensor', False), ('per_channel', True)):
            def loop(pc=pc):
                for (g, _, _) in nets:
                    lt.quantize_targ_layer(g, 8, 16, TARG, per_channel=pc)
            r = ab('loop', loop, 'batch_int8', plans[mode, 'int8'].run, args.reps, args.warmup)
            res['loop_vs_batch_' + mode] = r

    for mode, per_weight in (('per_tensor', 13), ('per_channel', 9)):
        r = ab('int32', plans[mode, 'int32'].run, 'int8', plans[mode, 'int8'].run, args.reps, args.warmup)
        for codes, extra in (('int32', 3), ('int8', 0)):
            gb = args.batch * weights * (per_weight + extra) / 1e9
            r[codes + '_GB'] = gb
            r[codes + '_TBps'] = gb / r[codes + '_us'] * 1e-3 * 1e6
        res['run_' + mode] = r

    make, close = [], []
    for i in range(args.reps):
        t0 = time.perf_counter()
        p = batch.quant_plan(8, 16, per_channel=bool(i % 2), codes='int8')
        t1 = time.perf_counter()
        p.close()
        t2 = time.perf_counter()
        make.append((t1 - t0) * 1e6)
        close.append((t2 - t1) * 1e6)
    res['plan_create_us'] = statistics.median(make)
    res['plan_create_spread_us'] = [min(make), max(make)]
    res['plan_destroy_us'] = statistics.median(close)
    for p in plans.values():
        p.close()
    res['device'] = torch.cuda.get_device_name(0)
    emit(res, args.out)


if __name__ == '__main__':
    main()
