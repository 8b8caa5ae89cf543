#!/usr/bin/env python3
"""Batch bias absorption and weight clipping (NetworkBatch.absorb_plan) against the loop of per-network bias_absorption +
clip_weight calls, on the GPU (device events, warm-up, alternating A/B, median of --reps), for a batch of --batch equalised
MobileNetV2 (synthetic.build('mobilenet_v2', seed=s % 4)) resident on the device:

  * (a) the loop `bias_absorption(g, r, b, N); clip_weight(g, clip, targ)` over the batch's networks against
    BatchAbsorbPlan.run() doing both;
  * (b) BatchAbsorbPlan.run() absorbing only, clipping only, and both; achieved TB/s counting 4 B per second-layer weight of
    an absorbed relation, 4 B per other clipped weight, and 4 B per weight the clamp changed (the stores made; the kernel
    stores 16-byte pieces, so this is the floor of what it wrote).

Every timed call starts from the same state: the batch allocation is restored from a snapshot in front of it, outside the
events (a second absorption of the same network finds every shift at zero, a second clip nothing to store).

    python tools/batch_absorb_bench.py [--reps 15] [--warmup 3] [--batch 64] [--N 0.5] [--clip 0.3] [--out profiles/batch_absorb_bench.json]

Kernel durations come from a separate `rocprofv3 --kernel-trace --stats -- python tools/batch_absorb_bench.py --reps 3`.
"""
import argparse
import contextlib
import io
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dfq_amd import arena, dfq                                       # noqa: E402
from batch_bench_common import ab, emit, nets as _nets               # noqa: E402

TARG = [torch.nn.Conv2d, torch.nn.Linear]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--N', type=float, default=0.5)
    ap.add_argument('--clip', type=float, default=0.3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    dev = torch.device('cuda', 0)
    nets = _nets(args.batch, dev, TARG)
    batch = arena.NetworkBatch(nets, TARG)
    le = batch.le_plan()
    le.run()
    le.close()
    torch.cuda.synchronize()
    clip = [-args.clip, args.clip]
    snap = batch.storage.clone()

    def restore():
        batch.storage.copy_(snap)

    g0, b0, r0 = nets[0]
    weights = sum(m.weight.numel() for m in g0.values() if type(m) in TARG)
    changed = sum(int(((m.weight < clip[0]) | (m.weight > clip[1])).sum()) for (g, _, _) in nets for m in g.values() if type(m) in TARG)
    plans = {'absorb': batch.absorb_plan(args.N), 'clip': batch.absorb_plan(args.N, clip, absorb=False),
             'both': batch.absorb_plan(args.N, clip)}
    res = {'networks': args.batch, 'weights_per_network': weights, 'N': args.N, 'range_clip': clip,
           'absorbed_relations': plans['both'].n_relations, 'relations': len(r0),
           'absorbed_weights_per_network': plans['both'].absorbed_elements,
           'clip_only_weights_per_network': plans['both'].clip_only_elements, 'weights_changed_by_clip': changed,
           'launches': {k: p.launches for k, p in plans.items()}}

    def loop():
        for (g, b, r) in nets:
            dfq.bias_absorption(g, r, b, args.N)
            dfq.clip_weight(g, clip, TARG)
    with contextlib.redirect_stdout(io.StringIO()):                    # bias_absorption prints a line per call
        res['loop_vs_batch'] = ab('loop', loop, 'batch', plans['both'].run, args.reps, args.warmup, restore)
    r = ab('absorb', plans['absorb'].run, 'clip', plans['clip'].run, args.reps, args.warmup, restore)
    r['both_us'] = res['loop_vs_batch']['batch_us']
    r.pop('ratio')
    read = {'absorb': plans['absorb'].absorbed_elements, 'clip': weights, 'both': weights}
    for k in ('absorb', 'clip', 'both'):
        gb = (args.batch * read[k] + (changed if k != 'absorb' else 0)) * 4 / 1e9
        r[k + '_GB'] = gb
        r[k + '_TBps'] = gb / r[k + '_us'] * 1e-3 * 1e6
    res['run'] = r
    for p in plans.values():
        p.close()
    res['device'] = torch.cuda.get_device_name(0)
    emit(res, args.out)


if __name__ == '__main__':
    main()
