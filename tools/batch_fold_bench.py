#!/usr/bin/env python3
"""Batch BatchNorm folding (NetworkBatch.from_unfolded + fold_plan) against the loop of per-network merge_batchnorm calls, on
the GPU (device events, warm-up, alternating A/B, median of --reps), for a batch of --batch MobileNetV2
(synthetic.build('mobilenet_v2', seed=s % 4)) resident on the device, BatchNorm not folded:

  * (a) the loop `lt.merge_batchnorm(None, g, b, targ)` over the networks against BatchFoldPlan.run();
  * (b) BatchFoldPlan.run() alone: achieved TB/s counting 8 B per folded weight (read once, written once), next to what
    tools/litmus/hbm_stream (a bare in-place scale of 1 GiB) reports in the same job, if that program has been built;
  * (c) from_unfolded + merge_batchnorm() inclusive, by the host's clock, against the loop + the plain constructor.

Every timed call starts from the unfolded state, restored in front of it outside the events: the batch allocation from a
snapshot, the loop's networks (twins with storages of their own: their BatchNorm tensors are in no batch allocation) from
clones of their tensors, with `eps` and the proxies as they were.

    python tools/batch_fold_bench.py [--reps 15] [--warmup 3] [--batch 64] [--inclusive-reps 3] [--out profiles/batch_fold_bench.json]

Kernel durations come from a separate `rocprofv3 --kernel-trace --stats -- python tools/batch_fold_bench.py --reps 3`.
"""
import argparse
import os
import re
import statistics
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dfq_amd import arena                                             # noqa: E402
from dfq_amd.utils import layer_transform as lt                      # noqa: E402
from batch_bench_common import ab, alternate, emit, wall, nets as _nets   # noqa: E402

TARG = [torch.nn.Conv2d, torch.nn.Linear]
BN_VECTORS = ('weight', 'bias', 'running_mean', 'running_var')


class Unfolded:
    """the unfolded state of a list of networks with storages of their own, and the way back to it"""

    def __init__(self, nets):
        self.nets = nets
        self.bns, self.tensors = [], []
        for (g, b, _) in nets:
            for lk, bk in lt._fold_pairs(g, b, TARG):
                lt._ensure_bias(g[lk])                                # merge_batchnorm would add the same zero bias
                self.bns.append((g[bk], g[bk].eps))
                self.tensors.append((g[lk], 'weight'))
                self.tensors.append((g[lk], 'bias'))
                self.tensors += [(g[bk], name) for name in BN_VECTORS]
        self.snap = [getattr(m, name).detach().clone() for m, name in self.tensors]

    def restore(self):
        with torch.no_grad():
            torch._foreach_copy_([getattr(m, name).detach() for m, name in self.tensors], self.snap)
        for bn, eps in self.bns:
            bn.eps = eps
            bn.__dict__['_buffers'].pop('fake_weight', None)
            bn.__dict__['_buffers'].pop('fake_bias', None)


def litmus():
    """what tools/litmus/hbm_stream reports for its largest grid, or None if the program is not there"""
    exe = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'litmus', 'hbm_stream')
    if not os.path.exists(exe):
        return None
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300).stdout
    best = None
    for line in out.splitlines():
        m = re.search(r'grid\s+(\d+).*scale in place ([\d.]+) / nt-store ([\d.]+) / nt-both ([\d.]+) TB/s', line)
        if m:
            row = {'grid': int(m.group(1)), 'scale_TBps': float(m.group(2)), 'scale_nt_store_TBps': float(m.group(3)),
                   'scale_nt_both_TBps': float(m.group(4))}
            if best is None or max(row['scale_TBps'], row['scale_nt_both_TBps']) > max(best['scale_TBps'], best['scale_nt_both_TBps']):
                best = row
    return best


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--inclusive-reps', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    dev = torch.device('cuda', 0)
    mine = Unfolded(_nets(args.batch, dev, TARG, fold=False))          # the batch's networks
    twins = Unfolded(_nets(args.batch, dev, TARG, fold=False))         # the loop's
    batch = arena.NetworkBatch.from_unfolded(mine.nets, TARG)
    torch.cuda.synchronize()
    snap = batch.storage.clone()
    plan = batch.fold_plan()

    def restore():
        batch.storage.copy_(snap)
        batch.folded = False
        twins.restore()

    def loop():
        for (g, b, _) in twins.nets:
            lt.merge_batchnorm(None, g, b, TARG)
    g0 = mine.nets[0][0]
    res = {'networks': args.batch, 'pairs': plan.n_pairs, 'launches': plan.launches, 'folded_weights_per_network': plan.elements,
           'weights_per_network': sum(m.weight.numel() for m in g0.values() if type(m) in TARG),
           'loop_launches': 3 * plan.n_pairs * args.batch}
    res['loop_vs_batch'] = ab('loop', loop, 'batch', plan.run, args.reps, args.warmup, restore)
    gb = args.batch * plan.elements * 8 / 1e9
    us = res['loop_vs_batch']['batch_us']
    res['run'] = {'batch_us': us, 'GB': gb, 'TBps': gb / us * 1e-3 * 1e6, 'litmus_in_place_scale': litmus()}
    plan.close()

    # (c) inclusive of everything the host does, the networks with storages of their own in front of both
    batch.storage.copy_(snap)
    batch.release()
    mine.restore()
    twins.restore()
    made = []

    def new_way():
        nb = arena.NetworkBatch.from_unfolded(mine.nets, TARG)
        nb.merge_batchnorm()
        made.append(nb)

    def old_way():
        for (g, b, _) in twins.nets:
            lt.merge_batchnorm(None, g, b, TARG)
        made.append(arena.NetworkBatch(twins.nets, TARG))

    def undo(which):
        def prep():
            while made:
                made.pop().release()
            which.restore()
        return prep

    def timer(prep):
        def t(fn):
            prep()
            return wall(fn)
        return t
    for _ in range(1):                                                 # warm-up of both ways
        undo(mine)(); new_way(); undo(twins)(); old_way()             # noqa: E702
    undo(mine)()
    undo(twins)()
    t = alternate({'from_unfolded_and_fold': (new_way, timer(undo(mine))), 'loop_and_constructor': (old_way, timer(undo(twins)))},
                  args.inclusive_reps, 0)
    a, b = statistics.median(t['from_unfolded_and_fold']), statistics.median(t['loop_and_constructor'])
    res['inclusive_host_clock'] = {'from_unfolded_and_fold_us': a, 'loop_and_constructor_us': b, 'ratio': b / a,
                                   'from_unfolded_and_fold_spread_us': [min(t['from_unfolded_and_fold']), max(t['from_unfolded_and_fold'])],
                                   'loop_and_constructor_spread_us': [min(t['loop_and_constructor']), max(t['loop_and_constructor'])],
                                   'reps': args.inclusive_reps}
    while made:
        made.pop().release()
    res['device'] = torch.cuda.get_device_name(0)
    emit(res, args.out)


if __name__ == '__main__':
    main()
