#!/usr/bin/env python3
"""Batch activation ranges (NetworkBatch.act_range_plan) against the loop of per-network set_quant_minmax calls, on the GPU,
for batches of 1, 8 and 64 equalised and bias-corrected MobileNetV2 (synthetic.build('mobilenet_v2', seed=s % 4), QConv2d /
QLinear layers so that the loop does its full work) resident on the device:

  * A, the baseline: `set_quant_minmax(graph_n, bottoms_n, verbose=False)` over the batch's networks.  Wall clock (the function
    synchronises by itself, once per quantiser behind an add); its library launches and read-backs per network are counted
    on the host (every dfq_* entry point it calls is one launch, every `.tolist()` one blocking read-back);
  * B: `plan.run()` alone between device events, and `batch.set_quant_minmax()` by the wall clock, inclusive of plan creation,
    the synchronisation and the binding of the quantisers -- the number for a caller who does this once;
  * next to them one trivial launch (a one-element `add_`) between the same device events: the floor for work of this size.

Warm-up, alternating A/B, median of --reps with the spread.  This is latency-bound work on channel vectors: no bandwidth is
reported.

    python tools/batch_act_bench.py [--reps 15] [--warmup 3] [--batches 1,8,64] [--out profiles/batch_act_bench.json]

Kernel durations and the loop's launch count as the device saw them come from a separate
`rocprofv3 --kernel-trace --stats -- python tools/batch_act_bench.py --reps 3 --batches 8`.
"""
import argparse
import contextlib
import io
import os
import statistics
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dfq_amd import _ffi, arena                                        # noqa: E402
from dfq_amd.utils import layer_transform as lt                          # noqa: E402
from batch_bench_common import alternate as _alternate, emit, events as _events, nets as _nets, wall as _wall   # noqa: E402
from dfq_amd.utils.quantize import QConv2d, QLinear                      # noqa: E402

QTARG = [QConv2d, QLinear]
ENTRY_POINTS = ('dfq_bn_ranges', 'dfq_relu_moments', 'dfq_moments_after_add', 'dfq_moment_range', 'dfq_bn_through_layer')


def _q_graph(graph, dev):
    out = type(graph)()
    for k, m in graph.items():
        if type(m) == torch.nn.Conv2d:
            q = QConv2d(m.in_channels, m.out_channels, m.kernel_size, m.stride, m.padding, m.dilation, m.groups, m.bias is not None)
        elif type(m) == torch.nn.Linear:
            q = QLinear(m.in_features, m.out_features, m.bias is not None)
        else:
            out[k] = m
            continue
        q.weight.data.copy_(m.weight.data)
        if m.bias is not None:
            q.bias.data.copy_(m.bias.data)
        out[k] = q.to(dev)
    return out


def _count_loop(graph, bottoms):
    """library launches and blocking read-backs of ONE set_quant_minmax call, counted on the host"""
    lib = _ffi.lib()
    counts = {k: 0 for k in ENTRY_POINTS}
    kept = {k: getattr(lib, k) for k in ENTRY_POINTS}
    reads = [0]
    tolist = torch.Tensor.tolist

    def counting(name):
        def call(*a):
            counts[name] += 1
            return kept[name](*a)
        return call

    def counted_tolist(self):
        reads[0] += 1
        return tolist(self)
    try:
        for k in ENTRY_POINTS:
            setattr(lib, k, counting(k))
        torch.Tensor.tolist = counted_tolist
        lt.set_quant_minmax(graph, bottoms, verbose=False)
    finally:
        for k in ENTRY_POINTS:
            setattr(lib, k, kept[k])
        torch.Tensor.tolist = tolist
    quantisers = sum(1 for k, m in graph.items() if hasattr(m, 'quant') and bottoms[k] is not None)
    return {'library_launches': counts, 'library_launches_total': sum(counts.values()), 'blocking_readbacks': reads[0],
            'quantisers': quantisers, 'fill_launches': 2 * quantisers}


def _stat(samples):
    return {'median_us': statistics.median(samples), 'spread_us': [min(samples), max(samples)]}


def bench(n, dev, reps, warmup):
    nets = _nets(n, dev, QTARG, _q_graph)
    batch = arena.NetworkBatch(nets, QTARG)
    le = batch.le_plan()
    le.run()
    le.close()
    bc = batch.bc_plan()
    bc.run(check=True)
    bc.close()
    torch.cuda.synchronize()
    plan = batch.act_range_plan()
    one = torch.zeros(1, device=dev)

    def loop():
        for (g, b, _) in nets:
            lt.set_quant_minmax(g, b, verbose=False)
    res = {'networks': n, 'results_per_network': plan.n_results, 'steps_per_network': plan.n_steps, 'launches': plan.launches}
    with contextlib.redirect_stdout(io.StringIO()):
        res['loop_per_network'] = _count_loop(nets[0][0], nets[0][1])
        t = _alternate({'loop': (loop, _wall), 'plan_run': (plan.run, _events), 'plan_run_wall': (plan.run, _wall),
                        'batch_set_quant_minmax': (batch.set_quant_minmax, _wall), 'trivial_launch': (lambda: one.add_(1.0), _events)},
                       reps, warmup)
    for k, v in t.items():
        res[k] = _stat(v)
    res['loop_over_plan_run_wall'] = res['loop']['median_us'] / res['plan_run_wall']['median_us']
    res['loop_over_batch_set_quant_minmax'] = res['loop']['median_us'] / res['batch_set_quant_minmax']['median_us']
    # faster by more than the run-to-run spread of the two medians: the slowest B sample against the fastest A sample
    res['plan_run_beats_loop_beyond_spread'] = res['plan_run_wall']['spread_us'][1] < res['loop']['spread_us'][0]
    res['inclusive_beats_loop_beyond_spread'] = res['batch_set_quant_minmax']['spread_us'][1] < res['loop']['spread_us'][0]
    # the two paths agree (the loop ran last on these quantisers or the plan did: compare a fresh pair)
    plan.run()
    torch.cuda.synchronize()
    got = plan.block.clone()
    with contextlib.redirect_stdout(io.StringIO()):
        loop()
    keys = plan.keys
    want = torch.stack([torch.stack([torch.cat([g[k].quant.running_min.reshape(1), g[k].quant.running_max.reshape(1)]) for k in keys])
                        for (g, _, _) in nets])
    res['bit_identical_to_loop'] = bool(torch.equal(got.view(torch.int32), want.view(torch.int32)))
    plan.close()
    batch.release()
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--batches', default='1,8,64')
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    dev = torch.device('cuda', 0)
    res = {'tool': 'tools/batch_act_bench.py', 'reps': args.reps, 'warmup': args.warmup, 'device': torch.cuda.get_device_name(0),
           'batches': [bench(int(n), dev, args.reps, args.warmup) for n in args.batches.split(',')]}
    try:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        res['commit'] = subprocess.run(['git', '-C', root, 'rev-parse', '--short', 'HEAD'], capture_output=True, text=True).stdout.strip() or None
    except OSError:
        res['commit'] = None
    emit(res, args.out)


if __name__ == '__main__':
    main()
