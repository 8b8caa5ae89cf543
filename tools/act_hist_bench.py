#!/usr/bin/env python3
"""Clipped activation ranges from histograms (improve_dfq.clip_quant_range, dfq_act_hist.hip) on the GPU:

  * the kernel: dfq_act_hist_accumulate (2048 bins over the tensor's own min / max) on [64, 96, 112, 112], [64, 320, 7, 7]
    and [64, 1000], each filled with randn and with relu(randn) -- half the elements in one bin -- between device events,
    alternating with dfq_tensor_minmax on the same tensor (the yardstick: also one read of x with a tiny result) and with
    eager ``torch.histc``: medians and min / max of --reps after --warmup.  The ratio to dfq_tensor_minmax is stated for both
    fills, and the ratio of the relu fill to the randn fill (above 1.5 the aggregation in front of the LDS is not working).
    TB/s at 4 B per element is quoted for the first shape only, next to the read rate tools/litmus/hbm_stream reports in the
    same job; the other two are launch-latency-sized;
  * the function: the config-5 set-up of tools/empirical_bc_bench.py (synthetic MobileNetV2, BatchNorm folded, weights
    quantised to 8 bits, QuantN* layers, ranges recorded from the batches) at --batches batches of [64, 3, 224, 224]: the whole
    clip_quant_range (two passes over the data, one selection launch) against two plain forward passes over the same data, wall
    time around a final synchronise, and the blocking device-to-host copies counted on the host.

    python tools/act_hist_bench.py [--reps 25] [--warmup 3] [--batches 2] [--fn-reps 3] [--net mobilenet_v2:64,3,224,224] [--out profiles/act_hist_bench.json]
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dfq_amd import _ffi, improve_dfq, synthetic                    # noqa: E402
from dfq_amd.utils import layer_transform as lt                     # noqa: E402
from dfq_amd.utils import quantize as q                             # noqa: E402
from batch_bench_common import alternate, emit, events, wall        # noqa: E402
from batch_table_bench import litmus_read                           # noqa: E402
from empirical_bc_bench import count_host_reads                     # noqa: E402

TARG = [nn.Conv2d, nn.Linear]
SHAPES = [(64, 96, 112, 112), (64, 320, 7, 7), (64, 1000)]
BINS = 2048


def _stat(samples):
    return {'median_us': statistics.median(samples), 'spread_us': [min(samples), max(samples)], 'reps': len(samples)}


def kernel_leg(shape, fill, dev, reps, warmup):
    lib = _ffi.lib()
    g = torch.Generator().manual_seed(len(shape))
    x = torch.randn(*shape, generator=g)
    if fill == 'relu':
        x = torch.relu(x)
    x = x.to(dev)
    n = x.numel()
    range2 = torch.stack([x.min(), x.max()]).to(torch.float32)
    counts = torch.zeros(BINS + 3, dtype=torch.int64, device=dev)
    out2 = torch.empty(2, dtype=torch.float32, device=dev)
    words = torch.zeros(2, dtype=torch.int32, device=dev)
    lo, hi = float(range2[0]), float(range2[1])

    def ours():
        _ffi.check(lib.dfq_act_hist_accumulate(_ffi.ptr(x), n, _ffi.ptr(range2), BINS, _ffi.ptr(counts), _ffi.stream_arg()))

    def minmax():
        _ffi.check(lib.dfq_tensor_minmax(_ffi.ptr(x), n, _ffi.ptr(out2), _ffi.ptr(words), _ffi.stream_arg()))

    def histc():
        return torch.histc(x, bins=BINS, min=lo, max=hi)
    ours()
    torch.cuda.synchronize()
    assert int(counts.sum()) == n and int(counts[BINS:].sum()) == 0, 'the histogram does not hold every element'
    # torch.histc computes its bin in another arithmetic: elements next to an edge may fall one bin to the side
    moved = int((counts[:BINS] - histc().to(torch.int64)).abs().sum()) // 2
    top = int(counts[:BINS].max())
    t = alternate({'act_hist': (ours, events), 'tensor_minmax': (minmax, events), 'torch_histc': (histc, events)}, reps, warmup)
    res = {'shape': list(shape), 'fill': fill, 'elements': n, 'bins': BINS, 'fullest_bin_share': top / n,
           'elements_histc_bins_differently': moved, 'run': {k: _stat(v) for k, v in t.items()}}
    res['act_hist_over_tensor_minmax'] = res['run']['act_hist']['median_us'] / res['run']['tensor_minmax']['median_us']
    res['torch_histc_over_act_hist'] = res['run']['torch_histc']['median_us'] / res['run']['act_hist']['median_us']
    if n * 4 >= (64 << 20):
        gb = n * 4 / 1e9
        for k in res['run']:
            res['run'][k]['GB'] = gb
            res['run'][k]['TBps'] = gb / res['run'][k]['median_us'] * 1e-3 * 1e6
    else:
        res['note'] = 'launch-latency-sized ({} KB): no bandwidth is quoted'.format(n * 4 // 1024)
    return res


def function_leg(dev, n_batches, reps, net='mobilenet_v2', shape=(64, 3, 224, 224)):
    model, graph, bottoms = synthetic.build(net, seed=0)
    lt.merge_batchnorm(model, graph, bottoms, TARG)
    lt.quantize_targ_layer(graph, 8, 16, TARG)
    swapped = improve_dfq._swap_modules(model, {nn.Conv2d: q.QuantNConv2d, nn.Linear: q.QuantNLinear})
    for k in graph:
        if not isinstance(graph[k], str) and graph[k] in swapped:
            graph[k] = swapped[graph[k]]
    qmodel = model.to(dev).eval()
    g = torch.Generator().manual_seed(1)
    data = [torch.randn(*shape, generator=g).clamp_(-2.1179, 2.64).to(dev) for _ in range(n_batches)]
    improve_dfq.set_update_stat(qmodel, [q.QuantMeasure], True)
    improve_dfq.update_quant_range(qmodel, data, graph, bottoms)
    improve_dfq.set_update_stat(qmodel, [q.QuantMeasure], False)
    measures = [m for m in qmodel.modules() if isinstance(m, q.QuantMeasure)]
    start = [(m.running_min.clone(), m.running_max.clone()) for m in measures]
    elements = [0]
    handles = [m.register_forward_pre_hook(lambda mod, a: elements.__setitem__(0, elements[0] + a[0].numel())) for m in measures]
    with torch.no_grad():
        qmodel(data[0])
    for h in handles:
        h.remove()

    def restore():
        with torch.no_grad():
            for m, (lo, hi) in zip(measures, start):
                m.running_min.copy_(lo)
                m.running_max.copy_(hi)

    def clip():
        restore()                                            # every repetition from the same ranges
        improve_dfq.clip_quant_range(qmodel, data, graph, bottoms, method='mse', bins=BINS)

    def two_forward_passes():
        restore()
        with torch.no_grad():
            for _ in range(2):
                for batch in data:
                    qmodel(batch)
    forms = {'clip_quant_range': clip, 'two_forward_passes': two_forward_passes}
    res = {'what': '{} (config-5 set-up of tools/empirical_bc_bench.py), {} batches of {}, {} quantisers, {} quantiser-input elements per '
                   'batch, {} bins, mse'.format(net, n_batches, list(shape), len(measures), elements[0], BINS)}
    for name, fn in forms.items():
        fn()                                                 # warm-up (MIOpen picks its kernels; the allocator has its blocks)
        torch.cuda.synchronize()
        reads = [0]
        with count_host_reads(reads):
            fn()
        torch.cuda.synchronize()
        samples = [wall(fn) for _ in range(reps)]
        res[name] = {'wall_ms': statistics.median(samples) / 1e3, 'spread_ms': [min(samples) / 1e3, max(samples) / 1e3], 'reps': reps,
                     'blocking_device_to_host_copies': reads[0]}
    res['clip_over_two_forward_passes'] = res['clip_quant_range']['wall_ms'] / res['two_forward_passes']['wall_ms']
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=25)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--batches', type=int, default=2)
    ap.add_argument('--fn-reps', type=int, default=3)
    ap.add_argument('--net', default='mobilenet_v2:64,3,224,224', help='net:shape of the function leg')
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), 'act_hist_bench.py needs a ROCm GPU'
    dev = torch.device('cuda', 0)
    res = {'kernel': [kernel_leg(s, fill, dev, args.reps, args.warmup) for s in SHAPES for fill in ('randn', 'relu')],
           'litmus_read': litmus_read()}
    for a, b in zip(res['kernel'][0::2], res['kernel'][1::2]):
        b['relu_over_randn'] = b['run']['act_hist']['median_us'] / a['run']['act_hist']['median_us']
    net, shape = args.net.split(':')
    res['function'] = function_leg(dev, args.batches, args.fn_reps, net, tuple(int(v) for v in shape.split(',')))
    res['device'] = torch.cuda.get_device_name(0)
    emit(res, args.out)


if __name__ == '__main__':
    main()
