#!/usr/bin/env python3
"""Empirical bias correction on distilled data (improve_dfq.bias_correction_distill, dfq_channel_sum.hip) on the GPU:

  * the kernel: dfq_channel_sum_accumulate on [64, 96, 112, 112], [64, 320, 7, 7] and [64, 1000] between device events,
    alternating with torch's eager float64 reduction of the same tensor (``x.sum(dim=(0, 2, 3), dtype=torch.float64)``, or
    ``dim=0`` for the matrix): medians of --reps after --warmup.  TB/s at 4 B per element is quoted for the first shape only,
    next to the read rate tools/litmus/hbm_stream reports in the same job; the other two are launch-latency-sized.  The
    yardsticks are the eager reduction and the stream read; neither is the code under test;
  * the function: the config-5 set-up of bench.py (synthetic MobileNetV2, BatchNorm folded, weights quantised to 8 bits,
    QuantN* layers, ranges recorded from the batches; without the tensor-op quantisers, see function_leg) at --batches batches of [64, 3, 224, 224]: bias_correction_distill against
    the eager restatement of improve_dfq.py:311-371 with hooks that keep the outputs, written here.  Per form: wall time
    around a final synchronise, torch.cuda.max_memory_allocated(), and the blocking device-to-host copies, counted on the
    host (calls of Tensor.cpu / Tensor.item / Tensor.tolist inside the call).

    python tools/empirical_bc_bench.py [--reps 25] [--warmup 3] [--batches 2] [--fn-reps 3] [--net mobilenet_v2:64,3,224,224] [--out profiles/empirical_bc_bench.json]
"""
import argparse
import contextlib
import copy
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

TARG = [nn.Conv2d, nn.Linear]
SHAPES = [(64, 96, 112, 112), (64, 320, 7, 7), (64, 1000)]


def _stat(samples):
    return {'median_us': statistics.median(samples), 'spread_us': [min(samples), max(samples)], 'reps': len(samples)}


def kernel_leg(shape, dev, reps, warmup):
    lib = _ffi.lib()
    g = torch.Generator().manual_seed(len(shape))
    x = torch.randn(*shape, generator=g).to(dev)
    n, c = shape[0], shape[1]
    hw = x[0, 0].numel()
    acc = torch.zeros(c, dtype=torch.float64, device=dev)
    scratch = torch.empty(int(lib.dfq_channel_sum_scratch_bytes(n, c, hw)) // 8, dtype=torch.float64, device=dev)
    dims = (0, 2, 3) if x.dim() == 4 else 0

    def ours():
        _ffi.check(lib.dfq_channel_sum_accumulate(_ffi.ptr(x), n, c, hw, 1.0, _ffi.ptr(acc), _ffi.ptr(scratch), _ffi.stream_arg()))

    def eager():
        return x.sum(dim=dims, dtype=torch.float64)
    ours()
    torch.cuda.synchronize()
    want = eager()
    rel = float(((acc - want).abs() / want.abs().clamp_min(1e-300)).max())
    assert rel < 1e-9, 'the legs do not compute the same sums ({})'.format(rel)
    t = alternate({'channel_sum': (ours, events), 'eager_float64_sum': (eager, events)}, reps, warmup)
    res = {'shape': list(shape), 'elements': x.numel(), 'max_rel_difference': rel, 'run': {k: _stat(v) for k, v in t.items()}}
    res['eager_over_channel_sum'] = res['run']['eager_float64_sum']['median_us'] / res['run']['channel_sum']['median_us']
    if x.numel() * 4 >= (64 << 20):
        gb = x.numel() * 4 / 1e9
        for k in res['run']:
            res['run'][k]['GB'] = gb
            res['run'][k]['TBps'] = gb / res['run'][k]['median_us'] * 1e-3 * 1e6
    else:
        res['note'] = 'launch-latency-sized ({} KB): no bandwidth is quoted'.format(x.numel() * 4 // 1024)
    return res


class _Keep:
    """the reference's ModuleHook: keeps the whole output"""

    def __init__(self):
        self.outputs = None

    def hook(self, module, inputs, output):
        self.outputs = output

    def clear(self):
        self.outputs = None


def eager_restatement(qmodel, model_original, data, targ_type, targ_type_original):
    """improve_dfq.py:311-371 as written there: retaining hooks, mean(0) and a blocking copy per hooked layer, model and batch"""
    hooks, hooks_original, handles = [], [], []
    for module in qmodel.modules():
        if type(module) in targ_type:
            hooks.append((_Keep(), module))
            handles.append(module.register_forward_hook(hooks[-1][0].hook))
    for module in model_original.modules():
        if type(module) in targ_type_original:
            hooks_original.append((_Keep(), module))
            handles.append(module.register_forward_hook(hooks_original[-1][0].hook))
    error_list = {}
    with torch.no_grad():
        for b, batch in enumerate(data):
            for h, _ in hooks + hooks_original:
                h.clear()
            qmodel(batch)
            model_original(batch)
            for idx in range(len(hooks)):
                if b == 0:
                    error_list[idx] = [hooks[idx][0].outputs.mean(0).cpu(), hooks_original[idx][0].outputs.mean(0).cpu()]
                else:
                    error_list[idx][0] += hooks[idx][0].outputs.mean(0).cpu()
                    error_list[idx][1] += hooks_original[idx][0].outputs.mean(0).cpu()
        for idx, (_, module) in enumerate(hooks):
            error = (error_list[idx][0] - error_list[idx][1]) / len(data)
            error = error.view(error.size(0), -1).sum(-1)
            if getattr(module, 'bias', None) is None:
                module.bias = nn.Parameter(torch.zeros(error.size(0), device=module.weight.device), requires_grad=False)
            module.bias.add_(-error.to(module.bias.device))
    for h in handles:
        h.remove()


@contextlib.contextmanager
def count_host_reads(counter):
    """count the calls that make the host wait for device data: Tensor.cpu / .item / .tolist on a device tensor"""
    saved = {name: getattr(torch.Tensor, name) for name in ('cpu', 'item', 'tolist')}

    def wrap(fn):
        def inner(self, *a, **kw):
            if self.is_cuda:
                counter[0] += 1
            return fn(self, *a, **kw)
        return inner
    for name, fn in saved.items():
        setattr(torch.Tensor, name, wrap(fn))
    try:
        yield
    finally:
        for name, fn in saved.items():
            setattr(torch.Tensor, name, fn)


def function_leg(dev, n_batches, reps, net='mobilenet_v2', shape=(64, 3, 224, 224)):
    model, graph, bottoms = synthetic.build(net, seed=0)
    lt.merge_batchnorm(model, graph, bottoms, TARG)
    original = copy.deepcopy(model).to(dev).eval()
    lt.quantize_targ_layer(graph, 8, 16, TARG)
    swapped = improve_dfq._swap_modules(model, {nn.Conv2d: q.QuantNConv2d, nn.Linear: q.QuantNLinear})
    for k in graph:
        if not isinstance(graph[k], str) and graph[k] in swapped:
            graph[k] = swapped[graph[k]]
    # (not fxgraph.quantize_tensor_ops on top, as bench.py has it: the GraphModule it returns inlines the QuantN* layers, and a
    # layer that is no module any more cannot be hooked by its type)
    qmodel = model.to(dev).eval()
    g = torch.Generator().manual_seed(1)
    data = [torch.randn(*shape, generator=g).clamp_(-2.1179, 2.64).to(dev) for _ in range(n_batches)]
    improve_dfq.set_update_stat(qmodel, [q.QuantMeasure], True)
    improve_dfq.update_quant_range(qmodel, data, graph, bottoms)
    improve_dfq.set_update_stat(qmodel, [q.QuantMeasure], False)
    targ_q = [q.QuantNConv2d, q.QuantNLinear]
    hooked = sum(1 for m in qmodel.modules() if type(m) in targ_q)
    forms = {'bias_correction_distill': lambda: improve_dfq.bias_correction_distill(qmodel, original, data, targ_q, TARG),
             'eager_retaining_hooks': lambda: eager_restatement(qmodel, original, data, targ_q, TARG)}
    res = {'what': '{} (config-5 set-up of bench.py), {} batches of {}, {} hooked layers per model'.format(net, n_batches, list(shape), hooked)}
    for name, fn in forms.items():
        fn()                                                 # warm-up (MIOpen picks its kernels; the allocator has its blocks)
        torch.cuda.synchronize()
        reads = [0]
        with count_host_reads(reads):
            fn()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        samples = [wall(fn) for _ in range(reps)]
        res[name] = {'wall_ms': statistics.median(samples) / 1e3, 'spread_ms': [min(samples) / 1e3, max(samples) / 1e3], 'reps': reps,
                     'max_memory_allocated_MB': torch.cuda.max_memory_allocated() / 2 ** 20, 'allocated_before_MB': base / 2 ** 20,
                     'blocking_device_to_host_copies': reads[0]}
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
    assert torch.cuda.is_available(), 'empirical_bc_bench.py needs a ROCm GPU'
    dev = torch.device('cuda', 0)
    res = {'kernel': [kernel_leg(s, dev, args.reps, args.warmup) for s in SHAPES], 'litmus_read': litmus_read()}
    net, shape = args.net.split(':')
    res['function'] = function_leg(dev, args.batches, args.fn_reps, net, tuple(int(v) for v in shape.split(',')))
    res['device'] = torch.cuda.get_device_name(0)
    emit(res, args.out)


if __name__ == '__main__':
    main()
