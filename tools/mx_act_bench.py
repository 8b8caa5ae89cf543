#!/usr/bin/env python3
"""MX block-scaled activations (dfq_mx_axis / prims.mx_axis / MXQuantMeasure) on the GPU: warm-up, the legs alternating
between device events in one job, median and min-max of --reps.  The tensors are seeded normal values.

Kernel level, for the activation shapes [64, 96, 112, 112], [64, 320, 7, 7] (blocks along the channels) and [64, 1000] (the row
case), E4M3 and E2M1, the exponent search off and on, the stored values alone and with codes and scale bytes:

  * axis        dfq_mx_axis;
  * transposed  what a caller had to do before: movedim(1, -1).contiguous(), dfq_mx_rows, movedim back, contiguous();
  * rows        dfq_mx_rows on a contiguous [outer * inner, len] tensor of the same element count;
  * fake_quant  the integer dfq_fake_quant with a given range on the same tensor (once per shape);
  * the in-place scale rate tools/litmus/hbm_stream reports, if that program has been built.

TB/s counts the bytes dfq_mx_axis moves: 8 B per element, 9 + 1/32 with codes and scales.  The two small shapes are
launch-latency-sized: their times are reported, no bandwidth is claimed for them.

Function level (--part model): one forward pass of the synthetic MobileNetV2 on [64, 3, 224, 224], its layers swapped for
QuantConv2d / QuantLinear, once with the integer QuantMeasure in eval mode and once switched by set_mx_format (activations E4M3
along the channels, weights as they are).  There are no trained weights and no dataset here: whether MX activations help or
hurt accuracy is not measured.

No time is a pass / fail condition.

    python tools/mx_act_bench.py [--part kernels|model|all] [--reps 15] [--warmup 3] [--out profiles/mx_act_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dfq_amd import _ffi, improve_dfq, prims, synthetic                 # noqa: E402
from dfq_amd.utils import layer_transform as lt                         # noqa: E402
from dfq_amd.utils import quantize as q                                 # noqa: E402
from batch_bench_common import alternate, events                        # noqa: E402
from batch_fold_bench import litmus                                     # noqa: E402

SHAPES = [(64, 96, 112, 112), (64, 320, 7, 7), (64, 1000)]
LARGE = SHAPES[0]


def _stat(samples):
    return {'median_us': statistics.median(samples), 'spread_us': [min(samples), max(samples)], 'reps': len(samples)}


def kernels(args, dev):
    lib = _ffi.lib()
    res = {}
    for shape in SHAPES:
        g = torch.Generator().manual_seed(len(shape) + shape[1])
        x = torch.randn(shape, generator=g).to(dev)
        n, length = x.numel(), shape[1]
        outer, inner = shape[0], n // (shape[0] * length)
        bpa = -(-length // _ffi.MX_BLOCK)
        y = torch.empty_like(x)
        codes = torch.empty(shape, dtype=torch.uint8, device=dev)
        scales = torch.empty(outer * bpa * inner, dtype=torch.uint8, device=dev)
        flat = x.reshape(outer * inner, length)                    # the same element count, blocks along contiguous rows
        mn, mx = float(x.min()), float(x.max())
        entry = {'elements': n, 'outer': outer, 'len': length, 'inner': inner}

        def fake_quant():
            q.fake_quant_device(x, y, 8, False, 0, mn, mx, None, None)
        for fmt in ('e4m3', 'e2m1'):
            fid = prims.MX_FORMATS[fmt]
            for search in (0, 1):
                for extra in (False, True):
                    c, s = (_ffi.ptr(codes), _ffi.ptr(scales)) if extra else (None, None)

                    def axis():
                        _ffi.check(lib.dfq_mx_axis(_ffi.ptr(x), _ffi.ptr(y), outer, length, inner, fid, search, c, s, None, _ffi.stream_arg()))

                    def rows():
                        _ffi.check(lib.dfq_mx_rows(_ffi.ptr(flat), _ffi.ptr(y), outer * inner, length, fid, search, c, s, None, _ffi.stream_arg()))

                    def transposed():
                        t = x.movedim(1, -1).contiguous()
                        _ffi.check(lib.dfq_mx_rows(_ffi.ptr(t), _ffi.ptr(t), outer * inner, length, fid, search, c, s, None, _ffi.stream_arg()))
                        return t.movedim(-1, 1).contiguous()
                    legs = {'axis': (axis, events), 'rows': (rows, events), 'fake_quant': (fake_quant, events)}
                    if inner > 1:
                        legs['transposed'] = (transposed, events)
                        # the two routes agree before either is timed
                        axis()
                        if not torch.equal(transposed().view(torch.int32), y.view(torch.int32)):
                            raise RuntimeError('mx_act_bench: dfq_mx_axis and the transposed dfq_mx_rows differ')
                    t = alternate(legs, args.reps, args.warmup)
                    row = {k: _stat(v) for k, v in t.items()}
                    med = {k: v['median_us'] for k, v in row.items()}
                    row['ratio_to_axis'] = {k: v / med['axis'] for k, v in med.items() if k != 'axis'}
                    row['ns_per_element'] = {k: v * 1e3 / n for k, v in med.items()}
                    if shape == LARGE:
                        moved = n * (9 + 1 / 32 if extra else 8)
                        row['bytes_axis'] = moved
                        row['TBps_at_the_bytes_of_axis'] = {k: moved / v * 1e-6 for k, v in med.items() if k != 'fake_quant'}
                        row['TBps_fake_quant_8B'] = 8 * n / med['fake_quant'] * 1e-6
                    entry['{} search {}{}'.format(fmt, search, ' +codes+scales' if extra else '')] = row
        res['x'.join(map(str, shape))] = entry
        del x, y, codes, scales, flat
        torch.cuda.empty_cache()
    res['note'] = 'only {} is large enough for a bandwidth figure; the others are launch-latency-sized'.format('x'.join(map(str, LARGE)))
    res['hbm_stream'] = litmus() or 'not measured yet'
    return res


def _quant_mobilenet(dev):
    model, graph, bottoms = synthetic.build('mobilenet_v2', seed=0)
    model.to(dev)
    lt.merge_batchnorm(model, graph, bottoms, [nn.Conv2d, nn.Linear])
    swapped = improve_dfq._swap_modules(model, {nn.Conv2d: q.QuantConv2d, nn.Linear: q.QuantLinear})
    for k in graph:
        if not isinstance(graph[k], str) and graph[k] in swapped:
            graph[k] = swapped[graph[k]]
    model.to(dev)                                                  # (the swapped layers' quantisers are born on the host)
    lt.set_quant_minmax(graph, bottoms, verbose=False)
    return model.eval(), graph


def model(args, dev):
    integer, _ = _quant_mobilenet(dev)
    mxnet, graph = _quant_mobilenet(dev)
    layers = q.set_mx_format(graph, 'e4m3', targ_type=[q.QuantConv2d, q.QuantLinear])
    g = torch.Generator().manual_seed(1)
    x = torch.randn(64, 3, 224, 224, generator=g).clamp_(-2.1179, 2.64).to(dev)
    with torch.no_grad():
        t = alternate({'integer': (lambda: integer(x), events), 'mx_e4m3': (lambda: mxnet(x), events)}, args.model_reps, 2)
    res = {k: _stat(v) for k, v in t.items()}
    res['ratio_mx_over_integer'] = res['mx_e4m3']['median_us'] / res['integer']['median_us']
    res['layers_switched'] = layers
    res['input'] = [64, 3, 224, 224]
    res['accuracy'] = 'not measured: no trained weights and no dataset'
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--part', choices=('kernels', 'model', 'all'), default='all')
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--model-reps', type=int, default=9)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    dev = torch.device('cuda', 0)
    res = {}
    if args.out and os.path.exists(args.out):                      # (the two parts may come from two runs)
        with open(args.out) as f:
            res = json.loads(f.read())
    if args.part in ('kernels', 'all'):
        res['kernels'] = kernels(args, dev)
    if args.part in ('model', 'all'):
        res['model'] = model(args, dev)
    res['device'] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or '.', exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
