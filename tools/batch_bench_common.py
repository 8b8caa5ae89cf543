"""What tools/batch_quant_bench.py, batch_absorb_bench.py, batch_act_bench.py and batch_fold_bench.py share: the batch of synthetic MobileNetV2 they
time, the device-event and wall-clock timers, the alternating A/B loop and the one JSON line they print and write."""
import json
import os
import statistics
import time

import torch

from dfq_amd import synthetic
from dfq_amd.utils import layer_transform as lt
from dfq_amd.utils import relation as rel


def nets(n, dev, targ, convert=None, fold=True):
    """[(graph, bottoms, relations)] of n MobileNetV2 (seed s % 4) on `dev`, BatchNorm folded (`fold=False`: as loaded, not
    folded); `convert(graph, dev)` may swap the graph's layers for others before that"""
    out = []
    for s in range(n):
        model, graph, bottoms = synthetic.build('mobilenet_v2', seed=s % 4)
        model.to(dev)
        if convert is not None:
            graph = convert(graph, dev)
        if fold:
            lt.merge_batchnorm(model, graph, bottoms, targ)
        out.append((graph, bottoms, rel.create_relation(graph, bottoms, targ, delete_single=False)))
    return out


def events(fn, prep=None):
    """us between two device events around fn(); `prep()` runs in front of them, outside the measurement"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if prep is not None:
        prep()
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def wall(fn):
    """us by the host's clock, the device idle before and after"""
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e6


def alternate(fns, reps, warmup, prep=None):
    """{name: (fn, timer)} -> {name: samples}, the order rotated from repetition to repetition"""
    names = list(fns)
    for _ in range(warmup):
        for k in names:
            if prep is not None:
                prep()
            fns[k][0]()
    torch.cuda.synchronize()
    out = {k: [] for k in names}
    for i in range(reps):
        for k in names[i % len(names):] + names[:i % len(names)]:
            fn, timer = fns[k]
            out[k].append(timer(fn))
    return out


def ab(name_a, fa, name_b, fb, reps, warmup, prep=None):
    """two functions alternating between device events: medians, their ratio and the spreads"""
    def timer(fn):
        return events(fn, prep)
    t = alternate({name_a: (fa, timer), name_b: (fb, timer)}, reps, warmup, prep)
    ma, mb = statistics.median(t[name_a]), statistics.median(t[name_b])
    return {name_a + '_us': ma, name_b + '_us': mb, 'ratio': ma / mb,
            name_a + '_spread_us': [min(t[name_a]), max(t[name_a])], name_b + '_spread_us': [min(t[name_b]), max(t[name_b])],
            'reps': reps}


def emit(res, out):
    """print the result as one JSON line and write it to `out` if given"""
    line = json.dumps(res)
    print(line)
    if out:
        os.makedirs(os.path.dirname(out) or '.', exist_ok=True)
        with open(out, 'w') as f:
            f.write(line + '\n')
