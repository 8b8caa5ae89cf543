#!/usr/bin/env python3
"""Batch ncnn calibration tables (NetworkBatch.table_plan / calibration_tables) against the loop of per-network
ncnn_table.calibration_table calls, on the GPU (warm-up, alternating legs, medians of --reps), for a batch of --batch
MobileNetV2 (synthetic.build('mobilenet_v2', seed=s % 4)) with QConv2d / QLinear layers, quantisers filled by
NetworkBatch.set_quant_minmax():

  * (a) BatchTablePlan.run() between device events, and the TB/s it implies at 4 B per weight (every weight read once,
    nothing written but the small block), alternating with BatchQuantPlan.run() per tensor without codes and biases -- the
    plan whose first launch, bq_chunk_minmax_kernel, is the other min/max pass over the same bytes (its own time: the
    rocprofv3 run below) -- and next to the read rate tools/litmus/hbm_stream reports in the same job, if it has been built;
  * (b) calibration_tables() by the host's clock, per tensor and per channel, against the loop of calibration_table calls in
    the same mode (the loop is the code the batch form replaces: one plan + read-back per network per tensor, one launch +
    read-back per layer per channel, two blocking reads per layer for the activation ranges);
  * (c) the two halves of calibration_tables() on their own: the device side (plan, run, two copies) and the host's
    formatting of the strings, which both forms pay alike.

    python tools/batch_table_bench.py [--reps 15] [--warmup 3] [--batch 64] [--loop-reps 5] [--out profiles/batch_table_bench.json]

Kernel durations come from a separate `rocprofv3 --kernel-trace --stats -- python tools/batch_table_bench.py --reps 3 --loop-reps 1`.
"""
import argparse
import os
import re
import statistics
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dfq_amd import _ffi, arena, ncnn_table                           # noqa: E402
from batch_bench_common import ab, alternate, emit, wall, nets as _nets   # noqa: E402
from batch_act_bench import QTARG, _q_graph                           # noqa: E402


def litmus_read():
    """the best read rate tools/litmus/hbm_stream reports over its grids, or None if the program is not there"""
    exe = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'litmus', 'hbm_stream')
    if not os.path.exists(exe):
        return None
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300).stdout
    best = None
    for line in out.splitlines():
        m = re.search(r'grid\s+(\d+) \| read ([\d.]+) / nt ([\d.]+) TB/s', line)
        if m:
            row = {'grid': int(m.group(1)), 'read_TBps': float(m.group(2)), 'read_nt_TBps': float(m.group(3))}
            if best is None or max(row['read_TBps'], row['read_nt_TBps']) > max(best['read_TBps'], best['read_nt_TBps']):
                best = row
    return best


def _stat(samples):
    return {'median_us': statistics.median(samples), 'spread_us': [min(samples), max(samples)], 'reps': len(samples)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--loop-reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    dev = torch.device('cuda', 0)
    nets = _nets(args.batch, dev, QTARG, _q_graph)
    batch = arena.NetworkBatch(nets, QTARG)
    act = batch.set_quant_minmax()
    torch.cuda.synchronize()
    plan = batch.table_plan()
    layers = plan.n_tensors
    res = {'networks': args.batch, 'layers': layers, 'weights_per_network': plan.elements, 'launches': plan.launches,
           'block_floats_per_network': int(plan.block.shape[1]),
           'loop_launches': {'per_tensor': args.batch, 'per_channel': args.batch * (1 + layers)},
           'loop_blocking_reads': {'per_tensor': args.batch * (1 + 2 * layers), 'per_channel': args.batch * (1 + 3 * layers)}}

    # (a) the read-only pass, alternating with the per-tensor quantisation plan over the same weights
    snap = batch.storage.clone()
    quant = batch.quant_plan(8, 32, per_channel=False, codes=None)
    r = ab('table', plan.run, 'quant_per_tensor', quant.run, args.reps, args.warmup)
    quant.close()
    batch.storage.copy_(snap)
    torch.cuda.synchronize()
    gb = args.batch * plan.elements * 4 / 1e9
    res['run'] = dict(r, GB=gb, TBps=gb / r['table_us'] * 1e-3 * 1e6, quant_per_tensor_launches=2,
                      litmus_read=litmus_read())
    plan.close()

    # (b) the whole call against the loop, by the host's clock; the lines must be the same
    def batch_tables(pc):
        return lambda: batch.calibration_tables(act=act, per_channel=pc)

    def loop_tables(pc):
        return lambda: [ncnn_table.calibration_table(g, targ_type=QTARG, per_channel=pc) for (g, _, _) in nets]
    for pc, mode in ((False, 'per_tensor'), (True, 'per_channel')):
        assert batch_tables(pc)() == loop_tables(pc)(), 'the batch tables differ from the loop ({})'.format(mode)
        t = alternate({'batch': (batch_tables(pc), wall), 'loop': (loop_tables(pc), wall)}, args.loop_reps, 1)
        a, b = _stat(t['batch']), _stat(t['loop'])
        res['tables_' + mode] = {'batch': a, 'loop': b, 'ratio': b['median_us'] / a['median_us']}

    # (c) the halves of the batch call
    names = ['{}_param_0'.format(k) for k in batch._table_keys()] + [str(k) for k in batch._table_keys()]
    stats = batch._table_statistics(act)
    t = alternate({'device_side': (lambda: batch._table_statistics(act), wall),
                   'format_per_tensor': (lambda: batch._format_tables(names, False, *stats), wall),
                   'format_per_channel': (lambda: batch._format_tables(names, True, *stats), wall)}, args.reps, 1)
    res['halves'] = {k: _stat(v) for k, v in t.items()}
    _ffi.synchronize()
    res['device'] = torch.cuda.get_device_name(0)
    emit(res, args.out)


if __name__ == '__main__':
    main()
