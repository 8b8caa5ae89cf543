#!/usr/bin/env python3
"""Dense bit-packing of a batch's codes (NetworkBatch.pack_plan / unpack_plan) on the GPU (warm-up, alternating legs between
device events, median and min-max of --reps), for a batch of --batch equalised MobileNetV2 (synthetic.build('mobilenet_v2',
seed=s % 4), BatchNorm folded, le_plan run once) quantised by mixed_plan((2, 3, 4, 6, 8), avg_bits=4, codes='int8'), whose
widths the packing reads on the device.  The weights are restored in front of every repetition, outside the measurement.

  * BatchPackPlan.run(): the offsets (one workgroup per network) and the packing, 1 B read and b / 8 B written per weight;
  * BatchUnpackPlan.run() to the weights: b / 8 B read and 4 B written per weight;
  * their yardsticks, alternating in the same job: BatchQuantPlan.run() per tensor at 4 bits with 1-byte codes (weights
    only: bits_bias=32; two launches, 13 B per weight as tools/batch_quant_bench.py counts them: the min/max read, the read,
    the write, the code), and the read rate tools/litmus/hbm_stream reports, if that program has been built;
  * the packed size against the allocation's ``used`` bits and against one byte per weight.

    python tools/batch_pack_bench.py [--reps 25] [--warmup 3] [--batch 64] [--avg-bits 4] [--out profiles/batch_pack_bench.json]
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dfq_amd import _ffi, arena                                        # noqa: E402
from batch_bench_common import alternate, emit, events, nets as _nets   # noqa: E402
from batch_table_bench import litmus_read                               # noqa: E402

TARG = [nn.Conv2d, nn.Linear]
WIDTHS = (2, 3, 4, 6, 8)


def _stat(samples):
    return {'median_us': statistics.median(samples), 'spread_us': [min(samples), max(samples)], 'reps': len(samples)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=25)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--avg-bits', type=float, default=4.0)
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    dev = torch.device('cuda', 0)
    nets = _nets(args.batch, dev, TARG)
    batch = arena.NetworkBatch(nets, TARG)
    le = batch.le_plan()
    le.run()
    le.close()
    torch.cuda.synchronize()
    pristine = batch.storage.clone()

    def restore():
        batch.storage.copy_(pristine)

    def ev(fn):
        return events(fn, restore)

    mixed = batch.mixed_plan(WIDTHS, avg_bits=args.avg_bits, codes='int8')
    mixed.run()                                                        # the codes, ranges and widths everything below reads
    _ffi.synchronize()
    quantised = batch.storage.clone()
    pack = batch.pack_plan(mixed)
    pack.run()
    unpack = batch.unpack_plan(pack, weights=True)
    unpack.run()
    _ffi.synchronize()
    quant = batch.quant_plan(4, 32, codes='int8')
    if any(pack.status_block.cpu().tolist()) or any(unpack.status_block.cpu().tolist()):
        raise RuntimeError('batch_pack_bench: a network did not pack')

    t = alternate({'pack_plan': (pack.run, ev), 'unpack_plan': (unpack.run, ev), 'quant_plan': (quant.run, ev)}, args.reps, args.warmup, restore)
    # what unpack leaves is what the mixed plan stored (value for value: a zero may have lost its sign)
    restore()
    unpack.run()
    _ffi.synchronize()
    if not torch.equal(batch.storage, quantised):
        raise RuntimeError('batch_pack_bench: the unpacked weights are not the quantised ones')

    weights = mixed.elements
    words = pack.offset_block[:, -1].cpu()
    used = mixed.used_block[:, 0].cpu()
    packed_bytes = 4 * int(words.sum())
    code_bytes = args.batch * weights
    res = {'networks': args.batch, 'widths': list(WIDTHS), 'avg_bits': args.avg_bits, 'weights_per_network': weights,
           'tensors_per_network': pack.n_tensors, 'budget_bits': mixed.budget, 'word_stride': pack.word_stride,
           'chunk_elements': int(_ffi.lib().dfq_batch_pack_chunk_elements())}
    res.update({k: _stat(v) for k, v in t.items()})
    res['launches'] = {'pack_plan': pack.launches, 'unpack_plan': unpack.launches, 'quant_plan': quant.launches}
    res['bytes'] = {'pack_plan': code_bytes + packed_bytes, 'unpack_plan': packed_bytes + 4 * code_bytes, 'quant_plan': 13 * code_bytes}
    res['TBps'] = {k: res['bytes'][k] / res[k]['median_us'] * 1e-6 for k in res['bytes']}
    res['packed_bits_per_weight'] = {'min': 32.0 * int(words.min()) / weights, 'max': 32.0 * int(words.max()) / weights}
    res['packed_minus_used_bits'] = {'min': int((32 * words - used).min()), 'max': int((32 * words - used).max()), 'bound': 159 * pack.n_tensors}
    res['packed_over_used'] = {'min': float((32.0 * words / used).min()), 'max': float((32.0 * words / used).max())}
    res['packed_over_one_byte_per_weight'] = packed_bytes / code_bytes
    for p in (unpack, pack, quant, mixed):
        p.close()
    restore()
    _ffi.synchronize()
    hbm = litmus_read()
    res['hbm_stream'] = hbm or 'not measured yet'
    if hbm:
        best = max(hbm['read_TBps'], hbm['read_nt_TBps'])
        res['fraction_of_hbm_stream'] = {k: v / best for k, v in res['TBps'].items()}
    res['device'] = torch.cuda.get_device_name(0)
    emit(res, args.out)


if __name__ == '__main__':
    main()
