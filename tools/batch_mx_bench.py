#!/usr/bin/env python3
"""MX block-scaled FP4 / FP6 / FP8 weights of a batch (NetworkBatch.mx_plan / quantize_mx) on the GPU (warm-up, alternating
legs between device events, median and min-max of --reps), for a batch of --batch equalised MobileNetV2
(synthetic.build('mobilenet_v2', seed=s % 4), BatchNorm folded, le_plan run once).  The weights are restored in front of every
repetition, outside the measurement.

  * the ERRORS stage for the widths (4, 6, 8): one read of every weight, three formats, the exponent search in each;
  * the QUANTISE stage at 4 bits with and without the search: 4 B read, 4 B written, 1 B code and 1/32 B scale per weight;
  * what quantize_mx(avg_bits=5) enqueues, end to end: ERRORS, the allocation of mixed_plan(costs=) on those errors, QUANTISE
    at the widths the allocation left on the device;
  * the decode launch of unpack_plan on MX-packed words: 1 B code read, 4 B written per weight;
  * the yardsticks, alternating in the same job: the per-channel BatchQuantPlan.run() at 4 bits with 1-byte codes (weights only:
    bits_bias=32; 4 B read, 4 B written and 1 B code per weight, the bytes of QUANTISE), and the read rate
    tools/litmus/hbm_stream reports, if that program has been built;
  * sum e^2 per format with and without the search, and the share of blocks that take the exponent above the floor rule's.

No time is a pass / fail condition.

    python tools/batch_mx_bench.py [--reps 25] [--warmup 3] [--batch 64] [--avg-bits 5] [--out profiles/batch_mx_bench.json]
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
WIDTHS = (4, 6, 8)


def _stat(samples):
    return {'median_us': statistics.median(samples), 'spread_us': [min(samples), max(samples)], 'reps': len(samples)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=25)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--avg-bits', type=float, default=5.0)
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    dev = torch.device('cuda', 0)
    batch = arena.NetworkBatch(_nets(args.batch, dev, TARG), TARG)
    le = batch.le_plan()
    le.run()
    le.close()
    torch.cuda.synchronize()
    pristine = batch.storage.clone()

    def restore():
        batch.storage.copy_(pristine)

    def ev(fn):
        return events(fn, restore)

    lib = _ffi.lib()
    search = batch.mx_plan(WIDTHS, bit_weight=4, search=True)
    floor = batch.mx_plan(WIDTHS, bit_weight=4, search=False)
    alloc_mx = batch.mx_plan(WIDTHS, bit_weight=4, search=True)
    mixed = batch.mixed_plan(WIDTHS, avg_bits=args.avg_bits, apply=False, costs=alloc_mx)
    alloc_mx.set_widths(mixed)
    quant = batch.quant_plan(4, 32, per_channel=True, codes='int8')

    def end_to_end():
        alloc_mx.run(alloc_mx.ERRORS)
        mixed.run()
        alloc_mx.run(alloc_mx.QUANTISE)

    # what the decode leg reads: the codes and scales of one end-to-end run, packed and unpacked once
    end_to_end()
    pack = batch.pack_plan(alloc_mx)
    pack.run()
    _ffi.synchronize()
    quantised = batch.storage.clone()
    unpack = batch.unpack_plan(pack, weights=True)
    restore()
    unpack.run()
    _ffi.synchronize()
    if any(alloc_mx.status_block.cpu().tolist()) or any(pack.status_block.cpu().tolist()) or any(unpack.status(n) for n in range(args.batch)):
        raise RuntimeError('batch_mx_bench: a network did not quantise, pack or unpack')
    if not torch.equal(batch.storage.view(torch.int32), quantised.view(torch.int32)):
        raise RuntimeError('batch_mx_bench: the decoded weights are not the quantised ones')
    bits = mixed.bits_block.cpu()

    def decode():
        _ffi.check(lib.dfq_batch_mx_decode_plan_run(unpack._decode, _ffi.stream_arg()))

    legs = {'errors': (lambda: search.run(search.ERRORS), ev), 'quantise_search': (lambda: search.run(search.QUANTISE), ev),
            'quantise_floor': (lambda: floor.run(floor.QUANTISE), ev), 'quantize_mx': (end_to_end, ev), 'decode': (decode, ev),
            'quant_plan': (quant.run, ev)}
    t = alternate(legs, args.reps, args.warmup, restore)

    # sum e^2 per format and the share of blocks above the floor rule's exponent, outside the measurement
    restore()
    search.run(search.ERRORS)
    floor.run(floor.ERRORS)
    _ffi.synchronize()
    e_search = search.error_block.sum(dim=(0, 1)).cpu().tolist()
    e_floor = floor.error_block.sum(dim=(0, 1)).cpu().tolist()
    raised = {}
    n_blocks = sum(n_blk for (_, _, n_blk, _) in search._scale_views)
    for width in WIDTHS:
        scales = []
        for rule in (True, False):
            restore()
            plan = batch.mx_plan(WIDTHS, bit_weight=width, search=rule)
            plan.run(plan.QUANTISE)
            _ffi.synchronize()
            scales.append(torch.cat([plan.scale_block[:, off:off + n_blk] for (_, off, n_blk, _) in plan._scale_views], dim=1).clone())
            plan.close()
        raised[str(width)] = float((scales[0] != scales[1]).sum()) / (args.batch * n_blocks)
    restore()
    _ffi.synchronize()

    weights = search.elements
    total = args.batch * weights
    res = {'networks': args.batch, 'widths': list(WIDTHS), 'avg_bits': args.avg_bits, 'weights_per_network': weights,
           'tensors_per_network': search.n_tensors, 'blocks_per_network': n_blocks, 'scale_bits_per_weight': 8.0 * n_blocks / weights}
    res.update({k: _stat(v) for k, v in t.items()})
    res['launches'] = {'errors': 2, 'quantise_search': 1, 'quantise_floor': 1, 'quantize_mx': 3 + mixed.launches, 'decode': 1,
                       'quant_plan': quant.launches}
    scale_bytes = args.batch * n_blocks
    res['bytes'] = {'errors': 4 * total, 'quantise_search': 9 * total + scale_bytes, 'quantise_floor': 9 * total + scale_bytes,
                    'decode': 5 * total + scale_bytes, 'quant_plan': 9 * total}
    res['TBps'] = {k: v / res[k]['median_us'] * 1e-6 for k, v in res['bytes'].items()}
    med = {k: res[k]['median_us'] for k in legs}
    res['ratios'] = {'quantise_search_over_quant_plan': med['quantise_search'] / med['quant_plan'],
                     'quantise_search_over_floor': med['quantise_search'] / med['quantise_floor'],
                     'errors_over_quantise_search': med['errors'] / med['quantise_search'],
                     'quantize_mx_over_quantise_search': med['quantize_mx'] / med['quantise_search'],
                     'decode_over_quant_plan': med['decode'] / med['quant_plan']}
    res['sum_e2'] = {'search': dict(zip(map(str, WIDTHS), e_search)), 'floor': dict(zip(map(str, WIDTHS), e_floor)),
                     'search_over_floor': {str(w): a / b for w, a, b in zip(WIDTHS, e_search, e_floor)}}
    res['blocks_above_the_floor_exponent'] = raised
    res['allocated_widths'] = {str(w): int((bits == w).sum()) for w in WIDTHS}
    for p in (unpack, pack, quant, mixed, alloc_mx, floor, search):
        p.close()
    hbm = litmus_read()
    res['hbm_stream'] = hbm or 'not measured yet'
    if hbm:
        best = max(hbm['read_TBps'], hbm['read_nt_TBps'])
        res['fraction_of_hbm_stream'] = {k: v / best for k, v in res['TBps'].items()}
    res['device'] = torch.cuda.get_device_name(0)
    emit(res, args.out)


if __name__ == '__main__':
    main()
