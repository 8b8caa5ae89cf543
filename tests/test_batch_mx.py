"""MX block-scaled FP4 / FP6 / FP8 weights: dfq_mx_rows, dfq_batch_mx_plan_*, dfq_batch_mx_decode_plan_* and what
dfq_amd.arena builds on them (NetworkBatch.mx_plan, quantize_mx, pack_plan / unpack_plan / save_packed / load_packed of an MX
source, mixed_plan(costs=mx)).

The reference is the definition in include/dfq_hip.h ("MX block-scaled") restated in numpy, in this file: the value grid of a
format built from its parameters, the nearest code by a comparison with the exact midpoint of the two neighbours (a tie to the
even code), the shared exponent from the float32 exponent field of the block's largest magnitude, the block error as the
five-level float64 tree, the search between e0 and e0 + 1 on it.  Everything is float64 arithmetic that is exact on these
operands, so codes, scale bytes, stored weights and block errors are compared bit for bit; only a tensor's error sum, whose
order is the plan's own, is compared within n 2^-53 E of math.fsum."""
import ctypes
import math
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

from dfq_amd import _ffi, arena, prims, synthetic
from dfq_amd.utils import layer_transform as lt
from dfq_amd.utils import relation as rel

from common import TARG

DFQ_ERR_ARG = -1     # include/dfq_hip.h
F32, F64 = np.float32, np.float64
BLOCK = _ffi.MX_BLOCK
assert BLOCK == 32
QNAN = 0x7fc00000
#           id, bits, exponent bits, mantissa bits, bias, largest, emax
FORMATS = OrderedDict([('e2m1', (_ffi.MX_E2M1, 4, 2, 1, 1, 6.0, 2)), ('e2m3', (_ffi.MX_E2M3, 6, 2, 3, 1, 7.5, 2)),
                       ('e3m2', (_ffi.MX_E3M2, 6, 3, 2, 3, 28.0, 4)), ('e4m3', (_ffi.MX_E4M3, 8, 4, 3, 7, 448.0, 8)),
                       ('e5m2', (_ffi.MX_E5M2, 8, 5, 2, 15, 57344.0, 15))])
assert [v[0] for v in FORMATS.values()] == [0, 1, 2, 3, 4] and prims.MX_FORMATS == {k: v[0] for k, v in FORMATS.items()}
NAMES = ['tiny_mobile', 'tiny_res', 'tiny_cat']
SEEDS = [0, 1, 2]


# ---- the definition in numpy ---------------------------------------------------------------------------------------------------
def _grid(fmt):
    """float64 [cmax + 1]: the values of the magnitude codes 0..cmax"""
    _, bits, _, m, bias, largest, _ = FORMATS[fmt]
    vals = []
    for k in range(1 << (bits - 1)):
        x, frac = k >> m, k & ((1 << m) - 1)
        v = frac * 2.0 ** (1 - bias - m) if x == 0 else ((1 << m) + frac) * 2.0 ** (x - bias - m)
        if v > largest:
            break
        vals.append(v)
    g = np.array(vals, dtype=F64)
    assert g[-1] == largest and (np.diff(g) > 0).all()
    return g


def _nearest(v, g):
    """int64 codes of v >= 0 (float64): the nearest grid value, a tie to the even code, saturated at the last"""
    v = np.asarray(v, dtype=F64)
    hi = np.clip(np.searchsorted(g, v, side='left'), 1, len(g) - 1)          # g[hi - 1] < v <= g[hi] inside the grid
    lo = hi - 1
    mid = (g[lo] + g[hi]) / 2                                                    # exact
    even = np.where(lo % 2 == 0, lo, hi)
    k = np.where(v < mid, lo, np.where(v > mid, hi, even))
    return np.where(v >= g[-1], len(g) - 1, k).astype(np.int64)


def _tree(q):
    """[nb]: the balanced tree over q float64 [nb, 32]: level m pairs index i with i xor m"""
    idx = np.arange(BLOCK)
    with np.errstate(all='ignore'):
        for m in (1, 2, 4, 8, 16):
            q = q + q[:, idx ^ m]
    assert (_bits64(q) == _bits64(q[:, :1])).all() or np.isnan(q).any()
    return q[:, 0].copy()


def _at(w, e, fmt):
    """codes, stored float32 and S of blocks w float32 [nb, 32] at the exponents e int [nb]"""
    g = _grid(fmt)
    with np.errstate(all='ignore'):
        v = np.ldexp(np.abs(w).astype(F64), -e[:, None])
        k = _nearest(np.where(np.isfinite(v), v, 0.0), g)
        stored = np.copysign(np.ldexp(g[k], e[:, None]), w).astype(F32)
        d = stored.astype(F64) - w.astype(F64)
        S = _tree(d * d)
    return k, stored, S


def _mx_ref(w, fmt, search):
    """w float32 [rows, row_len] -> dict: stored [rows, row_len] float32, codes uint8, scales uint8 [rows, bpr], S float64
    [rows, bpr], e0 and e int [rows, bpr]"""
    _, bits, _, _, _, _, emax = FORMATS[fmt]
    w = np.ascontiguousarray(w, dtype=F32)
    rows, row_len = w.shape
    bpr = -(-row_len // BLOCK)
    pad = np.zeros((rows, bpr * BLOCK), dtype=F32)                               # absent elements count as +0.0
    pad[:, :row_len] = w
    blk = pad.reshape(rows * bpr, BLOCK)
    amax = np.abs(blk).view(np.uint32).max(axis=1)                               # (NaN patterns on top)
    bad = amax >= 0x7f800000
    E = (amax >> 23).astype(np.int64) - 127
    e0 = np.maximum(E - emax, -127)
    k, stored, S = _at(blk, e0, fmt)
    e = e0.copy()
    if search:
        k1, stored1, S1 = _at(blk, e0 + 1, fmt)
        with np.errstate(all='ignore'):
            up = S1 < S                                                          # a tie or a NaN keeps e0
        e = np.where(up, e0 + 1, e0)
        k, stored, S = np.where(up[:, None], k1, k), np.where(up[:, None], stored1, stored), np.where(up, S1, S)
    codes = (k | (np.signbit(blk).astype(np.int64) << (bits - 1))).astype(np.uint8)
    codes[bad] = 0
    stored = stored.copy()
    stored.view(np.uint32)[bad] = QNAN
    S = np.where(bad, np.nan, S)
    scales = np.where(bad, 255, e + 127).astype(np.uint8)
    cut = lambda a: a.reshape(rows, bpr * BLOCK)[:, :row_len].copy()
    return dict(stored=cut(stored), codes=cut(codes), scales=scales.reshape(rows, bpr), S=S.reshape(rows, bpr),
                e0=e0.reshape(rows, bpr), e=e.reshape(rows, bpr), bad=bad.reshape(rows, bpr))


def _decode_ref(codes, scales, fmt):
    """stored float32 [rows, row_len] from uint8 codes [rows, row_len] and scale bytes [rows, bpr]"""
    _, bits, _, _, _, _, _ = FORMATS[fmt]
    g = _grid(fmt)
    rows, row_len = codes.shape
    s = np.repeat(scales.astype(np.int64), BLOCK, axis=1)[:, :row_len]
    k = codes.astype(np.int64) & ((1 << (bits - 1)) - 1)
    sign = np.where((codes.astype(np.int64) >> (bits - 1)) & 1, -1.0, 1.0)
    with np.errstate(all='ignore'):
        y = np.copysign(np.ldexp(g[k], s - 127), sign).astype(F32)
    y.view(np.uint32)[s == 255] = QNAN
    return y


def _bits64(a):
    return np.ascontiguousarray(a, dtype=F64).view(np.int64)


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.int32)


def _same64(got, want):
    return ((_bits64(got) == _bits64(want)) | (np.isnan(got) & np.isnan(want))).all()


def _assert_rows(got, ref, what):
    y, codes, scales, err = [t.cpu().numpy() for t in got]
    assert np.array_equal(scales, ref['scales']), what + ': scale bytes'
    assert np.array_equal(codes.reshape(ref['codes'].shape), ref['codes']), what + ': codes'
    assert np.array_equal(_bits(y).reshape(ref['stored'].shape), _bits(ref['stored'])), what + ': stored weights'
    assert _same64(err, ref['S']), what + ': block errors'


# ---- 1. the reference against itself and against torch -------------------------------------------------------------------------
def test_e2m1_known_answers():
    g = _grid('e2m1')
    assert g.tolist() == [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]
    for v, want in ((0.25, 0.0), (0.75, 1.0), (1.25, 1.0), (1.75, 2.0), (2.5, 2.0), (3.5, 4.0), (5.0, 4.0), (7.0, 6.0)):
        assert g[_nearest(np.array([v]), g)[0]] == want, v


@pytest.mark.parametrize('fmt', ['e2m1', 'e2m3', 'e3m2'])
def test_small_grids_by_enumeration(fmt):
    g = _grid(fmt)
    _, bits, x, m, _, _, _ = FORMATS[fmt]
    assert len(g) == (1 << (bits - 1)) and bits == 1 + x + m               # these formats have no Inf / NaN code: every code is a value
    idx = np.arange(len(g))
    assert np.array_equal(_nearest(g, g), idx)
    mid = (g[:-1] + g[1:]) / 2
    assert np.array_equal(_nearest(mid, g), np.where(idx[:-1] % 2 == 0, idx[:-1], idx[1:]))
    assert np.array_equal(_nearest(np.nextafter(mid, 0.0), g), idx[:-1])
    assert np.array_equal(_nearest(np.nextafter(mid, np.inf), g), idx[1:])
    assert np.array_equal(_nearest(np.array([g[-1] * 1.01, g[-1] * 2, 1e30]), g), [len(g) - 1] * 3)


@pytest.mark.parametrize('fmt,dtype', [('e4m3', 'float8_e4m3fn'), ('e5m2', 'float8_e5m2')])
def test_fp8_reference_against_torch(fmt, dtype):
    g = _grid(fmt)
    _, _, _, _, _, largest, _ = FORMATS[fmt]
    assert len(g) - 1 == {'e4m3': 126, 'e5m2': 123}[fmt]
    gen = np.random.default_rng(3)
    mid = ((g[:-1] + g[1:]) / 2).astype(F32)
    g32 = g.astype(F32)
    pts = [g32, mid, np.nextafter(mid, F32(0)), np.nextafter(mid, F32(np.inf)), np.nextafter(g32, F32(0))[1:],
           np.nextafter(g32[:-1], F32(np.inf)), gen.uniform(0, largest, 200000).astype(F32),
           np.exp2(gen.uniform(-24, np.log2(largest), 200000)).astype(F32), np.linspace(0, largest, 100001, dtype=F32)]
    x = np.concatenate(pts)
    x = x[x <= F32(largest)]
    want = torch.from_numpy(x).to(getattr(torch, dtype)).view(torch.uint8).numpy().astype(np.int64)
    assert np.array_equal(_nearest(x.astype(F64), g), want)


# ---- 2. dfq_mx_rows ---------------------------------------------------------------------------------------------------------------
def _tensor(gen, rows, row_len):
    """Gaussian rows at scales of their own, a few exact zeros, one all-zero block where there is room"""
    w = gen.standard_normal((rows, row_len)) * np.exp2(gen.integers(-12, 6, size=(rows, 1)))
    w = w.astype(F32)
    w[gen.random((rows, row_len)) < 0.03] = 0.0
    if row_len >= 64:
        w[0, 32:64] = 0.0
    return w


@pytest.mark.parametrize('search', [0, 1])
@pytest.mark.parametrize('fmt', list(FORMATS))
def test_mx_rows_every_shape(engine, fmt, search):
    gen = np.random.default_rng(11 + 7 * FORMATS[fmt][0] + search)
    for rows in (1, 3, 70):
        for row_len in (1, 9, 31, 32, 33, 64, 95, 1537):
            w = _tensor(gen, rows, row_len)
            ref = _mx_ref(w, fmt, search)
            x = torch.from_numpy(w).to(engine.device)
            got = prims.mx_rows(x, fmt, search)
            what = '{} search {} [{}, {}]'.format(fmt, search, rows, row_len)
            _assert_rows(got, ref, what)
            # the tensor's error: the blocks' S, against the exact sum of the elements' d^2
            d = ref['stored'].astype(F64) - w.astype(F64)
            exact = math.fsum((d * d).reshape(-1).tolist())
            total = math.fsum(got[3].cpu().numpy().reshape(-1).tolist())
            print(what, 'sum e^2', total, 'exact', exact)
            assert abs(total - exact) <= w.size * 2.0 ** -53 * exact, what
            again = prims.mx_rows(x, fmt, search)
            assert all(torch.equal(a.cpu().view(torch.uint8), b.cpu().view(torch.uint8)) for a, b in zip(got, again)), what
            assert np.array_equal(_bits(x.cpu().numpy()), _bits(w)), what + ': the input was written'
            assert np.array_equal(_bits(_decode_ref(ref['codes'], ref['scales'], fmt)), _bits(ref['stored'])), what + ': decode of the reference'


# ---- 3. adversarial blocks ----------------------------------------------------------------------------------------------------------
def _run_blocks(engine, blocks, fmt, search, row_len=BLOCK):
    w = np.ascontiguousarray(np.asarray(blocks, dtype=F32).reshape(-1, row_len))
    ref = _mx_ref(w, fmt, search)
    got = prims.mx_rows(torch.from_numpy(w).to(engine.device), fmt, search)
    _assert_rows(got, ref, '{} search {}'.format(fmt, search))
    return w, ref


@pytest.mark.parametrize('search', [0, 1])
@pytest.mark.parametrize('fmt', list(FORMATS))
def test_adversarial_blocks(engine, fmt, search):
    _, bits, _, _, _, largest, emax = FORMATS[fmt]
    g = _grid(fmt)
    gen = np.random.default_rng(5)
    cyc = lambda vals: np.resize(np.asarray(vals, dtype=F64), BLOCK)
    signs = np.where(np.arange(BLOCK) % 3 == 0, -1.0, 1.0)

    # zeros and -0.0: scale byte 0, the sign kept
    w, ref = _run_blocks(engine, [np.zeros(BLOCK), -np.zeros(BLOCK)], fmt, search)
    assert ref['scales'].reshape(-1).tolist() == [0, 0]
    assert (ref['codes'][0] == 0).all() and (ref['codes'][1] == 1 << (bits - 1)).all()
    assert (_bits(ref['stored'][1]) == _bits(F32(-0.0))).all()

    # a subnormal amax: e clamped at -127, the stored subnormals exact
    sub = g[g < 2.0]
    w, ref = _run_blocks(engine, [cyc(sub) * signs * 2.0 ** -127, cyc(sub[:2]) * 2.0 ** -127], fmt, search)
    assert (np.abs(w).max(axis=1) < 2.0 ** -126).all() and (ref['e0'] == -127).all() and (ref['scales'][:, 0] <= 1).all()
    if not search:
        assert ref['scales'].reshape(-1).tolist() == [0, 0] and np.array_equal(_bits(ref['stored']), _bits(w))
    assert ref['stored'][1, 1] == F32(g[1] * 2.0 ** -127) or search

    # the largest float32 as amax
    blk = (cyc(g) * signs * 2.0 ** (127 - emax)).astype(F32)
    blk[5] = np.finfo(F32).max
    w, ref = _run_blocks(engine, [blk], fmt, search)
    assert ref['e'][0, 0] == 127 - emax and np.isfinite(ref['stored']).all()

    # amax just below, at and just above a power of two
    rest = (gen.standard_normal(BLOCK) * 0.3).astype(F32)
    blocks = []
    for p in (-140, -126, -20, 0, 1, 100):
        for a in (np.nextafter(F32(1), F32(0)), F32(1), np.nextafter(F32(1), F32(2))):
            blk = (rest.astype(F64) * 2.0 ** p).astype(F32)
            blk[17] = -F32(a.astype(F64) * 2.0 ** p)
            blocks.append(blk)
    _run_blocks(engine, blocks, fmt, search)

    # amax in (7, 8) 2^k with the rest exact at both exponents: the floor rule saturates E2M1, the search does not
    blocks = []
    for k in (-100, -3, 0, 40):
        blk = cyc([0.0, 2.0, 4.0, 0.0]) * 2.0 ** k
        blk[9] = 7.5 * 2.0 ** k
        blocks.append(blk)
    w, ref = _run_blocks(engine, blocks, fmt, search)
    if fmt == 'e2m1':
        for i, k in enumerate((-100, -3, 0, 40)):
            assert ref['e0'][i, 0] == k
            assert ref['stored'][i, 9] == F32((8.0 if search else 6.0) * 2.0 ** k)
            assert ref['e'][i, 0] == k + search

    # every element on a tie (the block's exponent pinned by one element at the largest magnitude)
    mid = (g[:-1] + g[1:]) / 2
    blk = cyc(mid) * signs
    blk[0] = largest
    w, ref = _run_blocks(engine, [blk * 2.0 ** k for k in (-60, 0, 33)], fmt, search)
    if not search:
        lo = np.resize(np.arange(len(g) - 1), BLOCK)
        want = np.where(lo % 2 == 0, lo, lo + 1)
        assert np.array_equal((ref['codes'][1] & ((1 << (bits - 1)) - 1))[1:], want[1:])

    # a NaN block and an Inf block, each between two finite ones (rows of three blocks)
    fin = (gen.standard_normal((2, 3 * BLOCK)) * 0.1).astype(F32)
    fin[0, BLOCK + 3] = np.nan
    fin[1, BLOCK + 30] = -np.inf
    w, ref = _run_blocks(engine, fin, fmt, search, row_len=3 * BLOCK)
    assert ref['scales'][:, 1].tolist() == [255, 255] and (ref['scales'][:, [0, 2]] != 255).all()
    assert (ref['stored'][:, BLOCK:2 * BLOCK].view(np.uint32) == QNAN).all() and (ref['codes'][:, BLOCK:2 * BLOCK] == 0).all()
    assert np.isnan(ref['S'][:, 1]).all() and np.isfinite(ref['S'][:, [0, 2]]).all()
    assert np.isfinite(ref['stored'][:, :BLOCK]).all() and np.isfinite(ref['stored'][:, 2 * BLOCK:]).all()

    # Gaussian blocks: the search takes e0 + 1 for some and e0 for others
    if search:
        blocks = gen.standard_normal((96, BLOCK)).astype(F32)
        ref = _mx_ref(blocks, fmt, 1)
        up = (ref['e'] != ref['e0']).reshape(-1)
        print(fmt, 'e0 + 1 in', up.mean())
        assert up.any() and not up.all()
        floor = _mx_ref(blocks, fmt, 0)
        assert (ref['S'] <= floor['S']).all() and (ref['S'][up.reshape(-1, 1)] < floor['S'][up.reshape(-1, 1)]).all()
        _run_blocks(engine, blocks, fmt, 1)


# ---- 4. mx_plan on the batch ---------------------------------------------------------------------------------------------------------
def _prepared(name, seed, device):
    model, graph, bottoms = synthetic.build(name, seed=seed)
    model.to(device)
    lt.merge_batchnorm(model, graph, bottoms, TARG)
    rels = rel.create_relation(graph, bottoms, TARG, delete_single=False)
    return model, graph, bottoms, rels


def _targ(graph):
    return [(k, m) for k, m in graph.items() if type(m) in TARG]


def _batch(name, seeds, device):
    """(nets, batch) after merge_batchnorm and layer equalisation"""
    nets = [_prepared(name, s, device) for s in seeds]
    batch = arena.NetworkBatch([(g, b, r) for (_, g, b, r) in nets], TARG)
    le = batch.le_plan()
    le.run()
    le.close()
    _ffi.synchronize()
    return nets, batch


def _weights(graph):
    """{key: float32 numpy [rows, row_len]}"""
    return OrderedDict((k, m.weight.detach().cpu().numpy().reshape(m.weight.shape[0], -1).copy()) for k, m in _targ(graph))


def _restore(nets, snaps):
    with torch.no_grad():
        for (_, g, _, _), snap in zip(nets, snaps):
            for k, m in _targ(g):
                m.weight.copy_(torch.from_numpy(snap[k]).view(m.weight.shape))


def _storage_bits(batch):
    return batch.storage.cpu().numpy().view(np.int32).copy()


_REFS = {}


def _ref(w, fmt, search):
    """the reference of one tensor, computed once per content"""
    key = (w.tobytes(), w.shape, fmt, search)
    if key not in _REFS:
        _REFS[key] = _mx_ref(w, fmt, search)
    return _REFS[key]


def _fmt_of(width, fp6='e2m3', fp8='e4m3'):
    return {4: 'e2m1', 6: fp6, 8: fp8}[width]


def _check_errors(got, w, fmts, search, what):
    for f, fmt in enumerate(fmts):
        ref = _ref(w, fmt, search)
        d = ref['stored'].astype(F64) - w.astype(F64)
        exact = math.fsum((d * d).reshape(-1).tolist())
        print(what, fmt, 'sum e^2', float(got[f]), 'exact', exact)
        assert abs(float(got[f]) - exact) <= w.size * 2.0 ** -53 * exact, '{} {}: {!r} against {!r}'.format(what, fmt, float(got[f]), exact)


def _check_quantised(plan, nets, snaps, width_of, search, what, fp6='e2m3', fp8='e4m3'):
    """codes, scale bytes and weights of every tensor against the reference at width_of(n, key)"""
    for n, (_, g, _, _) in enumerate(nets):
        codes, scales, now = plan.codes(n), plan.scales(n), _weights(g)
        for k, w in snaps[n].items():
            ref = _ref(w, _fmt_of(width_of(n, k), fp6, fp8), search)
            assert np.array_equal(scales[k].cpu().numpy(), ref['scales']), '{} net {} {}: scale bytes'.format(what, n, k)
            assert np.array_equal(codes[k].cpu().numpy().reshape(w.shape), ref['codes']), '{} net {} {}: codes'.format(what, n, k)
            assert np.array_equal(_bits(now[k]), _bits(ref['stored'])), '{} net {} {}: weights'.format(what, n, k)


# (fp6, fp8, search, the width to quantise at) per seed: every format and both rules over the three seeds
_CONFIGS = {0: ('e2m3', 'e4m3', True, 4), 1: ('e3m2', 'e5m2', False, 6), 2: ('e2m3', 'e5m2', True, 8)}


@pytest.mark.parametrize('seed', SEEDS)
@pytest.mark.parametrize('name', NAMES)
def test_mx_plan_on_the_batch(engine, name, seed):
    """one run of a whole plan (ERRORS, then QUANTISE): every tensor's errors, codes, scale bytes and weights against the
    reference, and the second network again as a batch of its own"""
    fp6, fp8, search, width = _CONFIGS[seed]
    seeds = [seed, seed + 3]
    nets, batch = _batch(name, seeds, engine.device)
    snaps = [_weights(g) for (_, g, _, _) in nets]
    plan = batch.mx_plan(widths=(4, 6, 8), bit_weight=width, fp6=fp6, fp8=fp8, search=search)
    assert plan.launches == 3 and plan.cost_block is plan.error_block
    plan.run()
    _ffi.synchronize()
    for n in range(len(seeds)):
        for k, e in plan.errors(n).items():
            _check_errors(e, snaps[n][k], ['e2m1', fp6, fp8], int(search), '{} net {} {}'.format(name, n, k))
    _check_quantised(plan, nets, snaps, lambda n, k: width, int(search), '{} width {}'.format(name, width), fp6, fp8)
    assert plan.status_block.cpu().tolist() == [0] * len(seeds)
    alone_nets, alone = _batch(name, seeds[1:], engine.device)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(_weights(alone_nets[0][1]).values(), snaps[1].values()))
    one = alone.mx_plan(widths=(4, 6, 8), bit_weight=width, fp6=fp6, fp8=fp8, search=search)
    one.run()
    _ffi.synchronize()
    assert torch.equal(one.error_block[0].view(torch.int64), plan.error_block[1].view(torch.int64)), 'errors depend on the batch'
    assert torch.equal(one.code_block[0], plan.code_block[1]) and torch.equal(one.scale_block[0], plan.scale_block[1])
    for a, b in zip(_weights(alone_nets[0][1]).values(), _weights(nets[1][1]).values()):
        assert np.array_equal(_bits(a), _bits(b)), 'the weights depend on the batch'
    one.close()
    plan.close()


def test_the_errors_stage_writes_nothing_else(engine):
    """apply=False: two launches, no weight, code or scale byte written, two runs bit-equal, a subset of the widths the same numbers"""
    nets, batch = _batch('tiny_cat', SEEDS[:2], engine.device)
    before = _storage_bits(batch)
    plan = batch.mx_plan(widths=(4, 6, 8), fp6='e3m2', search=True, apply=False)
    assert plan.launches == 2
    plan.code_block.fill_(0xA5)
    plan.scale_block.fill_(0xA5)
    plan.run()
    _ffi.synchronize()
    first = plan.error_block.clone()
    assert bool((first > 0).all())
    assert np.array_equal(_storage_bits(batch), before), 'the ERRORS stage wrote into the batch'
    assert bool((plan.code_block == 0xA5).all()) and bool((plan.scale_block == 0xA5).all()), 'the ERRORS stage wrote codes or scales'
    plan.error_block.zero_()
    plan.run(plan.ERRORS)
    _ffi.synchronize()
    assert torch.equal(first.view(torch.int64), plan.error_block.view(torch.int64)), 'two runs differ'
    plan.close()
    sub = batch.mx_plan(widths=(6,), fp6='e3m2', search=True, apply=False)
    sub.run()
    _ffi.synchronize()
    assert torch.equal(sub.error_block[:, :, 0].contiguous().view(torch.int64), first[:, :, 1].contiguous().view(torch.int64))
    sub.close()
    assert np.array_equal(_storage_bits(batch), before)


# ---- 5. device widths -----------------------------------------------------------------------------------------------------------------
def test_widths_read_on_the_device(engine):
    name, seeds = 'tiny_mobile', SEEDS[:2]
    nets, batch = _batch(name, seeds, engine.device)
    snaps = [_weights(g) for (_, g, _, _) in nets]
    plan = batch.mx_plan(widths=(4, 6, 8), bit_weight=8, search=True)
    T = plan.n_tensors
    assert T >= 3
    host = np.array([[(4, 6, 8)[(n + 2 * t) % 3] for t in range(T)] for n in range(len(seeds))], dtype=np.int32)
    block = torch.from_numpy(host).to(engine.device)
    plan.set_widths(block)
    plan.status_block.fill_(7)
    plan.run(plan.QUANTISE)
    _ffi.synchronize()
    assert plan.status_block.cpu().tolist() == [0, 0]
    at = {k: t for t, k in enumerate(plan.keys)}
    _check_quantised(plan, nets, snaps, lambda n, k: int(host[n, at[k]]), 1, 'mixed widths')
    assert len(set(host.reshape(-1).tolist())) == 3

    # a width that is no candidate: that (network, tensor) untouched, status 2, everything around it as before
    _restore(nets, snaps)
    bad_n, bad_t = 1, 2
    bad_key = plan.keys[bad_t]
    host2 = host.copy()
    host2[bad_n, bad_t] = 5
    block.copy_(torch.from_numpy(host2))
    plan.code_block.fill_(0xA5)
    plan.scale_block.fill_(0x5A)
    plan.run(plan.QUANTISE)
    _ffi.synchronize()
    assert plan.status_block.cpu().tolist() == [0, 2]
    assert np.array_equal(_bits(_weights(nets[bad_n][1])[bad_key]), _bits(snaps[bad_n][bad_key])), 'the refused tensor was written'
    assert bool((plan.codes(bad_n)[bad_key] == 0xA5).all()) and bool((plan.scales(bad_n)[bad_key] == 0x5A).all())
    for n, (_, g, _, _) in enumerate(nets):
        codes, scales, now = plan.codes(n), plan.scales(n), _weights(g)
        for k, w in snaps[n].items():
            if (n, k) == (bad_n, bad_key):
                continue
            ref = _ref(w, _fmt_of(int(host2[n, at[k]])), 1)
            assert np.array_equal(codes[k].cpu().numpy().reshape(w.shape), ref['codes']) and np.array_equal(scales[k].cpu().numpy(), ref['scales'])
            assert np.array_equal(_bits(now[k]), _bits(ref['stored']))
    # the padding between the tensors' codes and scales keeps the fill
    used_c = np.zeros(plan.code_block.shape[1], dtype=bool)
    for (_, off, numel, _) in plan._code_views:
        used_c[off:off + numel] = True
    used_s = np.zeros(plan.scale_block.shape[1], dtype=bool)
    for (_, off, n_blk, _) in plan._scale_views:
        used_s[off:off + n_blk] = True
    assert (plan.code_block.cpu().numpy()[:, ~used_c] == 0xA5).all() and (plan.scale_block.cpu().numpy()[:, ~used_s] == 0x5A).all()

    # None: the table's width again, and status is not touched
    _restore(nets, snaps)
    plan.set_widths(None)
    plan.status_block.fill_(7)
    plan.run(plan.QUANTISE)
    _ffi.synchronize()
    assert plan.status_block.cpu().tolist() == [7, 7]
    _check_quantised(plan, nets, snaps, lambda n, k: 8, 1, 'after set_widths(None)')
    with pytest.raises(ValueError):
        plan.set_widths(block.to(torch.int64))
    plan.close()


def test_decode_widths_on_the_device_and_the_gate(engine):
    """dfq_batch_mx_decode_plan through the C ABI: a device width that is none of 4, 6, 8 leaves that (network, tensor) untouched
    and sets status 2; a network whose gate word is not 0 is left untouched, status included"""
    lib, dev = _ffi.lib(), engine.device
    gen = np.random.default_rng(9)
    shapes, n_nets, fill = [(3, 40), (2, 9)], 2, F32(7.5)
    host_w = np.array([[4, 5], [6, 8]], dtype=np.int32)
    fmt_at = lambda n, t: _fmt_of(int(host_w[n, t]) if host_w[n, t] != 5 else 4, 'e3m2', 'e5m2')
    refs = [[_mx_ref((gen.standard_normal(sh) * 3).astype(F32), fmt_at(n, t), 1) for t, sh in enumerate(shapes)] for n in range(n_nets)]
    w_off, c_off, s_off = [4, 132], [1, 131], [3, 17]
    w_stride, c_stride, s_stride = 160, 160, 32
    codes = np.full((n_nets, c_stride), 0x11, dtype=np.uint8)
    scales = np.full((n_nets, s_stride), 0x7f, dtype=np.uint8)
    for n in range(n_nets):
        for t, (rows, row_len) in enumerate(shapes):
            codes[n, c_off[t]:c_off[t] + rows * row_len] = refs[n][t]['codes'].reshape(-1)
            scales[n, s_off[t]:s_off[t] + refs[n][t]['scales'].size] = refs[n][t]['scales'].reshape(-1)
    code_dev, scale_dev = torch.from_numpy(codes).to(dev), torch.from_numpy(scales).to(dev)
    wdev = torch.from_numpy(host_w).to(dev)
    D = _ffi.DfqBatchMxDecodeTensor

    def run(gate_words):
        store = torch.full((n_nets, w_stride), float(fill), dtype=torch.float32, device=dev)
        status = torch.full((n_nets,), 7, dtype=torch.int32, device=dev)
        gate = torch.tensor(gate_words, dtype=torch.int32, device=dev)
        bases = (ctypes.c_void_p * n_nets)(*[store.data_ptr() + 4 * n * w_stride for n in range(n_nets)])
        arr = (D * 2)(*[D(store.data_ptr() + 4 * w_off[t], rows, row_len, c_off[t], s_off[t], 0, t) for t, (rows, row_len) in enumerate(shapes)])
        plan = ctypes.c_void_p()
        assert lib.dfq_batch_mx_decode_plan_create(arr, 2, bases, n_nets, code_dev.data_ptr(), c_stride, scale_dev.data_ptr(), s_stride,
                                                   wdev.data_ptr(), 2, _ffi.MX_E3M2, _ffi.MX_E5M2, gate.data_ptr(), status.data_ptr(),
                                                   ctypes.byref(plan)) == 0
        assert lib.dfq_batch_mx_decode_plan_run(plan, _ffi.stream_arg()) == 0
        _ffi.synchronize()
        lib.dfq_batch_mx_decode_plan_destroy(plan)
        return store.cpu().numpy(), status.cpu().tolist()

    def check(store, written):
        want = np.full((n_nets, w_stride), fill, dtype=F32)
        for (n, t) in written:
            rows, row_len = shapes[t]
            want[n, w_off[t]:w_off[t] + rows * row_len] = refs[n][t]['stored'].reshape(-1)
        assert np.array_equal(_bits(store), _bits(want))

    store, status = run([0, 0])
    assert status == [2, 0]
    check(store, [(0, 0), (1, 0), (1, 1)])                  # (0, 1) holds the width 5: untouched, like everything between the tensors
    store, status = run([0, 3])
    assert status == [2, 0]                                 # (cleared by the run; the gated network stores nothing, no status either)
    check(store, [(0, 0)])
    store, status = run([1, 0])
    assert status == [0, 0]
    check(store, [(1, 0), (1, 1)])


def test_errors_of_a_tensor_that_is_not_finite(engine):
    """the ERRORS stage on a batch: a tensor holding a NaN or an Inf has NaN errors at every format, every other tensor of every
    network the errors it had"""
    nets, batch = _batch('tiny_cat', SEEDS[:2], engine.device)
    plan = batch.mx_plan(widths=(4, 6, 8), search=True, apply=False)
    plan.run()
    _ffi.synchronize()
    clean = plan.error_block.clone()
    assert bool(torch.isfinite(clean).all())
    keys = plan.keys
    hit = {(0, 0): float('nan'), (1, len(keys) - 1): float('-inf'), (1, 1): float('inf')}
    with torch.no_grad():
        for (n, t), v in hit.items():
            w = nets[n][1][keys[t]].weight
            w.view(-1)[w.numel() // 2] = v
    plan.run()
    _ffi.synchronize()
    got = plan.error_block.cpu()
    for n in range(2):
        for t in range(len(keys)):
            if (n, t) in hit:
                assert bool(torch.isnan(got[n, t]).all()), (n, t)
            else:
                assert torch.equal(got[n, t].view(torch.int64), clean[n, t].cpu().view(torch.int64)), (n, t)
    plan.close()


# ---- 6. allocation ------------------------------------------------------------------------------------------------------------------------
def _alloc_ref(errors, sizes, widths, sens, fixed, budget):
    """the greedy walk of dfq_batch_mixed_plan_create (include/dfq_hip.h) as tests/test_batch_mixed.py restates it, on errors
    [T][B] (Python floats); fixed[t]: a width or 0.  Returns the widths."""
    T, B = len(sizes), len(widths)
    c = [[float(sens[t]) * float(errors[t][j]) for j in range(B)] for t in range(T)]
    at = [widths.index(fixed[t]) if fixed[t] else 0 for t in range(T)]
    used = sum(sizes[t] * widths[at[t]] for t in range(T))

    def step(t):
        j, best, kb = at[t], 0.0, -1
        for k in range(j + 1, B):
            g = (c[t][j] - c[t][k]) / float(sizes[t] * (widths[k] - widths[j]))
            if g > 0.0 and g >= best:
                best, kb = g, k
        return best, kb

    nxt = [(0.0, -1) if fixed[t] else step(t) for t in range(T)]
    while True:
        best, bt = 0.0, -1
        for t in range(T):
            if nxt[t][1] >= 0 and nxt[t][0] > best:
                best, bt = nxt[t][0], t
        if bt < 0:
            break
        k = nxt[bt][1]
        d = sizes[bt] * (widths[k] - widths[at[bt]])
        if used + d > budget:
            break
        at[bt] = k
        used += d
        nxt[bt] = step(bt)
    return [widths[j] for j in at], used


@pytest.mark.parametrize('name', NAMES)
def test_quantize_mx_allocates_on_its_own_errors(engine, name):
    nets, batch = _batch(name, SEEDS[:2], engine.device)
    snaps = [_weights(g) for (_, g, _, _) in nets]
    widths = (4, 6, 8)
    keys = list(snaps[0])
    sizes = [snaps[0][k].size for k in keys]
    pin = {keys[1]: 8}
    sens = {keys[0]: 3.0}
    codes, scales, bits, errors = batch.quantize_mx(widths, avg_bits=5, pin=pin, sensitivity=sens, search=True)
    budget = math.floor(5 * sum(sizes))
    seen = set()
    for n in range(2):
        for k in keys:
            _check_errors(errors[n][k], snaps[n][k], ['e2m1', 'e2m3', 'e4m3'], 1, '{} net {} {}'.format(name, n, k))
        want, used = _alloc_ref([errors[n][k].tolist() for k in keys], sizes, list(widths), [sens.get(k, 1.0) for k in keys],
                                [pin.get(k, 0) for k in keys], budget)
        assert [bits[n][k] for k in keys] == want and used <= budget, '{} net {}'.format(name, n)
        seen |= set(want)
        now = _weights(nets[n][1])
        for k in keys:
            ref = _ref(snaps[n][k], _fmt_of(bits[n][k]), 1)
            assert np.array_equal(codes[n][k].cpu().numpy().reshape(ref['codes'].shape), ref['codes']), k
            assert np.array_equal(scales[n][k].cpu().numpy(), ref['scales']) and np.array_equal(_bits(now[k]), _bits(ref['stored'])), k
    assert len(seen) >= 2, 'one width for everything: the test shows nothing'
    # one width, and no budget: the plan at that width
    _restore(nets, snaps)
    codes, scales, bits, errors = batch.quantize_mx((6,), avg_bits=5, fp6='e3m2')
    assert all(b == 6 for b in bits[0].values()) and all(e.shape == (1,) for e in errors[0].values())
    for k in keys:
        assert np.array_equal(codes[1][k].cpu().numpy().reshape(snaps[1][k].shape), _ref(snaps[1][k], 'e3m2', 1)['codes']), k


def test_mixed_plan_with_other_costs_is_unchanged(engine):
    """mixed_plan(costs=nsr) and costs=None give what they give on their own; costs=mx allocates on the MX errors"""
    name, seeds, widths = 'tiny_res', SEEDS[:2], (4, 6, 8)
    nets, batch = _batch(name, seeds, engine.device)
    mx = batch.mx_plan(widths=widths, apply=False)
    mx.run()
    nsr = batch.nsr_plan(widths)
    nsr.run()
    plain = batch.mixed_plan(widths, avg_bits=5, apply=False)
    plain.run()
    with_nsr = batch.mixed_plan(widths, avg_bits=5, apply=False, costs=nsr)
    with_nsr.run()
    with_mx = batch.mixed_plan(widths, avg_bits=5, apply=False, costs=mx)
    with_mx.run()
    _ffi.synchronize()
    # the plain plan's result is the restated walk on ITS errors, the nsr one's on the nsr costs: neither saw the mx plan
    keys = list(plain.keys)
    w0 = _weights(nets[0][1])
    assert keys == list(w0) == mx.keys
    sizes = [w0[k].size for k in keys]
    for n in range(len(seeds)):
        for plan, cost in ((plain, plain.error_block), (with_nsr, nsr.cost_block), (with_mx, mx.error_block)):
            want, _ = _alloc_ref(cost[n].cpu().numpy().tolist(), sizes, list(widths), [1.0] * len(keys), [0] * len(keys), plain.budget)
            assert [plan.bits(n)[k] for k in keys] == want
        assert torch.equal(plain.error_block.view(torch.int64), with_nsr.error_block.view(torch.int64))
        assert torch.equal(plain.error_block.view(torch.int64), with_mx.error_block.view(torch.int64))
    # a second plain plan and a second nsr plan made after the mx ones: bit-equal blocks
    again = batch.mixed_plan(widths, avg_bits=5, apply=False)
    again.run()
    again_nsr = batch.mixed_plan(widths, avg_bits=5, apply=False, costs=nsr)
    again_nsr.run()
    _ffi.synchronize()
    for a, b in ((plain, again), (with_nsr, again_nsr)):
        assert torch.equal(a.bits_block, b.bits_block) and torch.equal(a.used_block, b.used_block)
        assert torch.equal(a.cost_block.view(torch.int64), b.cost_block.view(torch.int64))
    with pytest.raises(ValueError):
        batch.mixed_plan((2, 4, 8), avg_bits=5, apply=False, costs=mx)
    with pytest.raises(ValueError):
        batch.mixed_plan(widths, avg_bits=5, apply=False, costs=plain)
    for p in (mx, nsr, plain, with_nsr, with_mx, again, again_nsr):
        p.close()


# ---- 7. pack, unpack, files ---------------------------------------------------------------------------------------------------------------
def _extent(n, b):
    words = -(-n * b // 32)
    return -(-words // 4) * 4


def _pack_ref(u, b):
    """uint32 [extent]: the words of one tensor's stream of unsigned codes (tests/test_batch_pack.py's restatement)"""
    u = (np.asarray(u, dtype=np.int64).reshape(-1) & ((1 << b) - 1)).astype(np.uint64)
    words = np.zeros(_extent(u.size, b), dtype=np.uint64)
    bit = np.arange(u.size, dtype=np.int64) * b
    w, s = bit >> 5, (bit & 31).astype(np.uint64)
    v = u << s
    np.bitwise_or.at(words, w, v & np.uint64(0xffffffff))
    spill = (v >> np.uint64(32)) != 0
    np.bitwise_or.at(words, w[spill] + 1, v[spill] >> np.uint64(32))
    return words.astype(np.uint32)


def _overwrite(nets, value=0.25):
    with torch.no_grad():
        for (_, g, _, _) in nets:
            for _, m in _targ(g):
                m.weight.fill_(value)


def _assert_weight_bits(nets, snaps, what):
    for n, (_, g, _, _) in enumerate(nets):
        for k, w in _weights(g).items():
            assert np.array_equal(_bits(w), _bits(snaps[n][k])), '{} net {} {}'.format(what, n, k)


@pytest.mark.parametrize('layered', [False, True])
def test_pack_unpack_and_files(engine, layered, tmp_path):
    name, seeds = 'tiny_mobile', SEEDS[:2]
    nets, batch = _batch(name, seeds, engine.device)
    with torch.no_grad():                                   # zeros of both signs and values that round to zero: the sign lives in the code
        w0 = _targ(nets[0][1])[0][1].weight
        w0.view(-1)[0:4] = torch.tensor([0.0, -0.0, -1e-30, 1e-30], device=w0.device)
    mx = batch.mx_plan(widths=(4, 6, 8), bit_weight=6, fp6='e3m2', fp8='e5m2', search=True)
    T = mx.n_tensors
    host = None
    if layered:
        host = np.array([[(8, 4, 6)[(n + t) % 3] for t in range(T)] for n in range(len(seeds))], dtype=np.int32)
        mx.set_widths(torch.from_numpy(host).to(engine.device))
    mx.run()
    pack = batch.pack_plan(mx)
    assert pack.launches == 2
    pack.run()
    _ffi.synchronize()
    assert mx.status_block.cpu().tolist() == [0, 0] and pack.status_block.cpu().tolist() == [0, 0]
    widths = pack.widths_array()
    assert np.array_equal(widths, host if layered else np.full((len(seeds), T), 6))
    for n in range(len(seeds)):
        codes, got = mx.codes(n), pack.words(n)
        for t, k in enumerate(pack.keys):
            want = _pack_ref(codes[k].cpu().numpy(), int(widths[n, t]))
            assert np.array_equal(got[k].cpu().numpy().view(np.uint32), want), 'net {} {}'.format(n, k)
    snaps = [_weights(g) for (_, g, _, _) in nets]
    first = snaps[0][pack.keys[0]].reshape(-1)
    assert _bits(first[1:3]).tolist() == [_bits(F32(-0.0))] * 2 and _bits(first[0:4:3]).tolist() == [0, 0]
    _overwrite(nets)
    un = batch.unpack_plan(pack, weights=True)
    assert un.launches == 2
    un.run()
    _ffi.synchronize()
    assert [un.status(n) for n in range(len(seeds))] == [0, 0]
    _assert_weight_bits(nets, snaps, 'unpacked')
    for n in range(len(seeds)):
        for k, c in mx.codes(n).items():
            assert torch.equal(un.codes(n)[k].cpu(), c.cpu()), k
    un.close()
    with pytest.raises(ValueError):
        batch.unpack_plan(pack, weights=True, codes='int32')
    # a network the unpack launch skips (its offsets do not start at 0) is not decoded: its weights stay as they were
    _overwrite(nets, 0.5)
    kept = pack.offset_block[1, 0].clone()
    pack.offset_block[1, 0] = 4
    un = batch.unpack_plan(pack, weights=True)
    un.run()
    _ffi.synchronize()
    pack.offset_block[1, 0] = kept
    assert un.statuses() == [0, 1] and un.status(1) == 1
    _assert_weight_bits(nets[:1], snaps[:1], 'the network beside a skipped one')
    assert all(bool((m.weight == 0.5).all()) for _, m in _targ(nets[1][1])), 'a skipped network was decoded'
    un.close()
    _restore(nets, snaps)

    # the file, into a fresh batch of other weights
    path = str(tmp_path / 'mx.npz')
    saved_plan = batch.save_packed(path, mx)
    with np.load(path, allow_pickle=False) as f:
        saved = {k: f[k] for k in f.files}
    assert int(saved['version']) == 2 and int(saved['mx_block']) == 32 and 'ranges' not in saved
    assert (int(saved['mx_format6']), int(saved['mx_format8'])) == (2, 4)
    assert np.array_equal(saved['widths'], widths) and np.array_equal(saved['offsets'], saved_plan.offset_block.cpu().numpy())
    want_scales = np.concatenate([np.stack([mx.scales(n)[k].cpu().numpy().reshape(-1) for n in range(len(seeds))]) for k in mx.keys], axis=1)
    assert np.array_equal(saved['mx_scales'], want_scales)
    nets2, batch2 = _batch(name, [5, 6], engine.device)
    loaded = batch2.load_packed(path)
    assert isinstance(loaded, arena.PackedBatch) and loaded.mx is not None and loaded.keys == pack.keys
    _assert_weight_bits(nets2, snaps, 'loaded')
    for wrong in (1, 3):                                    # an MX file under another version: refused, nothing read
        saved['version'] = np.int64(wrong)
        bumped = str(tmp_path / 'bumped.npz')
        np.savez(bumped, **saved)
        with pytest.raises(ValueError):
            batch2.load_packed(bumped)
    saved['version'] = np.int64(2)
    for gone in ('mx_scales', 'mx_format6', 'mx_block'):
        cut = str(tmp_path / 'cut.npz')
        np.savez(cut, **{k: v for k, v in saved.items() if k != gone})
        with pytest.raises(ValueError):
            batch2.load_packed(cut)
    saved['mx_block'] = np.int64(16)
    np.savez(str(tmp_path / 'block.npz'), **saved)
    with pytest.raises(ValueError):
        batch2.load_packed(str(tmp_path / 'block.npz'))
    _assert_weight_bits(nets2, snaps, 'after the refusals')
    mx.close()

    # a file of an integer source: version 1 and the keys it always had
    if not layered:
        q = batch.quant_plan(bit_weight=4, bits_bias=32, codes='int8')
        q.run()
        plain = str(tmp_path / 'plain.npz')
        batch.save_packed(plain, q)
        q.close()
        with np.load(plain, allow_pickle=False) as f:
            assert int(f['version']) == 1
            assert sorted(f.files) == sorted(['version', 'keys', 'offsets', 'widths', 'per_channel', 'signed', 'shapes', 'ranges', 'bias_keys',
                                              'biases'] + ['words_{}'.format(n) for n in range(len(seeds))])


# ---- 8. argument errors through the C ABI -------------------------------------------------------------------------------------------------
def test_abi_rejects_bad_arguments(engine):
    lib, dev = _ffi.lib(), engine.device
    buf = torch.zeros(4096, dtype=torch.float32, device=dev)
    errors = torch.zeros(64, dtype=torch.float64, device=dev)
    codes = torch.zeros(4096, dtype=torch.uint8, device=dev)
    scales = torch.zeros(256, dtype=torch.uint8, device=dev)
    wblock = torch.full((2, 2), 4, dtype=torch.int32, device=dev)
    status = torch.zeros(2, dtype=torch.int32, device=dev)
    T, C, D = _ffi.DfqBatchMxTensor, _ffi.DfqBatchMxConfig, _ffi.DfqBatchMxDecodeTensor
    p0 = buf.data_ptr()

    def bases(*ptrs):
        return (ctypes.c_void_p * len(ptrs))(*ptrs)

    def cfg(widths=(4, 6, 8), f6=1, f8=3, search=1, apply=1, bits=4):
        return C((ctypes.c_int32 * 3)(*(list(widths) + [0] * (3 - len(widths)))), len(widths), f6, f8, search, apply, bits, 0)

    def create(tensors, config, base=None, n_nets=1, err=errors, code=codes, code_stride=2048, scale=scales, scale_stride=128, n=None):
        plan = ctypes.c_void_p()
        arr = (T * max(1, len(tensors)))(*tensors) if tensors is not None else None
        rc = lib.dfq_batch_mx_plan_create(arr, len(tensors) if n is None and tensors is not None else (n or 0),
                                          None if config is None else ctypes.byref(config), bases(p0) if base is None else base, n_nets,
                                          None if err is None else err.data_ptr(), None if code is None else code.data_ptr(), code_stride,
                                          None if scale is None else scale.data_ptr(), scale_stride, ctypes.byref(plan))
        if rc == 0:
            lib.dfq_batch_mx_plan_destroy(plan)
        return rc

    def refused(rc, what):
        assert rc == DFQ_ERR_ARG, what
        assert b'dfq_' in lib.dfq_last_error(), what

    ok = T(p0, 4, 40, 0, 0)
    assert create([ok], cfg()) == 0
    refused(create(None, cfg()), 'null table')
    refused(create([ok], cfg(), n=0), 'empty table')
    refused(create([ok], None), 'null configuration')
    for widths in ((), (4, 4), (6, 4), (4, 5), (2, 4, 8), (8, 6, 4)):
        refused(create([ok], cfg(widths, bits=4)), 'widths {!r}'.format(widths))
    for f6, f8 in ((0, 3), (3, 3), (1, 1), (1, 5), (-1, 3)):
        refused(create([ok], cfg(f6=f6, f8=f8)), 'formats {} {}'.format(f6, f8))
    refused(create([ok], cfg((4, 8), bits=6)), 'apply at a width that is no candidate')
    assert create([ok], cfg((4, 8), bits=6, apply=0)) == 0
    for rows, row_len in ((0, 40), (4, 0), (-1, 40), (1, 1 << 31)):
        refused(create([T(p0, rows, row_len, 0, 0)], cfg()), 'geometry {} {}'.format(rows, row_len))
    refused(create([T(None, 4, 40, 0, 0)], cfg()), 'null weight')
    refused(create([T(p0 + 2, 4, 40, 0, 0)], cfg()), 'a weight off 4 bytes')
    refused(create([T(p0, 4, 40, 2048 - 159, 0)], cfg()), 'codes past the stride')
    assert create([T(p0, 4, 40, 2048 - 160, 0)], cfg()) == 0
    refused(create([T(p0, 4, 40, 0, 128 - 7)], cfg()), 'scales past the stride')
    assert create([T(p0, 4, 40, 0, 128 - 8)], cfg()) == 0
    refused(create([T(p0, 4, 40, -2, 0)], cfg()), 'negative offset')
    refused(create([ok], cfg(), err=None), 'null errors block')
    refused(create([ok], cfg(), code=None), 'null code block')
    refused(create([ok], cfg(), scale=None), 'null scale block')
    assert create([T(p0, 4, 40, -1, -1)], cfg(), code=None, scale=None) == 0
    refused(create([ok], cfg(), base=None, n_nets=0), 'no networks')
    refused(create([ok], cfg(), base=bases(p0, None), n_nets=2), 'null base')
    refused(create([ok], cfg(), base=bases(p0, p0 + 8), n_nets=2), 'a network off 16 bytes')
    assert create([ok], cfg(), base=bases(p0, p0 + 4096), n_nets=2) == 0

    # run_stages and set_widths
    plan = ctypes.c_void_p()
    arr = (T * 2)(ok, T(p0 + 4 * 256, 2, 9, 256, 16))
    assert lib.dfq_batch_mx_plan_create(arr, 2, ctypes.byref(cfg()), bases(p0, p0 + 8192), 2, errors.data_ptr(), codes.data_ptr(), 2048,
                                        scales.data_ptr(), 128, ctypes.byref(plan)) == 0
    assert lib.dfq_batch_mx_plan_launches(plan) == 3
    for stages in (0, 4, 7, -1):
        refused(lib.dfq_batch_mx_plan_run_stages(plan, stages, None), 'stages {}'.format(stages))
    refused(lib.dfq_batch_mx_plan_run_stages(None, 1, None), 'null plan')
    refused(lib.dfq_batch_mx_plan_run(None, None), 'null plan')
    idx = (ctypes.c_int32 * 2)(0, 1)
    refused(lib.dfq_batch_mx_plan_set_widths(None, wblock.data_ptr(), 2, idx, status.data_ptr()), 'null plan')
    refused(lib.dfq_batch_mx_plan_set_widths(plan, wblock.data_ptr(), 2, None, status.data_ptr()), 'no index')
    refused(lib.dfq_batch_mx_plan_set_widths(plan, wblock.data_ptr(), 2, idx, None), 'no status')
    refused(lib.dfq_batch_mx_plan_set_widths(plan, wblock.data_ptr(), 1, idx, status.data_ptr()), 'index past the stride')
    refused(lib.dfq_batch_mx_plan_set_widths(plan, wblock.data_ptr(), 2, (ctypes.c_int32 * 2)(0, -1), status.data_ptr()), 'negative index')
    assert lib.dfq_batch_mx_plan_set_widths(plan, wblock.data_ptr(), 2, idx, status.data_ptr()) == 0
    assert lib.dfq_batch_mx_plan_set_widths(plan, None, 0, None, None) == 0
    lib.dfq_batch_mx_plan_destroy(plan)
    assert lib.dfq_batch_mx_plan_launches(None) == 0

    # dfq_mx_rows
    def rows(x=p0, r=4, n=40, fmt=0):
        return lib.dfq_mx_rows(x, p0, r, n, fmt, 1, codes.data_ptr(), scales.data_ptr(), None, None)
    refused(rows(x=None), 'null x')
    refused(rows(r=0), 'no rows')
    refused(rows(n=0), 'empty rows')
    refused(rows(n=1 << 31), 'row_len above 2^31 - 1')
    refused(rows(fmt=5), 'unknown format')
    refused(rows(fmt=-1), 'unknown format')

    # the decode plan
    def decode(tensors, base=None, n_nets=1, code=codes, scale=scales, code_stride=2048, scale_stride=128, widths=wblock, wstride=2, f6=1, f8=3,
               st=status, n=None, gate=None):
        plan = ctypes.c_void_p()
        arr = (D * max(1, len(tensors)))(*tensors) if tensors is not None else None
        rc = lib.dfq_batch_mx_decode_plan_create(arr, len(tensors) if n is None and tensors is not None else (n or 0),
                                                 bases(p0) if base is None else base, n_nets, None if code is None else code.data_ptr(),
                                                 code_stride, None if scale is None else scale.data_ptr(), scale_stride,
                                                 None if widths is None else widths.data_ptr(), wstride, f6, f8,
                                                 None if gate is None else gate.data_ptr(), None if st is None else st.data_ptr(),
                                                 ctypes.byref(plan))
        if rc == 0:
            assert lib.dfq_batch_mx_decode_plan_launches(plan) == 1
            lib.dfq_batch_mx_decode_plan_destroy(plan)
        return rc

    dok = D(p0, 4, 40, 0, 0, 6, 0)
    assert decode([dok]) == 0 and decode([dok], widths=None, st=None) == 0 and decode([dok], gate=status) == 0
    refused(decode(None), 'null table')
    refused(decode([dok], n=0), 'empty table')
    refused(decode([dok], code=None), 'null codes')
    refused(decode([dok], scale=None), 'null scales')
    for bits in (5, 2, 16, -4):
        refused(decode([D(p0, 4, 40, 0, 0, bits, 0)]), 'num_bits {}'.format(bits))
    assert decode([D(p0, 4, 40, 0, 0, 0, 1)]) == 0
    refused(decode([D(p0, 4, 40, 0, 0, 0, 1)], widths=None), 'device widths without a width block')
    refused(decode([D(p0, 4, 40, 0, 0, 0, 1)], st=None), 'device widths without a status block')
    refused(decode([D(p0, 4, 40, 0, 0, 0, 2)]), 'width_index past the stride')
    refused(decode([D(p0, 4, 40, 0, 0, 0, -1)]), 'negative width_index')
    refused(decode([dok], f6=3), 'format6')
    refused(decode([dok], f8=1), 'format8')
    refused(decode([D(p0, 0, 40, 0, 0, 6, 0)]), 'no rows')
    refused(decode([D(p0, 4, 1 << 31, 0, 0, 6, 0)]), 'row_len above 2^31 - 1')
    refused(decode([D(None, 4, 40, 0, 0, 6, 0)]), 'null weight')
    refused(decode([D(p0 + 1, 4, 40, 0, 0, 6, 0)]), 'a weight off 4 bytes')
    refused(decode([D(p0, 4, 40, 2048 - 159, 0, 6, 0)]), 'codes past the stride')
    refused(decode([D(p0, 4, 40, 0, 121, 6, 0)]), 'scales past the stride')
    refused(decode([D(p0, 4, 40, -1, 0, 6, 0)]), 'negative offset')
    refused(decode([dok], base=bases(p0, p0 + 4), n_nets=2), 'a network off 16 bytes')
    refused(lib.dfq_batch_mx_decode_plan_run(None, None), 'null plan')


def test_python_refusals(engine):
    nets, batch = _batch('tiny_cat', SEEDS[:1], engine.device)
    for kw in (dict(widths=(4, 5)), dict(widths=(8, 4)), dict(widths=()), dict(widths=4), dict(fp6='e4m3'), dict(fp8='e2m3'),
               dict(bit_weight=5), dict(widths=(4, 8), bit_weight=6), dict(bit_weight=True)):
        with pytest.raises(ValueError):
            batch.mx_plan(**kw)
    with pytest.raises(ValueError):
        prims.mx_rows(torch.zeros(2, 8), 'e1m2')
    mx = batch.mx_plan(codes=False)
    with pytest.raises(ValueError):
        batch.pack_plan(mx)                                 # no codes to pack
    with pytest.raises(ValueError):
        mx.set_widths('mixed')
    other = batch.mixed_plan((2, 4, 8), avg_bits=5, apply=False)
    with pytest.raises(ValueError):
        mx.set_widths(other)                                # 2 is no MX width
    other.close()
    mx.close()
    with pytest.raises(RuntimeError):
        mx.run()
    with pytest.raises(RuntimeError):
        mx.set_widths(None)


def test_struct_layout_matches_header():
    import subprocess
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = r'''
    #include <stdio.h>
    #include "dfq_hip.h"
    int main(void) {
        printf("%zu %zu %zu %d %d %d\n", sizeof(dfq_batch_mx_tensor), sizeof(dfq_batch_mx_config), sizeof(dfq_batch_mx_decode_tensor),
               DFQ_MX_E2M1 + 10 * DFQ_MX_E2M3 + 100 * DFQ_MX_E3M2 + 1000 * DFQ_MX_E4M3 + 10000 * DFQ_MX_E5M2, DFQ_MX_BLOCK,
               DFQ_MX_ERRORS + 10 * DFQ_MX_QUANTISE);
        return 0;
    }'''
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, 't.c')
        open(c, 'w').write(src)
        exe = os.path.join(d, 't')
        subprocess.run(['gcc', '-I', os.path.join(root, 'include'), c, '-o', exe], check=True)
        got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    want = [ctypes.sizeof(t) for t in (_ffi.DfqBatchMxTensor, _ffi.DfqBatchMxConfig, _ffi.DfqBatchMxDecodeTensor)]
    want += [_ffi.MX_E2M1 + 10 * _ffi.MX_E2M3 + 100 * _ffi.MX_E3M2 + 1000 * _ffi.MX_E4M3 + 10000 * _ffi.MX_E5M2, _ffi.MX_BLOCK,
             _ffi.MX_ERRORS + 10 * _ffi.MX_QUANTISE]
    assert got == want
