"""NetworkBatch.clip_plan / clip_weight_mse / dfq.clip_weight_mse / dfq_batch_clip_plan_*: the MSE-optimal clipping range of
every weight (per tensor or per output row) of every network of a batch, and the clamp to it.

The reference is numpy, in this file, by the definition in include/dfq_hip.h: the shrink factors and candidate ends in
float64 (Python floats, the operations in the order the header writes them), the quantiser recipe of
tests/test_batch_error.py (``_qparams`` with an explicit (l, h), five separately rounded float32 operations per element) on
the weight clamped to (l, h), minus the weight as it is -- under the asymmetric recipe the quantiser's own saturation
already does what the clamp does, bit for bit (asserted), under the symmetric one it does not at the shorter end -- and
err_k = ``math.fsum`` of the float64 squares of the float32 errors, which is exact up to the final rounding.  The plan adds
the same n terms in float64 in an order of its own, so |got - exact| <= n u err_k with u = 2^-53 (Higham (4.4), as
test_batch_error.py argues it; every term is >= 0, so sum|term| is the sum).  Nothing looser anywhere.  The choice k* is
compared exactly except for units whose two smallest reference errors are closer than four times the largest bound of the
unit: there a different summation order may legitimately draw the other one; at most 1 % of a case's units, asserted."""
import ctypes
import math
import os
import subprocess
import tempfile
from collections import OrderedDict

import numpy as np
import pytest
import torch

from dfq_amd import _ffi, arena, dfq, synthetic
from dfq_amd.utils import layer_transform as lt
from dfq_amd.utils import relation as rel

from common import TARG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DFQ_ERR_ARG = -1     # include/dfq_hip.h
F32 = np.float32
U = 2.0 ** -53
K, ALPHA_MIN = 16, 0.25
CONFIGS = [(4, False, False), (8, False, False), (4, True, True), (6, True, False)]      # (bit_weight, per_channel, signed)
NAMES = ['tiny_mobile', 'tiny_res', 'tiny_cat']


# ---- the definition in numpy ---------------------------------------------------------------------------------------------
def _qparams(mn, mx, bits, signed):
    """utils/quantize.py:49-66 with Python floats: (qmin, qmax, -min, scale, min) as float32 (tests/test_batch_error.py)"""
    mn, mx = float(mn), float(mx)
    if signed:
        qmin, qmax = -float(1 << (bits - 1)), float((1 << (bits - 1)) - 1)
        mx, mn = abs(mx), abs(mn)
        if mx < mn:
            mx = mn
        scale, mn = mx / qmax, 0.0
    else:
        qmin, qmax = 0.0, float(1 << bits) - 1.0
        scale = (mx - mn) / (qmax - qmin)
    if 1e-8 > scale:
        scale = 1e-8
    with np.errstate(all='ignore'):
        return F32(qmin), F32(qmax), F32(-mn), F32(scale), F32(mn)


def _epsilon(w, prm, w_in=None):
    """Q(w_in) - w, float32, for w [units, n] and one parameter tuple per unit (w_in: what is quantised, default w)"""
    w_in = w if w_in is None else w_in
    qmin, qmax = prm[0][0], prm[0][1]
    neg_min, scale, min_value = (np.array([p[i] for p in prm], dtype=F32).reshape(-1, 1) for i in (2, 3, 4))
    with np.errstate(all='ignore'):
        q = w_in + neg_min
        q = q / scale
        q = np.where(q < qmin, qmin, q)
        q = np.where(q > qmax, qmax, q)
        q = np.rint(q)
        y = q * scale
        y = y + min_value
        e = y - w
    assert e.dtype == F32
    return e


def _alphas(k_cand, alpha_min):
    return [1.0 if k_cand == 1 else 1.0 - k * (1.0 - alpha_min) / (k_cand - 1) for k in range(k_cand)]


def _unit_range(x):
    """(mn, mx) of a unit by the house rule: NaN skipped, nothing but NaN gives (NaN, NaN)"""
    ok = ~np.isnan(x)
    return (F32(x[ok].min()), F32(x[ok].max())) if ok.any() else (F32(np.nan), F32(np.nan))


def _candidate(mn, mx, alpha):
    a, b = float(mn), float(mx)
    if math.isnan(a):
        return F32(np.nan), F32(np.nan)
    z = a if a > 0.0 else 0.0          # max(0, mn)
    z = z if z < b else b              # min(., mx)
    with np.errstate(all='ignore'):
        return F32(z + alpha * (a - z)), F32(z + alpha * (b - z))


def _fsum(row):
    vals = row.tolist()
    if any(math.isnan(v) for v in vals):
        return math.nan
    return math.fsum(vals)             # (every term is >= 0: an infinity among them gives inf)


class Ref:
    """cand float32 [units, K, 2], err float64 [units, K] (exact), bound [units, K], chosen [units], ambiguous [units];
    e = Q(clamp(w, l_k, h_k)) - w: what quant_plan stores for the clamped weight, minus the original"""

    def __init__(self, w, bits, signed, k_cand=K, alpha_min=ALPHA_MIN):
        assert w.dtype == F32 and w.ndim == 2
        units, n = w.shape
        al = _alphas(k_cand, alpha_min)
        rng = [_unit_range(r) for r in w]
        self.cand = np.empty((units, k_cand, 2), dtype=F32)
        self.err = np.empty((units, k_cand), dtype=np.float64)
        self.clamp_matters = np.zeros(units, dtype=bool)                # the clamp changed an e the quantiser's saturation would not
        for k in range(k_cand):
            ends = [_candidate(mn, mx, al[k]) for mn, mx in rng]
            self.cand[:, k, :] = np.array(ends, dtype=F32).reshape(units, 2)
            prm = [_qparams(l, h, bits, signed) for l, h in ends]
            lo, hi = self.cand[:, k, 0:1], self.cand[:, k, 1:2]
            with np.errstate(invalid='ignore'):
                clamped = np.where(w < lo, lo, np.where(w > hi, hi, w))       # the definition's clamp: NaN and -0.0 pass
            e = _epsilon(w, prm, clamped)
            plain = _epsilon(w, prm)                                    # the quantiser's own saturation alone
            self.clamp_matters |= ~((e.view(np.int32) == plain.view(np.int32)) | (np.isnan(e) & np.isnan(plain))).all(axis=1)
            d = e.astype(np.float64)
            self.err[:, k] = [_fsum(r) for r in d * d]
        for u, (mn, mx) in enumerate(rng):                          # candidate 0 is exactly (mn, mx)
            assert np.array_equal(self.cand[u, 0].view(np.int32), np.array([mn, mx], dtype=F32).view(np.int32)) or math.isnan(mn)
        with np.errstate(all='ignore'):
            self.bound = n * U * self.err
        self.chosen = np.zeros(units, dtype=np.int32)
        self.ambiguous = np.zeros(units, dtype=bool)
        for u in range(units):
            best, ks = self.err[u, 0], 0
            for k in range(1, k_cand):
                if self.err[u, k] < best:
                    best, ks = self.err[u, k], k
            self.chosen[u] = ks
            e = self.err[u]
            if np.isfinite(e).all() and k_cand > 1:
                two = np.sort(e)[:2]
                self.ambiguous[u] = two[1] - two[0] <= 4.0 * self.bound[u].max()


def _check_unit_errors(got, ref, what):
    """got float64 [units, K] against the exact sums, each within its bound"""
    assert got.shape == ref.err.shape, what
    for u in range(got.shape[0]):
        for k in range(got.shape[1]):
            g, exact = float(got[u, k]), float(ref.err[u, k])
            if math.isnan(exact):
                assert math.isnan(g), '{} unit {} candidate {}: {} for NaN'.format(what, u, k, g)
            elif math.isinf(exact):
                assert g == exact, '{} unit {} candidate {}: {} for inf'.format(what, u, k, g)
            else:
                assert abs(g - exact) <= ref.bound[u, k], '{} unit {} candidate {}: {!r} against {!r}, off by {:.3e} > {:.3e}'.format(
                    what, u, k, g, exact, abs(g - exact), ref.bound[u, k])


def _check_choice(chosen, ranges, ref, what):
    """k* against the reference's argmin (ambiguous units apart), the range bit for bit the candidate's; returns the number
    of units left out of the k comparison"""
    chosen, ranges = np.asarray(chosen).reshape(-1), np.asarray(ranges, dtype=F32).reshape(-1, 2)
    assert chosen.shape == ref.chosen.shape, what
    skipped = 0
    for u in range(len(chosen)):
        k = int(chosen[u])
        assert 0 <= k < ref.cand.shape[1], '{} unit {}: k* = {}'.format(what, u, k)
        if ref.ambiguous[u] and k != ref.chosen[u]:
            skipped += 1
        else:
            assert k == ref.chosen[u], '{} unit {}: k* = {} against {} (errors {!r})'.format(what, u, k, ref.chosen[u], ref.err[u].tolist())
        want = ref.cand[u, k]
        same = (ranges[u].view(np.int32) == want.view(np.int32)) | (np.isnan(ranges[u]) & np.isnan(want))
        assert same.all(), '{} unit {}: range {!r} against {!r}'.format(what, u, ranges[u].tolist(), want.tolist())
    return skipped


# ---- helpers -------------------------------------------------------------------------------------------------------------
def _prepared(name, seed, device):
    model, graph, bottoms = synthetic.build(name, seed=seed)
    model.to(device)
    lt.merge_batchnorm(model, graph, bottoms, TARG)
    return model, graph, bottoms, rel.create_relation(graph, bottoms, TARG, delete_single=False)


def _batch(name, seeds, engine):
    nets = [_prepared(name, s, engine.device)[1:] for s in seeds]
    return nets, arena.NetworkBatch(nets, TARG)


def _weights(graph):
    """{key: float32 [rows, row_len] host copy} of the targ_type weights"""
    return OrderedDict((k, m.weight.detach().cpu().numpy().reshape(m.weight.shape[0], -1).copy()) for k, m in graph.items() if type(m) in TARG)


def _units(w, per_channel):
    return w if per_channel else w.reshape(1, -1)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int64 if t.dtype is torch.float64 else torch.int32)


_REFS = {}


def _net_refs(name, seeds, config, nets):
    """the reference of every weight of every network of a case, computed once and shared by the engines (the weights of a
    seed are the same on both)"""
    key = (name, tuple(seeds), config)
    if key not in _REFS:
        bits, per_channel, signed = config
        _REFS[key] = [OrderedDict((k, (w, Ref(_units(w, per_channel), bits, signed))) for k, w in _weights(g).items()) for g, _, _ in nets]
    return _REFS[key]


# ---- 1. / 2. errors and choice -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('config', CONFIGS)
@pytest.mark.parametrize('name', NAMES)
def test_errors_and_choice(engine, name, config):
    bits, per_channel, signed = config
    nets, batch = _batch(name, [0, 1, 2], engine)
    refs = _net_refs(name, [0, 1, 2], config, nets)
    before = batch.storage.clone()
    plan = batch.clip_plan(bits, per_channel, signed, candidates=K, alpha_min=ALPHA_MIN, apply=False, keep_errors=True)
    assert 1 <= plan.launches <= 4
    assert (plan.n_nets, plan.candidates, plan.alpha_min, plan.apply) == (3, K, ALPHA_MIN, False)
    plan.run()
    _ffi.synchronize()
    assert torch.equal(_bits(batch.storage), _bits(before)), 'apply=False wrote into the batch allocation'
    units = skipped = 0
    for n in range(3):
        rng, cho, err = plan.ranges(n), plan.chosen(n), plan.errors(n)
        assert list(rng.keys()) == list(refs[n].keys()) == plan.keys
        for k, (w, ref) in refs[n].items():
            what = '{} {} net {} {}'.format(name, config, n, k)
            assert tuple(rng[k].shape) == ((w.shape[0], 2) if per_channel else (2,))
            assert tuple(cho[k].shape) == ((w.shape[0],) if per_channel else ())
            assert tuple(err[k].shape) == ((w.shape[0], K) if per_channel else (K,))
            _check_unit_errors(err[k].cpu().numpy().reshape(-1, K), ref, what)
            skipped += _check_choice(cho[k].cpu().numpy(), rng[k].cpu().numpy(), ref, what)
            units += len(ref.chosen)
            if not signed:
                assert not ref.clamp_matters.any(), what + ': the clamp changed an error the asymmetric saturation leaves alone'
    assert skipped <= 0.01 * units, '{} of {} units left out of the k comparison'.format(skipped, units)
    assert not torch.equal(plan.chosen_block[0], plan.chosen_block[1]) or not torch.equal(_bits(plan.range_block[0]), _bits(plan.range_block[1]))
    first = [b.clone() for b in (plan.range_block, plan.chosen_block, plan.error_block)]
    plan.run()
    _ffi.synchronize()
    for a, b in zip(first, (plan.range_block, plan.chosen_block, plan.error_block)):
        assert torch.equal(_bits(a), _bits(b)), 'two runs differ'
    plan.close()
    with pytest.raises(RuntimeError, match='closed'):
        plan.run()


def test_network_does_not_depend_on_the_batch(engine):
    _, three = _batch('tiny_mobile', [0, 1, 2], engine)
    _, one = _batch('tiny_mobile', [1], engine)
    for config in CONFIGS[:1] + CONFIGS[2:3]:
        p3 = three.clip_plan(*config, candidates=K, alpha_min=ALPHA_MIN, apply=False, keep_errors=True)
        p1 = one.clip_plan(*config, candidates=K, alpha_min=ALPHA_MIN, apply=False, keep_errors=True)
        for p in (p3, p1):
            p.run()
        _ffi.synchronize()
        for b3, b1 in ((p3.range_block, p1.range_block), (p3.chosen_block, p1.chosen_block), (p3.error_block, p1.error_block)):
            assert torch.equal(_bits(b3[1]), _bits(b1[0]))
            assert not torch.equal(_bits(b3[0]), _bits(b1[0]))
        p3.close()
        p1.close()


# ---- 3. apply ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('config', CONFIGS)
def test_apply(engine, config):
    """The weights after ``apply`` are the clamp of the originals to the chosen ranges, every unit's (min, max) is then that
    range, a quant_plan behind it reports it, and sum e^2 of the quantised result against the ORIGINAL weights is no larger
    than under min/max quantisation of the originals: err_k is the error of exactly that result, and candidate 0 is the
    min/max range."""
    bits, per_channel, signed = config
    nets, batch = _batch('tiny_mobile', [0, 1, 2], engine)
    refs = _net_refs('tiny_mobile', [0, 1, 2], config, nets)
    plan = batch.clip_plan(bits, per_channel, signed, candidates=K, alpha_min=ALPHA_MIN, apply=True, keep_errors=True)
    plan.run()
    _ffi.synchronize()
    rngs = [OrderedDict((k, v.cpu().numpy().reshape(-1, 2)) for k, v in plan.ranges(n).items()) for n in range(3)]
    chos = [OrderedDict((k, v.cpu().numpy().reshape(-1)) for k, v in plan.chosen(n).items()) for n in range(3)]
    plan.close()
    moved = 0
    for n, (g, _, _) in enumerate(nets):
        for k, w in _weights(g).items():
            w0, ref = refs[n][k]
            what = '{} net {} {}'.format(config, n, k)
            _check_choice(chos[n][k], rngs[n][k], ref, what)
            moved += int((chos[n][k] != 0).sum())
            got, orig = _units(w, per_channel), _units(w0, per_channel)
            l, h = rngs[n][k][:, 0:1], rngs[n][k][:, 1:2]
            assert np.array_equal(got.view(np.int32), np.clip(orig, l, h).view(np.int32)), what + ': not np.clip(w0, l, h)'
            assert np.array_equal(got.min(axis=1).view(np.int32), l[:, 0].view(np.int32)), what + ': min is not l'
            assert np.array_equal(got.max(axis=1).view(np.int32), h[:, 0].view(np.int32)), what + ': max is not h'
    assert moved > 0 or bits > 4, 'the search moved no range at {} bits: the case tests nothing'.format(bits)
    # a quant_plan behind it reports exactly these ranges, and its result is no further from the ORIGINAL weights than the
    # min/max quantisation of the originals (candidate 0), up to the two summation bounds
    qp = batch.quant_plan(bits, 32, per_channel, signed, codes=None)
    qp.run()
    _ffi.synchronize()
    qr = [OrderedDict((k, v.cpu().numpy().reshape(-1, 2)) for k, v in qp.ranges(n).items()) for n in range(3)]
    qp.close()
    units, worse, worst = 0, [], 1.0
    for n, (g, _, _) in enumerate(nets):
        for k, wq in _weights(g).items():
            w0, ref = refs[n][k]
            what = '{} net {} {}'.format(config, n, k)
            assert np.array_equal(qr[n][k].view(np.int32), rngs[n][k].view(np.int32)), what + ': quant_plan saw another range'
            d = (_units(wq, per_channel) - _units(w0, per_channel)).astype(np.float64)
            for u, row in enumerate(d * d):
                new, old = _fsum(row), float(ref.err[u, 0])
                units += 1
                if not new <= old + row.size * U * (new + old):
                    worse.append('{} unit {}: sum e^2 {!r} after the clamp > {!r} under min/max'.format(what, u, new, old))
                    worst = max(worst, new / old)
    print('{}: {} of {} units further from the originals than their min/max quantisation, worst ratio {:.3f}'.format(
        config, len(worse), units, worst))
    assert not worse, '{} of {} units, worst ratio {:.3f}; the first: {}'.format(len(worse), units, worst, worse[0])


# ---- 4. shapes through the C ABI ------------------------------------------------------------------------------------------
ROW_LENS = [1, 9, 16, 17, 27, 33, 64, 65, 128, 129, 1536, 1537, 4100]
ROW_COUNTS = [1, 5, 67]
ROW_SHAPES = [(r, n) for n in ROW_LENS for r in ROW_COUNTS]
TENSOR_SHAPES = [(1, 1536), (1, 1537), (4, 1024), (1, 4097), (1, 2 * 4096 + 3)]       # per tensor: 1536, 1537, 4096, 4097, 8195 elements


def _layout(shapes):
    offs, total = [], 0
    for j, (r, n) in enumerate(shapes):
        offs.append(total)
        total += -(-(r * n) // 4) * 4 + 4 * (j % 3)                   # 16-byte aligned, with gaps of 0, 4 or 8 floats
    return offs, total + 8


_DATA = {}


def _data(shapes, seed):
    key = (tuple(shapes), seed)
    if key not in _DATA:
        gen = np.random.default_rng(seed)
        xs = []
        for j, (r, n) in enumerate(shapes):
            x = (gen.standard_normal((r, n)) * (1 + j % 3)).astype(F32)
            if r * n > 8:
                x.reshape(-1)[gen.integers(0, r * n, size=1 + r * n // 50)] *= 6.0      # outliers: the search has something to clip
            xs.append(x)
        _DATA[key] = xs
    return _DATA[key]


def _abi_run(engine, shapes, seeds, per_row, bits, signed, k_cand, alpha_min, apply, with_errors=True, runs=1):
    """the plan over len(seeds) networks of `shapes` (network k: _data(shapes, seeds[k])) -> (ranges, chosen, errors, weights,
    launches) as numpy [n_nets, ...]; unit offsets leave one unit between the tensors"""
    lib = _ffi.lib()
    n_nets = len(seeds)
    offs, stride = _layout(shapes)
    host = np.full((n_nets, stride), 7.5e5, dtype=F32)              # a gap that leaks into a unit shows in its range
    for k, seed in enumerate(seeds):
        for x, o in zip(_data(shapes, seed), offs):
            host[k, o:o + x.size] = x.reshape(-1)
    store = torch.from_numpy(host.copy()).to(engine.device).contiguous()
    uoffs, units = [], 1
    for r, n in shapes:
        uoffs.append(units)
        units += (r if per_row else 1) + 1
    rng = torch.full((n_nets, units, 2), 9.0, dtype=torch.float32, device=engine.device)
    cho = torch.full((n_nets, units), -7, dtype=torch.int32, device=engine.device)
    err = torch.full((n_nets, units, k_cand), 9.0, dtype=torch.float64, device=engine.device)
    base0 = store.data_ptr()
    T = _ffi.DfqBatchClipTensor
    tabs = (T * len(shapes))(*[T(base0 + 4 * o, r, n, uo) for (r, n), o, uo in zip(shapes, offs, uoffs)])
    cfg = _ffi.DfqBatchClipConfig(bits, int(signed), int(per_row), k_cand, alpha_min, int(apply), 0)
    bases = (ctypes.c_void_p * n_nets)(*[base0 + 4 * k * stride for k in range(n_nets)])
    plan = ctypes.c_void_p()
    _ffi.check(lib.dfq_batch_clip_plan_create(tabs, len(shapes), ctypes.byref(cfg), bases, n_nets, rng.data_ptr(), cho.data_ptr(),
                                              err.data_ptr() if with_errors else None, units, ctypes.byref(plan)))
    try:
        launches = lib.dfq_batch_clip_plan_launches(plan)
        for i in range(runs):
            _ffi.check(lib.dfq_batch_clip_plan_run(plan, _ffi.stream_arg()))
            _ffi.synchronize()
            if i == 0:
                first = [t.clone() for t in (rng, cho, err, store)]
        for a, b in zip(first, (rng, cho, err, store)):
            assert torch.equal(_bits(a), _bits(b)), 'two runs differ'
    finally:
        lib.dfq_batch_clip_plan_destroy(plan)
    out = dict(ranges=rng.cpu().numpy(), chosen=cho.cpu().numpy(), errors=err.cpu().numpy(), store=store.cpu().numpy(), host=host,
               launches=launches, offs=offs, uoffs=uoffs, units=units)
    used = np.zeros(units, dtype=bool)
    for (r, n), uo in zip(shapes, uoffs):
        used[uo:uo + (r if per_row else 1)] = True
    assert (out['ranges'][:, ~used] == 9.0).all() and (out['chosen'][:, ~used] == -7).all() and (out['errors'][:, ~used] == 9.0).all(), \
        'something else in the blocks was touched'
    if not with_errors:
        assert (out['errors'] == 9.0).all()
    return out


_ABI_REFS = {}


def _abi_ref(shapes, seed, per_row, bits, signed, k_cand, alpha_min):
    key = (tuple(shapes), seed, per_row, bits, signed, k_cand, alpha_min)
    if key not in _ABI_REFS:
        _ABI_REFS[key] = [Ref(_units(x, per_row), bits, signed, k_cand, alpha_min) for x in _data(shapes, seed)]
    return _ABI_REFS[key]


def _check_abi(out, net, shapes, refs, per_row, k_cand, what):
    units = skipped = 0
    for j, ((r, n), uo, ref) in enumerate(zip(shapes, out['uoffs'], refs)):
        nu = r if per_row else 1
        w = '{} net {} shape {} x {}'.format(what, net, r, n)
        _check_unit_errors(out['errors'][net, uo:uo + nu], ref, w)
        skipped += _check_choice(out['chosen'][net, uo:uo + nu], out['ranges'][net, uo:uo + nu], ref, w)
        units += nu
    assert skipped <= 0.01 * units, '{}: {} of {} units left out of the k comparison'.format(what, skipped, units)


def _check_clamped(out, net, shapes, per_row, what):
    """the weights are the clamp of the originals to the reported ranges, and nothing between the tensors changed"""
    want = out['host'][net].copy()
    for (r, n), o, uo in zip(shapes, out['offs'], out['uoffs']):
        nu = r if per_row else 1
        x = want[o:o + r * n].reshape(nu, -1)
        l, h = out['ranges'][net, uo:uo + nu, 0:1], out['ranges'][net, uo:uo + nu, 1:2]
        with np.errstate(invalid='ignore'):
            x[...] = np.where(x < l, l, np.where(x > h, h, x))
    assert np.array_equal(out['store'][net].view(np.int32), want.view(np.int32)), what + ': the weights are not the clamp of the originals'


def _shape_case(engine, shapes, per_row, bits, signed, n_nets, seed, launches, what):
    """n_nets == 1: the search alone, twice (bit-equal runs, weights untouched), against the reference.  n_nets == 3, networks
    (seed, seed, seed + 1): search and clamp; network 0 against the reference, network 1 the same bits at another place,
    network 2 the bits it gets alone, every network's weights the clamp of its originals."""
    ref = _abi_ref(shapes, seed, per_row, bits, signed, K_SHAPES, ALPHA_MIN)
    if n_nets == 1:
        out = _abi_run(engine, shapes, [seed], per_row, bits, signed, K_SHAPES, ALPHA_MIN, apply=False, runs=2)
        assert out['launches'] == launches
        assert np.array_equal(out['store'].view(np.int32), out['host'].view(np.int32)), 'apply=False wrote into the weights'
        _check_abi(out, 0, shapes, ref, per_row, K_SHAPES, what)
        assert (out['chosen'][0] > 0).any(), 'the search moved no range: the case tests nothing'
        return
    out = _abi_run(engine, shapes, [seed, seed, seed + 1], per_row, bits, signed, K_SHAPES, ALPHA_MIN, apply=True)
    assert out['launches'] == launches + (1 if launches > 1 else 0)
    _check_abi(out, 0, shapes, ref, per_row, K_SHAPES, what)
    alone = _abi_run(engine, shapes, [seed + 1], per_row, bits, signed, K_SHAPES, ALPHA_MIN, apply=False)
    for name in ('ranges', 'chosen', 'errors'):
        a = out[name]
        assert np.array_equal(a[0].view(np.int32), a[1].view(np.int32)), name
        assert name != 'errors' or not np.array_equal(a[0].view(np.int32), a[2].view(np.int32)), name
        assert np.array_equal(a[2].view(np.int32), alone[name][0].view(np.int32)), name
    for net in range(3):
        _check_clamped(out, net, shapes, per_row, what)


K_SHAPES = 8
# the lane classes below 64 lanes (rows of <= 16, 32, 64, 128 elements; full and partial slots), the 64-lane class
# (129, 1536: every slot full), the looping wave (1537, 4100)
ROW_GROUPS = [[1, 9, 16, 17, 27, 33, 64, 65, 128], [129, 1536, 1537], [4100]]
assert sorted(n for g in ROW_GROUPS for n in g) == ROW_LENS


@pytest.mark.parametrize('group', [0, 1, 2])
@pytest.mark.parametrize('rows', ROW_COUNTS)
@pytest.mark.parametrize('n_nets', [1, 3])
def test_row_shapes_through_the_abi(engine, n_nets, rows, group):
    shapes = [(rows, n) for n in ROW_GROUPS[group]]
    _shape_case(engine, shapes, True, 4, False, n_nets, 5, 1, 'rows {} n_nets {}'.format(rows, n_nets))


@pytest.mark.parametrize('config', [(4, False), (5, True)])
@pytest.mark.parametrize('n_nets', [1, 3])
def test_tensor_shapes_through_the_abi(engine, n_nets, config):
    """per tensor: 1536 elements (in registers), 1537, 4096, 4097 and 2 * 4096 + 3 (flat pieces: one, one full, two, three
    with a tail of single floats)"""
    bits, signed = config
    _shape_case(engine, TENSOR_SHAPES, False, bits, signed, n_nets, 7, 4, 'per tensor {} n_nets {}'.format(config, n_nets))


K_SHAPES_ROW = [(5, 9), (3, 27), (2, 65), (2, 129), (1, 1536), (1, 1537)]
K_SHAPES_TENSOR = [(1, 1536), (1, 4097)]


@pytest.mark.parametrize('per_row', [True, False])
@pytest.mark.parametrize('k_cand', [1, 64])
def test_one_and_sixty_four_candidates(engine, k_cand, per_row):
    shapes = K_SHAPES_ROW if per_row else K_SHAPES_TENSOR
    what = 'K {} per_row {}'.format(k_cand, per_row)
    out = _abi_run(engine, shapes, [9], per_row, 4, False, k_cand, 0.5, apply=True)
    _check_abi(out, 0, shapes, _abi_ref(shapes, 9, per_row, 4, False, k_cand, 0.5), per_row, k_cand, what)
    _check_clamped(out, 0, shapes, per_row, what)
    if k_cand == 1:                                                    # the identity: k* = 0, nothing stored
        used = out['chosen'][0] != -7
        assert (out['chosen'][0][used] == 0).all()
        assert np.array_equal(out['store'].view(np.int32), out['host'].view(np.int32))
    else:
        assert (out['chosen'][0] > 0).any()


# ---- 5. special values -----------------------------------------------------------------------------------------------------
def _snan():
    return np.array([0x7fa00001], dtype=np.uint32).view(F32)[0]


SPECIALS = ['zero', 'constant', 'positive', 'negative', 'qnan', 'snan', 'all_nan', 'inf']
# one geometry per path: a small lane class, the 64-lane class, the looping wave, flat pieces (a unit per tensor)
SPECIAL_GEOMETRY = [('rows of 20', True, [(6, 20)]), ('rows of 200', True, [(4, 200)]), ('rows of 1600', True, [(3, 1600)]),
                    ('tensors of 5000', False, [(1, 5000)] * 3)]


def _plant(x, kind):
    """x: one unit, a float32 vector (a view)"""
    if kind == 'zero':
        x[:] = 0.0
    elif kind == 'constant':
        x[:] = 0.375
    elif kind == 'positive':
        x[:] = np.abs(x) + F32(0.25)
        x[3 % x.size] = 40.0
    elif kind == 'negative':
        x[:] = -np.abs(x) - F32(0.25)
        x[3 % x.size] = -40.0
    elif kind == 'qnan':
        x[x.size // 2] = np.nan
    elif kind == 'snan':
        x[x.size // 2] = _snan()
    elif kind == 'all_nan':
        x[:] = np.nan
    elif kind == 'inf':
        x[x.size - 1] = np.inf


@pytest.mark.parametrize('geometry', SPECIAL_GEOMETRY, ids=[g[0] for g in SPECIAL_GEOMETRY])
@pytest.mark.parametrize('kind', SPECIALS)
def test_special_values(engine, kind, geometry):
    _, per_row, shapes = geometry
    clean = _abi_run(engine, shapes, [11], per_row, 4, False, K, ALPHA_MIN, apply=True)
    key = (tuple(shapes), 11)
    kept = _DATA[key]
    try:
        xs = [x.copy() for x in kept]
        target = xs[0][1] if per_row else xs[1].reshape(-1)            # unit 1 of the case
        _plant(target, kind)
        assert xs[0].dtype == F32
        _DATA[key] = xs
        out = _abi_run(engine, shapes, [11], per_row, 4, False, K, ALPHA_MIN, apply=True)
    finally:
        _DATA[key] = kept
    refs = [Ref(_units(x, per_row), 4, False) for x in xs]
    what = '{} in {}'.format(kind, geometry[0])
    _check_abi(out, 0, shapes, refs, per_row, K, what)
    _check_clamped(out, 0, shapes, per_row, what)
    uo = out['uoffs'][0] + 1 if per_row else out['uoffs'][1]
    l, h = out['ranges'][0, uo]
    k, errs = int(out['chosen'][0, uo]), out['errors'][0, uo]
    o = out['offs'][0] + shapes[0][1] if per_row else out['offs'][1]
    mine = slice(o, o + target.size)
    if kind == 'zero':
        assert k == 0 and (l, h) == (0.0, 0.0) and (errs == 0.0).all()
    elif kind == 'constant':
        assert (l, h) == (F32(0.375), F32(0.375)) and k == 0
    elif kind in ('positive', 'negative'):
        assert l <= h and (l > 0 if kind == 'positive' else h < 0)
        assert (out['ranges'][0, uo, 0] <= out['ranges'][0, uo, 1])
    else:                                                              # NaN or inf in the unit: its errors are NaN, k* = 0, nothing stored
        assert k == 0 and np.isnan(errs).all()
        assert np.array_equal(out['store'][0, mine].view(np.int32), out['host'][0, mine].view(np.int32)), 'the unit was written'
        if kind == 'all_nan':
            assert np.isnan(l) and np.isnan(h)
        else:
            ok = ~np.isnan(target)
            assert (l, h) == (target[ok].min(), target[ok].max())     # NaN skipped
    # every other unit: what the clean run gave, weights included
    for name in ('ranges', 'chosen', 'errors'):
        a, b = out[name][0].copy(), clean[name][0].copy()
        a[uo], b[uo] = 0, 0
        assert np.array_equal(a.view(np.int32), b.view(np.int32)), '{}: {} of another unit changed'.format(what, name)
    a, b = out['store'][0].copy(), clean['store'][0].copy()
    a[mine], b[mine] = 0, 0
    assert np.array_equal(a.view(np.int32), b.view(np.int32)), what + ': the weights of another unit changed'


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------
def test_abi_rejects_bad_arguments(engine):
    lib = _ffi.lib()
    buf = torch.zeros(1024, dtype=torch.float32, device=engine.device)
    rng = torch.zeros(2 * 16 * 2, dtype=torch.float32, device=engine.device)
    cho = torch.zeros(2 * 16, dtype=torch.int32, device=engine.device)
    err = torch.zeros(2 * 16 * 64, dtype=torch.float64, device=engine.device)
    p0 = buf.data_ptr()
    bases = (ctypes.c_void_p * 2)(p0, p0 + 4 * 512)
    T, C = _ffi.DfqBatchClipTensor, _ffi.DfqBatchClipConfig

    def create(data=p0, rows=8, row_len=9, out_off=0, bits=8, sym=0, per_row=1, k=32, alpha=0.5, apply=1, b=bases, n_nets=2,
               r=rng.data_ptr(), c=cho.data_ptr(), e=err.data_ptr(), stride=16, n_tensors=1, table=True, config=True, place=True):
        plan = ctypes.c_void_p()
        cf = C(bits, sym, per_row, k, alpha, apply, 0)
        rc = lib.dfq_batch_clip_plan_create((T * 1)(T(data, rows, row_len, out_off)) if table else None, n_tensors,
                                            ctypes.byref(cf) if config else None, b, n_nets, r, c, e, stride,
                                            ctypes.byref(plan) if place else None)
        n = lib.dfq_batch_clip_plan_launches(plan) if rc == 0 else None
        if rc == 0:
            lib.dfq_batch_clip_plan_destroy(plan)
        return rc, n
    assert create() == (0, 1)
    assert create(out_off=8) == (0, 1)                                # the last eight units of the stride
    assert create(per_row=0, out_off=15) == (0, 1)
    assert create(e=None) == (0, 1)
    assert create(bits=2, k=1, alpha=1.0) == (0, 1) and create(bits=16, k=64, alpha=1e-3, sym=1) == (0, 1)
    assert create(data=p0 + 16) == (0, 1)
    assert create(rows=1, row_len=400, per_row=0, apply=0) == (0, 1)
    bad = [dict(table=False), dict(n_tensors=0), dict(n_tensors=-1), dict(place=False), dict(config=False),
           dict(bits=1), dict(bits=17), dict(bits=0), dict(bits=-4), dict(k=0), dict(k=65), dict(k=-1),
           dict(alpha=0.0), dict(alpha=-0.5), dict(alpha=1.0000001), dict(alpha=math.nan), dict(alpha=math.inf),
           dict(data=None), dict(data=p0 + 4), dict(data=p0 + 8), dict(rows=0), dict(rows=-3), dict(row_len=0), dict(row_len=-1),
           dict(r=None), dict(c=None), dict(stride=0), dict(stride=-5), dict(stride=7), dict(out_off=-1), dict(out_off=9),
           dict(per_row=0, out_off=16), dict(out_off=1 << 40),
           dict(b=None), dict(n_nets=0), dict(n_nets=-1), dict(b=(ctypes.c_void_p * 2)(p0, None)),
           dict(b=(ctypes.c_void_p * 2)(p0, p0 + 4 * 511)), dict(rows=1 << 40, row_len=1 << 40)]
    for kw in bad:
        assert create(**kw)[0] == DFQ_ERR_ARG, kw
        assert b'dfq_batch_clip_plan_create' in lib.dfq_last_error(), kw
    assert lib.dfq_batch_clip_plan_run(None, None) == DFQ_ERR_ARG
    assert b'dfq_batch_clip_plan_run' in lib.dfq_last_error()
    assert lib.dfq_batch_clip_plan_launches(None) == 0
    lib.dfq_batch_clip_plan_destroy(None)


def test_refusals(engine):
    nets, batch = _batch('tiny_mobile', [0, 1], engine)
    for bad in (dict(bit_weight=True), dict(bit_weight=8.0), dict(bit_weight=1), dict(bit_weight=17), dict(bit_weight='8'),
                dict(candidates=0), dict(candidates=65), dict(candidates=8.0), dict(candidates=True), dict(candidates=None),
                dict(alpha_min=0), dict(alpha_min=0.0), dict(alpha_min=-0.1), dict(alpha_min=1.5), dict(alpha_min=math.nan),
                dict(alpha_min='0.5'), dict(alpha_min=None), dict(alpha_min=True)):
        with pytest.raises(ValueError):
            batch.clip_plan(**bad)
        with pytest.raises(ValueError):
            dfq.clip_weight_mse(nets[0][0], **{('bits_weight' if k == 'bit_weight' else k): v for k, v in bad.items()})
    with pytest.raises(ValueError):
        batch.clip_weight_mse(bit_weight=1)
    plan = batch.clip_plan(np.int64(8), candidates=np.int32(4), alpha_min=1)      # integers of numpy, alpha_min = 1: every candidate the same
    assert (plan.bit_weight, plan.candidates, plan.alpha_min) == (8, 4, 1.0)
    with pytest.raises(RuntimeError, match='keep_errors'):
        plan.errors(0)
    plan.close()
    # a weight that left its slot (not the first layer's: the batch's own quick check watches that one)
    g0 = nets[0][0]
    keys = [k for k in g0 if type(g0[k]) in TARG]
    layer = g0[keys[1]]
    kept = layer.weight.data
    layer.weight.data = kept.clone()
    with pytest.raises(RuntimeError, match='weight of {} '.format(keys[1])):
        batch.clip_plan()
    with pytest.raises(RuntimeError, match='weight of {} '.format(keys[1])):
        batch.clip_weight_mse()
    layer.weight.data = kept
    plan = batch.clip_plan()
    batch.release()
    with pytest.raises(RuntimeError, match='released'):
        plan.run()
    with pytest.raises(RuntimeError, match='released'):
        batch.clip_plan()
    plan.close()
    plan.close()


def test_unfolded_batch_is_refused(engine):
    nets = []
    for seed in (0, 1):
        model, graph, bottoms = synthetic.build('tiny_mobile', seed=seed)
        model.to(engine.device)
        nets.append((graph, bottoms, rel.create_relation(graph, bottoms, TARG, delete_single=False)))
    batch = arena.NetworkBatch.from_unfolded(nets, TARG)
    with pytest.raises(RuntimeError, match='not been folded'):
        batch.clip_plan()
    with pytest.raises(RuntimeError, match='not been folded'):
        batch.clip_weight_mse()


def test_struct_layout_matches_header():
    src = r'''
    #include <stdio.h>
    #include <stddef.h>
    #include "dfq_hip.h"
    int main(void) {
        printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(dfq_batch_clip_tensor), offsetof(dfq_batch_clip_tensor, data),
               offsetof(dfq_batch_clip_tensor, rows), offsetof(dfq_batch_clip_tensor, row_len), offsetof(dfq_batch_clip_tensor, out_offset),
               sizeof(dfq_batch_clip_config), offsetof(dfq_batch_clip_config, num_bits), offsetof(dfq_batch_clip_config, symmetric),
               offsetof(dfq_batch_clip_config, per_row), offsetof(dfq_batch_clip_config, candidates),
               offsetof(dfq_batch_clip_config, alpha_min), offsetof(dfq_batch_clip_config, apply), offsetof(dfq_batch_clip_config, pad));
        return 0;
    }'''
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, 't.c')
        open(c, 'w').write(src)
        exe = os.path.join(d, 't')
        subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), c, '-o', exe], check=True)
        got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    P, Q = _ffi.DfqBatchClipTensor, _ffi.DfqBatchClipConfig
    assert got == [ctypes.sizeof(P), P.data.offset, P.rows.offset, P.row_len.offset, P.out_offset.offset,
                   ctypes.sizeof(Q), Q.num_bits.offset, Q.symmetric.offset, Q.per_row.offset, Q.candidates.offset,
                   Q.alpha_min.offset, Q.apply.offset, Q.pad.offset]


# ---- 7. the single network -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('resident', [False, True], ids=['cpu_model', 'device_model'])
def test_single_network_equals_the_batch_of_one(engine, resident):
    config = (4, True, False)
    bits, per_channel, signed = config
    nets, batch = _batch('tiny_mobile', [1], engine)
    want = batch.clip_weight_mse(bits, per_channel, signed, candidates=K, alpha_min=ALPHA_MIN)[0]
    want_w = _weights(nets[0][0])
    model, graph, bottoms, _ = _prepared('tiny_mobile', 1, engine.device if resident else torch.device('cpu'))
    got = dfq.clip_weight_mse(graph, bits, per_channel, signed, candidates=K, alpha_min=ALPHA_MIN, targ_type=TARG)
    assert list(got.keys()) == list(want.keys())
    assert any((v['chosen'] != 0).any() for v in got.values())
    for k in want:
        assert sorted(got[k]) == ['chosen', 'err', 'err_minmax', 'range']
        for name in ('range', 'chosen', 'err_minmax', 'err'):
            a, b = np.asarray(got[k][name]), np.asarray(want[k][name])
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), '{} {}'.format(k, name)
        assert (got[k]['err'] <= got[k]['err_minmax']).all()
        assert np.array_equal(got[k]['err'] < got[k]['err_minmax'], got[k]['chosen'] != 0)
    for k, w in _weights(graph).items():
        assert graph[k].weight.device.type == ('cpu' if not resident else engine.device.type)
        assert np.array_equal(w.view(np.int32), want_w[k].view(np.int32)), k
    # the steps behind it complete and see the chosen ranges
    dfq.bias_correction(graph, bottoms, TARG, bits_weight=bits, per_channel=True)
    _, _, ranges = lt.quantize_targ_layer(graph, bits, 16, TARG, return_codes=True, per_channel=True)
    for k in want:
        assert np.array_equal(ranges[k].cpu().numpy().view(np.int32), want[k]['range'].view(np.int32)), k


def test_per_tensor_report(engine):
    nets, batch = _batch('tiny_res', [0, 1], engine)
    refs = _net_refs('tiny_res', [0, 1], (4, False, False), nets)
    rep = batch.clip_weight_mse(4, candidates=K, alpha_min=ALPHA_MIN)
    assert len(rep) == 2
    for n in range(2):
        for k, (w0, ref) in refs[n].items():
            r = rep[n][k]
            assert isinstance(r['chosen'], int) and isinstance(r['err'], float) and r['range'].shape == (2,)
            _check_choice([r['chosen']], r['range'], ref, k)
            assert abs(r['err_minmax'] - ref.err[0, 0]) <= ref.bound[0, 0] and abs(r['err'] - ref.err[0, r['chosen']]) <= ref.bound[0, r['chosen']]
            got = _weights(nets[n][0])[k]
            assert np.array_equal(got.view(np.int32), np.clip(w0, r['range'][0], r['range'][1]).view(np.int32))
