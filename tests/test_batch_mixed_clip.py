"""NetworkBatch.mixed_plan(clip=) / quantize_mixed(clip=) / dfq.quantize_mixed(clip=) and dfq_batch_mixed_plan_create_clipped /
dfq_batch_mixed_plan_run_stages: the MSE-optimal clip of every unit at every candidate width, the allocation on those errors,
and the clamp and the quantisation of every layer at its own width and at that width's own range.

Two references.  (a) ``clip_plan`` at each width, existing code with the same summation order: ``clip_chosen``, ``clip_ranges``
and ``unit_errors`` equal it BIT FOR BIT, every unit of every network, no ambiguous-unit allowance.  (b) numpy, by the
definition in include/dfq_hip.h: ``_qparams`` / ``_fake_quant`` as tests/test_batch_error.py and tests/test_batch_clip.py state
them, restated here; the error of a unit is ``math.fsum`` of the float64 squares of the float32 errors, exact up to its final
rounding, and the plan adds the same n non-negative terms in float64 in an order of its own, so |got - exact| <= n u err with
u = 2^-53 (Higham (4.4)); a per-row tensor's E is a running float64 sum of its rows' errors: |E - fsum| <= rows u E.  The
allocation is the greedy walk of include/dfq_hip.h restated in Python floats on the plan's own E, compared exactly."""
import ctypes
import math
import os
import subprocess
import tempfile
import types
from collections import OrderedDict

import numpy as np
import pytest
import torch

from dfq_amd import _ffi, arena, dfq, synthetic
from dfq_amd.utils import layer_transform as lt
from dfq_amd.utils import relation as rel

from common import TARG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DFQ_ERR_ARG, DFQ_ERR_STATE = -1, -3          # include/dfq_hip.h
ALLOCATE, CLAMP, QUANTISE = 1, 2, 4
F32 = np.float32
U = 2.0 ** -53
WIDTHS = (2, 3, 4, 6, 8)
K, ALPHA_MIN = 8, 0.25
NAMES = ['tiny_mobile', 'tiny_res', 'tiny_cat']
SEEDS = [0, 1, 2]
PAIRS = [(False, False), (True, True), (True, False)]        # (per_channel, signed)


# ---- the definition in numpy ---------------------------------------------------------------------------------------------
def _qparams(mn, mx, bits, signed):
    """utils/quantize.py:49-66 with Python floats: (qmin, qmax, -min, scale, min) as float32"""
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


def _fake_quant(w, prm):
    """utils/quantize.py:70-74: five separately rounded float32 operations; (dequantised, code)"""
    qmin, qmax, neg_min, scale, min_value = prm
    with np.errstate(all='ignore'):
        q = w + neg_min
        q = q / scale
        q = np.where(q < qmin, qmin, q)
        q = np.where(q > qmax, qmax, q)
        q = np.rint(q)
        y = q * scale
        y = y + min_value
    assert y.dtype == F32
    return y, q


def _alphas(k_cand, alpha_min):
    return [1.0 if k_cand == 1 else 1.0 - k * (1.0 - alpha_min) / (k_cand - 1) for k in range(k_cand)]


def _unit_range(x):
    ok = ~np.isnan(x)
    return (F32(x[ok].min()), F32(x[ok].max())) if ok.any() else (F32(np.nan), F32(np.nan))


def _candidate(mn, mx, alpha):
    a, b = float(mn), float(mx)
    if math.isnan(a):
        return F32(np.nan), F32(np.nan)
    z = a if a > 0.0 else 0.0
    z = z if z < b else b
    with np.errstate(all='ignore'):
        return F32(z + alpha * (a - z)), F32(z + alpha * (b - z))


def _clamp(x, l, h):
    with np.errstate(invalid='ignore'):
        return np.where(x < l, l, np.where(x > h, h, x)).astype(F32)


def _unit_error(x, l, h, bits, signed):
    """exact sum e^2 of one unit under the range (l, h): Q(clamp(x)) - x in float32, squares in float64, math.fsum"""
    y, _ = _fake_quant(_clamp(x, l, h), _qparams(l, h, bits, signed))
    with np.errstate(all='ignore'):
        d = (y - x).astype(np.float64)
        vals = (d * d).tolist()
    if any(math.isnan(v) for v in vals):
        return math.nan
    return math.fsum(vals)


def _same(a, b):
    """bit for bit, any NaN for any NaN"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != 'f':
        return bool(np.array_equal(a, b))
    iv = {4: np.int32, 8: np.int64}[a.dtype.itemsize]
    return bool(((a.view(iv) == b.view(iv)) | (np.isnan(a) & np.isnan(b))).all())


def _check_numpy(x_units, widths, signed, k_cand, alpha_min, chosen, ranges, errs, what):
    """units [u, n]; chosen [u, B], ranges [u, B, 2], errs [u, B] of the plan against the definition at the plan's own k*"""
    al = _alphas(k_cand, alpha_min)
    n = x_units.shape[1]
    for u, x in enumerate(x_units):
        mn, mx = _unit_range(x)
        for j, b in enumerate(widths):
            k = int(chosen[u, j])
            assert 0 <= k < k_cand, what
            l, h = _candidate(mn, mx, al[k])
            assert _same(np.array([l, h], dtype=F32), ranges[u, j]), '{} unit {} width {}: range {!r} against {!r}'.format(
                what, u, b, ranges[u, j].tolist(), [l, h])
            exact, g = _unit_error(x, l, h, b, signed), float(errs[u, j])
            if math.isnan(exact):
                assert math.isnan(g), '{} unit {} width {}: {} for NaN'.format(what, u, b, g)
            elif math.isinf(exact):
                assert g == exact, '{} unit {} width {}'.format(what, u, b)
            else:
                assert abs(g - exact) <= n * U * exact, '{} unit {} width {}: {!r} against {!r}'.format(what, u, b, g, exact)


def _alloc_ref(errors, sizes, widths, sens, fixed, budget):
    """the allocation of include/dfq_hip.h on errors [T][B] (Python floats); fixed[t]: a width or 0"""
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
    steps, ended_early = 0, False
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
            ended_early = True
            break
        at[bt] = k
        used += d
        steps += 1
        nxt[bt] = step(bt)
    cost = 0.0
    for t in range(T):
        cost += c[t][at[t]]
    return dict(bits=[widths[j] for j in at], used=used, steps=steps, cost=cost, ended_early=ended_early)


# ---- networks --------------------------------------------------------------------------------------------------------------
def _prepared(name, seed, device):
    model, graph, bottoms = synthetic.build(name, seed=seed)
    model.to(device)
    lt.merge_batchnorm(model, graph, bottoms, TARG)
    return model, graph, bottoms, rel.create_relation(graph, bottoms, TARG, delete_single=False)


def _batch(name, seeds, engine):
    nets = [_prepared(name, s, engine.device)[1:] for s in seeds]
    return nets, arena.NetworkBatch(nets, TARG)


def _targ(graph):
    return [(k, m) for k, m in graph.items() if type(m) in TARG]


def _weights(graph):
    return OrderedDict((k, m.weight.detach().cpu().numpy().reshape(m.weight.shape[0], -1).copy()) for k, m in _targ(graph))


def _biases(graph):
    return {k: m.bias.detach().cpu().numpy().copy() for k, m in _targ(graph) if m.bias is not None}


def _np(t):
    return t.detach().cpu().numpy()


def _state(nets):
    """every tensor of every network the plans may write: weights, biases and the BatchNorm proxies, in one float32 vector"""
    parts = []
    for net in nets:
        for key, m in net[0].items():
            for name in ('weight', 'bias', 'fake_weight', 'fake_bias'):
                t = getattr(m, name, None)
                if torch.is_tensor(t):
                    parts.append(_np(t).reshape(-1).astype(F32))
    return np.concatenate(parts)


def _clipped(batch, **kw):
    kw.setdefault('clip', K)
    kw.setdefault('alpha_min', ALPHA_MIN)
    return batch.mixed_plan(WIDTHS, **kw)


def _blocks(plan):
    return [t.clone() for t in (plan.bits_block, plan.error_block, plan.used_block, plan.cost_block, plan.range_block,
                                plan.clip_range_block, plan.clip_chosen_block, plan.unit_error_block)]


def _blocks_same(a, b):
    return all(_same(_np(x), _np(y)) for x, y in zip(a, b))


# ---- 1. / 2. against clip_plan, exactly, and against numpy -----------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
@pytest.mark.parametrize('pair', PAIRS)
def test_against_clip_plan_and_numpy(engine, name, pair):
    per_channel, signed = pair
    nets, batch = _batch(name, SEEDS, engine)
    _, twin = _batch(name, SEEDS, engine)
    before = batch.storage.clone()
    plan = _clipped(batch, avg_bits=4, per_channel=per_channel, signed=signed, apply=False)
    assert 3 <= plan.launches <= 8 and (plan.clip, plan.alpha_min) == (K, ALPHA_MIN)
    plan.run()
    _ffi.synchronize()
    assert _same(_np(batch.storage), _np(before)), 'apply=False wrote into the batch allocation'
    B = len(WIDTHS)
    cr, cc, ue = _np(plan.clip_range_block), _np(plan.clip_chosen_block), _np(plan.unit_error_block)
    assert cr.shape[2:] == (B, 2) and cc.shape[2] == B and ue.shape == cc.shape
    for j, b in enumerate(WIDTHS):
        ref = twin.clip_plan(b, per_channel, signed, candidates=K, alpha_min=ALPHA_MIN, apply=False, keep_errors=True)
        ref.run()
        _ffi.synchronize()
        rr, rc, re = _np(ref.range_block), _np(ref.chosen_block), _np(ref.error_block)
        ref.close()
        assert rc.shape == cc.shape[:2]
        assert _same(cc[:, :, j], rc), 'width {}: k* differs from clip_plan'.format(b)
        assert _same(cr[:, :, j], rr), 'width {}: the ranges differ from clip_plan'.format(b)
        at = np.take_along_axis(re, rc[:, :, None].astype(np.int64), axis=2)[:, :, 0]
        assert _same(ue[:, :, j], at), 'width {}: the unit errors differ from clip_plan'.format(b)
        with np.errstate(invalid='ignore'):
            assert (np.isnan(re[:, :, 0]) | (ue[:, :, j] <= re[:, :, 0])).all(), 'an error above that of the min/max range'
    assert (cc != 0).any(), 'no range was narrowed: the test shows nothing'
    for n, (g, _, _) in enumerate(nets):
        rng, cho, err, E = plan.clip_ranges(n), plan.clip_chosen(n), plan.unit_errors(n), plan.errors(n)
        assert list(rng) == list(E) == plan.keys
        for key, w in _weights(g).items():
            what = '{} {} net {} {}'.format(name, pair, n, key)
            rows = w.shape[0]
            assert tuple(rng[key].shape) == ((rows, B, 2) if per_channel else (B, 2))
            assert tuple(cho[key].shape) == tuple(err[key].shape) == ((rows, B) if per_channel else (B,))
            units = w if per_channel else w.reshape(1, -1)
            e = _np(err[key]).reshape(-1, B)
            if n == 0:                                  # (numpy: one network is enough, the others are clip_plan's bit for bit)
                _check_numpy(units, WIDTHS, signed, K, ALPHA_MIN, _np(cho[key]).reshape(-1, B), _np(rng[key]).reshape(-1, B, 2), e, what)
            for j in range(B):
                if per_channel:
                    exact = math.fsum(e[:, j].tolist())
                    assert abs(float(E[key][j]) - exact) <= rows * U * exact, what
                else:
                    assert _same(np.float64(E[key][j]), np.float64(e[0, j])), what
    plan.close()


# ---- 3. allocation ---------------------------------------------------------------------------------------------------------
def _check_alloc(plan, nets, n, sens=None, pin=None, costs=None):
    errs = plan.errors(n)
    keys = list(errs)
    sizes = [m.weight.numel() for _, m in _targ(nets[0][0])]
    table = [errs[k].tolist() for k in keys] if costs is None else costs[n].tolist()
    ref = _alloc_ref(table, sizes, plan.widths, [(sens or {}).get(k, 1.0) for k in keys], [(pin or {}).get(k, 0) for k in keys], plan.budget)
    bits = plan.bits(n)
    assert [bits[k] for k in keys] == ref['bits'], 'net {}: bits'.format(n)
    assert plan.used(n) == (ref['used'], ref['steps']), 'net {}: used / steps'.format(n)
    assert _same(np.float64(plan.cost(n)), np.float64(ref['cost'])), 'net {}: cost'.format(n)
    return ref


@pytest.mark.parametrize('pair', PAIRS)
def test_allocation_is_the_restated_walk(engine, pair):
    per_channel, signed = pair
    nets, batch = _batch('tiny_mobile', SEEDS, engine)
    keys = [k for k, _ in _targ(nets[0][0])]
    plan = _clipped(batch, avg_bits=3.5, per_channel=per_channel, signed=signed, apply=False)
    plan.run()
    _ffi.synchronize()
    refs = [_check_alloc(plan, nets, n) for n in range(3)]
    assert any(r['ended_early'] for r in refs), 'the budget never ended a walk'
    assert all(plan.used(n)[0] <= plan.budget for n in range(3))
    # costs from a device block: the walk goes on them, E is still reported
    E = plan.error_block.clone()
    gen = torch.Generator().manual_seed(5)
    costs = (torch.rand(E.shape, dtype=torch.float64, generator=gen) + 0.5).to(E.device) * E
    plan.set_costs(types.SimpleNamespace(cost_block=costs))
    plan.run()
    _ffi.synchronize()
    assert _same(_np(plan.error_block), _np(E))
    for n in range(3):
        _check_alloc(plan, nets, n, costs=_np(costs))
    plan.set_costs(None)
    plan.close()
    pin = {keys[0]: 8, keys[-1]: 3}
    sens = {keys[1]: 4.0}
    pinned = _clipped(batch, avg_bits=5, per_channel=per_channel, signed=signed, apply=False, pin=pin, sensitivity=sens)
    pinned.run()
    _ffi.synchronize()
    for n in range(3):
        _check_alloc(pinned, nets, n, sens=sens, pin=pin)
        assert pinned.bits(n)[keys[0]] == 8 and pinned.bits(n)[keys[-1]] == 3
    pinned.close()


# ---- 4. apply --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('codes', ['int32', 'int8'])
@pytest.mark.parametrize('pair', PAIRS)
def test_apply_is_clip_plan_then_quant_plan(engine, pair, codes):
    per_channel, signed = pair
    name = 'tiny_mobile'
    nets, batch = _batch(name, SEEDS, engine)
    alloc = _clipped(batch, avg_bits=4, per_channel=per_channel, signed=signed, apply=False)
    alloc.run()
    _ffi.synchronize()
    first = _blocks(alloc)
    alloc.close()
    plan = _clipped(batch, avg_bits=4, per_channel=per_channel, signed=signed, codes=codes)
    plan.run()
    _ffi.synchronize()
    assert _blocks_same(first, _blocks(plan)), 'apply changed the allocation or the search'
    bits = [plan.bits(n) for n in range(3)]
    occurring = sorted({b for d in bits for b in d.values()})
    assert len(occurring) >= 3, 'fewer than three widths occur: {}'.format(occurring)
    for b in occurring:
        tnets, twin = _batch(name, SEEDS, engine)
        cp = twin.clip_plan(b, per_channel, signed, candidates=K, alpha_min=ALPHA_MIN, apply=True)
        cp.run()
        qp = twin.quant_plan(b, 16, per_channel, signed, codes=codes)
        qp.run()
        _ffi.synchronize()
        for n in range(3):
            got_w, want_w = _weights(nets[n][0]), _weights(tnets[n][0])
            for key, bb in bits[n].items():
                if bb != b:
                    continue
                what = '{} width {} net {} {}'.format(pair, b, n, key)
                assert _same(got_w[key], want_w[key]), what + ': weight'
                assert _same(_np(plan.codes(n)[key]), _np(qp.codes(n)[key])), what + ': code'
                assert _same(_np(plan.ranges(n)[key]), _np(cp.ranges(n)[key])), what + ': range against clip_plan'
                assert _same(_np(plan.ranges(n)[key]), _np(qp.ranges(n)[key])), what + ': range against quant_plan'
        cp.close()
        qp.close()
    plan.close()


# ---- 5. stages -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pair', PAIRS)
def test_stages(engine, pair):
    per_channel, signed = pair
    name = 'tiny_res'
    results = []
    for way in ('run', 'allocate+quantise', 'allocate,clamp,quantise'):
        nets, batch = _batch(name, SEEDS, engine)
        plan = _clipped(batch, avg_bits=4, per_channel=per_channel, signed=signed, codes='int32')
        if way == 'run':
            plan.run()
        elif way == 'allocate+quantise':
            plan.run(plan.ALLOCATE | plan.QUANTISE)
        else:
            plan.allocate()
            plan.clamp()
            _ffi.synchronize()
            for n in range(3):                          # after CLAMP every unit's own (min, max) is `ranges`
                for key, w in _weights(nets[n][0]).items():
                    units = w if per_channel else w.reshape(1, -1)
                    own = np.stack([units.min(axis=1), units.max(axis=1)], axis=1)
                    assert np.array_equal(own, _np(plan.ranges(n)[key]).reshape(-1, 2)), '{} net {} {}'.format(pair, n, key)
            plan.quantise()
        _ffi.synchronize()
        results.append((_state(nets), _np(plan.code_block).copy(), [_np(b) for b in _blocks(plan)]))
        plan.close()
    for other in results[1:]:
        assert _same(results[0][0], other[0]) and _same(results[0][1], other[1])
        assert all(_same(a, b) for a, b in zip(results[0][2], other[2]))


def test_stage_errors_and_the_unclipped_plan(engine):
    lib = _ffi.lib()
    nets, batch = _batch('tiny_mobile', SEEDS[:2], engine)
    fresh = _clipped(batch, avg_bits=4, apply=False)
    for stages in (CLAMP, QUANTISE, CLAMP | QUANTISE):
        assert lib.dfq_batch_mixed_plan_run_stages(fresh._plan, stages, _ffi.stream_arg()) == DFQ_ERR_STATE
        assert b'dfq_batch_mixed_plan_run_stages' in lib.dfq_last_error()
    for stages in (0, 8, -1):
        assert lib.dfq_batch_mixed_plan_run_stages(fresh._plan, stages, _ffi.stream_arg()) == DFQ_ERR_ARG
    assert lib.dfq_batch_mixed_plan_run_stages(None, ALLOCATE, _ffi.stream_arg()) == DFQ_ERR_ARG
    fresh.close()
    plain = batch.mixed_plan(WIDTHS, avg_bits=4, codes='int32')
    assert plain.clip is None and plain.clip_range_block is None
    assert lib.dfq_batch_mixed_plan_run_stages(plain._plan, CLAMP, _ffi.stream_arg()) == DFQ_ERR_ARG
    assert lib.dfq_batch_mixed_plan_run_stages(plain._plan, ALLOCATE | CLAMP, _ffi.stream_arg()) == DFQ_ERR_ARG
    assert lib.dfq_batch_mixed_plan_run_stages(plain._plan, QUANTISE, _ffi.stream_arg()) == DFQ_ERR_STATE
    with pytest.raises(RuntimeError):
        plain.clip_ranges(0)
    plain.allocate()
    plain.bits_block.fill_(1 << 20)                     # a caller's write: the stage reads the plan's own state
    plain.quantise()
    _ffi.synchronize()
    staged = (_state(nets), _np(plain.code_block).copy(), _np(plain.bits_block).copy(), _np(plain.range_block).copy())
    plain.close()
    tnets, twin = _batch('tiny_mobile', SEEDS[:2], engine)
    ran = twin.mixed_plan(WIDTHS, avg_bits=4, codes='int32')
    ran.run()
    _ffi.synchronize()
    for a, b in zip(staged, (_state(tnets), _np(ran.code_block), _np(ran.bits_block), _np(ran.range_block))):
        assert _same(a, b), 'ALLOCATE then QUANTISE on a plan without clipping differs from its run()'
    ran.close()


# ---- 6. hand-made tensors through the C ABI ----------------------------------------------------------------------------------
def _layout(shapes):
    offs, at = [], 4
    for r, n in shapes:
        offs.append(at)
        at += -(-(r * n) // 4) * 4 + 4
    return offs, at


class Abi:
    """len(data) networks of float32 [rows, n] tensors in one store with sentinels in between, and every block of a plan"""

    def __init__(self, engine, data, per_row):
        self.lib, self.dev, self.data, self.per_row = _ffi.lib(), engine.device, data, per_row
        self.n_nets, self.shapes = len(data), [x.shape for x in data[0]]
        self.T = len(self.shapes)
        self.offs, self.stride = _layout(self.shapes)
        self.host = np.full((self.n_nets, self.stride), 7.5e5, dtype=F32)
        for k in range(self.n_nets):
            for x, o in zip(data[k], self.offs):
                self.host[k, o:o + x.size] = x.reshape(-1)
        self.store = torch.from_numpy(self.host.copy()).to(self.dev).contiguous()
        base0 = self.store.data_ptr()
        self.bases = (ctypes.c_void_p * self.n_nets)(*[base0 + 4 * k * self.stride for k in range(self.n_nets)])
        self.units = [r if per_row else 1 for r, _ in self.shapes]
        self.u_offs = [1 + sum(self.units[:i]) + i for i in range(self.T)]       # one sentinel unit in front of every tensor
        self.u_stride = sum(self.units) + self.T + 1

    def tensor(self, net, i):
        r, n = self.shapes[i]
        return self.store[net, self.offs[i]:self.offs[i] + r * n].cpu().numpy().reshape(r, n)

    def gaps_untouched(self):
        mask = np.ones(self.stride, dtype=bool)
        for (r, n), o in zip(self.shapes, self.offs):
            mask[o:o + r * n] = False
        return bool((self.store.cpu().numpy()[:, mask] == 7.5e5).all())

    def clip(self, bits, signed, k_cand, alpha_min):
        """dfq_batch_clip_plan over the store, apply = 0: (ranges [n, U, 2], chosen [n, U], errors [n, U, K])"""
        P = _ffi.DfqBatchClipTensor
        base0 = self.store.data_ptr()
        tabs = (P * self.T)(*[P(base0 + 4 * o, r, n, u) for (r, n), o, u in zip(self.shapes, self.offs, self.u_offs)])
        cfg = _ffi.DfqBatchClipConfig(bits, int(signed), int(self.per_row), k_cand, alpha_min, 0, 0)
        rng = torch.full((self.n_nets, self.u_stride, 2), 9.0, dtype=torch.float32, device=self.dev)
        cho = torch.full((self.n_nets, self.u_stride), -7, dtype=torch.int32, device=self.dev)
        err = torch.full((self.n_nets, self.u_stride, k_cand), 9.0, dtype=torch.float64, device=self.dev)
        plan = ctypes.c_void_p()
        _ffi.check(self.lib.dfq_batch_clip_plan_create(tabs, self.T, ctypes.byref(cfg), self.bases, self.n_nets, rng.data_ptr(), cho.data_ptr(),
                                                       err.data_ptr(), self.u_stride, ctypes.byref(plan)))
        try:
            _ffi.check(self.lib.dfq_batch_clip_plan_run(plan, _ffi.stream_arg()))
            _ffi.synchronize()
        finally:
            self.lib.dfq_batch_clip_plan_destroy(plan)
        return rng.cpu().numpy(), cho.cpu().numpy(), err.cpu().numpy()

    def mixed(self, widths, signed, budget, k_cand, alpha_min, apply=0, code_bytes=4, stages=None, runs=1):
        """dfq_batch_mixed_plan_create_clipped over the store -> dict of numpy blocks"""
        B, T, n_nets = len(widths), self.T, self.n_nets
        c_offs, r_offs, cs, rs = [], [], 0, 0
        for (r, n), units in zip(self.shapes, self.units):
            c_offs.append(cs + 1)
            cs += r * n + 2
            r_offs.append(rs + 1)
            rs += 2 * units + 2
        code_dtype = {4: torch.int32, 1: torch.int8 if signed else torch.uint8}[code_bytes]
        dev = self.dev
        blocks = dict(bits=torch.full((n_nets, T), -7, dtype=torch.int32, device=dev),
                      errors=torch.full((n_nets, T, B), 9.0, dtype=torch.float64, device=dev),
                      used=torch.full((n_nets, 2), -7, dtype=torch.int64, device=dev),
                      cost=torch.full((n_nets,), 9.0, dtype=torch.float64, device=dev),
                      codes=torch.full((n_nets, cs), 77, dtype=code_dtype, device=dev),
                      ranges=torch.full((n_nets, rs), 9.0, dtype=torch.float32, device=dev),
                      clip_ranges=torch.full((n_nets, self.u_stride, B, 2), 9.0, dtype=torch.float32, device=dev),
                      clip_chosen=torch.full((n_nets, self.u_stride, B), -7, dtype=torch.int32, device=dev),
                      unit_errors=torch.full((n_nets, self.u_stride, B), 9.0, dtype=torch.float64, device=dev))
        base0 = self.store.data_ptr()
        P = _ffi.DfqBatchMixedTensor
        tabs = (P * T)(*[P(base0 + 4 * o, r, n, 1.0, 0, 0, c_offs[i], r_offs[i]) for i, ((r, n), o) in enumerate(zip(self.shapes, self.offs))])
        cfg = _ffi.DfqBatchMixedConfig((ctypes.c_int32 * 8)(*widths), B, int(signed), int(self.per_row), int(apply), code_bytes, 0, budget)
        uo = (ctypes.c_int64 * T)(*self.u_offs)
        clip = _ffi.DfqBatchMixedClip(k_cand, 0, alpha_min, blocks['clip_ranges'].data_ptr(), blocks['clip_chosen'].data_ptr(),
                                      blocks['unit_errors'].data_ptr(), self.u_stride, uo)
        plan = ctypes.c_void_p()
        _ffi.check(self.lib.dfq_batch_mixed_plan_create_clipped(
            tabs, T, ctypes.byref(cfg), self.bases, n_nets, blocks['bits'].data_ptr(), blocks['errors'].data_ptr(), blocks['used'].data_ptr(),
            blocks['cost'].data_ptr(), blocks['codes'].data_ptr(), cs, blocks['ranges'].data_ptr(), rs, ctypes.byref(clip), ctypes.byref(plan)))
        try:
            flat = (not self.per_row) and any(r * n > 1536 for r, n in self.shapes)
            rows = self.per_row or any(r * n <= 1536 for r, n in self.shapes)
            assert self.lib.dfq_batch_mixed_plan_launches(plan) == 3 * flat + rows + 2 + bool(apply) * (flat + rows)
            for i in range(runs):
                for s in (stages or [None]):
                    if s is None:
                        _ffi.check(self.lib.dfq_batch_mixed_plan_run(plan, _ffi.stream_arg()))
                    else:
                        _ffi.check(self.lib.dfq_batch_mixed_plan_run_stages(plan, s, _ffi.stream_arg()))
                _ffi.synchronize()
                if i == 0:
                    first = {k: v.clone() for k, v in blocks.items()}
            if not apply and stages is None:
                for k, v in blocks.items():
                    assert _same(_np(first[k]), _np(v)), 'two runs differ in ' + k
        finally:
            self.lib.dfq_batch_mixed_plan_destroy(plan)
        out = {k: _np(v) for k, v in first.items()}
        out.update(c_offs=c_offs, r_offs=r_offs)
        assert self.gaps_untouched(), 'a weight outside the tensors was written'
        umask = np.ones(self.u_stride, dtype=bool)
        cmask, rmask = np.ones(cs, dtype=bool), np.ones(rs, dtype=bool)
        for i, ((r, n), units) in enumerate(zip(self.shapes, self.units)):
            umask[self.u_offs[i]:self.u_offs[i] + units] = False
            cmask[c_offs[i]:c_offs[i] + r * n] = False
            rmask[r_offs[i]:r_offs[i] + 2 * units] = False
        assert (out['clip_ranges'][:, umask] == 9.0).all() and (out['clip_chosen'][:, umask] == -7).all() and (out['unit_errors'][:, umask] == 9.0).all()
        assert (out['codes'][:, cmask] == 77).all() and (out['ranges'][:, rmask] == 9.0).all(), 'something else in the blocks was touched'
        if not apply and stages is None:
            assert (out['codes'] == 77).all() and _same(self.store.cpu().numpy(), self.host), 'apply = 0 wrote'
        return out


def _rand(shapes, seed):
    rng = np.random.RandomState(seed)
    return [(rng.standard_normal(s) * rng.uniform(0.05, 2.0) * (1.0 + 3.0 * (rng.uniform(size=s) > 0.97))).astype(F32) for s in shapes]


def _check_abi(abi, out, widths, signed, k_cand, alpha_min, numpy_units=4, what=''):
    """as tests 1 and 2: every unit against dfq_batch_clip_plan bit for bit; the first units of every tensor against numpy;
    E against the units' errors; ranges = the chosen width's"""
    B = len(widths)
    for j, b in enumerate(widths):
        rr, rc, re = abi.clip(b, signed, k_cand, alpha_min)
        assert _same(out['clip_chosen'][:, :, j], rc), '{} width {}: k*'.format(what, b)
        assert _same(out['clip_ranges'][:, :, j], rr), '{} width {}: ranges'.format(what, b)
        live = rc >= 0
        at = np.take_along_axis(re, np.maximum(rc, 0)[:, :, None].astype(np.int64), axis=2)[:, :, 0]
        assert _same(out['unit_errors'][:, :, j][live], at[live]), '{} width {}: unit errors'.format(what, b)
        with np.errstate(invalid='ignore'):
            assert (np.isnan(re[:, :, 0][live]) | (out['unit_errors'][:, :, j][live] <= re[:, :, 0][live])).all()
    for net in range(abi.n_nets):
        for i, (r, n) in enumerate(abi.shapes):
            x = abi.data[net][i]
            units = x if abi.per_row else x.reshape(1, -1)
            u0, nu = abi.u_offs[i], abi.units[i]
            pick = sorted(set(list(range(min(numpy_units, nu))) + [nu - 1]))
            _check_numpy(units[pick], widths, signed, k_cand, alpha_min, out['clip_chosen'][net, u0:u0 + nu][pick],
                         out['clip_ranges'][net, u0:u0 + nu][pick], out['unit_errors'][net, u0:u0 + nu][pick],
                         '{} net {} tensor {}'.format(what, net, i))
            e = out['unit_errors'][net, u0:u0 + nu]
            for j in range(B):
                vals = e[:, j].tolist()
                E = float(out['errors'][net, i, j])
                if any(math.isnan(v) for v in vals):
                    assert math.isnan(E)
                elif nu == 1:
                    assert _same(np.float64(E), np.float64(vals[0]))
                else:
                    exact = math.fsum(vals)
                    assert E == exact or abs(E - exact) <= nu * U * exact
            jt = list(widths).index(int(out['bits'][net, i]))
            got = out['ranges'][net, out['r_offs'][i]:out['r_offs'][i] + 2 * nu].reshape(nu, 2)
            assert _same(got, out['clip_ranges'][net, u0:u0 + nu, jt]), '{} net {} tensor {}: ranges'.format(what, net, i)


@pytest.mark.parametrize('n_nets', [1, 3])
@pytest.mark.parametrize('kb', [(5, 8), (1, 2), (64, 8), (64, 2)])
def test_row_shapes_through_the_abi(engine, n_nets, kb):
    k_cand, B = kb
    widths = WIDTHS[:2] if B == 2 else (2, 3, 4, 5, 6, 7, 8, 10)
    signed = k_cand != 5
    # the lane-class edges, the register bound and the looping wave; 1, 3 and 67 rows (67: more than one wave of every class
    # it is used with).  The cases with 64 candidates keep one length per path: the emulation pays for every evaluation.
    lens = [1, 4, 9, 16, 17, 64, 65, 256, 257, 1536, 1537, 3000] if k_cand == 5 else [9, 65, 1537]
    rows = [1, 3, 67]
    shapes = [(rows[i % 3] if n <= 64 else min(rows[i % 3], 3), n) for i, n in enumerate(lens)]
    shapes += [(67, 9), (1, 257), (3, 64)] if k_cand == 5 else [(67, 4)]
    data = [_rand(shapes, 100 + k) for k in range(n_nets)]
    abi = Abi(engine, data, True)
    total = sum(r * n for r, n in shapes)
    out = abi.mixed(widths, signed, 4 * total, k_cand, 0.25)
    _check_abi(abi, out, widths, signed, k_cand, 0.25, numpy_units=2, what='rows K={} B={}'.format(k_cand, B))


@pytest.mark.parametrize('n_nets', [1, 3])
@pytest.mark.parametrize('kb', [(5, 8), (1, 2), (64, 8)])
def test_tensor_shapes_through_the_abi(engine, n_nets, kb):
    k_cand, B = kb
    widths = WIDTHS[:2] if B == 2 else (2, 3, 4, 5, 6, 7, 8, 10)
    signed = k_cand == 5
    shapes = [(1, 9), (3, 512), (1, 1537), (4, 1024), (1, 4097), (3, 2731)]        # 9, 1536, 1537, 4096, 4097, 8193 elements
    assert [r * n for r, n in shapes] == [9, 1536, 1537, 4096, 4097, 8193]
    if k_cand == 64:                                    # (one tensor per path: the emulation pays for every evaluation)
        shapes = [shapes[0], shapes[2], shapes[4]]
    data = [_rand(shapes, 200 + k) for k in range(n_nets)]
    abi = Abi(engine, data, False)
    total = sum(r * n for r, n in shapes)
    out = abi.mixed(widths, signed, 4 * total, k_cand, 0.25)
    _check_abi(abi, out, widths, signed, k_cand, 0.25, what='tensors K={} B={}'.format(k_cand, B))
    if B == 8:
        assert len(set(out['bits'].reshape(-1).tolist())) >= 2


def test_apply_through_the_abi(engine):
    """the clamp stage stores only what it changes and nothing where k* = 0; the quantising stage equals the definition"""
    for per_row in (False, True):
        shapes = [(3, 40), (2, 1000), (1, 5000), (5, 33)] if not per_row else [(3, 40), (2, 1600), (5, 33)]
        data = [_rand(shapes, 300 + k) for k in range(2)]
        total = sum(r * n for r, n in shapes)
        clamped = Abi(engine, data, per_row)
        out = clamped.mixed(WIDTHS, False, 4 * total, K, ALPHA_MIN, stages=[ALLOCATE, CLAMP])
        quant = Abi(engine, data, per_row)
        outq = quant.mixed(WIDTHS, False, 4 * total, K, ALPHA_MIN, apply=1)
        both = Abi(engine, data, per_row)
        outb = both.mixed(WIDTHS, False, 4 * total, K, ALPHA_MIN, stages=[ALLOCATE, CLAMP, QUANTISE])
        assert _same(quant.store.cpu().numpy(), both.store.cpu().numpy()) and _same(outq['codes'], outb['codes'])
        assert (out['codes'] == 77).all()
        moved = 0
        for net in range(2):
            for i, (r, n) in enumerate(shapes):
                x = data[net][i]
                units = x if per_row else x.reshape(1, -1)
                jt = WIDTHS.index(int(out['bits'][net, i]))
                u0 = clamped.u_offs[i]
                for u, row in enumerate(units):
                    l, h = out['clip_ranges'][net, u0 + u, jt]
                    ks = out['clip_chosen'][net, u0 + u, jt]
                    want = _clamp(row, l, h)
                    got = clamped.tensor(net, i).reshape(units.shape)[u]
                    assert _same(got, want)
                    if ks == 0:
                        assert _same(got, row)
                    moved += int(ks != 0)
                    y, q = _fake_quant(want, _qparams(l, h, WIDTHS[jt], False))
                    assert _same(quant.tensor(net, i).reshape(units.shape)[u], y)
                    c0 = outq['c_offs'][i] + u * units.shape[1]
                    assert np.array_equal(outq['codes'][net, c0:c0 + units.shape[1]], q.astype(np.int32))
        assert moved > 0


# ---- 7. special values -------------------------------------------------------------------------------------------------------
def _snan():
    return np.array([0x7fa00001], dtype=np.uint32).view(F32)[0]


@pytest.mark.parametrize('per_row', [False, True])
@pytest.mark.parametrize('kind', ['constant', 'nan', 'snan', 'inf', 'neg_inf', 'neg_zero_row', 'all_nan'])
def test_special_values(engine, kind, per_row):
    shapes = [(6, 40), (4, 50), (3, 1543) if not per_row else (3, 70), (5, 33)]
    data = [_rand(shapes, 40 + k) for k in range(2)]
    victim = 1 if kind != 'inf' else 2                 # (the long per-tensor tensor, too)
    x = data[1][victim]
    if kind == 'constant':
        x[:] = F32(0.375)
    elif kind == 'nan':
        x[1, 7] = np.nan
    elif kind == 'snan':
        x[2, 0] = _snan()
    elif kind == 'inf':
        x[0, 3] = np.inf
    elif kind == 'neg_inf':
        x[3, 1] = -np.inf
    elif kind == 'neg_zero_row':
        x[2, :] = F32(-0.0)
    else:
        x[:] = np.nan
    total = sum(r * n for r, n in shapes)
    search = Abi(engine, data, per_row)
    _check_abi(search, search.mixed(WIDTHS, False, 5 * total, K, ALPHA_MIN), WIDTHS, False, K, ALPHA_MIN, numpy_units=8, what=kind)
    abi = Abi(engine, data, per_row)
    out = abi.mixed(WIDTHS, False, 5 * total, K, ALPHA_MIN, stages=[ALLOCATE, CLAMP])
    u0, nu = abi.u_offs[victim], abi.units[victim]
    row = {'nan': 1, 'snan': 2, 'inf': 0, 'neg_inf': 3}.get(kind, 0) if per_row else 0
    err, cho = out['unit_errors'][1, u0 + row], out['clip_chosen'][1, u0 + row]
    if kind in ('nan', 'snan', 'all_nan'):
        assert np.isnan(err).all() and (cho == 0).all(), 'a unit holding NaN has NaN errors and k* = 0'
        assert np.isnan(out['errors'][1, victim]).all() and out['bits'][1, victim] == WIDTHS[0], 'its tensor takes no step'
    if kind in ('inf', 'neg_inf'):
        assert (cho == 0).all() and not np.isfinite(err).any(), 'a unit holding an infinity keeps k* = 0'
    if kind == 'constant':
        assert (out['unit_errors'][1, u0:u0 + nu] == 0).all() and (out['clip_chosen'][1, u0:u0 + nu] == 0).all()
        assert out['bits'][1, victim] == WIDTHS[0]
    # no unit is written where k* = 0: the victim's units with k* = 0 at the chosen width hold their bits, NaN payloads included
    jt = WIDTHS.index(int(out['bits'][1, victim]))
    got = abi.tensor(1, victim)
    units_got = got if per_row else got.reshape(1, -1)
    units_in = x if per_row else x.reshape(1, -1)
    for u in range(nu):
        if out['clip_chosen'][1, u0 + u, jt] == 0:
            assert np.array_equal(units_got[u].view(np.int32), units_in[u].view(np.int32)), 'a unit with k* = 0 was written'
    # the neighbours are undisturbed: network 0 and the other tensors of network 1 equal a run without the victim
    clean = [_rand(shapes, 40 + k) for k in range(2)]
    base = Abi(engine, clean, per_row).mixed(WIDTHS, False, 5 * total, K, ALPHA_MIN, stages=[ALLOCATE, CLAMP])
    for k in ('errors', 'bits', 'clip_ranges', 'clip_chosen', 'unit_errors'):
        assert _same(out[k][0], base[k][0]), k
    others = [i for i in range(len(shapes)) if i != victim]
    assert _same(out['errors'][1, others], base['errors'][1, others]) and np.isfinite(out['errors'][1, others]).all()
    for i in others:
        a0, an = abi.u_offs[i], abi.units[i]
        assert _same(out['clip_chosen'][1, a0:a0 + an], base['clip_chosen'][1, a0:a0 + an])
        assert _same(out['unit_errors'][1, a0:a0 + an], base['unit_errors'][1, a0:a0 + an])


# ---- 8. determinism ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pair', PAIRS)
def test_two_runs_a_network_s_place_and_the_batch_of_one(engine, pair):
    per_channel, signed = pair
    name = 'tiny_cat'
    nets, batch = _batch(name, SEEDS, engine)
    plan = _clipped(batch, avg_bits=4, per_channel=per_channel, signed=signed, apply=False)
    plan.run()
    _ffi.synchronize()
    first = _blocks(plan)
    plan.run()
    _ffi.synchronize()
    assert _blocks_same(first, _blocks(plan)), 'two runs differ'
    for place, seeds in ((0, [2]), (1, [0, 2, 1])):
        _, other = _batch(name, seeds, engine)
        alone = _clipped(other, avg_bits=4, per_channel=per_channel, signed=signed, apply=False)
        alone.run()
        _ffi.synchronize()
        for a, b in zip(first, _blocks(alone)):
            assert _same(_np(a[2]), _np(b[place])), 'a network depends on the batch or on its place in it'
        alone.close()
    # the single-network entry point
    model, graph, bottoms, _ = _prepared(name, 2, engine.device)
    res = dfq.quantize_mixed(graph, WIDTHS, avg_bits=4, per_channel=per_channel, signed=signed, clip=K, alpha_min=ALPHA_MIN)
    applied = _clipped(batch, avg_bits=4, per_channel=per_channel, signed=signed)
    applied.run()
    _ffi.synchronize()
    got_w = _weights(graph)
    bits, errs, rngs, cho = applied.bits(2), applied.errors(2), applied.ranges(2), applied.clip_chosen(2)
    for key, w in _weights(nets[2][0]).items():
        j = WIDTHS.index(bits[key])
        assert res[key]['bits'] == bits[key] and _same(np.float64(res[key]['err']), np.float64(errs[key][j])), key
        assert _same(res[key]['range'], _np(rngs[key])) and _same(got_w[key], w), key
        assert np.array_equal(res[key]['chosen'], _np(cho[key])[..., j]), key
    applied.close()
    plan.close()


# ---- 9. quantize_mixed(clip=) ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pair', PAIRS)
def test_quantize_mixed_clip(engine, pair):
    per_channel, signed = pair
    name = 'tiny_mobile'
    nets, batch = _batch(name, SEEDS, engine)
    codes, ranges, bits = batch.quantize_mixed(WIDTHS, avg_bits=4, per_channel=per_channel, signed=signed, clip=K, alpha_min=ALPHA_MIN)
    tnets, twin = _batch(name, SEEDS, engine)
    plan = _clipped(twin, avg_bits=4, per_channel=per_channel, signed=signed, codes='int32')
    plan.run()
    _ffi.synchronize()
    qnets, qb = _batch(name, SEEDS, engine)
    qb.quantize(8, 16, per_channel, signed)
    for n in range(3):
        assert bits[n] == dict(plan.bits(n))
        for key, w in _weights(nets[n][0]).items():
            assert _same(w, _weights(tnets[n][0])[key]) and _same(_np(codes[n][key]), _np(plan.codes(n)[key])), key
            assert _same(_np(ranges[n][key]), _np(plan.ranges(n)[key])), key
        want = _biases(qnets[n][0])
        assert want, 'no biases: the test shows nothing'
        for key, b in _biases(nets[n][0]).items():
            assert _same(b, want[key]), 'bias of ' + key
    plan.close()
    assert len({b for d in bits for b in d.values()}) >= 2


@pytest.mark.parametrize('pair', PAIRS[:2])
def test_quantize_mixed_clip_correct_is_the_sequence_by_hand(engine, pair):
    per_channel, signed = pair
    name = 'tiny_res'
    nets, batch = _batch(name, SEEDS, engine)
    codes, ranges, bits = batch.quantize_mixed(WIDTHS, avg_bits=4, per_channel=per_channel, signed=signed, clip=K, alpha_min=ALPHA_MIN,
                                               correct=True)
    hnets, hand = _batch(name, SEEDS, engine)
    plan = _clipped(hand, avg_bits=4, per_channel=per_channel, signed=signed, codes='int32')
    bc = hand.bc_plan()
    plan.allocate()
    plan.clamp()
    bc.run(signed=signed, per_channel=per_channel, widths=plan)
    plan.quantise()
    bias_plan = arena.BatchQuantPlan(hand, WIDTHS[-1], 16, per_channel, signed, None, _biases_only=True)
    bias_plan.run()
    bc.status()
    _ffi.synchronize()
    assert _same(_state(nets), _state(hnets)), 'weights, biases or beta~ differ from the sequence by hand'
    unets, uncorrected = _batch(name, SEEDS, engine)
    uncorrected.quantize_mixed(WIDTHS, avg_bits=4, per_channel=per_channel, signed=signed, clip=K, alpha_min=ALPHA_MIN)
    assert not _same(_state(nets), _state(unets)), 'the correction changed nothing'
    for n in range(3):
        assert bits[n] == dict(plan.bits(n))
        for key in plan.keys:
            assert _same(_np(codes[n][key]), _np(plan.codes(n)[key]))
    for p in (plan, bc, bias_plan):
        p.close()


@pytest.mark.parametrize('correct', [False, True])
def test_clip_none_is_today_s_path(engine, correct, monkeypatch):
    name = 'tiny_mobile'
    anets, a = _batch(name, SEEDS[:2], engine)
    bnets, b = _batch(name, SEEDS[:2], engine)
    ra = a.quantize_mixed(WIDTHS, avg_bits=4, per_channel=True, signed=True, correct=correct)
    calls = []
    lib = _ffi.lib()
    real = lib.dfq_batch_mixed_plan_create_clipped
    monkeypatch.setattr(lib, 'dfq_batch_mixed_plan_create_clipped', lambda *args: calls.append(1) or real(*args), raising=False)
    rb = b.quantize_mixed(WIDTHS, avg_bits=4, per_channel=True, signed=True, correct=correct, clip=None)
    assert not calls, 'clip=None went through the clipped entry point'
    assert _same(_state(anets), _state(bnets)) and ra[2] == rb[2]
    for n in range(2):
        for key in ra[0][n]:
            assert _same(_np(ra[0][n][key]), _np(rb[0][n][key]))
        for key in ra[1][n]:
            assert _same(_np(ra[1][n][key]), _np(rb[1][n][key]))


# ---- 10. pack round trip -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pair', PAIRS[:2])
def test_pack_round_trip(engine, pair, tmp_path):
    per_channel, signed = pair
    name = 'tiny_mobile'
    nets, batch = _batch(name, SEEDS[:2], engine)
    src = _clipped(batch, avg_bits=4, per_channel=per_channel, signed=signed, codes='int8')
    src.run()
    pack = batch.pack_plan(src)
    pack.run()
    _ffi.synchronize()
    assert pack.status_block.cpu().tolist() == [0, 0]
    snaps = [_weights(g) for (g, _, _) in nets]
    with torch.no_grad():
        for (g, _, _) in nets:
            for _, m in _targ(g):
                m.weight.fill_(0.25)
    un = batch.unpack_plan(pack, weights=True, codes='int32')
    un.run()
    _ffi.synchronize()
    assert un.status_block.cpu().tolist() == [0, 0]
    for n, (g, _, _) in enumerate(nets):
        for key, w in _weights(g).items():
            assert np.array_equal(w, snaps[n][key]), key                  # (value-equal: bit for bit off the zeros)
            off = snaps[n][key] != 0
            assert _same(w[off], snaps[n][key][off]), key
            assert torch.equal(un.codes(n)[key].cpu().to(torch.int64), src.codes(n)[key].cpu().to(torch.int64)), key
    path = str(tmp_path / 'packed.npz')
    batch.save_packed(path, src)
    nets2, batch2 = _batch(name, [5, 6], engine)
    batch2.load_packed(path)
    for n, (g, _, _) in enumerate(nets2):
        for key, w in _weights(g).items():
            assert np.array_equal(w, snaps[n][key]), key
    for p in (un, pack, src):
        p.close()


# ---- 11. refusals ------------------------------------------------------------------------------------------------------------
def test_abi_rejects_bad_arguments(engine):
    lib = _ffi.lib()
    dev = engine.device
    buf = torch.zeros(8192, dtype=torch.float32, device=dev)
    bits = torch.zeros(64, dtype=torch.int32, device=dev)
    errors = torch.zeros(64, dtype=torch.float64, device=dev)
    used = torch.zeros(8, dtype=torch.int64, device=dev)
    cost = torch.zeros(4, dtype=torch.float64, device=dev)
    codes = torch.zeros(8192, dtype=torch.int32, device=dev)
    ranges = torch.zeros(64, dtype=torch.float32, device=dev)
    cr = torch.zeros(4096, dtype=torch.float32, device=dev)
    cc = torch.zeros(2048, dtype=torch.int32, device=dev)
    ue = torch.zeros(2048, dtype=torch.float64, device=dev)
    P = _ffi.DfqBatchMixedTensor

    def create(widths=(2, 4, 8), k_cand=8, alpha_min=0.5, clip=True, cr_ptr=True, cc_ptr=True, ue_ptr=True, u_stride=6, u_offs=(0, 1),
               offsets=True, per_row=0, bits_ptr=True, n_nets=1, table=True, code_bytes=4, budget=10 ** 6, fixed=0, sens=1.0, data_off=0,
               rows=4):
        tabs = (P * 2)(P(buf.data_ptr() + data_off, rows, 16, sens, fixed, 0, 0, 0), P(buf.data_ptr() + 4096, 2, 8, 1.0, 0, 0, 64, 16))
        cfg = _ffi.DfqBatchMixedConfig((ctypes.c_int32 * 8)(*(list(widths) + [0] * (8 - len(widths)))), len(widths), 0, per_row, 1, code_bytes,
                                       0, budget)
        uo = (ctypes.c_int64 * 2)(*u_offs)
        desc = _ffi.DfqBatchMixedClip(k_cand, 0, alpha_min, cr.data_ptr() if cr_ptr else None, cc.data_ptr() if cc_ptr else None,
                                      ue.data_ptr() if ue_ptr else None, u_stride, uo if offsets else None)
        bases = (ctypes.c_void_p * 1)(buf.data_ptr())
        plan = ctypes.c_void_p()
        rc = lib.dfq_batch_mixed_plan_create_clipped(tabs if table else None, 2, ctypes.byref(cfg), bases, n_nets,
                                                     bits.data_ptr() if bits_ptr else None, errors.data_ptr(), used.data_ptr(), cost.data_ptr(),
                                                     codes.data_ptr(), 4096, ranges.data_ptr(), 32, ctypes.byref(desc) if clip else None,
                                                     ctypes.byref(plan))
        return rc, plan

    rc, plan = create()
    assert rc == 0
    assert lib.dfq_batch_mixed_plan_launches(plan) == 1 + 2 + 1
    lib.dfq_batch_mixed_plan_destroy(plan)
    rc, plan = create(ue_ptr=False)                     # null unit_errors: not written, not refused
    assert rc == 0
    lib.dfq_batch_mixed_plan_destroy(plan)
    rc, plan = create(widths=(2, 3, 4, 5, 6, 7, 8, 9), k_cand=64)      # 512 pairs: the most
    assert rc == 0
    lib.dfq_batch_mixed_plan_destroy(plan)
    bad = [dict(k_cand=0), dict(k_cand=65), dict(k_cand=-1), dict(alpha_min=0.0), dict(alpha_min=1.5), dict(alpha_min=math.nan),
           dict(alpha_min=-0.5), dict(n_nets=0),
           # (B <= 8 and K <= 64 keep B * K at or below 512: the pair bound is reached, never passed, by arguments that pass the others)
           dict(widths=(2, 3, 4, 5, 6, 7, 8, 9), k_cand=65), dict(clip=False), dict(cr_ptr=False), dict(cc_ptr=False), dict(offsets=False),
           dict(u_stride=0), dict(u_offs=(0, 6)), dict(u_offs=(-1, 1)), dict(per_row=1, u_offs=(0, 5)), dict(per_row=1, u_offs=(3, 0)),
           # everything the unclipped create refuses
           dict(widths=(4,)), dict(widths=(4, 2)), dict(widths=(1, 4)), dict(widths=(2, 17)), dict(bits_ptr=False), dict(table=False),
           dict(code_bytes=2), dict(budget=-1), dict(fixed=5), dict(sens=-1.0), dict(sens=math.inf), dict(data_off=4), dict(rows=0)]
    for kw in bad:
        rc, plan = create(**kw)
        assert rc == DFQ_ERR_ARG and not plan, kw
        assert b'dfq_batch_mixed_plan_create_clipped' in lib.dfq_last_error(), kw


def test_python_refusals(engine):
    _, batch = _batch('tiny_mobile', SEEDS[:1], engine)
    for kw in (dict(clip=0), dict(clip=65), dict(clip=True), dict(clip=4.0), dict(clip='8'), dict(clip=8, alpha_min=0), dict(clip=8, alpha_min=1.5),
               dict(clip=8, alpha_min=math.nan), dict(clip=8, alpha_min='x'), dict(clip=8, widths=(4,)), dict(clip=8, widths=(4, 2)),
               dict(clip=8, codes='int16'), dict(clip=8, pin={'nope': 4})):
        kw = dict(kw)
        widths = kw.pop('widths', WIDTHS)
        with pytest.raises(ValueError, match='mixed_plan'):
            batch.mixed_plan(widths, avg_bits=4, **kw)
    with pytest.raises(ValueError, match='exactly one'):
        batch.mixed_plan(WIDTHS, clip=8)
    with pytest.raises(ValueError, match='mixed_plan'):
        batch.quantize_mixed(WIDTHS, avg_bits=4, clip=65)
    model, graph, bottoms, _ = _prepared('tiny_mobile', 0, engine.device)
    with pytest.raises(ValueError, match='quantize_mixed'):
        dfq.quantize_mixed(graph, WIDTHS, avg_bits=4, clip=0)


def test_struct_layout_matches_header():
    src = r'''
    #include <stdio.h>
    #include <stddef.h>
    #include "dfq_hip.h"
    int main(void) {
        printf("%zu %zu %zu %zu %zu %zu %zu %zu %d %d %d\n", sizeof(dfq_batch_mixed_clip), offsetof(dfq_batch_mixed_clip, candidates),
               offsetof(dfq_batch_mixed_clip, alpha_min), offsetof(dfq_batch_mixed_clip, clip_ranges), offsetof(dfq_batch_mixed_clip, clip_chosen),
               offsetof(dfq_batch_mixed_clip, unit_errors), offsetof(dfq_batch_mixed_clip, unit_stride),
               offsetof(dfq_batch_mixed_clip, unit_offsets), DFQ_MIXED_ALLOCATE, DFQ_MIXED_CLAMP, DFQ_MIXED_QUANTISE);
        return 0;
    }'''
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, 't.c')
        open(c, 'w').write(src)
        exe = os.path.join(d, 't')
        subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), c, '-o', exe], check=True)
        got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    S = _ffi.DfqBatchMixedClip
    assert got == [ctypes.sizeof(S), S.candidates.offset, S.alpha_min.offset, S.clip_ranges.offset, S.clip_chosen.offset, S.unit_errors.offset,
                   S.unit_stride.offset, S.unit_offsets.offset, _ffi.MIXED_ALLOCATE, _ffi.MIXED_CLAMP, _ffi.MIXED_QUANTISE]
    assert (arena.BatchMixedPlan.ALLOCATE, arena.BatchMixedPlan.CLAMP, arena.BatchMixedPlan.QUANTISE) == (ALLOCATE, CLAMP, QUANTISE)
