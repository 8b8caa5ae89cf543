"""NetworkBatch.mixed_plan / quantize_mixed / dfq.quantize_mixed / dfq_batch_mixed_plan_*: a bit width per layer under a size
budget, found and applied on the device for every network of a batch.

The references are numpy and plain Python, in this file, by the definition in include/dfq_hip.h:
  errors      the quantiser recipe tests/test_batch_error.py and tests/test_batch_clip.py state (``_qparams`` in Python floats,
              five separately rounded float32 operations per element), e = Q(w) - w in float32, and E = ``math.fsum`` of the
              float64 squares, exact up to the final rounding.  The plan adds the same n_t terms in float64 in an order of its
              own, so |got - E| <= n_t u E with u = 2^-53 (Higham (4.4); every term is >= 0).  The same bound holds against
              ``error_plan``'s third sum.
  allocation  the greedy walk restated with Python floats (IEEE float64: one multiplication per cost, one subtraction and one
              division per g), fed the plan's OWN errors: bits, used and steps must then agree exactly and the cost bit for
              bit, whatever the budget.
  quantiser   the stored weight, the code and the range, bit for bit: against ``quant_plan`` on a twin batch at every width
              that occurs, and against the numpy recipe for the hand-made tensors."""
import ctypes
import itertools
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
WIDTHS = (2, 3, 4, 6, 8)
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
    """(Q(w), code) float32 for w [units, n] and one parameter tuple per unit: quantize.py:70-74, five float32 roundings"""
    qmin, qmax = prm[0][0], prm[0][1]
    neg_min, scale, min_value = (np.array([p[i] for p in prm], dtype=F32).reshape(-1, 1) for i in (2, 3, 4))
    with np.errstate(all='ignore'):
        q = w + neg_min
        q = q / scale
        q = np.where(q < qmin, qmin, q)
        q = np.where(q > qmax, qmax, q)
        q = np.rint(q)
        y = q * scale
        y = y + min_value
    assert y.dtype == F32 and q.dtype == F32
    return y, q


def _unit_range(x):
    """(mn, mx) of a unit by the house rule: NaN skipped, nothing but NaN keeps the identities (+inf, -inf)"""
    ok = ~np.isnan(x)
    return (F32(x[ok].min()), F32(x[ok].max())) if ok.any() else (F32(np.inf), F32(-np.inf))


def _fsum(vals):
    vals = vals.tolist()
    if any(math.isnan(v) for v in vals):
        return math.nan
    return math.fsum(vals)             # (every term is >= 0: an infinity among them gives inf)


def _units(w, per_row):
    return w if per_row else w.reshape(1, -1)


def _ref_tensor(w, per_row, signed, widths):
    """{'ranges' float32 [units, 2], 'err' [B] exact sums, 'y' / 'q': per width the stored weight and the code, float32}"""
    assert w.dtype == F32 and w.ndim == 2
    x = _units(w, per_row)
    rng = [_unit_range(r) for r in x]
    out = {'ranges': np.array(rng, dtype=F32).reshape(-1, 2), 'err': [], 'y': {}, 'q': {}, 'numel': w.size}
    for b in widths:
        y, q = _fake_quant(x, [_qparams(mn, mx, b, signed) for mn, mx in rng])
        with np.errstate(all='ignore'):
            d = (y - x).astype(np.float64).reshape(-1)
            out['err'].append(_fsum(d * d))
        out['y'][b], out['q'][b] = y.reshape(w.shape), q.reshape(w.shape)
    return out


def _check_errors(got, ref, what):
    """got float64 [B] against the exact sums, each within n_t u E"""
    for j, exact in enumerate(ref['err']):
        g = float(got[j])
        if math.isnan(exact):
            assert math.isnan(g), '{} width {}: {} for NaN'.format(what, j, g)
        elif math.isinf(exact):
            assert g == exact, '{} width {}: {} for inf'.format(what, j, g)
        else:
            bound = ref['numel'] * U * exact
            assert abs(g - exact) <= bound, '{} width {}: {!r} against {!r}, off by {:.3e} > {:.3e}'.format(
                what, j, g, exact, abs(g - exact), bound)


def _alloc_ref(errors, sizes, widths, sens, fixed, budget):
    """The allocation of include/dfq_hip.h on errors [T][B] (Python floats).  fixed[t]: a width or 0.  Returns a dict:
    bits, used, steps, cost, trace [(t, k, d, used after)], blocked: the walk ended on a step that did not fit while the next
    step of another tensor would have."""
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
    trace, blocked = [], False
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
            blocked = any(nxt[t][1] >= 0 and used + sizes[t] * (widths[nxt[t][1]] - widths[at[t]]) <= budget for t in range(T))
            break
        at[bt] = k
        used += d
        trace.append((bt, k, d, used))
        nxt[bt] = step(bt)
    cost = 0.0
    for t in range(T):
        cost += c[t][at[t]]
    return dict(bits=[widths[j] for j in at], used=used, steps=len(trace), cost=cost, trace=trace, blocked=blocked, c=c)


def _same_float(a, b):
    return np.float64(a).tobytes() == np.float64(b).tobytes() or (math.isnan(a) and math.isnan(b))


def _bits_of(a):
    return np.ascontiguousarray(a).view(np.int32)


# ---- networks ------------------------------------------------------------------------------------------------------------
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
    return OrderedDict((k, m.weight.detach().cpu().numpy().reshape(m.weight.shape[0], -1).copy()) for k, m in _targ(graph))


def _biases(graph):
    return {k: m.bias.detach().cpu().numpy().copy() for k, m in _targ(graph) if m.bias is not None}


_REFS = {}


def _net_ref(name, seed, pair, w0):
    """the exact errors of network (name, seed)'s equalised weights, computed once per (per_channel, signed)"""
    key = (name, seed, pair)
    if key not in _REFS:
        _REFS[key] = OrderedDict((k, _ref_tensor(w, pair[0], pair[1], WIDTHS)) for k, w in w0.items())
    return _REFS[key]


def _plan_alloc_ref(plan, n, sens=None, pin=None):
    """the restated allocation on network n's own errors"""
    errs = plan.errors(n)
    keys = list(errs)
    sizes = [plan._sizes[k] for k in keys]
    return _alloc_ref([errs[k].tolist() for k in keys], sizes, plan.widths, [(sens or {}).get(k, 1.0) for k in keys],
                      [(pin or {}).get(k, 0) for k in keys], plan.budget), keys


def _check_alloc(plan, n, sens=None, pin=None, what=''):
    ref, keys = _plan_alloc_ref(plan, n, sens, pin)
    bits, (used, steps), cost = plan.bits(n), plan.used(n), plan.cost(n)
    assert [bits[k] for k in keys] == ref['bits'], '{} net {}: bits'.format(what, n)
    assert (used, steps) == (ref['used'], ref['steps']), '{} net {}: used / steps'.format(what, n)
    assert _same_float(cost, ref['cost']), '{} net {}: cost {!r} against {!r}'.format(what, n, cost, ref['cost'])
    return ref


def _mixed(batch, nets, **kw):
    plan = batch.mixed_plan(WIDTHS, **kw)
    plan._sizes = {k: m.weight.numel() for k, m in _targ(nets[0][1])}
    return plan


# ---- 1. errors -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
@pytest.mark.parametrize('pair', PAIRS)
def test_errors_against_fsum_and_error_plan(engine, name, pair):
    per_channel, signed = pair
    nets, batch = _batch(name, SEEDS, engine.device)
    before = [_weights(g) for (_, g, _, _) in nets]
    plan = _mixed(batch, nets, avg_bits=4, per_channel=per_channel, signed=signed, apply=False)
    assert 2 <= plan.launches <= 3
    plan.run()
    _ffi.synchronize()
    ep = []
    for cfgs in (WIDTHS[:4], WIDTHS[4:]):
        e = batch.error_plan([(b, per_channel, signed) for b in cfgs])
        e.run()
        _ffi.synchronize()
        ep.append([e.errors(n) for n in range(len(SEEDS))])
        e.close()
    for n, seed in enumerate(SEEDS):
        refs = _net_ref(name, seed, pair, before[n])
        got = plan.errors(n)
        assert list(got) == list(refs)
        for k, ref in refs.items():
            what = '{} net {} {}'.format(name, n, k)
            assert got[k].dtype == np.float64 and got[k].shape == (len(WIDTHS),)
            _check_errors(got[k], ref, what)
            other = list(ep[0][n][k]['sum_sq']) + list(ep[1][n][k]['sum_sq'])
            for j in range(len(WIDTHS)):
                assert abs(got[k][j] - other[j]) <= ref['numel'] * U * ref['err'][j], what + ': against error_plan, width {}'.format(j)
        # apply=False: nothing written
        for k, w in _weights(nets[n][1]).items():
            assert np.array_equal(_bits_of(w), _bits_of(before[n][k])), k
    plan.close()


# ---- 2. the allocation, exactly ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
@pytest.mark.parametrize('pair', [(False, False), (True, True)])
def test_allocation_is_the_restated_walk(engine, name, pair):
    per_channel, signed = pair
    nets, batch = _batch(name, SEEDS, engine.device)
    keys = [k for k, _ in _targ(nets[0][1])]
    total = sum(m.weight.numel() for _, m in _targ(nets[0][1]))

    def run(**kw):
        plan = _mixed(batch, nets, per_channel=per_channel, signed=signed, apply=False, **kw)
        plan.run()
        _ffi.synchronize()
        return plan

    # the whole walk of network 0, from a budget above the all-highest size
    plan = run(budget_bits=total * WIDTHS[-1] + 1)
    full = [_check_alloc(plan, n, what='above') for n in range(len(SEEDS))]
    assert all(not r['blocked'] for r in full)
    assert plan.used(0)[0] <= total * WIDTHS[-1]
    trace = full[0]['trace']
    assert len(trace) >= 4, 'the walk of these networks is too short to place budgets in'
    plan.close()
    start = total * WIDTHS[0]
    mid = len(trace) // 2
    budgets = {'below the start': start - 1, 'the start': start, 'between steps': trace[mid][3] - 1, 'on a step': trace[mid][3],
               'one bit more': trace[mid][3] + 1, 'avg 4': None}
    for label, budget in budgets.items():
        plan = run(avg_bits=4) if budget is None else run(budget_bits=budget)
        if budget is None:
            assert plan.budget == 4 * total
        refs = [_check_alloc(plan, n, what=label) for n in range(len(SEEDS))]
        if label == 'below the start':
            assert all(plan.used(n) == (start, 0) for n in range(len(SEEDS))) and start > plan.budget
            assert all(set(plan.bits(n).values()) == {WIDTHS[0]} for n in range(len(SEEDS)))
        if label == 'on a step':                      # used + d == budget is taken
            assert plan.used(0) == (trace[mid][3], mid + 1)
        if label == 'between steps':
            assert plan.used(0) == (trace[mid - 1][3] if mid else start, mid)
        assert all(r['used'] <= plan.budget or r['steps'] == 0 for r in refs)
        plan.close()
    # the first and the last layer pinned to 8, one layer without sensitivity
    pin = {keys[0]: 8, keys[-1]: 8}
    sens = {keys[1]: 0.0, keys[2]: 3.5}
    plan = run(avg_bits=4.25, pin=pin, sensitivity=sens)
    assert plan.budget == (17 * total) // 4
    for n in range(len(SEEDS)):
        _check_alloc(plan, n, sens, pin, 'pinned')
        bits = plan.bits(n)
        assert bits[keys[0]] == 8 and bits[keys[-1]] == 8
        assert bits[keys[1]] == WIDTHS[0], 'a layer of sensitivity 0 takes no step (g is not > 0)'
    plan.close()


# ---- hand-made tensors through the C ABI ---------------------------------------------------------------------------------------
def _layout(shapes):
    """float offsets of the tensors in a network's slot, 16-byte aligned, four sentinel floats in between; the stride"""
    offs, at = [], 4
    for r, n in shapes:
        offs.append(at)
        at += -(-(r * n) // 4) * 4 + 4
    return offs, at


def _abi_run(engine, data, widths, per_row, signed, budget, apply=1, code_bytes=4, sens=None, fixed=None, runs=1):
    """the plan over len(data) networks; data[k]: the float32 [rows, n] tensors of network k -> dict of numpy blocks"""
    lib = _ffi.lib()
    n_nets, shapes = len(data), [x.shape for x in data[0]]
    T, B = len(shapes), len(widths)
    offs, stride = _layout(shapes)
    host = np.full((n_nets, stride), 7.5e5, dtype=F32)
    for k in range(n_nets):
        for x, o in zip(data[k], offs):
            host[k, o:o + x.size] = x.reshape(-1)
    store = torch.from_numpy(host.copy()).to(engine.device).contiguous()
    c_offs, r_offs, cs, rs = [], [], 0, 0
    for r, n in shapes:
        c_offs.append(cs + 1)
        cs += r * n + 2
        r_offs.append(rs + 1)
        rs += 2 * (r if per_row else 1) + 2
    dev = engine.device
    code_dtype = {4: torch.int32, 1: torch.int8 if signed else torch.uint8, 0: torch.int32}[code_bytes]
    blocks = dict(bits=torch.full((n_nets, T), -7, dtype=torch.int32, device=dev),
                  errors=torch.full((n_nets, T, B), 9.0, dtype=torch.float64, device=dev),
                  used=torch.full((n_nets, 2), -7, dtype=torch.int64, device=dev),
                  cost=torch.full((n_nets,), 9.0, dtype=torch.float64, device=dev),
                  codes=torch.full((n_nets, cs), 77, dtype=code_dtype, device=dev),
                  ranges=torch.full((n_nets, rs), 9.0, dtype=torch.float32, device=dev))
    base0 = store.data_ptr()
    P = _ffi.DfqBatchMixedTensor
    tabs = (P * T)(*[P(base0 + 4 * o, r, n, 1.0 if sens is None else sens[i], 0 if fixed is None else fixed[i], 0,
                       c_offs[i] if code_bytes else -1, r_offs[i]) for i, ((r, n), o) in enumerate(zip(shapes, offs))])
    cfg = _ffi.DfqBatchMixedConfig((ctypes.c_int32 * 8)(*widths), B, int(signed), int(per_row), int(apply), code_bytes, 0, budget)
    bases = (ctypes.c_void_p * n_nets)(*[base0 + 4 * k * stride for k in range(n_nets)])
    plan = ctypes.c_void_p()
    _ffi.check(lib.dfq_batch_mixed_plan_create(tabs, T, ctypes.byref(cfg), bases, n_nets, blocks['bits'].data_ptr(),
                                               blocks['errors'].data_ptr(), blocks['used'].data_ptr(), blocks['cost'].data_ptr(),
                                               blocks['codes'].data_ptr(), cs, blocks['ranges'].data_ptr(), rs, ctypes.byref(plan)))
    try:
        launches = lib.dfq_batch_mixed_plan_launches(plan)
        assert launches == 2 + int(bool(apply)) + int((not per_row) and any(r * n > _reg_elems() for r, n in shapes))
        for i in range(runs):
            _ffi.check(lib.dfq_batch_mixed_plan_run(plan, _ffi.stream_arg()))
            _ffi.synchronize()
            if i == 0:
                first = {k: v.clone() for k, v in blocks.items()}
        if not apply:
            for k, v in blocks.items():
                assert torch.equal(first[k].view(torch.uint8), v.view(torch.uint8)), 'two runs differ in ' + k
    finally:
        lib.dfq_batch_mixed_plan_destroy(plan)
    out = {k: v.cpu().numpy() for k, v in first.items()}
    out.update(store=store.cpu().numpy(), host=host, offs=offs, c_offs=c_offs, r_offs=r_offs, shapes=shapes, launches=launches)
    # the gaps between the tensors, and between the slots of the blocks, are as they were
    mask = np.ones(stride, dtype=bool)
    for (r, n), o in zip(shapes, offs):
        mask[o:o + r * n] = False
    assert (out['store'][:, mask] == 7.5e5).all(), 'a weight outside the tensors was written'
    cmask, rmask = np.ones(cs, dtype=bool), np.ones(rs, dtype=bool)
    for i, (r, n) in enumerate(shapes):
        cmask[c_offs[i]:c_offs[i] + r * n] = False
        rmask[r_offs[i]:r_offs[i] + 2 * (r if per_row else 1)] = False
    assert (out['codes'][:, cmask] == 77).all() and (out['ranges'][:, rmask] == 9.0).all(), 'something else in the blocks was touched'
    if not apply or not code_bytes:
        assert (out['codes'] == 77).all()
    if not apply:
        assert np.array_equal(_bits_of(out['store']), _bits_of(host)), 'apply = 0 wrote a weight'
    return out


def _reg_elems():
    return int(_ffi.lib().dfq_batch_quant_register_elements())


def _check_abi(out, data, widths, per_row, signed, budget, sens=None, fixed=None, code_bytes=4, apply=1, what=''):
    """errors against fsum, the allocation against the walk on the plan's own errors, and -- with apply -- weights, codes and
    ranges against the numpy quantiser at the chosen widths"""
    T = len(out['shapes'])
    refs_all = []
    for k in range(len(data)):
        refs = [_ref_tensor(x, per_row, signed, widths) for x in data[k]]
        refs_all.append(refs)
        for i, ref in enumerate(refs):
            _check_errors(out['errors'][k, i], ref, '{} net {} tensor {}'.format(what, k, i))
        al = _alloc_ref(out['errors'][k].tolist(), [x.size for x in data[k]], list(widths), sens or [1.0] * T, fixed or [0] * T, budget)
        assert out['bits'][k].tolist() == al['bits'], '{} net {}: bits {} against {}'.format(what, k, out['bits'][k].tolist(), al['bits'])
        assert out['used'][k].tolist() == [al['used'], al['steps']], '{} net {}'.format(what, k)
        assert _same_float(float(out['cost'][k]), al['cost']), '{} net {}: cost'.format(what, k)
        for i, ((r, n), ref) in enumerate(zip(out['shapes'], refs)):
            tag = '{} net {} tensor {}'.format(what, k, i)
            b = int(out['bits'][k, i])
            units = r if per_row else 1
            rg = out['ranges'][k, out['r_offs'][i]:out['r_offs'][i] + 2 * units].reshape(units, 2)
            assert np.array_equal(_bits_of(rg), _bits_of(ref['ranges'])), tag + ': ranges'
            got = out['store'][k, out['offs'][i]:out['offs'][i] + r * n].reshape(r, n)
            if not apply:
                continue
            want = ref['y'][b]
            same = (_bits_of(got) == _bits_of(want)) | (np.isnan(got) & np.isnan(want))
            assert same.all(), tag + ': stored weights at {} bits'.format(b)
            if code_bytes:
                q = ref['q'][b]
                ok = np.isfinite(q)
                codes = out['codes'][k, out['c_offs'][i]:out['c_offs'][i] + r * n].reshape(r, n).astype(np.int64)
                assert np.array_equal(codes[ok], q[ok].astype(np.int64)), tag + ': codes'
    return refs_all


def _rand(shapes, seed, scales=None):
    gen = np.random.default_rng(seed)
    return [(gen.standard_normal((r, n)) * (1.0 if scales is None else scales[i])).astype(F32) for i, (r, n) in enumerate(shapes)]


# ---- 3. optimality -------------------------------------------------------------------------------------------------------------
def test_no_cheaper_allocation_within_the_bits_used(engine):
    shapes, widths = [(8, 40), (1, 2000), (16, 9), (4, 600)], (2, 4, 8)
    data = [_rand(shapes, 11, scales=[1.0, 0.3, 4.0, 0.05])]
    sizes = [r * n for r, n in shapes]
    probe = _abi_run(engine, data, widths, False, False, sum(sizes) * 8, apply=0)
    full = _alloc_ref(probe['errors'][0].tolist(), sizes, list(widths), [1.0] * 4, [0] * 4, sum(sizes) * 8)
    # budgets one bit short of a step: the walk ends there; where a later step is small enough to fit, it must NOT be taken
    budgets, blocked = [], 0
    for (t, k, d, used) in full['trace']:
        ref = _alloc_ref(probe['errors'][0].tolist(), sizes, list(widths), [1.0] * 4, [0] * 4, used - 1)
        assert ref['used'] == used - d
        budgets.append(used - 1)
        blocked += ref['blocked']
    assert blocked >= 2, 'these tensors never end the walk on a step that does not fit while a cheaper one would'
    budgets += [sum(sizes) * 2, sum(sizes) * 8, full['trace'][2][3]]
    for budget in budgets:
        out = _abi_run(engine, data, widths, False, False, budget, apply=0)
        _check_abi(out, data, widths, False, False, budget, apply=0, what='budget {}'.format(budget))
        used, cost = int(out['used'][0, 0]), float(out['cost'][0])
        c = [[1.0 * float(e) for e in row] for row in out['errors'][0]]
        for choice in itertools.product(range(3), repeat=4):
            bits = sum(sizes[t] * widths[j] for t, j in enumerate(choice))
            total = 0.0
            for t, j in enumerate(choice):
                total += c[t][j]
            assert not (bits <= used and total < cost * (1.0 - 1e-12)), 'budget {}: {} takes {} <= {} bits and costs {} < {}'.format(
                budget, choice, bits, used, total, cost)


# ---- 4. the quantisation against the existing plan -----------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
@pytest.mark.parametrize('pair', [(False, False), (True, True)])
@pytest.mark.parametrize('codes', ['int32', 'int8'])
def test_quantised_like_quant_plan_at_each_width(engine, name, pair, codes):
    per_channel, signed = pair
    nets, batch = _batch(name, SEEDS, engine.device)
    before = [_weights(g) for (_, g, _, _) in nets]
    bias_before = [_biases(g) for (_, g, _, _) in nets]
    plan = _mixed(batch, nets, avg_bits=4.5, per_channel=per_channel, signed=signed, codes=codes)
    assert 3 <= plan.launches <= 4
    plan.run()
    _ffi.synchronize()
    bits = [plan.bits(n) for n in range(len(SEEDS))]
    occurring = sorted({b for d in bits for b in d.values()})
    assert len(occurring) >= 2, 'one width for everything: the test shows nothing'
    seen = 0
    for b in occurring:
        nets2, twin = _batch(name, SEEDS, engine.device)
        assert all(np.array_equal(_bits_of(a), _bits_of(c)) for a, c in zip(_weights(nets2[0][1]).values(), before[0].values())), 'twin'
        tp = twin.quant_plan(bit_weight=b, bits_bias=32, per_channel=per_channel, signed=signed, codes=codes)
        tp.run()
        _ffi.synchronize()
        for n in range(len(SEEDS)):
            got_w, want_w = _weights(nets[n][1]), _weights(nets2[n][1])
            got_c, want_c = plan.codes(n), tp.codes(n)
            got_r, want_r = plan.ranges(n), tp.ranges(n)
            for k, width in bits[n].items():
                if width != b:
                    continue
                seen += 1
                what = '{} net {} {} at {} bits'.format(name, n, k, b)
                assert np.array_equal(_bits_of(got_w[k]), _bits_of(want_w[k])), what + ': weight'
                assert got_c[k].dtype == want_c[k].dtype == (torch.int32 if codes == 'int32' else (torch.int8 if signed else torch.uint8))
                assert torch.equal(got_c[k].cpu(), want_c[k].cpu()), what + ': codes'
                assert np.array_equal(_bits_of(got_r[k].cpu().numpy()), _bits_of(want_r[k].cpu().numpy())), what + ': range'
        tp.close()
    assert seen == len(SEEDS) * len(bits[0])
    for n in range(len(SEEDS)):                        # weights only: the biases are as they were
        for k, bias in _biases(nets[n][1]).items():
            assert np.array_equal(_bits_of(bias), _bits_of(bias_before[n][k]))
    plan.close()
    with pytest.raises(RuntimeError):
        plan.run()


@pytest.mark.parametrize('pair', [(False, False), (True, True)])
def test_quantize_mixed_biases_are_quantize_s(engine, pair):
    per_channel, signed = pair
    name = 'tiny_mobile'
    nets, batch = _batch(name, SEEDS, engine.device)
    nets2, batch2 = _batch(name, SEEDS, engine.device)
    nets3, batch3 = _batch(name, SEEDS, engine.device)
    codes, ranges, bits = batch.quantize_mixed(WIDTHS, avg_bits=4, per_channel=per_channel, signed=signed, codes='int8', bits_bias=8)
    codes2, ranges2 = batch2.quantize(4, 8, per_channel=per_channel, signed=signed, codes='int8')
    plan = batch3.mixed_plan(WIDTHS, avg_bits=4, per_channel=per_channel, signed=signed, codes='int8')
    plan.run()
    _ffi.synchronize()
    assert len(codes) == len(ranges) == len(bits) == len(SEEDS)
    for n in range(len(SEEDS)):
        b1, b2 = _biases(nets[n][1]), _biases(nets2[n][1])
        assert sorted(b1) == sorted(b2) and b1
        for k in b1:
            assert np.array_equal(_bits_of(b1[k]), _bits_of(b2[k])), '{} net {} {}: bias'.format(name, n, k)
            assert np.array_equal(_bits_of(ranges[n][k + '.bias'].cpu().numpy()), _bits_of(ranges2[n][k + '.bias'].cpu().numpy()))
        assert sorted(ranges[n]) == sorted(ranges2[n])
        assert bits[n] == dict(plan.bits(n))
        w1, w3 = _weights(nets[n][1]), _weights(nets3[n][1])
        for k in w1:
            assert np.array_equal(_bits_of(w1[k]), _bits_of(w3[k])), k
            assert torch.equal(codes[n][k].cpu(), plan.codes(n)[k].cpu()), k
            assert np.array_equal(_bits_of(ranges[n][k].cpu().numpy()), _bits_of(plan.ranges(n)[k].cpu().numpy())), k
    plan.close()
    _, rng32, _ = batch2.quantize_mixed(WIDTHS, avg_bits=4, per_channel=per_channel, signed=signed, codes=None, bits_bias=32)
    assert not any(k.endswith('.bias') for k in rng32[0])


# ---- 5. shapes where the kernel can go wrong -----------------------------------------------------------------------------------
@pytest.mark.parametrize('signed', [False, True])
def test_row_shapes_through_the_abi(engine, signed):
    R = _reg_elems()
    shapes = [(7, 1), (37, 9), (5, 63), (9, 64), (3, 65), (2, R), (2, R + 1), (1, 130)]
    data = [_rand(shapes, 3 + k, scales=[1.0, 2.0, 0.5, 1.0, 3.0, 0.2, 1.0, 0.7]) for k in range(2)]
    total = sum(r * n for r, n in shapes)
    out = _abi_run(engine, data, WIDTHS, True, signed, 4 * total, code_bytes=1)
    _check_abi(out, data, WIDTHS, True, signed, 4 * total, code_bytes=1, what='rows')
    assert len(set(out['bits'][0].tolist())) >= 2


@pytest.mark.parametrize('signed', [False, True])
def test_tensor_shapes_through_the_abi(engine, signed):
    R = _reg_elems()
    shapes = [(1, R), (R + 1, 1), (3, 2 * 4096 // 3 + 1795), (1, 1), (4, 9), (1, 4096), (16, 257)]
    assert shapes[2][0] * shapes[2][1] > 2 * 4096 and (shapes[2][0] * shapes[2][1]) % 4096 != 0
    shapes.append((1, 3 * 4096 + 5))                   # a few flat pieces plus 5 elements
    data = [_rand(shapes, 20 + k, scales=[1.0, 0.5, 2.0, 1.0, 0.1, 1.0, 3.0, 0.4]) for k in range(2)]
    total = sum(r * n for r, n in shapes)
    out = _abi_run(engine, data, WIDTHS, False, signed, 5 * total)
    _check_abi(out, data, WIDTHS, False, signed, 5 * total, what='tensors')
    assert out['launches'] == 4 and len(set(out['bits'][0].tolist())) >= 2


def _snan():
    return np.array([0x7fa00001], dtype=np.uint32).view(F32)[0]


@pytest.mark.parametrize('per_row', [False, True])
@pytest.mark.parametrize('kind', ['constant', 'nan', 'snan', 'inf', 'neg_inf', 'neg_zero_row', 'all_nan'])
def test_special_values(engine, kind, per_row):
    R = _reg_elems()
    shapes = [(6, 40), (4, 50), (3, R + 7) if not per_row else (3, 70), (5, 33)]
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
    out = _abi_run(engine, data, WIDTHS, per_row, False, 5 * total)
    refs = _check_abi(out, data, WIDTHS, per_row, False, 5 * total, what=kind)
    err = out['errors'][1, victim]
    if kind in ('nan', 'snan', 'all_nan'):
        assert np.isnan(err).all(), 'a tensor holding NaN has NaN errors'
        assert out['bits'][1, victim] == WIDTHS[0], 'and stays at the lowest width'
    if kind == 'constant':                             # the max(scale, 1e-8) branch: (c - c) / 1e-8 = 0, and 0 * 1e-8 + c is c again
        assert refs[1][victim]['err'] == [0.0] * len(WIDTHS) and (err == 0).all()
        assert out['bits'][1, victim] == WIDTHS[0], 'nothing to gain: no step'
    if kind == 'neg_zero_row' and per_row:
        assert (out['ranges'][1, out['r_offs'][victim] + 4:out['r_offs'][victim] + 6] == 0).all()
    # the neighbours are unaffected: network 0 and the other tensors of network 1 are finite and equal a run without the victim
    clean = [_rand(shapes, 40 + k) for k in range(2)]
    base = _abi_run(engine, clean, WIDTHS, per_row, False, 5 * total)
    assert np.array_equal(out['errors'][0], base['errors'][0]) and np.array_equal(out['bits'][0], base['bits'][0])
    others = [i for i in range(len(shapes)) if i != victim]
    assert np.array_equal(out['errors'][1, others], base['errors'][1, others]) and np.isfinite(out['errors'][1, others]).all()


# ---- 6. determinism and independence -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pair', [(False, False), (True, True)])
def test_two_runs_and_a_network_s_place(engine, pair):
    per_channel, signed = pair
    name = 'tiny_cat'
    nets, batch = _batch(name, SEEDS, engine.device)
    plan = _mixed(batch, nets, avg_bits=4, per_channel=per_channel, signed=signed, apply=False)
    plan.run()
    _ffi.synchronize()
    first = [t.clone() for t in (plan.bits_block, plan.error_block, plan.used_block, plan.cost_block, plan.range_block)]
    plan.run()
    _ffi.synchronize()
    for a, b in zip(first, (plan.bits_block, plan.error_block, plan.used_block, plan.cost_block, plan.range_block)):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), 'two runs differ'
    nets1, batch1 = _batch(name, SEEDS[-1:], engine.device)
    alone = _mixed(batch1, nets1, avg_bits=4, per_channel=per_channel, signed=signed, apply=False)
    alone.run()
    _ffi.synchronize()
    last = len(SEEDS) - 1
    assert alone.bits(0) == plan.bits(last) and alone.used(0) == plan.used(last)
    for k, e in alone.errors(0).items():
        assert e.tobytes() == plan.errors(last)[k].tobytes(), k
    assert _same_float(alone.cost(0), plan.cost(last))
    plan.close()
    alone.close()
    # the ABI, with long tensors and two runs of every block
    shapes = [(3, 5000), (40, 9), (2, 1600)]
    data = [_rand(shapes, 60 + k) for k in range(3)]
    total = sum(r * n for r, n in shapes)
    three = _abi_run(engine, data, WIDTHS, per_channel, signed, 4 * total, apply=0, runs=2)
    one = _abi_run(engine, data[2:], WIDTHS, per_channel, signed, 4 * total, apply=0, runs=2)
    for k in ('bits', 'errors', 'used', 'cost', 'ranges'):
        assert one[k][0].tobytes() == three[k][2].tobytes(), k


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------
def test_abi_rejects_bad_arguments(engine):
    lib = _ffi.lib()
    dev = engine.device
    buf = torch.zeros(4096, dtype=torch.float32, device=dev)
    bits = torch.zeros(64, dtype=torch.int32, device=dev)
    errors = torch.zeros(64 * 8, dtype=torch.float64, device=dev)
    used = torch.zeros(16, dtype=torch.int64, device=dev)
    cost = torch.zeros(8, dtype=torch.float64, device=dev)
    codes = torch.zeros(4096, dtype=torch.int32, device=dev)
    ranges = torch.zeros(256, dtype=torch.float32, device=dev)
    P, Q = _ffi.DfqBatchMixedTensor, _ffi.DfqBatchMixedConfig

    def create(table=True, n_tensors=1, config=True, widths=(2, 4, 8), n_widths=None, data=0, rows=8, row_len=16, sens=1.0, fixed=0,
               code_off=0, range_off=0, budget=1000, code_bytes=4, bases=True, n_nets=2, base1=1024 * 4, blocks=(1, 1, 1, 1),
               codes_ptr=True, code_stride=1024, ranges_ptr=True, range_stride=64, place=True, per_row=1):
        plan = ctypes.c_void_p()
        w8 = list(widths) + [0] * (8 - len(widths))
        cfg = Q((ctypes.c_int32 * 8)(*w8[:8]), len(widths) if n_widths is None else n_widths, 0, per_row, 1, code_bytes, 0, budget)
        tabs = (P * max(n_tensors, 1))(*[P(buf.data_ptr() + data + 4 * 256 * i, rows, row_len, sens, fixed, 0, code_off, range_off)
                                         for i in range(max(n_tensors, 1))])
        ba = (ctypes.c_void_p * 2)(buf.data_ptr(), buf.data_ptr() + base1) if bases else None
        ptrs = [t.data_ptr() if on else None for t, on in zip((bits, errors, used, cost), blocks)]
        rc = lib.dfq_batch_mixed_plan_create(tabs if table else None, n_tensors, ctypes.byref(cfg) if config else None, ba, n_nets, *ptrs,
                                             codes.data_ptr() if codes_ptr else None, code_stride, ranges.data_ptr() if ranges_ptr else None,
                                             range_stride, ctypes.byref(plan) if place else None)
        return rc, plan

    def valid():
        rc, plan = create()
        assert rc == 0, lib.dfq_last_error()
        assert lib.dfq_batch_mixed_plan_launches(plan) == 3
        _ffi.check(lib.dfq_batch_mixed_plan_run(plan, _ffi.stream_arg()))
        _ffi.synchronize()
        lib.dfq_batch_mixed_plan_destroy(plan)
        assert bits.cpu()[:2].tolist() == [2, 2] and used.cpu()[:4].tolist() == [256, 0, 256, 0]     # (a tensor of zeros: no step)

    valid()
    bad = [dict(table=False), dict(n_tensors=0), dict(config=False), dict(place=False),
           dict(widths=(2,)), dict(widths=(2, 3, 4, 5, 6, 7, 8, 9), n_widths=9), dict(n_widths=0),
           dict(widths=(4, 2, 8)), dict(widths=(2, 4, 4)), dict(widths=(1, 4, 8)), dict(widths=(2, 4, 17)),
           dict(fixed=3), dict(fixed=-4), dict(sens=-1.0), dict(sens=math.inf), dict(sens=math.nan),
           dict(budget=-1), dict(code_bytes=2), dict(code_bytes=1, widths=(2, 4, 9)),
           dict(data=4), dict(base1=1024 * 4 + 8), dict(data=None),
           dict(rows=0), dict(row_len=0), dict(rows=-3),
           dict(code_off=1024 - 127), dict(code_off=-2), dict(range_off=64 - 15), dict(range_off=-2),
           dict(codes_ptr=False), dict(ranges_ptr=False), dict(code_bytes=0), dict(code_stride=-1), dict(range_stride=-1),
           dict(bases=False), dict(n_nets=0), dict(blocks=(0, 1, 1, 1)), dict(blocks=(1, 0, 1, 1)), dict(blocks=(1, 1, 0, 1)),
           dict(blocks=(1, 1, 1, 0)), dict(budget=-(2 ** 62))]
    for kw in bad:
        if kw.get('data', 0) is None:
            plan = ctypes.c_void_p()
            cfg = Q((ctypes.c_int32 * 8)(2, 4, 8, 0, 0, 0, 0, 0), 3, 0, 1, 1, 4, 0, 1000)
            ba = (ctypes.c_void_p * 2)(buf.data_ptr(), buf.data_ptr() + 4096)
            rc = lib.dfq_batch_mixed_plan_create((P * 1)(P(None, 8, 16, 1.0, 0, 0, 0, 0)), 1, ctypes.byref(cfg), ba, 2, bits.data_ptr(),
                                                 errors.data_ptr(), used.data_ptr(), cost.data_ptr(), codes.data_ptr(), 1024,
                                                 ranges.data_ptr(), 64, ctypes.byref(plan))
        else:
            rc, plan = create(**kw)
        assert rc == DFQ_ERR_ARG, kw
        assert b'dfq_batch_mixed_plan_create' in lib.dfq_last_error(), kw
        assert not plan.value, kw
        valid()
    # T * B beyond the allocation's table
    n = 4096 // 2 + 1
    big = (P * n)(*[P(buf.data_ptr(), 1, 4, 1.0, 0, 0, -1, -1) for _ in range(n)])
    cfg = Q((ctypes.c_int32 * 8)(2, 4, 0, 0, 0, 0, 0, 0), 2, 0, 0, 0, 0, 0, 10)
    ba = (ctypes.c_void_p * 1)(buf.data_ptr())
    wide = torch.zeros(n * 2, dtype=torch.float64, device=dev)
    plan = ctypes.c_void_p()
    rc = lib.dfq_batch_mixed_plan_create(big, n, ctypes.byref(cfg), ba, 1, wide.data_ptr(), wide.data_ptr(), used.data_ptr(), cost.data_ptr(),
                                         None, 0, None, 0, ctypes.byref(plan))
    assert rc == DFQ_ERR_ARG and b'4096' in lib.dfq_last_error()
    valid()
    assert lib.dfq_batch_mixed_plan_run(None, None) == DFQ_ERR_ARG
    assert b'dfq_batch_mixed_plan_run' in lib.dfq_last_error()
    assert lib.dfq_batch_mixed_plan_launches(None) == 0
    lib.dfq_batch_mixed_plan_destroy(None)
    valid()


def test_python_refusals(engine):
    nets, batch = _batch('tiny_res', [3], engine.device)
    keys = [k for k, _ in _targ(nets[0][1])]
    bad = [dict(), dict(avg_bits=4, budget_bits=100), dict(avg_bits=-1), dict(avg_bits=math.inf), dict(avg_bits=math.nan), dict(avg_bits='4'),
           dict(avg_bits=True), dict(budget_bits=-1), dict(budget_bits=4.0), dict(budget_bits=2 ** 63),
           dict(avg_bits=4, widths=(4,)), dict(avg_bits=4, widths=(2, 3, 4, 5, 6, 7, 8, 9, 10)), dict(avg_bits=4, widths=(4, 2)),
           dict(avg_bits=4, widths=(2, 2, 4)), dict(avg_bits=4, widths=(1, 4)), dict(avg_bits=4, widths=(4, 17)),
           dict(avg_bits=4, widths=(2.0, 4)), dict(avg_bits=4, widths=4), dict(avg_bits=4, codes='int16'),
           dict(avg_bits=4, codes='int8', widths=(2, 4, 9)), dict(avg_bits=4, pin={keys[0]: 5}), dict(avg_bits=4, pin={'nowhere': 4}),
           dict(avg_bits=4, sensitivity={keys[0]: -1.0}), dict(avg_bits=4, sensitivity={keys[0]: math.nan}),
           dict(avg_bits=4, sensitivity={keys[0]: math.inf}), dict(avg_bits=4, sensitivity={'nowhere': 1.0})]
    for kw in bad:
        with pytest.raises(ValueError):
            batch.mixed_plan(**kw)
        with pytest.raises(ValueError):
            batch.quantize_mixed(**kw)
        plan = batch.mixed_plan(avg_bits=4, apply=False)       # a valid plan still works
        plan.run()
        _ffi.synchronize()
        assert plan.used(0)[0] <= plan.budget
        plan.close()
    _, graph, _, _ = _prepared('tiny_res', 3, torch.device('cpu'))
    with pytest.raises(ValueError):
        dfq.quantize_mixed(graph, targ_type=TARG)
    with pytest.raises(ValueError):
        dfq.quantize_mixed(graph, avg_bits=4, pin={'nowhere': 4}, targ_type=TARG)
    with pytest.raises(ValueError):
        dfq.quantize_mixed(graph, avg_bits=4, targ_type=[torch.nn.LSTM])
    # avg_bits is taken at the float's own value, exactly
    total = sum(m.weight.numel() for _, m in _targ(nets[0][1]))
    from fractions import Fraction
    plan = batch.mixed_plan(avg_bits=4.3, apply=False)
    assert plan.budget == (Fraction(4.3) * total).__floor__() and plan.elements == total
    plan.close()
    plan = batch.mixed_plan(avg_bits=4)
    batch.release()
    with pytest.raises(RuntimeError):
        plan.run()
    with pytest.raises(RuntimeError):
        batch.mixed_plan(avg_bits=4)
    with pytest.raises(RuntimeError):
        batch.quantize_mixed(avg_bits=4)
    plan.close()


def test_struct_layout_matches_header():
    src = r'''
    #include <stdio.h>
    #include <stddef.h>
    #include "dfq_hip.h"
    #define T dfq_batch_mixed_tensor
    #define C dfq_batch_mixed_config
    int main(void) {
        printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu ", sizeof(T), offsetof(T, data), offsetof(T, rows), offsetof(T, row_len),
               offsetof(T, sensitivity), offsetof(T, fixed_bits), offsetof(T, pad), offsetof(T, code_offset), offsetof(T, range_offset));
        printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(C), offsetof(C, widths), offsetof(C, n_widths), offsetof(C, symmetric),
               offsetof(C, per_row), offsetof(C, apply), offsetof(C, code_bytes), offsetof(C, pad), offsetof(C, budget_bits));
        return 0;
    }'''
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, 't.c')
        open(c, 'w').write(src)
        exe = os.path.join(d, 't')
        subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), c, '-o', exe], check=True)
        got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    P, Q = _ffi.DfqBatchMixedTensor, _ffi.DfqBatchMixedConfig
    assert got == [ctypes.sizeof(P), P.data.offset, P.rows.offset, P.row_len.offset, P.sensitivity.offset, P.fixed_bits.offset,
                   P.pad.offset, P.code_offset.offset, P.range_offset.offset,
                   ctypes.sizeof(Q), Q.widths.offset, Q.n_widths.offset, Q.symmetric.offset, Q.per_row.offset, Q.apply.offset,
                   Q.code_bytes.offset, Q.pad.offset, Q.budget_bits.offset]


# ---- 8. the single network -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pair', [(False, False), (True, True)])
def test_single_network_equals_the_batch_of_one(engine, pair):
    per_channel, signed = pair
    name, seed = 'tiny_mobile', 1
    nets, batch = _batch(name, [seed], engine.device)
    keys = [k for k, _ in _targ(nets[0][1])]
    pin, sens = {keys[0]: 8}, {keys[2]: 2.0}
    plan = batch.mixed_plan(WIDTHS, avg_bits=4.5, per_channel=per_channel, signed=signed, sensitivity=sens, pin=pin)
    plan.run()
    _ffi.synchronize()
    want_bits, want_err, want_rng = plan.bits(0), plan.errors(0), {k: v.cpu().numpy() for k, v in plan.ranges(0).items()}
    want_w = _weights(nets[0][1])
    plan.close()
    _, graph, _, rels = _prepared(name, seed, torch.device('cpu'))
    dfq.cross_layer_equalization(graph, rels, TARG)
    got = dfq.quantize_mixed(graph, WIDTHS, avg_bits=4.5, per_channel=per_channel, signed=signed, sensitivity=sens, pin=pin, targ_type=TARG)
    assert list(got) == keys and got[keys[0]]['bits'] == 8
    assert len({v['bits'] for v in got.values()}) >= 2
    for k in keys:
        assert sorted(got[k]) == ['bits', 'err', 'range']
        assert got[k]['bits'] == want_bits[k], k
        assert _same_float(got[k]['err'], float(want_err[k][WIDTHS.index(want_bits[k])])), k
        assert np.array_equal(_bits_of(got[k]['range']), _bits_of(want_rng[k])), k
    for k, w in _weights(graph).items():
        assert graph[k].weight.device.type == 'cpu'
        assert np.array_equal(_bits_of(w), _bits_of(want_w[k])), k
