"""NetworkBatch.nsr_plan / mixed_plan(costs=) / quantize_mixed(cost='nsr') / dfq_batch_nsr_plan_* /
dfq_batch_mixed_plan_set_costs: data-free layer sensitivities, and the mixed-precision allocation on them.

The references are numpy and plain Python, in this file, by the definition in include/dfq_hip.h:
  moments   per source the (mean, var) of dfq_relu_moments itself (mode 1 behind a ReLU, else 0; a source without gamma~:
            (beta~, 0)), merged with float32 numpy additions (add) or concatenation (cat), clamped, and for the second moment
            formed in float64 and rounded once: bit for bit.
  rows      e = Q(w) - w in float32 by the quantiser recipe of tests/test_batch_mixed.py; Ne = sum a e^2 and S = sum a w^2 in
            exact rational arithmetic (fractions.Fraction) over the float32 a, e and w.  The plan rounds every product once and
            adds the L = row_len non-negative terms of each sum in float64 in some order, then divides once, so
            |got - Ne / S| <= gamma_{2L+1} Ne / S with gamma_k = k u / (1 - k u), u = 2^-53 (Higham, Lemma 3.1 and (4.4)), and
            |S_got - S| <= gamma_L S.  NaN matches NaN, and R = 0 exactly where S = 0.
  fold      the sequential float64 sum, in rising o, of the plan's OWN rows: bit for bit.
  set_costs the greedy walk of tests/test_batch_mixed.py restated, fed the costs the plan was given."""
import ctypes
import math
from collections import OrderedDict
from fractions import Fraction

import numpy as np
import pytest
import torch

from dfq_amd import _ffi, arena, dfq, synthetic
from dfq_amd.utils import layer_transform as lt
from dfq_amd.utils import relation as rel

from common import TARG

DFQ_ERR_ARG = -1     # include/dfq_hip.h
F32 = np.float32
U = 2.0 ** -53
WIDTHS = (2, 3, 4, 6, 8)
NAMES = ['tiny_mobile', 'tiny_res', 'tiny_cat']
SEEDS = [0, 1, 2]
PAIRS = [(False, False), (True, True), (True, False)]        # (per_channel, signed), as tests/test_batch_mixed.py
SENT = 7.5e5


def _gamma(k):
    return k * U / (1.0 - k * U)


# ---- the quantiser, as tests/test_batch_mixed.py states it -------------------------------------------------------------------
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
    """Q(w) float32 for w [units, n] and one parameter tuple per unit: quantize.py:70-74, five float32 roundings"""
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
    assert y.dtype == F32
    return y


def _unit_range(x):
    """(mn, mx) of a unit by the house rule: NaN skipped, nothing but NaN keeps the identities (+inf, -inf)"""
    ok = ~np.isnan(x)
    return (F32(x[ok].min()), F32(x[ok].max())) if ok.any() else (F32(np.inf), F32(-np.inf))


def _errors(w, per_row, signed, widths):
    """e [B, rows, row_len] float32"""
    x = w if per_row else w.reshape(1, -1)
    rng = [_unit_range(r) for r in x]
    out = []
    for b in widths:
        y = _fake_quant(x, [_qparams(mn, mx, b, signed) for mn, mx in rng])
        with np.errstate(all='ignore'):
            out.append((y - x).reshape(w.shape))
    return np.stack(out)


def _alloc_ref(costs, sizes, widths, sens, fixed, budget):
    """The allocation of include/dfq_hip.h on costs [T][B] (Python floats); fixed[t]: a width or 0 (tests/test_batch_mixed.py)"""
    T, B = len(sizes), len(widths)
    c = [[float(sens[t]) * float(costs[t][j]) for j in range(B)] for t in range(T)]
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
    steps = 0
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
        steps += 1
        nxt[bt] = step(bt)
    cost = 0.0
    for t in range(T):
        cost += c[t][at[t]]
    return dict(bits=[widths[j] for j in at], used=used, steps=steps, cost=cost)


def _same_float(a, b):
    return np.float64(a).tobytes() == np.float64(b).tobytes() or (math.isnan(a) and math.isnan(b))


def _bits_of(a):
    return np.ascontiguousarray(a).view(np.int32)


def _reg_elems():
    return int(_ffi.lib().dfq_batch_quant_register_elements())


# ---- the definition: moments and rows ------------------------------------------------------------------------------------------
def _relu_moments(engine, fw, fb, mode):
    """(mean, var) float32 numpy of dfq_relu_moments itself"""
    dev = engine.device
    w, b = torch.from_numpy(fw.copy()).to(dev), torch.from_numpy(fb.copy()).to(dev)
    mean, var = torch.zeros_like(w), torch.zeros_like(w)
    _ffi.check(_ffi.lib().dfq_relu_moments(w.data_ptr(), b.data_ptr(), w.numel(), mode, mean.data_ptr(), var.data_ptr(), 0, _ffi.stream_arg()))
    _ffi.synchronize()
    return mean.cpu().numpy(), var.cpu().numpy()


def _ref_moments(engine, srcs, channels, moment, input_moment):
    """srcs: [(fw or None, fb, relu, concat)] float32 numpy vectors -> a float32 [channels]"""
    if not srcs:
        return np.full(channels, input_moment, dtype=F32)
    mean = var = None
    for m, (fw, fb, relu, concat) in enumerate(srcs):
        if fw is None:
            mu, v = fb.copy(), np.zeros_like(fb)
        else:
            mu, v = _relu_moments(engine, fw, fb, 1 if relu else 0)
        with np.errstate(all='ignore'):
            if m == 0:
                mean, var = mu, v
            elif concat:
                mean, var = np.concatenate([mean, mu]), np.concatenate([var, v])
            else:
                mean, var = mean + mu, var + v
        assert mean.dtype == F32 and var.dtype == F32
    assert mean.size == channels
    vc = np.where(var < 0, F32(0), var)
    if moment == 0:
        return vc.astype(F32)
    with np.errstate(all='ignore'):
        return (mean.astype(np.float64) * mean.astype(np.float64) + vc.astype(np.float64)).astype(F32)


def _frac(v):
    return Fraction(float(v))


def _ref_rows(w, a, e, ipg, klen, groups):
    """exact (R [rows][B], S [rows]) as Fractions, None where NaN; w [rows, len], a [channels] float32, e [B, rows, len]"""
    rows, length = w.shape
    rpg = rows // groups
    R, S = [], []
    for o in range(rows):
        ch = (o // rpg) * ipg + np.arange(length) // klen
        ao = a[ch]
        if np.isnan(ao).any() or np.isnan(w[o]).any():
            R.append([None] * e.shape[0])
            S.append(None)
            continue
        af = [_frac(v) for v in ao]
        s = sum(x * _frac(v) ** 2 for x, v in zip(af, w[o]))
        S.append(s)
        R.append([Fraction(0) if s == 0 else sum(x * _frac(v) ** 2 for x, v in zip(af, e[j, o])) / s for j in range(e.shape[0])])
    return R, S


# ---- hand-made tensors through the C ABI ---------------------------------------------------------------------------------------
# a tensor: (rows, input channels per group, K, groups, source kind); the kinds:
KINDS = {'none': [], 'one': [(1, 0, 0)], 'one_relu': [(1, 1, 0)], 'no_gamma': [(0, 0, 0)], 'add': [(1, 1, 0), (1, 0, 0)],
         'add_relu': [(1, 0, 0), (1, 1, 0)], 'cat': [(1, 1, 0), (1, 0, 1)], 'cat_add': [(1, 0, 0), (1, 1, 1), (1, 0, 0)]}
# (has gamma~, relu, concat) per source; a `cat` source takes the upper half of the channels, an add behind it all of them


def _source_channels(kind, channels):
    out, have = [], 0
    spec = KINDS[kind]
    n_cat = sum(1 for s in spec if s[2])
    for m, (_, _, concat) in enumerate(spec):
        if m == 0:
            have = channels - (channels // 2 if n_cat else 0)
            out.append(have)
        elif concat:
            out.append(channels // 2)
            have += channels // 2
        else:
            out.append(have)
    return out


def _make(specs, n_nets, seed, edit=None):
    """the weights and proxies of n_nets networks: data[k][i] float32 [rows, len]; prox[k][i] = [(fw or None, fb, relu, concat)]"""
    gen = np.random.default_rng(seed)
    data, prox = [], []
    for k in range(n_nets):
        ws, ps = [], []
        for (rows, ipg, klen, groups, kind) in specs:
            ws.append((gen.standard_normal((rows, ipg * klen)) * gen.uniform(0.2, 3.0)).astype(F32))
            srcs = []
            for (has_fw, relu, concat), ch in zip(KINDS[kind], _source_channels(kind, ipg * groups)):
                fw = gen.uniform(0.05, 2.0, ch).astype(F32) if has_fw else None
                srcs.append((fw, gen.standard_normal(ch).astype(F32), relu, concat))
            ps.append(srcs)
        data.append(ws)
        prox.append(ps)
    if edit:
        edit(data, prox)
    return data, prox


def _nsr_abi(engine, specs, data, prox, widths, per_row, signed, moment=0, input_moment=1.0, with_signal=True, runs=2):
    """the plan over len(data) networks -> dict of numpy blocks (sentinels checked) and the layout"""
    lib = _ffi.lib()
    n_nets, T, B = len(data), len(specs), len(widths)
    # one network's slot: weights at 16-byte aligned offsets, four sentinel floats in between, then the proxies
    offs, at = [], 4
    for (rows, ipg, klen, groups, kind) in specs:
        offs.append(at)
        at += -(-(rows * ipg * klen) // 4) * 4 + 4
    poffs = []
    for i, (rows, ipg, klen, groups, kind) in enumerate(specs):
        mine = []
        for ch in _source_channels(kind, ipg * groups):
            mine.append((at, at + ch))
            at += 2 * ch
        poffs.append(mine)
    stride = -(-at // 4) * 4
    host = np.full((n_nets, stride), SENT, dtype=F32)
    for k in range(n_nets):
        for i, x in enumerate(data[k]):
            host[k, offs[i]:offs[i] + x.size] = x.reshape(-1)
            for (fw, fb, _, _), (ow, ob) in zip(prox[k][i], poffs[i]):
                if fw is not None:
                    host[k, ow:ow + fw.size] = fw
                host[k, ob:ob + fb.size] = fb
    dev = engine.device
    store = torch.from_numpy(host.copy()).to(dev).contiguous()
    base0 = store.data_ptr()
    src_rows, ranges = [], []
    for i, (rows, ipg, klen, groups, kind) in enumerate(specs):
        ranges.append((len(src_rows), len(KINDS[kind])))
        for (has_fw, relu, concat), ch, (ow, ob) in zip(KINDS[kind], _source_channels(kind, ipg * groups), poffs[i]):
            src_rows.append(_ffi.DfqBcSource(base0 + 4 * ow if has_fw else None, base0 + 4 * ob, ch, relu, concat))
    sources = (_ffi.DfqBcSource * max(len(src_rows), 1))(*src_rows)
    m_offs, r_offs, ms, rs = [], [], 3, 2
    for (rows, ipg, klen, groups, kind) in specs:
        m_offs.append(ms)
        ms += ipg * groups + 3
        r_offs.append(rs)
        rs += rows + 2
    blocks = dict(moments=torch.full((n_nets, ms), SENT, dtype=torch.float32, device=dev),
                  rows=torch.full((n_nets, rs, B), SENT, dtype=torch.float64, device=dev),
                  signal=torch.full((n_nets, rs), SENT, dtype=torch.float64, device=dev),
                  costs=torch.full((n_nets * T * B + 8,), SENT, dtype=torch.float64, device=dev))
    P = _ffi.DfqBatchNsrTensor
    tabs = (P * T)(*[P(base0 + 4 * offs[i], rows, ipg * klen, klen, groups, ranges[i][0], ranges[i][1], 0, m_offs[i], r_offs[i])
                     for i, (rows, ipg, klen, groups, kind) in enumerate(specs)])
    cfg = _ffi.DfqBatchNsrConfig((ctypes.c_int32 * 8)(*(list(widths) + [0] * (8 - B))), B, int(signed), int(per_row), moment, input_moment, 0)
    bases = (ctypes.c_void_p * n_nets)(*[base0 + 4 * k * stride for k in range(n_nets)])
    plan = ctypes.c_void_p()
    _ffi.check(lib.dfq_batch_nsr_plan_create(tabs, T, sources, len(src_rows), ctypes.byref(cfg), bases, n_nets, blocks['moments'].data_ptr(), ms,
                                             blocks['rows'].data_ptr(), blocks['signal'].data_ptr() if with_signal else None, rs,
                                             blocks['costs'].data_ptr() + 8 * 4, ctypes.byref(plan)))
    try:
        assert lib.dfq_batch_nsr_plan_launches(plan) == (3 if per_row else 4)
        for i in range(runs):
            _ffi.check(lib.dfq_batch_nsr_plan_run(plan, _ffi.stream_arg()))
            _ffi.synchronize()
            if i == 0:
                first = {k: v.clone() for k, v in blocks.items()}
        for k, v in blocks.items():
            assert torch.equal(first[k].view(torch.uint8), v.view(torch.uint8)), 'two runs differ in ' + k
    finally:
        lib.dfq_batch_nsr_plan_destroy(plan)
    out = {k: v.cpu().numpy() for k, v in first.items()}
    assert np.array_equal(_bits_of(store.cpu().numpy()), _bits_of(host)), 'the plan wrote a weight or a proxy'
    # nothing outside the declared slots
    mmask, rmask = np.ones(ms, dtype=bool), np.ones(rs, dtype=bool)
    for i, (rows, ipg, klen, groups, kind) in enumerate(specs):
        mmask[m_offs[i]:m_offs[i] + ipg * groups] = False
        rmask[r_offs[i]:r_offs[i] + rows] = False
    assert (out['moments'][:, mmask] == SENT).all() and (out['rows'][:, rmask] == SENT).all(), 'something else in the blocks was touched'
    assert (out['signal'][:, rmask] == SENT).all() if with_signal else (out['signal'] == SENT).all()
    assert (out['costs'][:4] == SENT).all() and (out['costs'][-4:] == SENT).all()
    out['costs'] = out['costs'][4:-4].reshape(n_nets, T, B)
    out.update(m_offs=m_offs, r_offs=r_offs)
    return out


def _check_nsr(engine, out, specs, data, prox, widths, per_row, signed, moment=0, input_moment=1.0, with_signal=True, what=''):
    B = len(widths)
    for k in range(len(data)):
        for i, (rows, ipg, klen, groups, kind) in enumerate(specs):
            tag = '{} net {} tensor {} {}'.format(what, k, i, specs[i])
            ch = ipg * groups
            a = out['moments'][k, out['m_offs'][i]:out['m_offs'][i] + ch]
            want = _ref_moments(engine, prox[k][i], ch, moment, F32(input_moment))
            assert np.array_equal(_bits_of(a), _bits_of(want)) or (np.isnan(a) == np.isnan(want)).all() and np.array_equal(
                _bits_of(a)[~np.isnan(a)], _bits_of(want)[~np.isnan(a)]), tag + ': moments'
            w = data[k][i]
            e = _errors(w, per_row, signed, widths)
            R, S = _ref_rows(w, a, e, ipg, klen, groups)
            got = out['rows'][k, out['r_offs'][i]:out['r_offs'][i] + rows]
            sig = out['signal'][k, out['r_offs'][i]:out['r_offs'][i] + rows]
            L = ipg * klen
            for o in range(rows):
                if S[o] is None:
                    assert np.isnan(got[o]).all() and (not with_signal or math.isnan(sig[o])), tag + ': row {} is not NaN'.format(o)
                    continue
                if with_signal:
                    assert abs(Fraction(float(sig[o])) - S[o]) <= Fraction(_gamma(L)) * S[o], tag + ': signal of row {}'.format(o)
                for j in range(B):
                    g = float(got[o, j])
                    if S[o] == 0:
                        assert g == 0.0 and not math.copysign(1.0, g) < 0, tag + ': S = 0 but R = {!r}'.format(g)
                    else:
                        assert not math.isnan(g), tag
                        err, bound = abs(Fraction(g) - R[o][j]), Fraction(_gamma(2 * L + 1)) * R[o][j]
                        assert err <= bound, tag + ': row {} width {}: {!r} against {!r}, off by {:.3e} > {:.3e}'.format(
                            o, j, g, float(R[o][j]), float(err), float(bound))
            # the fold: the sequential sum of the plan's own rows
            for j in range(B):
                s = 0.0
                for o in range(rows):
                    s += float(got[o, j])
                assert _same_float(float(out['costs'][k, i, j]), s), tag + ': fold, width {}'.format(j)


def _shape_specs():
    R = _reg_elems()
    assert R == 1536, 'the lane classes below are laid out for 64 lanes x 24 slots'
    return [
        (7, 1, 1, 1, 'one'),             # row length 1
        (5, 3, 1, 1, 'cat'),             # 3
        (37, 1, 9, 37, 'one_relu'),      # depthwise: I/g = 1, K = 9, a row set that is not full
        (6, 4, 9, 2, 'add'),             # 4 * 9 with g = 2
        (3, 16, 1, 1, 'none'), (3, 17, 1, 1, 'one'),           # L = 4 | 8
        (19, 32, 1, 1, 'add_relu'), (3, 33, 1, 1, 'cat'),      # L = 8 | 16
        (5, 64, 1, 1, 'one'), (5, 65, 1, 1, 'no_gamma'),       # L = 16 | 32
        (3, 128, 1, 1, 'cat_add'), (2, 129, 1, 1, 'one_relu'),  # L = 32 | 64
        (1, 3, 9, 1, 'none'),            # rows = 1, the first convolution: input_moment
        (2, R, 1, 1, 'one'), (2, R + 1, 1, 1, 'one_relu'),     # the longest row in registers | the looping wave, scalar
        (1, (R + 4) // 4, 4, 1, 'add'),  # the looping wave, 16-byte loads, K = 4
        (2, 171, 9, 1, 'one'),           # 1539 = 171 * 9: the looping wave with K = 9
    ]


@pytest.mark.parametrize('per_row,signed,widths', [(True, False, WIDTHS), (False, True, WIDTHS), (True, True, (4,)),
                                                   (False, False, (3, 8)), (True, False, (2, 3, 4, 5, 6, 7, 8, 16))])
def test_row_shapes_through_the_abi(engine, per_row, signed, widths):
    specs = _shape_specs()
    if len(widths) == 8:                               # (exact arithmetic over eight widths: the short rows)
        specs = [s for s in specs if s[1] * s[2] <= 129]
    data, prox = _make(specs, 2, 5)
    out = _nsr_abi(engine, specs, data, prox, widths, per_row, signed, input_moment=0.75)
    _check_nsr(engine, out, specs, data, prox, widths, per_row, signed, input_moment=0.75, what='shapes')
    assert (out['costs'] >= 0).all() and (out['costs'][:, 3] > 0).all()


@pytest.mark.parametrize('moment', [0, 1])
def test_moments_and_both_modes(engine, moment):
    specs = [(4, 6, 1, 1, kind) for kind in KINDS] + [(8, 2, 9, 4, 'cat'), (8, 2, 9, 4, 'add'), (3, 700, 1, 1, 'one_relu')]

    def edit(data, prox):                              # a ReLU channel far below zero: its variance cancels to <= 0 or just above
        prox[0][2][0][1][0] = F32(-30.0)
        prox[1][4][0][1][2] = F32(-12.0)
    data, prox = _make(specs, 2, 9, edit)
    out = _nsr_abi(engine, specs, data, prox, (2, 4, 8), True, False, moment=moment, input_moment=2.5, with_signal=False)
    _check_nsr(engine, out, specs, data, prox, (2, 4, 8), True, False, moment=moment, input_moment=2.5, with_signal=False, what='moments')
    a = out['moments'][0, out['m_offs'][0]:out['m_offs'][0] + 6]
    assert (a == F32(2.5)).all()
    assert (out['moments'][:, [m for i, m0 in enumerate(out['m_offs']) for m in range(m0, m0 + specs[i][1] * specs[i][3])]] >= 0).all()


@pytest.mark.parametrize('per_row', [False, True])
def test_special_values(engine, per_row):
    specs = [(6, 8, 1, 1, 'one'), (4, 5, 9, 1, 'one_relu'), (8, 2, 1, 4, 'no_gamma'), (3, 40, 1, 1, 'add'), (4, 200, 1, 1, 'one')]

    def edit(data, prox):
        data[1][0][2, 3] = np.nan                      # a NaN weight
        prox[1][1][0][1][2] = np.nan                   # a NaN beta~: channel 2 of tensor 1
        data[1][3][1, :] = F32(0.375)                  # a constant row
        data[0][4][:] = F32(-1.25)                     # a constant tensor: scale = 1e-8, e = 0
    data, prox = _make(specs, 2, 13, edit)
    out = _nsr_abi(engine, specs, data, prox, WIDTHS, per_row, False)
    _check_nsr(engine, out, specs, data, prox, WIDTHS, per_row, False, what='special')
    ro = out['r_offs']
    # 'no_gamma': var = 0 everywhere, so a = 0, S = 0 and R = 0
    assert (out['rows'][:, ro[2]:ro[2] + 8] == 0).all() and (out['signal'][:, ro[2]:ro[2] + 8] == 0).all() and (out['costs'][:, 2] == 0).all()
    # the NaN weight: its row, and with per-tensor ranges nothing more (the range skips it); the tensor's costs are NaN
    nan_rows = np.isnan(out['rows'][1, ro[0]:ro[0] + 6]).all(axis=1)
    assert nan_rows.tolist() == [False, False, True, False, False, False] and np.isnan(out['costs'][1, 0]).all()
    # the NaN moment: every row of tensor 1 reads channel 2
    assert np.isnan(out['rows'][1, ro[1]:ro[1] + 4]).all() and np.isnan(out['costs'][1, 1]).all()
    assert (out['rows'][0, ro[4]:ro[4] + 4] == 0).all(), 'a constant tensor has e = 0'
    if per_row:
        assert (out['rows'][1, ro[3] + 1] == 0).all(), 'a constant row has e = 0'
    # nothing else is touched by the NaNs: network 0 and the other tensors of network 1 equal a run without them
    clean_data, clean_prox = _make(specs, 2, 13, lambda d, p: d[0][4].fill(F32(-1.25)))
    base = _nsr_abi(engine, specs, clean_data, clean_prox, WIDTHS, per_row, False)
    assert np.array_equal(out['costs'][0], base['costs'][0]) and np.array_equal(out['rows'][0], base['rows'][0])
    assert np.array_equal(out['costs'][1, [2, 4]], base['costs'][1, [2, 4]]) and np.isfinite(out['costs'][1, 2:]).all()


def test_a_network_s_place_in_the_batch(engine):
    specs = [(9, 20, 1, 1, 'cat'), (16, 1, 9, 16, 'one_relu'), (2, 1600, 1, 1, 'add'), (5, 3, 9, 1, 'none')]
    data, prox = _make(specs, 3, 21)
    for per_row in (False, True):
        three = _nsr_abi(engine, specs, data, prox, WIDTHS, per_row, True)
        perm = [2, 0, 1]
        moved = _nsr_abi(engine, specs, [data[p] for p in perm], [prox[p] for p in perm], WIDTHS, per_row, True)
        one = _nsr_abi(engine, specs, data[1:2], prox[1:2], WIDTHS, per_row, True)
        for key in ('moments', 'rows', 'signal', 'costs'):
            for place, p in enumerate(perm):
                assert moved[key][place].tobytes() == three[key][p].tobytes(), key
            assert one[key][0].tobytes() == three[key][1].tobytes(), key


def test_abi_rejects_bad_arguments(engine):
    lib = _ffi.lib()
    dev = engine.device
    buf = torch.ones(4096, dtype=torch.float32, device=dev)
    moments = torch.zeros(256, dtype=torch.float32, device=dev)
    rows = torch.zeros(64 * 8, dtype=torch.float64, device=dev)
    signal = torch.zeros(64, dtype=torch.float64, device=dev)
    costs = torch.zeros(64, dtype=torch.float64, device=dev)
    P, Q, S = _ffi.DfqBatchNsrTensor, _ffi.DfqBatchNsrConfig, _ffi.DfqBcSource

    def create(table=True, n_tensors=1, srcs=True, n_sources=2, config=True, widths=(2, 4, 8), n_widths=None, data=0, rows_=8, row_len=18,
               klen=9, groups=2, begin=0, count=2, ch=(4, 4), concat=0, fb=True, moment=0, input_moment=1.0, m_off=0, r_off=0, bases=True,
               n_nets=2, base1=1024 * 4, blocks=(1, 1, 1), m_stride=64, r_stride=16, place=True):
        plan = ctypes.c_void_p()
        w8 = list(widths) + [0] * (8 - len(widths))
        cfg = Q((ctypes.c_int32 * 8)(*w8[:8]), len(widths) if n_widths is None else n_widths, 0, 1, moment, input_moment, 0)
        tabs = (P * max(n_tensors, 1))(*[P(None if data is None else buf.data_ptr() + data + 4 * 256 * i, rows_, row_len, klen, groups, begin,
                                           count, 0, m_off, r_off) for i in range(max(n_tensors, 1))])
        sa = (S * 2)(S(buf.data_ptr() + 4 * 600, buf.data_ptr() + 4 * 700 if fb else None, ch[0], 1, 0),
                     S(buf.data_ptr() + 4 * 800, buf.data_ptr() + 4 * 900, ch[1], 0, concat))
        ba = (ctypes.c_void_p * 2)(buf.data_ptr(), buf.data_ptr() + base1) if bases else None
        ptrs = [t.data_ptr() if on else None for t, on in zip((moments, rows, costs), blocks)]
        rc = lib.dfq_batch_nsr_plan_create(tabs if table else None, n_tensors, sa if srcs else None, n_sources, ctypes.byref(cfg) if config else None,
                                           ba, n_nets, ptrs[0], m_stride, ptrs[1], signal.data_ptr(), r_stride, ptrs[2],
                                           ctypes.byref(plan) if place else None)
        return rc, plan

    def valid(**kw):
        rc, plan = create(**kw)
        assert rc == 0, lib.dfq_last_error()
        assert lib.dfq_batch_nsr_plan_launches(plan) == 3
        _ffi.check(lib.dfq_batch_nsr_plan_run(plan, _ffi.stream_arg()))
        _ffi.synchronize()
        lib.dfq_batch_nsr_plan_destroy(plan)

    valid()
    valid(count=0, n_sources=0, srcs=False)            # no sources at all: input_moment everywhere
    valid(widths=(4,))
    valid(ch=(2, 2), concat=1)
    valid(input_moment=0.0)
    bad = [dict(table=False), dict(n_tensors=0), dict(config=False), dict(place=False), dict(srcs=False), dict(n_sources=-1),
           dict(n_widths=0), dict(widths=(2, 3, 4, 5, 6, 7, 8, 9), n_widths=9), dict(widths=(4, 2, 8)), dict(widths=(2, 4, 4)),
           dict(widths=(1, 4, 8)), dict(widths=(2, 4, 17)),
           dict(klen=4), dict(klen=0), dict(groups=3), dict(groups=0), dict(ch=(4, 3)), dict(ch=(3, 3)), dict(ch=(4, 4), concat=1),
           dict(ch=(2, 3), concat=1), dict(count=1, ch=(3, 4)), dict(begin=1, count=2), dict(count=3), dict(begin=-1), dict(count=-1),
           dict(fb=False), dict(ch=(0, 4)),
           dict(input_moment=-1.0), dict(input_moment=math.inf), dict(input_moment=math.nan), dict(moment=2), dict(moment=-1),
           dict(data=4), dict(data=None), dict(base1=1024 * 4 + 8),
           dict(rows_=0), dict(row_len=0), dict(rows_=-2),
           dict(m_off=64 - 3), dict(m_off=-1), dict(r_off=16 - 7), dict(r_off=-1), dict(m_stride=-1), dict(r_stride=-1),
           dict(bases=False), dict(n_nets=0), dict(blocks=(0, 1, 1)), dict(blocks=(1, 0, 1)), dict(blocks=(1, 1, 0))]
    for kw in bad:
        rc, plan = create(**kw)
        assert rc == DFQ_ERR_ARG, kw
        assert b'dfq_batch_nsr_plan_create' in lib.dfq_last_error(), kw
        assert not plan.value, kw
    valid()
    assert lib.dfq_batch_nsr_plan_run(None, None) == DFQ_ERR_ARG and b'dfq_batch_nsr_plan_run' in lib.dfq_last_error()
    assert lib.dfq_batch_nsr_plan_launches(None) == 0
    lib.dfq_batch_nsr_plan_destroy(None)
    assert lib.dfq_batch_mixed_plan_set_costs(None, None) == DFQ_ERR_ARG and b'dfq_batch_mixed_plan_set_costs' in lib.dfq_last_error()
    valid()


def test_struct_layout_matches_header():
    import os
    import subprocess
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = r'''
    #include <stdio.h>
    #include <stddef.h>
    #include "dfq_hip.h"
    #define T dfq_batch_nsr_tensor
    #define C dfq_batch_nsr_config
    int main(void) {
        printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu ", sizeof(T), offsetof(T, data), offsetof(T, rows), offsetof(T, row_len),
               offsetof(T, kernel_len), offsetof(T, groups), offsetof(T, source_begin), offsetof(T, source_count), offsetof(T, moment_offset),
               offsetof(T, row_offset));
        printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(C), offsetof(C, widths), offsetof(C, n_widths), offsetof(C, symmetric),
               offsetof(C, per_row), offsetof(C, moment), offsetof(C, input_moment));
        return 0;
    }'''
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, 't.c')
        open(c, 'w').write(src)
        exe = os.path.join(d, 't')
        subprocess.run(['gcc', '-I', os.path.join(root, 'include'), c, '-o', exe], check=True)
        got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    P, Q = _ffi.DfqBatchNsrTensor, _ffi.DfqBatchNsrConfig
    assert got == [ctypes.sizeof(P), P.data.offset, P.rows.offset, P.row_len.offset, P.kernel_len.offset, P.groups.offset,
                   P.source_begin.offset, P.source_count.offset, P.moment_offset.offset, P.row_offset.offset,
                   ctypes.sizeof(Q), Q.widths.offset, Q.n_widths.offset, Q.symmetric.offset, Q.per_row.offset, Q.moment.offset,
                   Q.input_moment.offset]


# ---- networks ------------------------------------------------------------------------------------------------------------------
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


def _state(graph):
    """every tensor the calibration may touch, as bits"""
    out = {}
    for k, m in graph.items():
        for name in ('weight', 'bias', 'fake_weight', 'fake_bias'):
            t = getattr(m, name, None)
            if torch.is_tensor(t):
                out[(k, name)] = _bits_of(t.detach().cpu().numpy().astype(F32)).copy()
    return out


def _same_state(a, b):
    return sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize('name', NAMES)
def test_nsr_plan_on_networks(engine, name):
    nets, batch = _batch(name, SEEDS[:2], engine.device)
    before = [_state(g) for (_, g, _, _) in nets]
    had_bias = [[m.bias is None for _, m in _targ(g)] for (_, g, _, _) in nets]
    plan = batch.nsr_plan(WIDTHS, per_channel=True, moment='second_moment', input_moment=0.5)
    assert plan.launches == 3 and plan.widths == WIDTHS and plan.keys == [k for k, _ in _targ(nets[0][1])]
    assert [[m.bias is None for _, m in _targ(g)] for (_, g, _, _) in nets] == had_bias, 'creating the plan gave a layer a bias'
    plan.run()
    _ffi.synchronize()
    assert all(_same_state(_state(g), s) for (_, g, _, _), s in zip(nets, before)), 'the plan wrote a tensor of the networks'
    fed_by_data = [k for k, m in _targ(nets[0][1]) if nets[0][2][k] is None or nets[0][2][k][0] == 'Data']
    assert fed_by_data
    for n in range(2):
        graph, bottoms = nets[n][1], nets[n][2]
        costs, rows, moments = plan.costs(n), plan.rows(n), plan.moments(n)
        assert list(costs) == list(rows) == list(moments) == plan.keys
        # the sources, from the walk itself
        _, steps, keys = dfq._bc_tables(graph, bottoms, TARG, torch.nn.BatchNorm2d, ensure_bias=False)
        srcs_of = {key: srcs for key, (_, srcs, _, _) in zip(keys, steps)}
        for k, m in _targ(graph):
            w = _weights(graph)[k]
            groups = getattr(m, 'groups', 1)
            klen = int(np.prod(m.weight.shape[2:])) if m.weight.dim() > 2 else 1
            ipg = w.shape[1] // klen
            srcs = [(None if fw is None else fw.detach().cpu().numpy(), fb.detach().cpu().numpy(), relu, cat) for (fw, fb, relu, cat) in srcs_of.get(k, [])]
            assert bool(srcs) == (k not in fed_by_data)
            a = _ref_moments(engine, srcs, ipg * groups, 1, F32(0.5))
            assert np.array_equal(_bits_of(moments[k]), _bits_of(a)), '{} net {} {}: moments'.format(name, n, k)
            e = _errors(w, True, False, WIDTHS)
            some = sorted({0, w.shape[0] // 2, w.shape[0] - 1})
            R, S = _ref_rows(w[some], a, e[:, some], ipg, klen, 1) if groups == 1 else _ref_rows(w, a, e, ipg, klen, groups)
            for i, o in enumerate(some if groups == 1 else range(w.shape[0])):
                for j in range(len(WIDTHS)):
                    g = Fraction(float(rows[k][o, j]))
                    assert abs(g - R[i][j]) <= Fraction(_gamma(2 * w.shape[1] + 1)) * R[i][j], '{} net {} {} row {}'.format(name, n, k, o)
            for j in range(len(WIDTHS)):
                s = 0.0
                for o in range(w.shape[0]):
                    s += float(rows[k][o, j])
                assert _same_float(float(costs[k][j]), s)
    assert all(m.bias is None for (_, g, _, _), hb in zip(nets, had_bias) for (_, m), none in zip(_targ(g), hb) if none)
    plan.close()
    with pytest.raises(RuntimeError):
        plan.run()


def test_walk_without_its_side_effect(engine):
    """_bc_tables(ensure_bias=False) lists the same steps and sources and leaves every bias as it was, None included"""
    for name in NAMES:
        _, graph, bottoms, _ = _prepared(name, 0, engine.device)
        for _, m in _targ(graph):                      # (the structure alone is looked at)
            m.bias = None
        none = [k for k, m in _targ(graph) if m.bias is None]
        _, steps, keys = dfq._bc_tables(graph, bottoms, TARG, torch.nn.BatchNorm2d, ensure_bias=False)
        assert [k for k, m in _targ(graph) if m.bias is None] == none
        _, steps2, keys2 = dfq._bc_tables(graph, bottoms, TARG, torch.nn.BatchNorm2d)
        assert keys == keys2 and [(s[0], [(id(a), id(b), c, d) for a, b, c, d in s[1]]) for s in steps] == \
            [(s[0], [(id(a), id(b), c, d) for a, b, c, d in s[1]]) for s in steps2]
        assert keys2 and not any(graph[k].bias is None for k in keys2), 'the ordinary walk gives the layers it corrects a bias'


# ---- set_costs -----------------------------------------------------------------------------------------------------------------
def _check_alloc(plan, nsr, n, sizes, sens=None, pin=None, what=''):
    costs = nsr.costs(n) if nsr is not None else plan.errors(n)
    keys = list(costs)
    ref = _alloc_ref([costs[k].tolist() for k in keys], [sizes[k] for k in keys], list(plan.widths), [(sens or {}).get(k, 1.0) for k in keys],
                     [(pin or {}).get(k, 0) for k in keys], plan.budget)
    bits, (used, steps), cost = plan.bits(n), plan.used(n), plan.cost(n)
    assert [bits[k] for k in keys] == ref['bits'], '{} net {}: bits'.format(what, n)
    assert (used, steps) == (ref['used'], ref['steps']), '{} net {}: used / steps'.format(what, n)
    assert _same_float(cost, ref['cost']), '{} net {}: cost {!r} against {!r}'.format(what, n, cost, ref['cost'])
    return ref


@pytest.mark.parametrize('name', NAMES)
@pytest.mark.parametrize('pair', PAIRS)
def test_mixed_plan_allocates_on_the_costs(engine, name, pair):
    per_channel, signed = pair
    nets, batch = _batch(name, SEEDS, engine.device)
    keys = [k for k, _ in _targ(nets[0][1])]
    sizes = {k: m.weight.numel() for k, m in _targ(nets[0][1])}
    total = sum(sizes.values())
    nsr = batch.nsr_plan(WIDTHS, per_channel=per_channel, signed=signed)
    nsr.run()
    plain = batch.mixed_plan(WIDTHS, avg_bits=4, per_channel=per_channel, signed=signed, apply=False)
    plain.run()
    _ffi.synchronize()
    plain_blocks = [t.clone() for t in (plain.bits_block, plain.error_block, plain.used_block, plain.cost_block, plain.range_block)]
    for label, kw in [('avg 4', dict(avg_bits=4)), ('avg 2.5', dict(avg_bits=2.5)), ('tight', dict(budget_bits=2 * total + 7)),
                      ('everything', dict(budget_bits=8 * total)),
                      ('pinned', dict(avg_bits=4.25, pin={keys[0]: 8, keys[-1]: 8}, sensitivity={keys[1]: 0.0, keys[2]: 3.5}))]:
        plan = batch.mixed_plan(WIDTHS, per_channel=per_channel, signed=signed, apply=False, costs=nsr, **kw)
        plan.run()
        _ffi.synchronize()
        for n in range(len(SEEDS)):
            _check_alloc(plan, nsr, n, sizes, kw.get('sensitivity'), kw.get('pin'), label)
        if label == 'avg 4':
            assert torch.equal(plan.error_block.view(torch.uint8), plain.error_block.view(torch.uint8)), 'errors change with the costs'
            assert torch.equal(plan.range_block.view(torch.uint8), plain.range_block.view(torch.uint8))
            # back to the plan's own errors: every block is that of a plan that never had costs
            plan.set_costs(None)
            plan.run()
            _ffi.synchronize()
            for a, b in zip(plain_blocks, (plan.bits_block, plan.error_block, plan.used_block, plan.cost_block, plan.range_block)):
                assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), 'set_costs(None) is not the plain plan'
            plan.set_costs(nsr)
            plan.run()
            _ffi.synchronize()
            _check_alloc(plan, nsr, 0, sizes, what='set again')
        plan.close()
    assert not torch.equal(nsr.cost_block, plain.error_block), 'the costs are the errors: the test shows nothing'
    # a layer whose costs are all NaN takes no step
    saved = nsr.cost_block.clone()
    nsr.cost_block[1, 2, :] = math.nan
    plan = batch.mixed_plan(WIDTHS, avg_bits=5, per_channel=per_channel, signed=signed, apply=False, costs=nsr)
    plan.run()
    _ffi.synchronize()
    assert plan.bits(1)[keys[2]] == WIDTHS[0] and math.isnan(plan.cost(1))
    for n in range(len(SEEDS)):
        _check_alloc(plan, nsr, n, sizes, what='NaN costs')
    nsr.cost_block.copy_(saved)
    plan.close()
    plain.close()
    nsr.close()


@pytest.mark.parametrize('name', NAMES)
@pytest.mark.parametrize('pair', [(False, False), (True, True)])
def test_quantised_like_quant_plan_at_each_width(engine, name, pair):
    per_channel, signed = pair
    nets, batch = _batch(name, SEEDS, engine.device)
    before = [_weights(g) for (_, g, _, _) in nets]
    nsr = batch.nsr_plan(WIDTHS, per_channel=per_channel, signed=signed)
    nsr.run()
    plan = batch.mixed_plan(WIDTHS, avg_bits=4.5, per_channel=per_channel, signed=signed, codes='int8', costs=nsr)
    plan.run()
    _ffi.synchronize()
    sizes = {k: m.weight.numel() for k, m in _targ(nets[0][1])}
    bits = [plan.bits(n) for n in range(len(SEEDS))]
    for n in range(len(SEEDS)):
        _check_alloc(plan, nsr, n, sizes, what='applied')
    occurring = sorted({b for d in bits for b in d.values()})
    assert len(occurring) >= 2, 'one width for everything: the test shows nothing'
    seen = 0
    for b in occurring:
        nets2, twin = _batch(name, SEEDS, engine.device)
        assert all(np.array_equal(_bits_of(a), _bits_of(c)) for a, c in zip(_weights(nets2[0][1]).values(), before[0].values())), 'twin'
        tp = twin.quant_plan(bit_weight=b, bits_bias=32, per_channel=per_channel, signed=signed, codes='int8')
        tp.run()
        _ffi.synchronize()
        for n in range(len(SEEDS)):
            got_w, want_w = _weights(nets[n][1]), _weights(nets2[n][1])
            got_c, want_c, got_r, want_r = plan.codes(n), tp.codes(n), plan.ranges(n), tp.ranges(n)
            for k, width in bits[n].items():
                if width != b:
                    continue
                seen += 1
                what = '{} net {} {} at {} bits'.format(name, n, k, b)
                assert np.array_equal(_bits_of(got_w[k]), _bits_of(want_w[k])), what + ': weight'
                assert torch.equal(got_c[k].cpu(), want_c[k].cpu()), what + ': codes'
                assert np.array_equal(_bits_of(got_r[k].cpu().numpy()), _bits_of(want_r[k].cpu().numpy())), what + ': range'
        tp.close()
    assert seen == len(SEEDS) * len(bits[0])
    plan.close()
    nsr.close()


# ---- the Python surface --------------------------------------------------------------------------------------------------------
def test_python_refusals(engine):
    nets, batch = _batch('tiny_res', [3], engine.device)
    nets2, other = _batch('tiny_res', [3], engine.device)
    nsr = batch.nsr_plan(WIDTHS, per_channel=True, signed=False)
    for kw in [dict(widths=(2, 4, 8)), dict(per_channel=False), dict(signed=True), dict(widths=4)]:
        args = dict(widths=WIDTHS, per_channel=True, signed=False, avg_bits=4)
        args.update(kw)
        with pytest.raises(ValueError):
            batch.mixed_plan(costs=nsr, **args)
    with pytest.raises(ValueError):
        other.mixed_plan(WIDTHS, avg_bits=4, per_channel=True, costs=nsr)
    with pytest.raises(ValueError):
        batch.mixed_plan(WIDTHS, avg_bits=4, per_channel=True, costs=nsr.cost_block)
    plan = batch.mixed_plan(WIDTHS, avg_bits=4, per_channel=True, costs=nsr, apply=False)      # a matching one works
    nsr.run()
    plan.run()
    _ffi.synchronize()
    assert plan.used(0)[0] <= plan.budget
    plan.close()
    nsr.close()
    for kw in [dict(widths=()), dict(widths=(4, 2)), dict(widths=(2, 17)), dict(widths=(2.0, 4)), dict(widths=(1, 2, 3, 4, 5, 6, 7, 8, 9)),
               dict(moment='mean'), dict(moment=0), dict(input_moment=-1.0), dict(input_moment=math.inf), dict(input_moment=math.nan),
               dict(input_moment='1'), dict(input_moment=True), dict(input_moment=1e39)]:
        with pytest.raises(ValueError):
            batch.nsr_plan(**kw)
    with pytest.raises(ValueError):
        batch.quantize_mixed(WIDTHS, avg_bits=4, cost='hessian')
    _, graph, bottoms, _ = _prepared('tiny_res', 3, torch.device('cpu'))
    with pytest.raises(ValueError):
        dfq.quantize_mixed(graph, WIDTHS, avg_bits=4, targ_type=TARG, cost='nsr')
    with pytest.raises(ValueError):
        dfq.quantize_mixed(graph, WIDTHS, avg_bits=4, targ_type=TARG, cost='hessian', bottoms=bottoms)
    batch.release()
    with pytest.raises(RuntimeError):
        batch.nsr_plan()


@pytest.mark.parametrize('pair', [(False, False), (True, True)])
def test_quantize_mixed_nsr_with_correction_is_the_four_steps(engine, pair):
    per_channel, signed = pair
    name = 'tiny_mobile'
    nets, batch = _batch(name, SEEDS, engine.device)
    nets2, batch2 = _batch(name, SEEDS, engine.device)
    codes, ranges, bits = batch.quantize_mixed(WIDTHS, avg_bits=4, per_channel=per_channel, signed=signed, codes='int8', bits_bias=32,
                                               correct=True, cost='nsr', moment='second_moment', input_moment=0.25)
    nsr = batch2.nsr_plan(WIDTHS, per_channel=per_channel, signed=signed, moment='second_moment', input_moment=0.25)
    nsr.run()
    first = batch2.mixed_plan(WIDTHS, avg_bits=4, per_channel=per_channel, signed=signed, apply=False, costs=nsr)
    first.run()
    bc = batch2.bc_plan()
    bc.run(signed=signed, per_channel=per_channel, widths=first)
    last = batch2.mixed_plan(WIDTHS, avg_bits=4, per_channel=per_channel, signed=signed, codes='int8', costs=nsr)
    last.run()
    bc.status()
    _ffi.synchronize()
    for n in range(len(SEEDS)):
        assert bits[n] == dict(last.bits(n)) == dict(first.bits(n))
        assert _same_state(_state(nets[n][1]), _state(nets2[n][1])), 'net {}: weights, biases or proxies differ'.format(n)
        for k in bits[n]:
            assert torch.equal(codes[n][k].cpu(), last.codes(n)[k].cpu()), k
            assert np.array_equal(_bits_of(ranges[n][k].cpu().numpy()), _bits_of(last.ranges(n)[k].cpu().numpy())), k
    for p in (nsr, first, bc, last):
        p.close()


@pytest.mark.parametrize('pair', [(False, False), (True, True)])
def test_single_network_equals_the_batch_of_one(engine, pair):
    per_channel, signed = pair
    name, seed = 'tiny_cat', 1
    nets, batch = _batch(name, [seed], engine.device)
    keys = [k for k, _ in _targ(nets[0][1])]
    nsr = batch.nsr_plan(WIDTHS, per_channel=per_channel, signed=signed, input_moment=0.5)
    nsr.run()
    plan = batch.mixed_plan(WIDTHS, avg_bits=4.5, per_channel=per_channel, signed=signed, pin={keys[0]: 8}, costs=nsr)
    plan.run()
    _ffi.synchronize()
    want_bits, want_err, want_cost = plan.bits(0), plan.errors(0), nsr.costs(0)
    want_rng, want_w = {k: v.cpu().numpy() for k, v in plan.ranges(0).items()}, _weights(nets[0][1])
    plan.close()
    nsr.close()
    _, graph, bottoms, rels = _prepared(name, seed, torch.device('cpu'))
    dfq.cross_layer_equalization(graph, rels, TARG)
    none = [k for k, m in _targ(graph) if m.bias is None]
    proxies = {k: v for k, v in _state(graph).items() if k[1].startswith('fake')}
    got = dfq.quantize_mixed(graph, WIDTHS, avg_bits=4.5, per_channel=per_channel, signed=signed, pin={keys[0]: 8}, targ_type=TARG,
                             cost='nsr', bottoms=bottoms, input_moment=0.5)
    assert list(got) == keys and got[keys[0]]['bits'] == 8
    assert [k for k, m in _targ(graph) if m.bias is None] == none, 'quantize_mixed gave a layer a bias'
    assert all(np.array_equal(v, _state(graph)[k]) for k, v in proxies.items())
    for k in keys:
        assert sorted(got[k]) == ['bits', 'err', 'nsr', 'range']
        assert got[k]['bits'] == want_bits[k], k
        j = WIDTHS.index(want_bits[k])
        assert _same_float(got[k]['err'], float(want_err[k][j])) and _same_float(got[k]['nsr'], float(want_cost[k][j])), k
        assert np.array_equal(_bits_of(got[k]['range']), _bits_of(want_rng[k])), k
    for k, w in _weights(graph).items():
        assert np.array_equal(_bits_of(w), _bits_of(want_w[k])), k
