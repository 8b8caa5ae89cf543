"""The activation-statistics kernels at the edges: dfq_relu_moments, dfq_moments_after_add, dfq_moment_range, dfq_bn_ranges,
dfq_bn_through_layer (dfq_amd/csrc/dfq_act.hip, dfq_act_shared.hpp, normal_pdf_cdf of dfq_common.hpp) and the same arithmetic
inside the batch plan (dfq_act_batch.hip), each called through the C ABI on data of the test's choosing: guard elements in
front of and behind every output buffer, outputs pre-filled with a sentinel, inputs checked unmodified.

Reference of the moments: the clipped-normal moments in float64 numpy on the float32 inputs, in the raw-moment form
    ReLU   E[Y]  = w pdf(l) + b Phi(-l)                         E[Y^2] = (b^2 + w^2) Phi(-l) + b w pdf(l)
    ReLU6  E[Y]  = w (pdf(l) - pdf(h)) + b dPhi + 6 Phi(-h)     E[Y^2] = (b^2 + w^2) dPhi + b w (pdf(l) - pdf(h)) - 6 w pdf(h) + 36 Phi(-h)
with l = -b / w, h = (6 - b) / w, dPhi = Phi(h) - Phi(l), var = E[Y^2] - E[Y]^2; for w == 0 the point mass (mean = clip(b),
var = 0).  That is NOT the three- / five-term form the kernels and the oracle evaluate.  Its own error is a few 2^-53
(b^2 + w^2 + c^2), nine orders below the bound.  Cross-check against mpmath at 50 digits (test_float64_reference_against_mpmath,
CPU only, 98 channels of the input set, grid + band + tails): worst |float64 - mpmath| = 0.84 * 2^-53 (|b| + w + c) for the
mean and 2.04 * 2^-53 (b^2 + w^2 + c^2) for the variance; the test allows 16 * 2^-53.

Bounds (u = 2^-24, c = 6 for ReLU6, else 0, eta = 2^-149 the float32 subnormal spacing):
    |mean - exact| <= Km u (|b| + w + c)       + 4 eta
    |var  - exact| <= Kv u (b^2 + w^2 + c^2)   + 8 eta
The eta terms are the absolute error of gradual underflow, one per rounded operation that can underflow: without them the
relative model is false for w = 1e-30 (w * w = 1e-60 is 0 in float32); they are 40 orders below every other channel's bound.
Km, Kv = twice the error of the ORACLE (orc.moments_relu / moments_relu6: the reference's float32 operation order with
scipy's pdf / cdf) measured in these units over the input set below, because device and host libm may round pdf / cdf to
neighbouring float32 values.  Measured on the CPU (test_oracle_error_is_what_the_header_says asserts them):

                       mean, ReLU   mean, ReLU6   var, ReLU   var, ReLU6
    oracle vs float64     1.54         0.87         3.69        2.11
    chosen K              Km = 3.1 (2 x 1.54, rounded up)     Kv = 7.4 (2 x 3.69, rounded up)

The input set (_moment_inputs, 1543 channels): channel 0 is the channel of the finding (w = 0.0010381973, b = 5.99877: ReLU6
variance -6.8e-6 in float32, true value 8.7e-7); the grid W_GRID x B_GRID; a dense band b in [5.99, 6.01], w in [1e-3, 1e-2];
tails with |b / w| and |(6 - b) / w| from 5 to 60 (pdf leaves float32 at 13.2 / 14.4, 1 - cdf at 5.4, both leave float64 at
38.5); random fill between the grid points.  fake_weight is |gamma|: w < 0 is out of contract and not tested.

Planted exclusions from the comparison with float64 -- the oracle is NaN exactly there, and the tests assert that the set of
the oracle's NaN positions EQUALS this list:
    (w, b) = (0, 0) and (0, -0.0)                  t = 0 / 0
    (0, 6) in mode 2                               h = 0 / 0
    (1, 2e19), (1, -2e19), (0.5, 1e30)             b * b overflows: inf - inf, 0 * inf
In dfq_moments_after_add the same list with w = sd: the variances -1e-6, -2e-6, -7e-6 (var + eps <= 0: sd = 0) with mean 0,
-0.0 or (mode 2) 6, the overflowing means 2e19 and -2e19, and the three planted NaN variances.

Mutations of the kernels that this file catches on the emulation: t4 dropped in moments_relu6, `mean` for `6 - mean` in t5
(test_moments_whole_set, test_moments_lengths, test_moments_after_add); overwrite under accumulate (test_moments_accumulate);
fminf for nan_min (test_moment_range, test_bn_ranges_*); the moment_range loop started at threadIdx.x + kBlock
(test_moment_range); o / groups as the group index (test_bn_through_layer).  NOT visible to the fiber emulation, which runs
a workgroup's threads one after the other between barriers: the __syncthreads() in front of act_range_kernel's fold.

The finding (a rounding-negative variance made sqrt(var + eps) NaN): the radicand is clamped at 0 by `sd_of`
(dfq_act_shared.hpp) at all four sites; NaN still propagates.  The tests of sections b, c, e and f hold the clamp.
"""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn as nn

from dfq_amd import _ffi, arena
from oracle import dfq_oracle as orc
from tests.common import F32, TARG, assert_bitexact

DFQ_ERR_ARG = -1                # include/dfq_hip.h
GUARD = 16                      # elements in front of and behind every buffer handed to the library
SENTINEL = -777.25
U = 2.0 ** -24
ETA = 2.0 ** -149
KM, KV = 3.1, 7.4
ORACLE_MAX = {('mean', 1): 1.54, ('mean', 2): 0.87, ('var', 1): 3.69, ('var', 2): 2.11}     # the header's table
EPS = 1e-6
W_Q, B_Q = 0.0010381973, 5.99877                    # the channel of the finding

_below6, _above6 = np.nextafter(F32(6), F32(0)), np.nextafter(F32(6), F32(7))
W_GRID = [0.0, 1e-30, 1e-6, 1e-3, 0.01, 0.1, 0.5, 1.0, 3.0, 10.0, 100.0, 1e4]
B_GRID = [0.0, -0.0, 1e-3, -1e-3, 0.1, -0.1, 1.0, -1.0, 3.0, -3.0, 5.9, _below6, 6.0, _above6, 6.1, 9.0, 13.0, -13.0, 40.0, -40.0,
          100.0, -100.0, 1e4, -1e4]
PLANTED = [(0.0, 0.0, (1, 2)), (0.0, -0.0, (1, 2)), (0.0, 6.0, (2,)), (1.0, 2e19, (1, 2)), (1.0, -2e19, (1, 2)), (0.5, 1e30, (1, 2))]
NEG_VAR = [-1e-9, -9.9e-7, -1e-6, -2e-6, -7e-6]     # sizes dfq_relu_moments really leaves in mode 2; fl(-1e-6 + eps) == 0
LENGTHS = [1, 255, 256, 257, 1000]


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=F32)).view(np.int32)


# ---- the input set ------------------------------------------------------------------------------------------------------
def _moment_inputs():
    """(w, b, {mode: sorted planted positions}).  Every length of LENGTHS cuts a prefix that holds the finding (0), grid,
    band, tail and random channels: the parts are interleaved by a fixed permutation behind channel 0."""
    rng = np.random.RandomState(20240611)
    w, b = [], []
    for wi in W_GRID:
        for bi in B_GRID:
            w.append(wi)
            b.append(bi)
    for wi, bi, _ in PLANTED[3:]:                                            # (the first three are grid points)
        w.append(wi)
        b.append(bi)
    w += list(np.exp(rng.uniform(math.log(1e-3), math.log(1e-2), 400)))      # the dense band around the ReLU6 ceiling
    b += list(rng.uniform(5.99, 6.01, 400))
    for wi in (1e-3, 0.1, 1.0, 30.0):                                        # tails: |l| or |h| = r
        for r in (5.0, 5.5, 8.0, 13.0, 13.5, 14.5, 20.0, 37.0, 38.4, 38.6, 39.0, 60.0):
            for bi in (r * wi, -r * wi, 6.0 + r * wi, 6.0 - r * wi):
                w.append(wi)
                b.append(bi)
    w += list(np.exp(rng.uniform(math.log(1e-6), math.log(1e4), 300)))       # between the grid points: everything
    b += list(np.exp(rng.uniform(math.log(1e-3), math.log(1e4), 300)) * rng.choice([-1.0, 1.0], 300))
    w += list(np.exp(rng.uniform(math.log(1e-3), math.log(10.0), 359)))      # ... and where ReLU / ReLU6 bend
    b += list(rng.uniform(-10.0, 16.0, 359))
    w, b = np.asarray(w, dtype=F32), np.asarray(b, dtype=F32)
    perm = rng.permutation(len(w))
    w = np.concatenate([[F32(W_Q)], w[perm]]).astype(F32)
    b = np.concatenate([[F32(B_Q)], b[perm]]).astype(F32)
    planted = {1: [], 2: []}
    for wi, bi, modes in PLANTED:
        hit = np.flatnonzero((_bits(w) == _bits(F32(wi))) & (_bits(b) == _bits(F32(bi))))
        assert len(hit) == 1, (wi, bi, hit)
        for m in modes:
            planted[m].append(int(hit[0]))
    return w, b, {m: sorted(v) for m, v in planted.items()}


_INPUTS = _moment_inputs()


# ---- float64 reference ---------------------------------------------------------------------------------------------------
def _exact_moments(mode, w32, b32):
    """mean, var of clip(N(b, w^2)) in float64 (module docstring); mode 0: (b, w^2)"""
    from scipy.special import ndtr
    w, b = np.asarray(w32, dtype=F32).astype(np.float64), np.asarray(b32, dtype=F32).astype(np.float64)
    if mode == 0:
        return b.copy(), w * w
    pdf = lambda x: np.exp(-(x * x) / 2.0) / math.sqrt(2.0 * math.pi)
    with np.errstate(all='ignore'):
        lo = -b / w
        if mode == 1:
            mean = w * pdf(lo) + b * ndtr(-lo)
            second = (b * b + w * w) * ndtr(-lo) + b * w * pdf(lo)
            point = np.maximum(b, 0.0)
        else:
            hi = (6.0 - b) / w
            dphi, dpdf = ndtr(hi) - ndtr(lo), pdf(lo) - pdf(hi)
            mean = w * dpdf + b * dphi + 6.0 * ndtr(-hi)
            second = (b * b + w * w) * dphi + b * w * dpdf - 6.0 * w * pdf(hi) + 36.0 * ndtr(-hi)
            point = np.clip(b, 0.0, 6.0)
        var = second - mean * mean
    dead = w == 0
    return np.where(dead, point, mean), np.where(dead, 0.0, var)


def _units(mode, w32, b32, mean, var):
    """the errors of (mean, var) against float64 in units of u (|b| + w + c) and u (b^2 + w^2 + c^2), after the eta terms"""
    w, b = np.asarray(w32, dtype=np.float64), np.asarray(b32, dtype=np.float64)
    c = 6.0 if mode == 2 else 0.0
    em, ev = _exact_moments(mode, w32, b32)
    with np.errstate(all='ignore'):
        dm = np.maximum(np.abs(np.asarray(mean, dtype=np.float64) - em) - 4 * ETA, 0.0) / (U * (np.abs(b) + w + c))
        dv = np.maximum(np.abs(np.asarray(var, dtype=np.float64) - ev) - 8 * ETA, 0.0) / (U * (b * b + w * w + c * c))
    return dm, dv


def _oracle(mode, w, b):
    if mode == 0:
        return np.asarray(b, dtype=F32).copy(), (np.asarray(w, dtype=F32) * np.asarray(w, dtype=F32)).astype(F32)
    return (orc.moments_relu if mode == 1 else orc.moments_relu6)(w, b)


def _sd(var, eps=EPS):
    """sd_of (dfq_act_shared.hpp) in numpy float32: sqrt of the radicand clamped at 0 by a comparison (NaN stays NaN)"""
    with np.errstate(invalid='ignore'):
        r = (np.asarray(var, dtype=F32) + F32(eps)).astype(F32)
        return np.sqrt(np.where(r < 0, F32(0), r)).astype(F32)


def _nan_min(a):
    a = np.asarray(a, dtype=F32)
    return F32(np.nan) if np.isnan(a).any() else a.min()


def _nan_max(a):
    a = np.asarray(a, dtype=F32)
    return F32(np.nan) if np.isnan(a).any() else a.max()


def _range_ref(b, x, n_sigma):
    """(min_c fl(b - fl(N x)), max_c fl(b + fl(N x))) with torch's NaN propagation, numpy float32"""
    with np.errstate(all='ignore'):
        nw = (F32(n_sigma) * np.asarray(x, dtype=F32)).astype(F32)
        b = np.asarray(b, dtype=F32)
        return _nan_min((b - nw).astype(F32)), _nan_max((b + nw).astype(F32))


# ---- the C ABI with guard elements --------------------------------------------------------------------------------------
class _Guarded:
    def __init__(self, engine, n, init=None, dtype=torch.float32):
        self.n = n
        host = torch.full((n + 2 * GUARD,), SENTINEL if dtype.is_floating_point else -777, dtype=dtype)
        if init is not None:
            host[GUARD:GUARD + n] = torch.as_tensor(np.ascontiguousarray(init)).reshape(-1).to(dtype)
        self.host0 = host.clone()
        self.buf = engine.to(host)
        self.view = self.buf[GUARD:GUARD + n]

    def ptr(self, offset=0):
        return ctypes.c_void_p(self.view.data_ptr() + offset * self.view.element_size())

    def addr(self, offset=0):
        return self.view.data_ptr() + offset * self.view.element_size()

    def check_guards(self, what):
        got = self.buf.cpu()
        assert torch.equal(got[:GUARD], self.host0[:GUARD]) and torch.equal(got[GUARD + self.n:], self.host0[GUARD + self.n:]), \
            '{}: a guard element was written'.format(what)

    def check_unchanged(self, what):
        got, want = self.buf.cpu(), self.host0
        same = (got == want) | (torch.isnan(got) & torch.isnan(want))
        if got.dtype == torch.float32:
            same = same & ((got.view(torch.int32) == want.view(torch.int32)) | torch.isnan(got))
        assert bool(same.all()), '{}: an input buffer was written'.format(what)

    def numpy(self):
        return self.view.cpu().numpy().copy()


def _relu_moments(engine, w, b, mode, old=None):
    """dfq_relu_moments on guarded buffers; old = (mean, var) -> accumulate = 1"""
    n = len(w)
    ws, bs = _Guarded(engine, n, w), _Guarded(engine, n, b)
    ms = _Guarded(engine, n, None if old is None else old[0])
    vs = _Guarded(engine, n, None if old is None else old[1])
    _ffi.check(_ffi.lib().dfq_relu_moments(ws.ptr(), bs.ptr(), n, mode, ms.ptr(), vs.ptr(), 0 if old is None else 1, _ffi.stream_arg()))
    _ffi.synchronize()
    ws.check_unchanged('weight')
    bs.check_unchanged('bias')
    ms.check_guards('mean')
    vs.check_guards('var')
    return ms.numpy(), vs.numpy()


def _same_specials(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)), '{}: NaN at {}, the oracle has NaN at {}'.format(
        what, np.flatnonzero(np.isnan(got)).tolist(), np.flatnonzero(np.isnan(want)).tolist())
    assert np.array_equal(np.isposinf(got), np.isposinf(want)) and np.array_equal(np.isneginf(got), np.isneginf(want)), \
        '{}: the infinities differ from the oracle\'s'.format(what)


def _assert_moments(mode, w, b, mean, var, planted, what):
    """the assertions of section a for one (mean, var) the engine returned for channels (w, b)"""
    om, ov = _oracle(mode, w, b)
    excluded = np.flatnonzero(np.isnan(om) | np.isnan(ov)).tolist()
    assert excluded == sorted(planted), '{}: the oracle is NaN at {}, planted are {}'.format(what, excluded, sorted(planted))
    _same_specials(mean, om, what + ' mean')
    _same_specials(var, ov, what + ' var')
    dm, dv = _units(mode, w, b, mean, var)
    keep_m, keep_v = ~np.isnan(om), ~np.isnan(ov)
    worst_m, worst_v = float(dm[keep_m].max(initial=0.0)), float(dv[keep_v].max(initial=0.0))
    print('{}: mean {:.2f} u (|b| + w + c), var {:.2f} u (b^2 + w^2 + c^2)'.format(what, worst_m, worst_v))
    i, j = int(np.argmax(np.where(keep_m, dm, -1))), int(np.argmax(np.where(keep_v, dv, -1)))
    assert worst_m <= KM, '{}: mean of channel {} (w {!r}, b {!r}) is {!r}: {:.2f} units > {}'.format(what, i, w[i], b[i], mean[i], worst_m, KM)
    assert worst_v <= KV, '{}: var of channel {} (w {!r}, b {!r}) is {!r}: {:.2f} units > {}'.format(what, j, w[j], b[j], var[j], worst_v, KV)
    return worst_m, worst_v


# ---- the reference itself -------------------------------------------------------------------------------------------------
def test_float64_reference_against_mpmath():
    mp = pytest.importorskip('mpmath')
    mp.mp.dps = 50
    w, b, planted = _INPUTS
    pick = [0] + list(range(1, len(w), 16))
    Phi = lambda x: mp.erfc(-x / mp.sqrt(2)) / 2
    pdf = lambda x: mp.exp(-x * x / 2) / mp.sqrt(2 * mp.pi)
    worst = {}
    for mode in (1, 2):
        em, ev = _exact_moments(mode, w, b)
        c = 6.0 if mode == 2 else 0.0
        for i in pick:
            wi, bi = mp.mpf(float(w[i])), mp.mpf(float(b[i]))
            if wi == 0:
                continue                                            # the point mass is not a formula
            lo = -bi / wi
            if mode == 1:
                m1 = wi * pdf(lo) + bi * Phi(-lo)
                m2 = (bi * bi + wi * wi) * Phi(-lo) + bi * wi * pdf(lo)
            else:
                hi = (6 - bi) / wi
                m1 = wi * (pdf(lo) - pdf(hi)) + bi * (Phi(hi) - Phi(lo)) + 6 * Phi(-hi)
                m2 = (bi * bi + wi * wi) * (Phi(hi) - Phi(lo)) + bi * wi * (pdf(lo) - pdf(hi)) - 6 * wi * pdf(hi) + 36 * Phi(-hi)
            dm = float(abs(mp.mpf(float(em[i])) - m1) / (abs(bi) + wi + c)) / 2.0 ** -53
            dv = float(abs(mp.mpf(float(ev[i])) - (m2 - m1 * m1)) / (bi * bi + wi * wi + c * c)) / 2.0 ** -53
            worst[mode] = (max(worst.get(mode, (0, 0))[0], dm), max(worst.get(mode, (0, 0))[1], dv))
    print('float64 vs mpmath in 2^-53 units (mean, var): ReLU {}, ReLU6 {}'.format(worst[1], worst[2]))
    assert len(pick) >= 96 and max(worst[1] + worst[2]) <= 16.0, worst


def test_oracle_error_is_what_the_header_says():
    """Km / Kv rest on these figures: the oracle's own error over the input set, and K = twice the larger of the two modes"""
    w, b, planted = _INPUTS
    got = {}
    for mode in (1, 2):
        om, ov = _oracle(mode, w, b)
        assert np.flatnonzero(np.isnan(om) | np.isnan(ov)).tolist() == planted[mode]
        dm, dv = _units(mode, w, b, om, ov)
        got[('mean', mode)], got[('var', mode)] = float(np.nanmax(dm[~np.isnan(om)])), float(np.nanmax(dv[~np.isnan(ov)]))
    print('oracle vs float64:', got)
    for k, v in got.items():
        assert abs(v - ORACLE_MAX[k]) <= 0.006, (k, v, ORACLE_MAX[k])
    assert KM >= 2 * max(ORACLE_MAX['mean', 1], ORACLE_MAX['mean', 2]) > KM - 0.2
    assert KV >= 2 * max(ORACLE_MAX['var', 1], ORACLE_MAX['var', 2]) > KV - 0.2
    # the finding: a negative ReLU6 variance below -eps in float32, 8.7e-7 in truth
    _, ov = orc.moments_relu6(np.array([W_Q], dtype=F32), np.array([B_Q], dtype=F32))
    assert -7.5e-6 < float(ov[0]) < -EPS and 8.6e-7 < float(_exact_moments(2, [W_Q], [B_Q])[1][0]) < 8.8e-7 < W_Q ** 2


# ---- a. dfq_relu_moments --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', [1, 2])
def test_moments_whole_set(engine, mode):
    w, b, planted = _INPUTS
    assert len(w) == 1543                       # seven workgroups, the last one partly filled
    mean, var = _relu_moments(engine, w, b, mode)
    _assert_moments(mode, w, b, mean, var, planted[mode], 'mode {} n {}'.format(mode, len(w)))


@pytest.mark.parametrize('n', LENGTHS)
def test_moments_lengths(engine, n):
    w, b, planted = _INPUTS
    w, b = w[:n], b[:n]
    for mode in (1, 2):
        mean, var = _relu_moments(engine, w, b, mode)
        _assert_moments(mode, w, b, mean, var, [p for p in planted[mode] if p < n], 'mode {} n {}'.format(mode, n))
    mean, var = _relu_moments(engine, w, b, 0)
    assert_bitexact(mean, b, 'mode 0 mean')
    assert (_bits(mean) == _bits(b)).all(), 'mode 0: the mean is the bias, bit for bit (-0.0 included)'
    assert_bitexact(var, (w * w).astype(F32), 'mode 0 var')


def test_moments_mode0_whole_set(engine):
    w, b, _ = _INPUTS
    mean, var = _relu_moments(engine, w, b, 0)
    assert (_bits(mean) == _bits(b)).all()
    with np.errstate(over='ignore'):
        assert_bitexact(var, (w * w).astype(F32), 'mode 0 var')


@pytest.mark.parametrize('n', [257, 1543])
def test_moments_accumulate(engine, n):
    """accumulate = 1: fl(old + new) bit for bit, `new` being what the same engine returns without accumulation"""
    w, b, _ = _INPUTS
    w, b = w[:n], b[:n]
    rng = np.random.RandomState(5)
    old_m = (rng.standard_normal(n) * 3).astype(F32)
    old_v = np.concatenate([NEG_VAR, [0.0, 1e-12, 1e-6, 1.0, 1e4]])[rng.randint(0, 10, n)].astype(F32)
    for k, v in enumerate([np.nan, np.inf, -np.inf]):
        old_m[3 + 7 * k::41] = v
        old_v[5 + 7 * k::43] = v
    for mode in (0, 1, 2):
        new_m, new_v = _relu_moments(engine, w, b, mode)
        got_m, got_v = _relu_moments(engine, w, b, mode, old=(old_m, old_v))
        with np.errstate(all='ignore'):
            assert_bitexact(got_m, (old_m + new_m).astype(F32), 'mode {} accumulated mean'.format(mode))
            assert_bitexact(got_v, (old_v + new_v).astype(F32), 'mode {} accumulated var'.format(mode))
        assert np.isnan(got_m[3::41]).all() and np.isnan(got_v[5::43]).all()
        fin = np.isfinite(new_m) & np.isinf(old_m)
        assert fin.any() and (got_m[fin] == old_m[fin]).all()


def test_moments_reject_bad_arguments(engine):
    lib = _ffi.lib()
    w, b, _ = _INPUTS
    ws, bs, ms, vs = (_Guarded(engine, 8, w[:8]), _Guarded(engine, 8, b[:8]), _Guarded(engine, 8), _Guarded(engine, 8))
    for mode, n in ((-1, 8), (3, 8), (1, 0), (1, -1)):
        assert lib.dfq_relu_moments(ws.ptr(), bs.ptr(), n, mode, ms.ptr(), vs.ptr(), 0, _ffi.stream_arg()) == DFQ_ERR_ARG
    assert lib.dfq_relu_moments(None, bs.ptr(), 8, 1, ms.ptr(), vs.ptr(), 0, _ffi.stream_arg()) == DFQ_ERR_ARG
    for mode in (0, 3):
        assert lib.dfq_moments_after_add(ms.ptr(), vs.ptr(), 8, mode, EPS, _ffi.stream_arg()) == DFQ_ERR_ARG
        assert b'dfq_moments_after_add' in lib.dfq_last_error()
    assert lib.dfq_moments_after_add(ms.ptr(), None, 8, 1, EPS, _ffi.stream_arg()) == DFQ_ERR_ARG
    assert lib.dfq_moments_after_add(ms.ptr(), vs.ptr(), 0, 1, EPS, _ffi.stream_arg()) == DFQ_ERR_ARG
    assert lib.dfq_moment_range(ms.ptr(), vs.ptr(), 0, EPS, 6.0, ms.ptr(), _ffi.stream_arg()) == DFQ_ERR_ARG
    _ffi.synchronize()
    for g in (ms, vs):
        g.check_unchanged('a refused call wrote')


# ---- b. dfq_moments_after_add ---------------------------------------------------------------------------------------------
def _after_add_inputs():
    """(mean, var, {mode: planted NaN positions}): ordinary and rounding-negative variances x the means of section a"""
    rng = np.random.RandomState(77)
    variances = [0.0, 1e-12, 1e-6, 1.0, 1e4] + NEG_VAR
    means = B_GRID + [B_Q, 5.9993, 6.0004, 5.95, 2e19, -2e19] + list(rng.uniform(-10, 16, 9))
    mean = np.asarray([m for v in variances for m in means], dtype=F32)
    var = np.asarray([v for v in variances for m in means], dtype=F32)
    mean = np.concatenate([mean, [1.0, B_Q, -3.0]]).astype(F32)            # a NaN variance stays NaN
    var = np.concatenate([var, [np.nan, np.nan, np.nan]]).astype(F32)
    perm = rng.permutation(len(mean))
    mean, var = mean[perm], var[perm]
    sd = _sd(var)
    planted = {}
    for mode in (1, 2):
        zero = (sd == 0) & ((mean == 0) | ((mean == 6) & (mode == 2)))              # sd == 0: -1e-6, -2e-6, -7e-6
        planted[mode] = np.flatnonzero(zero | (np.abs(mean) > 1.8e19) | np.isnan(var)).tolist()
    assert len(planted[1]) == 3 * 2 + 10 * 2 + 3 and len(planted[2]) == len(planted[1]) + 3
    return mean, var, planted


@pytest.mark.parametrize('mode', [1, 2])
def test_moments_after_add(engine, mode):
    mean, var, planted = _after_add_inputs()
    n = len(mean)
    assert n == 393                             # two workgroups
    sd = _sd(var)
    assert (sd[np.isin(var, np.asarray(NEG_VAR[2:], dtype=F32))] == 0).all() and sd[var == F32(-9.9e-7)][0] > 0
    ms, vs = _Guarded(engine, n, mean), _Guarded(engine, n, var)
    _ffi.check(_ffi.lib().dfq_moments_after_add(ms.ptr(), vs.ptr(), n, mode, EPS, _ffi.stream_arg()))
    _ffi.synchronize()
    ms.check_guards('mean')
    vs.check_guards('var')
    got_m, got_v = ms.numpy(), vs.numpy()
    want_m, want_v = _relu_moments(engine, sd, mean, mode)
    assert_bitexact(got_m, want_m, 'mean against dfq_relu_moments(sd, mean)')
    assert_bitexact(got_v, want_v, 'var against dfq_relu_moments(sd, mean)')
    assert np.isnan(got_m[np.isnan(var)]).all() and np.isnan(got_v[np.isnan(var)]).all(), 'a NaN variance stays NaN'
    neg = (var < 0) & ~np.isin(np.arange(n), planted[mode])
    assert neg.sum() >= 5 * 30 and np.isfinite(got_m[neg]).all() and np.isfinite(got_v[neg]).all(), \
        'a rounding-negative variance gave NaN at {}'.format(np.flatnonzero(neg & ~(np.isfinite(got_m) & np.isfinite(got_v))).tolist())
    keep = ~np.isnan(var)                       # (the float64 reference takes w = sd; a NaN sd is no channel)
    _assert_moments(mode, sd[keep], mean[keep], got_m[keep], got_v[keep],
                    [int(np.searchsorted(np.flatnonzero(keep), p)) for p in planted[mode] if keep[p]], 'after add, mode {}'.format(mode))


# ---- c. dfq_moment_range and dfq_bn_ranges --------------------------------------------------------------------------------
COUNTS = [1, 63, 64, 65, 255, 256, 257, 1025]
KINDS = ['min', 'max', 'nan', '+inf', '-inf']


def _positions(count):
    return sorted({p for p in (0, 63, 64, 255, 256, count - 1) if p < count})


def _range_cases(count, rng):
    """[(name, centre vector, width vector)]: base vectors with every planted value in turn.  Unplanted values lie strictly
    inside: centres in [-1, 1], widths in [0.1, 0.2]"""
    centre = rng.uniform(-1, 1, count).astype(F32)
    width = rng.uniform(0.1, 0.2, count).astype(F32)
    cases = [('random', centre, width), ('all equal', np.full(count, 0.37, dtype=F32), np.full(count, 0.15, dtype=F32))]
    for p in _positions(count):
        for kind in KINDS:
            c = centre.copy()
            c[p] = {'min': -50.0, 'max': 50.0, 'nan': np.nan, '+inf': np.inf, '-inf': -np.inf}[kind]
            cases.append(('{} at {}'.format(kind, p), c, width))
        x = width.copy()
        x[p] = np.nan                                           # a NaN width as well
        cases.append(('nan width at {}'.format(p), centre, x))
    return cases


@pytest.mark.parametrize('count', COUNTS)
def test_moment_range(engine, count):
    """bit-exact against numpy float32; the variance is width^2 - eps, so sd is about the width, with rounding-negative
    variances planted next to the extrema"""
    lib = _ffi.lib()
    rng = np.random.RandomState(count)
    cases = _range_cases(count, rng)
    rows_m, rows_v = [], []
    for name, c, x in cases:
        v = ((x * x).astype(F32) - F32(EPS)).astype(F32)
        rows_m.append(c)
        rows_v.append(v)
    for k, nv in enumerate(NEG_VAR + [-0.5]):                  # negative variances: sd = sqrt(max(var + eps, 0)), never NaN
        c, v = rows_m[0].copy(), rows_v[0].copy()
        v[:] = nv if k % 2 else v
        v[(k * 37) % count] = nv
        c[(k * 37) % count] = 3.0 + k                          # the maximum of both bounds sits on the negative variance
        cases.append(('var {}'.format(nv), None, None))
        rows_m.append(c)
        rows_v.append(v)
    sigmas = [0.0, 3.0, 6.0]
    ms, vs = _Guarded(engine, len(cases) * count, np.stack(rows_m)), _Guarded(engine, len(cases) * count, np.stack(rows_v))
    out = _Guarded(engine, 2 * len(cases) * len(sigmas))
    for s, ns in enumerate(sigmas):
        for k in range(len(cases)):
            _ffi.check(lib.dfq_moment_range(ms.ptr(k * count), vs.ptr(k * count), count, EPS, ns, out.ptr(2 * (s * len(cases) + k)),
                                            _ffi.stream_arg()))
    _ffi.synchronize()
    ms.check_unchanged('mean')
    vs.check_unchanged('var')
    out.check_guards('out2')
    got = out.numpy().reshape(len(sigmas), len(cases), 2)
    for s, ns in enumerate(sigmas):
        for k, (name, _, _) in enumerate(cases):
            sd = _sd(rows_v[k])
            lo, hi = _range_ref(rows_m[k], sd, ns)
            what = '{} channels, N {}, {}'.format(count, ns, name)
            assert_bitexact(got[s, k], np.array([lo, hi], dtype=F32), what)
            if name.startswith('nan'):
                assert np.isnan(got[s, k]).all(), what + ': a NaN must win both min and max'
            elif name.startswith('var'):
                assert np.isfinite(got[s, k]).all(), what + ': a negative variance gave a NaN range'
            elif name.startswith('min') or name.startswith('-inf'):
                assert got[s, k, 0] <= -49.0 and (count == 1 or abs(got[s, k, 1]) < 3), what
            elif name.startswith('max') or name.startswith('+inf'):
                assert got[s, k, 1] >= 49.0 and (count == 1 or abs(got[s, k, 0]) < 3), what


def _bn_ranges(engine, reqs, n_sigma, pool_w, pool_b):
    """reqs: [(offset into the pools, channels, relu mode)] -> [n][2] through ONE dfq_bn_ranges call on guarded buffers"""
    lib = _ffi.lib()
    arr = (_ffi.DfqBnRangeReq * len(reqs))(*[_ffi.DfqBnRangeReq(pool_w.addr(o), pool_b.addr(o), c, m) for o, c, m in reqs])
    out = _Guarded(engine, 2 * len(reqs))
    nbytes = int(lib.dfq_bn_ranges_scratch_bytes(len(reqs)))
    assert nbytes >= 24 * len(reqs)
    scratch = _Guarded(engine, (nbytes + 3) // 4, dtype=torch.int32)
    _ffi.check(lib.dfq_bn_ranges(arr, len(reqs), n_sigma, out.ptr(), scratch.ptr(), _ffi.stream_arg()))
    _ffi.synchronize()
    pool_w.check_unchanged('fake_weight')
    pool_b.check_unchanged('fake_bias')
    out.check_guards('out')
    scratch.check_guards('scratch')
    return out.numpy().reshape(len(reqs), 2)


def _clamped_ref(b, w, n_sigma, mode):
    lo, hi = _range_ref(b, w, n_sigma)
    lo, hi = float(lo), float(hi)
    if mode >= 1:
        lo = max(0., lo)                        # Python's max(0., NaN) is 0.
    if mode == 2:
        hi = min(6., hi)                        # ... and min(6., NaN) is 6.
    return np.array([lo, hi], dtype=F32)


@pytest.mark.parametrize('count', COUNTS)
def test_bn_ranges_planted(engine, count):
    """every planted case in every ReLU mode and for n_sigma 0, 3, 6: one request each, one call per n_sigma"""
    rng = np.random.RandomState(1000 + count)
    cases = _range_cases(count, rng)
    pool_b = _Guarded(engine, len(cases) * count, np.stack([c for _, c, _ in cases]))
    pool_w = _Guarded(engine, len(cases) * count, np.stack([x for _, _, x in cases]))
    reqs = [(k * count, count, mode) for k in range(len(cases)) for mode in (0, 1, 2)]
    for ns in (0.0, 3.0, 6.0):
        got = _bn_ranges(engine, reqs, ns, pool_w, pool_b)
        for r, (o, _, mode) in enumerate(reqs):
            name, c, x = cases[o // count]
            what = '{} channels, N {}, mode {}, {}'.format(count, ns, mode, name)
            assert_bitexact(got[r], _clamped_ref(c, x, ns, mode), what)
            if mode == 0 and name.startswith('nan'):
                assert np.isnan(got[r]).all(), what + ': a NaN must win both min and max'
            if mode == 0 and name.startswith('min'):
                assert got[r, 0] <= -49.0
            if mode == 0 and name.startswith('max'):
                assert got[r, 1] >= 49.0


@pytest.mark.parametrize('n_sigma', [0.0, 3.0, 6.0])
def test_bn_ranges_seven_requests(engine, n_sigma):
    """seven requests of different lengths and all ReLU modes in one call; a NaN request leaves its neighbours alone and is
    clamped as Python clamps it (max(0., NaN) = 0., min(6., NaN) = 6.)"""
    rng = np.random.RandomState(3)
    lengths = [1, 63, 257, 64, 1025, 256, 300]
    modes = [2, 0, 1, 2, 2, 0, 1]
    offs = np.concatenate([[0], np.cumsum(lengths)])
    w = rng.uniform(0.05, 1.5, offs[-1]).astype(F32)
    b = (rng.standard_normal(offs[-1]) * 2 + 1).astype(F32)
    b[offs[1]:offs[2]] -= 9.0                                   # a negative range without ReLU
    clean = _bn_ranges(engine, [(int(offs[i]), lengths[i], modes[i]) for i in range(7)], n_sigma, _Guarded(engine, len(w), w),
                       _Guarded(engine, len(b), b))
    for i in range(7):
        sl = slice(offs[i], offs[i + 1])
        assert_bitexact(clean[i], _clamped_ref(b[sl], w[sl], n_sigma, modes[i]), 'request {}'.format(i))
        assert np.isfinite(clean[i]).all()
    for victim, mode, want_nan in ((2, 1, [False, True]), (4, 2, [False, False]), (5, 0, [True, True])):
        b2 = b.copy()
        b2[offs[victim] + lengths[victim] - 1] = np.nan
        got = _bn_ranges(engine, [(int(offs[i]), lengths[i], modes[i]) for i in range(7)], n_sigma, _Guarded(engine, len(w), w),
                         _Guarded(engine, len(b2), b2))
        assert modes[victim] == mode and np.isnan(got[victim]).tolist() == want_nan
        if mode >= 1:
            assert got[victim, 0] == 0.0
        if mode == 2:
            assert got[victim, 1] == 6.0
        for i in range(7):
            if i != victim:
                assert (_bits(got[i]) == _bits(clean[i])).all(), 'request {} saw the NaN of request {}'.format(i, victim)


# ---- d. dfq_bn_through_layer ----------------------------------------------------------------------------------------------
SHAPES = [(1, 1, 1, 1), (5, 3, 9, 1), (8, 1, 9, 8), (6, 65, 1, 2), (7, 130, 4, 1), (12, 64, 25, 3)]


def _through_bound(w, v, bias, groups):
    """(float64 value, bound) per output row.  The kernel sums a row's taps in float32 one after the other (error at most
    gamma_{k-1} sum_k |w_k| per input, gamma_n = n u / (1 - n u)), multiplies and accumulates in float64 (I/g + 6 roundings of
    2^-53 on sum |ws v|), rounds the accumulator to float32 once and rounds the bias add once."""
    O, I, K = w.shape
    w64, v64 = w.astype(np.float64), v.astype(np.float64)
    vin = v64.reshape(groups, I)[np.arange(O) // (O // groups)]                # [O, I]
    exact_sum = (w64.sum(-1) * vin).sum(-1)
    gamma = (K - 1) * U / (1 - (K - 1) * U)
    e1 = (gamma * np.abs(w64).sum(-1) * np.abs(vin)).sum(-1)
    e1 = e1 + (I + 6) * 2.0 ** -53 * (np.abs(w64).sum(-1) * np.abs(vin)).sum(-1)
    e2 = U * (np.abs(exact_sum) + e1)
    exact = exact_sum + (0.0 if bias is None else bias.astype(np.float64))
    e3 = U * (np.abs(exact) + e1 + e2) if bias is not None else 0.0
    return exact, e1 + e2 + e3


@pytest.mark.parametrize('with_bias', [False, True])
@pytest.mark.parametrize('shape', SHAPES)
def test_bn_through_layer(engine, shape, with_bias):
    O, I, K, G = shape
    lib = _ffi.lib()
    rng = np.random.RandomState(O * 1000 + I)
    w = (rng.standard_normal((O, I, K)) * 0.5).astype(F32)
    if K > 1:                                                   # cancelling rows: large taps whose sum is near 0
        w[::2, :, 0] = 1000.0 + rng.standard_normal(w[::2, :, 0].shape).astype(F32)
        w[::2, :, 1] = -1000.0
    v = rng.uniform(0.5, 1.5, G * I).astype(F32)
    v.reshape(G, I)[np.arange(G), (np.arange(G) * 7 + I - 1) % I] = 1000.0 * (1 + np.arange(G))     # one dominant entry per group
    bias = (rng.standard_normal(O) * 3).astype(F32) if with_bias else None
    nan_row = O // 2

    def run(w, bias):
        ws, vs = _Guarded(engine, w.size, w), _Guarded(engine, v.size, v)
        bs = _Guarded(engine, O, bias) if bias is not None else None
        out = _Guarded(engine, O)
        _ffi.check(lib.dfq_bn_through_layer(ws.ptr(), O, I, K, G, bs.ptr() if bs else None, vs.ptr(), out.ptr(), _ffi.stream_arg()))
        _ffi.synchronize()
        ws.check_unchanged('weight')
        vs.check_unchanged('v_in')
        if bs:
            bs.check_unchanged('bias')
        out.check_guards('v_out')
        return out.numpy()

    got = run(w, bias)
    exact, bound = _through_bound(w, v, bias, G)
    err = np.abs(got.astype(np.float64) - exact)
    print('{} bias {}: worst error / bound {:.3f}'.format(shape, with_bias, float((err / bound).max())))
    assert (err <= bound).all(), 'rows {}: error {} > bound {}'.format(np.flatnonzero(err > bound).tolist(), err, bound)
    # a NaN in one row's weights, or in its bias, gives NaN in that row alone
    w2 = w.copy()
    w2[nan_row, I - 1, K - 1] = np.nan
    got2 = run(w2, bias)
    assert np.isnan(got2[nan_row]) and (_bits(np.delete(got2, nan_row)) == _bits(np.delete(got, nan_row))).all()
    if with_bias:
        b2 = bias.copy()
        b2[O - 1] = np.nan
        got3 = run(w, b2)
        assert np.isnan(got3[O - 1]) and (_bits(got3[:O - 1]) == _bits(got[:O - 1])).all()


def test_bn_through_layer_rejects_bad_geometry(engine):
    lib = _ffi.lib()
    buf = _Guarded(engine, 64, np.ones(64, dtype=F32))
    out = _Guarded(engine, 8)
    for O, I, K, G in ((0, 1, 1, 1), (8, 0, 1, 1), (8, 1, 0, 1), (8, 1, 1, 0), (8, 1, 1, 3)):
        assert lib.dfq_bn_through_layer(buf.ptr(), O, I, K, G, None, buf.ptr(), out.ptr(), _ffi.stream_arg()) == DFQ_ERR_ARG
    assert lib.dfq_bn_through_layer(None, 8, 1, 1, 1, None, buf.ptr(), out.ptr(), _ffi.stream_arg()) == DFQ_ERR_ARG
    _ffi.synchronize()
    out.check_unchanged('a refused call wrote')


# ---- e. the batch plan on the same values -----------------------------------------------------------------------------------
def _finite_pool(mode):
    """channels of section a whose moments are finite in `mode`, the finding first"""
    w, b, planted = _INPUTS
    keep = np.ones(len(w), dtype=bool)
    keep[planted[1] + planted[2]] = False
    keep &= np.abs(b) < 1e3                                     # (b^2 of 1e4 would own every maximum)
    if mode == 2:
        om, ov = orc.moments_relu6(w, b)
        order = np.argsort(np.where(keep, ov, np.inf), kind='stable')      # the most negative variances first
        return w[order[:keep.sum()]], b[order[:keep.sum()]]
    return w[keep], b[keep]


def _chain(engine, program, vectors, n_sigma):
    """a MOM ... MOM_RANGE program through the single-network entry points; vectors: {name: numpy}"""
    lib = _ffi.lib()
    mean = var = None
    for op, name, mode in program:
        if op == _ffi.ACT_MOM:
            mean, var = _relu_moments(engine, vectors[name + 'w'], vectors[name + 'b'], mode)
        elif op == _ffi.ACT_MOM_ADD:
            mean, var = _relu_moments(engine, vectors[name + 'w'], vectors[name + 'b'], mode, old=(mean, var))
        elif op == _ffi.ACT_MOM_RELU:
            ms, vs = _Guarded(engine, len(mean), mean), _Guarded(engine, len(var), var)
            _ffi.check(lib.dfq_moments_after_add(ms.ptr(), vs.ptr(), len(mean), mode, EPS, _ffi.stream_arg()))
            _ffi.synchronize()
            mean, var = ms.numpy(), vs.numpy()
        else:
            ms, vs, out = _Guarded(engine, len(mean), mean), _Guarded(engine, len(var), var), _Guarded(engine, 2)
            _ffi.check(lib.dfq_moment_range(ms.ptr(), vs.ptr(), len(mean), EPS, n_sigma, out.ptr(), _ffi.stream_arg()))
            _ffi.synchronize()
            return out.numpy(), mean, var


def test_batch_plan_on_adversarial_vectors(engine):
    """DFQ_ACT_MOM / MOM_ADD / MOM_RELU / MOM_RANGE programs over two networks whose vectors are those of sections a to c, with
    257 and 1025 channels: bit-equal to the chain of single-network calls, and finite where the chain's inputs are -- the
    ReLU6 band and its negative variances included, so the batch path is held to the clamp and not to a copy of its absence."""
    A = _ffi
    lib = A.lib()
    rng = np.random.RandomState(42)
    w6, b6 = _finite_pool(2)
    w1, b1 = _finite_pool(1)
    assert len(w6) >= 1400 and len(w1) >= 1400
    _, neg = orc.moments_relu6(w6[:40], b6[:40])
    assert (neg < 0).sum() >= 30 and (neg < -EPS).sum() >= 1, 'the pool lost its negative variances'

    def vectors(net):
        """per network: a..f, (w, b) each; `a`, `c`: the ReLU6 pool, most negative variances in front; `b`, `d`: dead channels
        with a small mean (variance 0: the sum stays negative); `e`, `f`: the ReLU pool"""
        out = {}
        for name, c in (('a', 257), ('c', 1025)):
            sel = np.concatenate([np.arange(24), 24 + rng.permutation(len(w6) - 24)[:c - 24]])
            sel = sel[rng.permutation(c)] if net else sel
            out[name + 'w'], out[name + 'b'] = w6[sel], b6[sel]
        for name, c in (('b', 257), ('d', 1025)):
            out[name + 'w'] = np.where(rng.uniform(size=c) < 0.5, 0.0, rng.uniform(0, 2e-3, c)).astype(F32)
            out[name + 'b'] = (rng.uniform(-0.01, 0.01, c) - (0.2 if net else 0.0)).astype(F32)
        for name, c in (('e', 257), ('f', 1025)):
            sel = rng.permutation(len(w1))[:c]
            out[name + 'w'], out[name + 'b'] = w1[sel], b1[sel]
        out['gw'], out['gb'] = out['ew'].copy(), out['eb'].copy()          # ... and one vector with a NaN-producing channel
        out['gw'][200], out['gb'][200] = 0.0, 0.0
        return out

    nets = [vectors(0), vectors(1)]
    names = sorted(nets[0])
    offs, at = {}, 0
    for k in names:
        offs[k] = at
        at += -(-len(nets[0][k]) // 64) * 64
    stride = at
    host = np.full((2, stride), SENTINEL, dtype=F32)
    for n in range(2):
        for k in names:
            host[n, offs[k]:offs[k] + len(nets[n][k])] = nets[n][k]
    buf = _Guarded(engine, 2 * stride, host)
    programs = [
        [(A.ACT_MOM, 'a', 2), (A.ACT_MOM_ADD, 'b', 0), (A.ACT_MOM_RELU, None, 2), (A.ACT_MOM_RANGE, None, 0)],
        [(A.ACT_MOM, 'a', 2), (A.ACT_MOM_ADD, 'b', 0), (A.ACT_MOM_RANGE, None, 0)],                       # negative variance -> range
        [(A.ACT_MOM, 'c', 2), (A.ACT_MOM_ADD, 'd', 0), (A.ACT_MOM_RELU, None, 1), (A.ACT_MOM_ADD, 'f', 1), (A.ACT_MOM_RANGE, None, 0)],
        [(A.ACT_MOM, 'd', 0), (A.ACT_MOM_ADD, 'c', 2), (A.ACT_MOM_RANGE, None, 0)],
        [(A.ACT_MOM, 'f', 1), (A.ACT_MOM_ADD, 'c', 2), (A.ACT_MOM_RELU, None, 2), (A.ACT_MOM_RELU, None, 1), (A.ACT_MOM_RANGE, None, 0)],
        [(A.ACT_MOM, 'e', 1), (A.ACT_MOM_ADD, 'a', 2), (A.ACT_MOM_ADD, 'b', 1), (A.ACT_MOM_RANGE, None, 0)],
        [(A.ACT_MOM, 'c', 2), (A.ACT_MOM_RANGE, None, 0)],
        [(A.ACT_MOM, 'g', 1), (A.ACT_MOM_ADD, 'a', 2), (A.ACT_MOM_RELU, None, 2), (A.ACT_MOM_RANGE, None, 0)],       # NaN: 0 / 0 at channel 200
    ]
    S = A.DfqBatchActStep
    steps, results = [], []
    for prog in programs:
        results.append(A.DfqBatchActResult(len(steps), len(prog)))
        for op, name, mode in prog:
            if name is None:
                steps.append(S(None, None, op, 0, mode, 0, -1, -1, 0, 0))
            else:
                steps.append(S(buf.addr(offs[name + 'w']), buf.addr(offs[name + 'b']), op, len(nets[0][name + 'w']), mode, 0, -1, -1, 0, 0))
    for n_sigma in (6.0, 3.0):
        out = _Guarded(engine, 2 * 2 * len(programs))
        bases = (ctypes.c_void_p * 2)(buf.addr(0), buf.addr(stride))
        plan = ctypes.c_void_p()
        A.check(lib.dfq_batch_act_plan_create((A.DfqBatchActResult * len(results))(*results), len(results), (S * len(steps))(*steps), len(steps),
                                              None, 0, bases, 2, ctypes.c_float(n_sigma), ctypes.c_float(EPS), out.ptr(), 2 * len(programs),
                                              ctypes.byref(plan)))
        try:
            assert lib.dfq_batch_act_plan_launches(plan) == 1
            A.check(lib.dfq_batch_act_plan_run(plan, A.stream_arg()))
            A.synchronize()
        finally:
            lib.dfq_batch_act_plan_destroy(plan)
        buf.check_unchanged('the networks')
        out.check_guards('the ranges')
        got = out.numpy().reshape(2, len(programs), 2)
        for n in range(2):
            for q, prog in enumerate(programs):
                want, mean, var = _chain(engine, prog, nets[n], n_sigma)
                what = 'N {}, network {}, program {}'.format(n_sigma, n, q)
                assert_bitexact(got[n, q], want, what)
                if q == len(programs) - 1:
                    assert np.isnan(got[n, q]).all(), what
                else:
                    assert np.isfinite(got[n, q]).all(), what + ': {} (a rounding-negative variance became a NaN range)'.format(got[n, q])
                if q in (1, 3, 6):
                    assert (var < -EPS).any(), what + ': no variance below -eps reached the range step'


# ---- f. the finding, end to end ----------------------------------------------------------------------------------------------
def test_narrow_channel_on_the_relu6_ceiling_end_to_end(engine):
    """lt.set_quant_minmax and NetworkBatch.act_range_plan on tiny_res: the stem's BatchNorm channel 3 is the channel of the
    finding, and the channel it is added to (l1.bn2) is dead, so the sum's variance is -6.8e-6 and sqrt(var + eps) was NaN:
    running_min / running_max of the next layers became NaN.  synthetic.build keeps tiny_res's nn.ReLU whatever keep_relu6
    says (the model has no ReLU6 to keep), so the test puts nn.ReLU6 modules into the graph in their place: the walk reads
    only the type."""
    from tests.test_batch_act import _prepared, _single
    nets = [_prepared('tiny_res', s, engine.device, relu6=True) for s in (0, 1)]
    for graph, bottoms, _ in nets:
        for k in list(graph):
            if type(graph[k]) == nn.ReLU:
                graph[k] = nn.ReLU6()
    batch = arena.NetworkBatch(nets, TARG)
    graph = nets[1][0]
    bns = [m for m in graph.values() if isinstance(m, nn.BatchNorm2d) and hasattr(m, 'fake_bias')]
    with torch.no_grad():
        bns[0].fake_weight[3], bns[0].fake_bias[3] = W_Q, B_Q          # stem: BN -> ReLU6 -> maxpool -> l1's add
        bns[2].fake_weight[3], bns[2].fake_bias[3] = 0.0, 0.0          # l1.bn2
    single = _single(graph, nets[1][1], engine.device)
    plan = batch.act_range_plan()
    plan.run()
    _ffi.synchronize()
    flat = [r for v in single.values() for r in (v if isinstance(v, list) else [v])]
    assert len(flat) >= 8
    for k, r in zip(single, flat):
        assert bool(torch.isfinite(r).all()), 'set_quant_minmax left {} at {}'.format(r.tolist(), k)
    for n in range(2):
        for k, r in plan.ranges(n).items():
            assert bool(torch.isfinite(r).all()), 'act_range_plan, network {}: {} at {}'.format(n, r.tolist(), k)
    for (k, r), s in zip(plan.ranges(1).items(), flat):
        assert torch.equal(r.cpu().view(torch.int32), s.view(torch.int32)), k
    # the planted channel does reach the quantisers behind the add (a min / max over channels shows a finite channel only when
    # it is the extreme one, so the probe is a NaN in its place): the ranges that were NaN before the clamp
    with torch.no_grad():
        bns[0].fake_bias[3] = math.nan
    probe = _single(graph, nets[1][1], engine.device)
    hit = [k for k, r in probe.items() if bool(torch.isnan(r).any())]
    assert len(hit) >= 2 and 'Conv2d_12' in hit, hit
    plan.close()
