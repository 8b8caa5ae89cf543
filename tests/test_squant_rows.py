"""dfq_squant_rows / prims.squant_rows: adaptive rounding (SQuant) of one [rows, row_len] tensor.

The reference is `squant_ref` below, a numpy restatement of the DEFINITION in include/dfq_hip.h ("Adaptive rounding").  The
definition is integer-exact (every sum is a sum of P = rint(p * 2^30)), so every comparison here is exact: codes, stored
weights (as bit patterns), stats.  tests/test_batch_squant.py imports the restatement from here."""
import math

import numpy as np
import pytest
import torch

from dfq_amd import _ffi, prims

DFQ_ERR_ARG = -1     # include/dfq_hip.h
ONE, HALF = 1 << 30, 1 << 29
F32 = np.float32


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def qparams(mn, mx, bits, signed):
    """qparams_double: the float64 recipe, every result cast to float32 -> (qmin, qmax, neg_min, scale, min_value)"""
    mn, mx = float(mn), float(mx)
    if signed:
        qmin, qmax = -float(1 << (bits - 1)), float((1 << (bits - 1)) - 1)
        mx, mn = abs(mx), abs(mn)
        if mx < mn:
            mx = mn
        scale = mx / qmax
        mn = 0.0
    else:
        qmin, qmax = 0.0, float(1 << bits) - 1.0
        scale = (mx - mn) / (qmax - qmin)
    if 1e-8 > scale:
        scale = 1e-8
    with np.errstate(over='ignore'):
        return F32(qmin), F32(qmax), F32(-mn), F32(scale), F32(mn)


def row_range(row):
    """(min, max) with NaN skipped; nothing but NaN: (NaN, NaN)"""
    ok = row[~np.isnan(row)]
    return (F32(ok.min()), F32(ok.max())) if ok.size else (F32(np.nan), F32(np.nan))


def _first(keys, n):
    """the first n candidates (key > 0) by key descending, then by index ascending; there are at least n"""
    cand = np.flatnonzero(keys > 0)
    assert len(cand) >= n, 'the definition promises {} candidates, there are {}'.format(n, len(cand))
    return cand[np.lexsort((cand, -keys[cand]))][:n]


def squant_row(w, K, bits, signed, mn, mx):
    """one row -> (stored float32, codes int64, nearest codes c0 as float32, (sum of P, flips), scale)"""
    qmin, qmax, neg_min, scale, min_value = qparams(mn, mx, bits, signed)
    with np.errstate(all='ignore'):
        t = (w + neg_min) / scale
        t = np.where(t < qmin, qmin, t)             # NaN-propagating clamp, as torch.clamp_
        t = np.where(t > qmax, qmax, t).astype(F32)
        c0 = np.rint(t)
        p = (c0 - t).astype(F32)
    finite = all(np.isfinite(v) for v in (neg_min, scale, min_value))
    c = c0.copy()
    stats = (0, 0)
    if finite and not np.isnan(t).any():
        P = np.rint(p.astype(np.float64) * ONE).astype(np.int64)
        G = len(w) // K
        if K > 1:
            for j in range(G):
                pk = P[j * K:(j + 1) * K]
                e = int(pk.sum())
                n, s = (abs(e) + HALF) >> 30, (e > 0) - (e < 0)
                at = _first(s * pk, n)
                pk[at] -= s * ONE
                c[j * K + at] -= s
                assert abs(int(pk.sum())) <= HALF
        e_j = P.reshape(G, K).sum(1)
        E = int(e_j.sum())
        N, S = (abs(E) + HALF) >> 30, (E > 0) - (E < 0)
        for j in _first(S * e_j, N):
            keys = S * P[j * K:(j + 1) * K]
            k = int(np.argmax(keys))                # the lowest index on a tie
            assert keys[k] > 0
            P[j * K + k] -= S * ONE
            c[j * K + k] -= S
        stats = (int(P.sum()), int((c != c0).sum()))
        assert abs(stats[0]) <= HALF and np.abs(P.reshape(G, K).sum(1)).max() <= ONE
        assert np.abs(c - c0).max() <= 1 and c.min() >= qmin and c.max() <= qmax
    with np.errstate(all='ignore'):
        y = (c.astype(F32) * scale).astype(F32) + min_value
    codes = np.where(np.isnan(c), 0, c).astype(np.int64)
    return y.astype(F32), codes, c0, stats, scale


def squant_ref(x, K, bits, signed, mins=None, maxs=None):
    """[rows, row_len] float32 -> dict(y, codes, c0, stats [rows, 2], ranges [rows, 2], scale [rows])"""
    x = np.ascontiguousarray(x, dtype=F32)
    rows = x.shape[0]
    out = dict(y=np.empty_like(x), codes=np.empty(x.shape, np.int64), c0=np.empty_like(x), stats=np.zeros((rows, 2), np.int64),
               ranges=np.empty((rows, 2), F32), scale=np.empty(rows, F32))
    for r in range(rows):
        mn, mx = row_range(x[r]) if mins is None else (F32(mins[r]), F32(maxs[r]))
        out['y'][r], out['codes'][r], out['c0'][r], out['stats'][r], out['scale'][r] = squant_row(x[r], K, bits, signed, mn, mx)
        out['ranges'][r] = (mn, mx)
    return out


def bits_of(a):
    """the bit patterns; every NaN as one pattern (the sign and payload of a NaN an operation makes are the machine's)"""
    a = np.ascontiguousarray(a, dtype=F32)
    return np.where(np.isnan(a), np.uint32(0x7fc00000), a.view(np.uint32))


# ---- the library against it -----------------------------------------------------------------------------------------------------
def run(engine, x, K, bits, signed, mins=None, maxs=None, in_place=False):
    """prims.squant_rows, or the C call in place -> (y, codes, stats) as numpy"""
    xd = torch.from_numpy(np.array(x, dtype=F32)).to(engine.device)       # (a copy: in place must not reach the caller's x)
    md = None if mins is None else torch.from_numpy(np.asarray(mins, F32)).to(engine.device)
    Md = None if maxs is None else torch.from_numpy(np.asarray(maxs, F32)).to(engine.device)
    if in_place:
        codes = torch.empty(xd.shape, dtype=torch.int32, device=engine.device)
        stats = torch.empty((xd.shape[0], 2), dtype=torch.int64, device=engine.device)
        _ffi.check(_ffi.lib().dfq_squant_rows(_ffi.ptr(xd), _ffi.ptr(xd), xd.shape[0], xd.shape[1], K, _ffi.ptr(md), _ffi.ptr(Md), bits,
                                              int(signed), _ffi.ptr(codes), _ffi.ptr(stats), _ffi.stream_arg()))
        _ffi.synchronize()
        y = xd
    else:
        y, codes, stats = prims.squant_rows(xd, K, bits, md, Md, signed, return_codes=True, return_stats=True)
        assert torch.equal(xd.cpu(), torch.from_numpy(np.ascontiguousarray(x, dtype=F32))) or np.isnan(x).any()
    return y.cpu().numpy(), codes.cpu().numpy().astype(np.int64), stats.cpu().numpy()


def check(engine, x, K, bits, signed, given=False, in_place=False, what=''):
    mins = maxs = None
    if given:                                       # per tensor: every row the tensor's pair
        mn, mx = row_range(np.asarray(x, F32).reshape(-1))
        mins, maxs = np.full(x.shape[0], mn, F32), np.full(x.shape[0], mx, F32)
    want = squant_ref(x, K, bits, signed, mins, maxs)
    y, codes, stats = run(engine, x, K, bits, signed, mins, maxs, in_place)
    tag = '{} K={} bits={} signed={} given={} in_place={}'.format(what, K, bits, signed, given, in_place)
    assert np.array_equal(codes, want['codes']), tag + ': codes'
    assert np.array_equal(bits_of(y), bits_of(want['y'])), tag + ': stored weights'
    assert np.array_equal(stats, want['stats']), tag + ': stats'
    # the invariants, on the library's own output
    qmin, qmax = (-(1 << (bits - 1)), (1 << (bits - 1)) - 1) if signed else (0, (1 << bits) - 1)
    assert np.abs(stats[:, 0]).max() <= HALF, tag
    ok = ~np.isnan(want['c0'])
    assert np.abs(codes - np.where(ok, want['c0'], 0).astype(np.int64))[ok].max(initial=0) <= 1, tag
    assert codes.min() >= qmin and codes.max() <= qmax, tag
    for r in range(x.shape[0]):
        _, _, _, _, min_value = qparams(want['ranges'][r, 0], want['ranges'][r, 1], bits, signed)
        with np.errstate(all='ignore'):
            again = (codes[r].astype(F32) * want['scale'][r]).astype(F32) + min_value
        assert np.array_equal(bits_of(y[r])[ok[r]], bits_of(again)[ok[r]]), tag + ': y == c * scale + min'
    return want, stats


MODES = [(bits, signed, given) for bits in (2, 4, 8) for signed in (False, True) for given in (False, True)]


def all_modes(engine, x, K, what):
    """every mode on a small tensor; four of them, a different four from shape to shape, where the tensor is large (each mode
    is still met at every row-length class)"""
    flips = 0
    modes = list(enumerate(MODES))
    if x.size > 4096:
        first = (x.shape[0] + x.shape[1] + K) % 3
        modes = modes[first::3]
    for i, (bits, signed, given) in modes:
        _, stats = check(engine, x, K, bits, signed, given, in_place=i % 2 == 1, what=what)
        flips += int(stats[:, 1].sum())
    return flips


@pytest.mark.parametrize('rows', [1, 3, 67])
@pytest.mark.parametrize('row_len', [1, 2, 63, 64, 65, 257, 1280])
def test_linear_rows(engine, rows, row_len):
    rng = np.random.default_rng(1000 * rows + row_len)
    x = (rng.standard_normal((rows, row_len)) * rng.uniform(0.05, 2.0, (rows, 1))).astype(F32)
    flips = all_modes(engine, x, 1, 'K=1 [{}, {}]'.format(rows, row_len))
    assert flips > 0 or row_len <= 2


@pytest.mark.parametrize('K,G', [(9, 1), (9, 7), (9, 65), (4, 5), (25, 2), (49, 3),
                                 (9, 256), (96, 2), (3, 1000), (1024, 2)])   # the last four: the kernel's other paths
def test_kernels(engine, K, G):
    """G kernels of K: the listed shapes, then a row of the workgroup class with short kernels (2304), kernels longer than one
    lane selects on its own inside a wave (96 x 2) and inside the workgroup (1024 x 2), and many short kernels (3 x 1000)"""
    rng = np.random.default_rng(100 * K + G)
    rows = 3 if K * G > 1000 else 5
    x = (rng.standard_normal((rows, K * G)) * rng.uniform(0.05, 2.0, (rows, 1))).astype(F32)
    assert all_modes(engine, x, K, '[{}, {} x {}]'.format(rows, G, K)) > 0


def test_longest_row(engine):
    lib = _ffi.lib()
    most = int(lib.dfq_squant_max_row_len())
    assert most >= 16384
    rng = np.random.default_rng(7)
    x = rng.standard_normal((1, most)).astype(F32)
    check(engine, x, 1, 4, False, what='longest row')
    check(engine, x, 4, 8, True, in_place=True, what='longest row')
    xd = torch.zeros((1, most + 1), device=engine.device)
    rc = lib.dfq_squant_rows(_ffi.ptr(xd), _ffi.ptr(xd), 1, most + 1, 1, None, None, 8, 0, None, None, _ffi.stream_arg())
    assert rc == DFQ_ERR_ARG and b'dfq_squant_max_row_len' in lib.dfq_last_error()
    with pytest.raises(_ffi.DfqError):
        prims.squant_rows(xd)


def adversarial(row_len, rng):
    """rows of `row_len` >= 8 that press on the selection"""
    u = rng.uniform(0.0, 15.0, row_len)
    two = np.where(rng.integers(0, 2, row_len) == 1, 4.3, 9.7)
    two[0], two[-1] = 0.0, 15.0                       # two values and the extremes: nothing but equal keys
    near = np.floor(u) + 0.49
    near[0], near[-1] = 0.0, 15.0                     # p near +0.49 everywhere: N is about row_len / 2
    halves = np.floor(u) + 0.5
    halves[0], halves[-1] = 0.0, 15.0                 # exactly on .5 (at 4 bits the scale is 1): |e| may equal HALF
    const = np.full(row_len, 0.37)                    # the scale floor of 1e-8
    nan = u.copy()
    nan[row_len // 2] = np.nan
    inf = u.copy()
    inf[1] = np.inf
    return np.stack([two, near, halves, const, nan, inf, u]).astype(F32)


@pytest.mark.parametrize('K,row_len', [(1, 8), (1, 200), (1, 1280), (9, 9 * 31), (4, 2048), (1, 4000)])
def test_adversarial_rows(engine, K, row_len):
    x = adversarial(row_len, np.random.default_rng(row_len + K))
    for bits, signed in ((4, False), (8, False), (2, True), (4, True)):
        want, stats = check(engine, x, K, bits, signed, what='adversarial', in_place=signed)
        # the NaN row and the +inf row fall back to nearest: bit for bit what dfq_fake_quant_rows stores
        xd = torch.from_numpy(x[4:6]).to(engine.device)
        near = prims.fake_quant_rows(xd, bits, symmetric=signed).cpu().numpy()
        got = run(engine, x[4:6], K, bits, signed)[0]
        assert np.array_equal(near.view(np.uint32), got.view(np.uint32)) and np.array_equal(bits_of(near), bits_of(want['y'][4:6]))
        assert not stats[4:6].any()
    if K == 1 and row_len >= 200:
        _, stats = check(engine, x, K, 4, False, what='adversarial')
        assert stats[1, 1] >= row_len // 3, 'the +0.49 row flips about half of its elements, got {}'.format(stats[1, 1])
    # given ranges: the finite rows share one pair; one row far outside it is clamped everywhere and nothing flips
    fin = np.concatenate([x[:4], x[6:], x[6:] + F32(1000.0)])
    mins, maxs = np.full(len(fin), 0.0, F32), np.full(len(fin), 15.0, F32)
    want = squant_ref(fin, K, 4, False, mins, maxs)
    y, codes, stats = run(engine, fin, K, 4, False, mins, maxs)
    assert np.array_equal(codes, want['codes']) and np.array_equal(bits_of(y), bits_of(want['y'])) and np.array_equal(stats, want['stats'])
    assert not stats[-1].any() and (codes[-1] == 15).all()


def test_argument_errors(engine):
    lib = _ffi.lib()
    x = torch.zeros((4, 18), device=engine.device)
    m = torch.zeros(4, device=engine.device)

    def rc(xp, yp, rows, row_len, K, mins, maxs, bits):
        return lib.dfq_squant_rows(xp, yp, rows, row_len, K, mins, maxs, bits, 0, None, None, _ffi.stream_arg())
    p = _ffi.ptr(x)
    assert rc(p, p, 4, 18, 9, None, None, 8) == 0
    for bad in [(None, p, 4, 18, 9, None, None, 8), (p, None, 4, 18, 9, None, None, 8), (p, p, 0, 18, 9, None, None, 8),
                (p, p, 4, 0, 9, None, None, 8), (p, p, 4, 18, 9, None, None, 1), (p, p, 4, 18, 9, None, None, 17),
                (p, p, 4, 18, 4, None, None, 8), (p, p, 4, 18, 0, None, None, 8), (p, p, 4, 18, 9, _ffi.ptr(m), None, 8)]:
        assert rc(*bad) == DFQ_ERR_ARG, bad
        assert b'dfq_squant_rows' in lib.dfq_last_error()
    _ffi.synchronize()


def test_plan_argument_errors(engine):
    import ctypes
    lib = _ffi.lib()
    w = torch.zeros((4, 18), device=engine.device)
    codes = torch.zeros(128, dtype=torch.int32, device=engine.device)
    ranges = torch.zeros(16, device=engine.device)
    stats = torch.zeros(16, dtype=torch.int64, device=engine.device)
    bases = (ctypes.c_void_p * 1)(w.data_ptr())

    def create(t, code_bytes=4, code_stride=128, range_stride=16, stats_stride=16, n_nets=1, n=1, base=bases):
        plan = ctypes.c_void_p()
        arr = (_ffi.DfqBatchSquantTensor * 1)(t)
        rc = lib.dfq_batch_squant_plan_create(arr if n else None, n, base, n_nets, codes.data_ptr(), code_bytes, code_stride,
                                              ranges.data_ptr(), range_stride, stats.data_ptr(), stats_stride, ctypes.byref(plan))
        if rc == 0:
            lib.dfq_batch_squant_plan_destroy(plan)
        return rc

    def tensor(rows=4, row_len=18, bits=8, per_row=1, c=0, r=0, K=9, s=0, data=w.data_ptr()):
        return _ffi.DfqBatchSquantTensor(data, rows, row_len, bits, 0, per_row, 0, c, r, K, s)
    assert create(tensor()) == 0
    assert lib.dfq_batch_squant_plan_launches(None) == 0
    for rc in [create(tensor(), n=0), create(tensor(), n_nets=0), create(tensor(), base=None), create(tensor(data=None)),
               create(tensor(rows=0)), create(tensor(bits=1)), create(tensor(bits=17)), create(tensor(K=4)), create(tensor(K=0)),
               create(tensor(rows=1, row_len=int(lib.dfq_squant_max_row_len()) + 9)), create(tensor(bits=9), code_bytes=1),
               create(tensor(), code_bytes=2), create(tensor(c=128 - 71)), create(tensor(r=9)), create(tensor(s=9)),
               create(tensor(per_row=0, r=15)), create(tensor(c=-2))]:
        assert rc == DFQ_ERR_ARG
        assert b'dfq_batch_squant_plan_create' in lib.dfq_last_error()
    assert create(tensor(bits=8), code_bytes=1) == 0 and create(tensor(c=128 - 72, r=8, s=8)) == 0
    assert lib.dfq_batch_squant_plan_run(None, None) == DFQ_ERR_ARG
