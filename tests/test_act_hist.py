"""dfq_act_hist_accumulate and dfq_hist_clip_range (dfq_act_hist.hip) through the C ABI and dfq_amd.prims: the histogram of a
quantiser's input and the clipped range read off it.

The numpy restatements below restate the rules of include/dfq_hip.h literally.

Histogram: every one of the bins + 3 slots must be EQUAL -- counts are integers, there is no tolerance.

Selection: percentile results are integers and one rounding, so they must be EQUAL.  The MSE search compares float64 sums of
bins non-negative terms that the kernel adds in an order of its own; any-order recursive summation in a format of unit
roundoff u = 2^-53 is within n u sum|term| of the exact sum (Higham (4.4), as tests/test_batch_error.py uses it), and the
restatement's own sum is within the same bound, so: the returned pair must be candidate edges (exact float32 equality with
edge(.)), and for each of the two searches the restatement's err at the returned candidate must be <= the restatement's minimum
over all candidates + 2 bins 2^-53 sum_b n_b d_b^2 at that candidate."""
import ctypes
import functools
import math
import os
import subprocess

import numpy as np
import pytest
import torch

from dfq_amd import _ffi, prims

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DFQ_ERR_ARG = -1     # include/dfq_hip.h
F32 = np.float32
U = 2.0 ** -53
P = 4096             # kHistRound of dfq_act_hist.hip: floats one workgroup reads per round; a piece is ONE round up to
GROUPS = 1024        # P * GROUPS elements, then as many rounds (at most 32) as leave about GROUPS workgroups
SIZES = [1, 3, 4, 5, 63, 64, 65, 255, 257, P - 1, P, P + 1, 2 * P + 1, 3 * P + 7]
BINS = [2, 16, 2047, 2048, 4096]
QNAN = np.array([0x7fc00000], dtype=np.uint32).view(F32)[0]
NEG_SNAN = np.array([0xffa00000], dtype=np.uint32).view(F32)[0]      # negative, signalling


# ---- the rules, restated ---------------------------------------------------------------------------------------------------
def ref_slots(x, lo, hi, bins):
    """the slot of every element: include/dfq_hip.h, in float32"""
    x = np.ascontiguousarray(x, dtype=F32)
    lo, hi = F32(lo), F32(hi)
    with np.errstate(all='ignore'):
        w = F32(hi - lo)
        degenerate = not (np.isfinite(w) and w > 0)
        if degenerate:
            s = np.where(x < lo, bins, np.where(x > hi, bins + 1, 0))
        else:
            inv = F32(F32(bins) / w)
            t = ((x - lo).astype(F32) * inv).astype(F32)
            inside = np.where(t > 0, np.trunc(np.where(t > 0, np.minimum(t, F32(bins)), 0)), 0).astype(np.int64)
            s = np.where(t < 0, bins, np.where(t >= F32(bins), np.where(x <= hi, bins - 1, bins + 1), inside))
        s = np.where(np.isnan(x), bins + 2, s)
    return s.astype(np.int64)


def ref_hist(x, lo, hi, bins):
    return np.bincount(ref_slots(x, lo, hi, bins).reshape(-1), minlength=bins + 3).astype(np.int64)


def ref_degenerate(lo, hi):
    with np.errstate(all='ignore'):
        w = F32(F32(hi) - F32(lo))
    return not (np.isfinite(w) and w > 0)


def ref_edges(lo, hi, bins):
    lo64, hi64 = float(F32(lo)), float(F32(hi))
    e = (lo64 + np.arange(bins + 1, dtype=np.float64) * (hi64 - lo64) / bins).astype(F32)
    e[0], e[bins] = F32(lo), F32(hi)
    return e


def ref_reps(lo, hi, bins):
    lo64, hi64 = float(F32(lo)), float(F32(hi))
    r = (lo64 + (np.arange(bins, dtype=np.float64) + 0.5) * (hi64 - lo64) / bins).astype(F32)
    r[0], r[bins - 1] = F32(lo), F32(hi)
    return r


def ref_nb(counts, bins):
    nb = np.array(counts[:bins], dtype=np.int64)
    nb[0] += counts[bins]
    nb[bins - 1] += counts[bins + 1]
    return nb


def ref_fq(v, l, h, bits):
    """dfq_fake_quant's asymmetric recipe with a float64 scale: five separately rounded float32 operations on v"""
    l64, h64 = float(F32(l)), float(F32(h))
    scale = F32(max((h64 - l64) / (2.0 ** bits - 1.0), 1e-8))
    qmax = F32(2.0 ** bits - 1.0)
    v = np.asarray(v, dtype=F32)
    q = (v + F32(-l64)).astype(F32)
    q = (q / scale).astype(F32)
    q = np.where(q < 0, F32(0), q)
    q = np.where(q > qmax, qmax, q)
    q = np.rint(q).astype(F32)
    y = (q * scale).astype(F32)
    return (y + F32(l64)).astype(F32)


def ref_err(nb, reps, l, h, bits):
    d = ref_fq(reps, l, h, bits).astype(np.float64) - reps.astype(np.float64)
    return float(np.sum(nb.astype(np.float64) * (d * d)))


def ref_percentile(counts, lo, hi, bins, p):
    nb = ref_nb(counts, bins)
    total = int(nb.sum())
    if ref_degenerate(lo, hi) or total == 0:
        return F32(lo), F32(hi)
    k = int(min(max(math.ceil(p * float(total)), 1.0), float(total)))
    k = min(k, total)
    e = ref_edges(lo, hi, bins)
    b_hi = int(np.argmax(np.cumsum(nb) >= k))
    b_lo = int(np.flatnonzero(np.cumsum(nb[::-1])[::-1] >= k)[-1])
    return e[b_lo], e[b_hi + 1]


def assert_mse_choice(got, counts, lo, hi, bins, bits, C, what):
    """the rule of the module docstring; returns nothing"""
    nb = ref_nb(counts, bins)
    if ref_degenerate(lo, hi) or int(nb.sum()) == 0:
        assert got[0] == F32(lo) and got[1] == F32(hi), what
        return
    e, reps = ref_edges(lo, hi, bins), ref_reps(lo, hi, bins)
    k_h = [k for k in range(C) if e[bins - k] == got[1]]
    assert k_h, '{}: hi = {!r} is no candidate edge'.format(what, got[1])
    errs = [ref_err(nb, reps, F32(lo), e[bins - k], bits) for k in range(C)]
    assert errs[k_h[0]] <= min(errs) + 2 * bins * U * errs[k_h[0]], '{}: upper search {} against {}'.format(what, errs[k_h[0]], min(errs))
    k_l = [k for k in range(C) if e[k] == got[0]]
    assert k_l, '{}: lo = {!r} is no candidate edge'.format(what, got[0])
    errs = [ref_err(nb, reps, e[k], got[1], bits) for k in range(C)]
    assert errs[k_l[0]] <= min(errs) + 2 * bins * U * errs[k_l[0]], '{}: lower search {} against {}'.format(what, errs[k_l[0]], min(errs))


# ---- helpers -----------------------------------------------------------------------------------------------------------------
def _device(engine, a):
    return torch.from_numpy(np.array(a, copy=True)).to(engine.device).contiguous()


def _hist(engine, x, lo, hi, bins, counts=None, extra=0):
    """the table after one call, as int64 numpy [bins + 3 + extra]"""
    lib = _ffi.lib()
    xd = _device(engine, np.ascontiguousarray(x, dtype=F32).reshape(-1))
    r = _device(engine, np.array([lo, hi], dtype=F32))
    c = torch.zeros(bins + 3 + extra, dtype=torch.int64, device=engine.device) if counts is None else counts
    _ffi.check(lib.dfq_act_hist_accumulate(_ffi.ptr(xd), xd.numel(), _ffi.ptr(r), bins, _ffi.ptr(c), _ffi.stream_arg()))
    _ffi.synchronize()
    return c.cpu().numpy()


def _fill(kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind == 'randn':
        return rng.standard_normal(n).astype(F32)
    if kind == 'relu':                                       # half the elements are one value
        return np.maximum(rng.standard_normal(n), 0.0).astype(F32)
    if kind == 'two':                                        # two values, a coin each: the lane's candidate bin keeps changing
        return np.where(rng.random(n) < 0.5, F32(-0.75), F32(1.25)).astype(F32)
    raise KeyError(kind)


def _same(got, want, what):
    assert got.dtype == np.int64 and got.shape == want.shape, what
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, '{}: slot {} holds {} and not {} ({} slots differ)'.format(what, bad[0], got[bad[0]], want[bad[0]], bad.size)


# ---- 1. histogram: every slot, exactly -------------------------------------------------------------------------------------
@pytest.mark.parametrize('bins', BINS)
@pytest.mark.parametrize('kind', ['randn', 'relu', 'two'])
def test_histogram_of_every_size(engine, kind, bins):
    for n in SIZES:
        x = _fill(kind, n, seed=n + bins)
        lo, hi = (-2.5, 3.0) if kind != 'relu' else (F32(x.min()), F32(x.max()))          # randn: both tails outside the range
        got = _hist(engine, x, lo, hi, bins)
        _same(got, ref_hist(x, lo, hi, bins), '{} n={} bins={}'.format(kind, n, bins))
        assert int(got.sum()) == n


@pytest.mark.parametrize('n', [P * GROUPS, P * GROUPS + 1, 2 * P * GROUPS + P + 7])
def test_sizes_at_which_a_piece_takes_another_round(engine, n):
    """one round per piece up to P * GROUPS elements, two from the next element on (the last piece then holds ONE element), three
    beyond 2 * P * GROUPS: the loop over rounds, the loads issued a round ahead, a last piece that ends inside its second round"""
    x = _fill('relu', n, seed=n % 1000)
    lo, hi = 0.25, F32(x.max())                              # the zeros are below
    got = _hist(engine, x, lo, hi, 2048)
    _same(got, ref_hist(x, lo, hi, 2048), 'n={}'.format(n))
    assert int(got.sum()) == n and got[2048] >= n // 3


@pytest.mark.parametrize('bins', BINS)
def test_edges_and_their_neighbours(engine, bins):
    """all bins + 1 float32 edges and their nextafter neighbours on both sides, for a range that is no round number, one that
    starts at zero and one that is a single ulp wide"""
    for lo, hi in ((-1.7, 2.9), (0.0, 6.0), (F32(3.0), np.nextafter(F32(3.0), F32(4.0)))):
        e = ref_edges(lo, hi, bins)
        x = np.concatenate([e, np.nextafter(e, F32(-np.inf)), np.nextafter(e, F32(np.inf))]).astype(F32)
        got = _hist(engine, x, lo, hi, bins)
        _same(got, ref_hist(x, lo, hi, bins), 'edges of ({}, {}) bins={}'.format(lo, hi, bins))
        assert int(got.sum()) == x.size and got[bins + 1] >= 1
        # (the denormal in front of lo = 0 is below only where inv >= 1: with 2 bins t = -1e-45 / 3 rounds to -0.0, and -0.0 < 0 is
        # false -- the rule's answer, and the kernel's)
        assert got[bins] >= (1 if lo != 0.0 or bins >= 16 else 0)


@pytest.mark.parametrize('n', [5, 257, P + 1])
def test_constant_and_extreme_tensors(engine, n):
    bins = 16
    for value, lo, hi, slot in ((1.5, 1.5, 1.5, 0),          # a constant tensor, lo == hi: degenerate, bin 0
                                (-2.0, -2.0, 3.0, 0),        # every element equal to lo
                                (3.0, -2.0, 3.0, bins - 1),  # ... to hi
                                (-2.5, -2.0, 3.0, bins),     # below
                                (3.5, -2.0, 3.0, bins + 1),  # above
                                (0.5, 1.5, 1.5, bins),       # degenerate: below, above
                                (2.5, 1.5, 1.5, bins + 1)):
        x = np.full(n, value, dtype=F32)
        got = _hist(engine, x, lo, hi, bins)
        _same(got, ref_hist(x, lo, hi, bins), 'constant {} over ({}, {})'.format(value, lo, hi))
        assert got[slot] == n


@pytest.mark.parametrize('bins', [2, 2048])
def test_special_values_and_degenerate_ranges(engine, bins):
    rng = np.random.default_rng(11)
    x = (3.0 * rng.standard_normal(2 * P + 1)).astype(F32)
    plants = [F32(np.inf), F32(-np.inf), QNAN, NEG_SNAN, F32(-0.0), F32(0.0), F32(1e-45), F32(-1e-45), F32(1e-39), F32(-3e-39),
              F32(3.4e38), F32(-3.4e38)]
    for i, v in enumerate(plants * 3):                       # in the first vectors, across the piece boundary, in the tail
        x[(0, P - 6, 2 * P - 11)[i // len(plants)] + i % len(plants)] = v
    for lo, hi in ((-4.0, 4.0), (0.0, 5.0), (-0.0, 5.0), (-3e38, 3e38), (2.0, -2.0), (0.0, 1e-40), (-1e-45, 1e-45),
                   (-np.inf, np.inf), (0.0, np.inf), (np.nan, 1.0), (-3.4e38, 0.0)):
        got = _hist(engine, x, lo, hi, bins)
        _same(got, ref_hist(x, lo, hi, bins), 'special values over ({}, {}) bins={}'.format(lo, hi, bins))
        assert int(got.sum()) == x.size and got[bins + 2] == 6
    got = _hist(engine, x, -4.0, 4.0, bins)
    assert got[bins] >= 3 and got[bins + 1] >= 3             # -inf and +inf are below and above


def test_denormal_range_where_bins_over_width_overflows(engine):
    """w = 1e-40: inv = bins / w = +inf, so t = 0 * inf = NaN for x == lo -- bin 0 by the header's rule"""
    bins = 16
    x = np.array([0.0, -0.0, 1e-41, 1e-40, 2e-40, -1e-41, 5e-41, 0.0], dtype=F32)
    got = _hist(engine, x, 0.0, 1e-40, bins)
    _same(got, ref_hist(x, 0.0, 1e-40, bins), 'denormal width')
    assert got[0] == 3 and got[bins] == 1 and got[bins + 1] == 1 and got[bins - 1] == 3


# ---- 2. accumulation, carry, determinism, bounds --------------------------------------------------------------------------
def test_a_second_call_adds_and_the_carry_is_64_bit(engine):
    bins = 16
    a, b = _fill('randn', P + 5, seed=1), _fill('relu', 300, seed=2)
    c = torch.zeros(bins + 3, dtype=torch.int64, device=engine.device)
    first = _hist(engine, a, -2.0, 2.0, bins, counts=c)
    _same(first, ref_hist(a, -2.0, 2.0, bins), 'first call')
    second = _hist(engine, b, -2.0, 2.0, bins, counts=c)
    _same(second, ref_hist(a, -2.0, 2.0, bins) + ref_hist(b, -2.0, 2.0, bins), 'second call')
    assert int(second.sum()) == a.size + b.size
    c.zero_()
    c[3] = 2 ** 32 - 1
    c[bins + 2] = 2 ** 32 - 1
    x = np.array([-1.1] * 5 + [np.nan] * 5, dtype=F32)       # bin (int)((-1.1 + 2) * 4) = 3
    got = _hist(engine, x, -2.0, 2.0, bins, counts=c)
    assert got[3] == 2 ** 32 + 4 and got[bins + 2] == 2 ** 32 + 4 and int(got.sum()) == 2 ** 33 + 8


@pytest.mark.parametrize('kind,bins', [('randn', 2047), ('relu', 4096)])
def test_two_runs_are_bit_equal_and_the_table_ends_where_it_should(engine, kind, bins):
    x = _fill(kind, 3 * P + 7, seed=7)
    c = torch.zeros(bins + 3 + 8, dtype=torch.int64, device=engine.device)
    c[bins + 3:] = -0x0123456789abcdef                       # poison behind the table
    first = _hist(engine, x, -3.0, 3.0, bins, counts=c)
    assert (first[bins + 3:] == -0x0123456789abcdef).all(), 'the call wrote behind bins + 3 slots'
    _same(first[:bins + 3], ref_hist(x, -3.0, 3.0, bins), kind)
    again = _hist(engine, x, -3.0, 3.0, bins)
    assert np.array_equal(again, first[:bins + 3])


# ---- 3. arguments ------------------------------------------------------------------------------------------------------------
def _check_refusals(lib, x, r, c, bits, out, stream):
    """every refusal returns DFQ_ERR_ARG before any HIP call, with a message that names the function"""
    def accumulate(x=x, n=64, r=r, bins=16, c=c):
        return lib.dfq_act_hist_accumulate(x, n, r, bins, c, stream)

    def select(c=c, r=r, n_hist=1, bins=16, bits=bits, method=1, param=0.999, cand=8, out=out):
        return lib.dfq_hist_clip_range(c, r, n_hist, bins, bits, method, param, cand, out, stream)
    for kw in (dict(x=None), dict(r=None), dict(c=None), dict(bins=1), dict(bins=0), dict(bins=-5), dict(bins=4097), dict(n=-1),
               dict(x=x + 4), dict(x=x + 8), dict(x=x + 12), dict(x=x + 2), dict(c=c + 4), dict(r=r + 2), dict(n=1 << 50)):
        assert accumulate(**kw) == DFQ_ERR_ARG, kw
        assert b'dfq_act_hist_accumulate' in lib.dfq_last_error(), kw
    assert b'16-byte' in (accumulate(x=x + 4), lib.dfq_last_error())[1]
    assert accumulate(n=0) == 0 and accumulate(n=0, x=None) == 0                          # a no-op, nothing is launched
    for kw in (dict(c=None), dict(r=None), dict(bits=None), dict(out=None), dict(n_hist=-1), dict(bins=1), dict(bins=4097),
               dict(method=2), dict(method=-1), dict(method=0, param=0.5), dict(method=0, param=1.0000001), dict(method=0, param=0.2),
               dict(method=0, param=float('nan')), dict(cand=0), dict(cand=9), dict(cand=-3), dict(c=c + 4), dict(out=out + 2)):
        assert select(**kw) == DFQ_ERR_ARG, kw
        assert b'dfq_hist_clip_range' in lib.dfq_last_error(), kw
    assert select(n_hist=0) == 0


def test_abi_rejects_bad_arguments(engine):
    lib = _ffi.lib()
    x = torch.zeros(128, dtype=torch.float32, device=engine.device)
    r = torch.tensor([0.0, 1.0]).to(engine.device)
    c = torch.zeros(32, dtype=torch.int64, device=engine.device)
    bits = torch.full((4,), 8, dtype=torch.int32).to(engine.device)
    out = torch.zeros(8, dtype=torch.float32, device=engine.device)
    _check_refusals(lib, x.data_ptr(), r.data_ptr(), c.data_ptr(), bits.data_ptr(), out.data_ptr(), _ffi.stream_arg())
    assert lib.dfq_act_hist_accumulate(_ffi.ptr(x), 64, _ffi.ptr(r), 16, _ffi.ptr(c), _ffi.stream_arg()) == 0
    _ffi.synchronize()
    assert int(c.sum()) == 64 and int(c[0]) == 64


def test_product_library_rejects_bad_arguments_without_a_gpu():
    """the same refusals from the gfx950 build, which never gets as far as a HIP call: the addresses are never dereferenced"""
    if not os.path.exists(_ffi.LIB_PATH):
        subprocess.run(['make', '-C', os.path.join(ROOT, 'dfq_amd', 'csrc'), '-j', '8'], check=True)
    lib = _ffi.bind(ctypes.CDLL(_ffi.LIB_PATH))
    _check_refusals(lib, 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, None)


def test_an_unaligned_view_is_refused_by_the_library_and_copied_by_the_python_layer(engine):
    lib = _ffi.lib()
    bins = 16
    x = _fill('randn', 1000, seed=3)
    buf = torch.zeros(1000 + 4, dtype=torch.float32, device=engine.device)
    buf[1:1001] = _device(engine, x)
    view = buf[1:1001]
    assert view.data_ptr() % 16 == 4
    r = torch.tensor([-2.0, 2.0]).to(engine.device)
    c = torch.zeros(bins + 3, dtype=torch.int64, device=engine.device)
    assert lib.dfq_act_hist_accumulate(_ffi.ptr(view), 1000, _ffi.ptr(r), bins, _ffi.ptr(c), _ffi.stream_arg()) == DFQ_ERR_ARG
    assert b'16-byte' in lib.dfq_last_error()
    got = prims.act_histogram(view, r, bins=bins)
    _same(got.cpu().numpy(), ref_hist(x, -2.0, 2.0, bins), 'prims.act_histogram of an unaligned view')
    # ... a range given as numbers, a table of the caller's, a strided and a float64 input
    table = torch.zeros((2, bins + 3), dtype=torch.int64, device=engine.device)
    assert prims.act_histogram(view, (-2.0, 2.0), bins=bins, counts=table[1]) is not None
    prims.act_histogram(_device(engine, x.astype(np.float64))[::2], (-2.0, 2.0), bins=bins, counts=table[1])
    _same(table[1].cpu().numpy(), ref_hist(x, -2.0, 2.0, bins) + ref_hist(x[::2], -2.0, 2.0, bins), 'a table row')
    assert int(table[0].sum()) == 0
    with pytest.raises(ValueError):
        prims.act_histogram(view, r, bins=1)
    with pytest.raises(ValueError):
        prims.act_histogram(view, r, bins=bins, counts=table[0][:-1])


# ---- 4. selection ------------------------------------------------------------------------------------------------------------
def _select(engine, counts, ranges, bits, **kw):
    c = _device(engine, np.asarray(counts, dtype=np.int64))
    r = _device(engine, np.asarray(ranges, dtype=F32))
    out = prims.hist_clip_range(c, r, num_bits=bits, **kw)
    _ffi.synchronize()
    return out.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _trial(name):
    """the samples of the trial in the issue (seed 0, 2^20 of them), their true range and their histogram over it, 2048 bins"""
    rng = np.random.default_rng(0)
    n = 1 << 20
    if name == 'randn':
        x = rng.standard_normal(n)
    elif name == 'relu':
        x = np.maximum(rng.standard_normal(n), 0.0)
    elif name == 'student':
        x = rng.standard_t(3, n)
    else:
        x = np.clip(3.0 * rng.standard_normal(n), 0.0, 6.0)
    x = x.astype(F32)
    x.setflags(write=False)
    lo, hi = F32(x.min()), F32(x.max())
    counts = ref_hist(x, lo, hi, 2048)
    counts.setflags(write=False)
    return x, lo, hi, counts


def _true_err(x, l, h, bits):
    d = ref_fq(x, l, h, bits).astype(np.float64) - x.astype(np.float64)
    return float(np.sum(d * d))


@pytest.mark.parametrize('bits', [8, 6, 4])
@pytest.mark.parametrize('name', ['randn', 'relu', 'student', 'clip'])
def test_mse_range_on_the_trial_distributions(engine, name, bits):
    x, lo, hi, counts = _trial(name)
    assert counts[2048] == 0 and counts[2049] == 0 and int(counts.sum()) == x.size
    got = _select(engine, counts, [lo, hi], bits, method='mse', candidates=1024)
    assert_mse_choice(got, counts, lo, hi, 2048, bits, 1024, '{} at {} bits'.format(name, bits))
    before, after = _true_err(x, lo, hi, bits), _true_err(x, got[0], got[1], bits)
    print('{} {} bits: ({}, {}) -> ({}, {}), true error {:.6g} -> {:.6g}'.format(name, bits, lo, hi, got[0], got[1], before, after))
    assert after <= before
    if name == 'clip' and bits == 8:
        assert got[0] == lo and got[1] == hi and lo == 0.0 and hi == 6.0


@pytest.mark.parametrize('p', [1.0, 0.9999, 0.99, 0.75, 0.5000001])
def test_percentile_range(engine, p):
    for name in ('randn', 'relu', 'student'):
        _, lo, hi, counts = _trial(name)
        got = _select(engine, counts, [lo, hi], 8, method='percentile', percentile=p)
        want = ref_percentile(counts, lo, hi, 2048, p)
        assert got[0] == want[0] and got[1] == want[1], '{} p={}: {} against {}'.format(name, p, got, want)
        assert got[0] < got[1]
        if p == 1.0:
            assert got[0] == lo and got[1] == hi


def _corner_histograms(bins):
    """(counts, lo, hi, what)"""
    def table(**slots):
        c = np.zeros(bins + 3, dtype=np.int64)
        for k, v in slots.items():
            c[int(k[1:])] = v
        return c
    rng = np.random.default_rng(5)
    spread = np.concatenate([rng.integers(0, 50, bins), [7, 9, 4]]).astype(np.int64)
    return [(table(**{'s{}'.format(bins // 3): 1000}), -1.0, 2.0, 'all mass in one bin'),
            (table(**{'s{}'.format(bins): 500}), -1.0, 2.0, 'all mass below'),
            (table(**{'s{}'.format(bins + 1): 500}), -1.0, 2.0, 'all mass above'),
            (table(**{'s{}'.format(bins): 300, 's{}'.format(bins + 1): 200}), -1.0, 2.0, 'below and above'),
            (table(**{'s{}'.format(bins + 2): 77}), -1.0, 2.0, 'total == 0 (NaN is ignored)'),
            (table(), 0.0, 1.0, 'an empty table'),
            (spread, 1.5, 1.5, 'lo == hi'),
            (spread, 2.0, -2.0, 'lo > hi'),
            (spread, -3e38, 3e38, 'a width that overflows'),
            (spread, -0.37, 4.11, 'spread'),
            (table(s0=2 ** 40, **{'s{}'.format(bins - 1): 3}), 0.0, 6.0, 'counts beyond 2^32')]


@pytest.mark.parametrize('bins,C', [(2, 1), (16, 8), (2047, 300), (4096, 5)])
def test_selection_corner_cases(engine, bins, C):
    for counts, lo, hi, what in _corner_histograms(bins):
        what = '{} bins={}'.format(what, bins)
        for bits in ((8, 4, 2, 16) if bins <= 16 else (8, 3)):
            got = _select(engine, counts, [lo, hi], bits, method='mse', candidates=C)
            assert_mse_choice(got, counts, lo, hi, bins, bits, C, what)
        for p in (1.0, 0.999, 0.51):
            got = _select(engine, counts, [lo, hi], 8, method='percentile', percentile=p)
            want = ref_percentile(counts, lo, hi, bins, p)
            assert got[0] == want[0] and got[1] == want[1], '{} p={}: {} against {}'.format(what, p, got, want)
        if ref_degenerate(lo, hi) or int(ref_nb(counts, bins).sum()) == 0:
            assert got[0] == F32(lo) and got[1] == F32(hi), what + ': the range comes back unchanged'


def test_several_histograms_with_their_own_bit_widths_in_one_launch(engine):
    bins = 256
    rng = np.random.default_rng(8)
    tables, ranges, bits = [], [], [8, 4, 6, 2, 16, 5, 3]
    for i, b in enumerate(bits):
        x = (rng.standard_t(3, 20000) * (i + 1)).astype(F32) if i % 2 else np.maximum(rng.standard_normal(20000), 0).astype(F32)
        lo, hi = F32(x.min()), F32(x.max())
        tables.append(ref_hist(x, lo, hi, bins))
        ranges.append([lo, hi])
    tables[3][:] = 0                                         # one empty histogram among them
    for kw in (dict(method='mse'), dict(method='mse', candidates=17), dict(method='percentile', percentile=0.999)):
        together = _select(engine, np.stack(tables), ranges, bits, **kw)
        assert together.shape == (len(bits), 2) and together.dtype == F32
        for i, b in enumerate(bits):
            alone = _select(engine, tables[i], ranges[i], b, **kw)
            assert alone.shape == (2,)
            assert np.array_equal(alone.view(np.int32), together[i].view(np.int32)), 'histogram {} {}'.format(i, kw)
        assert np.array_equal(together[3], np.array(ranges[3], dtype=F32))
    assert not np.array_equal(_select(engine, tables[2], ranges[2], 8), _select(engine, tables[2], ranges[2], 3))


def test_python_layer_refuses_what_the_library_cannot_see(engine):
    c = torch.zeros(19, dtype=torch.int64, device=engine.device)
    r = torch.tensor([0.0, 1.0]).to(engine.device)
    for bits in (1, 17, 0, [8, 1]):
        with pytest.raises(ValueError):
            prims.hist_clip_range(c if not isinstance(bits, list) else torch.stack([c, c]), r if not isinstance(bits, list) else torch.stack([r, r]),
                                  num_bits=bits)
    with pytest.raises(ValueError):
        prims.hist_clip_range(c, r, method='kl')
    with pytest.raises(_ffi.DfqError, match='dfq_hist_clip_range'):
        prims.hist_clip_range(c, r, method='percentile', percentile=0.5)
    with pytest.raises(_ffi.DfqError, match='dfq_hist_clip_range'):
        prims.hist_clip_range(c, r, candidates=9)
