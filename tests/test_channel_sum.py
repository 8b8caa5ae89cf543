"""dfq_channel_sum_accumulate / dfq_bias_sub_channel_delta (dfq_channel_sum.hip) through the C ABI: the per-channel sums of
an activation [N, C, HW] that the empirical bias correction on distilled data (improve_dfq.py:349-368) is made of.

The truth for channel c is ``math.fsum`` over the float64 values of x[:, c, :], times ``weight``.  The kernel adds the same
terms in float64 in an order of its own, then multiplies by the weight and adds to acc, so the tolerance is the bound of
any-order recursive summation in a format of unit roundoff u = 2^-53 (Higham (4.4), as tests/test_batch_error.py uses it):
|acc[c] - truth| <= n u sum|term| with n = N * HW + 2 -- the two extra operations are the product and the addition to acc.
For unit-scale data that is 1e-14 ... 1e-7 on the shapes below, far under a float32 ulp of the result: a dropped or doubled
element cannot hide in it."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest
import torch

from dfq_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DFQ_ERR_ARG = -1     # include/dfq_hip.h
F32 = np.float32
U = 2.0 ** -53
P = 4096             # kSumPiece of dfq_channel_sum.hip: floats one workgroup reads

# (N, C, HW): a Linear output; more than P rows of one element (the channel index wraps across a piece boundary); C * HW < P
# (a channel several times in one piece); short rows, none 16-byte aligned; rows of exactly a piece; rows over 2 and 3 pieces
# with a first or last element alone in a piece; fewer than 16 elements; N = 1; C = 1; a total that is no multiple of 4
SHAPES = [(3, 5, 1), (2, P + 4, 1), (40, 3, 5), (5, 7, 9), (4, 6, 49), (2, 3, P), (2, 3, P + 1), (3, 2, 2 * P + 1), (1, 1, 7), (1, 4, 3),
          (6, 1, 11), (3, 5, 1023)]
VALUES = ['randn', 'offset', 'huge', 'zeros', 'negzeros', 'denormal']


def _values(kind, shape, seed=0):
    rng = np.random.default_rng(seed)
    n, c, hw = shape
    if kind == 'randn':
        x = rng.standard_normal(shape)
    elif kind == 'offset':                                  # what a float32 accumulation loses
        x = 3e4 + 0.01 * rng.standard_normal(shape)
    elif kind == 'huge':                                    # one element of +-1e30 per channel next to unit values
        x = rng.standard_normal(shape)
        for k in range(c):
            x[rng.integers(n), k, rng.integers(hw)] = 1e30 if k % 2 == 0 else -1e30
    elif kind == 'zeros':
        x = np.zeros(shape)
    elif kind == 'negzeros':
        x = np.full(shape, -0.0)
    else:                                                   # float32 denormals (and a few zeros)
        x = rng.integers(-(1 << 22), 1 << 22, shape).astype(np.float64) * 2.0 ** -149
    return np.ascontiguousarray(x.astype(F32))


def _truth(x, weight, acc0=None):
    """[(exact, bound)] per channel: fsum of the float64 values times weight (+ acc0), n u sum|term|"""
    n, c, hw = x.shape
    out = []
    for k in range(c):
        d = x[:, k, :].astype(np.float64).reshape(-1).tolist()
        a0 = 0.0 if acc0 is None else float(acc0[k])
        exact = math.fsum(d) * weight + a0
        out.append((exact, (n * hw + 2) * U * (math.fsum(abs(v) for v in d) * abs(weight) + abs(a0))))
    return out


def _device(engine, x):
    return torch.from_numpy(np.array(x, copy=True)).to(engine.device).contiguous()


def _scratch(lib, engine, shape):
    """the scratch of a shape, poisoned: an entry the fold reads without the piece kernel having written it shows as NaN"""
    nbytes = int(lib.dfq_channel_sum_scratch_bytes(*shape))
    assert nbytes > 0 and nbytes % 8 == 0
    return torch.full((nbytes // 8,), float('nan'), dtype=torch.float64, device=engine.device)


def _accumulate(engine, xd, shape, weight, acc):
    lib = _ffi.lib()
    scratch = _scratch(lib, engine, shape)
    _ffi.check(lib.dfq_channel_sum_accumulate(_ffi.ptr(xd), shape[0], shape[1], shape[2], float(weight), _ffi.ptr(acc), _ffi.ptr(scratch),
                                              _ffi.stream_arg()))
    _ffi.synchronize()
    if engine.kind == 'gpu':
        torch.cuda.synchronize()


def _sums(engine, x, weight=1.0, acc0=None):
    """acc after one call, as a float64 numpy vector"""
    acc = torch.zeros(x.shape[1], dtype=torch.float64, device=engine.device) if acc0 is None else _device(engine, acc0)
    _accumulate(engine, _device(engine, x), x.shape, weight, acc)
    return acc.cpu().numpy()


def _assert_within(got, want, what):
    for k, (g, (exact, bound)) in enumerate(zip(got.tolist(), want)):
        assert abs(g - exact) <= bound, '{} channel {}: {!r} against {!r}, off by {:.3e} > {:.3e}'.format(what, k, g, exact, abs(g - exact), bound)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


# ---- 1. against an exact sum ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', VALUES)
def test_sums_against_fsum(engine, kind):
    for shape in SHAPES:
        x = _values(kind, shape, seed=len(kind) + shape[2])
        weight = 1.0 / shape[0]
        _assert_within(_sums(engine, x, weight), _truth(x, weight), '{} {}'.format(kind, shape))


def test_float32_accumulation_would_miss_the_bound():
    """why the sums are float64 from the first addition: the eager float32 form of improve_dfq.py:349-365 on a common offset"""
    x = _values('offset', (4, 6, 49), seed=3)
    t = torch.from_numpy(x).view(4, 6, 7, 7)
    eager = t.mean(0).view(6, -1).sum(-1).numpy().astype(np.float64)
    want = _truth(x, 0.25)
    assert max(abs(e - w[0]) for e, w in zip(eager.tolist(), want)) > 100 * max(w[1] for w in want)


# ---- 2. accumulation -----------------------------------------------------------------------------------------------------
def test_two_calls_add_and_a_preset_acc_is_kept(engine):
    c, hw = 7, 9
    a, b = _values('randn', (5, c, hw), seed=1), _values('offset', (3, c, hw), seed=2)
    acc0 = np.linspace(-2.0, 2.0, c)
    acc = _device(engine, acc0)
    _accumulate(engine, _device(engine, a), a.shape, 1.0 / 5, acc)
    first = acc.cpu().numpy()
    _assert_within(first, _truth(a, 1.0 / 5, acc0), 'first call on a preset acc')
    _accumulate(engine, _device(engine, b), b.shape, 1.0 / 3, acc)
    ta, tb = _truth(a, 1.0 / 5, acc0), _truth(b, 1.0 / 3)
    want = [(ea + eb, ba + bb + U * abs(ea + eb)) for (ea, ba), (eb, bb) in zip(ta, tb)]       # (the sum of two exact values, rounded here)
    _assert_within(acc.cpu().numpy(), want, 'two calls')


# ---- 3. determinism ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(40, 3, 5), (4, 6, 49), (2, 3, P + 1), (2, P + 4, 1)])
def test_runs_are_bit_equal_wherever_x_lies(engine, shape):
    x = _values('randn', shape, seed=5)
    first = _sums(engine, x, 0.5)
    assert np.array_equal(_bits(_sums(engine, x, 0.5)), _bits(first)), 'two runs differ'
    keep = _device(engine, x)                                # a second allocation while the first is alive, and a view 16 bytes into one
    other = _device(engine, x)
    assert keep.data_ptr() != other.data_ptr()
    acc = torch.zeros(shape[1], dtype=torch.float64, device=engine.device)
    _accumulate(engine, other, shape, 0.5, acc)
    assert np.array_equal(_bits(acc.cpu().numpy()), _bits(first)), 'another address, other bits'
    padded = torch.zeros(x.size + 4, dtype=torch.float32, device=engine.device)
    padded[4:] = _device(engine, x).reshape(-1)
    view = padded[4:]
    assert view.data_ptr() == padded.data_ptr() + 16
    acc.zero_()
    _accumulate(engine, view, shape, 0.5, acc)
    assert np.array_equal(_bits(acc.cpu().numpy()), _bits(first)), 'a view 16 bytes into a buffer, other bits'


def test_an_x_that_is_only_4_byte_aligned_is_refused(engine):
    """the library's choice (include/dfq_hip.h): x is 16-byte aligned, the Python layer copies a view that is not"""
    lib = _ffi.lib()
    buf = torch.zeros(64 + 4, dtype=torch.float32, device=engine.device)
    acc = torch.zeros(4, dtype=torch.float64, device=engine.device)
    scratch = _scratch(lib, engine, (4, 4, 4))
    for off in (4, 8, 12):
        rc = lib.dfq_channel_sum_accumulate(buf.data_ptr() + off, 4, 4, 4, 1.0, _ffi.ptr(acc), _ffi.ptr(scratch), _ffi.stream_arg())
        assert rc == DFQ_ERR_ARG and b'dfq_channel_sum_accumulate' in lib.dfq_last_error() and b'16-byte' in lib.dfq_last_error()
    assert lib.dfq_channel_sum_accumulate(buf.data_ptr() + 16, 4, 4, 4, 1.0, _ffi.ptr(acc), _ffi.ptr(scratch), _ffi.stream_arg()) == 0
    _ffi.synchronize()


# ---- 4. NaN and inf stay in their channel ----------------------------------------------------------------------------------
QNAN = np.array([0x7fc00000], dtype=np.uint32).view(F32)[0]
SNAN = np.array([0x7fa00000], dtype=np.uint32).view(F32)[0]     # signalling: quiet bit clear, a payload bit set
PLANTS = [('qnan', QNAN), ('snan', SNAN), ('+inf', F32(np.inf)), ('-inf', F32(-np.inf))]


def _positions(shape):
    """flat positions: the first and the last element, the first and last element of a row in the middle, every component of
    the 16-byte vectors on both sides of the piece boundaries (or of two vectors in the middle of a small tensor)"""
    n, c, hw = shape
    total = n * c * hw
    pos = {0, total - 1, (c + 1) * hw % total, ((c + 2) * hw - 1) % total}
    edges = [b for b in (P, 2 * P) if b + 4 <= total] or [(total // 8) * 4]
    for b in edges:
        pos.update(range(max(b - 4, 0), min(b + 4, total)))
    return sorted(pos)


@pytest.mark.parametrize('shape', [(2, 3, P + 1), (40, 3, 5), (5, 7, 9), (2, P + 4, 1), (3, 5, 1023)])
def test_nan_and_inf_stay_in_their_channel(engine, shape):
    n, c, hw = shape
    x = _values('randn', shape, seed=9)
    xd = _device(engine, x)
    flat = xd.view(-1)
    clean = _sums(engine, x)
    acc = torch.zeros(c, dtype=torch.float64, device=engine.device)
    for pos in _positions(shape):
        ch = (pos // hw) % c
        others = [k for k in range(c) if k != ch]
        for name, value in PLANTS:
            kept = flat[pos].clone()
            flat[pos:pos + 1] = torch.from_numpy(np.array([value], dtype=F32)).to(engine.device)
            acc.zero_()
            _accumulate(engine, xd, shape, 1.0, acc)
            flat[pos] = kept
            got = acc.cpu().numpy()
            what = '{} at {} of {}'.format(name, pos, shape)
            if 'nan' in name:
                assert math.isnan(got[ch]), what
            else:
                assert got[ch] == float(value), what
            assert np.array_equal(_bits(got[others]), _bits(clean[others])), what + ': another channel changed'
    assert np.array_equal(_bits(_sums(engine, xd.cpu().numpy())), _bits(clean))          # every plant was taken back
    # +inf and -inf in one channel: NaN there, and only there
    if n * hw >= 2:
        y = x.copy()
        y[0, c // 2, 0], y[n - 1, c // 2, hw - 1] = np.inf, -np.inf
        got = _sums(engine, y)
        others = [k for k in range(c) if k != c // 2]
        assert math.isnan(got[c // 2])
        assert np.array_equal(_bits(got[others]), _bits(clean[others]))


# ---- 5. the bias update ----------------------------------------------------------------------------------------------------
def test_bias_sub_channel_delta_rounds_once_and_subtracts_once(engine):
    lib = _ffi.lib()
    rng = np.random.default_rng(4)
    c = 300                                                  # more than one workgroup
    b = rng.standard_normal(c).astype(F32)
    aq, ar = rng.standard_normal(c) * 50.0, rng.standard_normal(c) * 50.0
    aq[3], ar[5] = np.nan, np.nan                            # a NaN touches its own element only
    aq[7], ar[9] = np.inf, np.inf
    aq[11], ar[11] = 1e300, -1e300                           # a shift that overflows float32
    aq[13], ar[13] = 1e-40, 0.0                              # ... and one that is a float32 denormal
    aq[15], ar[15] = 1.0 + 2.0 ** -30, 1.0                   # a difference float32 operands would lose
    b[17] = 2.0 ** 24
    for scale in (1.0 / 3, 1.0 / (3 * 49), 1.0):
        with np.errstate(all='ignore'):
            want = b - ((aq - ar) * scale).astype(F32)
        assert want.dtype == F32
        bias, dq, dr = _device(engine, b), _device(engine, aq), _device(engine, ar)
        _ffi.check(lib.dfq_bias_sub_channel_delta(_ffi.ptr(bias), _ffi.ptr(dq), _ffi.ptr(dr), c, scale, _ffi.stream_arg()))
        _ffi.synchronize()
        got = bias.cpu().numpy()
        assert np.array_equal(got.view(np.int32)[~np.isnan(want)], want.view(np.int32)[~np.isnan(want)])
        assert np.array_equal(np.isnan(got), np.isnan(want))
        assert np.flatnonzero(np.isnan(got)).tolist() == [3, 5] and got[7] == -np.inf and got[9] == np.inf and got[11] == -np.inf


# ---- 6. argument errors ----------------------------------------------------------------------------------------------------
def _check_refusals(lib, x, acc, scratch, bias, stream):
    """every refusal returns DFQ_ERR_ARG before any HIP call, with a message that names the function"""
    def accumulate(x=x, n=2, c=3, hw=5, acc=acc, scratch=scratch):
        return lib.dfq_channel_sum_accumulate(x, n, c, hw, 0.5, acc, scratch, stream)

    def delta(bias=bias, aq=acc, ar=acc, c=3):
        return lib.dfq_bias_sub_channel_delta(bias, aq, ar, c, 1.0, stream)
    for kw in (dict(x=None), dict(acc=None), dict(scratch=None), dict(n=0), dict(n=-1), dict(c=0), dict(c=-2), dict(hw=0), dict(hw=-7),
               dict(x=x + 4), dict(x=x + 8), dict(x=x + 2), dict(acc=acc + 4), dict(acc=acc + 1), dict(scratch=scratch + 4),
               dict(hw=1 << 31), dict(c=1 << 31), dict(n=1 << 40, c=1 << 20, hw=1 << 10), dict(n=1 << 30, c=1 << 10, hw=1 << 10)):
        assert accumulate(**kw) == DFQ_ERR_ARG, kw
        assert b'dfq_channel_sum_accumulate' in lib.dfq_last_error(), kw
    for kw in (dict(bias=None), dict(aq=None), dict(ar=None), dict(c=0), dict(c=-1), dict(bias=bias + 2), dict(aq=acc + 4), dict(ar=acc + 4)):
        assert delta(**kw) == DFQ_ERR_ARG, kw
        assert b'dfq_bias_sub_channel_delta' in lib.dfq_last_error(), kw
    for shape in ((0, 3, 5), (2, 0, 5), (2, 3, 0), (-1, 3, 5), (2, 3, 1 << 31), (1 << 30, 1 << 10, 1 << 10)):
        assert lib.dfq_channel_sum_scratch_bytes(*shape) == 0, shape
        assert b'dfq_channel_sum_scratch_bytes' in lib.dfq_last_error(), shape
    assert lib.dfq_channel_sum_scratch_bytes(2, 3, 5) == 8 * (6 + 2)
    assert lib.dfq_channel_sum_scratch_bytes(2, 3, P + 1) == 8 * (6 + 2 * 7)


def test_abi_rejects_bad_arguments(engine):
    lib = _ffi.lib()
    x = torch.zeros(64, dtype=torch.float32, device=engine.device)
    acc = torch.zeros(8, dtype=torch.float64, device=engine.device)
    scratch = torch.zeros(64, dtype=torch.float64, device=engine.device)
    bias = torch.zeros(8, dtype=torch.float32, device=engine.device)
    _check_refusals(lib, x.data_ptr(), acc.data_ptr(), scratch.data_ptr(), bias.data_ptr(), _ffi.stream_arg())
    assert lib.dfq_channel_sum_accumulate(_ffi.ptr(x), 2, 3, 5, 0.5, _ffi.ptr(acc), _ffi.ptr(scratch), _ffi.stream_arg()) == 0
    _ffi.synchronize()


def test_product_library_rejects_bad_arguments_without_a_gpu():
    """the same refusals from the gfx950 build, which never gets as far as a HIP call: the addresses are never dereferenced"""
    if not os.path.exists(_ffi.LIB_PATH):
        subprocess.run(['make', '-C', os.path.join(ROOT, 'dfq_amd', 'csrc'), '-j', '8'], check=True)
    lib = _ffi.bind(ctypes.CDLL(_ffi.LIB_PATH))
    _check_refusals(lib, 0x10000, 0x20000, 0x30000, 0x40000, None)
