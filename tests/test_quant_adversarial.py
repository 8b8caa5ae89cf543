"""Adversarial inputs for the per-tensor range reductions and the fake-quant round trip of dfq_quant.hip, through the C ABI.

test_engine_parity.py feeds these kernels Gaussian data at a few sizes.  Here the data is built against the code:
  A  a unique maximum (+5) and a unique minimum (-7) planted at chosen positions of uniform(-1, 1) data, so that over a test the
     extremum sits in every float4 component, every unroll slot of every load tier of thread_minmax_range, every element of the
     scalar tail, the first and last element of a chunk, and in vectors owned by threads 0, 63, 64 and 255;
  B  tensors longer than one pass of the grid-stride loops (minmax_kernel, fake_quant_kernel, quant_error_kernel,
     quant_error_rows_kernel);
  C  special values: NaN of any payload (quiet and signalling) is skipped by every reduction, nothing but NaN gives (NaN, NaN),
     infinities are ordinary values, denormals are kept -- the same on the 16-byte path and on the scalar path;
  D  quantiser parameters at their edges (1 .. 30 bits, degenerate / inverted / huge / tiny ranges, round-half-even ties);
  E  the symmetric recipe with one bit (qmax = 0) is refused.

References: numpy on the host for min / max (selections: compared with ==, the sign of a zero is free); for the quantiser
both oracle.uniform_quantize and `ref_torch`, the reference's own lines restated with torch CPU in-place operations, bit-exact.
The integer code is unspecified where the float code is NaN (the conversion of NaN to an integer is undefined in C and in
numpy alike): at a NaN input, and where x + (-min) is infinite under an infinite float32 scale (inf / inf: one bit over
+-3e38 in section D, at the three inputs +inf, -inf and 3.4e38 -- at most three positions of a tensor, which _check_quant
asserts).  Those positions, and no others, are left out of the comparison of integer codes; the values are compared there."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import dfq_oracle as orc
from dfq_amd import _ffi, arena, dfq, synthetic
from dfq_amd.utils import layer_transform as lt
from dfq_amd.utils import quantize as q
from dfq_amd.utils import relation as rel

from common import F32, TARG, assert_bitexact

DFQ_ERR_ARG = -1                     # include/dfq_hip.h
BLOCK, CHUNK = 256, 4096             # kBlock, kChunk of dfq_quant.hip
LONG = 4096 * 3 + 4 * 700 + 3        # three full chunks, a chunk of 700 vectors (single-vector tier only), a 3-element tail
HI, LO = F32(5.0), F32(-7.0)         # the planted extrema


# ---- helpers ---------------------------------------------------------------------------------------------------------------

def _dev(engine, a):
    """host float32 array -> device tensor, bit for bit (NaN payloads included)"""
    a = np.ascontiguousarray(a, dtype=F32)
    return torch.from_numpy(a.view(np.int32).copy()).to(engine.device).view(torch.float32)


def _host(t):
    """device float32 / int32 tensor -> host array, bit for bit"""
    t = t.detach().contiguous()
    if t.dtype == torch.float32:
        return t.view(torch.int32).cpu().numpy().view(F32)
    return t.cpu().numpy()


def _bits(*words):
    return np.array(words, dtype=np.uint32).view(F32)


def _same_values(got, want, what):
    """selections: equal as values (-0 == +0), NaN where NaN is wanted"""
    got, want = np.asarray(got, dtype=F32).reshape(-1), np.asarray(want, dtype=F32).reshape(-1)
    ok = (got == want) | (np.isnan(got) & np.isnan(want))
    assert ok.all(), '{}: got {}, want {}'.format(what, got.tolist(), want.tolist())


def ref_torch(x, num_bits, min_value, max_value, symmetric=False):
    """utils/quantize.py:49-74 of the reference, line for line, on a torch CPU copy of x.  min_value / max_value: Python floats
    (the float64 recipe) or 0-dim float32 tensors (the recipe of the min_value=None path).  Returns (values, codes as float32)."""
    if symmetric:
        qmin = -2. ** (num_bits - 1)
        qmax = 2 ** (num_bits - 1) - 1
        max_value = abs(max_value)
        min_value = abs(min_value)
        if max_value < min_value:
            max_value = min_value
        scale = max_value / qmax
        min_value = 0.
    else:
        qmin = 0.
        qmax = 2. ** num_bits - 1.
        scale = (max_value - min_value) / (qmax - qmin)
    scale = max(scale, 1e-8)
    output = torch.from_numpy(np.array(x, dtype=F32).view(np.int32)).view(torch.float32)
    output.add_(-min_value).div_(scale)
    output.clamp_(qmin, qmax).round_()
    codes = output.clone()
    output.mul_(scale).add_(min_value)
    return _host(output), _host(codes)


def _orc_float32_recipe(x, num_bits, mn, mx, symmetric):
    """oracle.uniform_quantize's min_value=None branch for a GIVEN float32 pair (the oracle takes its pair from the data)"""
    mn, mx = F32(mn), F32(mx)
    with np.errstate(all='ignore'):
        if symmetric:
            qmin, qmax = -2.0 ** (num_bits - 1), 2 ** (num_bits - 1) - 1
            mx, mn = F32(abs(mx)), F32(abs(mn))
            if mx < mn:
                mx = mn
            scale, used = F32(mx / F32(qmax)), F32(0.0)
        else:
            qmin, qmax = 0.0, 2.0 ** num_bits - 1.0
            scale, used = F32(F32(mx - mn) / F32(qmax - qmin)), mn
        if scale < F32(1e-8):
            scale = F32(1e-8)
        return orc.fake_quant_f32(x, qmin, qmax, F32(-used), scale, used, True)


def _check_quant(what, x, y, codes, num_bits, mn, mx, symmetric=False, float32_recipe=False):
    """engine values y (and int32 codes, unless None) of host input x against both references"""
    x = np.asarray(x, dtype=F32).reshape(-1)
    with np.errstate(all='ignore'):
        if float32_recipe:
            y_o, c_o = _orc_float32_recipe(x, num_bits, mn, mx, symmetric)
            y_t, c_t = ref_torch(x, num_bits, torch.tensor(float(mn), dtype=torch.float32),
                                 torch.tensor(float(mx), dtype=torch.float32), symmetric)
        else:
            y_o, c_o = orc.uniform_quantize(x, num_bits, float(mn), float(mx), symmetric, return_codes=True)
            y_t, c_t = ref_torch(x, num_bits, float(mn), float(mx), symmetric)
    ok = ~np.isnan(c_t)                     # the float code is NaN: a NaN input, or inf / inf under an infinite scale
    assert np.isnan(c_t[np.isnan(x)]).all() and (~ok).sum() <= np.isnan(x).sum() + 3 and np.array_equal(np.isnan(c_o), ~ok), what
    assert_bitexact(y_o, y_t, what + ': oracle against the reference restated')
    assert np.array_equal(c_o[ok], c_t[ok]), what + ': codes, oracle against the reference restated'
    assert_bitexact(np.asarray(y).reshape(-1), y_t, what + ': values')
    if codes is not None:
        assert np.array_equal(np.asarray(codes).reshape(-1)[ok], c_t[ok].astype(np.int64)), what + ': integer codes'


def _fake_quant(xd, num_bits, symmetric, mode, mn=0.0, mx=0.0, pair=None, codes=False):
    """dfq_fake_quant out of place: (values, int32 codes or None) on the host"""
    y = torch.empty(xd.shape, dtype=torch.float32, device=xd.device)
    c = torch.empty(xd.shape, dtype=torch.int32, device=xd.device) if codes else None
    _ffi.check(_ffi.lib().dfq_fake_quant(_ffi.ptr(xd), _ffi.ptr(y), xd.numel(), num_bits, int(symmetric), mode, float(mn),
                                         float(mx), _ffi.ptr(pair), _ffi.ptr(c), _ffi.stream_arg()))
    _ffi.synchronize()
    return _host(y), (None if c is None else _host(c))


def _minmax(xd):
    return _host(q.tensor_minmax(xd))


class _Plan:
    """dfq_quant_plan over [(device tensor, bits, symmetric, int32 code tensor or None)]"""

    def __init__(self, segs):
        self.lib, self.n, self.keep = _ffi.lib(), len(segs), segs
        arr = (_ffi.DfqSegment * len(segs))(*[_ffi.DfqSegment(t.data_ptr(), t.numel(), b, s, None if c is None else c.data_ptr())
                                              for (t, b, s, c) in segs])
        self.plan = ctypes.c_void_p()
        _ffi.check(self.lib.dfq_quant_plan_create(arr, len(segs), ctypes.byref(self.plan)))

    def _pairs(self, dev):
        _ffi.synchronize()
        addr = self.lib.dfq_quant_plan_minmax(self.plan)
        return _host(dfq._RawDeviceBuffer(addr, 2 * self.n, dev).tensor()).reshape(self.n, 2).copy()

    def measure(self, dev):
        _ffi.check(self.lib.dfq_quant_plan_measure(self.plan, _ffi.stream_arg()))
        return self._pairs(dev)

    def run(self, dev):
        _ffi.check(self.lib.dfq_quant_plan_run(self.plan, _ffi.stream_arg()))
        return self._pairs(dev)

    def close(self):
        self.lib.dfq_quant_plan_destroy(self.plan)


# ---- where thread_minmax_range reads what ----------------------------------------------------------------------------------

def _vector_map(n4):
    """(tier, slot) of every float4 of a 16-byte aligned range of n4 vectors: tier 8 / 4 / 1 = the 8-deep, 4-deep and
    single-vector loops of thread_minmax_range, slot = the unroll index.  Vector v belongs to thread v % 256."""
    tier, slot = np.zeros(n4, dtype=np.int64), np.zeros(n4, dtype=np.int64)
    for t in range(BLOCK):
        i = t
        for depth in (8, 4, 1):
            while i + (depth - 1) * BLOCK < n4:
                for u in range(depth):
                    tier[i + u * BLOCK], slot[i + u * BLOCK] = depth, u
                i += depth * BLOCK
    assert (tier > 0).all()
    return tier, slot


def _class_positions(length, all_components):
    """Offsets into a 16-byte aligned range of `length` floats that one workgroup reduces: its first and last element, every
    element of the scalar tail, and for every (tier, slot) that occurs a vector owned by each of the threads 0, 63, 64, 255
    -- in all four components, or (all_components False) in one, rotating."""
    n4 = length // 4
    out = [0, length - 1] + list(range(4 * n4, length))
    if n4:
        tier, slot = _vector_map(n4)
        k = 0
        for depth in (8, 4, 1):
            for u in range(depth):
                for t in (0, 63, 64, 255):
                    v = np.flatnonzero((tier == depth) & (slot == u) & (np.arange(n4) % BLOCK == t))
                    if v.size:
                        comps = range(4) if all_components else [k % 4]
                        out += [4 * int(v[-1]) + c for c in comps]
                        k += 1
    seen, uniq = set(), []
    for p in out:
        if p not in seen:
            seen.add(p)
            uniq.append(p)
    return uniq


def test_position_classes_cover_the_tiers():
    """the planted positions of section A reach what they claim to (pure host arithmetic)"""
    tier, slot = _vector_map(13315 // 4)
    assert sorted(set(zip(tier.tolist(), slot.tolist()))) == [(1, 0)] + [(4, u) for u in range(4)] + [(8, u) for u in range(8)]
    pos = _class_positions(13315, True)
    assert len(pos) <= 257 and {13312, 13313, 13314, 0} <= set(pos)
    got = {(int(tier[p // 4]), int(slot[p // 4]), (p // 4) % BLOCK, p % 4) for p in pos if p < 13312}
    assert {(8, u, t, k) for u in range(8) for t in (0, 63, 64, 255) for k in range(4)} <= got
    assert {(4, u, t, k) for u in range(4) for t in (0, 63, 64, 255) for k in range(4)} <= got
    assert {(1, 0, t, k) for t in (0, 63, 64, 255) for k in range(4)} <= got
    t1023, _ = _vector_map(1023)                       # the second chunk of 8191 floats: thread 255 alone misses the 4-deep trip
    assert set(np.flatnonzero(t1023 == 1).tolist()) == {255, 511, 767}


# ---- A. planted extrema ----------------------------------------------------------------------------------------------------

PLAN_LENGTHS = [1, 2, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8193, LONG]


@functools.lru_cache(maxsize=None)
def _plan_layout():
    """[(start, length, max position, min position)] of the segments carved out of one buffer, and the buffer (host).  Aligned
    segments (start a multiple of 4) walk over the position classes of each of their chunks, two per segment; segments that
    start at element 1 or 3 of a 16-byte group take the scalar loop.  The gaps hold +-100: a read past a segment's end shows."""
    rng = np.random.default_rng(41)
    segs, at = [], 0
    for n in PLAN_LENGTHS:
        pos = []
        for b in range(0, n, CHUNK):
            pos += [b + p for p in _class_positions(min(CHUNK, n - b), False)]
        pos = list(dict.fromkeys(pos))
        if len(pos) % 2:
            pos.append(pos[0])
        pairs = [(pos[i], pos[i + 1]) for i in range(0, len(pos), 2)] if n > 1 else [(0, 0)]
        odd = list(dict.fromkeys(p for p in (0, n - 1, n // 2, CHUNK - 1, CHUNK, n - 2) if 0 <= p < n))
        for k, (pmax, pmin) in enumerate(pairs):
            segs.append((0, n, pmax, pmin))
        for k, off in enumerate((1, 3, 1)):
            segs.append((off, n, odd[k % len(odd)], odd[(k + 1) % len(odd)]))
    rng.shuffle(segs)
    placed = []
    for (off, n, pmax, pmin) in segs:
        at = (at + 3) // 4 * 4 + 4 * int(rng.integers(1, 4)) + off
        placed.append((at, n, pmax, pmin))
        at += n
    buf = np.where(np.arange(at + 8) % 2 == 0, F32(100.0), F32(-100.0)).astype(F32)
    for (start, n, pmax, pmin) in placed:
        buf[start:start + n] = rng.uniform(-1.0, 1.0, n).astype(F32)
        buf[start + pmax] = HI
        if pmin != pmax:
            buf[start + pmin] = LO
    return placed, buf


def test_plan_layout_is_what_the_issue_asks():
    placed, buf = _plan_layout()
    assert 150 <= len(placed) <= 260
    assert {s % 4 for (s, _, _, _) in placed} == {0, 1, 3}
    aligned = [(n, p) for (s, n, pmax, pmin) in placed if s % 4 == 0 for p in (pmax, pmin)]
    assert {p % 4 for (n, p) in aligned if n >= 8} == {0, 1, 2, 3}
    assert {(p % CHUNK // 4) // BLOCK for (n, p) in aligned if n == 4096} == {0, 1, 2, 3}         # the four unroll slots
    assert {(p % CHUNK // 4) % BLOCK for (n, p) in aligned if n == 4096} >= {0, 63, 64, 255}
    assert {p for (n, p) in aligned if n == LONG} >= {0, LONG - 1, LONG - 2, LONG - 3, CHUNK - 1, CHUNK, 3 * CHUNK}


@pytest.mark.parametrize('entry', ['measure', 'run'])
def test_plan_planted_extrema(engine, entry):
    placed, buf = _plan_layout()
    xd = _dev(engine, buf)
    assert xd.data_ptr() % 16 == 0
    bits = [(8, 0), (4, 1), (16, 0), (2, 1), (1, 0), (30, 0), (8, 1), (3, 0)]
    segs = []
    for j, (start, n, _, _) in enumerate(placed):
        b, s = bits[j % len(bits)]
        c = torch.full((n,), -77, dtype=torch.int32, device=engine.device) if entry == 'run' else None
        segs.append((xd[start:start + n], b, s, c))
    plan = _Plan(segs)
    pairs = plan.measure(engine.device) if entry == 'measure' else plan.run(engine.device)
    plan.close()
    after = _host(xd)
    for j, (start, n, pmax, pmin) in enumerate(placed):
        x = buf[start:start + n]
        what = 'segment {} (start {} = {} mod 4, {} elements, max at {}, min at {})'.format(j, start, start % 4, n, pmax, pmin)
        _same_values(pairs[j], [x.min(), x.max()], what)
        if entry == 'run':
            _check_quant(what, x, after[start:start + n], _host(segs[j][3]), segs[j][1], pairs[j][0], pairs[j][1], segs[j][2])
    mask = np.ones(buf.size, dtype=bool)
    for (start, n, _, _) in placed:
        mask[start:start + n] = False
    assert np.array_equal(after[mask], buf[mask]), 'something between the segments was written'


def test_tensor_minmax_planted_extrema(engine):
    rng = np.random.default_rng(42)
    base = rng.uniform(-1.0, 1.0, LONG + 1).astype(F32)
    last = 3 * CHUNK                                     # the chunk of 700 vectors: every thread in the single-vector tier
    pos = [last + 4 * t + t % 4 for t in range(BLOCK)] + [LONG - 3, LONG - 2, LONG - 1, 0, CHUNK - 1, CHUNK]
    for off in (0, 1):
        xd = _dev(engine, base)[off:off + LONG]
        assert xd.data_ptr() % 16 == 4 * off
        x = base[off:off + LONG].copy()
        for i, pmax in enumerate(pos):
            pmin = pos[(i + 97) % len(pos)]
            x[pmax], x[pmin] = HI, LO
            xd[pmax], xd[pmin] = float(HI), float(LO)
            got = _minmax(xd)
            assert got[0] == x.min() == LO and got[1] == x.max() == HI, 'offset {}: max at {}, min at {}: {}'.format(off, pmax, pmin, got)
            x[pmax], x[pmin] = base[off + pmax], base[off + pmin]
            xd[pmax], xd[pmin] = float(x[pmax]), float(x[pmin])
        got = _minmax(xd)
        assert got[0] == x.min() and got[1] == x.max()


SAMPLES, SAMPLE_LEN = 1025, 13315     # from 1025 samples on a workgroup sees a whole sample; 13315 = 4 * (2048 + 1024 + 256) + 3


@functools.lru_cache(maxsize=None)
def _sample_case():
    """x [1025, 13315] with the extrema of sample s planted by class: every fourth sample starts on a 16-byte boundary (13315
    = 3 mod 4) and those walk over all classes of the 8-deep, 4-deep and single-vector tiers and the tail; the others take the
    scalar loop.  Returns x and the references of the two QuantMeasure calls (running range narrower, then wider)."""
    rng = np.random.default_rng(43)
    x = rng.uniform(-1.0, 1.0, (SAMPLES, SAMPLE_LEN)).astype(F32)
    pos = _class_positions(SAMPLE_LEN, True)
    s = np.arange(SAMPLES)
    pmax = np.array([pos[(k // 4 + (k % 4) * 50) % len(pos)] for k in s])
    pmin = np.array([pos[(k // 4 + (k % 4) * 50 + len(pos) // 2) % len(pos)] for k in s])
    assert (pmax != pmin).all()
    assert set(pmax[::4].tolist()) == set(pos) and set(pmin[::4].tolist()) == set(pos)
    x[s, pmax] = HI
    x[s, pmin] = LO
    x.setflags(write=False)
    mean = orc.sample_minmax_mean(x)
    assert mean == (LO, HI)
    refs = {}
    for name, (r0, r1) in (('narrower', (0.0, 0.0)), ('wider', (-10.0, 10.0))):
        lo, hi = min(F32(r0), mean[0]), max(F32(r1), mean[1])
        y_o = orc.uniform_quantize(x.reshape(-1), 8, float(lo), float(hi))
        y_t, _ = ref_torch(x.reshape(-1), 8, float(lo), float(hi))
        assert_bitexact(y_o, y_t, 'the two references')
        refs[name] = (lo, hi, y_t)
    return x, mean, refs


def test_sample_minmax_planted_extrema(engine):
    x, mean, _ = _sample_case()
    xd = _dev(engine, x)
    assert xd.data_ptr() % 16 == 0
    assert_bitexact(_host(q.sample_minmax_mean(xd, SAMPLES)), np.array(mean, dtype=F32), 'means')
    for r0, r1 in ((-10.0, 10.0), (-1.0, 1.0)):           # already wider than the data, narrower
        running = _dev(engine, np.array([r0, r1], dtype=F32))
        got = q.sample_minmax_mean(xd, SAMPLES, running=running)
        assert_bitexact(_host(got), np.array(mean, dtype=F32), 'means')
        assert_bitexact(_host(running), np.array([min(F32(r0), mean[0]), max(F32(r1), mean[1])], dtype=F32), 'running2')


@pytest.mark.parametrize('fused', [False, True])
def test_quant_measure_planted_extrema(engine, monkeypatch, fused):
    x, mean, refs = _sample_case()
    monkeypatch.setattr(q, '_QM_FUSED', fused)
    xd = _dev(engine, x)
    m = q.QuantMeasure(update_stat=True).to(engine.device).eval()
    for name, start in (('narrower', (0.0, 0.0)), ('wider', (-10.0, 10.0))):
        m.running_min.fill_(start[0])
        m.running_max.fill_(start[1])
        y = m(xd)
        lo, hi, want = refs[name]
        assert_bitexact(_host(m.running_min), np.array([lo], dtype=F32), name + ': running_min')
        assert_bitexact(_host(m.running_max), np.array([hi], dtype=F32), name + ': running_max')
        assert_bitexact(_host(y).reshape(-1), want, name + ': quantised output')
    m.check_fused_status()


@pytest.mark.parametrize('shape', [(1, 1), (1, 5), (7, 4097), (2049, 3), (1024, 8200)])
def test_sample_minmax_shape_edges(engine, shape):
    """(1024, 8200): two spans per sample, the second of 8 elements; (2049, 3): more samples than workgroups of the split"""
    rng = np.random.default_rng(shape[1])
    x = rng.standard_normal(shape).astype(F32)
    running = _dev(engine, np.array([-0.5, 0.5], dtype=F32))
    got = q.sample_minmax_mean(_dev(engine, x), shape[0], running=running)
    want = orc.sample_minmax_mean(x)
    assert_bitexact(_host(got), np.array(want, dtype=F32), 'means')
    assert_bitexact(_host(running), np.array([min(F32(-0.5), want[0]), max(F32(0.5), want[1])], dtype=F32), 'running2')


# ---- B. more than one pass of the grid-stride loops ------------------------------------------------------------------------

BIG = 2048 * 4096 + 3 * 4096 + 5


@functools.lru_cache(maxsize=None)
def _big_case():
    rng = np.random.default_rng(44)
    x = rng.uniform(-1.0, 1.0, BIG).astype(F32)
    x[2048 * 4096 + 1234] = LO                           # the first chunk of workgroup 0's second pass
    x[BIG - 2] = HI
    x.setflags(write=False)
    y_o, c_o = orc.uniform_quantize(x, 8, float(LO), float(HI), return_codes=True)
    y_t, c_t = ref_torch(x, 8, float(LO), float(HI))
    assert_bitexact(y_o, y_t, 'the two references')
    assert np.array_equal(c_o, c_t)
    return x, y_t, c_t.astype(np.int32)


def test_grid_stride_minmax_and_fake_quant(engine):
    x, want, want_codes = _big_case()
    xd = _dev(engine, x)
    got = _minmax(xd)
    assert got[0] == x.min() == LO and got[1] == x.max() == HI, got
    y, _ = _fake_quant(xd, 8, 0, 0, LO, HI)                         # aligned, no codes: the 16-byte path
    assert_bitexact(y, want, '16-byte path')
    y, c = _fake_quant(xd, 8, 0, 0, LO, HI, codes=True)             # with codes: the scalar path
    assert_bitexact(y, want, 'scalar path')
    assert np.array_equal(c, want_codes)


def test_grid_stride_quant_error(engine):
    x, want, _ = _big_case()
    xd = _dev(engine, x)
    eps = (want - x).astype(F32)
    assert_bitexact(_host(dfq._quantize_error(xd, 8, None)), eps, 'elementwise')
    got = float(_host(dfq._quantize_error(xd, 8, 'mean')))
    ref = float(eps.astype(np.float64).mean())
    print('mean: got {!r}, float64 reference {!r}'.format(got, ref))
    assert abs(got - ref) <= 1e-6 * max(1.0, abs(ref))


@pytest.mark.parametrize('shape,reduction', [((8200, 1, 1, 1), 'channel'), ((96, 96, 1, 1), 'spatial'), ((5, 1, 63), 'spatial'),
                                             ((5, 1, 64), 'spatial'), ((5, 1, 65), 'channel'), ((3, 1, 4097), 'spatial'),
                                             ((3, 1, 4097), 'channel')])
def test_quant_error_row_shapes(engine, shape, reduction):
    """more rows than the kernel has waves (8200, 9216 > 4096), rows of one element, rows around the 64 lanes of a wave"""
    rng = np.random.default_rng(sum(shape))
    w = rng.standard_normal(shape).astype(F32)
    for signed in (False, True):
        got = float(_host(dfq._quantize_error(_dev(engine, w).reshape(shape), 8, reduction, signed)))
        want = float(orc.quantize_error(w, 8, reduction, signed))
        print('{} {} signed {}: got {!r}, oracle {!r}'.format(shape, reduction, signed, got, want))
        assert abs(got - want) <= 1e-6 * max(1.0, abs(want))


# ---- C. special values -----------------------------------------------------------------------------------------------------

QNAN, NEG_QNAN, SNAN, NEG_SNAN = 0x7FC00000, 0xFFC00000, 0x7FA00000, 0xFFA00000
INF, NEG_INF, FLT_MAX, NEG_FLT_MAX = 0x7F800000, 0xFF800000, 0x7F7FFFFF, 0xFF7FFFFF
# name -> (base data, [(distance from the planted position, word)])
SPECIALS = {
    'quiet NaN': ('gauss', [(0, QNAN)]), 'negative quiet NaN': ('gauss', [(0, NEG_QNAN)]),
    'signalling NaN': ('gauss', [(0, SNAN)]), 'negative signalling NaN': ('gauss', [(0, NEG_SNAN)]),
    '+inf': ('gauss', [(0, INF)]), '-inf': ('gauss', [(0, NEG_INF)]), 'both infinities': ('gauss', [(0, INF), (-1, NEG_INF)]),
    '+FLT_MAX': ('gauss', [(0, FLT_MAX)]), '-FLT_MAX': ('gauss', [(0, NEG_FLT_MAX)]),
    '-0.0': ('positive', [(0, 0x80000000)]), 'denormals': ('zero', [(0, 0x00000001), (-1, 0x80000001)]),
}
N_SPECIAL = 9000
# first chunk's vector body, second chunk's vector body, the last element, element 0 of the view that starts at element 1
SPECIAL_POSITIONS = [4 * 300 + 2, CHUNK + 4 * 77 + 3, N_SPECIAL - 1, 1]


def _special_tensor(name, position):
    base, plants = SPECIALS[name]
    rng = np.random.default_rng(45)
    g = rng.standard_normal(N_SPECIAL).astype(F32)
    x = {'gauss': g, 'positive': np.abs(g) + F32(0.25), 'zero': np.zeros(N_SPECIAL, dtype=F32)}[base].astype(F32)
    w = x.view(np.uint32)
    for d, word in plants:
        w[(position + d) % N_SPECIAL if position + d >= 1 else position + 1] = word
    return x


def _nan_skipping(x):
    """(min, max) with NaN skipped; (NaN, NaN) for nothing but NaN"""
    x = np.asarray(x, dtype=F32).reshape(-1)
    keep = x[~np.isnan(x)]
    return (F32(np.nan), F32(np.nan)) if keep.size == 0 else (keep.min(), keep.max())


def _sample_means(x2):
    with np.errstate(all='ignore'):
        pairs = [_nan_skipping(r) for r in x2]
        return orc._mean_f32([p[0] for p in pairs]), orc._mean_f32([p[1] for p in pairs])


def test_nan_skipping_reference_sees_the_planted_values():
    x = _special_tensor('denormals', SPECIAL_POSITIONS[0])
    assert _nan_skipping(x) == (F32(-1e-45), F32(1e-45)) and F32(1e-45) > 0
    x = _special_tensor('signalling NaN', SPECIAL_POSITIONS[1])
    assert x.view(np.uint32)[SPECIAL_POSITIONS[1]] == SNAN and np.isnan(x).sum() == 1
    assert _host(torch.from_numpy(x.view(np.int32)).view(torch.float32)).view(np.uint32)[SPECIAL_POSITIONS[1]] == SNAN


@pytest.mark.parametrize('name', list(SPECIALS))
def test_special_values_in_every_reduction(engine, name):
    rng = np.random.default_rng(46)
    plain = [_dev(engine, rng.standard_normal(n).astype(F32)) for n in (700, 5000)]
    for position in SPECIAL_POSITIONS:
        x = _special_tensor(name, position)
        xd = _dev(engine, x)
        assert xd.data_ptr() % 16 == 0
        what = '{} at {}'.format(name, position)
        # the whole tensor, on the 16-byte path and on the scalar path
        for off in (0, 1):
            _same_values(_minmax(xd[off:]), _nan_skipping(x[off:]), '{}: dfq_tensor_minmax from element {}'.format(what, off))
        # three samples of 3000 (all aligned), then three of 2999 from element 1 (mixed)
        for off, n in ((0, 3000), (1, 2999)):
            x2 = x[off:off + 3 * n].reshape(3, n)
            running = _dev(engine, np.array([-0.5, 0.5], dtype=F32))
            with np.errstate(all='ignore'):
                want = _sample_means(x2)
                fold = [want[0] if want[0] < F32(-0.5) else F32(-0.5), want[1] if want[1] > F32(0.5) else F32(0.5)]
            got = q.sample_minmax_mean(xd[off:off + 3 * n], 3, running=running)
            _same_values(_host(got), want, '{}: dfq_sample_minmax_mean from element {}'.format(what, off))
            _same_values(_host(running), fold, '{}: running2 from element {}'.format(what, off))
        # a mixed segment table
        segs = [plain[0], xd, plain[1][3:], xd[1:], xd[3:N_SPECIAL - 2]]
        hosts = [_host(t) for t in segs]
        plan = _Plan([(t, 8, 0, None) for t in segs])
        pairs = plan.measure(engine.device)
        plan.close()
        for j, h in enumerate(hosts):
            _same_values(pairs[j], _nan_skipping(h), '{}: segment {}'.format(what, j))
    if name == 'denormals':
        assert tuple(_minmax(xd)) == (F32(-1e-45), F32(1e-45))


def test_nothing_but_nan(engine):
    words = np.array([QNAN, NEG_QNAN, SNAN, NEG_SNAN, 0x7FFFFFFF, 0x7F800001], dtype=np.uint32)
    rng = np.random.default_rng(47)
    nan = words[rng.integers(0, len(words), N_SPECIAL)].view(F32)
    nd = _dev(engine, nan)
    for off in (0, 1):
        assert np.isnan(_minmax(nd[off:])).all()
        assert np.isnan(_minmax(nd[off:off + 3])).all()
    # one sample of nothing but NaN among ordinary ones: both means are NaN, running2 stays (Python min(r, nan))
    for off, n in ((0, 3000), (1, 2999)):
        x = rng.standard_normal(3 * n + 1).astype(F32)
        x[off + n:off + 2 * n] = nan[:n]
        running = _dev(engine, np.array([-0.5, 0.5], dtype=F32))
        got = _host(q.sample_minmax_mean(_dev(engine, x)[off:off + 3 * n], 3, running=running))
        assert np.isnan(got).all(), got
        assert_bitexact(_host(running), np.array([-0.5, 0.5], dtype=F32), 'running2')
        # ... and QuantMeasure.forward quantises with the range it had
        m = q.QuantMeasure(update_stat=True).to(engine.device).eval()
        m.running_min.fill_(-0.5)
        m.running_max.fill_(0.5)
        x3 = x[off:off + 3 * n].reshape(3, n)
        y = m(_dev(engine, x)[off:off + 3 * n].reshape(3, n))
        assert float(m.running_min) == -0.5 and float(m.running_max) == 0.5
        _check_quant('QuantMeasure', x3, _host(y), None, 8, -0.5, 0.5)
    # a segment of nothing but NaN between ordinary ones
    plain = _dev(engine, rng.standard_normal(5000).astype(F32))
    segs = [plain[:700], nd, plain[701:], nd[1:], nd[2:3]]
    plan = _Plan([(t, 8, 0, None) for t in segs])
    pairs = plan.measure(engine.device)
    plan.close()
    for j, t in enumerate(segs):
        _same_values(pairs[j], _nan_skipping(_host(t)), 'segment {}'.format(j))
    assert np.isnan(pairs[[1, 3, 4]]).all()


@pytest.mark.parametrize('name', list(SPECIALS))
def test_special_values_through_the_quantiser(engine, name):
    """modes 0, 1 and 2 with the range of the finite values: a NaN input gives a NaN output, an infinity clamps"""
    for position in SPECIAL_POSITIONS:
        x = _special_tensor(name, position)
        xd = _dev(engine, x)
        finite = x[np.isfinite(x)]
        mn, mx = finite.min(), finite.max()
        pair = _dev(engine, np.array([mn, mx], dtype=F32))
        for mode in (0, 1, 2):
            what = '{} at {}, mode {}'.format(name, position, mode)
            y, _ = _fake_quant(xd, 8, 0, mode, mn, mx, pair if mode else None)                          # 16-byte path
            _check_quant(what, x, y, None, 8, mn, mx, False, mode == 2)
            y, c = _fake_quant(xd[1:], 8, 0, mode, mn, mx, pair if mode else None, codes=True)          # scalar path
            _check_quant(what + ', from element 1', x[1:], y, c, 8, mn, mx, False, mode == 2)
            assert np.isnan(y[np.isnan(x[1:])]).all()
        y, c = _fake_quant(xd, 8, 1, 1, mn, mx, pair, codes=True)
        _check_quant('{} at {}, symmetric'.format(name, position), x, y, c, 8, mn, mx, True)


# ---- D. quantiser parameter edges ------------------------------------------------------------------------------------------

BIT_CASES = [(b, s) for b in (1, 2, 3, 8, 16, 24, 25, 30) for s in (0, 1) if not (b == 1 and s)]


def _edge_tensor():
    rng = np.random.default_rng(48)
    x = (rng.standard_normal(5003) * 3).astype(F32)
    x[[5, 1030, 4099, 5002]] = [np.inf, -np.inf, 3.4e38, 1e-45]
    x[[77, 2050]] = [np.nan, -0.0]
    return x


@pytest.mark.parametrize('rng_pair', [(-2.5, 3.0), (0.0, 0.0), (1.0, 1.0), (-3e38, 3e38), (3.0, -2.5), (-1e-30, 1e-30), (0.0, 255.0)])
def test_quantiser_parameter_edges(engine, rng_pair):
    mn, mx = float(F32(rng_pair[0])), float(F32(rng_pair[1]))       # mode 1 reads the pair as float32: the same numbers for mode 0
    x = _edge_tensor()
    if rng_pair == (0.0, 255.0):                         # every code on a round-half-even tie
        x[100:356] = np.arange(256, dtype=F32) + F32(0.5)
    xd = _dev(engine, x)
    pair = _dev(engine, np.array([mn, mx], dtype=F32))
    for bits, sym in BIT_CASES:
        for mode in (0, 1):
            what = 'range {} bits {} symmetric {} mode {}'.format(rng_pair, bits, sym, mode)
            y, c = _fake_quant(xd, bits, sym, mode, mn, mx, pair if mode else None, codes=True)
            _check_quant(what, x, y, c, bits, mn, mx, sym)
            y, _ = _fake_quant(xd, bits, sym, mode, mn, mx, pair if mode else None)
            _check_quant(what + ' (16-byte path)', x, y, None, bits, mn, mx, sym)


def test_ties_are_ties():
    y, c = ref_torch(np.arange(256, dtype=F32) + F32(0.5), 8, 0.0, 255.0)
    assert np.array_equal(c, np.minimum((np.arange(256) + 1) // 2 * 2, 255).astype(F32))


@pytest.mark.parametrize('factor', [1.0, 3e38, 1e-40, 0.0])
@pytest.mark.parametrize('bits,sym', [(1, False), (8, False), (8, True), (16, False), (30, False), (30, True)])
def test_quantize_without_a_range(engine, factor, bits, sym):
    """quantize(x, bits): the float32 recipe of quantize.py:24-35 on the range of the data (one row: num_chunks = shape[0])"""
    rng = np.random.default_rng(49)
    with np.errstate(all='ignore'):
        x = (rng.uniform(-1.0, 1.0, (4, 1000)).astype(F32) * F32(factor)).astype(F32)
        if factor == 3e38:
            assert np.isfinite(x).all() and np.isinf(x.max() - x.min())          # the float32 span overflows
        y_o = orc.uniform_quantize(x, bits, symmetric=sym)
        flat = torch.from_numpy(x.copy()).view(1, -1)
        y_t, _ = ref_torch(x.reshape(-1), bits, flat.min(-1)[0].mean(-1), flat.max(-1)[0].mean(-1), sym)
    assert_bitexact(y_o.reshape(-1), y_t, 'oracle against the reference restated')
    y = q.quantize(_dev(engine, x).reshape(4, 1000), bits, symmetric=sym)
    assert_bitexact(_host(y).reshape(-1), y_t, 'factor {} bits {} symmetric {}'.format(factor, bits, sym))


# ---- E. one bit, symmetric: qmax = 0 ---------------------------------------------------------------------------------------

def test_one_bit_symmetric_is_refused(engine):
    """the reference divides by qmax = 2 ** 0 - 1 = 0 there (quantize.py:56, ZeroDivisionError); so does the oracle"""
    with pytest.raises(ZeroDivisionError):
        orc.quant_params(1, -1.0, 1.0, True)
    with pytest.raises(ZeroDivisionError):
        ref_torch(np.zeros(4, dtype=F32), 1, -1.0, 1.0, True)
    lib = _ffi.lib()
    x = _dev(engine, np.linspace(-1, 1, 64).astype(F32))
    y = torch.empty_like(x)
    pair = _dev(engine, np.array([-1.0, 1.0], dtype=F32))
    for mode in (0, 1, 2):
        assert lib.dfq_fake_quant(_ffi.ptr(x), _ffi.ptr(y), 64, 1, 1, mode, -1.0, 1.0, _ffi.ptr(pair), None, _ffi.stream_arg()) == DFQ_ERR_ARG
        assert b'dfq_fake_quant' in lib.dfq_last_error() and b'num_bits=1' in lib.dfq_last_error()
        assert lib.dfq_fake_quant(_ffi.ptr(x), _ffi.ptr(y), 64, 1, 0, mode, -1.0, 1.0, _ffi.ptr(pair), None, _ffi.stream_arg()) == 0
    plan = ctypes.c_void_p()
    seg = (_ffi.DfqSegment * 2)(_ffi.DfqSegment(x.data_ptr(), 64, 8, 1, None), _ffi.DfqSegment(y.data_ptr(), 64, 1, 1, None))
    assert lib.dfq_quant_plan_create(seg, 2, ctypes.byref(plan)) == DFQ_ERR_ARG
    assert b'dfq_quant_plan_create: segment 1' in lib.dfq_last_error()
    seg[1].symmetric = 0
    assert lib.dfq_quant_plan_create(seg, 2, ctypes.byref(plan)) == 0
    lib.dfq_quant_plan_destroy(plan)
    scratch = torch.zeros(int(lib.dfq_quant_error_scratch_bytes(64, 8)) // 4 + 4, dtype=torch.int32, device=engine.device)
    for reduction in range(5):
        assert lib.dfq_quant_error(_ffi.ptr(x), 64, 8, 1, 1, reduction, _ffi.ptr(y), _ffi.ptr(scratch), _ffi.stream_arg()) == DFQ_ERR_ARG
        assert b'dfq_quant_error' in lib.dfq_last_error()
        assert lib.dfq_quant_error(_ffi.ptr(x), 64, 8, 1, 0, reduction, _ffi.ptr(y), _ffi.ptr(scratch), _ffi.stream_arg()) == 0
    codes = torch.zeros(256, dtype=torch.int32, device=engine.device)
    ranges = torch.zeros(16, dtype=torch.float32, device=engine.device)
    bases = (ctypes.c_void_p * 1)(x.data_ptr())
    for sym, want in ((1, DFQ_ERR_ARG), (0, 0)):
        t = (_ffi.DfqBatchQuantTensor * 1)(_ffi.DfqBatchQuantTensor(x.data_ptr(), 4, 16, 1, sym, 0, 0, 0, 0))
        plan = ctypes.c_void_p()
        assert lib.dfq_batch_quant_plan_create(t, 1, bases, 1, codes.data_ptr(), 4, 256, ranges.data_ptr(), 16, ctypes.byref(plan)) == want
        if want == 0:
            lib.dfq_batch_quant_plan_destroy(plan)
        else:
            assert b'dfq_batch_quant_plan_create' in lib.dfq_last_error()
    _ffi.synchronize()
    # the Python layer raises where the reference raises
    with pytest.raises(_ffi.DfqError):
        q.quantize(x, 1, -1.0, 1.0, symmetric=True)
    with pytest.raises(_ffi.DfqError):
        q.quantize(x.reshape(4, 16), 1, symmetric=True)
    with pytest.raises(_ffi.DfqError):
        dfq._quantize_error(x, 1, 'sum', True)
    model, graph, bottoms = synthetic.build('tiny_mobile', seed=0)
    model.to(engine.device)
    lt.merge_batchnorm(model, graph, bottoms, TARG)
    with pytest.raises(_ffi.DfqError):
        lt.quantize_targ_layer(graph, 1, 16, TARG, signed=True)
    rels = rel.create_relation(graph, bottoms, TARG, delete_single=False)
    batch = arena.NetworkBatch([(graph, bottoms, rels)], TARG)
    with pytest.raises((ValueError, _ffi.DfqError)):
        batch.quant_plan(bit_weight=1, signed=True)
    batch.quant_plan(bit_weight=1, signed=False).close()
    batch.release()
