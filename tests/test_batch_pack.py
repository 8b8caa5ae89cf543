"""NetworkBatch.pack_plan / unpack_plan / save_packed / load_packed and dfq_batch_pack_plan_* / dfq_batch_unpack_plan_*: the
integer codes of a batch packed densely, every tensor of every network at its own width, and the way back.

Every comparison is exact.  The reference is the definition in include/dfq_hip.h restated in numpy, in this file: the unsigned
code u = (q - qmin) & (2^b - 1), element i at bits [i b, (i + 1) b) of its tensor's stream, least significant bit first, as a
shift and an OR over 64-bit integers (``_pack_ref``; ``_unpack_ref`` is the same arithmetic read backwards, and the test of the
reference itself checks the two against a bit-by-bit loop); the extent of a tensor is ceil(n b / 32) words rounded up to 4, the
offsets are their running sum; the weight of a code is ``q * scale + min`` in two float32 roundings with the ``_qparams`` recipe
tests/test_batch_mixed.py states (a division by qmax = 0, symmetric at one bit, is IEEE's here as it is in the library)."""
import ctypes
import os
import subprocess
import tempfile
from collections import OrderedDict

import numpy as np
import pytest
import torch

from dfq_amd import _ffi, arena, synthetic
from dfq_amd.utils import layer_transform as lt
from dfq_amd.utils import relation as rel

from common import TARG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DFQ_ERR_ARG = -1     # include/dfq_hip.h
F32 = np.float32
FILL = 0xA5A5A5A5
FILL_I32 = int(np.array([FILL], dtype=np.uint32).view(np.int32)[0])
WIDTHS = (2, 3, 4, 6, 8)
NAMES = ['tiny_mobile', 'tiny_res', 'tiny_cat']
SEEDS = [0, 1, 2]
PAIRS = [(False, False), (True, True), (True, False)]        # (per_channel, signed), as tests/test_batch_mixed.py


# ---- the definition in numpy ---------------------------------------------------------------------------------------------
def _extent(n, b):
    words = -(-n * b // 32)
    return -(-words // 4) * 4


def _qmin(b, signed):
    return -(1 << (b - 1)) if signed else 0


def _masked(q, b, signed):
    """the code the packed words hold for a stored code q: q itself inside [qmin, qmax]"""
    return ((np.asarray(q, dtype=np.int64) - _qmin(b, signed)) & ((1 << b) - 1)) + _qmin(b, signed)


def _pack_ref(q, b, signed):
    """uint32 [extent]: the words of one tensor's stream"""
    u = ((np.asarray(q, dtype=np.int64).reshape(-1) - _qmin(b, signed)) & ((1 << b) - 1)).astype(np.uint64)
    words = np.zeros(_extent(u.size, b), dtype=np.uint64)
    bit = np.arange(u.size, dtype=np.int64) * b
    w, s = bit >> 5, (bit & 31).astype(np.uint64)
    v = u << s                                          # at most 31 + 16 bits
    np.bitwise_or.at(words, w, v & np.uint64(0xffffffff))
    spill = (v >> np.uint64(32)) != 0
    np.bitwise_or.at(words, w[spill] + 1, v[spill] >> np.uint64(32))
    return words.astype(np.uint32)


def _unpack_ref(words, n, b, signed):
    """int64 [n]: the codes of a tensor's words"""
    ext = np.concatenate([words.astype(np.uint64), np.zeros(1, dtype=np.uint64)])
    bit = np.arange(n, dtype=np.int64) * b
    w, s = bit >> 5, (bit & 31).astype(np.uint64)
    pair = ext[w] | (ext[w + 1] << np.uint64(32))
    return ((pair >> s) & np.uint64((1 << b) - 1)).astype(np.int64) + _qmin(b, signed)


def _qparams(mn, mx, bits, signed):
    """utils/quantize.py:49-66 with float64 scalars: (scale, min) as float32"""
    mn, mx = np.float64(mn), np.float64(mx)
    with np.errstate(all='ignore'):
        if signed:
            qmax = np.float64((1 << (bits - 1)) - 1)
            mx, mn = abs(mx), abs(mn)
            if mx < mn:
                mx = mn
            scale, mn = mx / qmax, np.float64(0.0)
        else:
            scale = (mx - mn) / (np.float64(1 << bits) - 1.0)
        if 1e-8 > scale:
            scale = np.float64(1e-8)
        return F32(scale), F32(mn)


def _weights_ref(q, ranges, b, signed):
    """float32 [units, n]: (float)q * scale + min, two roundings, per unit of q [units, n] with ranges [units, 2]"""
    prm = [_qparams(mn, mx, b, signed) for mn, mx in ranges]
    scale = np.array([p[0] for p in prm], dtype=F32).reshape(-1, 1)
    minv = np.array([p[1] for p in prm], dtype=F32).reshape(-1, 1)
    with np.errstate(all='ignore'):
        y = q.astype(F32) * scale
        y = y + minv
    assert y.dtype == F32
    return y


def _bits_of(a):
    return np.ascontiguousarray(a).view(np.int32)


def _same_floats(got, want):
    return ((_bits_of(got) == _bits_of(want)) | (np.isnan(got) & np.isnan(want))).all()


def test_the_reference_against_a_bit_loop():
    gen = np.random.default_rng(5)
    for b in (1, 3, 5, 7, 8, 11, 16):
        for signed in (False, True):
            n = 77
            q = gen.integers(_qmin(b, signed), _qmin(b, signed) + (1 << b), size=n)
            words = _pack_ref(q, b, signed)
            want = np.zeros(_extent(n, b), dtype=np.uint32)
            for i in range(n):
                u = int(q[i]) - _qmin(b, signed)
                for j in range(b):
                    k = i * b + j
                    want[k // 32] |= np.uint32(((u >> j) & 1) << (k % 32))
            assert np.array_equal(words, want), (b, signed)
            assert np.array_equal(_unpack_ref(words, n, b, signed), q), (b, signed)
            assert 0 <= 32 * words.size - n * b < 128


# ---- the C ABI on hand-made tensors ----------------------------------------------------------------------------------------
def _chunk():
    return int(_ffi.lib().dfq_batch_pack_chunk_elements())


def _rows_of(numel, mode):
    """rows of a tensor of `numel` elements: 0 per tensor (one row), 1 a few rows, 2 rows of one element"""
    if mode == 0:
        return 1
    if mode == 2:
        return numel
    return max(d for d in range(1, 17) if numel % d == 0)


class _Abi:
    """One batch of hand-made tensors: ``tensors`` [(numel, num_bits or 0, width_index, signed)], ``codes[n][t]`` int64, the
    width block (numpy [n_nets, width_stride]) for the tensors with num_bits 0.  Tensor t is per tensor, per row with a few rows
    or per row with rows of one element as t % 3 says; every second tensor's codes start off a 16-byte boundary."""

    def __init__(self, engine, tensors, codes, code_bytes, wblock=None, seed=0):
        self.engine, self.tensors, self.codes, self.code_bytes = engine, tensors, codes, code_bytes
        self.n_nets, self.T = len(codes), len(tensors)
        self.wblock = None if wblock is None else np.ascontiguousarray(wblock, dtype=np.int32)
        dev = engine.device
        self.c_offs, at = [], 0
        for i, (numel, _, _, _) in enumerate(tensors):
            off = at + (i % 2)
            self.c_offs.append(off)
            at = -(-(off + numel) // 16) * 16
        self.code_stride = at
        raw = np.full((self.n_nets, at), 77, dtype=np.int32 if code_bytes == 4 else np.uint8)
        for n in range(self.n_nets):
            for (numel, _, _, _), off, q in zip(tensors, self.c_offs, codes[n]):
                raw[n, off:off + numel] = q if code_bytes == 4 else (np.asarray(q) & 0xff)
        self.code_dev = torch.from_numpy(raw).to(dev)
        self.wdev = None if self.wblock is None else torch.from_numpy(self.wblock).to(dev)
        # weights, ranges: for unpack
        gen = np.random.default_rng(1000 + seed)
        self.rows = [_rows_of(numel, i % 3) for i, (numel, _, _, _) in enumerate(tensors)]
        self.w_offs, at = [], 4
        for numel, _, _, _ in tensors:
            self.w_offs.append(at)
            at += -(-numel // 4) * 4 + 4
        self.w_stride = at
        self.r_offs, at = [], 1
        for r in self.rows:
            self.r_offs.append(at)
            at += 2 * r + 1
        self.r_stride = at
        rng = np.full((self.n_nets, at), 9.0, dtype=F32)
        for n in range(self.n_nets):
            for r, off in zip(self.rows, self.r_offs):
                lo = -np.abs(gen.standard_normal(r)).astype(F32)
                hi = (np.abs(gen.standard_normal(r)) + 0.1).astype(F32)
                if r > 2:
                    lo[1], hi[1] = F32(0.375), F32(0.375)           # a constant unit: the max(scale, 1e-8) branch
                    lo[2] = F32(0.0)                                  # one-sided
                rng[n, off:off + 2 * r] = np.stack([lo, hi], axis=1).reshape(-1)
        self.ranges = rng
        self.range_dev = torch.from_numpy(rng).to(dev)
        self.store = torch.full((self.n_nets, self.w_stride), 7.5e5, dtype=torch.float32, device=dev)
        self.bases = (ctypes.c_void_p * self.n_nets)(*[self.store.data_ptr() + 4 * n * self.w_stride for n in range(self.n_nets)])

    def width(self, n, t):
        _, b, wi, _ = self.tensors[t]
        return b if b else int(self.wblock[n, wi])

    def sizes(self):
        return [sum(_extent(self.tensors[t][0], self.width(n, t)) for t in range(self.T)) for n in range(self.n_nets)]

    def pack(self, word_stride=None, runs=1):
        lib, dev = _ffi.lib(), self.engine.device
        if word_stride is None:
            word_stride = max(self.sizes()) + 7
        self.word_stride = word_stride
        self.packed = torch.full((self.n_nets, word_stride), FILL_I32, dtype=torch.int32, device=dev)
        self.offsets = torch.full((self.n_nets, self.T + 1), -7, dtype=torch.int64, device=dev)
        self.status = torch.full((self.n_nets,), -7, dtype=torch.int32, device=dev)
        P = _ffi.DfqBatchPackTensor
        tab = (P * self.T)(*[P(off, numel, b, wi, int(s), 0) for (numel, b, wi, s), off in zip(self.tensors, self.c_offs)])
        plan = ctypes.c_void_p()
        _ffi.check(lib.dfq_batch_pack_plan_create(tab, self.T, self.bases, self.n_nets, self.code_dev.data_ptr(), self.code_bytes,
                                                  self.code_stride, None if self.wdev is None else self.wdev.data_ptr(),
                                                  0 if self.wblock is None else self.wblock.shape[1], self.packed.data_ptr(), word_stride,
                                                  self.offsets.data_ptr(), self.status.data_ptr(), ctypes.byref(plan)))
        try:
            assert lib.dfq_batch_pack_plan_launches(plan) == 2
            first = None
            for _ in range(runs):
                _ffi.check(lib.dfq_batch_pack_plan_run(plan, _ffi.stream_arg()))
                _ffi.synchronize()
                now = [t.cpu().numpy().copy() for t in (self.packed, self.offsets, self.status)]
                if first is not None:
                    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, now)), 'two runs differ'
                first = now
        finally:
            lib.dfq_batch_pack_plan_destroy(plan)
        return first[0].view(np.uint32), first[1], first[2]

    def check_packed(self, words, offsets, status, skipped=()):
        """every network not in `skipped` against the restatement: words, padding, the fill behind the end, offsets, status"""
        for n in range(self.n_nets):
            if n in skipped:
                continue
            assert status[n] == 0, 'network {}: status {}'.format(n, status[n])
            want_off, parts = [0], []
            for t, (numel, _, _, s) in enumerate(self.tensors):
                b = self.width(n, t)
                parts.append(_pack_ref(self.codes[n][t], b, s))
                want_off.append(want_off[-1] + parts[-1].size)
            assert offsets[n].tolist() == want_off, 'network {}: offsets'.format(n)
            want = np.concatenate(parts)
            got = words[n, :want.size]
            if not np.array_equal(got, want):
                t = int(np.searchsorted(want_off, int(np.nonzero(got != want)[0][0]), side='right')) - 1
                raise AssertionError('network {}: words differ first in tensor {} {} at {} bits'.format(n, t, self.tensors[t], self.width(n, t)))
            assert (words[n, want.size:] == FILL).all(), 'network {}: a word at or behind offset[T] was written'.format(n)
            assert 0 <= 32 * want_off[-1] - sum(self.tensors[t][0] * self.width(n, t) for t in range(self.T)) < 159 * self.T

    def unpack(self, code_bytes=None, weights=True, skipped=(), expect_status=None):
        """unpack what pack left (self.packed, self.offsets): codes into a fresh block of `code_bytes` (None: no codes), weights
        into the store; both checked against the restatement for every network not in `skipped`, untouched for the others"""
        lib, dev = _ffi.lib(), self.engine.device
        out_offs, at = [], 0
        for i, (numel, _, _, _) in enumerate(self.tensors):
            off = at + ((i + 1) % 2)
            out_offs.append(off)
            at = -(-(off + numel) // 16) * 16
        codes = None
        if code_bytes:
            codes = torch.full((self.n_nets, at), 77, dtype=torch.int32 if code_bytes == 4 else torch.uint8, device=dev)
        self.store.fill_(7.5e5)
        status = torch.full((self.n_nets,), -7, dtype=torch.int32, device=dev)
        P = _ffi.DfqBatchUnpackTensor
        tab = (P * self.T)(*[P(self.store.data_ptr() + 4 * w_off if weights else None, r, numel // r, c_off, numel, r_off, b, wi, int(s),
                               int(r > 1 or i % 3 == 2))
                             for i, ((numel, b, wi, s), w_off, c_off, r_off, r) in
                             enumerate(zip(self.tensors, self.w_offs, out_offs, self.r_offs, self.rows))])
        plan = ctypes.c_void_p()
        _ffi.check(lib.dfq_batch_unpack_plan_create(tab, self.T, self.bases, self.n_nets, self.packed.data_ptr(), self.word_stride,
                                                    self.offsets.data_ptr(), None if self.wdev is None else self.wdev.data_ptr(),
                                                    0 if self.wblock is None else self.wblock.shape[1],
                                                    self.range_dev.data_ptr(), self.r_stride, None if codes is None else codes.data_ptr(),
                                                    code_bytes or 0, at, status.data_ptr(), ctypes.byref(plan)))
        try:
            assert lib.dfq_batch_unpack_plan_launches(plan) == 1
            _ffi.check(lib.dfq_batch_unpack_plan_run(plan, _ffi.stream_arg()))
            _ffi.synchronize()
        finally:
            lib.dfq_batch_unpack_plan_destroy(plan)
        st = status.cpu().numpy()
        assert st.tolist() == (expect_status if expect_status is not None else [0] * self.n_nets)
        store = self.store.cpu().numpy()
        got_codes = None if codes is None else codes.cpu().numpy()
        wmask = np.ones(self.w_stride, dtype=bool)
        cmask = np.ones(at, dtype=bool)
        for (numel, _, _, _), w_off, c_off in zip(self.tensors, self.w_offs, out_offs):
            wmask[w_off:w_off + numel] = False
            cmask[c_off:c_off + numel] = False
        assert (store[:, wmask] == 7.5e5).all(), 'a float outside the tensors was written'
        assert got_codes is None or (got_codes[:, cmask] == 77).all(), 'a code outside the tensors was written'
        for n in range(self.n_nets):
            if n in skipped:
                assert (store[n] == 7.5e5).all() and (got_codes is None or (got_codes[n] == 77).all()), 'a skipped network was written'
                continue
            for t, (numel, _, _, s) in enumerate(self.tensors):
                b = self.width(n, t)
                what = 'network {} tensor {} {} at {} bits'.format(n, t, self.tensors[t], b)
                q = _masked(self.codes[n][t], b, s)
                if got_codes is not None:
                    raw = got_codes[n, out_offs[t]:out_offs[t] + numel]
                    got = raw.astype(np.int64) if code_bytes == 4 else (raw.view(np.int8) if s else raw).astype(np.int64)
                    assert np.array_equal(got, q), what + ': codes'
                y = store[n, self.w_offs[t]:self.w_offs[t] + numel]
                if not weights:
                    assert (y == 7.5e5).all(), what + ': weights=off wrote a weight'
                    continue
                r = self.rows[t]
                want = _weights_ref(q.reshape(r, numel // r), self.ranges[n, self.r_offs[t]:self.r_offs[t] + 2 * r].reshape(r, 2), b, s)
                assert _same_floats(y.reshape(r, -1), want), what + ': weights'
        return st


def _full_range(gen, numel, b, signed):
    """random codes over the whole range with both extremes among them"""
    lo = _qmin(b, signed)
    q = gen.integers(lo, lo + (1 << b), size=numel)
    q[0] = lo + (1 << b) - 1
    q[-1] = lo if numel > 1 else q[-1]
    if numel > 2:
        q[numel // 2] = lo
    return q.astype(np.int64)


def _numels():
    C = _chunk()
    assert C % 32 == 0
    return [1, 31, 32, 33, 63, 64, 65, C - 1, C, C + 1, 2 * C + 17]


# ---- 1. + 4. every size and width, packed and back ---------------------------------------------------------------------------
@pytest.mark.parametrize('code_bytes', [4, 1])
def test_every_size_and_width_through_the_abi(engine, code_bytes):
    gen = np.random.default_rng(10 + code_bytes)
    tensors = [(numel, b, 0, signed) for signed in (False, True) for b in range(1, (8 if code_bytes == 1 else 16) + 1) for numel in _numels()]
    assert code_bytes == 1 or len(tensors) > 256, 'the offsets are scanned 256 tensors at a time: more than one round'
    codes = [[_full_range(gen, numel, b, s) for (numel, b, _, s) in tensors]]
    abi = _Abi(engine, tensors, codes, code_bytes)
    words, offsets, status = abi.pack()
    abi.check_packed(words, offsets, status)
    abi.unpack(code_bytes=code_bytes)


def test_sizes_around_a_workgroup_s_span(engine):
    """a workgroup takes several chunks of one tensor in a row: sizes around every multiple of the chunk up to six"""
    C = _chunk()
    gen = np.random.default_rng(21)
    numels = [k * C + d for k in (2, 3, 4, 5, 6) for d in (-1, 0, 1)] + [6 * C + 33]
    for code_bytes, widths in ((4, (3, 8, 11, 16)), (1, (1, 5, 8))):
        tensors = [(numel, b, 0, (i + b) % 2 == 1) for b in widths for i, numel in enumerate(numels)]
        codes = [[_full_range(gen, numel, b, s) for (numel, b, _, s) in tensors]]
        abi = _Abi(engine, tensors, codes, code_bytes)
        words, offsets, status = abi.pack()
        abi.check_packed(words, offsets, status)
        abi.unpack(code_bytes=code_bytes)


# ---- 2. widths from the device ---------------------------------------------------------------------------------------------------
def _device_width_case(engine, code_bytes, seed=0, n_nets=2, wblock=None, out_of_range=False):
    C = _chunk()
    numels = [100, C + 5, 33, 777, 2 * C]
    index = [3, 0, 4, 1, 2]
    if wblock is None:
        wblock = np.array([[5, 8, 3, 1, 7, -1, 99, 0], [3, 2, 6, 8, 4, -1, 99, 0], [7, 7, 1, 5, 2, 0, 0, 0]][:n_nets], dtype=np.int32)
        if code_bytes == 4:
            wblock[0, 0], wblock[1, 4] = 13, 16
    tensors = [(numel, 0, index[t], t % 2 == 1) for t, numel in enumerate(numels)]
    gen = np.random.default_rng(30 + seed)
    codes = []
    for n in range(len(wblock)):
        row = []
        for (numel, _, wi, s) in tensors:
            b = int(wblock[n, wi])
            b = b if 1 <= b <= 16 else 4
            q = _full_range(gen, numel, b, s)
            if out_of_range:
                q = q + gen.integers(-3, 4, size=numel) * (1 << b)
            row.append(q)
        codes.append(row)
    return _Abi(engine, tensors, codes, code_bytes, wblock, seed)


@pytest.mark.parametrize('code_bytes', [4, 1])
def test_widths_read_on_the_device(engine, code_bytes):
    abi = _device_width_case(engine, code_bytes)
    assert abi.wblock.shape[1] > abi.T and abi.sizes()[0] != abi.sizes()[1]
    assert all(abi.width(0, t) != abi.width(1, t) for t in range(abi.T))
    words, offsets, status = abi.pack()
    abi.check_packed(words, offsets, status)
    assert not np.array_equal(offsets[0], offsets[1])
    abi.unpack(code_bytes=code_bytes)
    abi.unpack(code_bytes=None)                        # weights alone
    abi.unpack(code_bytes=4, weights=False)            # codes alone, always possible as int32


# ---- 3. capacity, bad widths, the mask -------------------------------------------------------------------------------------------
def test_a_row_one_word_short(engine):
    wblock = _device_width_case(engine, 4).wblock[::-1].copy()          # (the larger network second)
    abi = _device_width_case(engine, 4, wblock=wblock)
    sizes = abi.sizes()
    assert sizes[1] > sizes[0]
    words, offsets, status = abi.pack(word_stride=sizes[1] - 1)
    assert status.tolist() == [0, 1]
    assert (words[1] == FILL).all(), 'a network that does not fit is not written'
    want = np.cumsum([0] + [_extent(abi.tensors[t][0], abi.width(1, t)) for t in range(abi.T)])
    assert offsets[1].tolist() == want.tolist() and offsets[1, -1] == sizes[1], 'its offsets say what it needs'
    abi.check_packed(words, offsets, status, skipped=(1,))
    # and unpack skips it under the same rule
    abi.unpack(code_bytes=4, skipped=(1,), expect_status=[0, 1])


@pytest.mark.parametrize('bad, code_bytes', [(0, 4), (17, 4), (-3, 4), (9, 1)])
def test_a_bad_width_on_the_device(engine, bad, code_bytes):
    abi = _device_width_case(engine, code_bytes)
    wblock = abi.wblock.copy()
    wblock[1, 4] = bad
    abi = _device_width_case(engine, code_bytes, wblock=wblock)
    words, offsets, status = abi.pack(word_stride=4 * abi.code_stride)
    assert status.tolist() == [0, 2]
    assert (words[1] == FILL).all() and (offsets[1] == -7).all(), 'nothing of a network with a bad width is written'
    abi.check_packed(words, offsets, status, skipped=(1,))
    abi.unpack(code_bytes=code_bytes, skipped=(1,), expect_status=[0, 2])


def test_unpack_checks_the_offsets_it_is_given(engine):
    abi = _device_width_case(engine, 4, n_nets=3)
    words, offsets, status = abi.pack()
    abi.check_packed(words, offsets, status)
    off = offsets.copy()
    off[1, 2:] += 4                                    # a tensor of network 1 four words longer than its width says
    off[2, 0] = 4                                      # network 2 does not start at 0
    abi.offsets = torch.from_numpy(off).to(engine.device)
    abi.unpack(code_bytes=4, skipped=(1, 2), expect_status=[0, 1, 1])
    abi.offsets = torch.from_numpy(offsets).to(engine.device)
    abi.word_stride = int(offsets[:, -1].max()) - 1    # the longest network no longer fits what unpack is told the rows hold
    longest = int(np.argmax(offsets[:, -1]))
    abi.packed = abi.packed[:, :abi.word_stride].contiguous()
    want = [0, 0, 0]
    want[longest] = 1
    abi.unpack(code_bytes=4, skipped=(longest,), expect_status=want)


@pytest.mark.parametrize('code_bytes', [4, 1])
def test_out_of_range_codes_are_masked(engine, code_bytes):
    abi = _device_width_case(engine, code_bytes, seed=7, out_of_range=True)
    assert any((q != _masked(q, abi.width(0, t), abi.tensors[t][3])).any() for t, q in enumerate(abi.codes[0]))
    words, offsets, status = abi.pack()
    abi.check_packed(words, offsets, status)
    abi.unpack(code_bytes=code_bytes)                  # (compares with the masked codes)


# ---- 5. batches --------------------------------------------------------------------------------------------------------------------
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
    return OrderedDict((k, m.weight.detach().cpu().numpy().copy()) for k, m in _targ(graph))


def _source(batch, kind, per_channel, signed):
    if kind == 'mixed':
        return batch.mixed_plan(WIDTHS, avg_bits=4.5, per_channel=per_channel, signed=signed, codes='int8', apply=True)
    if kind == 'quant':
        return batch.quant_plan(bit_weight=4, bits_bias=32, per_channel=per_channel, signed=signed, codes='int8')
    return batch.squant_plan(bit_weight=3, per_channel=per_channel, signed=signed, codes='int32')


def _assert_weights(nets, snaps, what):
    """value-equal everywhere, bit-equal wherever the snapshot is not a zero"""
    for n, (_, g, _, _) in enumerate(nets):
        for k, w in _weights(g).items():
            s = snaps[n][k]
            assert np.array_equal(w, s), '{} net {} {}: values'.format(what, n, k)
            nz = s != 0
            assert np.array_equal(_bits_of(w)[nz], _bits_of(s)[nz]), '{} net {} {}: bits'.format(what, n, k)


def _overwrite(nets, value=0.25):
    with torch.no_grad():
        for (_, g, _, _) in nets:
            for _, m in _targ(g):
                m.weight.fill_(value)


@pytest.mark.parametrize('name', NAMES)
@pytest.mark.parametrize('pair', PAIRS)
@pytest.mark.parametrize('kind', ['mixed', 'quant', 'squant'])
def test_batches_round_trip(engine, name, pair, kind):
    per_channel, signed = pair
    nets, batch = _batch(name, SEEDS, engine.device)
    src = _source(batch, kind, per_channel, signed)
    src.run()
    pack = batch.pack_plan(src)
    assert pack.launches == 2
    pack.run()
    _ffi.synchronize()
    T = len(pack.keys)
    assert pack.status_block.cpu().tolist() == [0] * len(SEEDS)
    widths = pack.widths_array()
    sizes = [m.weight.numel() for _, m in _targ(nets[0][1])]
    for n in range(len(SEEDS)):
        used = src.used(n)[0] if kind == 'mixed' else sum(sizes) * {'quant': 4, 'squant': 3}[kind]
        assert used == int((widths[n].astype(np.int64) * np.array(sizes)).sum())
        assert 0 <= pack.size_bits(n) - used < 159 * T
        assert pack.status(n) == 0
        # the words are the restatement of the source's own codes
        codes, got = src.codes(n), pack.words(n)
        for t, k in enumerate(pack.keys):
            want = _pack_ref(codes[k].cpu().numpy().astype(np.int64), int(widths[n, t]), signed)
            assert np.array_equal(got[k].cpu().numpy().view(np.uint32), want), '{} net {} {}'.format(name, n, k)
    if kind == 'mixed':
        assert len(set(widths.reshape(-1).tolist())) >= 2, 'one width for everything: the test shows nothing'
    snaps = [_weights(g) for (_, g, _, _) in nets]
    _overwrite(nets)
    un = batch.unpack_plan(pack, weights=True, codes='int32')
    assert un.launches == 1
    un.run()
    _ffi.synchronize()
    assert un.status_block.cpu().tolist() == [0] * len(SEEDS)
    _assert_weights(nets, snaps, '{} {}'.format(name, kind))
    for n in range(len(SEEDS)):
        for k, c in src.codes(n).items():
            assert torch.equal(un.codes(n)[k].cpu().to(torch.int64), c.cpu().to(torch.int64)), k
    for p in (un, pack, src):
        p.close()
    with pytest.raises(RuntimeError):
        pack.run()


# ---- 6. the file -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pair', [(False, False), (True, True)])
def test_save_and_load(engine, pair, tmp_path):
    per_channel, signed = pair
    name, seeds = 'tiny_mobile', SEEDS[:2]
    nets, batch = _batch(name, seeds, engine.device)
    src = _source(batch, 'mixed', per_channel, signed)
    src.run()
    path = str(tmp_path / 'packed.npz')
    pack = batch.save_packed(path, src)
    src.close()
    snaps = [_weights(g) for (_, g, _, _) in nets]
    biases = [{k: m.bias.detach().cpu().numpy().copy() for k, m in _targ(g) if m.bias is not None} for (_, g, _, _) in nets]
    offsets = pack.offset_block.cpu().numpy()
    with np.load(path, allow_pickle=False) as f:
        assert int(f['version']) == 1
        for n in range(len(seeds)):
            assert f['words_{}'.format(n)].dtype == np.uint32 and f['words_{}'.format(n)].size == int(offsets[n, -1])
        assert np.array_equal(f['offsets'], offsets) and np.array_equal(f['widths'], pack.widths_array())
        assert [str(k) for k in f['keys']] == pack.keys
        saved = {k: f[k] for k in f.files}
    # a fresh batch of the same architecture, other weights
    nets2, batch2 = _batch(name, [5, 6], engine.device)
    assert not np.array_equal(list(_weights(nets2[0][1]).values())[0], list(snaps[0].values())[0])
    loaded = batch2.load_packed(path)
    assert isinstance(loaded, arena.PackedBatch) and loaded.keys == pack.keys
    _assert_weights(nets2, snaps, 'loaded')
    for n, (_, g, _, _) in enumerate(nets2):
        for k, b in biases[n].items():
            assert np.array_equal(_bits_of(g[k].bias.detach().cpu().numpy()), _bits_of(b)), k
    assert [loaded.size_bits(n) for n in range(len(seeds))] == [pack.size_bits(n) for n in range(len(seeds))]
    # the loaded blocks unpack again, to codes
    un = batch2.unpack_plan(loaded, weights=False, codes='int8')
    un.run()
    _ffi.synchronize()
    for n in range(len(seeds)):
        for t, k in enumerate(pack.keys):
            want = _unpack_ref(saved['words_{}'.format(n)][offsets[n, t]:offsets[n, t + 1]], snaps[n][k].size, int(saved['widths'][n, t]), signed)
            assert np.array_equal(un.codes(n)[k].cpu().numpy().astype(np.int64).reshape(-1), want), k
    un.close()
    # another architecture, another batch size, a bumped version
    _, other = _batch('tiny_res', seeds[:1], engine.device)
    with pytest.raises(ValueError):
        other.load_packed(path)
    _, two = _batch(name, seeds[:1], engine.device)
    with pytest.raises(ValueError):
        two.load_packed(path)
    saved['version'] = np.int64(2)
    bumped = str(tmp_path / 'bumped.npz')
    np.savez(bumped, **saved)
    with pytest.raises(ValueError):
        batch2.load_packed(bumped)
    saved['version'] = np.int64(1)
    for gone in ('offsets', 'keys', 'words_1', 'biases'):           # a truncated or foreign file: ValueError, not KeyError
        cut = str(tmp_path / 'cut.npz')
        np.savez(cut, **{k: v for k, v in saved.items() if k != gone})
        with pytest.raises(ValueError):
            batch2.load_packed(cut)
    _assert_weights(nets2, snaps, 'after the refusals')


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------
def test_abi_rejects_bad_arguments(engine):
    lib, dev = _ffi.lib(), engine.device
    buf = torch.zeros(4096, dtype=torch.float32, device=dev)
    codes = torch.zeros(2 * 1024, dtype=torch.int32, device=dev)
    widths = torch.full((2 * 4,), 4, dtype=torch.int32, device=dev)
    packed = torch.zeros(2 * 512, dtype=torch.int32, device=dev)
    offsets = torch.zeros(2 * 3, dtype=torch.int64, device=dev)
    status = torch.zeros(2, dtype=torch.int32, device=dev)
    ranges = torch.zeros(2 * 64, dtype=torch.float32, device=dev)
    ranges[0::2], ranges[1::2] = -1.0, 1.0
    P, Q = _ffi.DfqBatchPackTensor, _ffi.DfqBatchUnpackTensor

    def pack(table=True, n_tensors=2, numel=300, bits=4, widx=1, code_off=0, code_bytes=4, code_stride=1024, widths_ptr=True, width_stride=4,
             codes_ptr=True, packed_ptr=True, offsets_ptr=True, status_ptr=True, word_stride=512, bases=True, n_nets=2, base1=1024 * 4,
             place=True):
        plan = ctypes.c_void_p()
        tabs = (P * 2)(P(code_off, numel, bits, widx, 0, 0), P(512, 100, 0, 3, 1, 0))
        ba = (ctypes.c_void_p * 2)(buf.data_ptr(), buf.data_ptr() + base1) if bases else None
        rc = lib.dfq_batch_pack_plan_create(tabs if table else None, n_tensors, ba, n_nets, codes.data_ptr() if codes_ptr else None, code_bytes,
                                            code_stride, widths.data_ptr() if widths_ptr else None, width_stride,
                                            packed.data_ptr() if packed_ptr else None, word_stride, offsets.data_ptr() if offsets_ptr else None,
                                            status.data_ptr() if status_ptr else None, ctypes.byref(plan) if place else None)
        return rc, plan

    def unpack(data=0, rows=10, row_len=30, numel=300, range_off=0, per_row=1, ranges_ptr=True, range_stride=64, codes_ptr=True, words_ptr=True,
               offsets_ptr=True, status_ptr=True, code_bytes=4, bits=4, widths_ptr=True, widx=1, width_stride=4, code_off=0, code_stride=1024,
               table=True, n_tensors=1, bases=True, n_nets=2, base1=1024 * 4, place=True, word_stride=512):
        plan = ctypes.c_void_p()
        tabs = (Q * 1)(Q(None if data is None else buf.data_ptr() + data, rows, row_len, code_off, numel, range_off, bits, widx, 0, per_row))
        ba = (ctypes.c_void_p * 2)(buf.data_ptr(), buf.data_ptr() + base1) if bases else None
        rc = lib.dfq_batch_unpack_plan_create(tabs if table else None, n_tensors, ba, n_nets, packed.data_ptr() if words_ptr else None, word_stride,
                                              offsets.data_ptr() if offsets_ptr else None, widths.data_ptr() if widths_ptr else None,
                                              width_stride, ranges.data_ptr() if ranges_ptr else None, range_stride,
                                              codes.data_ptr() if codes_ptr else None, code_bytes, code_stride,
                                              status.data_ptr() if status_ptr else None, ctypes.byref(plan) if place else None)
        return rc, plan

    def valid():
        rc, plan = pack()
        assert rc == 0, lib.dfq_last_error()
        assert lib.dfq_batch_pack_plan_launches(plan) == 2
        _ffi.check(lib.dfq_batch_pack_plan_run(plan, _ffi.stream_arg()))
        _ffi.synchronize()
        lib.dfq_batch_pack_plan_destroy(plan)
        assert status.cpu().tolist() == [0, 0] and offsets.cpu().tolist() == [0, 40, 56, 0, 40, 56]
        rc, plan = unpack(n_tensors=1, numel=300)
        assert rc == 0, lib.dfq_last_error()
        lib.dfq_batch_unpack_plan_destroy(plan)

    valid()
    bad_pack = [dict(table=False), dict(n_tensors=0), dict(place=False), dict(code_bytes=2), dict(code_bytes=0), dict(bits=17), dict(bits=-1),
                dict(bits=9, code_bytes=1), dict(bits=0, widths_ptr=False), dict(bits=0, widx=4), dict(bits=0, widx=-1),
                dict(widths_ptr=False),                # (the second tensor reads the block)
                dict(code_off=1024 - 299), dict(code_off=-1), dict(code_stride=-1), dict(word_stride=-1), dict(width_stride=-1),
                dict(codes_ptr=False), dict(packed_ptr=False), dict(offsets_ptr=False), dict(status_ptr=False),
                dict(numel=0), dict(numel=-5), dict(bases=False), dict(n_nets=0), dict(base1=1024 * 4 + 8)]
    for kw in bad_pack:
        rc, plan = pack(**kw)
        assert rc == DFQ_ERR_ARG, kw
        assert b'dfq_batch_pack_plan_create' in lib.dfq_last_error(), kw
        assert not plan.value, kw
    valid()
    bad_unpack = [dict(table=False), dict(n_tensors=0), dict(place=False), dict(code_bytes=2), dict(bits=17), dict(bits=9, code_bytes=1),
                  dict(bits=0, widths_ptr=False), dict(bits=0, widx=4), dict(code_off=1024 - 299), dict(code_off=-1), dict(numel=0),
                  dict(words_ptr=False), dict(offsets_ptr=False), dict(status_ptr=False), dict(bases=False), dict(n_nets=0),
                  dict(base1=1024 * 4 + 8), dict(ranges_ptr=False), dict(range_off=-1), dict(range_off=64 - 19), dict(range_stride=-1),
                  dict(data=4), dict(rows=7), dict(rows=0), dict(row_len=0), dict(data=None, codes_ptr=False), dict(word_stride=-1)]
    for kw in bad_unpack:
        rc, plan = unpack(**kw)
        assert rc == DFQ_ERR_ARG, kw
        assert b'dfq_batch_unpack_plan_create' in lib.dfq_last_error(), kw
        assert not plan.value, kw
    # codes only needs no range block; with a null code block its offsets and width mean nothing
    for kw in (dict(data=None, ranges_ptr=False, range_off=-1), dict(codes_ptr=False, code_off=-9, code_bytes=0)):
        rc, plan = unpack(**kw)
        assert rc == 0, (kw, lib.dfq_last_error())
        lib.dfq_batch_unpack_plan_destroy(plan)
    valid()
    assert lib.dfq_batch_pack_plan_run(None, None) == DFQ_ERR_ARG and b'dfq_batch_pack_plan_run' in lib.dfq_last_error()
    assert lib.dfq_batch_unpack_plan_run(None, None) == DFQ_ERR_ARG and b'dfq_batch_unpack_plan_run' in lib.dfq_last_error()
    assert lib.dfq_batch_pack_plan_launches(None) == 0 and lib.dfq_batch_unpack_plan_launches(None) == 0
    lib.dfq_batch_pack_plan_destroy(None)
    lib.dfq_batch_unpack_plan_destroy(None)


def test_python_refusals(engine):
    nets, batch = _batch('tiny_res', [3], engine.device)
    _, other = _batch('tiny_res', [4], engine.device)
    plain = batch.quant_plan(4, 32)                    # no codes
    with pytest.raises(ValueError):
        batch.pack_plan(plain)
    plain.close()
    alloc = batch.mixed_plan(WIDTHS, avg_bits=4, codes='int8', apply=False)
    with pytest.raises(ValueError):
        batch.pack_plan(alloc)
    alloc.close()
    src = batch.quant_plan(4, 32, codes='int8')
    with pytest.raises(ValueError):
        other.pack_plan(src)                           # a plan of another batch
    with pytest.raises(ValueError):
        batch.pack_plan('quant_plan')
    for ws in (-1, 2.5, True):
        with pytest.raises(ValueError):
            batch.pack_plan(src, word_stride=ws)
    src.run()
    pack = batch.pack_plan(src)
    pack.run()
    _ffi.synchronize()
    for kw in (dict(weights=False), dict(codes='int16'), dict(packed=src)):
        with pytest.raises(ValueError):
            batch.unpack_plan(kw.pop('packed', pack), **kw)
    _, res2 = _batch('tiny_cat', [3], engine.device)
    with pytest.raises(ValueError):
        res2.unpack_plan(pack)                         # another architecture
    src.close()
    with pytest.raises(ValueError):
        batch.pack_plan(src)                           # a closed source
    with pytest.raises(ValueError):
        batch.save_packed(os.devnull, src)
    wide = batch.quant_plan(12, 32, codes='int32')
    wide.run()
    wp = batch.pack_plan(wide)
    with pytest.raises(ValueError):
        batch.unpack_plan(wp, codes='int8')            # twelve bits in a byte
    un = batch.unpack_plan(pack)                       # what was valid still works
    un.run()
    _ffi.synchronize()
    assert un.status(0) == 0
    for p in (un, wp, wide):
        p.close()
    batch.release()
    with pytest.raises(RuntimeError):
        pack.run()
    with pytest.raises(RuntimeError):
        batch.pack_plan(src)
    pack.close()


# ---- 8. ABI layout -----------------------------------------------------------------------------------------------------------------
def test_struct_layout_matches_header():
    src = r'''
    #include <stdio.h>
    #include <stddef.h>
    #include "dfq_hip.h"
    #define P dfq_batch_pack_tensor
    #define U dfq_batch_unpack_tensor
    int main(void) {
        printf("%zu %zu %zu %zu %zu %zu %zu ", sizeof(P), offsetof(P, code_offset), offsetof(P, numel), offsetof(P, num_bits),
               offsetof(P, width_index), offsetof(P, symmetric), offsetof(P, pad));
        printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(U), offsetof(U, data), offsetof(U, rows), offsetof(U, row_len),
               offsetof(U, code_offset), offsetof(U, numel), offsetof(U, range_offset), offsetof(U, num_bits), offsetof(U, width_index),
               offsetof(U, symmetric), offsetof(U, per_row));
        return 0;
    }'''
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, 't.c')
        open(c, 'w').write(src)
        exe = os.path.join(d, 't')
        subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), c, '-o', exe], check=True)
        got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    P, U = _ffi.DfqBatchPackTensor, _ffi.DfqBatchUnpackTensor
    assert got == [ctypes.sizeof(P), P.code_offset.offset, P.numel.offset, P.num_bits.offset, P.width_index.offset, P.symmetric.offset,
                   P.pad.offset,
                   ctypes.sizeof(U), U.data.offset, U.rows.offset, U.row_len.offset, U.code_offset.offset, U.numel.offset,
                   U.range_offset.offset, U.num_bits.offset, U.width_index.offset, U.symmetric.offset, U.per_row.offset]


# ---- 9. determinism and independence -----------------------------------------------------------------------------------------------
def test_two_runs_and_a_network_s_place(engine):
    three = _device_width_case(engine, 4, n_nets=3)
    words3, offsets3, status3 = three.pack(runs=2)
    three.check_packed(words3, offsets3, status3)
    alone = _Abi(engine, three.tensors, three.codes[1:2], 4, three.wblock[1:2])
    words1, offsets1, status1 = alone.pack(word_stride=three.word_stride, runs=2)
    assert words1[0].tobytes() == words3[1].tobytes() and offsets1[0].tobytes() == offsets3[1].tobytes() and status1[0] == status3[1]
    # the same through the Python layer: a batch of three and the batch that holds network 1 alone
    nets, batch = _batch('tiny_cat', SEEDS, engine.device)
    nets1, batch1 = _batch('tiny_cat', SEEDS[1:2], engine.device)
    got = []
    for b in (batch, batch1):
        src = _source(b, 'mixed', True, True)
        src.run()
        pack = b.pack_plan(src)
        pack.run()
        _ffi.synchronize()
        first = pack.packed_block.clone()
        pack.packed_block.fill_(FILL_I32)              # packing needs no cleared block: a second run over other contents
        pack.run()
        _ffi.synchronize()
        size = [int(v) for v in pack.offset_block[:, -1].cpu()]
        for n, s in enumerate(size):
            assert torch.equal(first[n, :s], pack.packed_block[n, :s]), 'two runs differ'
            assert (pack.packed_block[n, s:] == FILL_I32).all()
        got.append((pack.packed_block.cpu().numpy(), pack.offset_block.cpu().numpy(), size))
        pack.close()
        src.close()
    (w3, o3, s3), (w1, o1, s1) = got
    assert s1[0] == s3[1] and o1[0].tobytes() == o3[1].tobytes() and w1[0, :s1[0]].tobytes() == w3[1, :s3[1]].tobytes()
