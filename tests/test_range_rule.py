"""The NaN rule of the ranges at every place a lane folds a value from memory (dfq_range.hpp): "a NaN of any payload, quiet or
signalling, is SKIPPED" (include/dfq_hip.h, "Special values").

v_min_f32 / v_max_f32 return a NaN for a SIGNALLING operand, and the step after it then keeps its other operand: a fold
without quiet_nan() loses what the lane had accumulated.  So every case plants an extremum of large magnitude and puts a NaN
word in the element the SAME lane folds directly behind it ('behind'), or directly in front of it ('in front'), for each of
the four NaN words of tests/test_quant_adversarial.py.  Results are compared bit for bit with numpy's NaN-skipping min / max
and with the single-network entry point that computes the same thing.  Network 0 of every batch carries the plants, network
1 is clean: its results must be those of its own values.

What the cases did on the commit before dfq_range.hpp, on the CPU emulation (its fminf / fmaxf return a NaN for a signalling
operand like the raw instructions).  Cases of the two quiet words passed; of the signalling words:
  * test_quant_plan_sites, both orders, FAILED: 'behind' lost the planted value in bq_rows (every lane class), bq_long_row and
    bq_chunk_minmax_kernel; 'in front' failed on the row of nothing but signalling NaN alone, which got (NaN, NaN) instead of
    the identities the single-network path gives.  The raw instructions do the same on the MI355X.
  * test_table_plan_sites, all ten, FAILED: a row of nothing but signalling NaN got max|w| = NaN instead of 0 everywhere;
    'vector', 'slot' and 'tail' 'behind' also lost the planted value from the tensor's range (the next extremum of the
    Gaussian data instead of -1000), 'vector' from the row's max|w| too.  'scan' and 'boundary' hand on a lane's RESULT, which is never signalling:
    no loss of their own.  The same is expected on the MI355X.
  * test_single_network_sites, both orders, and test_bc_row_range['behind'] FAILED on the emulation only: row_seg_quant_kernel,
    fake_quant_rows_kernel and bc_row_range_kernel used fminf without the guard.  On the MI355X fminf canonicalises its
    operands, so these are expected to have passed there.  dfq_row_range, dfq_col_range and dfq_tensor_minmax had the guard.
  * test_error_plan_sites passed: dfq_batch_error_plan reports sums only, and a tensor holding a NaN has NaN sums whatever
    range be_range_kernel found, so no input shows that kernel's rule through the C ABI.  The cases pin what can be seen --
    NaN sums in that tensor's slot alone, the clean network's bits unchanged -- and be_range_kernel's folds are the
    range_fold calls that the table plan's cases exercise in bt_stream_kernel.
"""
import ctypes

import numpy as np
import pytest
import torch

from dfq_amd import _ffi, dfq, prims, synthetic
from dfq_amd.utils import layer_transform as lt
from dfq_amd.utils import quantize as q

from common import F32, TARG, assert_bitexact
from test_batch_quant import _row_quant
from test_quant_adversarial import NEG_QNAN, NEG_SNAN, QNAN, SNAN

WORDS = {'quiet': QNAN, 'negative quiet': NEG_QNAN, 'signalling': SNAN, 'negative signalling': NEG_SNAN}
ORDERS = ('behind', 'in front')
LOW, HIGH = F32(-1000.0), F32(2000.0)
PIECE = 4096                      # floats of a flat piece of the table / error plans (dfq_batch_shared.hpp)


def _put(x, planted, nan, value, word, order):
    """`value` at flat position `planted` and the NaN word at `nan` -- the other way round for 'in front'"""
    a, b = (planted, nan) if order == 'behind' else (nan, planted)
    flat = x.reshape(-1)
    flat[a] = value
    flat.view(np.uint32)[b] = word


def _fill(x, word):
    x.reshape(-1).view(np.uint32)[:] = word


def _range(x):
    """(min, max) of the values that are not NaN; the identities (inf, -inf) if there is none"""
    keep = x.reshape(-1)[~np.isnan(x.reshape(-1))]
    return (F32(np.inf), F32(-np.inf)) if keep.size == 0 else (keep.min(), keep.max())


def _row_ranges(x):
    return np.array([_range(r) for r in x], dtype=F32)


def _tensor_range(x):
    mn, mx = _range(x)
    return np.array([np.nan, np.nan] if mn > mx else [mn, mx], dtype=F32)


def _dev(engine, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(engine.device)


def _host(t):
    return t.detach().cpu().numpy()


class _Store:
    """two networks' tensors in one allocation, 16-byte aligned, with gaps that would show in a range"""

    def __init__(self, nets):
        self.offs, total = [], 0
        for x in nets[0]:
            self.offs.append(total)
            total += -(-x.size // 4) * 4 + 8
        self.stride = total
        host = np.full((len(nets), total), 7.5e5, dtype=F32)
        for k, xs in enumerate(nets):
            for x, o in zip(xs, self.offs):
                host[k, o:o + x.size] = x.reshape(-1)
        self.host = host

    def to(self, engine):
        self.dev = _dev(engine, self.host)
        base = self.dev.data_ptr()
        self.bases = (ctypes.c_void_p * len(self.host))(*[base + 4 * k * self.stride for k in range(len(self.host))])
        return base

    def view(self, k, j, shape):
        o = self.offs[j]
        return self.dev[k, o:o + int(np.prod(shape))].view(*shape)


# ---- dfq_batch_quant_plan: bq_rows, bq_long_row, bq_chunk_minmax_kernel -------------------------------------------------------
# (row length, lanes per row L): a lane folds elements g, g + L, ...; four slots per lane below L = 64, 24 there
ROW_CLASSES = [(9, 4), (27, 8), (64, 16), (128, 32), (1536, 64)]
LONG_ROW = 1537                   # one wave, stride 64
CHUNKED = 4096 + 259              # per tensor, two chunks of 256 threads x 16 slots, the second with a partial slot


def _quant_tensors(word, order, rng):
    """[(x [rows, len], per_row)]: rows 0 / 1 carry a minimum / a maximum pair, row 2 is nothing but NaN, row 4 both pairs"""
    out = []
    for n, L in ROW_CLASSES + [(LONG_ROW, 64)]:
        x = rng.standard_normal((6, n)).astype(F32)
        lo, hi = n % L if n % L and n > 2 * L else 0, n - 1 - L       # the first pair of lanes of a row, and the last
        _put(x[0], lo, lo + L, LOW, word, order)
        _put(x[1], hi, hi + L, HIGH, word, order)
        _fill(x[2], word)
        _put(x[4], hi, hi + L, LOW, word, order)
        _put(x[4], lo, lo + L, HIGH, word, order)
        out.append((x, 1))
    x = rng.standard_normal((1, CHUNKED)).astype(F32)
    _put(x, 10, 10 + 256, LOW, word, order)                           # thread 10 of the first chunk, slots 0 and 1
    _put(x, PIECE + 1, PIECE + 1 + 256, HIGH, word, order)            # thread 1 of the second, its whole and its partial slot
    out.append((x, 0))
    x = rng.standard_normal((1, CHUNKED)).astype(F32)
    _fill(x, word)
    out.append((x, 0))
    return out


@pytest.mark.parametrize('order', ORDERS)
@pytest.mark.parametrize('name', list(WORDS))
def test_quant_plan_sites(engine, name, order):
    lib = _ffi.lib()
    rng = np.random.default_rng(1)
    planted = _quant_tensors(WORDS[name], order, rng)
    clean = [rng.standard_normal(x.shape).astype(F32) for x, _ in planted]
    store = _Store([[x for x, _ in planted], clean])
    base0 = store.to(engine)
    rng_offs, rs = [], 0
    for x, per_row in planted:
        rng_offs.append(rs)
        rs += 2 * (x.shape[0] if per_row else 1)
    ranges = torch.full((2, rs + 1), 5.0, dtype=torch.float32, device=engine.device)
    T = _ffi.DfqBatchQuantTensor
    tabs = (T * len(planted))(*[T(base0 + 4 * o, x.shape[0], x.shape[1], 8, 0, per_row, 0, -1, ro)
                                for (x, per_row), o, ro in zip(planted, store.offs, rng_offs)])
    singles = []                  # the single-network paths, on copies taken before the plan quantises in place
    for j, (x, per_row) in enumerate(planted):
        xd = store.view(0, j, x.shape).clone()
        singles.append(_row_quant(lib, xd, 8, 0)[2] if per_row else q.tensor_minmax(xd))
    plan = ctypes.c_void_p()
    _ffi.check(lib.dfq_batch_quant_plan_create(tabs, len(planted), store.bases, 2, None, 4, 0, ranges.data_ptr(), rs + 1, ctypes.byref(plan)))
    assert lib.dfq_batch_quant_plan_launches(plan) == 2
    _ffi.check(lib.dfq_batch_quant_plan_run(plan, _ffi.stream_arg()))
    _ffi.synchronize()
    lib.dfq_batch_quant_plan_destroy(plan)
    got = _host(ranges)
    for j, ((x, per_row), ro) in enumerate(zip(planted, rng_offs)):
        what = '{} {}: tensor {} {}'.format(name, order, j, x.shape)
        for k, xs in enumerate((x, clean[j])):
            want = _row_ranges(xs) if per_row else _tensor_range(xs)
            assert_bitexact(got[k, ro:ro + want.size], want.reshape(-1), '{} net {} against numpy'.format(what, k))
        assert_bitexact(got[0, ro:ro + 2 * (x.shape[0] if per_row else 1)], _host(singles[j]).reshape(-1), what + ' against the single-network path')
    assert (got[:, -1] == 5.0).all()


# ---- the flat pieces: bt_stream_kernel (range and max|w|), be_range_kernel ------------------------------------------------------
# (rows, row_len): a second piece of 7 floats or a few more, ending in three single floats where the row length allows it
PIECE_SHAPES = [(4103, 1), (1369, 3), (459, 9), (65, 64), (1, 4103)]
PLACES = ('vector', 'slot', 'scan', 'boundary', 'tail')


def _place(place, rows, n):
    """(planted, nan) flat positions for 'behind', or None where the shape has no such place"""
    size = rows * n
    if place == 'vector':         # two neighbours in one 16-byte vector, in one row where rows have two elements
        e = next(e for e in range(20, 200) if e % 4 <= 2 and (n == 1 or e // n == (e + 1) // n))
        return e, e + 1
    if place == 'slot':           # the last element of lane 7's first vector, the first of its second (256 vectors further)
        return 4 * 7 + 3, 4 * (7 + 256)
    if place == 'scan':           # the last element of one lane's vector, the first of the next lane's, both vectors starting in one row
        if n < 8:
            return None
        v = next(v for v in range(9, 200) if (4 * v) // n == (4 * v + 7) // n)
        return 4 * v + 3, 4 * v + 4
    if place == 'boundary':       # the last element of the first piece, the first of the second
        return PIECE - 1, PIECE
    nv, tail = (size - PIECE) >> 2, (size - PIECE) & 3                 # the second piece: whole vectors, single floats
    t = min(1, nv - 1)            # a lane that has a vector and a single float: the float is folded behind the vector
    return (PIECE + 4 * t + 3, PIECE + 4 * nv + t) if t < tail else None


def _piece_tensors(place, word, value, order, rng):
    xs = []
    for rows, n in PIECE_SHAPES:
        x = rng.standard_normal((rows, n)).astype(F32)
        at = _place(place, rows, n)
        if at is not None:
            _put(x, at[0], at[1], value, word, order)
        if rows > 1:
            _fill(x[2000 // n], word)                                   # a row of nothing but NaN, away from the plants
        xs.append(x)
    x = rng.standard_normal((457, 9)).astype(F32)
    _fill(x, word)
    xs.append(x)
    return xs


def _table_plan(engine, store, shapes, n_nets=2):
    """dfq_batch_table_plan over the store -> [n_nets][tensor] of ((min, max), max|w| per row)"""
    lib = _ffi.lib()
    base0 = store.dev.data_ptr()
    offs, total = [], 0
    for rows, _ in shapes:
        offs.append(total)
        total += 2 + rows + 1
    out = torch.full((n_nets, total), 9.0, dtype=torch.float32, device=engine.device)
    T = _ffi.DfqBatchTableTensor
    tabs = (T * len(shapes))(*[T(base0 + 4 * o, rows, n, f, f + 2) for (rows, n), o, f in zip(shapes, store.offs, offs)])
    plan = ctypes.c_void_p()
    _ffi.check(lib.dfq_batch_table_plan_create(tabs, len(shapes), store.bases, n_nets, out.data_ptr(), total, ctypes.byref(plan)))
    _ffi.check(lib.dfq_batch_table_plan_run(plan, _ffi.stream_arg()))
    _ffi.synchronize()
    lib.dfq_batch_table_plan_destroy(plan)
    got = _host(out)
    return [[(got[k, f:f + 2], got[k, f + 2:f + 2 + rows]) for (rows, _), f in zip(shapes, offs)] for k in range(n_nets)]


@pytest.mark.parametrize('order', ORDERS)
@pytest.mark.parametrize('place', PLACES)
def test_table_plan_sites(engine, place, order):
    shapes = PIECE_SHAPES + [(457, 9)]
    for name, word in WORDS.items():
        for value in (LOW, HIGH):
            rng = np.random.default_rng(2)
            planted = _piece_tensors(place, word, value, order, rng)
            clean = [rng.standard_normal(x.shape).astype(F32) for x in planted]
            store = _Store([planted, clean])
            store.to(engine)
            got = _table_plan(engine, store, shapes)
            for j, x in enumerate(planted):
                what = '{} {} {} {}: tensor {} {}'.format(place, order, name, value, j, x.shape)
                for k, xs in enumerate((x, clean[j])):
                    with np.errstate(invalid='ignore'):
                        rows = np.array([max(-r[0], r[1]) if r[0] <= r[1] else 0.0 for r in _row_ranges(xs)], dtype=F32)
                    assert_bitexact(got[k][j][0], _tensor_range(xs), '{} net {} (min, max) against numpy'.format(what, k))
                    assert_bitexact(got[k][j][1], rows, '{} net {} max|w| against numpy'.format(what, k))
                xd = store.view(0, j, x.shape)
                assert_bitexact(got[0][j][0], _host(q.tensor_minmax(xd)), what + ' (min, max) against dfq_tensor_minmax')
                # dfq_row_range spends a wave on every row: the rows of the plants, the row of NaN, the first and the last
                at = _place(place, *x.shape) or (0, 0)
                pick = sorted({0, at[0] // x.shape[1], at[1] // x.shape[1], 2000 // x.shape[1], x.shape[0] - 1} & set(range(x.shape[0])))
                single = _host(prims.row_range(xd[pick].contiguous(), signed=True))
                empty = np.isnan(x[pick]).all(axis=1)
                assert (single[empty] == -np.inf).all() and (got[0][j][1][pick][empty] == 0.0).all(), what   # nothing but NaN
                assert_bitexact(got[0][j][1][pick][~empty], single[~empty], what + ' max|w| against dfq_row_range')


@pytest.mark.parametrize('order', ORDERS)
@pytest.mark.parametrize('place', PLACES)
def test_error_plan_sites(engine, place, order):
    """The plan reports sums, and a NaN element makes every sum of its tensor NaN: that, and nothing else, is what a NaN does."""
    lib = _ffi.lib()
    shapes = PIECE_SHAPES + [(457, 9)]
    configs = ((8, 0, 0), (4, 1, 1))                                    # (bits, symmetric, per_row)
    n_vals = 1 + 3 * len(configs)
    T, C = _ffi.DfqBatchErrorTensor, _ffi.DfqBatchErrorConfig
    cfgs = (C * len(configs))(*[C(b, s, p, 0) for b, s, p in configs])

    def run(store, n_nets):
        out = torch.full((n_nets, n_vals * len(shapes) + 1), 9.0, dtype=torch.float64, device=engine.device)
        base0 = store.dev.data_ptr()
        tabs = (T * len(shapes))(*[T(base0 + 4 * o, rows, n, n_vals * j) for j, ((rows, n), o) in enumerate(zip(shapes, store.offs))])
        plan = ctypes.c_void_p()
        _ffi.check(lib.dfq_batch_error_plan_create(tabs, len(shapes), cfgs, len(configs), store.bases, n_nets, out.data_ptr(),
                                                   n_vals * len(shapes) + 1, ctypes.byref(plan)))
        _ffi.check(lib.dfq_batch_error_plan_run(plan, _ffi.stream_arg()))
        _ffi.synchronize()
        lib.dfq_batch_error_plan_destroy(plan)
        return _host(out)
    want = None
    for name, word in WORDS.items():
        rng = np.random.default_rng(3)
        planted = _piece_tensors(place, word, LOW, order, rng)
        clean = [rng.standard_normal(x.shape).astype(F32) for x in planted]       # (the same values for every word)
        if want is None:
            alone = _Store([clean])
            alone.to(engine)
            want = run(alone, 1)
        both = _Store([planted, clean])
        both.to(engine)
        got = run(both, 2)
        assert np.isnan(got[0, :-1]).all(), '{} {} {}'.format(place, order, name)      # every tensor of network 0 holds a NaN
        assert np.isfinite(want[0, :-1]).all() and (got[:, -1] == 9.0).all()
        assert np.array_equal(got[1].view(np.int64), want[0].view(np.int64)), '{} {} {}: the clean network'.format(place, order, name)


# ---- the single-network kernels: one wave per row, one thread per channel -----------------------------------------------------------
@pytest.mark.parametrize('order', ORDERS)
@pytest.mark.parametrize('name', list(WORDS))
def test_single_network_sites(engine, name, order):
    lib = _ffi.lib()
    word = WORDS[name]
    rng = np.random.default_rng(4)
    x = rng.standard_normal((4, 130)).astype(F32)                       # lane 1 folds elements 1, 65, 129
    _put(x[0], 1, 65, LOW, word, order)
    _put(x[1], 65, 129, HIGH, word, order)
    _fill(x[2], word)
    want = _row_ranges(x)
    what = '{} {}'.format(name, order)
    xd = _dev(engine, x)
    assert_bitexact(_host(_row_quant(lib, xd, 8, 0)[2]), want, what + ': dfq_row_quant_plan_run')
    assert_bitexact(_host(prims.fake_quant_rows(xd, 8, return_codes=True)[2]), want, what + ': dfq_fake_quant_rows')
    with np.errstate(invalid='ignore'):
        assert_bitexact(_host(prims.row_range(xd, signed=False)), want[:, 1] - want[:, 0], what + ': dfq_row_range')
        assert_bitexact(_host(prims.row_range(xd, signed=True)), np.maximum(want[:, 1], -want[:, 0]) + F32(0.0), what + ': dfq_row_range signed')
    assert_bitexact(_host(q.tensor_minmax(xd[:2])), _tensor_range(x[:2]), what + ': dfq_tensor_minmax')
    # the second layer's input channels: a thread folds the taps of a (row, channel) one after another
    w2 = rng.standard_normal((4, 6, 3, 3)).astype(F32)
    _put(w2[1, 0], 3, 4, LOW, word, order)
    _put(w2[2, 1], 7, 8, HIGH, word, order)
    _fill(w2[:, 2], word)
    cols = np.array([_range(w2[:, c]) for c in range(6)], dtype=F32)
    with np.errstate(invalid='ignore'):
        assert_bitexact(_host(prims.col_range(_dev(engine, w2), 6, signed=False)), cols[:, 1] - cols[:, 0], what + ': dfq_col_range')
        assert_bitexact(_host(prims.col_range(_dev(engine, w2), 6, signed=True)), np.maximum(cols[:, 1], -cols[:, 0]) + F32(0.0),
                        what + ': dfq_col_range signed')


@pytest.mark.parametrize('order', ORDERS)
def test_bc_row_range(engine, monkeypatch, order):
    """bc_row_range_kernel through the per-channel bias correction: the materialised row sums of eps (DFQ_BC_EPS=1) of a row
    holding a NaN are those of the row's NaN-skipping range wherever the NaN itself is not part of the sum."""
    from oracle import dfq_oracle as orc
    monkeypatch.setenv('DFQ_BC_EPS', '1')
    model, graph, bottoms = synthetic.build('tiny_wide', seed=0)
    model.to(engine.device)
    lt.merge_batchnorm(model, graph, bottoms, TARG)
    for m in graph.values():
        if type(m) in TARG and m.bias is None:
            lt._ensure_bias(m)
    plan, keys = dfq.build_bc_plan(graph, bottoms, TARG)
    step, layer = next((s, graph[k]) for s, k in enumerate(keys) if graph[k].weight[0].numel() >= 130)
    clean = _host(layer.weight).astype(F32).copy()
    for name, word in WORDS.items():
        w = clean.copy()
        _put(w[0], 1, 65, LOW, word, order)                             # lane 1 of the row's wave folds elements 1, 65, 129
        _put(w[1], 65, 129, HIGH, word, order)
        with torch.no_grad():
            layer.weight.copy_(_dev(engine, w))
        plan.run(check=False, per_channel=True, bits=8)                 # (the weights are only read; eps does not depend on the biases)
        _ffi.synchronize()
        got = _host(plan.eps(step))
        for o in (0, 1, 2):
            r = w[o]
            mn, mx = _range(r)
            with np.errstate(invalid='ignore'):
                e = (orc.uniform_quantize(r, 8, float(mn), float(mx), False) - r).astype(F32).reshape(r.shape[0], -1)
            acc = np.zeros(e.shape[0], dtype=F32)
            for k in range(e.shape[1]):
                acc = (acc + e[:, k]).astype(F32)
            assert np.isnan(acc).sum() == (1 if o < 2 else 0)
            assert_bitexact(got[o].reshape(-1), acc, '{} {}: eps of row {}'.format(name, order, o))
    plan.close()
