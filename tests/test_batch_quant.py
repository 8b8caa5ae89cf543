"""NetworkBatch.quant_plan / dfq_batch_quant_plan_*: quantize_targ_layer for every network of a batch in one plan.

Every weight, bias, integer code and range must be bit-identical to what the per-network path writes for the same network
(dfq_quant_plan_run per tensor, dfq_row_quant_plan_run per row); networks of a batch must not see each other.

Floats are compared as bit patterns (_same), so a zero of the other sign is a difference.  On the MI355X that holds exactly:
v_min_f32 / v_max_f32 order -0 below +0, so a min / max does not depend on the order it was folded in.  The CPU emulation's
min / max (fminf / fmaxf of the C library) return the second operand on a tie of -0 and +0, so there the sign of a zero
extreme depends on the fold order -- of the per-network kernels as much as of the batch kernels -- and the emulation
compares with the sign of zero ignored."""
import ctypes

import numpy as np
import pytest
import torch

from dfq_amd import _ffi, arena, dfq, synthetic
from dfq_amd.utils import layer_transform as lt
from dfq_amd.utils import relation as rel

from common import TARG

DFQ_ERR_ARG = -1     # include/dfq_hip.h


def _prepared(name, seed, device):
    model, graph, bottoms = synthetic.build(name, seed=seed)
    model.to(device)
    lt.merge_batchnorm(model, graph, bottoms, TARG)
    rels = rel.create_relation(graph, bottoms, TARG, delete_single=False)
    return model, graph, bottoms, rels


def _targ(graph):
    return [(k, m) for k, m in graph.items() if type(m) in TARG]


def _match_biases(g_batch, g_twin):
    """the batch gives every layer it corrects or equalises a bias (dfq.py:91-92); so does the per-network pipeline"""
    for (k, m), (_, t) in zip(_targ(g_batch), _targ(g_twin)):
        if m.bias is not None and t.bias is None:
            lt._ensure_bias(t)


def _expect(g_twin, bw, bb, per_channel, signed):
    """quantize_targ_layer on a twin: (weights, biases, codes, ranges) as the per-network path leaves them"""
    pre = {k: (m.weight.detach().clone(), None if m.bias is None else m.bias.detach().clone()) for k, m in _targ(g_twin)}
    out = lt.quantize_targ_layer(g_twin, bw, bb, TARG, return_codes=True, per_channel=per_channel, signed=signed)
    codes = out[1]
    ranges = {}
    for k, (w, b) in pre.items():
        ranges[k] = out[2][k] if per_channel else torch.stack([w.min(), w.max()])
        if b is not None and bb < 32:
            ranges[k + '.bias'] = torch.stack([b.min(), b.max()])
    return codes, ranges


def _same(a, b, exact):
    """bit-identical float32 tensors (exact=False: up to the sign of zeros, see the module docstring)"""
    a, b = a.detach().contiguous(), b.detach().contiguous().to(a.device)
    if a.shape != b.shape or a.dtype != torch.float32 or b.dtype != torch.float32:
        return False
    if not exact:
        a, b = a + 0.0, b + 0.0                       # -0 -> +0, every other value unchanged
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _compare(g, g_twin, codes, ranges, want_codes, want_ranges, what, exact):
    for (k, m), (_, t) in zip(_targ(g), _targ(g_twin)):
        assert _same(m.weight, t.weight, exact), '{} {}: weight'.format(what, k)
        assert (m.bias is None) == (t.bias is None)
        if m.bias is not None:
            assert _same(m.bias, t.bias, exact), '{} {}: bias'.format(what, k)
        if codes is not None:
            assert codes[k].shape == want_codes[k].shape
            assert torch.equal(codes[k].to(torch.int64), want_codes[k].to(torch.int64)), '{} {}: codes'.format(what, k)
    assert sorted(ranges) == sorted(want_ranges), what
    for k in want_ranges:
        assert _same(ranges[k], want_ranges[k], exact), '{} {}: range'.format(what, k)


@pytest.mark.parametrize('name', ['tiny_mobile', 'tiny_res', 'tiny_cat'])
@pytest.mark.parametrize('per_channel', [False, True])
@pytest.mark.parametrize('signed', [False, True])
@pytest.mark.parametrize('bw,bb', [(8, 16), (4, 8), (8, 32)])
@pytest.mark.parametrize('codes', ['int8', 'int32'])
def test_batch_equals_per_network(engine, name, per_channel, signed, bw, bb, codes):
    seeds = [0, 1, 2, 3, 4]
    nets = [_prepared(name, s, engine.device) for s in seeds]
    twins = [_prepared(name, s, engine.device) for s in seeds]
    batch = arena.NetworkBatch([(g, b, r) for (_, g, b, r) in nets], TARG)
    plan = batch.quant_plan(bw, bb, per_channel=per_channel, signed=signed, codes=codes)
    plan.run()
    _ffi.synchronize()
    want_dtype = torch.int32 if codes == 'int32' else (torch.int8 if signed else torch.uint8)
    for n, ((_, g, _, _), (_, gt, _, _)) in enumerate(zip(nets, twins)):
        _match_biases(g, gt)
        wc, wr = _expect(gt, bw, bb, per_channel, signed)
        c = plan.codes(n)
        assert all(v.dtype == want_dtype for v in c.values())
        _compare(g, gt, c, plan.ranges(n), wc, wr, '{} net {}'.format(name, n), engine.kind == 'gpu')
    plan.close()


def test_full_pipeline(engine):
    seeds = [0, 1, 2]
    nets = [_prepared('tiny_mobile', s, engine.device) for s in seeds]
    twins = [_prepared('tiny_mobile', s, engine.device) for s in seeds]
    batch = arena.NetworkBatch([(g, b, r) for (_, g, b, r) in nets], TARG)
    le = batch.le_plan()
    le.run()
    le.close()
    bc = batch.bc_plan()
    bc.run(check=True)
    bc.close()
    codes, ranges = batch.quantize(8, 16, codes='int8')
    for n, ((_, g, _, _), (_, gt, bt, rt)) in enumerate(zip(nets, twins)):
        dfq.cross_layer_equalization(gt, rt, TARG)
        dfq.bias_correction(gt, bt, TARG)
        wc, wr = _expect(gt, 8, 16, False, False)
        _compare(g, gt, codes[n], ranges[n], wc, wr, 'pipeline net {}'.format(n), engine.kind == 'gpu')


@pytest.mark.parametrize('bits', [2, 16])
def test_tiny_wide(engine, bits):
    nets = [_prepared('tiny_wide', s, engine.device) for s in (0, 1, 2)]
    twins = [_prepared('tiny_wide', s, engine.device) for s in (0, 1, 2)]
    batch = arena.NetworkBatch([(g, b, r) for (_, g, b, r) in nets], TARG)
    for per_channel in (False, True):
        codes, ranges = batch.quantize(bits, bits, per_channel=per_channel, codes='int32' if bits > 8 else 'int8')
        for n, ((_, g, _, _), (_, gt, _, _)) in enumerate(zip(nets, twins)):
            _match_biases(g, gt)
            wc, wr = _expect(gt, bits, bits, per_channel, False)
            _compare(g, gt, codes[n], ranges[n], wc, wr, 'tiny_wide net {} per_channel={}'.format(n, per_channel),
                     engine.kind == 'gpu')


def test_networks_are_independent(engine):
    nets = [_prepared('tiny_res', s, engine.device) for s in range(5)]
    for per_channel in (False, True):
        k = 3
        alone = _prepared('tiny_res', k, engine.device)
        big = arena.NetworkBatch([(g, b, r) for (_, g, b, r) in nets], TARG)
        one = arena.NetworkBatch([alone[1:]], TARG)
        cb, rb = big.quantize(4, 8, per_channel=per_channel, signed=True, codes='int8')
        co, ro = one.quantize(4, 8, per_channel=per_channel, signed=True, codes='int8')
        _compare(nets[k][1], alone[1], cb[k], rb[k], co[0], ro[0], 'network {} of 5 vs alone'.format(k), engine.kind == 'gpu')
        big.release()
        one.release()
        nets = [_prepared('tiny_res', s, engine.device) for s in range(5)]


# ---- the C ABI on hand-made tensors ---------------------------------------------------------------------------------------

def _special_rows(x, rng):
    """constant rows, an all-negative row, rows of signed zeros"""
    rows, n = x.shape
    if rows > 1:
        x[1] = 0.37
    if rows > 2:
        x[2] = -rng.random(n) - 0.5
    if rows > 3:
        x[3] = 0.0
        x[3, ::2] = -0.0
    if rows > 4:
        x[4] = -0.0
    if rows > 5:
        x[5] = np.where(np.arange(n) % 3 == 0, -0.0, rng.standard_normal(n))
    return x


def _row_quant(lib, x, bits, sym):
    """dfq_row_quant_plan_run on a copy: (quantised, int32 codes, ranges)"""
    y = x.clone()
    c = torch.empty(y.shape, dtype=torch.int32, device=y.device)
    r = torch.empty((y.shape[0], 2), dtype=torch.float32, device=y.device)
    seg = (_ffi.DfqRowSegment * 1)(_ffi.DfqRowSegment(y.data_ptr(), y.shape[0], y.shape[1], bits, sym, c.data_ptr(), r.data_ptr()))
    plan = ctypes.c_void_p()
    _ffi.check(lib.dfq_row_quant_plan_create(seg, 1, ctypes.byref(plan)))
    _ffi.check(lib.dfq_row_quant_plan_run(plan, _ffi.stream_arg()))
    _ffi.synchronize()
    lib.dfq_row_quant_plan_destroy(plan)
    return y, c, r


def _tensor_quant(lib, x, bits, sym):
    """dfq_quant_plan_run on a copy: (quantised, int32 codes, (min, max))"""
    y = x.clone()
    c = torch.empty(y.shape, dtype=torch.int32, device=y.device)
    seg = (_ffi.DfqSegment * 1)(_ffi.DfqSegment(y.data_ptr(), y.numel(), bits, sym, c.data_ptr()))
    plan = ctypes.c_void_p()
    _ffi.check(lib.dfq_quant_plan_create(seg, 1, ctypes.byref(plan)))
    _ffi.check(lib.dfq_quant_plan_run(plan, _ffi.stream_arg()))
    _ffi.synchronize()
    lib.dfq_quant_plan_destroy(plan)
    return y, c, torch.stack([x.min(), x.max()])


@pytest.mark.parametrize('code_bytes', [1, 4])
def test_row_length_edges_through_the_abi(engine, code_bytes):
    lib = _ffi.lib()
    reg = int(lib.dfq_batch_quant_register_elements())
    assert reg >= 1280
    rng = np.random.default_rng(7)
    # (rows, row_len, bits, symmetric, per_row): every lane class, its edges, a row longer than the register budget, and
    # per-tensor tensors on both sides of that budget (the longest takes the two-launch path)
    shapes = [(7, n, 8, i % 2, 1) for i, n in enumerate([1, 3, 4, 5, 8, 9, 16, 17, 63, 64, 65, 320, 1280])]
    shapes += [(6, reg + 37, 2, 0, 1), (6, 33, 2, 1, 1), (9, 20, 16, 0, 1), (3, 100, 16, 1, 1)]
    shapes += [(1, 1, 8, 0, 0), (1, 9, 5, 1, 0), (4, 300, 8, 0, 0), (1, reg, 8, 1, 0), (3, reg, 16, 0, 0),
               (7, 1900, 2, 1, 0), (5, 17, 30, 0, 0)]
    n_nets = 3
    offs, total = [], 0
    for (r, n, _, _, _) in shapes:
        offs.append(total)
        total += -(-(r * n) // 64) * 64 + 64 * (len(offs) % 3)        # gaps between the tensors
    stride = total + 128
    store = torch.full((n_nets * stride,), 3.25, dtype=torch.float32)
    for k in range(n_nets):
        for (r, n, _, _, _), o in zip(shapes, offs):
            x = _special_rows(rng.standard_normal((r, n)).astype(np.float32) * (k + 1), rng)
            store[k * stride + o:k * stride + o + r * n] = torch.from_numpy(x.reshape(-1))
    store = store.to(engine.device)
    pristine = store.clone()
    code_dtype = torch.int32 if code_bytes == 4 else torch.uint8
    code_offs, rng_offs, cs, rs = [], [], 0, 0
    for (r, n, bits, _, per_row) in shapes:
        writes = code_bytes == 4 or bits <= 8
        code_offs.append(cs if writes else -1)
        cs += r * n if writes else 0
        rng_offs.append(rs)
        rs += 2 * (r if per_row else 1)
    code_stride, range_stride = cs + 3, rs + 1
    codes = torch.full((n_nets, code_stride), 77, dtype=code_dtype, device=engine.device)
    ranges = torch.full((n_nets, range_stride), 5.0, dtype=torch.float32, device=engine.device)
    base0 = store.data_ptr()
    tabs = (_ffi.DfqBatchQuantTensor * len(shapes))(*[
        _ffi.DfqBatchQuantTensor(base0 + 4 * o, r, n, bits, sym, per_row, 0, co, ro)
        for (r, n, bits, sym, per_row), o, co, ro in zip(shapes, offs, code_offs, rng_offs)])
    bases = (ctypes.c_void_p * n_nets)(*[base0 + 4 * k * stride for k in range(n_nets)])
    plan = ctypes.c_void_p()
    _ffi.check(lib.dfq_batch_quant_plan_create(tabs, len(shapes), bases, n_nets, codes.data_ptr(), code_bytes, code_stride,
                                               ranges.data_ptr(), range_stride, ctypes.byref(plan)))
    assert lib.dfq_batch_quant_plan_launches(plan) == 2
    _ffi.check(lib.dfq_batch_quant_plan_run(plan, _ffi.stream_arg()))
    _ffi.synchronize()
    lib.dfq_batch_quant_plan_destroy(plan)
    exact = engine.kind == 'gpu'
    for k in range(n_nets):
        for (r, n, bits, sym, per_row), o, co, ro in zip(shapes, offs, code_offs, rng_offs):
            what = 'net {} rows {} x {} bits {} sym {} per_row {}'.format(k, r, n, bits, sym, per_row)
            x = pristine[k * stride + o:k * stride + o + r * n].view(r, n)
            y, c, rg = (_row_quant if per_row else _tensor_quant)(lib, x, bits, sym)
            got = store[k * stride + o:k * stride + o + r * n].view(r, n)
            assert _same(got, y, exact), what
            if co >= 0:
                got_c = codes[k, co:co + r * n].view(r, n)
                if code_bytes == 1 and sym:
                    got_c = got_c.view(torch.int8)                       # symmetric 1-byte codes are int8
                assert torch.equal(got_c.to(torch.int64), c.to(torch.int64)), what
            assert _same(ranges[k, ro:ro + rg.numel()], rg.reshape(-1), exact), what
        # nothing outside the tensors was touched
        mask = torch.ones(stride, dtype=torch.bool)
        for (r, n, _, _, _), o in zip(shapes, offs):
            mask[o:o + r * n] = False
        mask = mask.to(engine.device)
        assert _same(store[k * stride:(k + 1) * stride][mask], pristine[k * stride:(k + 1) * stride][mask], True)
    assert (codes[:, -3:] == 77).all() and (ranges[:, -1:] == 5.0).all()


# ---- errors ----------------------------------------------------------------------------------------------------------------

def test_abi_rejects_bad_arguments(engine):
    lib = _ffi.lib()
    buf = torch.zeros(4 * 64, dtype=torch.float32, device=engine.device)
    codes = torch.zeros(1024, dtype=torch.int32, device=engine.device)
    ranges = torch.zeros(64, dtype=torch.float32, device=engine.device)
    bases = (ctypes.c_void_p * 2)(buf.data_ptr(), buf.data_ptr() + 4 * 128)

    def create(rows=4, row_len=16, bits=8, per_row=1, code_off=0, range_off=0, n_nets=2, b=bases, code_bytes=4,
               code_stride=256, range_stride=16, c=codes.data_ptr()):
        t = (_ffi.DfqBatchQuantTensor * 1)(_ffi.DfqBatchQuantTensor(buf.data_ptr(), rows, row_len, bits, 0, per_row, 0, code_off, range_off))
        plan = ctypes.c_void_p()
        rc = lib.dfq_batch_quant_plan_create(t, 1, b, n_nets, c, code_bytes, code_stride, ranges.data_ptr(), range_stride,
                                             ctypes.byref(plan))
        if rc == 0:
            lib.dfq_batch_quant_plan_destroy(plan)
        return rc

    assert create() == 0
    assert create(per_row=0, bits=30, range_stride=2) == 0
    bad = [dict(bits=1), dict(bits=17), dict(per_row=0, bits=0), dict(per_row=0, bits=31),
           dict(code_bytes=1, bits=9), dict(code_bytes=2), dict(n_nets=0), dict(n_nets=-1), dict(b=None),
           dict(b=(ctypes.c_void_p * 2)(buf.data_ptr(), None)), dict(code_off=193), dict(range_off=9), dict(range_off=-2),
           dict(c=None), dict(rows=0), dict(row_len=0), dict(code_stride=63)]
    for kw in bad:
        assert create(**kw) == DFQ_ERR_ARG, kw
        assert b'dfq_batch_quant_plan_create' in lib.dfq_last_error(), kw
    assert create(code_bytes=1, bits=8) == 0
    assert create(code_bytes=1, bits=9, code_off=-1) == 0            # no codes: any width
    rc = lib.dfq_batch_quant_plan_create(None, 0, bases, 2, None, 4, 0, None, 0, ctypes.byref(ctypes.c_void_p()))
    assert rc == DFQ_ERR_ARG
    assert lib.dfq_batch_quant_plan_run(None, None) == DFQ_ERR_ARG
    assert b'dfq_batch_quant_plan_run' in lib.dfq_last_error()


def test_quant_plan_rejects_bad_arguments(engine):
    nets = [_prepared('tiny_mobile', s, engine.device) for s in (0, 1)]
    batch = arena.NetworkBatch([(g, b, r) for (_, g, b, r) in nets], TARG)
    # what quantize_targ_layer would refuse (per tensor: inside the library, per channel: _quantize_targ_layer_rows)
    for kw in [dict(bit_weight=0), dict(bit_weight=31), dict(bit_weight='eight'), dict(bits_bias=31), dict(bits_bias=0),
               dict(bit_weight=1, per_channel=True), dict(bit_weight=17, per_channel=True), dict(bits_bias=17, per_channel=True),
               dict(bit_weight=8.0, per_channel=True), dict(bit_weight=True, per_channel=True),
               dict(bit_weight=9, codes='int8'), dict(codes='int16')]:
        with pytest.raises(ValueError):
            batch.quant_plan(**kw)
    batch.quant_plan(bit_weight=9, codes='int32').close()
    # ... and what it takes: per tensor a width through int(), the bias skipped from 32 bits on, also as a float
    p = batch.quant_plan(bit_weight=8.0, bits_bias=16.0, codes='int8')
    assert p.code_dtype is torch.uint8 and any(k.endswith('.bias') for k in p.ranges(0))
    p.close()
    for bb in (32, 32.0, 64):
        p = batch.quant_plan(bit_weight=8, bits_bias=bb, per_channel=bb == 64, codes='int8')
        assert not any(k.endswith('.bias') for k in p.ranges(0))
        p.close()
    plan = batch.quant_plan()
    assert plan.codes(0) == {}
    batch.release()
    with pytest.raises(RuntimeError, match='released'):
        batch.quant_plan()
    with pytest.raises(RuntimeError, match='released'):
        plan.run()
    plan.close()


@pytest.mark.parametrize('moved', ['weight', 'bias'])
def test_a_tensor_that_left_its_slot_is_refused(engine, moved):
    """network n is written at network 0's addresses moved by a fixed offset: a tensor of network 0 that no longer lives in
    the batch allocation would send every network's writes outside it.  check() looks at the first and last slots only."""
    nets = [_prepared('tiny_mobile', s, engine.device) for s in (0, 1, 2)]
    batch = arena.NetworkBatch([(g, b, r) for (_, g, b, r) in nets], TARG)
    layers = _targ(nets[0][1])
    _, mid = layers[len(layers) // 2]
    assert mid.bias is not None
    t = mid.weight if moved == 'weight' else mid.bias
    t.data = t.data.clone()                           # the misuse check() documents: a new tensor behind the parameter
    batch.check()                                     # (the quick check does not see a middle slot)
    before, moved_before = batch.storage.clone(), t.detach().clone()
    with pytest.raises(RuntimeError, match='no longer lives in its slot'):
        batch.quant_plan()
    with pytest.raises(RuntimeError, match='no longer lives in its slot'):
        batch.quantize(per_channel=True, codes='int8')
    _ffi.synchronize()
    assert _same(batch.storage, before, True) and _same(t, moved_before, True)      # nothing was written anywhere


def test_codes_and_ranges_outlive_the_plan(engine):
    nets = [_prepared('tiny_mobile', s, engine.device) for s in (0, 1)]
    batch = arena.NetworkBatch([(g, b, r) for (_, g, b, r) in nets], TARG)
    plan = batch.quant_plan(codes='int8')
    plan.run()
    _ffi.synchronize()
    c, r = plan.codes(1), plan.ranges(1)
    keep_c = {k: v.clone() for k, v in c.items()}
    plan.close()
    del plan
    for k in keep_c:
        assert torch.equal(c[k], keep_c[k])
    assert all(v.shape[-1] == 2 for v in r.values())


# ---- full size, on the MI355X -----------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize('per_channel', [False, True])
def test_batch_of_64_mobilenet_v2(per_channel):
    dev = torch.device('cuda', 0)
    nets = [_prepared('mobilenet_v2', s % 4, dev) for s in range(64)]
    batch = arena.NetworkBatch([(g, b, r) for (_, g, b, r) in nets], TARG)
    plan = batch.quant_plan(8, 16, per_channel=per_channel, codes='int8')
    plan.run()
    torch.cuda.synchronize()
    for n in (0, 17, 42, 63):
        _, gt, _, _ = _prepared('mobilenet_v2', n % 4, dev)
        _match_biases(nets[n][1], gt)
        wc, wr = _expect(gt, 8, 16, per_channel, False)
        _compare(nets[n][1], gt, plan.codes(n), plan.ranges(n), wc, wr, 'mobilenet_v2 net {}'.format(n), True)
    plan.close()
    batch.release()
