"""NetworkBatch.error_plan / quantize_error / dfq_batch_error_plan_*: the weight quantisation error of every network of a
batch under several quantiser configurations from one plan (the batch form of ``_quantize_error``, dfq.py:8-25).

The expected value of every sum is exact: e = Q(w) - w is formed in numpy from a numpy restatement of the recipe
(utils/quantize.py:49-74: the scalars in float64, each cast to float32 where torch casts a Python scalar; five separately
rounded float32 operations per element) on the same (min, max), and the sums are ``math.fsum`` of float64 terms (e^2 and w^2
as float64 products of float32 values, which are exact).  The plan adds the same terms in float64 in an order of its own, so
the tolerance is the bound of any-order recursive summation of n terms in a format of unit roundoff u = 2^-53,
|got - exact| <= n u sum|term| (Higham, Accuracy and Stability of Numerical Algorithms, (4.4) with (n - 1) u / (1 - (n - 1) u)
<= n u) -- for sum e the bound therefore uses sum|e|.  Nothing looser anywhere."""
import ctypes
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
TINY = ['tiny_mobile', 'tiny_res', 'tiny_cat', 'tiny_seg', 'tiny_head']
CONFIGS = ((8, False, False), (8, True, False), (8, False, True), (4, True, True))      # (bit_weight, per_channel, signed)


class _Gpu:
    kind, device = 'gpu', torch.device('cuda', 0)


# ---- the recipe in numpy -------------------------------------------------------------------------------------------------
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
    return F32(qmin), F32(qmax), F32(-mn), F32(scale), F32(mn)


def _epsilon(w, bits, per_channel, signed):
    """Q(w) - w, float32, for w [rows, row_len]; NaN is skipped by the ranges"""
    assert w.dtype == F32 and w.ndim == 2
    with np.errstate(all='ignore'):
        if per_channel:
            prm = [_qparams(np.nanmin(r) if not np.isnan(r).all() else np.nan, np.nanmax(r) if not np.isnan(r).all() else np.nan,
                            bits, signed) for r in w]
            qmin, qmax = prm[0][0], prm[0][1]
            neg_min, scale, min_value = (np.array([p[i] for p in prm], dtype=F32).reshape(-1, 1) for i in (2, 3, 4))
        else:
            nan = np.isnan(w).all()
            qmin, qmax, neg_min, scale, min_value = _qparams(np.nan if nan else np.nanmin(w), np.nan if nan else np.nanmax(w), bits, signed)
        q = w + neg_min
        q = q / scale
        q = np.where(q < qmin, qmin, q)
        q = np.where(q > qmax, qmax, q)
        q = np.rint(q)
        y = q * scale
        y = y + min_value
        e = y - w
    assert e.dtype == F32
    return e


def _fsum(a):
    return math.fsum(a.reshape(-1).tolist())


def _sums_of(e):
    """[(exact, bound)] of sum e, sum |e|, sum e^2 for a float32 array"""
    d = e.astype(np.float64).reshape(-1)
    n = d.size
    s_abs, s_sq = _fsum(np.abs(d)), _fsum(d * d)
    return [(_fsum(d), n * U * s_abs), (s_abs, n * U * s_abs), (s_sq, n * U * s_sq)]


def _expected(w, configs):
    """[(exact, bound)] of the 1 + 3 * len(configs) sums of one weight [rows, row_len]"""
    d = w.astype(np.float64).reshape(-1)
    s_w = _fsum(d * d)
    out = [(s_w, d.size * U * s_w)]
    for bits, per_channel, signed in configs:
        out += _sums_of(_epsilon(w, bits, per_channel, signed))
    return out


def _assert_sums(got, want, what):
    assert len(got) == len(want), what
    for i, (g, (exact, bound)) in enumerate(zip(got, want)):
        if math.isnan(exact):
            assert math.isnan(g), '{} value {}: {} for NaN'.format(what, i, g)
        else:
            assert abs(g - exact) <= bound, '{} value {}: {!r} against {!r}, off by {:.3e} > {:.3e}'.format(what, i, g, exact, abs(g - exact), bound)


def _flat(e):
    """errors(n)[key] as the 1 + 3 k values of the block"""
    out = [e['sum_sq_w']]
    for c in range(len(e['sum'])):
        out += [float(e['sum'][c]), float(e['sum_abs'][c]), float(e['sum_sq'][c])]
    return out


# ---- helpers -------------------------------------------------------------------------------------------------------------
def _prepared(name, seed, device):
    model, graph, bottoms = synthetic.build(name, seed=seed)
    model.to(device)
    lt.merge_batchnorm(model, graph, bottoms, TARG)
    return graph, bottoms, rel.create_relation(graph, bottoms, TARG, delete_single=False)


def _batch(name, seeds, engine):
    nets = [_prepared(name, s, engine.device) for s in seeds]
    return nets, arena.NetworkBatch(nets, TARG)


def _weights(graph):
    """{key: float32 [rows, row_len] host copy} of the targ_type weights"""
    return OrderedDict((k, m.weight.detach().cpu().numpy().reshape(m.weight.shape[0], -1).copy()) for k, m in graph.items() if type(m) in TARG)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int64 if t.dtype is torch.float64 else torch.int32)


def _run(batch, configs):
    plan = batch.error_plan(configs)
    plan.run()
    _ffi.synchronize()
    return plan


def _check_against_exact(plan, nets, configs, what):
    for n, (g, _, _) in enumerate(nets):
        got = plan.errors(n)
        ws = _weights(g)
        assert list(got.keys()) == list(ws.keys()) == plan.keys
        for k, w in ws.items():
            assert got[k]['numel'] == w.size
            assert got[k]['sum'].dtype == np.float64 and got[k]['sum'].shape == (len(configs),)
            _assert_sums(_flat(got[k]), _expected(w, configs), '{} net {} {}'.format(what, n, k))


# ---- 1. against an exact sum ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', TINY)
def test_sums_against_fsum(engine, name):
    nets, batch = _batch(name, [0, 1, 2], engine)
    plan = _run(batch, CONFIGS)
    assert plan.launches <= 4
    assert plan.n_nets == 3 and plan.n_tensors == len(plan.keys)
    assert plan.configs == [(8, False, False), (8, True, False), (8, False, True), (4, True, True)]
    assert plan.block.dtype is torch.float64
    _check_against_exact(plan, nets, CONFIGS, name)
    a, b = plan.errors(0), plan.errors(1)
    assert any(_flat(a[k]) != _flat(b[k]) for k in a)              # a plan that read network 0 for everybody would be seen
    plan.close()
    # the convenience form: the reference's 'sum' and 'mean', mse and SQNR from the sums of a plan of that one configuration,
    # which are the bits the plan of four holds for it (a configuration's sums do not depend on the others)
    res = batch.quantize_error(8, True, False)
    assert len(res) == 3
    for n in range(3):
        e = plan.errors(n)
        assert list(res[n].keys()) == plan.keys
        for k in plan.keys:
            r, numel = res[n][k], e[k]['numel']
            assert sorted(r) == ['mean', 'mse', 'sqnr_db', 'sum']
            assert r['sum'] == e[k]['sum_abs'][1] and r['mean'] == e[k]['sum'][1] / numel and r['mse'] == e[k]['sum_sq'][1] / numel
            assert r['sqnr_db'] == 10.0 * math.log10(e[k]['sum_sq_w'] / e[k]['sum_sq'][1])    # ... and inf where nothing is lost: a weight of zeros and ones under 1 bit
    w = nets[0][0][plan.keys[0]].weight
    with torch.no_grad():
        w.copy_((torch.arange(w.numel(), device=w.device) % 2).to(w.dtype).view(w.shape))
    r = batch.quantize_error(1, False, False)[0][plan.keys[0]]
    assert r['sum'] == 0.0 and r['mse'] == 0.0 and r['sqnr_db'] == math.inf


# ---- 2. the error is the production quantiser's ----------------------------------------------------------------------------
@pytest.mark.parametrize('config', [(8, False, False), (8, True, False), (4, True, True)])
def test_epsilon_is_what_quantize_stores(engine, config):
    bits, per_channel, signed = config
    nets, batch = _batch('tiny_mobile', [0, 1, 2], engine)
    twins, twin_batch = _batch('tiny_mobile', [0, 1, 2], engine)
    plan = _run(batch, (config,))
    w0 = [_weights(g) for g, _, _ in twins]
    twin_batch.quantize(bits, 16, per_channel, signed, codes=None)
    for n, (g, _, _) in enumerate(twins):
        got = plan.errors(n)
        for k, wq in _weights(g).items():
            e = wq - w0[n][k]
            assert e.dtype == F32
            _assert_sums(_flat(got[k])[1:], _sums_of(e), '{} net {} {}'.format(config, n, k))
    plan.close()


# ---- 3. / 4. weights untouched, determinism, independence -------------------------------------------------------------------
def test_weights_untouched_and_runs_bit_equal(engine):
    nets, batch = _batch('tiny_res', [0, 1, 2], engine)
    before = batch.storage.clone()
    plan = _run(batch, CONFIGS)
    first = plan.block.clone()
    assert torch.equal(_bits(batch.storage), _bits(before)), 'run() wrote into the batch allocation'
    plan.block.fill_(-1.0)
    plan.run()
    _ffi.synchronize()
    assert torch.equal(_bits(plan.block), _bits(first)), 'two runs differ'
    assert torch.equal(_bits(batch.storage), _bits(before))
    plan.close()
    assert torch.equal(_bits(plan.block), _bits(first))            # the block outlives the plan
    with pytest.raises(RuntimeError, match='closed'):
        plan.run()


@pytest.mark.parametrize('name', ['tiny_mobile', 'tiny_cat'])
def test_network_does_not_depend_on_the_batch(engine, name):
    _, three = _batch(name, [0, 1, 2], engine)
    _, one = _batch(name, [1], engine)
    p3, p1 = _run(three, CONFIGS), _run(one, CONFIGS)
    assert torch.equal(_bits(p3.block[1]), _bits(p1.block[0]))
    assert not torch.equal(_bits(p3.block[0]), _bits(p1.block[0]))
    p3.close()
    p1.close()


# ---- 5. agreement with the single-network function --------------------------------------------------------------------------
def test_agrees_with_quantize_error(engine):
    """``dfq._quantize_error(w, 8, 'sum' | 'mean')`` (dfq_quant_error, dfq_quant.hip) forms the same float32 e from the same
    (min, max) and adds (double)|e| or (double)e in float64: per lane, then wave_sum, then block_sum, then the at most
    kQerrPartials partials one after another -- another order of the same n terms.  With T = sum of the terms, A = sum|e| and
    u = 2^-53 both float64 results lie within n u A of T, so they differ by at most 2 n u A.  It then returns
    float32(t / denom) with denom = 1 ('sum') or n ('mean'); here a = S / denom is formed the same way from the plan's S.
    The float64 division rounds once on either side, |a' - b'| <= 2 n u A / denom + u (|a'| + |b'|), and the roundings to
    float32 add at most 2^-24 |a'| and 2^-24 |b'| (2^-150 each below the normal range):
        |float32(a') - float32(b')| <= 2 n u A / denom + (2^-24 + u) (|a'| + |b'|) + 2^-149."""
    nets, batch = _batch('tiny_mobile', [0, 1, 2], engine)
    plan = _run(batch, ((8, False, False),))
    for n, (g, _, _) in enumerate(nets):
        got = plan.errors(n)
        for k, m in g.items():
            if type(m) not in TARG:
                continue
            e = got[k]
            numel, A = e['numel'], float(e['sum_abs'][0])
            for red, mine, denom in (('sum', A, 1.0), ('mean', float(e['sum'][0]) / numel, float(numel))):
                single = dfq._quantize_error(m.weight, 8, red)
                assert single.dtype is torch.float32
                b32 = float(single.cpu())
                a32 = float(F32(mine))
                tol = 2 * numel * U * A / denom + (2.0 ** -24 + U) * (abs(mine) + abs(b32)) + 2.0 ** -149
                assert abs(a32 - b32) <= tol, 'net {} {} {}: {!r} against {!r} (tolerance {:.3e})'.format(n, k, red, a32, b32, tol)
    plan.close()


# ---- 6. geometry through the raw ABI ----------------------------------------------------------------------------------------
# (rows, row_len): rows of 1 (fewer and more than the rows staged at a time, and than a piece holds), of 3, 9 and 27; a row
# of exactly a piece (4096 floats) and one of 4097; 5 elements; three pieces whose row boundaries fall on the piece
# boundaries; rows longer than a piece that do not; a constant tensor; a tensor of NaN in front of a clean one
SHAPES = [(7, 1), (5000, 1), (11, 3), (37, 9), (16, 27), (2, 4096), (2, 4097), (1, 5), (6, 2048), (3, 5000), (130, 96), (3, 10), (4, 33),
          (5, 33)]
CONSTANT, ALL_NAN = 11, 12


@pytest.mark.parametrize('n_nets', [1, 3])
def test_geometry_through_the_abi(engine, n_nets):
    lib = _ffi.lib()
    rng = np.random.default_rng(11)
    offs, total = [], 0
    for j, (r, n) in enumerate(SHAPES):
        offs.append(total)
        total += -(-(r * n) // 4) * 4 + 4 * (j % 3)                   # 16-byte aligned, with gaps of 0, 4 or 8 floats
    stride = total + 8
    host = np.full((n_nets, stride), 7.5e5, dtype=np.float32)        # a gap that leaks into a tensor shows in its range
    xs = []
    for k in range(n_nets):
        xs.append([])
        gen = np.random.default_rng(100 + k) if k != 1 else np.random.default_rng(100)     # network 1 repeats network 0 ...
        for j, ((r, n), o) in enumerate(zip(SHAPES, offs)):
            x = (gen.standard_normal((r, n)) * (1 + j % 3)).astype(np.float32)
            if j == CONSTANT:
                x[:] = 0.25
            elif j == ALL_NAN:
                x[:] = np.nan
            elif r > 2:
                x[1, :] = -1.5                                        # a constant row
                x[2, 0], x[r - 1, n - 1] = 9.0, -11.0                 # the extrema in the first and the last element of a row
            host[k, o:o + r * n] = x.reshape(-1)
            xs[k].append(x)
    store = torch.from_numpy(host).to(engine.device).contiguous()
    pristine = store.clone()
    n_vals = 1 + 3 * len(CONFIGS)
    s = (n_vals + 2) * len(SHAPES) + 1                                # two doubles between the tensors' sums
    out = torch.full((n_nets, s), 9.0, dtype=torch.float64, device=engine.device)
    base0 = store.data_ptr()
    T, C = _ffi.DfqBatchErrorTensor, _ffi.DfqBatchErrorConfig
    tabs = (T * len(SHAPES))(*[T(base0 + 4 * o, r, n, 1 + (n_vals + 2) * j) for j, ((r, n), o) in enumerate(zip(SHAPES, offs))])
    cfgs = (C * len(CONFIGS))(*[C(b, int(sg), int(pc), 0) for b, pc, sg in CONFIGS])
    bases = (ctypes.c_void_p * n_nets)(*[base0 + 4 * k * stride for k in range(n_nets)])
    plan = ctypes.c_void_p()
    _ffi.check(lib.dfq_batch_error_plan_create(tabs, len(SHAPES), cfgs, len(CONFIGS), bases, n_nets, out.data_ptr(), s, ctypes.byref(plan)))
    try:
        assert lib.dfq_batch_error_plan_launches(plan) <= 4
        _ffi.check(lib.dfq_batch_error_plan_run(plan, _ffi.stream_arg()))
        _ffi.synchronize()
        first = out.clone()
        _ffi.check(lib.dfq_batch_error_plan_run(plan, _ffi.stream_arg()))
        _ffi.synchronize()
    finally:
        lib.dfq_batch_error_plan_destroy(plan)
    assert torch.equal(_bits(out), _bits(first)), 'two runs differ'
    assert torch.equal(_bits(store), _bits(pristine)), 'run() wrote into the weights'
    got = out.cpu().numpy()
    want0 = None
    for k in range(n_nets):
        used = np.zeros(s, dtype=bool)
        want = [_expected(x, CONFIGS) for x in xs[k]] if k != 1 else want0
        want0 = want0 or want
        for j, (r, n) in enumerate(SHAPES):
            o = 1 + (n_vals + 2) * j
            vals = got[k, o:o + n_vals].tolist()
            if j == ALL_NAN:
                assert all(math.isnan(v) for v in vals), 'net {} rows {} x {}: {}'.format(k, r, n, vals)
            else:
                _assert_sums(vals, want[j], 'net {} rows {} x {}'.format(k, r, n))
            used[o:o + n_vals] = True
        assert (got[k][~used] == 9.0).all()                           # nothing else in the block is touched
    if n_nets > 1:
        assert np.array_equal(got[0].view(np.int64), got[1].view(np.int64))        # ... and gets the same bits at another place


# ---- 7. argument errors -----------------------------------------------------------------------------------------------------
def test_abi_rejects_bad_arguments(engine):
    lib = _ffi.lib()
    buf = torch.zeros(1024, dtype=torch.float32, device=engine.device)
    out = torch.zeros(2 * 64, dtype=torch.float64, device=engine.device)
    p0 = buf.data_ptr()
    bases = (ctypes.c_void_p * 2)(p0, p0 + 4 * 512)
    T, C = _ffi.DfqBatchErrorTensor, _ffi.DfqBatchErrorConfig

    def create(data=p0, rows=8, row_len=9, out_off=0, cfg=((8, 0, 0),), n_configs=None, b=bases, n_nets=2, o=out.data_ptr(), stride=64,
               n_tensors=1, table=True, place=True):
        plan = ctypes.c_void_p()
        cf = (C * len(cfg))(*[C(nb, sy, pr, 0) for nb, sy, pr in cfg]) if cfg else None
        rc = lib.dfq_batch_error_plan_create((T * 1)(T(data, rows, row_len, out_off)) if table else None, n_tensors, cf,
                                             len(cfg) if n_configs is None else n_configs, b, n_nets, o, stride,
                                             ctypes.byref(plan) if place else None)
        n = lib.dfq_batch_error_plan_launches(plan) if rc == 0 else None
        if rc == 0:
            lib.dfq_batch_error_plan_destroy(plan)
        return rc, n
    assert create() == (0, 3)
    assert create(out_off=60) == (0, 3)                               # the last four doubles of the stride
    assert create(cfg=((8, 0, 0),) * 4, out_off=51) == (0, 3)
    assert create(cfg=((2, 1, 1), (16, 0, 1), (1, 0, 0), (30, 1, 0))) == (0, 3)
    assert create(data=p0 + 16) == (0, 3)
    bad = [dict(table=False), dict(n_tensors=0), dict(n_tensors=-1), dict(place=False), dict(data=None), dict(rows=0), dict(rows=-3),
           dict(row_len=0), dict(row_len=-1), dict(data=p0 + 4), dict(data=p0 + 8), dict(out_off=-1), dict(out_off=61), dict(out_off=64),
           dict(out_off=1 << 40), dict(cfg=((8, 0, 0),) * 4, out_off=52), dict(o=None), dict(stride=0), dict(stride=-5), dict(stride=3),
           dict(cfg=None, n_configs=1), dict(n_configs=0), dict(n_configs=-1), dict(cfg=((8, 0, 0),) * 5),
           dict(cfg=((1, 0, 1),)), dict(cfg=((17, 0, 1),)), dict(cfg=((0, 0, 0),)), dict(cfg=((31, 0, 0),)), dict(cfg=((-8, 0, 0),)),
           dict(cfg=((1, 1, 0),)), dict(cfg=((8, 0, 0), (1, 1, 1))),
           dict(b=None), dict(n_nets=0), dict(n_nets=-1), dict(b=(ctypes.c_void_p * 2)(p0, None)),
           dict(b=(ctypes.c_void_p * 2)(p0, p0 + 4 * 511)), dict(rows=1 << 40, row_len=1 << 40)]
    for kw in bad:
        assert create(**kw)[0] == DFQ_ERR_ARG, kw
        assert b'dfq_batch_error_plan_create' in lib.dfq_last_error(), kw
    assert lib.dfq_batch_error_plan_run(None, None) == DFQ_ERR_ARG
    assert b'dfq_batch_error_plan_run' in lib.dfq_last_error()
    assert lib.dfq_batch_error_plan_launches(None) == 0
    lib.dfq_batch_error_plan_destroy(None)


def test_refusals(engine):
    nets, batch = _batch('tiny_mobile', [0, 1], engine)
    for bad in ((), ((8, False, False),) * 5, ((8, False),), 8, ((1, True, False),), ((17, True, False),), ((8.0, True, False),),
                ((0, False, False),), ((31, False, False),), (('x', False, False),), ((1, False, True),), ((8, False, False), (1, True, True))):
        with pytest.raises(ValueError):
            batch.error_plan(bad)
    with pytest.raises(ValueError):
        batch.quantize_error(1, True)
    plan = batch.error_plan(((8.0, False, False),))                   # per tensor through int(), as quant_plan
    assert plan.configs == [(8, False, False)]
    plan.close()
    # a weight that left its slot (not the first layer's: the batch's own quick check watches that one)
    g0 = nets[0][0]
    keys = [k for k in g0 if type(g0[k]) in TARG]
    layer = g0[keys[1]]
    kept = layer.weight.data
    layer.weight.data = kept.clone()
    with pytest.raises(RuntimeError, match='weight of {} '.format(keys[1])):
        batch.error_plan()
    with pytest.raises(RuntimeError, match='weight of {} '.format(keys[1])):
        batch.quantize_error()
    layer.weight.data = kept
    plan = batch.error_plan()
    batch.release()
    with pytest.raises(RuntimeError, match='released'):
        plan.run()
    with pytest.raises(RuntimeError, match='released'):
        batch.error_plan()
    plan.close()
    plan.close()


def test_unfolded_batch_is_refused(engine):
    nets = []
    for seed in (0, 1):
        model, graph, bottoms = synthetic.build('tiny_mobile', seed=seed)
        model.to(engine.device)
        nets.append((graph, bottoms, rel.create_relation(graph, bottoms, TARG, delete_single=False)))
    batch = arena.NetworkBatch.from_unfolded(nets, TARG)
    with pytest.raises(RuntimeError, match='not been folded'):
        batch.error_plan()
    with pytest.raises(RuntimeError, match='not been folded'):
        batch.quantize_error()
    batch.merge_batchnorm()
    plan = _run(batch, ((8, False, False), (8, True, False)))
    _check_against_exact(plan, nets, ((8, False, False), (8, True, False)), 'folded by the batch')
    plan.close()


def test_struct_layout_matches_header():
    src = r'''
    #include <stdio.h>
    #include <stddef.h>
    #include "dfq_hip.h"
    int main(void) {
        printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(dfq_batch_error_tensor), offsetof(dfq_batch_error_tensor, data),
               offsetof(dfq_batch_error_tensor, rows), offsetof(dfq_batch_error_tensor, row_len),
               offsetof(dfq_batch_error_tensor, out_offset), sizeof(dfq_batch_error_config), offsetof(dfq_batch_error_config, num_bits),
               offsetof(dfq_batch_error_config, symmetric), offsetof(dfq_batch_error_config, per_row), offsetof(dfq_batch_error_config, pad));
        return 0;
    }'''
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, 't.c')
        open(c, 'w').write(src)
        exe = os.path.join(d, 't')
        subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), c, '-o', exe], check=True)
        got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    P, Q = _ffi.DfqBatchErrorTensor, _ffi.DfqBatchErrorConfig
    assert got == [ctypes.sizeof(P), P.data.offset, P.rows.offset, P.row_len.offset, P.out_offset.offset,
                   ctypes.sizeof(Q), Q.num_bits.offset, Q.symmetric.offset, Q.per_row.offset, Q.pad.offset]


# ---- 8. full size, on the GPU -----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('name', ['mobilenet_v2', 'resnet18'])
def test_big_networks_against_fsum(name):
    assert torch.cuda.is_available(), 'gpu-marked test needs a ROCm GPU'
    _ffi.lib()
    configs = ((8, False, False), (8, True, False))
    nets, batch = _batch(name, [0, 1], _Gpu())
    plan = _run(batch, configs)
    assert plan.launches <= 4
    _check_against_exact(plan, nets, configs, name)
    plan.close()
    torch.cuda.synchronize()
