"""NetworkBatch.from_unfolded / fold_plan / dfq_batch_fold_plan_*: merge_batchnorm for every network of a batch in one plan.

Every folded weight and bias, the proxies ``fake_weight`` / ``fake_bias`` and the four BatchNorm vectors must be bit-identical
to what ``lt.merge_batchnorm`` leaves on a twin of that network alone; networks of a batch must not see each other.  Floats
are compared as bit patterns (a zero of the other sign is a difference), on the CPU emulation and on the MI355X alike:
nothing here reduces, so both engines are held to the same standard."""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch
import torch.nn as nn

from dfq_amd import _ffi, arena, synthetic
from dfq_amd.utils import layer_transform as lt
from dfq_amd.utils import relation as rel

from common import TARG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DFQ_ERR_ARG = -1     # include/dfq_hip.h
ARCHS = ['tiny_mobile', 'tiny_res', 'tiny_cat', 'tiny_seg', 'tiny_head']
SYNTHETIC = ARCHS + ['tiny_wide', 'tiny_tail']
CLIP = (-0.4, 0.25)
BN_VECTORS = ('weight', 'bias', 'running_mean', 'running_var')


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and torch.equal(_bits(a), _bits(b.to(a.device)))


def _plant(graph, bottoms, seed):
    """what the draw of synthetic.init_weights never gives: a negative and a zero gamma, running variances at and next to 0
    (in the first and the last folded BatchNorm), and a folded layer with a bias of its own that is not zero"""
    pairs = lt._fold_pairs(graph, bottoms, TARG)
    gen = torch.Generator(device='cpu')
    gen.manual_seed(1000 + seed)
    with torch.no_grad():
        for (_, bk), at in ((pairs[0], 0), (pairs[-1], 1)):
            bn = graph[bk]
            assert bn.num_features >= 6
            bn.weight[at] = -0.75
            bn.weight[at + 2] = 0.0
            bn.running_var[at + 1] = 0.0
            bn.running_var[at + 3] = 1e-9
        layer = graph[pairs[1][0]]
        if layer.bias is None:
            layer.bias = nn.Parameter(torch.randn(layer.weight.shape[0], generator=gen) * 0.1)
        else:
            layer.bias.copy_(torch.randn(layer.weight.shape[0], generator=gen) * 0.1)


def _unfolded(name, seed, device):
    """(model, graph, bottoms, relations) as loaded: nothing folded; a function of (name, seed) alone"""
    model, graph, bottoms = synthetic.build(name, seed=seed)
    _plant(graph, bottoms, seed)
    model.to(device)
    return model, graph, bottoms, rel.create_relation(graph, bottoms, TARG, delete_single=False)


def _state(graph):
    """{name: tensor} of everything a fold may touch"""
    out = {}
    for k, m in graph.items():
        if type(m) in TARG:
            out[k + '.weight'] = m.weight
            if m.bias is not None:
                out[k + '.bias'] = m.bias
        elif type(m) == nn.BatchNorm2d:
            for name in BN_VECTORS + ('fake_weight', 'fake_bias'):
                t = getattr(m, name, None)
                if t is not None:
                    out[k + '.' + name] = t
    return out


def _assert_equal(graph, gt, what):
    a, b = _state(graph), _state(gt)
    assert sorted(a) == sorted(b), what
    for k in a:
        assert _same(a[k], b[k]), '{}: {}'.format(what, k)


def _old_walk(graph, bottoms, targ_type):
    """the loop merge_batchnorm held inline before ``_fold_pairs`` was factored out of it, restated"""
    pairs = []
    for key in graph:
        bots = bottoms[key]
        if bots is None:
            continue
        bn = graph[key]
        if type(bn) != nn.BatchNorm2d:
            continue
        for bk in bots:
            layer = graph[bk]
            if type(layer) not in targ_type:
                continue
            pairs.append((bk, key))
            break
    return pairs


# ---- 1. the batch equals the per-network function --------------------------------------------------------------------------

@pytest.mark.parametrize('name', ARCHS)
def test_batch_equals_per_network(engine, name):
    seeds = [0, 1, 2, 3]
    nets = [_unfolded(name, s, engine.device) for s in seeds]
    twins = [_unfolded(name, s, engine.device) for s in seeds]
    untouched = []
    for n, (_, g, b, _) in enumerate(nets):                # the case bites, in every network
        pairs = lt._fold_pairs(g, b, TARG)
        layers = [lk for lk, _ in pairs]
        own = [lk for lk in layers if g[lk].bias is not None]
        assert any(bool((g[lk].bias != 0).any()) for lk in own), 'net {}: no folded layer with a bias of its own'.format(n)
        assert any(g[lk].bias is None for lk in layers), 'net {}: no folded layer gets its bias from _ensure_bias'.format(n)
        gamma = torch.cat([g[bk].weight.detach() for _, bk in pairs])
        var = torch.cat([g[bk].running_var.detach() for _, bk in pairs])
        assert bool((gamma < 0).any()) and bool((gamma == 0).any()) and bool((var.abs() <= 1e-8).any())
        plain = [k for k, m in g.items() if type(m) in TARG and k not in layers]
        assert plain, 'net {}: every layer has a BatchNorm behind it'.format(n)
        untouched.append({k: (g[k].weight.detach().clone(), None if g[k].bias is None else g[k].bias.detach().clone()) for k in plain})
    batch = arena.NetworkBatch.from_unfolded([(g, b, r) for (_, g, b, r) in nets], TARG)
    assert batch.folded is False
    plan = batch.fold_plan()
    assert plan.launches <= 2 and plan.n_nets == len(seeds) and plan.n_pairs == len(lt._fold_pairs(nets[0][1], nets[0][2], TARG))
    assert plan.elements == sum(nets[0][1][lk].weight.numel() for lk, _ in lt._fold_pairs(nets[0][1], nets[0][2], TARG))
    plan.close()
    batch.merge_batchnorm()                                # ONE run for all networks, then everything is compared
    assert batch.folded is True
    for n, ((_, g, b, _), (mt, gt, bt, _)) in enumerate(zip(nets, twins)):
        lt.merge_batchnorm(mt, gt, bt, TARG)
        _assert_equal(g, gt, '{} net {}'.format(name, n))
        folded = [bk for _, bk in lt._fold_pairs(g, b, TARG)]
        for bk in folded:
            bn = g[bk]
            assert bn.eps == 1e-12 == gt[bk].eps
            assert bool((bn.weight == 1).all()) and bool((bn.running_var == 1).all())
            assert bool((_bits(bn.bias) == 0).all()) and bool((_bits(bn.running_mean) == 0).all())
        assert any(bool((g[bk].fake_weight == 0.75).any()) for bk in folded)           # |gamma| of the planted -0.75
        for k, (w, bias) in untouched[n].items():
            assert _same(g[k].weight, w), '{} net {}: {} has no BatchNorm behind it and changed'.format(name, n, k)
            assert (g[k].bias is None) == (bias is None) and (bias is None or _same(g[k].bias, bias))
    batch.release()


def test_networks_are_independent(engine):
    runs = []
    for bump in (False, True):
        nets = [_unfolded('tiny_res', s, engine.device) for s in (0, 1, 2)]
        if bump:
            with torch.no_grad():
                g, b = nets[1][1], nets[1][2]
                for _, bk in lt._fold_pairs(g, b, TARG):
                    g[bk].weight += 0.5
        batch = arena.NetworkBatch.from_unfolded([(g, b, r) for (_, g, b, r) in nets], TARG)
        batch.merge_batchnorm()
        runs.append([{k: v.detach().clone() for k, v in _state(g).items()} for (_, g, _, _) in nets])
        batch.release()
    for n in (0, 2):
        assert all(_same(runs[0][n][k], runs[1][n][k]) for k in runs[0][n]), n
    assert not all(_same(runs[0][1][k], runs[1][1][k]) for k in runs[0][1] if k.endswith('.weight'))


# ---- 2. the layout is the constructor's --------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['tiny_mobile', 'tiny_res', 'tiny_cat'])
def test_layout_is_the_constructors(engine, name):
    seeds = [0, 1, 2]
    nets = [_unfolded(name, s, engine.device) for s in seeds]
    twins = [_unfolded(name, s, engine.device) for s in seeds]
    new = arena.NetworkBatch.from_unfolded([(g, b, r) for (_, g, b, r) in nets], TARG)
    new.merge_batchnorm()
    for (mt, gt, bt, _) in twins:
        lt.merge_batchnorm(mt, gt, bt, TARG)
    old = arena.NetworkBatch([(g, b, r) for (_, g, b, r) in twins], TARG)
    assert old.folded is True and new.folded is True
    assert new.slots_per_network > old.slots_per_network
    assert list(new.offsets[:old.slots_per_network]) == list(old.offsets)
    results = []
    for batch in (new, old):
        le = batch.le_plan()
        le.run()
        le.close()
        _ffi.synchronize()
        batch.absorb(N=0.5, range_clip=CLIP)
        bc = batch.bc_plan()
        bc.run(check=True)
        _ffi.synchronize()
        bc.close()
        codes, ranges = batch.quantize()
        act = batch.set_quant_minmax()
        results.append((codes, ranges, [act.ranges(n) for n in range(len(seeds))]))
    (codes_a, ranges_a, act_a), (codes_b, ranges_b, act_b) = results
    for n, ((_, g, _, r), (_, gt, _, rt)) in enumerate(zip(nets, twins)):
        _assert_equal(g, gt, '{} net {}'.format(name, n))
        assert len(r) == len(rt) and all(_same(x.S, y.S) for x, y in zip(r, rt)), 'net {}: scale vectors'.format(n)
        assert sorted(codes_a[n]) == sorted(codes_b[n]) and codes_a[n]
        for k in codes_a[n]:
            assert torch.equal(codes_a[n][k], codes_b[n][k]), 'net {} {}: codes'.format(n, k)
        assert sorted(ranges_a[n]) == sorted(ranges_b[n]) and all(_same(ranges_a[n][k], ranges_b[n][k]) for k in ranges_a[n])
        assert list(act_a[n]) == list(act_b[n]) and act_a[n]
        for k in act_a[n]:
            xa, xb = act_a[n][k], act_b[n][k]
            if isinstance(xa, list):
                assert len(xa) == len(xb) and all(_same(p, q) for p, q in zip(xa, xb)), 'net {} {}: ranges'.format(n, k)
            else:
                assert _same(xa, xb), 'net {} {}: range'.format(n, k)


# ---- 3. row geometry at the C ABI ---------------------------------------------------------------------------------------

def _pad(n):
    return -(-n // 64) * 64


ROW_LENS = [1, 3, 9, 27, 64, 65, 1536, 1537, 5000, 70001]


def _rows_for(row_len):
    return 7 if row_len <= 65 else (3 if row_len <= 5000 else 2)


GEOMETRY = {'len{}'.format(L): [(_rows_for(L), L)] for L in ROW_LENS}
GEOMETRY['many_rows'] = [(70000, 1)]                       # more rows than a 16-bit grid dimension
GEOMETRY['one_row'] = [(1, 37)]
GEOMETRY['one_element'] = [(1, 1)]
GEOMETRY['mixed'] = [(_rows_for(L), L) for L in ROW_LENS] + [(70000, 1), (1, 37), (5, 4096), (1, 1), (300, 9)]
VECTORS = ('b', 'gamma', 'beta', 'mean', 'var', 'fw', 'fb')


@pytest.mark.parametrize('n_nets', [1, 3])
@pytest.mark.parametrize('case', sorted(GEOMETRY))
def test_row_geometry_through_the_abi(engine, case, n_nets):
    """hand-made pair tables over a flat buffer against dfq_fold_batchnorm on a copy of every network: rows shorter than a
    16-byte vector, rows longer than a piece, pieces and row sets that cross tensor boundaries"""
    lib = _ffi.lib()
    table = GEOMETRY[case]
    rng = np.random.default_rng(11)
    eps = 1e-5
    layout, stride = [], 0
    for (out_ch, row_len) in table:
        offs = {'w': (stride, out_ch * row_len)}
        stride += _pad(out_ch * row_len)
        for name in VECTORS:
            offs[name] = (stride, out_ch)
            stride += _pad(out_ch)
        layout.append(offs)
    host = rng.standard_normal((n_nets, stride)).astype(np.float32)
    for offs, (out_ch, _) in zip(layout, table):
        o, c = offs['var']
        host[:, o:o + c] = np.abs(host[:, o:o + c]) + 0.05
        host[:, o] = 0.0
        o, c = offs['gamma']
        host[:, o + c - 1] = 0.0
        if c > 2:
            host[:, o + 1] = -1.25
    buf = torch.from_numpy(host.copy()).to(engine.device)        # (on the CPU from_numpy shares the array's memory)
    ref = buf.clone()
    pairs = []
    for offs, (out_ch, row_len) in zip(layout, table):
        for n in range(n_nets):
            p = {k: ref[n, o:o + c].data_ptr() for k, (o, c) in offs.items()}
            _ffi.check(lib.dfq_fold_batchnorm(p['w'], p['b'], out_ch, row_len, p['gamma'], p['beta'], p['mean'], p['var'],
                                              ctypes.c_float(eps), p['fw'], p['fb'], _ffi.stream_arg()))
        a = {k: buf[0, o:o + c].data_ptr() for k, (o, c) in offs.items()}
        pairs.append(_ffi.DfqBatchFoldPair(a['w'], a['b'], a['gamma'], a['beta'], a['mean'], a['var'], a['fw'], a['fb'],
                                           row_len, out_ch, eps))
    bases = (ctypes.c_void_p * n_nets)(*[buf[n].data_ptr() for n in range(n_nets)])
    plan = ctypes.c_void_p()
    _ffi.check(lib.dfq_batch_fold_plan_create((_ffi.DfqBatchFoldPair * len(pairs))(*pairs), len(pairs), bases, n_nets,
                                              ctypes.byref(plan)))
    assert lib.dfq_batch_fold_plan_launches(plan) <= 2
    assert lib.dfq_batch_fold_plan_elements(plan) == sum(o * r for o, r in table)
    _ffi.check(lib.dfq_batch_fold_plan_run(plan, _ffi.stream_arg()))
    _ffi.synchronize()
    lib.dfq_batch_fold_plan_destroy(plan)
    for i, offs in enumerate(layout):
        for name, (o, c) in offs.items():
            for n in range(n_nets):
                assert _same(buf[n, o:o + c], ref[n, o:o + c]), '{} pair {} {} net {}'.format(case, i, name, n)
    assert _same(buf, ref)                                 # the padding between the tensors is nobody's
    o, c = layout[0]['w']
    assert not torch.equal(_bits(buf[:, o:o + c]), _bits(torch.from_numpy(host[:, o:o + c]).to(engine.device)))


# ---- 4. states and refusals ----------------------------------------------------------------------------------------------

def _batch(engine, name='tiny_mobile', seeds=(0, 1)):
    nets = [_unfolded(name, s, engine.device) for s in seeds]
    return nets, arena.NetworkBatch.from_unfolded([(g, b, r) for (_, g, b, r) in nets], TARG)


def test_other_plans_wait_for_the_fold(engine):
    nets, batch = _batch(engine)
    before = batch.storage.clone()
    calls = [batch.le_plan, batch.bc_plan, batch.quant_plan, batch.absorb_plan, batch.act_range_plan, batch.quantize, batch.absorb,
             batch.set_quant_minmax]
    for call in calls:
        with pytest.raises(RuntimeError, match='not been folded'):
            call()
    assert _same(batch.storage, before)
    plan = batch.fold_plan()
    plan.run()
    _ffi.synchronize()
    assert batch.folded is True
    with pytest.raises(RuntimeError, match='folded already'):
        plan.run()
    plan.close()
    with pytest.raises(RuntimeError, match='closed'):
        plan.run()
    again = batch.fold_plan()                              # making a plan is harmless, running it is refused
    after = batch.storage.clone()
    with pytest.raises(RuntimeError, match='folded already'):
        again.run()
    with pytest.raises(RuntimeError, match='folded already'):
        batch.merge_batchnorm()
    assert _same(batch.storage, after)
    again.close()
    for call in (batch.le_plan, batch.bc_plan, batch.quant_plan, batch.absorb_plan, batch.act_range_plan):
        call().close()


def test_fold_plan_on_a_plain_batch_is_refused(engine):
    nets = [_unfolded('tiny_mobile', s, engine.device) for s in (0, 1)]
    for (m, g, b, _) in nets:
        lt.merge_batchnorm(m, g, b, TARG)
    batch = arena.NetworkBatch([(g, b, r) for (_, g, b, r) in nets], TARG)
    assert batch.folded is True
    with pytest.raises(RuntimeError, match='folded networks'):
        batch.fold_plan()
    with pytest.raises(RuntimeError, match='folded networks'):
        batch.merge_batchnorm()
    batch.le_plan().close()


def _first_pairs(nets):
    _, g, b, _ = nets[0]
    return lt._fold_pairs(g, b, TARG)


def _refused(engine, spoil, key_of, name='tiny_mobile'):
    """from_unfolded raises ValueError naming the graph key, and has touched nothing"""
    nets = [_unfolded(name, s, engine.device) for s in (0, 1, 2)]
    key = key_of(nets)
    spoil(nets)
    biases = [[k for k, m in g.items() if type(m) in TARG and m.bias is not None] for (_, g, _, _) in nets]
    proxies = [[k for k, m in g.items() if hasattr(m, 'fake_weight')] for (_, g, _, _) in nets]
    with pytest.raises(ValueError, match=re.escape(key) + r'\b'):
        arena.NetworkBatch.from_unfolded([(g, b, r) for (_, g, b, r) in nets], TARG)
    assert biases == [[k for k, m in g.items() if type(m) in TARG and m.bias is not None] for (_, g, _, _) in nets]
    assert proxies == [[k for k, m in g.items() if hasattr(m, 'fake_weight')] for (_, g, _, _) in nets]


def test_a_folded_batchnorm_is_refused(engine):
    def spoil(nets):
        m, g, b, _ = nets[1]
        lt.merge_batchnorm(m, g, b, TARG)
    _refused(engine, spoil, lambda nets: _first_pairs(nets)[0][1])


def test_a_batchnorm_without_statistics_is_refused(engine):
    def spoil(nets):
        bn = nets[2][1][_first_pairs(nets)[3][1]]
        bn.running_mean = None
        bn.running_var = None
    _refused(engine, spoil, lambda nets: _first_pairs(nets)[3][1])


def test_a_batchnorm_without_affine_parameters_is_refused(engine):
    def spoil(nets):
        bn = nets[0][1][_first_pairs(nets)[2][1]]
        bn.weight = None
        bn.bias = None
    _refused(engine, spoil, lambda nets: _first_pairs(nets)[2][1])


def test_a_layer_claimed_by_two_batchnorms_is_refused(engine):
    def spoil(nets):
        for (_, g, b, _) in nets:
            (l0, _), (_, b1) = lt._fold_pairs(g, b, TARG)[:2]
            b[b1] = [l0]                                   # the second BatchNorm now hangs behind the first pair's layer
    _refused(engine, spoil, lambda nets: _first_pairs(nets)[0][0])


def test_networks_with_other_pairs_are_refused(engine):
    def spoil(nets):
        _, g, b, _ = nets[1]
        g[_first_pairs(nets)[4][1]] = nn.Identity()        # network 1 has no BatchNorm there
    _refused(engine, spoil, lambda nets: _first_pairs(nets)[4][1])


def test_networks_with_another_eps_are_refused(engine):
    def spoil(nets):
        nets[2][1][_first_pairs(nets)[1][1]].eps = 1e-3
    _refused(engine, spoil, lambda nets: _first_pairs(nets)[1][1])


@pytest.mark.parametrize('which', ['weight', 'running_var'])
def test_a_tensor_of_another_type_is_refused(engine, which):
    def spoil(nets):
        lk, bk = _first_pairs(nets)[2]
        if which == 'weight':
            layer = nets[1][1][lk]
            layer.weight = nn.Parameter(layer.weight.detach().double())
        else:
            bn = nets[1][1][bk]
            bn.running_var = bn.running_var.double()
    _refused(engine, spoil, lambda nets: _first_pairs(nets)[2][0 if which == 'weight' else 1])


class _Orphan(nn.Module):
    """conv - BN - ReLU twice, then a BatchNorm behind the ReLU: it follows no targ_type layer"""

    def __init__(self):
        super().__init__()
        self.a = nn.Sequential(nn.Conv2d(3, 8, 3, 1, 1, bias=False), nn.BatchNorm2d(8), nn.ReLU())
        self.b = nn.Sequential(nn.Conv2d(8, 12, 1, bias=True), nn.BatchNorm2d(12), nn.ReLU())
        self.post = nn.BatchNorm2d(12)
        self.fc = nn.Linear(12, 5)

    def forward(self, x):
        x = self.post(self.b(self.a(x)))
        return self.fc(torch.mean(x.view(x.size(0), x.size(1), -1), -1))


def test_a_batchnorm_behind_no_layer_is_left_alone(engine):
    """merge_batchnorm skips a BatchNorm without a targ_type layer among its bottoms, so does the batch: it keeps its tensors,
    its eps and its storages, and gets no proxies"""
    targ = [nn.Conv2d]

    def build(s):
        from dfq_amd.fxgraph import trace
        gen = torch.Generator(device='cpu')
        gen.manual_seed(s)
        with torch.no_grad():
            m = _Orphan()
            synthetic.init_weights(m, gen)
        m.eval()
        g, b = trace(m)
        m.to(engine.device)
        return m, g, b, rel.create_relation(g, b, targ, delete_single=False)
    nets = [build(s) for s in (0, 1)]
    twins = [build(s) for s in (0, 1)]
    g0, b0 = nets[0][1], nets[0][2]
    orphan = [k for k, m in g0.items() if m is nets[0][0].post]
    assert len(orphan) == 1 and len(lt._fold_pairs(g0, b0, targ)) == 2 and orphan[0] not in [bk for _, bk in lt._fold_pairs(g0, b0, targ)]
    bk = orphan[0]
    batch = arena.NetworkBatch.from_unfolded([(g, b, r) for (_, g, b, r) in nets], targ)
    batch.merge_batchnorm()
    for n, ((_, g, _, _), (mt, gt, bt, _)) in enumerate(zip(nets, twins)):
        lt.merge_batchnorm(mt, gt, bt, targ)
        _assert_equal(g, gt, 'net {}'.format(n))
        assert not hasattr(g[bk], 'fake_weight') and g[bk].eps == 1e-5 and not bool((g[bk].weight == 1).all())
        assert g[bk].weight.untyped_storage().data_ptr() != batch.storage.untyped_storage().data_ptr()
        assert any(hasattr(m, 'fake_weight') for m in g.values())


@pytest.mark.parametrize('moved', ['weight', 'bias', 'bn.weight', 'bn.running_var', 'bn.fake_bias'])
def test_a_tensor_that_left_its_slot_is_refused(engine, moved):
    nets, batch = _batch(engine, seeds=(0, 1, 2))
    g = nets[0][1]
    lk, bk = _first_pairs(nets)[3]
    if moved == 'bn.fake_bias':
        g[bk].fake_bias = g[bk].fake_bias.clone()
    elif moved == 'bn.running_var':
        g[bk].running_var = g[bk].running_var.clone()
    else:
        t = getattr(g[bk], 'weight') if moved == 'bn.weight' else getattr(g[lk], moved)
        t.data = t.data.clone()
    batch.check()                                          # (the quick check does not see a middle slot)
    before = batch.storage.clone()
    with pytest.raises(RuntimeError, match='no longer lives in its slot'):
        batch.fold_plan()
    with pytest.raises(RuntimeError, match='no longer lives in its slot'):
        batch.merge_batchnorm()
    _ffi.synchronize()
    assert _same(batch.storage, before) and batch.folded is False


def test_release(engine):
    nets, batch = _batch(engine, seeds=(0, 1, 2))
    plan = batch.fold_plan()
    batch.merge_batchnorm()
    want = [{k: v.detach().clone() for k, v in _state(g).items()} for (_, g, _, _) in nets]
    home = batch.storage.untyped_storage().data_ptr()
    batch.release()
    with pytest.raises(RuntimeError, match='released'):
        batch.fold_plan()
    with pytest.raises(RuntimeError, match='released'):
        plan.run()
    with pytest.raises(RuntimeError, match='released'):
        batch.le_plan()
    plan.close()
    seen = set()
    for n, (_, g, b, _) in enumerate(nets):
        now = _state(g)
        assert sorted(now) == sorted(want[n])
        for k, t in now.items():
            assert _same(t, want[n][k]), 'net {} {}'.format(n, k)
            p = t.untyped_storage().data_ptr()
            assert p != home and p not in seen, 'net {} {} shares a storage'.format(n, k)
            seen.add(p)
        for _, bk in lt._fold_pairs(g, b, TARG):
            bn = g[bk]
            assert bool((bn.weight == 1).all()) and bool((bn.running_var == 1).all())
            assert bool((_bits(bn.bias) == 0).all()) and bool((_bits(bn.running_mean) == 0).all())


# ---- 5. the C ABI ----------------------------------------------------------------------------------------------------------

def test_struct_layout_matches_header():
    src = r'''
    #include <stdio.h>
    #include <stddef.h>
    #include "dfq_hip.h"
    int main(void) {
        printf("%zu %zu %zu %zu %zu\n", sizeof(dfq_batch_fold_pair), offsetof(dfq_batch_fold_pair, fake_bias),
               offsetof(dfq_batch_fold_pair, row_len), offsetof(dfq_batch_fold_pair, out_ch), offsetof(dfq_batch_fold_pair, eps));
        return 0;
    }'''
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, 't.c')
        open(c, 'w').write(src)
        exe = os.path.join(d, 't')
        subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), c, '-o', exe], check=True)
        sizes = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    P = _ffi.DfqBatchFoldPair
    assert sizes == [ctypes.sizeof(P), P.fake_bias.offset, P.row_len.offset, P.out_ch.offset, P.eps.offset]


def test_abi_rejects_bad_arguments(engine):
    lib = _ffi.lib()
    buf = torch.zeros(2 * 2048, dtype=torch.float32, device=engine.device)
    at = lambda i: buf.data_ptr() + 4 * 64 * i             # noqa: E731
    bases = (ctypes.c_void_p * 2)(buf.data_ptr(), buf.data_ptr() + 4 * 2048)

    def pair(w=at(0), b=at(4), gamma=at(5), beta=at(6), mean=at(7), var=at(8), fw=at(9), fb=at(10), row_len=27, out_ch=8, eps=1e-5):
        return _ffi.DfqBatchFoldPair(w, b, gamma, beta, mean, var, fw, fb, row_len, out_ch, eps)

    def create(pairs=None, n_pairs=None, n_nets=2, b=bases, out=True):
        pairs = [pair()] if pairs is None else pairs
        plan = ctypes.c_void_p()
        arr = (_ffi.DfqBatchFoldPair * len(pairs))(*pairs) if pairs else None
        rc = lib.dfq_batch_fold_plan_create(arr, len(pairs) if n_pairs is None else n_pairs, b, n_nets,
                                            ctypes.byref(plan) if out else None)
        got = (lib.dfq_batch_fold_plan_launches(plan), lib.dfq_batch_fold_plan_elements(plan)) if rc == 0 else None
        if rc == 0:
            lib.dfq_batch_fold_plan_destroy(plan)
        return rc, got

    second = dict(w=at(12), b=at(16), gamma=at(17), beta=at(18), mean=at(19), var=at(20), fw=at(21), fb=at(22))
    assert create() == (0, (2, 216))
    assert create(pairs=[pair(), pair(**second)]) == (0, (2, 432))
    bad = [dict(pairs=[]), dict(n_pairs=0), dict(n_pairs=-1), dict(out=False)]
    bad += [dict(pairs=[pair(**{k: None})]) for k in ('w', 'b', 'gamma', 'beta', 'mean', 'var', 'fw', 'fb')]
    bad += [dict(pairs=[pair(out_ch=0)]), dict(pairs=[pair(out_ch=-3)]), dict(pairs=[pair(row_len=0)]), dict(pairs=[pair(row_len=-1)]),
            dict(pairs=[pair(w=at(0) + 4)]), dict(pairs=[pair(w=at(0) + 8)]),
            dict(pairs=[pair(), pair(**dict(second, w=at(0)))])]
    bad += [dict(pairs=[pair(), pair(**dict(second, **{k: at(i)}))])
            for k, i in (('b', 4), ('gamma', 5), ('beta', 6), ('mean', 7), ('var', 8), ('fw', 9), ('fb', 10), ('gamma', 8), ('fb', 6))]
    bad += [dict(n_nets=0), dict(n_nets=-2), dict(b=None), dict(b=(ctypes.c_void_p * 2)(buf.data_ptr(), None)),
            dict(b=(ctypes.c_void_p * 2)(buf.data_ptr(), buf.data_ptr() + 4 * 2047))]
    for kw in bad:
        assert create(**kw)[0] == DFQ_ERR_ARG, kw
        assert b'dfq_batch_fold_plan_create' in lib.dfq_last_error(), kw
    assert lib.dfq_batch_fold_plan_run(None, None) == DFQ_ERR_ARG
    assert b'dfq_batch_fold_plan_run' in lib.dfq_last_error()
    assert lib.dfq_batch_fold_plan_launches(None) == 0 and lib.dfq_batch_fold_plan_elements(None) == 0
    lib.dfq_batch_fold_plan_destroy(None)


# ---- 6. full size, on the MI355X -------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize('name,count', [('mobilenet_v2', 4), ('resnet18', 2), ('deeplab_mnv2', 2)])
def test_full_size(name, count):
    dev = torch.device('cuda', 0)
    nets = [_unfolded(name, s, dev) for s in range(count)]
    twins = [_unfolded(name, s, dev) for s in range(count)]
    batch = arena.NetworkBatch.from_unfolded([(g, b, r) for (_, g, b, r) in nets], TARG)
    plan = batch.fold_plan()
    assert plan.launches <= 2
    pairs = lt._fold_pairs(nets[0][1], nets[0][2], TARG)
    assert plan.n_pairs == len(pairs) == {'mobilenet_v2': 52, 'resnet18': 20, 'deeplab_mnv2': 60}[name]
    plan.close()
    batch.merge_batchnorm()
    torch.cuda.synchronize()
    for n, ((_, g, _, _), (mt, gt, bt, _)) in enumerate(zip(nets, twins)):
        lt.merge_batchnorm(mt, gt, bt, TARG)
        _assert_equal(g, gt, '{} net {}'.format(name, n))
        assert all(g[bk].eps == 1e-12 for _, bk in pairs)
    batch.release()


# ---- 7. the walk merge_batchnorm and the batch share -----------------------------------------------------------------------

@pytest.mark.parametrize('name', SYNTHETIC)
def test_the_merged_walk(name):
    _, graph, bottoms = synthetic.build(name, seed=0)
    got = lt._fold_pairs(graph, bottoms, TARG)
    assert got == _old_walk(graph, bottoms, TARG) and got
    assert lt._fold_pairs(graph, bottoms, [nn.Linear]) == _old_walk(graph, bottoms, [nn.Linear]) == []
    before = {k: (type(m), None if not isinstance(m, nn.Module) else sorted(m.state_dict())) for k, m in graph.items()}
    lt._fold_pairs(graph, bottoms, TARG)
    assert before == {k: (type(m), None if not isinstance(m, nn.Module) else sorted(m.state_dict())) for k, m in graph.items()}
