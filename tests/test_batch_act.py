"""NetworkBatch.act_range_plan / dfq_batch_act_plan_*: set_quant_minmax (utils/layer_transform.py:347-609) for every network
of a batch in one plan.

The contract is "the same operations in the same order": every (min, max) must be the bit pattern ``lt.set_quant_minmax``
leaves on a twin of that network alone (own storages, QConv2d / QLinear layers), NaN equal to NaN, on the CPU emulation and
on the MI355X alike.  The reference's recorded outputs (tests/golden/minmax_*.npz) are held to 1e-5 * max(1, |ref|), the
bound tests/test_minmax.py uses for the engine, for the reason given there: float64 pdf / cdf from different libms."""
import copy
import ctypes
import glob
import math
import os
import re
from collections import OrderedDict

import numpy as np
import pytest
import torch
import torch.nn as nn

from dfq_amd import _ffi, arena, ncnn_table, synthetic
from dfq_amd.utils import layer_transform as lt
from dfq_amd.utils import relation as rel
from dfq_amd.utils.quantize import QConv2d, QLinear

from common import GOLD, TARG

DFQ_ERR_ARG = -1     # include/dfq_hip.h
QTARG = [QConv2d, QLinear]
TINY = ['tiny_mobile', 'tiny_res', 'tiny_cat', 'tiny_wide', 'tiny_head', 'tiny_seg', 'tiny_tail']
BIG = ['mobilenet_v2', 'resnet18', 'deeplab_mnv2']
CASE_D = {'tiny_head'}                       # a conv / linear without BatchNorm in front of a quantiser
CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLD, 'minmax_*.npz')))


class _Gpu:
    kind, device = 'gpu', torch.device('cuda', 0)


# ---- helpers -----------------------------------------------------------------------------------------------------------
def _prepared(name, seed, device, relu6=False, targ=TARG):
    model, graph, bottoms = synthetic.build(name, seed=seed, keep_relu6=relu6)
    model.to(device)
    if targ is QTARG:
        graph = _twin_graph(graph, device)
    lt.merge_batchnorm(model, graph, bottoms, targ)
    rels = rel.create_relation(graph, bottoms, targ, delete_single=False)
    return graph, bottoms, rels


def _twin_graph(graph, device):
    """the same network with storages of its own: QConv2d / QLinear for the conv / linear layers (tests/test_minmax.py:
    _q_graph), BatchNorm modules with cloned parameters and buffers (the proxies among them)"""
    out = OrderedDict()
    for k, m in graph.items():
        if isinstance(m, nn.Conv2d):
            q = QConv2d(m.in_channels, m.out_channels, m.kernel_size, m.stride, m.padding, m.dilation, m.groups, m.bias is not None)
        elif isinstance(m, nn.Linear):
            q = QLinear(m.in_features, m.out_features, m.bias is not None)
        elif isinstance(m, nn.BatchNorm2d):
            bn = copy.copy(m)
            bn._parameters = OrderedDict((n, nn.Parameter(p.detach().clone(), requires_grad=False)) for n, p in m._parameters.items())
            bn._buffers = OrderedDict((n, None if b is None else b.detach().clone()) for n, b in m._buffers.items())
            out[k] = bn
            continue
        else:
            out[k] = m
            continue
        q.weight.data.copy_(m.weight.data)
        if m.bias is not None:
            q.bias.data.copy_(m.bias.data)
        out[k] = q.to(device)
    return out


def _tensor_ops(graph, bottoms):
    """{key: count} of the tensor ops the reference quantises (utils/layer_transform.py:10-14), as tests/test_minmax.py"""
    out = OrderedDict()
    for k, m in graph.items():
        if isinstance(m, str) and k != 'Data':
            if 'add' in k or 'cat' in k:
                out[k] = len(bottoms[k])
            elif 'mean' in k or 'interpolate' in k or 'softmax' in k:
                out[k] = 1
    return out


NO_BATCH_BC = {'tiny_head'}     # dfq_bc_plan_create refuses its layers without BatchNorm (an older limit of the correction plan)


def _batch(name, seeds, engine, relu6=False, targ=TARG, calibrate=True):
    """A batch whose proxies are the ones a real run sees: equalised and bias-corrected through the batch's own plans
    (equalised only where the correction plan cannot be built).  On the MI355X the equalisation runs to convergence; the fiber
    emulation gets ONE sweep, because it spends minutes on the converged run of tiny_wide -- the proxies are scaled either way,
    and what is compared are two evaluations of the same proxies."""
    nets = [_prepared(name, s, engine.device, relu6, targ) for s in seeds]
    batch = arena.NetworkBatch(nets, targ)
    if calibrate:
        if nets[0][2]:                           # (with ReLU6 kept some architectures have no relation: nothing to equalise)
            le = batch.le_plan()
            le.run(max_sweeps=1 if engine.kind == 'emu' else None)
            le.close()
        if name not in NO_BATCH_BC:
            bc = batch.bc_plan()
            bc.run(check=True)
            bc.close()
        _ffi.synchronize()
    return nets, batch


def _single(graph, bottoms, device, is_detection=False, N=6, ops=None):
    """lt.set_quant_minmax on a twin of `graph`: OrderedDict key -> float32 tensor [2], or a list of them for a tensor op"""
    gq = _twin_graph(graph, device)
    tq = None
    if ops:
        from dfq_amd.utils.quantize import QuantMeasure
        tq = {k: [QuantMeasure().to(device) for _ in range(c)] for k, c in ops.items()}
    lt.set_quant_minmax(gq, bottoms, is_detection=is_detection, N=N, verbose=False, tensor_op_quant=tq)
    out = OrderedDict()
    for k, m in gq.items():
        if bottoms[k] is None:
            continue
        if hasattr(m, 'quant'):
            out[k] = torch.cat([m.quant.running_min.reshape(1), m.quant.running_max.reshape(1)]).cpu()
        elif tq and k in tq:
            out[k] = [torch.cat([q.running_min.reshape(1), q.running_max.reshape(1)]).cpu() for q in tq[k]]
    return out


def _flat(ranges):
    out = []
    for v in ranges.values():
        out.extend(v if isinstance(v, list) else [v])
    return out


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _assert_same_bits(got, want, what):
    """two range dicts: same keys in the same order, every float the same bit pattern (NaN equal to NaN)"""
    assert list(got.keys()) == list(want.keys()), what
    a, b = _flat(got), _flat(want)
    assert len(a) == len(b), what
    for i, (x, y) in enumerate(zip(a, b)):
        x, y = x.detach().cpu(), y.detach().cpu()
        same = (_bits(x) == _bits(y)) | (torch.isnan(x) & torch.isnan(y))
        assert bool(same.all()), '{}: range {} is {} (bits {}), the single-network function gives {} (bits {})'.format(
            what, i, x.tolist(), _bits(x).tolist(), y.tolist(), _bits(y).tolist())


def _check_against_single(nets, batch, engine, what, **kw):
    plan = batch.act_range_plan(is_detection=kw.get('is_detection', False), N=kw.get('N', 6), tensor_ops=kw.get('ops'))
    plan.run()
    _ffi.synchronize()
    for n, (g, b, _) in enumerate(nets):
        want = _single(g, b, engine.device, kw.get('is_detection', False), kw.get('N', 6), kw.get('ops'))
        assert plan.keys == list(want.keys())
        _assert_same_bits(plan.ranges(n), want, '{} net {}'.format(what, n))
    return plan


# ---- 1. bit identity with the single-network function ------------------------------------------------------------------
@pytest.mark.parametrize('name', TINY)
@pytest.mark.parametrize('relu6,det,N', [(False, False, 6), (True, False, 6), (False, True, 3), (True, True, 3)])
def test_batch_equals_per_network(engine, name, relu6, det, N):
    nets, batch = _batch(name, [0, 1, 2], engine, relu6)
    plan = _check_against_single(nets, batch, engine, name, is_detection=det, N=N)
    # 4. launch count: one launch, and one more for the vectors pushed through a layer without BatchNorm
    assert plan.launches == (2 if name in CASE_D else 1)
    assert plan.n_sources == (6 if name in CASE_D else 0)           # 3 of tiny_head's 6 quantisers, two vectors each
    # the networks differ, so a plan that read network 0 for everybody would have been seen
    # (with ReLU6 kept and N = 6 every range of the small networks is clamped to [0, 6])
    assert relu6 or not torch.equal(_bits(plan.block[0]), _bits(plan.block[1]))
    plan.close()


@pytest.mark.parametrize('name', TINY)
def test_batch_equals_per_network_with_tensor_ops(engine, name):
    """the quantisers of add / cat / mean inputs (1 to 1 with several quantisers, and many to many)"""
    nets, batch = _batch(name, [3, 4, 5], engine, True)
    ops = _tensor_ops(nets[0][0], nets[0][1])
    plan = _check_against_single(nets, batch, engine, name, ops=ops)
    for k, c in ops.items():
        assert len(plan.ranges(0)[k]) == c
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize('name', BIG)
def test_big_networks_equal_per_network(name):
    """the three benchmark architectures, on the MI355X (the fiber emulation would spend minutes on their equalisation)"""
    assert torch.cuda.is_available(), 'gpu-marked test needs a ROCm GPU'
    _ffi.lib()
    engine = _Gpu()
    nets, batch = _batch(name, [0, 1, 2], engine)
    plan = _check_against_single(nets, batch, engine, name)
    assert plan.launches == 1
    plan.close()
    plan = _check_against_single(nets, batch, engine, name + ' ops', N=3, ops=_tensor_ops(nets[0][0], nets[0][1]))
    plan.close()
    torch.cuda.synchronize()


# ---- 2. against the reference's recorded outputs ----------------------------------------------------------------------
def _parse(tag):
    m = re.match(r'minmax_(\w+?)_s(\d+)((?:_relu6)?)((?:_det)?)((?:_ops)?)$', tag)
    return m.group(1), int(m.group(2)), bool(m.group(3)), bool(m.group(4)), bool(m.group(5))


def test_fixtures_exist():
    assert len(CASES) >= 17


@pytest.mark.parametrize('tag', CASES)
def test_against_reference_fixture(engine, tag):
    """The fixture's proxies (and case-(d) weights) in network 1 of a batch of three whose other networks hold other values.
    Every fixture's topology is one a NetworkBatch holds (the synthetic builder's); the `_ops` fixtures go through
    ``tensor_ops`` on that plain graph, which is the graph the reference's quantised tensor ops were recorded on."""
    name, seed, relu6, det, with_ops = _parse(tag)
    gold = np.load(os.path.join(GOLD, tag + '.npz'))
    nets = [_prepared(name, s, engine.device, relu6) for s in (seed + 11, seed, seed + 12)]
    for g, _, _ in nets:
        for i, k in enumerate(g):
            if type(g[k]) in TARG and 'b{}'.format(i) in gold.files:
                lt._ensure_bias(g[k])
    batch = arena.NetworkBatch(nets, TARG)
    g, b, _ = nets[1]
    with torch.no_grad():
        for i, k in enumerate(g):
            m = g[k]
            if type(m) == nn.BatchNorm2d:
                fw = torch.from_numpy(gold['bn{}'.format(i)][0].copy()).to(engine.device)
                fb = torch.from_numpy(gold['bn{}'.format(i)][1].copy()).to(engine.device)
                if hasattr(m, 'fake_weight'):
                    m.fake_weight.copy_(fw)
                    m.fake_bias.copy_(fb)
                else:
                    m.register_buffer('fake_weight', fw)
                    m.register_buffer('fake_bias', fb)
            elif type(m) in TARG and 'w{}'.format(i) in gold.files:
                m.weight.copy_(torch.from_numpy(gold['w{}'.format(i)]))
                if 'b{}'.format(i) in gold.files:
                    m.bias.copy_(torch.from_numpy(gold['b{}'.format(i)]))
    batch.check(thorough=True)                                      # the copies went INTO the slots
    ops = _tensor_ops(g, b) if with_ops else None
    plan = batch.act_range_plan(is_detection=det, N=int(gold['cfg'][2]), tensor_ops=ops)
    plan.run()
    _ffi.synchronize()
    keys = list(g.keys())
    assert [keys.index(k) for k in plan.keys] == gold['layers'].tolist()
    got = _flat(plan.ranges(1))
    assert len(got) == len(gold['ranges'])
    worst = 0.0
    for r, (rlo, rhi) in zip(got, gold['ranges']):
        lo, hi = r.tolist()
        worst = max(worst, abs(lo - rlo) / max(1.0, abs(rlo)), abs(hi - rhi) / max(1.0, abs(rhi)))
    print('{}: worst relative deviation from the reference {:.3e}'.format(tag, worst))
    for r, (rlo, rhi) in zip(got, gold['ranges']):
        lo, hi = r.tolist()
        assert abs(lo - rlo) <= 1e-5 * max(1.0, abs(rlo)) and abs(hi - rhi) <= 1e-5 * max(1.0, abs(rhi)), (tag, (lo, hi), (rlo, rhi))
    # the neighbours hold other numbers (with ReLU6 kept the small networks' ranges may all be the clamps, [0, 6])
    assert relu6 or not torch.equal(_bits(plan.block[0]), _bits(plan.block[1])) and (relu6 or not torch.equal(_bits(plan.block[2]), _bits(plan.block[1])))
    plan.close()


# ---- 3. isolation and purity ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['tiny_res', 'tiny_head'])
def test_isolation_and_purity(engine, name):
    nets, batch = _batch(name, [0, 1, 2, 3], engine)
    plan = batch.act_range_plan()
    before = batch.storage.clone()
    plan.run()
    _ffi.synchronize()
    first = plan.block.clone()
    assert torch.equal(_bits(batch.storage), _bits(before)), 'run() wrote into the batch allocation'
    plan.run()
    _ffi.synchronize()
    assert torch.equal(_bits(plan.block), _bits(first)), 'a second run gave another block'
    with torch.no_grad():
        for m in nets[2][0].values():
            if isinstance(m, nn.BatchNorm2d) and hasattr(m, 'fake_bias'):
                m.fake_bias.add_(0.37)
                m.fake_weight.mul_(1.5)
    plan.run()
    _ffi.synchronize()
    for n in (0, 1, 3):
        assert torch.equal(_bits(plan.block[n]), _bits(first[n])), 'network {} saw the change made to network 2'.format(n)
    changed = (_bits(plan.block[2]) != _bits(first[2])).any(dim=1)
    const = [i for i, k in enumerate(plan.keys) if nets[0][1][k] == ['Data']]
    assert [i for i in range(plan.n_results) if not bool(changed[i])] == const      # every range but the input's constant
    _assert_same_bits(plan.ranges(2), _single(nets[2][0], nets[2][1], engine.device), name + ' changed network')
    plan.close()


# ---- 5. degenerate channels --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['tiny_mobile', 'tiny_res', 'tiny_cat', 'tiny_head'])
@pytest.mark.parametrize('relu6', [False, True])
def test_degenerate_channels(engine, name, relu6):
    """a dead channel (gamma~ = 0: t = -beta~ / 0), a NaN and an infinite proxy in ONE network"""
    nets, batch = _batch(name, [0, 1, 2], engine, relu6)
    plan = batch.act_range_plan()
    plan.run()
    _ffi.synchronize()
    clean = plan.block.clone()
    bns = [m for m in nets[1][0].values() if isinstance(m, nn.BatchNorm2d) and hasattr(m, 'fake_bias')]
    assert len(bns) >= 3
    with torch.no_grad():
        for j, m in enumerate(bns):
            m.fake_weight[0] = 0.0                                   # dead, with a mean of either sign or zero
            m.fake_bias[0] = (0.0, 0.8, -0.8)[j % 3]
        bns[len(bns) // 3].fake_bias[1] = math.nan
        bns[(2 * len(bns)) // 3].fake_weight[1] = math.inf
        bns[-1].fake_bias[1] = -math.inf
    plan.run()
    _ffi.synchronize()
    for n in (0, 2):
        assert torch.equal(_bits(plan.block[n]), _bits(clean[n]))
    assert not torch.isfinite(plan.block[1]).all(), 'the planted values reached no quantiser'
    _assert_same_bits(plan.ranges(1), _single(nets[1][0], nets[1][1], engine.device), name + ' degenerate')
    plan.close()


# ---- 6. quantiser binding ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['tiny_mobile', 'tiny_res', 'tiny_head'])
def test_quantiser_binding(engine, name):
    nets, batch = _batch(name, [0, 1, 2], engine, targ=QTARG)
    twins = []
    for g, b, _ in nets:
        gq = _twin_graph(g, engine.device)
        lt.set_quant_minmax(gq, b, verbose=False)
        twins.append(gq)
    plan = batch.set_quant_minmax()
    block = plan.block
    lo, hi = block.data_ptr(), block.data_ptr() + 4 * block.numel()
    gen = torch.Generator().manual_seed(5)
    for n, ((g, b, _), gq) in enumerate(zip(nets, twins)):
        qkeys = [k for k, m in g.items() if hasattr(m, 'quant') and b[k] is not None]
        assert qkeys == plan.keys
        for k in qkeys:
            q, qt = g[k].quant, gq[k].quant
            assert torch.equal(_bits(q.running_min), _bits(qt.running_min)) and torch.equal(_bits(q.running_max), _bits(qt.running_max)), (n, k)
            assert q.running_min.shape == (1,) and q.running_max.shape == (1,)
            pair = q._packed_range(engine.device)                   # adopted as it is: no re-pack
            assert pair is not None and lo <= pair.data_ptr() < hi and pair.data_ptr() == q.running_min.data_ptr()
            assert q.running_min.untyped_storage().data_ptr() == block.untyped_storage().data_ptr()
        assert ncnn_table.calibration_table(g, targ_type=QTARG) == ncnn_table.calibration_table(gq, targ_type=QTARG)
        k = qkeys[len(qkeys) // 2]
        x = (torch.randn(2, 5, 7, generator=gen) * 3).to(engine.device)
        g[k].quant.update_stat = gq[k].quant.update_stat = False
        assert torch.equal(_bits(g[k].quant.eval()(x)), _bits(gq[k].quant.eval()(x)))
    with pytest.raises(RuntimeError, match='closed'):
        plan.run()
    want = [{k: (g[k].quant.running_min.clone(), g[k].quant.running_max.clone()) for k in plan.keys} for g, _, _ in nets]
    batch.release()
    home = block.untyped_storage().data_ptr()
    for (g, b, _), w in zip(nets, want):
        for k in plan.keys:
            q = g[k].quant
            assert q.running_min.untyped_storage().data_ptr() != home and q.running_max.untyped_storage().data_ptr() != home
            assert torch.equal(_bits(q.running_min), _bits(w[k][0])) and torch.equal(_bits(q.running_max), _bits(w[k][1]))
    block.fill_(123.0)                                               # nobody looks at the block any more
    for (g, b, _), w in zip(nets, want):
        for k in plan.keys:
            assert torch.equal(_bits(g[k].quant.running_min), _bits(w[k][0]))


def test_binding_tensor_op_quantisers(engine):
    """batch.set_quant_minmax(tensor_op_quant=[one dict per network]) derives tensor_ops and binds those modules too"""
    from dfq_amd.utils.quantize import QuantMeasure
    nets, batch = _batch('tiny_res', [0, 1], engine, targ=QTARG)
    ops = _tensor_ops(nets[0][0], nets[0][1])
    assert ops
    tqs = [{k: [QuantMeasure().to(engine.device) for _ in range(c)] for k, c in ops.items()} for _ in nets]
    plan = batch.set_quant_minmax(N=3, tensor_op_quant=tqs)
    for n, (g, b, _) in enumerate(nets):
        want = _single(g, b, engine.device, N=3, ops=ops)
        _assert_same_bits(plan.ranges(n), want, 'net {}'.format(n))
        for k in ops:
            for q, w in zip(tqs[n][k], want[k]):
                assert torch.equal(_bits(torch.cat([q.running_min, q.running_max])), _bits(w))
    with pytest.raises(ValueError):
        batch.set_quant_minmax(tensor_op_quant=tqs[:1])
    batch.release()
    assert all(q.running_min.untyped_storage().data_ptr() != plan.block.untyped_storage().data_ptr() for tq in tqs for qs in tq.values() for q in qs)


def test_plain_layers_get_ranges_and_nothing_is_bound(engine):
    """a batch of plain nn.Conv2d / nn.Linear: a range per targ layer (its input's), no module to bind"""
    nets, batch = _batch('tiny_mobile', [0, 1], engine)
    plan = batch.set_quant_minmax()
    g, b, _ = nets[0]
    assert plan.keys == [k for k, m in g.items() if type(m) in TARG]
    assert not batch._act_bound
    assert plan.ranges(0)[plan.keys[0]].tolist() == [np.float32(-2.11790393), np.float32(2.64)]


# ---- 7. errors ---------------------------------------------------------------------------------------------------------
def test_act_range_plan_rejects_bad_arguments(engine):
    nets, batch = _batch('tiny_res', [0, 1], engine, calibrate=False)
    g0, b0, _ = nets[0]
    add = next(k for k in _tensor_ops(g0, b0))
    for kw in [dict(N='six'), dict(N=None), dict(N=math.nan), dict(N=math.inf), dict(N=True), dict(tensor_ops={'no such node': 1}),
               dict(tensor_ops={next(k for k, m in g0.items() if type(m) in TARG): 1}), dict(tensor_ops={'Data': 1}),
               dict(tensor_ops={add: 0}), dict(tensor_ops={add: -2}), dict(tensor_ops={add: 1.5}), dict(tensor_ops={add: True})]:
        with pytest.raises(ValueError):
            batch.act_range_plan(**kw)
    p = batch.act_range_plan()
    p.run()
    p.close()
    p.close()
    with pytest.raises(RuntimeError, match='closed'):
        p.run()
    # a proxy that has left its slot, or is not what the kernels read
    bn_key = next(k for k, m in g0.items() if isinstance(m, nn.BatchNorm2d) and hasattr(m, 'fake_weight'))
    bn = g0[bn_key]
    kept = bn._buffers['fake_weight']
    for moved in (kept.clone(), kept.double(), torch.cat([kept, kept])[::2]):
        bn._buffers['fake_weight'] = moved
        with pytest.raises(RuntimeError, match='fake_weight of {} '.format(re.escape(bn_key))):
            batch.act_range_plan()
    bn._buffers['fake_weight'] = kept
    kept_b = bn._buffers['fake_bias']
    bn._buffers['fake_bias'] = kept_b.clone()
    with pytest.raises(RuntimeError, match='fake_bias of {} '.format(re.escape(bn_key))):
        batch.act_range_plan()
    bn._buffers['fake_bias'] = kept_b
    del bn._buffers['fake_weight']
    with pytest.raises(ValueError, match='merge_batchnorm first'):
        batch.act_range_plan()
    bn._buffers['fake_weight'] = kept
    p = batch.act_range_plan()
    batch.release()
    with pytest.raises(RuntimeError, match='released'):
        p.run()
    with pytest.raises(RuntimeError, match='released'):
        p.bind_quantisers()
    with pytest.raises(RuntimeError, match='released'):
        batch.act_range_plan()
    with pytest.raises(RuntimeError, match='released'):
        batch.set_quant_minmax()
    p.close()


def test_case_d_weight_must_be_in_its_slot(engine):
    nets, batch = _batch('tiny_head', [0, 1], engine, calibrate=False)
    g0 = nets[0][0]
    plan = batch.act_range_plan()
    assert plan.launches == 2
    plan.close()
    hit = 0
    for k, m in g0.items():
        if type(m) in TARG:
            kept = m.weight.data
            if kept.data_ptr() == int(batch.bases[0]):
                continue                             # the first layer (fed by the input): the batch's own quick check watches it
            m.weight.data = kept.clone()
            try:
                batch.act_range_plan().close()
            except RuntimeError as e:
                assert 'weight of {} '.format(k) in str(e)
                hit += 1
            m.weight.data = kept
    assert hit == 3                                  # the three layers without BatchNorm in front of a quantiser


def test_c_entry_points_reject_bad_tables(engine):
    lib = _ffi.lib()
    buf = torch.zeros(4096, dtype=torch.float32, device=engine.device)
    out = torch.zeros(64, dtype=torch.float32, device=engine.device)
    bases = (ctypes.c_void_p * 2)(buf.data_ptr(), buf.data_ptr() + 4 * 2048)

    def at(i):
        return buf.data_ptr() + 256 * i
    A = _ffi
    Step, Res, Src = A.DfqBatchActStep, A.DfqBatchActResult, A.DfqBatchActSource

    def step(op, fw=at(0), fb=at(1), ch=16, relu=0, operand=0, sw=-1, sb=-1, lo=0.0, hi=0.0):
        return Step(fw, fb, op, ch, relu, operand, sw, sb, lo, hi)

    def create(steps, results=None, sources=(), b=bases, n_nets=2, N=6.0, eps=1e-6, o=out.data_ptr(), stride=None, n_results=None):
        results = [Res(0, len(steps))] if results is None else results
        stride = 2 * len(results) if stride is None else stride
        plan = ctypes.c_void_p()
        rc = lib.dfq_batch_act_plan_create(
            (Res * len(results))(*results) if results else None, len(results) if n_results is None else n_results,
            (Step * len(steps))(*steps) if steps else None, len(steps),
            (Src * len(sources))(*sources) if sources else None, len(sources), b, n_nets,
            ctypes.c_float(N), ctypes.c_float(eps), o, stride, ctypes.byref(plan))
        n = lib.dfq_batch_act_plan_launches(plan) if rc == 0 else None
        if rc == 0:
            lib.dfq_batch_act_plan_destroy(plan)
        return rc, n
    src = Src(at(2), at(3), at(0), 16, 4, 1, 1)
    good_mom = [step(A.ACT_MOM, relu=1), step(A.ACT_MOM_ADD, fw=at(4), fb=at(5)), step(A.ACT_MOM_RELU, None, None, 0, 2),
                step(A.ACT_MOM_RANGE, None, None, 0)]
    assert create([step(A.ACT_CONST, None, None, 0, lo=-1.0, hi=1.0)]) == (0, 1)
    assert create([step(A.ACT_RANGE, relu=2)]) == (0, 1)
    assert create([step(A.ACT_RANGE), step(A.ACT_RANGE_CAT, relu=1), step(A.ACT_RANGE_ONE), step(A.ACT_RANGE_DIV, None, None, 0, operand=3)]) == (0, 1)
    assert create(good_mom) == (0, 1)
    assert create([step(A.ACT_RANGE, None, None, sw=1, sb=0)], sources=[src, src]) == (0, 2)
    assert create(good_mom + [step(A.ACT_RANGE)], results=[Res(0, 4), Res(4, 1)]) == (0, 1)
    bad = [dict(steps=[]), dict(steps=[step(A.ACT_RANGE)], results=[]), dict(steps=[step(A.ACT_RANGE)], n_results=0),
           dict(steps=[step(A.ACT_RANGE)], b=None), dict(steps=[step(A.ACT_RANGE)], n_nets=0),
           dict(steps=[step(A.ACT_RANGE)], b=(ctypes.c_void_p * 2)(buf.data_ptr(), None)),
           dict(steps=[step(A.ACT_RANGE)], N=math.nan), dict(steps=[step(A.ACT_RANGE)], N=math.inf), dict(steps=[step(A.ACT_RANGE)], eps=math.nan),
           dict(steps=[step(A.ACT_RANGE)], o=None), dict(steps=[step(A.ACT_RANGE)], stride=1),
           dict(steps=[step(A.ACT_RANGE, fw=None)]), dict(steps=[step(A.ACT_RANGE, fb=None)]), dict(steps=[step(A.ACT_RANGE, ch=0)]),
           dict(steps=[step(A.ACT_RANGE, relu=3)]), dict(steps=[step(A.ACT_RANGE, relu=-1)]), dict(steps=[step(9)]), dict(steps=[step(-1)]),
           dict(steps=[step(A.ACT_RANGE)], results=[Res(0, 2)]), dict(steps=[step(A.ACT_RANGE)], results=[Res(-1, 1)]),
           dict(steps=[step(A.ACT_RANGE)], results=[Res(0, 0)]), dict(steps=[step(A.ACT_RANGE)], results=[Res(1, 1)]),
           dict(steps=[step(A.ACT_RANGE_CAT)]), dict(steps=[step(A.ACT_RANGE_DIV, operand=2)]), dict(steps=[step(A.ACT_MOM_RANGE)]),
           dict(steps=[step(A.ACT_MOM)]), dict(steps=[step(A.ACT_MOM), step(A.ACT_MOM_ADD)]),
           dict(steps=[step(A.ACT_MOM), step(A.ACT_RANGE_CAT), step(A.ACT_MOM_RANGE)]),
           dict(steps=[step(A.ACT_MOM), step(A.ACT_MOM_ADD, ch=8), step(A.ACT_MOM_RANGE)]),
           dict(steps=[step(A.ACT_MOM), step(A.ACT_MOM_RELU, relu=0), step(A.ACT_MOM_RANGE)]),
           dict(steps=[step(A.ACT_RANGE), step(A.ACT_MOM_ADD)]), dict(steps=[step(A.ACT_RANGE), step(A.ACT_RANGE_DIV, operand=0)]),
           dict(steps=[step(A.ACT_CONST), step(A.ACT_RANGE_CAT)]),
           dict(steps=[step(A.ACT_RANGE, sw=0, sb=0)]), dict(steps=[step(A.ACT_RANGE, sw=2, sb=0)], sources=[src, src]),
           dict(steps=[step(A.ACT_RANGE, sw=1, sb=-1)], sources=[src, src]), dict(steps=[step(A.ACT_RANGE, ch=8, sw=1, sb=0)], sources=[src, src]),
           dict(steps=[step(A.ACT_RANGE)], sources=[Src(None, at(3), at(0), 16, 4, 1, 1)]),
           dict(steps=[step(A.ACT_RANGE)], sources=[Src(at(2), at(3), None, 16, 4, 1, 1)]),
           dict(steps=[step(A.ACT_RANGE)], sources=[Src(at(2), at(3), at(0), 0, 4, 1, 1)]),
           dict(steps=[step(A.ACT_RANGE)], sources=[Src(at(2), at(3), at(0), 16, 0, 1, 1)]),
           dict(steps=[step(A.ACT_RANGE)], sources=[Src(at(2), at(3), at(0), 16, 4, 0, 1)]),
           dict(steps=[step(A.ACT_RANGE)], sources=[Src(at(2), at(3), at(0), 16, 4, 1, 0)]),
           dict(steps=[step(A.ACT_RANGE)], sources=[Src(at(2), at(3), at(0), 16, 4, 1, 3)])]
    for kw in bad:
        assert create(**kw)[0] == DFQ_ERR_ARG, kw
        assert b'dfq_batch_act_plan_create' in lib.dfq_last_error(), kw
    plan = ctypes.c_void_p()
    assert lib.dfq_batch_act_plan_create(None, 1, None, 1, None, 0, bases, 2, ctypes.c_float(6.0), ctypes.c_float(1e-6), out.data_ptr(), 2,
                                         ctypes.byref(plan)) == DFQ_ERR_ARG
    assert lib.dfq_batch_act_plan_create((Res * 1)(Res(0, 1)), 1, (Step * 1)(step(A.ACT_RANGE)), 1, None, 1, bases, 2, ctypes.c_float(6.0),
                                         ctypes.c_float(1e-6), out.data_ptr(), 2, ctypes.byref(plan)) == DFQ_ERR_ARG      # sources null, count 1
    assert lib.dfq_batch_act_plan_create((Res * 1)(Res(0, 1)), 1, (Step * 1)(step(A.ACT_RANGE)), 1, None, 0, bases, 2, ctypes.c_float(6.0),
                                         ctypes.c_float(1e-6), out.data_ptr(), 2, None) == DFQ_ERR_ARG
    assert lib.dfq_batch_act_plan_run(None, None) == DFQ_ERR_ARG
    assert b'dfq_batch_act_plan_run' in lib.dfq_last_error()
    assert lib.dfq_batch_act_plan_launches(None) == 0
    lib.dfq_batch_act_plan_destroy(None)


def test_c_plan_on_hand_made_tables(engine):
    """the C layer on its own: the scalar steps in float64, rounded once (a third of a float32 sum is not a float32 third)"""
    lib = _ffi.lib()
    g = torch.Generator().manual_seed(11)
    host = torch.zeros(2, 1024)
    host[:, 0:300] = torch.rand(2, 300, generator=g) + 0.1         # gamma~ of A
    host[:, 320:620] = torch.randn(2, 300, generator=g) + 2.0      # beta~ of A (positive ranges)
    host[:, 640:680] = torch.rand(2, 40, generator=g) + 0.1
    host[:, 704:744] = torch.randn(2, 40, generator=g) + 1.0
    buf = host.to(engine.device).contiguous()
    out = torch.zeros(2, 4, dtype=torch.float32, device=engine.device)
    p0 = buf.data_ptr()
    bases = (ctypes.c_void_p * 2)(p0, p0 + 4 * 1024)
    A = _ffi
    S = A.DfqBatchActStep
    steps = [S(p0, p0 + 4 * 320, A.ACT_RANGE, 300, 0, 0, -1, -1, 0, 0), S(p0 + 4 * 640, p0 + 4 * 704, A.ACT_RANGE_ONE, 40, 0, 0, -1, -1, 0, 0),
             S(p0 + 4 * 640, p0 + 4 * 704, A.ACT_RANGE_ONE, 40, 0, 0, -1, -1, 0, 0), S(None, None, A.ACT_RANGE_DIV, 0, 0, 3, -1, -1, 0, 0),
             S(p0, p0 + 4 * 320, A.ACT_RANGE, 300, 2, 0, -1, -1, 0, 0)]
    res = [A.DfqBatchActResult(0, 4), A.DfqBatchActResult(4, 1)]
    plan = ctypes.c_void_p()
    _ffi.check(lib.dfq_batch_act_plan_create((A.DfqBatchActResult * 2)(*res), 2, (S * 5)(*steps), 5, None, 0, bases, 2, ctypes.c_float(6.0),
                                             ctypes.c_float(1e-6), out.data_ptr(), 4, ctypes.byref(plan)))
    try:
        assert lib.dfq_batch_act_plan_launches(plan) == 1
        _ffi.check(lib.dfq_batch_act_plan_run(plan, _ffi.stream_arg()))
        _ffi.synchronize()
    finally:
        lib.dfq_batch_act_plan_destroy(plan)
    six = torch.tensor(6.0)
    for n in range(2):
        wa, ba, wb, bb = host[n, 0:300], host[n, 320:620], host[n, 640:680], host[n, 704:744]
        lo_a, hi_a = float((ba - six * wa).min()), float((ba + six * wa).max())
        lo_b, hi_b = float((bb - six * wb).min()), float((bb + six * wb).max())
        vmin = (lo_a + max(0., lo_b) + max(0., lo_b)) / 3
        vmax = (hi_a + hi_b + hi_b) / 3
        want = torch.tensor([vmin, vmax, max(0., lo_a), min(6., hi_a)], dtype=torch.float32)
        assert torch.equal(_bits(out[n]), _bits(want)), (n, out[n].tolist(), want.tolist())
