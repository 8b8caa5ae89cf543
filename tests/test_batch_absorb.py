"""NetworkBatch.absorb_plan / dfq_batch_absorb_plan_*: bias_absorption (+ clip_weight) for every network of a batch in one plan.

Every weight, bias, fake_bias and shift vector must be bit-identical to what ``dfq.bias_absorption`` followed by
``dfq.clip_weight`` leaves on a twin of that network alone; networks of a batch must not see each other.  Floats are compared
as bit patterns (a zero of the other sign is a difference), on the CPU emulation and on the MI355X alike: nothing here folds
a min / max, so both engines are held to the same standard."""
import ctypes
import math

import numpy as np
import pytest
import torch

from dfq_amd import _ffi, arena, dfq, synthetic
from dfq_amd.utils import layer_transform as lt
from dfq_amd.utils import relation as rel

from common import TARG, compare_stage, load_stage, net_fixture, snapshot

DFQ_ERR_ARG = -1     # include/dfq_hip.h
CLIP = (-0.4, 0.25)  # far inside the default +-15 (which no synthetic weight reaches)
# per architecture, from the equalised weights' extremes: every network keeps a layer wholly inside and has weights outside
CLIP_OF = {'tiny_mobile': (-0.5, 0.5), 'tiny_res': (-0.5, 0.5), 'tiny_cat': (-2.0, 1.7)}


def _prepared(name, seed, device):
    model, graph, bottoms = synthetic.build(name, seed=seed)
    model.to(device)
    lt.merge_batchnorm(model, graph, bottoms, TARG)
    rels = rel.create_relation(graph, bottoms, TARG, delete_single=False)
    return model, graph, bottoms, rels


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and torch.equal(_bits(a), _bits(b.to(a.device)))


def _state(graph):
    """{name: tensor} of everything absorption and clipping may touch"""
    out = {}
    for k, m in graph.items():
        if type(m) in TARG:
            out[k + '.weight'] = m.weight
            if m.bias is not None:
                out[k + '.bias'] = m.bias
        elif isinstance(m, torch.nn.Module) and hasattr(m, 'fake_bias'):
            out[k + '.fake_weight'] = m.fake_weight
            out[k + '.fake_bias'] = m.fake_bias
    return out


def _twin(name, seed, graph, device):
    """a network of its own (own storages) in the state `graph` is in"""
    _, gt, bt, rt = _prepared(name, seed, device)
    with torch.no_grad():
        for k, m in graph.items():
            if type(m) in TARG and m.bias is not None and gt[k].bias is None:
                lt._ensure_bias(gt[k])
        src, dst = _state(graph), _state(gt)
        assert sorted(src) == sorted(dst)
        for k in src:
            dst[k].copy_(src[k])
    return gt, bt, rt


def _absorbed(graph, bottoms, rels):
    """indices into `rels` of the relations bias_absorption does not skip"""
    return [i for i, rr in enumerate(rels) if dfq._relu_between(graph, bottoms, rr.get_idxs()[1], rr.get_idxs()[0])]


def _shift(graph, rr, N):
    """c = max(0, beta~ - N gamma~) as the kernels form it: float32 product, float32 difference, one select"""
    bn = graph[rr.get_idxs()[2]]
    c = bn.fake_bias.detach() - torch.tensor(N, dtype=torch.float32, device=bn.fake_bias.device) * bn.fake_weight.detach()
    return torch.where(c < 0, torch.zeros_like(c), c)


def _plant(graph, bottoms, rels, N):
    """raise one proxy mean and lower another in every absorbed relation: a positive and a zero shift whatever the draw"""
    with torch.no_grad():
        for i in _absorbed(graph, bottoms, rels):
            bn = graph[rels[i].get_idxs()[2]]
            bn.fake_bias[0] = N * bn.fake_weight[0] + 0.75
            if bn.fake_bias.numel() > 1:
                bn.fake_bias[1] = -1.0


def _assert_equal(graph, gt, what):
    a, b = _state(graph), _state(gt)
    assert sorted(a) == sorted(b), what
    for k in a:
        assert _same(a[k], b[k]), '{}: {}'.format(what, k)


def _batch_and_twins(name, seeds, engine, N, reverse=False, equalise=True):
    nets = [_prepared(name, s, engine.device) for s in seeds]
    batch = arena.NetworkBatch([(g, b, r) for (_, g, b, r) in nets], TARG)
    if equalise:
        le = batch.le_plan()
        le.run()
        le.close()
        _ffi.synchronize()
    for (_, g, b, r) in nets:
        if reverse:
            r.reverse()          # (the equalisation wants graph order; the batch holds this very list, absorb_plan walks it)
        _plant(g, b, r, N)
    twins = [_twin(name, s, g, engine.device) for s, (_, g, _, _) in zip(seeds, nets)]
    if reverse:
        twins = [(g, b, r[::-1]) for (g, b, r) in twins]
    return nets, batch, twins


@pytest.mark.parametrize('name', ['tiny_mobile', 'tiny_res', 'tiny_cat'])
@pytest.mark.parametrize('N,clip,absorb', [(3, False, True), (0.5, False, True), (3, True, True), (0.5, True, True), (3, True, False)])
def test_batch_equals_per_network(engine, name, N, clip, absorb):
    seeds = [0, 1, 2, 3]
    clip = CLIP_OF[name] if clip else None
    nets, batch, twins = _batch_and_twins(name, seeds, engine, N)
    plan = batch.absorb_plan(N, clip, absorb)
    assert plan.launches == (2 if absorb else 1)
    for n, ((_, g, b, r), (gt, bt, rt)) in enumerate(zip(nets, twins)):
        idx = _absorbed(gt, bt, rt)
        want = {i: _shift(gt, rt[i], N) for i in idx} if absorb else {}
        if absorb:                                   # the case bites: a positive and a zero shift in every network
            assert idx and any((c > 0).any() for c in want.values()) and any((c == 0).any() for c in want.values())
        if clip is not None:                         # ... a weight outside the range, and a layer with none outside it
            out = [bool(((m.weight < clip[0]) | (m.weight > clip[1])).any()) for m in gt.values() if type(m) in TARG]
            assert any(out) and not all(out), out
        if n == 0:
            plan.run()
            _ffi.synchronize()
        if absorb:
            dfq.bias_absorption(gt, rt, bt, N)
        if clip is not None:
            dfq.clip_weight(gt, list(clip), TARG)
        _assert_equal(g, gt, '{} net {}'.format(name, n))
        got = plan.shifts(n)
        assert sorted(got) == sorted(want)
        for i in want:
            assert _same(got[i], want[i]), '{} net {}: shift of relation {}'.format(name, n, i)
    plan.close()


@pytest.mark.parametrize('reverse', [False, True])
def test_bias_updated_from_both_sides(engine, reverse):
    """a layer that is second of one absorbed relation and first of the next gets (b + wc) - c or (b - c) + wc, whichever
    the relations list says"""
    N = 0.5
    nets, batch, twins = _batch_and_twins('tiny_mobile', [0, 1, 2], engine, N, reverse=reverse)
    g0, b0, r0 = twins[0]
    idx = _absorbed(g0, b0, r0)
    firsts = {r0[i].get_idxs()[0]: i for i in idx}
    both = [(i, firsts[r0[i].get_idxs()[1]]) for i in idx if r0[i].get_idxs()[1] in firsts]     # (second of, first of)
    assert both, 'no layer is second of one absorbed relation and first of another'
    assert any((i < j) != reverse for (i, j) in both)
    plan = batch.absorb_plan(N)
    plan.run()
    _ffi.synchronize()
    for n, ((_, g, b, r), (gt, bt, rt)) in enumerate(zip(nets, twins)):
        hit = False
        for (i, j) in both:                          # both updates non-zero on one element
            key = rt[i].get_idxs()[1]
            w2 = gt[key].weight.detach()
            ci, cj = _shift(gt, rt[i], N), _shift(gt, rt[j], N)
            ipg = w2.shape[1]
            step = w2.shape[0] // (ci.numel() // ipg)
            ws = w2.reshape(w2.shape[0], ipg, -1).sum(-1)
            wc = torch.stack([(ws[o] * ci[(o // step) * ipg:(o // step + 1) * ipg]).sum() for o in range(w2.shape[0])])
            hit = hit or bool(((wc.abs() > 1e-6) & (cj > 0)).any())
        assert hit, 'net {}: no bias element with both updates'.format(n)
        dfq.bias_absorption(gt, rt, bt, N)
        _assert_equal(g, gt, 'net {} reverse={}'.format(n, reverse))
    plan.close()


def test_networks_are_independent(engine):
    N = 0.5
    runs = []
    for bump in (False, True):
        nets, batch, _ = _batch_and_twins('tiny_res', [0, 1, 2], engine, N)
        if bump:
            with torch.no_grad():
                g, b, r = nets[1][1:]
                for i in _absorbed(g, b, r):
                    g[r[i].get_idxs()[2]].fake_bias += 0.5
        batch.absorb(N, CLIP)
        runs.append([{k: v.detach().clone() for k, v in _state(g).items()} for (_, g, _, _) in nets])
        batch.release()
    for n in (0, 2):
        assert all(_same(runs[0][n][k], runs[1][n][k]) for k in runs[0][n]), n
    assert not all(_same(runs[0][1][k], runs[1][1][k]) for k in runs[0][1] if k.endswith('.bias'))


def test_full_sequence(engine):
    """le -> absorb (+ clip) -> bc -> quant on a batch against the per-network sequence (main_cls.py:149-181)"""
    seeds, N = [0, 1, 2], 0.5
    nets = [_prepared('tiny_mobile', s, engine.device) for s in seeds]
    twins = [_prepared('tiny_mobile', s, engine.device) for s in seeds]
    batch = arena.NetworkBatch([(g, b, r) for (_, g, b, r) in nets], TARG)
    le, ab, bc, qp = batch.le_plan(), batch.absorb_plan(N, CLIP), batch.bc_plan(), batch.quant_plan(8, 16, codes='int8')
    le.run()
    ab.run()
    bc.run(check=True)
    qp.run()
    _ffi.synchronize()
    for n, ((_, g, _, _), (_, gt, bt, rt)) in enumerate(zip(nets, twins)):
        dfq.cross_layer_equalization(gt, rt, TARG)
        dfq.bias_absorption(gt, rt, bt, N)
        dfq.clip_weight(gt, list(CLIP), TARG)
        dfq.bias_correction(gt, bt, TARG)
        _, codes = lt.quantize_targ_layer(gt, 8, 16, TARG, return_codes=True)[:2]
        for k, m in g.items():
            if type(m) in TARG:
                assert _same(m.weight, gt[k].weight), 'net {} {}: weight'.format(n, k)
                assert (m.bias is None) == (gt[k].bias is None) or gt[k].bias is None
                if gt[k].bias is not None:
                    assert _same(m.bias, gt[k].bias), 'net {} {}: bias'.format(n, k)
                assert torch.equal(qp.codes(n)[k].to(torch.int64), codes[k].to(torch.int64)), 'net {} {}: codes'.format(n, k)
    for p in (le, ab, bc, qp):
        p.close()


@pytest.mark.parametrize('name,seed', [('tiny_mobile', 1), ('tiny_cat', 3)])
def test_reference_fixture(engine, name, seed):
    """the state the unmodified reference left after bias_absorption(N=3), from its state after the equalisation"""
    gold = net_fixture(name, seed, '_abs')
    assert bool(gold['cfg'][0])
    nets = [_prepared(name, seed, engine.device) for _ in range(3)]
    batch = arena.NetworkBatch([(g, b, r) for (_, g, b, r) in nets], TARG)
    for (_, g, _, _) in nets:
        load_stage(g, gold, 'le')
    batch.check(thorough=True)
    batch.absorb(3)
    for n, (_, g, _, _) in enumerate(nets):
        compare_stage(snapshot(g), gold, 'abs', what='{} net {}'.format(name, n))


# ---- the C ABI on hand-made tensors ---------------------------------------------------------------------------------------

def _pad(n):
    return -(-n // 64) * 64


# (o1, in_per_group, o2, khkw)
GEOMETRY = [(70, 1, 70, 9), (8, 1, 16, 49), (7, 1, 7, 1), (12, 3, 8, 9), (40, 20, 6, 49), (64, 32, 4, 49), (66, 33, 4, 49),
            (63, 63, 5, 1), (64, 64, 5, 1), (65, 65, 5, 1), (1280, 1280, 3, 1), (130, 65, 6, 9), (70, 70, 3, 49), (10, 5, 4, 25)]


@pytest.mark.parametrize('clip', [None, (-0.5, 0.5)])
def test_geometry_edges_through_the_abi(engine, clip):
    """grouped and depthwise second layers, 1 / 9 / 25 / 49 taps, 1 .. 1280 input channels per group, rows that are no
    multiple of four floats; one relation per case plus a clip-only tensor with NaN, infinities and signed zeros, against
    dfq_bias_absorb and dfq_clamp on copies of every network"""
    lib = _ffi.lib()
    rng = np.random.default_rng(7)
    n_nets, N = 3, 0.5
    sizes, stride = [], 0
    for (o1, ipg, o2, khkw) in GEOMETRY:
        offs = {}
        for name, c in (('w2', o2 * ipg * khkw), ('b1', o1), ('b2', o2), ('fw', o1), ('fb', o1)):
            offs[name] = (stride, c)
            stride += _pad(c)
        sizes.append(offs)
    extra = (stride, 1027)
    stride += _pad(1027)
    host = rng.standard_normal((n_nets, stride)).astype(np.float32)
    for offs in sizes:
        o, c = offs['fw']
        host[:, o:o + c] = np.abs(host[:, o:o + c])
        o, c = offs['w2']
        host[:, o + 3] = -0.0
    o, c = extra
    host[:, o + 1], host[:, o + 2], host[:, o + 3], host[:, o + 4], host[:, o + 1026] = np.nan, np.inf, -np.inf, -0.0, 7.0
    buf = torch.from_numpy(host).to(engine.device)
    ref = buf.clone()
    # the per-network calls on the copy
    want_c = torch.zeros((n_nets, sum(_pad(g[0]) for g in GEOMETRY)), dtype=torch.float32, device=engine.device)
    rels, c_off = [], 0
    for (o1, ipg, o2, khkw), offs in zip(GEOMETRY, sizes):
        for n in range(n_nets):
            p = {k: ref[n, o:o + c] for k, (o, c) in offs.items()}
            c = p['fb'] - torch.tensor(N, dtype=torch.float32, device=engine.device) * p['fw']
            want_c[n, c_off:c_off + o1] = torch.where(c < 0, torch.zeros_like(c), c)
            _ffi.check(lib.dfq_bias_absorb(p['w2'].data_ptr(), o2, ipg, khkw, o1, p['b1'].data_ptr(), p['b2'].data_ptr(),
                                           p['fw'].data_ptr(), p['fb'].data_ptr(), ctypes.c_float(N), _ffi.stream_arg()))
        a = {k: buf[0, o:o + c].data_ptr() for k, (o, c) in offs.items()}
        rels.append(_ffi.DfqBatchAbsorbRelation(a['w2'], a['b1'], a['b2'], a['fw'], a['fb'], o2, ipg, khkw, o1, c_off))
        c_off += _pad(o1)
    clips = []
    if clip is not None:
        for offs in sizes + [{'w2': extra}]:
            o, c = offs['w2']
            clips.append(_ffi.DfqBatchAbsorbClip(buf[0, o:o + c].data_ptr(), c))
            for n in range(n_nets):
                _ffi.check(lib.dfq_clamp(ref[n, o:o + c].data_ptr(), c, ctypes.c_float(clip[0]), ctypes.c_float(clip[1]), _ffi.stream_arg()))
    shifts = torch.full((n_nets, c_off), -5.0, dtype=torch.float32, device=engine.device)
    bases = (ctypes.c_void_p * n_nets)(*[buf[n].data_ptr() for n in range(n_nets)])
    plan = ctypes.c_void_p()
    _ffi.check(lib.dfq_batch_absorb_plan_create(
        (_ffi.DfqBatchAbsorbRelation * len(rels))(*rels), len(rels),
        (_ffi.DfqBatchAbsorbClip * len(clips))(*clips) if clips else None, len(clips), bases, n_nets,
        ctypes.c_float(N), ctypes.c_float(clip[0] if clip else 0), ctypes.c_float(clip[1] if clip else 0),
        shifts.data_ptr(), c_off, ctypes.byref(plan)))
    assert lib.dfq_batch_absorb_plan_launches(plan) == 2
    a, c = ctypes.c_int64(), ctypes.c_int64()
    _ffi.check(lib.dfq_batch_absorb_plan_elements(plan, ctypes.byref(a), ctypes.byref(c)))
    assert a.value == sum(g[1] * g[2] * g[3] for g in GEOMETRY) and c.value == (1027 if clip else 0)
    _ffi.check(lib.dfq_batch_absorb_plan_run(plan, _ffi.stream_arg()))
    _ffi.synchronize()
    lib.dfq_batch_absorb_plan_destroy(plan)
    for gi, offs in enumerate(sizes + [{'w2': extra}]):
        for name, (o, c) in offs.items():
            for n in range(n_nets):
                assert _same(buf[n, o:o + c], ref[n, o:o + c]), 'case {} {} net {}'.format(gi, name, n)
    off = 0
    for (o1, _, _, _) in GEOMETRY:
        assert _same(shifts[:, off:off + o1], want_c[:, off:off + o1])
        assert bool((shifts[:, off + o1:off + _pad(o1)] == -5.0).all())           # the padding is nobody's
        off += _pad(o1)
    if clip is not None:
        o, c = extra
        got = buf[:, o:o + 5].cpu().numpy()
        assert np.isnan(got[:, 1]).all() and (got[:, 2] == clip[1]).all() and (got[:, 3] == clip[0]).all()
        assert np.signbit(got[:, 4]).all() and (got[:, 4] == 0).all()


def test_abi_rejects_bad_arguments(engine):
    lib = _ffi.lib()
    buf = torch.zeros(2 * 1024, dtype=torch.float32, device=engine.device)
    shifts = torch.zeros(2 * 64, dtype=torch.float32, device=engine.device)
    at = lambda i: buf.data_ptr() + 4 * 64 * i
    bases = (ctypes.c_void_p * 2)(buf.data_ptr(), buf.data_ptr() + 4 * 1024)

    def relation(w2=at(0), b1=at(4), b2=at(5), fw=at(6), fb=at(7), o2=8, ipg=4, khkw=9, o1=8, off=0):
        return _ffi.DfqBatchAbsorbRelation(w2, b1, b2, fw, fb, o2, ipg, khkw, o1, off)

    def create(rels=None, clips=(), n_nets=2, b=bases, N=3.0, lo=-1.0, hi=1.0, s=shifts.data_ptr(), stride=64):
        rels = [relation()] if rels is None else rels
        plan = ctypes.c_void_p()
        rc = lib.dfq_batch_absorb_plan_create(
            (_ffi.DfqBatchAbsorbRelation * len(rels))(*rels) if rels else None, len(rels),
            (_ffi.DfqBatchAbsorbClip * len(clips))(*clips) if clips else None, len(clips), b, n_nets,
            ctypes.c_float(N), ctypes.c_float(lo), ctypes.c_float(hi), s, stride, ctypes.byref(plan))
        n = lib.dfq_batch_absorb_plan_launches(plan) if rc == 0 else None
        if rc == 0:
            lib.dfq_batch_absorb_plan_destroy(plan)
        return rc, n

    clip = _ffi.DfqBatchAbsorbClip
    second = dict(w2=at(8), b1=at(12), b2=at(13), fw=at(14), fb=at(15), off=8)
    assert create() == (0, 2)
    assert create(clips=[clip(at(0), 288)]) == (0, 2)
    assert create(rels=[], clips=[clip(at(0), 288)], s=None, stride=0) == (0, 1)
    assert create(rels=[], s=None, stride=0) == (0, 0)                  # nothing to do is legal and launches nothing
    assert create(rels=[relation(), relation(**second)]) == (0, 2)
    assert create(rels=[relation(), relation(**dict(second, b1=at(5)))]) == (0, 2)      # a chain: second of one, first of the next
    bad = [dict(rels=[relation(w2=None)]), dict(rels=[relation(b1=None)]), dict(rels=[relation(b2=None)]),
           dict(rels=[relation(fw=None)]), dict(rels=[relation(fb=None)]), dict(rels=[relation(o2=0)]),
           dict(rels=[relation(ipg=0)]), dict(rels=[relation(khkw=0)]), dict(rels=[relation(o1=0)]),
           dict(rels=[relation(ipg=3)]), dict(rels=[relation(o1=12, o2=8)]), dict(rels=[relation(khkw=4000)]),
           dict(rels=[relation(off=-1)]), dict(rels=[relation(off=57)]), dict(N=math.nan), dict(N=math.inf),
           dict(clips=[clip(at(0), 288)], lo=1.0, hi=-1.0), dict(clips=[clip(at(0), 288)], lo=math.nan),
           dict(clips=[clip(at(0), 287)]), dict(clips=[clip(None, 10)]), dict(clips=[clip(at(20), 0)]),
           dict(clips=[clip(at(20), 10), clip(at(20), 10)]), dict(n_nets=0), dict(b=None),
           dict(b=(ctypes.c_void_p * 2)(buf.data_ptr(), None)), dict(s=None), dict(stride=0),
           dict(rels=[relation(), relation(**dict(second, off=4))]), dict(rels=[relation(), relation(**dict(second, w2=at(0)))]),
           dict(rels=[relation(), relation(**dict(second, b2=at(5)))]), dict(rels=[relation(), relation(**dict(second, b1=at(4)))]),
           dict(rels=[relation(), relation(**dict(second, fb=at(7)))]),
           dict(rels=[relation(), relation(**dict(second, b1=at(5), o1=4, ipg=4))])]
    for kw in bad:
        assert create(**kw)[0] == DFQ_ERR_ARG, kw
        assert b'dfq_batch_absorb_plan_create' in lib.dfq_last_error(), kw
    assert lib.dfq_batch_absorb_plan_run(None, None) == DFQ_ERR_ARG
    assert b'dfq_batch_absorb_plan_run' in lib.dfq_last_error()
    assert lib.dfq_batch_absorb_plan_elements(None, None, None) == DFQ_ERR_ARG
    assert lib.dfq_batch_absorb_plan_launches(None) == 0


def test_absorb_plan_rejects_bad_arguments(engine):
    nets = [_prepared('tiny_mobile', s, engine.device) for s in (0, 1)]
    batch = arena.NetworkBatch([(g, b, r) for (_, g, b, r) in nets], TARG)
    for kw in [dict(N='three'), dict(N=None), dict(N=math.nan), dict(N=math.inf), dict(N=True), dict(range_clip=(1, -1)),
               dict(range_clip=(0.5,)), dict(range_clip=(-1, 0, 1)), dict(range_clip=5), dict(range_clip=(math.nan, 1)),
               dict(range_clip=('a', 'b'))]:
        with pytest.raises(ValueError):
            batch.absorb_plan(**kw)
    p = batch.absorb_plan(absorb=False)                 # nothing to do: legal, launches nothing
    assert p.launches == 0 and p.shifts(0) == {}
    p.run()
    p.close()
    with pytest.raises(RuntimeError, match='closed'):
        p.run()
    p = batch.absorb_plan(3.0, [-1, 1])
    assert p.launches == 2 and p.absorbed_elements > 0 and p.clip_only_elements > 0
    batch.release()
    with pytest.raises(RuntimeError, match='released'):
        batch.absorb_plan()
    with pytest.raises(RuntimeError, match='released'):
        p.run()
    p.close()


def test_a_missing_bias_slot_is_refused(engine):
    nets = [_prepared('tiny_mobile', s, engine.device) for s in (0, 1)]
    batch = arena.NetworkBatch([(g, b, r) for (_, g, b, r) in nets], TARG)
    g, b, r = nets[0][1:]
    key = r[_absorbed(g, b, r)[0]].get_idxs()[1]
    g[key].bias = None
    before = batch.storage.clone()
    with pytest.raises(ValueError, match=key):
        batch.absorb_plan()
    batch.absorb_plan(absorb=False, range_clip=CLIP).close()         # the clip does not need it
    assert _same(batch.storage, before)


@pytest.mark.parametrize('moved', ['weight', 'bias', 'fake_bias'])
def test_a_tensor_that_left_its_slot_is_refused(engine, moved):
    nets = [_prepared('tiny_mobile', s, engine.device) for s in (0, 1, 2)]
    batch = arena.NetworkBatch([(g, b, r) for (_, g, b, r) in nets], TARG)
    g, b, r = nets[0][1:]
    idx = _absorbed(g, b, r)
    kf, ks, kb = r[idx[len(idx) // 2]].get_idxs()
    if moved == 'fake_bias':
        g[kb].fake_bias = g[kb].fake_bias.clone()
    else:
        t = getattr(g[ks], moved)
        t.data = t.data.clone()
    batch.check()                                     # (the quick check does not see a middle slot)
    before = batch.storage.clone()
    with pytest.raises(RuntimeError, match='no longer lives in its slot'):
        batch.absorb_plan(3, CLIP)
    with pytest.raises(RuntimeError, match='no longer lives in its slot'):
        batch.absorb(0.5)
    _ffi.synchronize()
    assert _same(batch.storage, before)               # nothing was written anywhere


# ---- full size, on the MI355X -----------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_batch_of_64_mobilenet_v2():
    dev = torch.device('cuda', 0)
    N, clip = 0.5, (-0.3, 0.3)
    nets = [_prepared('mobilenet_v2', s % 4, dev) for s in range(64)]
    batch = arena.NetworkBatch([(g, b, r) for (_, g, b, r) in nets], TARG)
    le = batch.le_plan()
    le.run()
    le.close()
    torch.cuda.synchronize()
    picks = (0, 17, 42, 63)
    twins = {n: _twin('mobilenet_v2', n % 4, nets[n][1], dev) for n in picks}
    plan = batch.absorb_plan(N, clip)
    assert plan.launches == 2
    plan.run()
    torch.cuda.synchronize()
    for n, (gt, bt, rt) in twins.items():
        idx = _absorbed(gt, bt, rt)
        want = {i: _shift(gt, rt[i], N) for i in idx}
        assert len(idx) == 35 and any((c > 0).any() for c in want.values()) and any((c == 0).any() for c in want.values())
        out = [bool(((m.weight < clip[0]) | (m.weight > clip[1])).any()) for m in gt.values() if type(m) in TARG]
        assert any(out)
        dfq.bias_absorption(gt, rt, bt, N)
        dfq.clip_weight(gt, list(clip), TARG)
        _assert_equal(nets[n][1], gt, 'mobilenet_v2 net {}'.format(n))
        got = plan.shifts(n)
        assert all(_same(got[i], want[i]) for i in want) and sorted(got) == sorted(want)
    plan.close()
    batch.release()
