"""Bias correction at each layer's own bit width: ``BCPlan.run(widths=)`` (dfq_bc_plan_run_widths, include/dfq_hip.h).

The oracle is built the way tests/test_per_channel.py builds its own: ``orc.bias_correction`` calls ``quant_error_rowsum``
through its module, so patching that one function with a closure that quantises each layer at THAT layer's width -- per tensor or
per row, the widths handed over in the order the oracle visits the layers -- turns the whole reference correction (E[x], matvec,
bias / beta~ updates, chain order) into the widths reference.  Ranges skip NaN (the rule of include/dfq_hip.h, "Special values").

Tolerances are the project's: weights and fake_weight bit-exact, biases and beta~ ``assert_close`` (the 1e-5 contract),
materialised eps bit-exact."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import dfq_oracle as orc
from oracle import graphspec
from dfq_amd import _ffi, arena, dfq, synthetic
from dfq_amd.utils import layer_transform as lt
from dfq_amd.utils import relation as rel

from common import F32, TARG, assert_bitexact, assert_close, load_inputs, load_stage, net_fixture, npy, snapshot

ERR_ARG = -1                 # DFQ_ERR_ARG (include/dfq_hip.h)
GOLDEN_NETS = {'tiny_mobile': 0, 'tiny_res': 0, 'tiny_cat': 0}
CYCLE = (2, 3, 4, 6, 8)      # step i of a network gets CYCLE[i % 5]: neighbouring steps differ
WIDTHS = (2, 3, 4, 6, 8)     # the candidates of the mixed plans
BATCH_SEEDS = (0, 1, 2)      # chosen on the CPU emulation: test_batch_widths_from_the_device asserts what they must give


# ---- the oracle -----------------------------------------------------------------------------------------------------------------

def _range(a):
    """(min, max) with NaN skipped; the identities for nothing but NaN"""
    v = a[~np.isnan(a)]
    return (float(v.min()), float(v.max())) if v.size else (float('inf'), float('-inf'))


def _rowsum_at(weight, bits, signed, per_channel):
    """eps.view(O, I, -1).sum(-1) with the tensor (or row o) quantised by its own (min, max) at `bits` bits"""
    w = np.asarray(weight, dtype=F32)
    eps = np.empty_like(w)
    if per_channel:
        for o in range(w.shape[0]):
            mn, mx = _range(w[o])
            eps[o] = (orc.uniform_quantize(w[o], bits, mn, mx, signed) - w[o]).astype(F32)
    else:
        mn, mx = _range(w)
        eps = (orc.uniform_quantize(w, bits, mn, mx, signed) - w).astype(F32)
    e3 = eps.reshape(w.shape[0], w.shape[1], -1)
    acc = np.zeros(e3.shape[:2], dtype=F32)
    for k in range(e3.shape[2]):
        acc = (acc + e3[:, :, k]).astype(F32)
    return acc


def _rowsum_widths(widths, per_channel):
    """the closure: call j quantises at widths[j] (the oracle visits the layers in the order of the plan's steps)"""
    todo = list(widths)

    def rowsum(weight, signed=False, num_bits=8):
        return _rowsum_at(weight, todo.pop(0), signed, per_channel)
    rowsum.todo = todo
    return rowsum


def _oracle(graph, bottoms, monkeypatch, widths, signed, per_channel, collect=None):
    """widths: one per step, in step order; None: the reference as it is (8 bits per tensor)"""
    spec = graphspec.from_torch(graph, bottoms, TARG)
    with monkeypatch.context() as m:
        if widths is not None:
            fn = _rowsum_widths(widths, per_channel)
            m.setattr(orc, 'quant_error_rowsum', fn)
        orc.bias_correction(spec, signed=signed, collect=collect)
        if widths is not None:
            assert not fn.todo, 'the oracle visited fewer layers than the plan has steps'
    return spec


def _spec_snapshot(spec):
    snap = {}
    for i, k in enumerate(spec.order):
        n = spec.nodes[k]
        if n.kind == 'targ':
            snap['L{}.w'.format(i)] = n.weight
            if n.bias is not None:
                snap['L{}.b'.format(i)] = n.bias
        elif n.kind == 'bn' and n.fake_weight is not None:
            snap['L{}.fw'.format(i)] = n.fake_weight
            snap['L{}.fb'.format(i)] = n.fake_bias
    return snap


def _match(graph, spec, what=''):
    osnap, esnap = _spec_snapshot(spec), snapshot(graph)
    assert set(osnap) <= set(esnap)
    for k in osnap:
        if k.endswith('.w') or k.endswith('.fw'):
            assert_bitexact(esnap[k], osnap[k], what + k)
        else:
            keep = ~np.isnan(osnap[k])
            assert np.array_equal(~np.isnan(esnap[k]), keep), what + k + ': NaN in other places'
            assert_close(esnap[k][keep], osnap[k][keep], what + k)


def _same(graph, want, what=''):
    for k, v in snapshot(graph).items():
        assert_bitexact(v, want[k], what + k)


def _load(graph, snap):
    with torch.no_grad():
        for i, k in enumerate(graph):
            m = graph[k]
            if 'L{}.w'.format(i) in snap:
                m.weight.copy_(torch.from_numpy(snap['L{}.w'.format(i)]))
                if m.bias is not None:
                    m.bias.copy_(torch.from_numpy(snap['L{}.b'.format(i)]))
            if 'L{}.fb'.format(i) in snap:
                m.fake_weight.copy_(torch.from_numpy(snap['L{}.fw'.format(i)]))
                m.fake_bias.copy_(torch.from_numpy(snap['L{}.fb'.format(i)]))


def _ensure_biases(graph):
    for k in graph:
        if type(graph[k]) in TARG:
            dfq._ensure_bias(graph[k])


def _net(name, engine, seed=0):
    """(model, graph, bottoms) after BN folding, in the state the correction starts from (tests/test_per_channel.py)"""
    if name in GOLDEN_NETS and seed == GOLDEN_NETS[name]:
        gold = net_fixture(name, seed, '')
        model, graph, bottoms = synthetic.build(name, seed=seed)
        load_inputs(graph, gold, 'cpu')
        model.to(engine.device)
        lt.merge_batchnorm(model, graph, bottoms, TARG)
        load_stage(graph, gold, 'abs')
    else:
        model, graph, bottoms = synthetic.build(name, seed=seed)
        model.to(engine.device)
        lt.merge_batchnorm(model, graph, bottoms, TARG)
    _ensure_biases(graph)
    return model, graph, bottoms


def _cyclic(keys):
    return {k: CYCLE[i % len(CYCLE)] for i, k in enumerate(keys)}


def _max_bias_gap(a, b):
    sa, sb = _spec_snapshot(a), _spec_snapshot(b)
    return max(float(np.abs(sa[k].astype(np.float64) - sb[k]).max()) for k in sa if k.endswith('.b'))


# ---- 1. against the oracle, a width per layer -------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['tiny_mobile', 'tiny_res', 'tiny_cat', 'tiny_wide'])
@pytest.mark.parametrize('per_channel', [False, True])
@pytest.mark.parametrize('signed', [False, True])
def test_widths_per_layer_against_oracle(engine, monkeypatch, name, per_channel, signed):
    model, graph, bottoms = _net(name, engine)
    plan, keys = dfq.build_bc_plan(graph, bottoms, TARG)
    wmap = _cyclic(keys)
    spec = _oracle(graph, bottoms, monkeypatch, [wmap[k] for k in keys], signed, per_channel)
    # what keeps the test honest: a run that ignored the widths would be the same oracle at a uniform 8 bits
    spec8 = _oracle(graph, bottoms, monkeypatch, [8] * len(keys), signed, per_channel)
    gap = _max_bias_gap(spec, spec8)
    print('{} per_channel={} signed={}: widths oracle vs uniform 8 bits, largest bias gap {:.3e}'.format(name, per_channel, signed, gap))
    assert gap > 1e-3, 'the widths change no bias by more than 1e-3 ({:.3e}): the test shows nothing'.format(gap)
    plan.run(signed=signed, check=True, per_channel=per_channel, widths=wmap)
    assert plan.repeated == 0
    plan.close()
    _match(graph, spec, '{} per_channel={} signed={}: '.format(name, per_channel, signed))


# ---- 2. eps bit for bit -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name,per_channel,signed', [('tiny_res', False, False), ('tiny_mobile', True, True), ('tiny_wide', False, True),
                                                     ('tiny_wide', True, False)])
def test_eps_and_corrections_at_widths(engine, monkeypatch, name, per_channel, signed):
    """DFQ_BC_EPS=1: the materialised row sums are the patched oracle's bit for bit, the corrections within 1e-5."""
    monkeypatch.setenv('DFQ_BC_EPS', '1')
    model, graph, bottoms = _net(name, engine)
    plan, keys = dfq.build_bc_plan(graph, bottoms, TARG)
    wmap = _cyclic(keys)
    collect = {}
    _oracle(graph, bottoms, monkeypatch, [wmap[k] for k in keys], signed, per_channel, collect=collect)
    plan.run(signed=signed, check=True, per_channel=per_channel, widths=wmap)
    assert keys == list(collect.keys())
    for step, k in enumerate(keys):
        e = npy(plan.eps(step))
        assert_bitexact(e, collect[k]['eps'].reshape(e.shape), 'eps of {} at {} bits'.format(k, wmap[k]))
        assert_close(npy(plan.correction(step)), collect[k]['bias'].reshape(-1), 'correction of {}'.format(k))
    plan.close()


# ---- 3. the new path equals the old ones where they meet ----------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['tiny_mobile', 'tiny_cat'])
@pytest.mark.parametrize('signed', [False, True])
def test_widths_meet_the_existing_modes(engine, name, signed):
    """run(widths=8) is run(); run(per_channel=True, widths=b) is run(per_channel=True, bits=b): every bias and beta~ bit for bit."""
    model, graph, bottoms = _net(name, engine)
    start = snapshot(graph)
    plan, _ = dfq.build_bc_plan(graph, bottoms, TARG)
    plan.run(signed=signed, check=True)
    want = snapshot(graph)
    _load(graph, start)
    plan.run(signed=signed, check=True, widths=8)
    _same(graph, want, 'widths=8 vs run(): ')
    for b in (4, 6, 8):
        _load(graph, start)
        plan.run(signed=signed, check=True, per_channel=True, bits=b)
        want = snapshot(graph)
        _load(graph, start)
        plan.run(signed=signed, check=True, per_channel=True, widths=b)
        _same(graph, want, 'per channel, widths={0} vs bits={0}: '.format(b))
    plan.close()


# ---- 4. protocol matrix ---------------------------------------------------------------------------------------------------------------

PROTOCOLS = [                                             # (restated from tests/test_per_channel.py)
    {},                                                   # the default (tagged; one launch where the plan picks it)
    {'DFQ_BC_TAGGED': '0'},                               # counters
    {'DFQ_BC_MERGED': '0'},                               # one launch per chain position
    {'DFQ_BC_FOLD': '0'},
    {'DFQ_BC_ONE_LAUNCH': '1'},
    {'DFQ_BC_ONE_LAUNCH': '0'},
    {'DFQ_GRAPH': '1'},
    {'DFQ_BC_ONE_LAUNCH': '1', 'DFQ_BC_FOLD': '0', 'DFQ_BC_TAGGED': '0'},
]


@pytest.mark.parametrize('name', ['tiny_mobile', 'tiny_cat'])
@pytest.mark.parametrize('per_channel', [False, True])
def test_protocol_matrix_at_widths(engine, monkeypatch, name, per_channel):
    """Every hand-over protocol gives the default's bits with a width per layer (two runs per plan: the second run of a tagged
    plan uses the other parities and epoch); the default matches the oracle."""
    model, graph, bottoms = _net(name, engine)
    start = snapshot(graph)
    ref = None
    for env in PROTOCOLS:
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            plan, keys = dfq.build_bc_plan(graph, bottoms, TARG)
            wmap = _cyclic(keys)
            for _ in range(2):
                _load(graph, start)
                plan.run(signed=True, check=True, per_channel=per_channel, widths=wmap)
            assert plan.repeated == 0
            plan.close()
        if ref is None:
            ref = snapshot(graph)
            got = snapshot(graph)
            _load(graph, start)
            spec = _oracle(graph, bottoms, monkeypatch, [wmap[k] for k in keys], True, per_channel)
            _load(graph, got)
            _match(graph, spec, 'default: ')
            continue
        _same(graph, ref, '{}: '.format(env))


def test_safe_mode_and_modes_alternate_at_widths(engine, monkeypatch):
    """One plan: widths runs alternate with run() and run(per_channel=True), the last ones in safe mode; each run matches its own
    oracle."""
    model, graph, bottoms = _net('tiny_mobile', engine)
    start = snapshot(graph)
    plan, keys = dfq.build_bc_plan(graph, bottoms, TARG)
    wmap = _cyclic(keys)
    order = [wmap[k] for k in keys]
    for mode, per_channel, safe in [('widths', False, False), ('plain', False, False), ('widths', True, False), ('plain', True, False),
                                    ('widths', False, True), ('plain', True, True), ('widths', True, True), ('plain', False, True)]:
        _load(graph, start)
        if safe:
            plan.set_safe_mode()
            assert not plan.has_waits
        if mode == 'widths':
            spec = _oracle(graph, bottoms, monkeypatch, order, False, per_channel)
            plan.run(check=True, per_channel=per_channel, widths=wmap)
        else:
            spec = _oracle(graph, bottoms, monkeypatch, [8] * len(keys) if per_channel else None, False, per_channel)
            plan.run(check=True, per_channel=per_channel, bits=8)
        _match(graph, spec, '{} per_channel={} safe={}: '.format(mode, per_channel, safe))
    plan.close()


# ---- 5. a batch, the widths read on the device ---------------------------------------------------------------------------------------

def _batch(engine, seeds):
    nets = [_net('tiny_mobile', engine, seed=s) for s in seeds]
    batch = arena.NetworkBatch([(g, b, rel.create_relation(g, b, TARG)) for (_, g, b) in nets], TARG)
    return nets, batch


@pytest.mark.parametrize('per_channel', [False, True])
@pytest.mark.parametrize('signed', [False, True])
def test_batch_widths_from_the_device(engine, monkeypatch, per_channel, signed):
    """mixed_plan(apply=False) leaves a width per (network, layer) on the device; bc_plan().run(widths=that plan) corrects every
    network at ITS widths: each matches the oracle run with its own bits, and is bit-equal to the network corrected alone."""
    nets, batch = _batch(engine, BATCH_SEEDS)
    starts = [snapshot(g) for (_, g, _) in nets]
    mixed = batch.mixed_plan(WIDTHS, avg_bits=4.5, apply=False, per_channel=per_channel, signed=signed)
    mixed.run()
    plan = batch.bc_plan()
    plan.run(signed=signed, check=True, per_channel=per_channel, widths=mixed)
    assert plan.repeated == 0
    bits = [mixed.bits(n) for n in range(len(nets))]
    keys = plan.keys
    assert keys == dfq.build_bc_plan(nets[0][1], nets[0][2], TARG)[1]
    # what the seeds must give (chosen on the CPU emulation): mixed widths inside every network, and between networks
    for n, b in enumerate(bits):
        assert len({b[k] for k in keys}) >= 2, 'network {} got one width for every corrected layer'.format(n)
    assert any(len({b[k] for b in bits}) >= 2 for k in keys), 'every network got the same widths: the stride shows nothing'
    got = [snapshot(g) for (_, g, _) in nets]
    for n, (_, graph, bottoms) in enumerate(nets):
        for k in got[n]:
            if k.endswith('.w'):
                assert_bitexact(got[n][k], starts[n][k], 'allocation and correction write no weight: net {} {}'.format(n, k))
        _load(graph, starts[n])
        spec = _oracle(graph, bottoms, monkeypatch, [bits[n][k] for k in keys], signed, per_channel)
        _load(graph, got[n])
        _match(graph, spec, 'net {}: '.format(n))
    plan.close()
    mixed.close()
    batch.release()
    # batch-independence: network n corrected alone
    for n, seed in enumerate(BATCH_SEEDS):
        (one,), solo = _batch(engine, (seed,))
        m1 = solo.mixed_plan(WIDTHS, avg_bits=4.5, apply=False, per_channel=per_channel, signed=signed)
        m1.run()
        p1 = solo.bc_plan()
        p1.run(signed=signed, check=True, per_channel=per_channel, widths=m1)
        assert m1.bits(0) == bits[n]
        _same(one[1], got[n], 'net {} alone vs in the batch: '.format(n))
        p1.close()
        m1.close()
        solo.release()


# ---- 6. quantize_mixed(correct=True) -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('per_channel,signed', [(False, False), (True, True)])
def test_quantize_mixed_correct(engine, monkeypatch, per_channel, signed):
    """correct=True: bits, codes, weights and ranges are those of correct=False (the correction writes no weight, so the applying
    plan allocates what the allocating one did); beta~ is the oracle's at those bits; the biases are ``quantize``'s rule -- per
    tensor, asymmetric, 16 bits, the tensor's own (min, max) -- applied to the corrected biases.

    How the biases are compared: the corrected bias b~ carries the correction's 1e-5 contract, and a 16-bit rounding of two
    values 1e-5 apart may fall on neighbouring codes, one quantum q = (max - min) / 65535 apart.  So (a) a twin batch that stops
    behind the correction gives b~ itself, which is the oracle's within ``assert_close``, (b) the stored bias is Q(b~) of THAT b~
    bit for bit, and (c) against Q(oracle's bias) it lies within one quantum plus the contract."""
    kw = dict(avg_bits=4.5, per_channel=per_channel, signed=signed)
    nets, batch = _batch(engine, BATCH_SEEDS[:2])
    codes0, ranges0, bits0 = batch.quantize_mixed(WIDTHS, **kw)
    w0 = [snapshot(g) for (_, g, _) in nets]
    batch.release()
    # the twin: allocation and correction only
    twins, tbatch = _batch(engine, BATCH_SEEDS[:2])
    starts = [snapshot(g) for (_, g, _) in twins]
    mixed = tbatch.mixed_plan(WIDTHS, apply=False, **kw)
    mixed.run()
    plan = tbatch.bc_plan()
    plan.run(signed=signed, check=True, per_channel=per_channel, widths=mixed)
    alloc = [dict(mixed.bits(n)) for n in range(2)]
    keys = plan.keys
    corrected = [snapshot(g) for (_, g, _) in twins]
    plan.close()
    mixed.close()
    tbatch.release()
    nets, batch = _batch(engine, BATCH_SEEDS[:2])
    codes1, ranges1, bits1 = batch.quantize_mixed(WIDTHS, correct=True, **kw)
    assert bits1 == bits0 == alloc, 'the applying plan must allocate what the allocating plan did'
    for n, (_, graph, bottoms) in enumerate(nets):
        got = snapshot(graph)
        for k in codes0[n]:
            assert torch.equal(codes1[n][k].cpu(), codes0[n][k].cpu()), 'codes of net {} {}'.format(n, k)
        for k in ranges0[n]:
            if not k.endswith('.bias'):
                assert_bitexact(npy(ranges1[n][k]), npy(ranges0[n][k]), 'range of net {} {}'.format(n, k))
        _load(graph, starts[n])
        spec = _oracle(graph, bottoms, monkeypatch, [alloc[n][k] for k in keys], signed, per_channel)
        _load(graph, got)
        osnap = _spec_snapshot(spec)
        for k, v in got.items():
            if k.endswith('.w'):
                assert_bitexact(v, w0[n][k], 'weight of net {} {}'.format(n, k))
            elif k.endswith('.fw') or k.endswith('.fb'):
                assert_bitexact(v, corrected[n][k], 'net {} {} vs the twin'.format(n, k))
                (assert_bitexact if k.endswith('.fw') else assert_close)(v, osnap[k], 'net {} {} vs the oracle'.format(n, k))
            else:
                b = corrected[n][k]
                assert_close(b, osnap[k], 'corrected bias of net {} {}'.format(n, k))
                assert_bitexact(v, orc.uniform_quantize(b, 16, float(b.min()), float(b.max()), False), 'net {} {}: Q(b~)'.format(n, k))
                ob = osnap[k]
                want = orc.uniform_quantize(ob, 16, float(ob.min()), float(ob.max()), False)
                q = (float(ob.max()) - float(ob.min())) / 65535.0
                assert float(np.abs(v.astype(np.float64) - want).max()) <= q + 1e-5 * max(1.0, float(np.abs(ob).max())), k
    batch.release()
    # dfq.bias_correction(graph, ..., widths={key: bits}) on one network equals the batch of one
    (one,), solo = _batch(engine, BATCH_SEEDS[:1])
    p1 = solo.bc_plan()
    p1.run(signed=signed, check=True, per_channel=per_channel, widths=alloc[0])
    want = snapshot(one[1])
    p1.close()
    solo.release()
    model, graph, bottoms = _net('tiny_mobile', engine, seed=BATCH_SEEDS[0])
    dfq.bias_correction(graph, bottoms, TARG, signed=signed, per_channel=per_channel, widths=alloc[0])
    _same(graph, want, 'bias_correction(widths=) vs the batch of one: ')
    _same(graph, corrected[0], 'bias_correction(widths=) vs the batch of two: ')


def test_plan_cache_keeps_widths_apart(engine, monkeypatch):
    """bias_correction on one graph: per-tensor, widths, per-channel, per-channel widths, per-tensor -- each matches its own oracle."""
    model, graph, bottoms = _net('tiny_res', engine)
    start = snapshot(graph)
    keys = dfq.build_bc_plan(graph, bottoms, TARG)[1]
    wmap = _cyclic(keys)
    for per_channel, widths in [(False, None), (False, wmap), (True, None), (True, wmap), (False, 4), (False, None)]:
        _load(graph, start)
        order = [widths] * len(keys) if isinstance(widths, int) else [wmap[k] for k in keys] if widths else ([4] * len(keys) if per_channel else None)
        spec = _oracle(graph, bottoms, monkeypatch, order, False, per_channel)
        dfq.bias_correction(graph, bottoms, TARG, bits_weight=4, per_channel=per_channel, widths=widths)
        _match(graph, spec, 'per_channel={} widths={}: '.format(per_channel, widths))


# ---- 7. refusals and special values ---------------------------------------------------------------------------------------------------

def test_refusals(engine):
    model, graph, bottoms = _net('tiny_mobile', engine)
    start = snapshot(graph)
    plan, keys = dfq.build_bc_plan(graph, bottoms, TARG)
    lib = _ffi.lib()
    for bad in (1, 17, 0, -3, True, 8.0):
        with pytest.raises(ValueError):
            plan.run(widths=bad)
        with pytest.raises(ValueError):
            dfq.bias_correction(graph, bottoms, TARG, widths=bad)
    for bits in (1, 17):
        assert lib.dfq_bc_plan_run_widths(plan._plan, 0, 0, None, 0, None, bits, None) == ERR_ARG
        assert lib.dfq_last_error()
    wmap = _cyclic(keys)
    missing = dict(wmap)
    del missing[keys[1]]
    with pytest.raises(ValueError, match=repr(keys[1])):
        plan.run(widths=missing)
    with pytest.raises(ValueError):
        dfq.bias_correction(graph, bottoms, TARG, widths=missing)
    for bad in (1, 17, 4.0, True):
        with pytest.raises(ValueError):
            plan.run(widths=dict(wmap, **{keys[0]: bad}))
    # the C ABI: device widths without an index table, a negative index, a negative stride, a null plan
    dev = torch.tensor([wmap[k] for k in keys], dtype=torch.int32, device=engine.device)
    index = (ctypes.c_int32 * len(keys))(*range(len(keys)))
    assert lib.dfq_bc_plan_run_widths(plan._plan, 0, 0, dev.data_ptr(), 0, None, 8, None) == ERR_ARG
    assert lib.dfq_last_error()
    assert lib.dfq_bc_plan_run_widths(plan._plan, 0, 0, dev.data_ptr(), -1, index, 8, None) == ERR_ARG
    index[2] = -1
    assert lib.dfq_bc_plan_run_widths(plan._plan, 0, 0, dev.data_ptr(), 0, index, 8, None) == ERR_ARG
    assert lib.dfq_bc_plan_run_widths(None, 0, 0, None, 0, None, 8, None) == ERR_ARG
    # the Python form of it: an index table that is too short, reaches outside the tensor, or widths of another type / device
    with pytest.raises(ValueError):
        plan.run(widths=(dev, list(range(len(keys) - 1))))
    with pytest.raises(ValueError):
        plan.run(widths=(dev, [len(keys)] * len(keys)))
    with pytest.raises(ValueError):
        plan.run(widths=(dev.to(torch.int64), list(range(len(keys)))))
    with pytest.raises(ValueError):
        plan.run(widths='8')
    plan.close()
    _same(graph, start, 'untouched after the rejected calls: ')
    # a mixed plan whose per_channel / signed differ from the run's, or that covers another number of networks
    nets, batch = _batch(engine, BATCH_SEEDS[:2])
    mixed = batch.mixed_plan(WIDTHS, avg_bits=4.5, apply=False, per_channel=False, signed=True)
    mixed.run()
    bplan = batch.bc_plan()
    for kw in (dict(per_channel=True, signed=True), dict(per_channel=False, signed=False)):
        with pytest.raises(ValueError):
            bplan.run(widths=mixed, **kw)
    (one,), solo = _batch(engine, BATCH_SEEDS[:1])
    splan = solo.bc_plan()
    with pytest.raises(ValueError):
        splan.run(widths=mixed, signed=True)
    bplan.run(widths=mixed, signed=True, check=True)
    for p in (splan, bplan, mixed):
        p.close()
    solo.release()
    batch.release()


@pytest.mark.parametrize('per_channel', [False, True])
def test_device_widths_are_clamped(engine, per_channel):
    """A width of 0 or 40 read on the device behaves as 2 or 16."""
    model, graph, bottoms = _net('tiny_mobile', engine)
    start = snapshot(graph)
    plan, keys = dfq.build_bc_plan(graph, bottoms, TARG)
    index = list(range(len(keys)))
    wild = [(0, 40, -7, 1 << 30, 17, 1)[i % 6] for i in index]
    tame = [min(max(b, 2), 16) for b in wild]
    assert set(tame) == {2, 16}
    plan.run(check=True, per_channel=per_channel, widths=(torch.tensor(tame, dtype=torch.int32, device=engine.device), index))
    want = snapshot(graph)
    _load(graph, start)
    plan.run(check=True, per_channel=per_channel, widths=(torch.tensor(wild, dtype=torch.int32, device=engine.device), index))
    _same(graph, want, 'clamped vs in range: ')
    _load(graph, start)
    plan.run(check=True, per_channel=per_channel, widths=dict(zip(keys, tame)))
    _same(graph, want, 'mapping vs tensor: ')
    plan.close()


@pytest.mark.parametrize('per_channel', [False, True])
def test_one_nan_in_one_network(engine, monkeypatch, per_channel):
    """One NaN in one layer of one network of a batch: that network gets the corrections the oracle gives under the range rule
    (the NaN is skipped by the layer's / row's range and poisons the sums it enters), no other network changes."""
    nets, batch = _batch(engine, BATCH_SEEDS)
    starts = [snapshot(g) for (_, g, _) in nets]
    plan = batch.bc_plan()
    keys = plan.keys
    wmap = _cyclic(keys)
    plan.run(check=True, per_channel=per_channel, widths=wmap)
    clean = [snapshot(g) for (_, g, _) in nets]
    for (_, g, _), st in zip(nets, starts):
        _load(g, st)
    graph = nets[1][1]
    pw = [k for k in keys if graph[k].weight.shape[2:] == (1, 1) and graph[k].weight.shape[1] > 1]
    victim = pw[len(pw) // 2]
    with torch.no_grad():
        graph[victim].weight[1, 2] = float('nan')
    spec = _oracle(graph, nets[1][2], monkeypatch, [wmap[k] for k in keys], False, per_channel)
    plan.run(check=True, per_channel=per_channel, widths=wmap)
    plan.close()
    osnap = _spec_snapshot(spec)
    assert any(np.isnan(v).any() for k, v in osnap.items() if k.endswith('.b')), 'the NaN reaches no bias: the test shows nothing'
    assert not all(np.isnan(v).all() for k, v in osnap.items() if k.endswith('.b'))
    _match(graph, spec, 'the network with the NaN: ')
    for n in (0, 2):
        _same(nets[n][1], clean[n], 'net {} next to the NaN: '.format(n))
    batch.release()


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------

def test_abi_of_the_widths_entry_point(engine):
    """What the binding adds to _ffi.py: one symbol, no struct.  Its ctypes signature is the header's prototype, argument for
    argument, and the library under test exports it."""
    import os
    import re
    res, args = _ffi.SIGNATURES['dfq_bc_plan_run_widths']
    assert res is ctypes.c_int32
    assert args == [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_int32),
                    ctypes.c_int32, ctypes.c_void_p]
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'dfq_hip.h')).read()
    proto = re.search(r'int dfq_bc_plan_run_widths\((.*?)\);', header, flags=re.S).group(1)
    proto = re.sub(r'/\*.*?\*/', '', proto, flags=re.S)
    params = [' '.join(p.split()) for p in proto.split(',')]
    assert params == ['dfq_bc_plan* plan', 'int32_t symmetric', 'int32_t per_row', 'const int32_t* widths', 'int64_t width_stride',
                      'const int32_t* width_index', 'int32_t uniform_bits', 'void* stream']
    assert hasattr(_ffi.lib(), 'dfq_bc_plan_run_widths')
