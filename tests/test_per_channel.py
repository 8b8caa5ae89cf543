"""Per-channel weight mode of bias correction and weight quantisation (extension): the quantiser of output row o is the
reference's UniformQuantize recipe (utils/quantize.py:23-76, Python-float min/max) with row o's own (min, max).

The oracle is the numpy restatement with its per-tensor row-sum function replaced by a per-row one:
``orc.bias_correction`` calls ``quant_error_rowsum`` through its module, so patching that one function turns the whole
reference correction (E[x], matvec, bias / beta~ updates, chain order) into the per-channel reference."""
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


def _rowsum_per_channel(bits):
    """eps.view(O, I, -1).sum(-1) with row o quantised by its own (min, max) at `bits` bits (sequential float32 sum over k)."""
    def rowsum(weight, signed=False, num_bits=8):
        w = np.asarray(weight, dtype=F32)
        eps = np.empty_like(w)
        for o in range(w.shape[0]):
            r = w[o]
            eps[o] = (orc.uniform_quantize(r, bits, float(r.min()), float(r.max()), signed) - r).astype(F32)
        e3 = eps.reshape(w.shape[0], w.shape[1], -1)
        acc = np.zeros(e3.shape[:2], dtype=F32)
        for k in range(e3.shape[2]):
            acc = (acc + e3[:, :, k]).astype(F32)
        return acc
    return rowsum


def _net(name, engine):
    """(model, graph, bottoms) after BN folding, in the state the correction starts from (the `abs` stage of the golden
    fixture where there is one, else the synthetic net's own folded weights)."""
    if name in GOLDEN_NETS:
        gold = net_fixture(name, GOLDEN_NETS[name], '')
        model, graph, bottoms = synthetic.build(name, seed=GOLDEN_NETS[name])
        load_inputs(graph, gold, 'cpu')
        model.to(engine.device)
        lt.merge_batchnorm(model, graph, bottoms, TARG)
        load_stage(graph, gold, 'abs')
    else:
        model, graph, bottoms = synthetic.build(name, seed=0)
        model.to(engine.device)
        lt.merge_batchnorm(model, graph, bottoms, TARG)
    return model, graph, bottoms


def _oracle(graph, bottoms, monkeypatch, bits, signed, per_channel=True, collect=None):
    spec = graphspec.from_torch(graph, bottoms, TARG)
    with monkeypatch.context() as m:
        if per_channel:
            m.setattr(orc, 'quant_error_rowsum', _rowsum_per_channel(bits))
        orc.bias_correction(spec, signed=signed, collect=collect)
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
            assert_close(esnap[k], osnap[k], what + k)


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


# ---- bias correction against the per-channel oracle ---------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['tiny_mobile', 'tiny_res', 'tiny_cat', 'tiny_wide'])
@pytest.mark.parametrize('bits,signed', [(8, False), (6, True), (4, False), (8, True)])
def test_bias_correction_per_channel_against_oracle(engine, monkeypatch, name, bits, signed):
    model, graph, bottoms = _net(name, engine)
    _ensure_biases(graph)
    spec = _oracle(graph, bottoms, monkeypatch, bits, signed)
    dfq.bias_correction(graph, bottoms, TARG, bits_weight=bits, signed=signed, per_channel=True)
    _match(graph, spec, '{} {}b signed={}: '.format(name, bits, signed))


@pytest.mark.parametrize('name,bits,signed', [('tiny_res', 8, False), ('tiny_mobile', 4, True), ('tiny_wide', 6, False)])
def test_eps_and_corrections_per_channel(engine, monkeypatch, name, bits, signed):
    """DFQ_BC_EPS=1: the materialised row sums are the per-row oracle's bit for bit, the corrections within 1e-5."""
    monkeypatch.setenv('DFQ_BC_EPS', '1')
    model, graph, bottoms = _net(name, engine)
    _ensure_biases(graph)
    collect = {}
    _oracle(graph, bottoms, monkeypatch, bits, signed, collect=collect)
    plan, keys = dfq.build_bc_plan(graph, bottoms, TARG)
    plan.run(signed=signed, check=True, per_channel=True, bits=bits)
    assert keys == list(collect.keys())
    for step, k in enumerate(keys):
        e = npy(plan.eps(step))
        assert_bitexact(e, collect[k]['eps'].reshape(e.shape), 'eps of {}'.format(k))
        assert_close(npy(plan.correction(step)), collect[k]['bias'].reshape(-1), 'correction of {}'.format(k))
    plan.close()


PROTOCOLS = [
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
def test_protocol_matrix_per_channel(engine, monkeypatch, name):
    """Every hand-over protocol gives the same bits in per-channel mode (and runs twice on one plan: the second run of a
    tagged plan uses the other slot parity and epoch)."""
    model, graph, bottoms = _net(name, engine)
    _ensure_biases(graph)
    start = snapshot(graph)
    spec = _oracle(graph, bottoms, monkeypatch, 6, True)
    ref = None
    for env in PROTOCOLS:
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            plan, _ = dfq.build_bc_plan(graph, bottoms, TARG)
            for _ in range(2):
                _load(graph, start)
                plan.run(signed=True, check=True, per_channel=True, bits=6)
            plan.close()
        got = snapshot(graph)
        if ref is None:
            ref = got
            _match(graph, spec, 'default: ')
            continue
        for k in ref:
            assert_bitexact(got[k], ref[k], '{}: {}'.format(env, k))


def test_safe_mode_and_plan_modes_alternate(engine, monkeypatch):
    """One plan, per-tensor -> per-channel -> per-tensor -> per-channel in safe mode: each run matches its own oracle."""
    model, graph, bottoms = _net('tiny_mobile', engine)
    _ensure_biases(graph)
    start = snapshot(graph)
    plan, _ = dfq.build_bc_plan(graph, bottoms, TARG)
    for per_channel, safe in [(False, False), (True, False), (False, False), (True, True)]:
        _load(graph, start)
        if safe:
            plan.set_safe_mode()
        spec = _oracle(graph, bottoms, monkeypatch, 8, False, per_channel=per_channel)
        plan.run(check=True, per_channel=per_channel, bits=8)
        _match(graph, spec, 'per_channel={} safe={}: '.format(per_channel, safe))
    plan.close()


def test_plan_cache_keeps_modes_apart(engine, monkeypatch):
    """bias_correction on one graph: per-tensor, then per-channel, then per-tensor again -- each matches its own oracle."""
    model, graph, bottoms = _net('tiny_res', engine)
    _ensure_biases(graph)
    start = snapshot(graph)
    for per_channel in (False, True, False, True):
        _load(graph, start)
        spec = _oracle(graph, bottoms, monkeypatch, 4, False, per_channel=per_channel)
        dfq.bias_correction(graph, bottoms, TARG, bits_weight=4, per_channel=per_channel)
        _match(graph, spec, 'per_channel={}: '.format(per_channel))


def test_row_extremes_make_the_modes_agree(engine):
    """Where every row holds its tensor's min and max, per-channel at 8 bits IS per-tensor: bit-identical results."""
    model, graph, bottoms = _net('tiny_mobile', engine)
    _ensure_biases(graph)
    with torch.no_grad():
        for k in graph:
            if type(graph[k]) in TARG:
                w = graph[k].weight.view(graph[k].weight.shape[0], -1)
                lo, hi = float(w.min()), float(w.max())
                w[:, 0] = lo
                w[:, -1] = hi
    start = snapshot(graph)
    dfq.bias_correction(graph, bottoms, TARG)
    per_tensor = snapshot(graph)
    _load(graph, start)
    dfq.bias_correction(graph, bottoms, TARG, bits_weight=8, per_channel=True)
    for k, v in snapshot(graph).items():
        assert_bitexact(v, per_tensor[k], k)


def test_edge_rows(engine, monkeypatch):
    """A constant row (the scale clamps to 1e-8), an all-zero row, in a 1x1 layer and in a folded depthwise layer."""
    model, graph, bottoms = _net('tiny_mobile', engine)
    _ensure_biases(graph)
    layers = [k for k in graph if type(graph[k]) in TARG]
    dw = [k for k in layers if getattr(graph[k], 'groups', 1) > 1 and graph[k].weight.shape[1] == 1]
    pw = [k for k in layers if graph[k].weight.shape[2:] == (1, 1) and graph[k].weight.shape[1] > 1]
    assert dw and pw
    with torch.no_grad():
        for k in (dw[0], pw[0]):
            graph[k].weight[0].fill_(0.25)
            graph[k].weight[1].zero_()
    for signed in (False, True):
        start = snapshot(graph)
        spec = _oracle(graph, bottoms, monkeypatch, 8, signed)
        dfq.bias_correction(graph, bottoms, TARG, signed=signed, per_channel=True)
        _match(graph, spec, 'signed={}: '.format(signed))
        _load(graph, start)


def test_wide_rows_take_the_streaming_path(engine, monkeypatch):
    """A row of more than 1536 inputs (the chain's register capacity) in a grouped 1x1 layer: its row sums stream from memory."""
    model, graph, bottoms = _net('tiny_wide', engine)
    assert any(type(graph[k]) in TARG and graph[k].weight[0].numel() > 1536 for k in graph)
    _ensure_biases(graph)
    spec = _oracle(graph, bottoms, monkeypatch, 5, True)
    dfq.bias_correction(graph, bottoms, TARG, bits_weight=5, signed=True, per_channel=True)
    _match(graph, spec)


# ---- batches ------------------------------------------------------------------------------------------------------------------

def _batch_nets(engine, n):
    nets = []
    for s in range(n):
        model, graph, bottoms = synthetic.build('tiny_mobile', seed=s)
        model.to(engine.device)
        lt.merge_batchnorm(model, graph, bottoms, TARG)
        _ensure_biases(graph)
        nets.append((model, graph, bottoms))
    return nets


def test_batch_plans_per_channel(engine, monkeypatch):
    """build_bc_plan_batch and a NetworkBatch give every network what its own plan gives it, bit for bit (skewed too)."""
    nets = _batch_nets(engine, 3)
    starts = [snapshot(g) for (_, g, _) in nets]
    want = []
    for (model, graph, bottoms), st in zip(nets, starts):
        plan, _ = dfq.build_bc_plan(graph, bottoms, TARG)
        plan.run(check=True, per_channel=True, bits=6)
        plan.close()
        want.append(snapshot(graph))
        _load(graph, st)
    for env in ({}, {'DFQ_BC_SKEW': '1.5'}, {'DFQ_BC_ONE_LAUNCH': '1'}):
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            plan = dfq.build_bc_plan_batch([(g, b) for (_, g, b) in nets], TARG)
            plan.run(check=True, per_channel=True, bits=6)
            plan.close()
        for i, (_, graph, _) in enumerate(nets):
            for k, v in snapshot(graph).items():
                assert_bitexact(v, want[i][k], '{} net {}: {}'.format(env, i, k))
            _load(graph, starts[i])
    batch = arena.NetworkBatch([(g, b, rel.create_relation(g, b, TARG)) for (_, g, b) in nets], TARG)
    plan = batch.bc_plan()
    plan.run(check=True, per_channel=True, bits=6)
    plan.close()
    for i, (_, graph, _) in enumerate(nets):
        for k, v in snapshot(graph).items():
            assert_bitexact(v, want[i][k], 'NetworkBatch net {}: {}'.format(i, k))
    batch.release()


# ---- quantize_targ_layer ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('bits,signed', [(8, False), (8, True), (4, False), (4, True)])
def test_quantize_targ_layer_per_channel(engine, bits, signed):
    model, graph, bottoms = _net('tiny_wide', engine)
    _ensure_biases(graph)
    gen = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for k in graph:
            if type(graph[k]) in TARG:
                graph[k].bias.copy_(torch.randn(graph[k].bias.shape, generator=gen) * 0.1)
    spec = graphspec.from_torch(graph, bottoms, TARG)
    before = {k: npy(graph[k].weight) for k in graph if type(graph[k]) in TARG}
    out = lt.quantize_targ_layer(graph, bits, 16, TARG, return_codes=True, per_channel=True, signed=signed)
    assert len(out) == 3
    _, codes, ranges = out
    orc.quantize_targ_layer(spec, 8, 16)                   # (the biases: per tensor, at 16 bits)
    for k, w0 in before.items():
        rows = w0.reshape(w0.shape[0], -1)
        ys, qs = [], []
        for r in rows:
            y, q = orc.uniform_quantize(r, bits, float(r.min()), float(r.max()), signed, return_codes=True)
            ys.append(y)
            qs.append(q)
        assert_bitexact(npy(graph[k].weight).reshape(rows.shape), np.stack(ys), 'weight {}'.format(k))
        assert np.array_equal(codes[k].cpu().numpy().reshape(rows.shape), np.stack(qs).astype(np.int32)), 'codes {}'.format(k)
        rg = npy(ranges[k])
        assert rg.shape == (rows.shape[0], 2)
        assert_bitexact(rg[:, 0], rows.min(1), 'row min {}'.format(k))
        assert_bitexact(rg[:, 1], rows.max(1), 'row max {}'.format(k))
        assert_bitexact(npy(graph[k].bias), spec.nodes[k].bias, 'bias {}'.format(k))
        assert max(len(np.unique(r)) for r in npy(graph[k].weight).reshape(rows.shape)) <= 2 ** bits


def test_quantize_targ_layer_other_modes_unchanged(engine):
    """per_channel=False keeps its return values; signed=True there is the symmetric per-tensor recipe."""
    model, graph, bottoms = _net('tiny_mobile', engine)
    spec = graphspec.from_torch(graph, bottoms, TARG)
    before = {k: npy(graph[k].weight) for k in graph if type(graph[k]) in TARG}
    res = lt.quantize_targ_layer(graph, 8, 16, TARG, return_codes=True, signed=True)
    assert len(res) == 2
    for k, w0 in before.items():
        y = orc.uniform_quantize(w0, 8, float(w0.min()), float(w0.max()), True)
        assert_bitexact(npy(graph[k].weight), y, k)
    assert lt.quantize_targ_layer(graph, 8, 16, TARG, per_channel=True) is graph


# ---- bad input ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('bits', [0, 1, 17, 32, 8.0, True])
def test_bad_bit_widths_raise(engine, bits):
    model, graph, bottoms = _net('tiny_mobile', engine)
    _ensure_biases(graph)
    start = snapshot(graph)
    with pytest.raises(ValueError):
        dfq.bias_correction(graph, bottoms, TARG, bits_weight=bits, per_channel=True)
    with pytest.raises(ValueError):
        lt.quantize_targ_layer(graph, bits, 16, TARG, per_channel=True)
    for k, v in snapshot(graph).items():
        assert_bitexact(v, start[k], 'untouched after a rejected call: {}'.format(k))
    dfq.bias_correction(graph, bottoms, TARG, bits_weight=bits if not isinstance(bits, bool) else 8)   # ignored per tensor


def test_c_entry_points_reject_bad_arguments(engine):
    lib = _ffi.lib()
    assert lib.dfq_bc_plan_run_per_channel(None, 0, 8, None) == ERR_ARG
    assert lib.dfq_row_quant_plan_run(None, None) == ERR_ARG
    assert lib.dfq_row_quant_plan_create(None, 1, ctypes.byref(ctypes.c_void_p())) == ERR_ARG
    lib.dfq_row_quant_plan_destroy(None)
    x = torch.zeros(4, 3, device=engine.device)
    for seg in (_ffi.DfqRowSegment(x.data_ptr(), 4, 3, 1, 0, None, None), _ffi.DfqRowSegment(x.data_ptr(), 4, 3, 17, 0, None, None),
                _ffi.DfqRowSegment(x.data_ptr(), 0, 3, 8, 0, None, None), _ffi.DfqRowSegment(None, 4, 3, 8, 0, None, None)):
        plan = ctypes.c_void_p()
        assert lib.dfq_row_quant_plan_create((_ffi.DfqRowSegment * 1)(seg), 1, ctypes.byref(plan)) == ERR_ARG
    model, graph, bottoms = _net('tiny_mobile', engine)
    _ensure_biases(graph)
    plan, _ = dfq.build_bc_plan(graph, bottoms, TARG)
    for bits in (1, 17, -8):
        assert lib.dfq_bc_plan_run_per_channel(plan._plan, 0, bits, None) == ERR_ARG
        with pytest.raises(ValueError):
            plan.run(per_channel=True, bits=bits)
    plan.close()


# ---- the example --------------------------------------------------------------------------------------------------------------

def test_calibrate_example_per_channel(engine, tmp_path, capsys):
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'examples'))
    import calibrate
    table = str(tmp_path / 't.table')
    model, graph, bottoms = calibrate.main(['--net', 'tiny_mobile', '--table', table, '--device', str(engine.device),
                                            '--per-channel', '--bits-weight', '4', '--signed'])
    lines = open(table).read().splitlines()
    keys = [k for k in graph if hasattr(graph[k], 'quant')]
    assert len(lines) == 2 * len(keys)
    for line, k in zip(lines, keys):
        w = graph[k].weight.detach().cpu().reshape(graph[k].weight.shape[0], -1)
        scales = [float(v) for v in line.split()[1:]]
        assert len(scales) == w.shape[0]
        assert len(set(scales)) > 1 or w.shape[0] == 1           # one scale per output channel
        assert max(len(torch.unique(r)) for r in w) <= 16
    model(torch.randn(2, 3, 32, 32, device=engine.device))


# ---- full-size networks (GPU only: the CPU emulation would take minutes) ------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize('name', ['mobilenet_v2', 'resnet18', 'deeplab_mnv2'])
def test_full_size_per_channel_against_oracle(monkeypatch, name):
    model, graph, bottoms = synthetic.build(name, seed=0)
    model.to(torch.device('cuda', 0))
    lt.merge_batchnorm(model, graph, bottoms, TARG)
    _ensure_biases(graph)
    spec = _oracle(graph, bottoms, monkeypatch, 8, False)
    dfq.bias_correction(graph, bottoms, TARG, bits_weight=8, per_channel=True)
    _match(graph, spec, name + ': ')


@pytest.mark.gpu
def test_batch_of_64_mobilenets_per_channel(monkeypatch):
    """A batch of 64 MobileNetV2s: a fixed sample of networks gets what its own plan gives it, bit for bit."""
    dev = torch.device('cuda', 0)
    nets = []
    for s in range(64):
        model, graph, bottoms = synthetic.build('mobilenet_v2', seed=s % 4)
        model.to(dev)
        lt.merge_batchnorm(model, graph, bottoms, TARG)
        _ensure_biases(graph)
        nets.append((model, graph, bottoms))
    sample = [0, 1, 17, 42, 63]
    starts = {i: snapshot(nets[i][1]) for i in sample}
    want = {}
    for i in sample:
        _, graph, bottoms = nets[i]
        plan, _ = dfq.build_bc_plan(graph, bottoms, TARG)
        plan.run(check=True, per_channel=True, bits=8)
        plan.close()
        want[i] = snapshot(graph)
        _load(graph, starts[i])
    plan = dfq.build_bc_plan_batch([(g, b) for (_, g, b) in nets], TARG)
    plan.run(check=True, per_channel=True, bits=8)
    plan.close()
    for i in sample:
        for k, v in snapshot(nets[i][1]).items():
            assert_bitexact(v, want[i][k], 'net {}: {}'.format(i, k))
