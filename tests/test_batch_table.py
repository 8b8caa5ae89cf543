"""NetworkBatch.table_plan / calibration_tables / dfq_batch_table_plan_*: the ncnn int8 calibration table
(``ncnn_table``, convert_ncnn.py:178-201) of every network of a batch from one plan.

The contract is equality, not closeness.  The plan selects values (a tensor's min and max, a row's max|w|) and computes
nothing, so ``ranges(n)`` / ``row_absmax(n)`` are compared with ``==`` against ``ncnn_table.weight_ranges`` /
``prims.row_range(w, signed=True)`` and numpy (which leaves the sign of a zero free and nothing else), and the tables are
compared string for string with ``ncnn_table.calibration_table`` on each network alone, on the CPU emulation and on the
MI355X alike.  A tensor holding NaN must not fault and must not reach any other tensor."""
import copy
import ctypes
import json
import math
import os
import subprocess
import tempfile
from collections import OrderedDict

import numpy as np
import pytest
import torch
import torch.nn as nn

from dfq_amd import _ffi, arena, ncnn_table, prims, synthetic
from dfq_amd.utils import layer_transform as lt
from dfq_amd.utils import relation as rel
from dfq_amd.utils.quantize import QConv2d, QLinear, QuantMeasure

from common import GOLD, TARG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DFQ_ERR_ARG = -1     # include/dfq_hip.h
QTARG = [QConv2d, QLinear]
TINY = ['tiny_mobile', 'tiny_res', 'tiny_cat', 'tiny_seg', 'tiny_head']
BIG = [('mobilenet_v2', 4), ('resnet18', 2), ('deeplab_mnv2', 2)]


class _Gpu:
    kind, device = 'gpu', torch.device('cuda', 0)


# ---- helpers -----------------------------------------------------------------------------------------------------------
def _twin_graph(graph, device):
    """the same network with storages of its own: QConv2d / QLinear (which carry a ``.quant``) for the conv / linear layers,
    BatchNorm modules with cloned parameters and buffers (tests/test_batch_act.py)"""
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


def _prepared(name, seed, device, targ=TARG):
    model, graph, bottoms = synthetic.build(name, seed=seed)
    model.to(device)
    if targ is QTARG:
        graph = _twin_graph(graph, device)
    lt.merge_batchnorm(model, graph, bottoms, targ)
    return graph, bottoms, rel.create_relation(graph, bottoms, targ, delete_single=False)


def _batch(name, seeds, engine, targ=TARG):
    nets = [_prepared(name, s, engine.device, targ) for s in seeds]
    return nets, arena.NetworkBatch(nets, targ)


def _alone(graph, bottoms, device):
    """a twin of the network, calibrated alone: ``lt.set_quant_minmax`` fills its quantisers"""
    gq = _twin_graph(graph, device)
    lt.set_quant_minmax(gq, bottoms, verbose=False)
    return gq


def _names(graph, targ):
    keys = [k for k in graph if type(graph[k]) in tuple(targ)]
    return ['w{}_blob'.format(i) for i in range(len(keys))] + ['a{}_blob'.format(i) for i in range(len(keys))]


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _assert_tables_equal(got, want, what):
    assert len(got) == len(want), what
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, '{}: line {} differs:\n  batch  {}\n  single {}'.format(what, i, a[:200], b[:200])


def _check_statistics(plan, nets, targ, what):
    """ranges(n) == ncnn_table.weight_ranges, row_absmax(n) == prims.row_range(w, signed=True): as floats, exactly"""
    for n, (g, _, _) in enumerate(nets):
        want = ncnn_table.weight_ranges(g, targ)
        got, rows = plan.ranges(n), plan.row_absmax(n)
        assert list(got.keys()) == list(want.keys()) == list(rows.keys()) == plan.keys
        for k in plan.keys:
            assert tuple(got[k].tolist()) == tuple(want[k]), '{} net {} {}: {} != {}'.format(what, n, k, got[k].tolist(), want[k])
            a = prims.row_range(g[k].weight, signed=True)
            assert rows[k].shape == a.shape and rows[k].tolist() == a.tolist(), '{} net {} {}'.format(what, n, k)


# ---- 1. batch equals per network -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', TINY)
def test_batch_equals_per_network(engine, name):
    nets, batch = _batch(name, [0, 1, 2], engine, QTARG)
    twins = [_alone(g, b, engine.device) for g, b, _ in nets]
    act = batch.set_quant_minmax()                               # the closed plan; the quantisers are bound to its block
    names = _names(nets[0][0], QTARG)
    seen = set()
    for per_channel in (False, True):
        for nm in (None, names):
            want = [ncnn_table.calibration_table(gq, targ_type=QTARG, names=nm, per_channel=per_channel) for gq in twins]
            for a in (act, None):
                got = batch.calibration_tables(act=a, names=nm, per_channel=per_channel)
                assert len(got) == len(nets)
                for n in range(len(nets)):
                    _assert_tables_equal(got[n], want[n], '{} net {} per_channel {} names {} act {}'.format(
                        name, n, per_channel, nm is not None, a is not None))
            seen.add(tuple(want[0]))
            assert want[0] != want[1] and want[1] != want[2]      # a plan that read network 0 for everybody would be seen
    assert len(seen) == 4
    plan = batch.table_plan()
    # 7. launch count: two launches (and the clear of the block), whatever the number of networks and layers
    assert plan.launches <= 2
    assert plan.n_nets == 3 and plan.n_tensors == len(plan.keys) == len(names) // 2
    assert plan.elements == sum(nets[0][0][k].weight.numel() for k in plan.keys)
    plan.run()
    _ffi.synchronize()
    _check_statistics(plan, nets, QTARG, name)
    first = plan.block.clone()
    plan.run()                                                   # a second run clears and fills the block again
    _ffi.synchronize()
    assert torch.equal(_bits(plan.block), _bits(first))
    plan.close()
    assert torch.equal(_bits(plan.block), _bits(first))          # the block outlives the plan


@pytest.mark.parametrize('name', ['tiny_mobile', 'tiny_head'])
def test_plain_layers_with_an_act_plan(engine, name, tmp_path):
    """nn.Conv2d / nn.Linear graphs carry no ``.quant``: the activation ranges come from the act_range_plan"""
    nets, batch = _batch(name, [3, 4, 5], engine)
    twins = [_alone(g, b, engine.device) for g, b, _ in nets]
    storage = batch.storage.clone()
    act = batch.act_range_plan()
    act.run()
    _ffi.synchronize()
    for per_channel in (False, True):
        got = batch.calibration_tables(act=act, per_channel=per_channel)          # an open plan
        for n, gq in enumerate(twins):
            _assert_tables_equal(got[n], ncnn_table.calibration_table(gq, targ_type=QTARG, per_channel=per_channel),
                                 '{} net {} per_channel {}'.format(name, n, per_channel))
    act.close()
    paths = [str(tmp_path / 'net{}.table'.format(n)) for n in range(3)]
    written = batch.write_calibration_tables(paths, act=act)                       # a closed one
    for n, gq in enumerate(twins):
        ref_path = str(tmp_path / 'alone{}.table'.format(n))
        want = ncnn_table.write_calibration_table(ref_path, gq, targ_type=QTARG)
        assert written[n] == want and open(paths[n]).read() == open(ref_path).read()
    assert torch.equal(_bits(batch.storage), _bits(storage)), 'the tables wrote into the batch allocation'
    with pytest.raises(AttributeError, match='no quantiser'):
        batch.calibration_tables()
    with pytest.raises(ValueError, match='one path per network'):
        batch.write_calibration_tables(paths[:2], act=act)


# ---- 2. pinned to the reference ------------------------------------------------------------------------------------------
def test_tables_against_the_reference(engine, tmp_path):
    """tests/test_minmax.py::test_ncnn_calibration_table_against_the_reference on a batch that holds the fixture's network
    twice: the lines the reference's own block convert_ncnn.py:180-197 wrote for the bench's synthetic MobileNetV2 (seed 0,
    weights as built), under the names of the table the reference holds, with the fixture's seeded activation ranges."""
    gold = json.load(open(os.path.join(GOLD, 'ncnn_table.json')))
    names = gold['names']
    want = [' '.join([n] + [s] * c) for n, s, c in gold['lines']]
    assert len(want) == 106 and len(names) == 106
    model, graph, _ = synthetic.build('mobilenet_v2', seed=0)
    fixture = OrderedDict((k, m.weight.detach().clone()) for k, m in graph.items() if type(m) in TARG)
    assert len(fixture) == 53
    nets, batch = _batch('mobilenet_v2', [0, 0], engine)
    for g, _, _ in nets:
        with torch.no_grad():
            for i, (k, w) in enumerate(fixture.items()):
                g[k].weight.copy_(w.to(engine.device))                # INTO the slot: the network as the fixture saw it
                q = QuantMeasure()
                q.running_min.fill_(gold['act_min'][i])
                q.running_max.fill_(gold['act_max'][i])
                g[k].quant = q.to(engine.device)
    batch.check(thorough=True)
    paths = [str(tmp_path / 'model_int8_tensor_{}.table'.format(n)) for n in range(2)]
    tables = batch.write_calibration_tables(paths, names=names)
    for n in range(2):
        _assert_tables_equal(tables[n], want, 'net {}'.format(n))
        assert open(paths[n]).read() == '\n'.join(want) + '\n'
    plain = batch.calibration_tables()
    assert [l.split(' ')[1:] for l in plain[1]] == [l.split(' ')[1:] for l in want]


# ---- 3. independence -----------------------------------------------------------------------------------------------------
def test_networks_are_independent(engine):
    nets, batch = _batch('tiny_mobile', [0, 1, 2], engine)
    act = batch.set_quant_minmax()
    before = {pc: batch.calibration_tables(act=act, per_channel=pc) for pc in (False, True)}
    keys = [k for k in nets[0][0] if type(nets[0][0][k]) in TARG]
    i = len(keys) // 2
    w = nets[1][0][keys[i]].weight
    assert w.shape[0] >= 3
    with torch.no_grad():
        w[2].mul_(0.0).add_(1000.0)                                   # one row of one weight of network 1
    after = {pc: batch.calibration_tables(act=act, per_channel=pc) for pc in (False, True)}
    for pc in (False, True):
        assert after[pc][0] == before[pc][0] and after[pc][2] == before[pc][2]
        changed = [j for j, (a, b) in enumerate(zip(after[pc][1], before[pc][1])) if a != b]
        assert changed == [i], (pc, changed)
    a, b = after[True][1][i].split(' '), before[True][1][i].split(' ')
    assert [j for j in range(len(a)) if a[j] != b[j]] == [1 + 2] and a[3] == str(128. / 1000.)
    assert set(after[False][1][i].split(' ')[1:]) == {str(128. / 1000.)}


# ---- 4. row geometry through the ABI ---------------------------------------------------------------------------------------
# (rows, row_len): rows of 1, depthwise rows of 9, the stem's 27, 64, a piece's worth and one more, rows longer than a piece
# (4096 floats), more rows of 1 than a piece holds; 37 x 9, 3 x 1537, 1 x 9001 and 7 x 1 are no multiples of 4 elements
SHAPES = [(7, 1), (37, 9), (16, 27), (24, 64), (3, 1536), (3, 1537), (2, 5000), (1, 9001), (5000, 1), (1, 4096), (2, 4097), (130, 96)]


@pytest.mark.parametrize('n_nets', [1, 3])
def test_row_geometry_through_the_abi(engine, n_nets):
    lib = _ffi.lib()
    rng = np.random.default_rng(5 + n_nets)
    offs, total = [], 0
    for j, (r, n) in enumerate(SHAPES):
        offs.append(total)
        total += -(-(r * n) // 4) * 4 + 4 * (j % 3)                   # 16-byte aligned, with gaps of 0, 4 or 8 floats
    stride = total + 8
    host = np.full((n_nets, stride), 7.5e5, dtype=np.float32)        # a gap that leaks into a tensor shows as its maximum
    xs = []
    for k in range(n_nets):
        xs.append([])
        for j, ((r, n), o) in enumerate(zip(SHAPES, offs)):
            x = (rng.standard_normal((r, n)) * (k + 1)).astype(np.float32)
            x[0, 0] = 50.0 + j                                       # the extremum in the first element of a row ...
            x[-1, -1] = -(60.0 + k)                                  # ... and in the last one
            if r > 2:
                x[1, -1], x[2, 0] = 40.0, -45.0
            if j % 4 == 1:
                x[r // 2, n // 2] = np.inf
            if j % 4 == 2:
                x[r // 2, n - 1] = -np.inf
            if j % 4 == 3 and r > 1:
                x[r - 1, :] = 0.0
                x[r - 1, n // 2] = -0.0                              # an all-zero row
            host[k, o:o + r * n] = x.reshape(-1)
            xs[k].append(x)
    store = torch.from_numpy(host).to(engine.device).contiguous()
    pristine = store.clone()
    out_offs, s = [], 2 * len(SHAPES) + 3
    for (r, n) in SHAPES:
        out_offs.append(s)
        s += r + 1                                                    # one word between the tensors' rows
    out = torch.full((n_nets, s), 9.0, dtype=torch.float32, device=engine.device)
    base0 = store.data_ptr()
    T = _ffi.DfqBatchTableTensor
    tabs = (T * len(SHAPES))(*[T(base0 + 4 * o, r, n, 2 * j, ro) for j, ((r, n), o, ro) in enumerate(zip(SHAPES, offs, out_offs))])
    bases = (ctypes.c_void_p * n_nets)(*[base0 + 4 * k * stride for k in range(n_nets)])
    plan = ctypes.c_void_p()
    _ffi.check(lib.dfq_batch_table_plan_create(tabs, len(SHAPES), bases, n_nets, out.data_ptr(), s, ctypes.byref(plan)))
    try:
        assert lib.dfq_batch_table_plan_launches(plan) <= 2
        for _ in range(2):                                            # a second run gives the same block
            _ffi.check(lib.dfq_batch_table_plan_run(plan, _ffi.stream_arg()))
            _ffi.synchronize()
    finally:
        lib.dfq_batch_table_plan_destroy(plan)
    assert torch.equal(_bits(store), _bits(pristine)), 'run() wrote into the weights'
    got = out.cpu().numpy()
    for k in range(n_nets):
        used = np.zeros(s, dtype=bool)
        for j, ((r, n), ro) in enumerate(zip(SHAPES, out_offs)):
            x = xs[k][j]
            what = 'net {} rows {} x {}'.format(k, r, n)
            assert got[k, 2 * j] == x.min() and got[k, 2 * j + 1] == x.max(), (what, got[k, 2 * j:2 * j + 2], x.min(), x.max())
            assert np.array_equal(got[k, ro:ro + r], np.abs(x).max(axis=1)), what
            assert not np.signbit(got[k, ro:ro + r]).any(), what      # max|w| of an all-zero row is +0
            used[2 * j:2 * j + 2] = True
            used[ro:ro + r] = True
        assert (got[k][~used] == 0.0).all()                           # the rest of the block is cleared


# ---- 5. NaN isolation ----------------------------------------------------------------------------------------------------
def test_nan_stays_in_its_tensor(engine):
    nets, batch = _batch('tiny_res', [0, 1, 2], engine)
    plan = batch.table_plan()
    plan.run()
    _ffi.synchronize()
    clean = plan.block.clone()
    i = len(plan.keys) // 2
    key, r_off, a_off, rows = plan._views[i]
    w = nets[1][0][key].weight
    with torch.no_grad():
        w.view(-1)[w.numel() // 3] = math.nan
        w[rows - 1] = math.nan                                        # and a whole row of them
    plan.run()
    _ffi.synchronize()
    same = _bits(plan.block) == _bits(clean)
    assert bool(same[0].all()) and bool(same[2].all()), 'another network saw the NaN'
    mine = torch.zeros(plan.block.shape[1], dtype=torch.bool)
    mine[r_off:r_off + 2] = True
    mine[a_off:a_off + rows] = True
    assert bool(same[1][~mine].all()), 'another tensor of the network saw the NaN'
    plan.close()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------
def test_refusals(engine):
    nets, batch = _batch('tiny_mobile', [0, 1], engine, QTARG)
    other_nets, other = _batch('tiny_mobile', [2, 3], engine, QTARG)
    act, other_act = batch.set_quant_minmax(), other.set_quant_minmax()
    g0 = nets[0][0]
    keys = [k for k in g0 if type(g0[k]) in QTARG]
    with pytest.raises(ValueError, match='of this batch'):
        batch.calibration_tables(act=other_act)
    with pytest.raises(ValueError, match='of this batch'):
        batch.calibration_tables(act=other_nets[0][0])
    for bad in (['x'] * (2 * len(keys) - 1), ['x'] * len(keys), []):
        with pytest.raises(ValueError, match='one name per layer'):
            batch.calibration_tables(act=act, names=bad)
    # a closed plan
    plan = batch.table_plan()
    plan.run()
    plan.close()
    plan.close()
    with pytest.raises(RuntimeError, match='closed'):
        plan.run()
    # a weight that left its slot (not the first layer's: the batch's own quick check watches that one)
    layer = g0[keys[1]]
    kept = layer.weight.data
    for moved in (kept.clone(), kept.double()):
        layer.weight.data = moved
        with pytest.raises(RuntimeError, match='weight of {} '.format(keys[1])):
            batch.table_plan()
        with pytest.raises(RuntimeError, match='weight of {} '.format(keys[1])):
            batch.calibration_tables(act=act)
    layer.weight.data = kept
    # an all-zero row: the exception of the single-network function, on that network
    with torch.no_grad():
        nets[1][0][keys[2]].weight[1].zero_()
    with pytest.raises(ZeroDivisionError):
        ncnn_table.calibration_table(nets[1][0], targ_type=QTARG, per_channel=True)
    with pytest.raises(ZeroDivisionError, match='network 1, weight of {}, row 1'.format(keys[2])):
        batch.calibration_tables(act=act, per_channel=True)
    assert batch.calibration_tables(act=act)[1] == ncnn_table.calibration_table(nets[1][0], targ_type=QTARG)     # per tensor: no error
    with torch.no_grad():
        nets[0][0][keys[0]].weight.zero_()
    with pytest.raises(ZeroDivisionError):
        ncnn_table.calibration_table(nets[0][0], targ_type=QTARG)
    with pytest.raises(ZeroDivisionError, match='network 0, weight of {}'.format(keys[0])):
        batch.calibration_tables(act=act)
    # a released batch
    plan = batch.table_plan()
    batch.release()
    with pytest.raises(RuntimeError, match='released'):
        plan.run()
    with pytest.raises(RuntimeError, match='released'):
        batch.table_plan()
    with pytest.raises(RuntimeError, match='released'):
        batch.calibration_tables(act=act)
    plan.close()


def test_unfolded_batch_is_refused(engine):
    nets = []
    for seed in (0, 1):
        model, graph, bottoms = synthetic.build('tiny_mobile', seed=seed)
        model.to(engine.device)
        nets.append((graph, bottoms, rel.create_relation(graph, bottoms, TARG, delete_single=False)))
    batch = arena.NetworkBatch.from_unfolded(nets, TARG)
    with pytest.raises(RuntimeError, match='not been folded'):
        batch.table_plan()
    with pytest.raises(RuntimeError, match='not been folded'):
        batch.calibration_tables()
    batch.merge_batchnorm()
    plan = batch.table_plan()
    plan.run()
    _ffi.synchronize()
    _check_statistics(plan, nets, TARG, 'folded by the batch')
    plan.close()


def test_abi_rejects_bad_arguments(engine):
    lib = _ffi.lib()
    buf = torch.zeros(1024, dtype=torch.float32, device=engine.device)
    out = torch.zeros(2 * 64, dtype=torch.float32, device=engine.device)
    p0 = buf.data_ptr()
    bases = (ctypes.c_void_p * 2)(p0, p0 + 4 * 512)
    T = _ffi.DfqBatchTableTensor

    def create(data=p0, rows=8, row_len=9, range_off=0, row_off=2, b=bases, n_nets=2, o=out.data_ptr(), stride=64, n_tensors=1, table=True,
               place=True):
        plan = ctypes.c_void_p()
        rc = lib.dfq_batch_table_plan_create((T * 1)(T(data, rows, row_len, range_off, row_off)) if table else None, n_tensors, b, n_nets,
                                             o, stride, ctypes.byref(plan) if place else None)
        n = lib.dfq_batch_table_plan_launches(plan) if rc == 0 else None
        if rc == 0:
            lib.dfq_batch_table_plan_destroy(plan)
        return rc, n
    assert create() == (0, 2)
    assert create(range_off=62, row_off=0) == (0, 2)                  # the last pair of the stride
    assert create(row_off=56) == (0, 2)                               # the last rows of it
    assert create(data=p0 + 16) == (0, 2)
    bad = [dict(table=False), dict(n_tensors=0), dict(n_tensors=-1), dict(place=False), dict(data=None), dict(rows=0), dict(rows=-3),
           dict(row_len=0), dict(row_len=-1), dict(data=p0 + 4), dict(data=p0 + 8), dict(range_off=-1), dict(range_off=63), dict(range_off=64),
           dict(row_off=-1), dict(row_off=57), dict(row_off=1 << 40), dict(o=None), dict(stride=0), dict(stride=-5), dict(stride=1),
           dict(b=None), dict(n_nets=0), dict(n_nets=-1), dict(b=(ctypes.c_void_p * 2)(p0, None)),
           dict(b=(ctypes.c_void_p * 2)(p0, p0 + 4 * 511)), dict(rows=1 << 40, row_len=1 << 40)]
    for kw in bad:
        assert create(**kw)[0] == DFQ_ERR_ARG, kw
        assert b'dfq_batch_table_plan_create' in lib.dfq_last_error(), kw
    assert lib.dfq_batch_table_plan_run(None, None) == DFQ_ERR_ARG
    assert b'dfq_batch_table_plan_run' in lib.dfq_last_error()
    assert lib.dfq_batch_table_plan_launches(None) == 0
    lib.dfq_batch_table_plan_destroy(None)


def test_struct_layout_matches_header():
    src = r'''
    #include <stdio.h>
    #include <stddef.h>
    #include "dfq_hip.h"
    int main(void) {
        printf("%zu %zu %zu %zu %zu %zu\n", sizeof(dfq_batch_table_tensor), offsetof(dfq_batch_table_tensor, data),
               offsetof(dfq_batch_table_tensor, rows), offsetof(dfq_batch_table_tensor, row_len),
               offsetof(dfq_batch_table_tensor, range_offset), offsetof(dfq_batch_table_tensor, row_offset));
        return 0;
    }'''
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, 't.c')
        open(c, 'w').write(src)
        exe = os.path.join(d, 't')
        subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), c, '-o', exe], check=True)
        got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    P = _ffi.DfqBatchTableTensor
    assert got == [ctypes.sizeof(P), P.data.offset, P.rows.offset, P.row_len.offset, P.range_offset.offset, P.row_offset.offset]


# ---- 8. full size, on the GPU --------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('name,count', BIG)
def test_big_networks_equal_per_network(name, count):
    assert torch.cuda.is_available(), 'gpu-marked test needs a ROCm GPU'
    _ffi.lib()
    engine = _Gpu()
    nets, batch = _batch(name, list(range(count)), engine, QTARG)
    le = batch.le_plan()                                              # the tables of equalised weights, as convert_ncnn.py writes them
    le.run(signed=True)
    le.close()
    _ffi.synchronize()
    twins = [_alone(g, b, engine.device) for g, b, _ in nets]
    act = batch.set_quant_minmax()
    for per_channel in (False, True):
        got = batch.calibration_tables(act=act, per_channel=per_channel)
        for n, gq in enumerate(twins):
            _assert_tables_equal(got[n], ncnn_table.calibration_table(gq, targ_type=QTARG, per_channel=per_channel),
                                 '{} net {} per_channel {}'.format(name, n, per_channel))
        assert got[0] != got[1]
    plan = batch.table_plan()
    assert plan.launches <= 2
    plan.run()
    _ffi.synchronize()
    _check_statistics(plan, nets, QTARG, name)
    plan.close()
    torch.cuda.synchronize()
