"""improve_dfq.clip_quant_range and HistogramMeter: clipped activation ranges from the histograms of the quantisers' inputs over
the distilled batches.

The truth comes from the test's own pre-hooks, which clone every quantiser input during both passes: min / max, the counts and
the selection are taken from those clones with the numpy restatements of tests/test_act_hist.py.  Counts must be EQUAL,
percentile ranges EQUAL, MSE ranges within the any-order summation rule stated there."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from dfq_amd import improve_dfq, prims
from dfq_amd.utils import quantize as q

from test_act_hist import F32, assert_mse_choice, ref_hist, ref_percentile

BINS = 64
PIN = (F32(-2.11790393), F32(2.64))


class Net(nn.Module):
    """three quantised layers and one add: c0 is fed by the data, c1 by a ReLU, fc by the pooled sum of both branches"""

    def __init__(self, bits=(8, 6, 4)):
        super().__init__()
        self.c0 = q.QuantConv2d(3, 6, 3, padding=1, num_bits_act=bits[0])
        self.c1 = q.QuantConv2d(6, 6, 3, padding=1, num_bits_act=bits[1])
        self.fc = q.QuantLinear(6, 5, num_bits_act=bits[2])

    def forward(self, x):
        a = torch.relu(self.c0(x))
        b = self.c1(a) + a
        return self.fc(b.mean((2, 3)))


def _build(device, seed=0):
    torch.manual_seed(seed)
    net = Net().to(device).eval()
    graph = {'Data': 'Data', 'c0': net.c0, 'c1': net.c1, 'fc': net.fc}
    bottoms = {'Data': None, 'c0': ['Data'], 'c1': ['c0'], 'fc': ['c1']}
    g = torch.Generator().manual_seed(seed + 1)
    data = [torch.randn(4, 3, 8, 8, generator=g).clamp_(-2.1179, 2.64) for _ in range(2)]
    # ranges "as update_quant_range leaves them": the pin, and something plausible for the two others
    with torch.no_grad():
        for m, (lo, hi) in ((net.c0.quant, PIN), (net.c1.quant, (0.0, 1.5)), (net.fc.quant, (-0.5, 0.9))):
            m.running_min.fill_(float(lo))
            m.running_max.fill_(float(hi))
    return net, graph, bottoms, data


def _run(engine, method, **kw):
    net, graph, bottoms, data = _build(engine.device)
    assert net.c0.quant.num_bits == 8 and net.c1.quant.num_bits == 6 and net.fc.quant.num_bits == 4
    with torch.no_grad():
        net(data[0].to(engine.device))                       # (a QuantMeasure packs its two buffers into one pair on its first forward)
    seen = {'c1.quant': [], 'fc.quant': [], 'c0.quant': []}
    hooks = [m.register_forward_pre_hook(lambda mod, a, k=n: seen[k].append(a[0].detach().cpu().numpy().copy()))
             for n, m in net.named_modules() if isinstance(m, q.QuantMeasure)]
    ids = {n: (m.running_min, m.running_max) for n, m in net.named_modules() if isinstance(m, q.QuantMeasure)}
    report = {}
    out = improve_dfq.clip_quant_range(net, data, graph, bottoms, method=method, bins=BINS, report=report, **kw)
    for h in hooks:
        h.remove()
    assert out is net
    return net, seen, ids, report


def _check_tables(net, seen, ids, report):
    """what does not depend on the method; returns {name: (counts, lo, hi)} from the clones"""
    assert sorted(report) == ['c0.quant', 'c1.quant', 'fc.quant']
    truth = {}
    for name in ('c1.quant', 'fc.quant'):
        acts = seen[name]
        assert len(acts) == 4                                # two batches, two passes
        for a, b in zip(acts[:2], acts[2:]):
            assert np.array_equal(a, b), 'the two passes saw different inputs: the ranges changed in between'
        lo, hi = F32(min(a.min() for a in acts[:2])), F32(max(a.max() for a in acts[:2]))
        counts = sum(ref_hist(a, lo, hi, BINS) for a in acts[2:])
        entry = report[name]
        assert not entry['pinned']
        assert np.array_equal(entry['hist_range'].cpu().numpy(), np.array([lo, hi], dtype=F32)), name
        got = entry['counts'].cpu().numpy()
        assert got.dtype == np.int64 and np.array_equal(got, counts), name
        assert got[BINS] == 0 and got[BINS + 1] == 0 and got[BINS + 2] == 0
        assert int(got.sum()) == sum(a.size for a in acts[2:])
        truth[name] = (counts, lo, hi)
    assert truth['c1.quant'][1] == 0.0                       # the input of c1 comes out of a ReLU
    for name, m in net.named_modules():
        if isinstance(m, q.QuantMeasure):
            assert m.running_min is ids[name][0] and m.running_max is ids[name][1], name + ': a buffer was replaced'
            assert tuple(m.running_min.shape) == (1,) and tuple(m.running_max.shape) == (1,)
            new = report[name]['new_range'].cpu().numpy()
            assert new[0] == float(m.running_min) and new[1] == float(m.running_max)
    # the quantiser fed by 'Data' is pinned, not searched
    pin = report['c0.quant']
    assert pin['pinned'] and 'counts' not in pin
    assert F32(float(net.c0.quant.running_min)) == PIN[0] and F32(float(net.c0.quant.running_max)) == PIN[1]
    assert np.array_equal(report['c1.quant']['old_range'].cpu().numpy(), np.array([0.0, 1.5], dtype=F32))
    return truth


@pytest.mark.parametrize('p', [0.999, 0.9, 1.0])
def test_percentile_ranges_equal_the_restatement(engine, p):
    net, seen, ids, report = _run(engine, 'percentile', percentile=p)
    truth = _check_tables(net, seen, ids, report)
    for name, m in (('c1.quant', net.c1.quant), ('fc.quant', net.fc.quant)):
        counts, lo, hi = truth[name]
        want = ref_percentile(counts, lo, hi, BINS, p)
        assert F32(float(m.running_min)) == want[0] and F32(float(m.running_max)) == want[1], name
        if p == 1.0:
            assert want[0] == lo and want[1] == hi


@pytest.mark.parametrize('candidates', [None, 5])
def test_mse_ranges_follow_the_rule_with_each_quantisers_own_bits(engine, candidates):
    net, seen, ids, report = _run(engine, 'mse', candidates=candidates)
    truth = _check_tables(net, seen, ids, report)
    for name, m in (('c1.quant', net.c1.quant), ('fc.quant', net.fc.quant)):
        counts, lo, hi = truth[name]
        got = np.array([float(m.running_min), float(m.running_max)], dtype=F32)
        assert_mse_choice(got, counts, lo, hi, BINS, m.num_bits, candidates or BINS // 2, name)
        assert lo <= got[0] < got[1] <= hi


def test_detection_pin_and_refusals(engine):
    net, graph, bottoms, data = _build(engine.device)
    improve_dfq.clip_quant_range(net, data, graph, bottoms, method='percentile', bins=BINS, is_detection=True)
    assert float(net.c0.quant.running_min) == -1.0 and float(net.c0.quant.running_max) == 1.0
    for kw in (dict(method='kl'), dict(bins=1), dict(bins=4097), dict(method='percentile', percentile=0.5), dict(candidates=0),
               dict(bins=BINS, candidates=BINS // 2 + 1)):
        with pytest.raises(ValueError):
            improve_dfq.clip_quant_range(net, data, graph, bottoms, **kw)
    net.c1.quant.update_stat = True
    with pytest.raises(ValueError, match='update_stat'):
        improve_dfq.clip_quant_range(net, data, graph, bottoms)
    net.c1.quant.update_stat = False
    net.fc.quant.num_bits = 1
    with pytest.raises(ValueError, match='num_bits'):
        improve_dfq.clip_quant_range(net, data, graph, bottoms)


def test_histogram_meter_on_its_own(engine):
    """the two phases of one meter, tables of its own, NaN skipped by the range and counted by the histogram"""
    rng = np.random.default_rng(2)
    a, b = rng.standard_normal((3, 5, 7)).astype(F32), (2.0 * rng.standard_normal((2, 70))).astype(F32)
    a[1, 2, 3] = np.nan
    meter = improve_dfq.HistogramMeter(bins=32)
    quant = q.QuantMeasure().to(engine.device).eval()
    quant.running_min.fill_(-1.0)
    quant.running_max.fill_(1.0)
    handle = quant.register_forward_pre_hook(meter.hook)
    ta, tb = torch.from_numpy(a).to(engine.device), torch.from_numpy(b).to(engine.device)
    quant(ta), quant(tb)
    lo, hi = F32(min(np.nanmin(a), b.min())), F32(max(np.nanmax(a), b.max()))
    assert np.array_equal(meter.range2.cpu().numpy(), np.array([lo, hi], dtype=F32))
    assert int(meter.counts.sum()) == 0
    meter.phase = 'count'
    quant(ta), quant(tb[:, 1:])                              # (a view that is not contiguous)
    handle.remove()
    want = ref_hist(a, lo, hi, 32) + ref_hist(b[:, 1:], lo, hi, 32)
    assert np.array_equal(meter.counts.cpu().numpy(), want) and want[32 + 2] == 1 and meter.calls == 4
    new = prims.hist_clip_range(meter.counts, meter.range2, num_bits=4).cpu().numpy()
    assert_mse_choice(new, want, lo, hi, 32, 4, 16, 'a meter of its own')
    meter.phase = 'both'
    with pytest.raises(ValueError):
        meter.add(ta)


# ---- sharded ---------------------------------------------------------------------------------------------------------------
def _dp_worker(rank, world, port, out_dir, emu_path):
    import ctypes
    import torch.distributed as dist
    from dfq_amd import _ffi
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        torch.set_num_threads(1)
        _ffi._lib = _ffi.bind(ctypes.CDLL(emu_path))
        _ffi.target_device = lambda: torch.device('cpu')
        _ffi.current_stream = lambda: 0
        _ffi.synchronize = lambda: None
        net, graph, bottoms, data = _build(torch.device('cpu'))
        g = torch.Generator().manual_seed(9)
        data = data + [torch.randn(4, 3, 8, 8, generator=g) * (1.0 + i) for i in range(3)]        # five batches: an uneven split
        report = {}
        improve_dfq.clip_quant_range(net, data, graph, bottoms, method='mse', bins=BINS, report=report,
                                     group=dist.group.WORLD if world > 1 else None)
        names = sorted(n for n in report if not report[n]['pinned'])
        np.savez(os.path.join(out_dir, 'w{}_rank{}.npz'.format(world, rank)),
                 ranges=np.array([[float(m.running_min), float(m.running_max)] for m in net.modules() if isinstance(m, q.QuantMeasure)], dtype=F32),
                 counts=np.stack([report[n]['counts'].numpy() for n in names]),
                 hist_range=np.stack([report[n]['hist_range'].numpy() for n in names]))
    finally:
        dist.destroy_process_group()


def test_sharded_over_two_ranks_is_bit_identical_to_the_sequential_call(tmp_path, emu_lib_path):
    """gloo world-2, the kernels on the CPU emulation: rank r takes batches r, r + 2, ...; counts are integers and extrema are
    selections, so -- unlike update_quant_range and bias_correction_distill -- both ranks end with exactly the sequential result"""
    import socket
    import torch.multiprocessing as mp

    def port():
        with socket.socket() as s:
            s.bind(('127.0.0.1', 0))
            return s.getsockname()[1]
    for world in (1, 2):
        mp.spawn(_dp_worker, args=(world, port(), str(tmp_path), emu_lib_path), nprocs=world, join=True)
    seq = np.load(os.path.join(str(tmp_path), 'w1_rank0.npz'))
    assert int(seq['counts'].sum()) > 0 and (seq['ranges'][:, 0] < seq['ranges'][:, 1]).all()
    for rank in (0, 1):
        got = np.load(os.path.join(str(tmp_path), 'w2_rank{}.npz'.format(rank)))
        assert np.array_equal(got['counts'], seq['counts']), 'rank {}: counts'.format(rank)
        assert np.array_equal(got['hist_range'].view(np.int32), seq['hist_range'].view(np.int32)), 'rank {}: histogram ranges'.format(rank)
        assert np.array_equal(got['ranges'].view(np.int32), seq['ranges'].view(np.int32)), 'rank {}: ranges'.format(rank)
