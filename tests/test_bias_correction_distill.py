"""improve_dfq.bias_correction_distill (improve_dfq.py:311-371) and its hook, improve_dfq.ChannelSumMeter.

The expected biases come from this file's own float64 statement of improve_dfq.py:349-365: the hooked outputs of both models
are captured with plain forward hooks on ``copy.deepcopy`` models, and per layer and channel
    T = sum_b (fsum(out_q[b][:, c]) - fsum(out_ref[b][:, c])) / N_b,      shift = T * scale,      A = sum_b (fsum|out_q| + fsum|out_ref|) / N_b
with ``math.fsum`` (exactly rounded sums) and a handful of float64 operations around them.  The product adds the same terms in
float64 in an order of its own, so the tolerance is the bound of any-order recursive summation of n terms with u = 2^-53,
n u A scale (Higham (4.4), as tests/test_batch_error.py uses it; n counts every element of both models plus, per batch and
model, the product with 1 / N_b and the addition to the table, plus the difference and the scale), plus ONE float32 rounding
of the shift, 2^-24 |shift|, and ONE of the subtraction, 2^-24 (|bias| + |shift32|).  Nothing looser anywhere."""
import copy
import gc
import math
import os
import weakref
from collections import OrderedDict

import numpy as np
import pytest
import torch
import torch.nn as nn

from dfq_amd import _ffi, improve_dfq
from dfq_amd.utils import layer_transform as lt

F32 = np.float32
U = 2.0 ** -53
TARG = [nn.Conv2d, nn.Linear]
LAYERS = ('c0', 'c1', 'c2', 'fc')
SIZES = (4, 4, 2)                                            # unequal batches: each weighs 1 / N_b (the reference's mean(0))


class Net(nn.Module):
    """conv 3->8 3x3, ReLU, depthwise 8 (no bias), ReLU6, 1x1 conv 8->12, global mean, Linear 12->5: plain modules"""

    def __init__(self):
        super().__init__()
        self.c0 = nn.Conv2d(3, 8, 3, padding=1)
        self.r0 = nn.ReLU()
        self.c1 = nn.Conv2d(8, 8, 3, padding=1, groups=8, bias=False)
        self.r1 = nn.ReLU6()
        self.c2 = nn.Conv2d(8, 12, 1)
        self.fc = nn.Linear(12, 5)

    def forward(self, x):
        x = self.r0(self.c0(x))
        x = self.r1(self.c1(x))
        x = self.c2(x)
        return self.fc(x.mean(3).mean(2))


def _models(device, seed=0):
    """(the copy with weights fake-quantised to 4 bits, the original), and the distilled-data stand-ins"""
    torch.manual_seed(seed)
    ref = Net().eval()
    with torch.no_grad():
        for m in ref.modules():
            if isinstance(m, (nn.Conv2d, nn.Linear)) and m.bias is not None:
                m.bias.copy_(torch.randn(m.bias.shape) * 0.2)
    g = torch.Generator().manual_seed(seed + 100)
    data = [torch.randn(n, 3, 9, 9, generator=g) for n in SIZES]
    ref.to(device)
    qm = copy.deepcopy(ref)
    graph = OrderedDict((k, getattr(qm, k)) for k in LAYERS)
    lt.quantize_targ_layer(graph, 4, 32, TARG)                # the error of 4-bit weights is far above rounding
    _ffi.synchronize()
    return qm, ref, data


def _capture(model, data, device):
    """{layer: [float32 numpy output per batch]} from plain forward hooks on a deep copy"""
    model = copy.deepcopy(model).to(device).eval()
    outs = {k: [] for k in LAYERS}
    handles = [getattr(model, k).register_forward_hook(lambda m, i, o, k=k: outs[k].append(o.detach().cpu().numpy().copy())) for k in LAYERS]
    with torch.no_grad():
        for batch in data:
            model(batch.to(device))
    for h in handles:
        h.remove()
    return outs


def _fsum(a):
    return math.fsum(np.asarray(a, dtype=np.float64).reshape(-1).tolist())


def _statement(outs_q, outs_ref, spatial):
    """{layer: (shift [C], n u A scale [C], hw)} -- the float64 statement of improve_dfq.py:349-365"""
    res = {}
    n_batches = len(SIZES)
    for k in LAYERS:
        c = outs_q[k][0].shape[1]
        hw = int(np.prod(outs_q[k][0].shape[2:]))
        scale = 1.0 / (n_batches * hw) if spatial == 'mean' else 1.0 / n_batches
        n = 2 * sum(o.shape[0] for o in outs_q[k]) * hw + 4 * n_batches + 2
        shift, bound = [], []
        for ch in range(c):
            t = a = 0.0
            for oq, orf in zip(outs_q[k], outs_ref[k]):
                t += (_fsum(oq[:, ch]) - _fsum(orf[:, ch])) / oq.shape[0]
                a += (_fsum(np.abs(oq[:, ch])) + _fsum(np.abs(orf[:, ch]))) / oq.shape[0]
            shift.append(t * scale)
            bound.append(n * U * a * scale)
        res[k] = (np.array(shift), np.array(bound), hw)
    return res


def _eager_float32(outs_q, outs_ref):
    """{layer: error [C]} -- improve_dfq.py:349-365 as the reference runs it, in eager float32 on retained outputs"""
    res = {}
    for k in LAYERS:
        error_list = None
        for b, (oq, orf) in enumerate(zip(outs_q[k], outs_ref[k])):
            hq, ho = torch.from_numpy(oq), torch.from_numpy(orf)
            if b == 0:
                error_list = [hq.mean(0), ho.mean(0)]                       # :352
            else:
                error_list[0] += hq.mean(0)                                 # :354
                error_list[1] += ho.mean(0)                                 # :355
        error = (error_list[0] - error_list[1]) / len(SIZES)                # :361
        res[k] = error.view(error.size(0), -1).sum(-1).numpy()              # :365
    return res


def _biases(model):
    return {k: (getattr(model, k).bias.detach().cpu().numpy().copy() if getattr(model, k).bias is not None else None) for k in LAYERS}


def _assert_biases(got, before, stated, what):
    for k in LAYERS:
        shift, bound, _ = stated[k]
        old = before[k].astype(np.float64) if before[k] is not None else np.zeros(len(shift))
        want = old - shift
        tol = bound + 2.0 ** -24 * np.abs(shift) + 2.0 ** -24 * (np.abs(old) + np.abs(shift) * (1 + 2.0 ** -23)) + 2.0 ** -149
        err = np.abs(got[k].astype(np.float64) - want)
        print('{} {}: worst error {:.3e}, its tolerance {:.3e}'.format(what, k, err.max(), tol[err.argmax()]))
        assert got[k].dtype == F32 and (err <= tol).all(), '{} {}: off by {} against {}'.format(what, k, err, tol)


# ---- 1. the formula --------------------------------------------------------------------------------------------------------
def test_biases_against_the_float64_statement(engine):
    qm, ref, data = _models(engine.device)
    outs_q, outs_ref = _capture(qm, data, engine.device), _capture(ref, data, engine.device)
    before = _biases(qm)
    # the statement is the reference's arithmetic: its eager float32 form lies within 2^-22 sum|term| of it (measured on
    # these shapes: 2^-24; the margin of 4 is for torch's unspecified reduction order)
    stated = _statement(outs_q, outs_ref, 'sum')
    eager = _eager_float32(outs_q, outs_ref)
    for k in LAYERS:
        shift, bound, hw = stated[k]
        n = 2 * sum(SIZES) * hw + 4 * len(SIZES) + 2
        a_scaled = bound / (n * U)                                          # sum|term| * scale
        err = np.abs(eager[k].astype(np.float64) - shift)
        print('eager float32 {}: worst {:.3e} of 2^-22 sum|term| = {:.3e}'.format(k, err.max(), (2.0 ** -22 * a_scaled)[err.argmax()]))
        assert (err <= 2.0 ** -22 * a_scaled).all(), k
    got = {}
    for spatial in ('sum', 'mean'):
        model = copy.deepcopy(qm)
        out = improve_dfq.bias_correction_distill(model, copy.deepcopy(ref), data, TARG, TARG, spatial=spatial)
        _ffi.synchronize()
        assert out is model
        got[spatial] = _biases(model)
        _assert_biases(got[spatial], before, _statement(outs_q, outs_ref, spatial), spatial)
        for k in LAYERS:                                                    # it did something: the error of 4 bits is no rounding
            old = before[k] if before[k] is not None else np.zeros_like(got[spatial][k])
            assert (got[spatial][k] != old).any(), k
    assert np.array_equal(got['sum']['fc'].view(np.int32), got['mean']['fc'].view(np.int32))       # H * W = 1: the two coincide
    assert not np.array_equal(got['sum']['c0'], got['mean']['c0'])
    with pytest.raises(ValueError, match='spatial'):
        improve_dfq.bias_correction_distill(copy.deepcopy(qm), copy.deepcopy(ref), data, TARG, TARG, spatial='max')


# ---- 2. it corrects --------------------------------------------------------------------------------------------------------
def _mean_error(outs_q, outs_ref, k):
    """per-channel mean output error of layer k over the batches, each weighted 1 / N_b, and max|output|"""
    err = 0.0
    for oq, orf in zip(outs_q[k], outs_ref[k]):
        d = oq.astype(np.float64) - orf.astype(np.float64)
        err = err + d.mean(axis=(0, 2, 3))
    top = max(float(np.abs(o).max()) for o in outs_q[k] + outs_ref[k])
    return np.abs(err / len(outs_q[k])), top


def test_mean_output_error_of_the_first_layer_goes(engine):
    qm, ref, data = _models(engine.device)
    outs_ref = _capture(ref, data, engine.device)
    before, top = _mean_error(_capture(qm, data, engine.device), outs_ref, 'c0')
    improve_dfq.bias_correction_distill(qm, copy.deepcopy(ref), data, TARG, TARG, spatial='mean')
    _ffi.synchronize()
    after, top_after = _mean_error(_capture(qm, data, engine.device), outs_ref, 'c0')
    small = 2.0 ** -22 * max(top, top_after)
    print('mean output error of c0: before {}, after {}, 2^-22 max|output| = {:.3e}'.format(before, after, small))
    assert (before >= 100 * small).all()
    assert (after <= small).all()


# ---- 3. mechanics ----------------------------------------------------------------------------------------------------------
def _hook_count(model):
    return sum(len(m._forward_hooks) for m in model.modules())


def test_parameters_hooks_and_refusals(engine):
    qm, ref, data = _models(engine.device)
    kept = {k: getattr(qm, k).bias for k in LAYERS}
    assert kept['c1'] is None
    ref_before = _biases(ref)
    improve_dfq.bias_correction_distill(qm, ref, data, TARG, TARG)
    _ffi.synchronize()
    for k in ('c0', 'c2', 'fc'):
        assert getattr(qm, k).bias is kept[k]                               # an existing Parameter keeps its identity
    b = qm.c1.bias
    assert isinstance(b, nn.Parameter) and not b.requires_grad and b.device == engine.device and b.shape == (8,) and b.dtype is torch.float32
    assert ref.c1.bias is None
    for k in ('c0', 'c2', 'fc'):
        assert np.array_equal(_biases(ref)[k], ref_before[k])               # the original model is read only
    assert _hook_count(qm) == 0 and _hook_count(ref) == 0
    assert not qm.training and not ref.training
    # a forward that raises: the hooks go all the same
    bad = data[:1] + [torch.randn(2, 4, 9, 9)]
    with pytest.raises(RuntimeError):
        improve_dfq.bias_correction_distill(qm, ref, bad, TARG, TARG)
    assert _hook_count(qm) == 0 and _hook_count(ref) == 0
    # the reference's assertion, and a pair whose channels differ
    with pytest.raises(AssertionError, match='len of hooks in 2 models must be the same'):
        improve_dfq.bias_correction_distill(qm, ref, data, TARG, [nn.Linear])
    other = Net().to(engine.device)
    other.c2 = nn.Conv2d(8, 10, 1).to(engine.device)
    other.fc = nn.Linear(10, 5).to(engine.device)
    with pytest.raises(ValueError, match='channels'):
        improve_dfq.bias_correction_distill(qm, other, data, TARG, TARG)
    with pytest.raises(ValueError, match='no batches'):
        improve_dfq.bias_correction_distill(qm, ref, [], TARG, TARG)
    assert _hook_count(qm) == 0 and _hook_count(ref) == 0 and _hook_count(other) == 0
    # exact type match, as in the reference: a subclass is not hooked
    class MyLinear(nn.Linear):
        pass
    sub = copy.deepcopy(ref)
    sub.fc.__class__ = MyLinear
    with pytest.raises(AssertionError, match='len of hooks'):
        improve_dfq.bias_correction_distill(qm, sub, data, TARG, TARG)


def test_two_calls_are_bit_equal(engine):
    qm, ref, data = _models(engine.device)
    got = []
    for _ in range(2):
        model = copy.deepcopy(qm)
        improve_dfq.bias_correction_distill(model, copy.deepcopy(ref), data, TARG, TARG)
        _ffi.synchronize()
        got.append(_biases(model))
    for k in LAYERS:
        assert np.array_equal(got[0][k].view(np.int32), got[1][k].view(np.int32)), k


def test_hooks_do_not_keep_outputs(engine):
    qm, ref, data = _models(engine.device)
    refs, dead = [], []

    def watch(module, inputs, output):
        if refs:
            dead.append(refs[-1]() is None)                                 # the output of the batch before is gone by now
        refs.append(weakref.ref(output))
    handle = qm.c0.register_forward_hook(watch)
    improve_dfq.bias_correction_distill(qm, ref, data, TARG, TARG)
    handle.remove()
    gc.collect()
    assert len(refs) == len(data) and dead == [True] * (len(data) - 1) and refs[-1]() is None


def test_meter_stands_alone(engine):
    """ChannelSumMeter outside the function: its own table, a Linear and a conv output, a view that is not 16-byte aligned"""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(3, 5, 7, 2, generator=g)
    meter = improve_dfq.ChannelSumMeter()
    meter.add(x.to(engine.device))
    meter.add(x.to(engine.device).permute(0, 1, 3, 2), weight=2.0)          # not contiguous: copied first
    buf = torch.zeros(x.numel() + 1).to(engine.device)
    buf[1:] = x.reshape(-1).to(engine.device)
    meter.add(buf[1:].view(3, 5, 14))                                       # 4 bytes into a buffer: copied first
    _ffi.synchronize()
    assert meter.hw == 14 and meter.calls == 3 and meter.acc.dtype is torch.float64
    want = x.double().sum(dim=(0, 2, 3)) * (1.0 / 3 + 2.0 + 1.0 / 3)
    assert torch.allclose(meter.acc.cpu(), want, rtol=1e-13, atol=1e-13)
    lin = improve_dfq.ChannelSumMeter(torch.zeros(5, dtype=torch.float64, device=engine.device))
    lin.add(x[:, :, 0, 0].contiguous().to(engine.device))
    _ffi.synchronize()
    assert lin.hw == 1 and torch.allclose(lin.acc.cpu(), x[:, :, 0, 0].double().mean(0), rtol=1e-13, atol=1e-13)
    with pytest.raises(ValueError, match='channels'):
        lin.add(torch.zeros(2, 6).to(engine.device))
    with pytest.raises(TypeError):
        lin.add((x,))
    with pytest.raises(ValueError, match='float64'):
        improve_dfq.ChannelSumMeter(torch.zeros(5))


def test_nan_in_one_channel_of_one_layer(engine):
    qm, ref, data = _models(engine.device)
    with torch.no_grad():
        qm.c2.weight[3] = float('nan')
    improve_dfq.bias_correction_distill(qm, ref, data, TARG, TARG)
    _ffi.synchronize()
    got = _biases(qm)
    assert np.isfinite(got['c0']).all() and np.isfinite(got['c1']).all()
    assert np.flatnonzero(np.isnan(got['c2'])).tolist() == [3]
    assert np.isnan(got['fc']).all()                                        # the Linear layer mixes every channel of c2: the network carries it there


# ---- 4. data-parallel ------------------------------------------------------------------------------------------------------
def _dp_worker(rank, world, port, out_dir, emu_path):
    import ctypes
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        torch.set_num_threads(1)
        _ffi._lib = _ffi.bind(ctypes.CDLL(emu_path))
        _ffi.target_device = lambda: torch.device('cpu')
        _ffi.current_stream = lambda: 0
        _ffi.synchronize = lambda: None
        cpu = torch.device('cpu')
        qm, ref, data = _models(cpu)
        if world == 1:                                                      # the statement, from the same arithmetic as the workers'
            stated = _statement(_capture(qm, data, cpu), _capture(ref, data, cpu), 'mean')
            before = _biases(qm)
            np.savez(os.path.join(out_dir, 'stated.npz'), **{k + '.shift': stated[k][0] for k in LAYERS}, **{k + '.bound': stated[k][1] for k in LAYERS},
                     **{k + '.before': before[k] for k in LAYERS if before[k] is not None})
        improve_dfq.bias_correction_distill(qm, ref, data, TARG, TARG, spatial='mean', group=dist.group.WORLD if world > 1 else None)
        np.savez(os.path.join(out_dir, 'w{}_rank{}.npz'.format(world, rank)), **_biases(qm))
    finally:
        dist.destroy_process_group()


def test_data_parallel_over_two_ranks(tmp_path, emu_lib_path):
    """the three batches split over two ranks (gloo; kernels on the CPU emulation), ONE all_reduce of the float64 table: both
    ranks end with the same biases bit for bit, and they lie within the sequential call's bound of the float64 statement"""
    import socket
    import torch.multiprocessing as mp

    def port():
        with socket.socket() as s:
            s.bind(('127.0.0.1', 0))
            return s.getsockname()[1]
    for world in (1, 2):
        mp.spawn(_dp_worker, args=(world, port(), str(tmp_path), emu_lib_path), nprocs=world, join=True)
    load = lambda name: dict(np.load(os.path.join(str(tmp_path), name)))
    seq, r0, r1, st = load('w1_rank0.npz'), load('w2_rank0.npz'), load('w2_rank1.npz'), load('stated.npz')
    stated = {k: (st[k + '.shift'], st[k + '.bound'], None) for k in LAYERS}
    before = {k: st.get(k + '.before') for k in LAYERS}
    for k in LAYERS:
        assert np.array_equal(r0[k].view(np.int32), r1[k].view(np.int32)), 'the two ranks differ in ' + k
    _assert_biases(seq, before, stated, 'sequential')
    _assert_biases(r0, before, stated, 'two ranks')
