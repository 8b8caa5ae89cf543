"""NetworkBatch.squant_plan / quantize_squant and quantize_targ_layer(rounding='squant'): adaptive rounding (SQuant) of the
weights of a whole batch in one plan.

Every network of a batch must equal the numpy restatement of the definition (tests/test_squant_rows.py) and
quantize_targ_layer(rounding='squant') on a twin network, bit for bit: codes, stored weights, ranges, stats.  The biases keep
the nearest rounding of quantize(), and the default rounding is what it always was."""
import math

import numpy as np
import pytest
import torch

from dfq_amd import _ffi, arena, dfq, synthetic
from dfq_amd.utils import layer_transform as lt
from dfq_amd.utils import relation as rel

from common import TARG
from test_squant_rows import F32, HALF, bits_of, qparams, row_range, squant_ref

NAMES = ['tiny_mobile', 'tiny_res', 'tiny_cat']
CONFIGS = [(4, False, False), (8, False, False), (4, True, True), (6, True, False)]   # (bit_weight, per_channel, signed)


def _prepared(name, seed, device):
    model, graph, bottoms = synthetic.build(name, seed=seed)
    model.to(device)
    lt.merge_batchnorm(model, graph, bottoms, TARG)
    rels = rel.create_relation(graph, bottoms, TARG, delete_single=False)
    return model, graph, bottoms, rels


def _targ(graph):
    return [(k, m) for k, m in graph.items() if type(m) in TARG]


def _batch(name, seeds, device):
    """(nets, batch) after merge_batchnorm and layer equalisation"""
    nets = [_prepared(name, s, device) for s in seeds]
    batch = arena.NetworkBatch([(g, b, r) for (_, g, b, r) in nets], TARG)
    le = batch.le_plan()
    le.run()
    le.close()
    _ffi.synchronize()
    return nets, batch


def _twin(name, seed, device):
    model, g, b, r = _prepared(name, seed, device)
    dfq.cross_layer_equalization(g, r, TARG)
    return g


def _weights(graph):
    return {k: m.weight.detach().cpu().numpy().copy() for k, m in _targ(graph)}


def _biases(graph):
    return {k: m.bias.detach().cpu().numpy().copy() for k, m in _targ(graph) if m.bias is not None}


_REFS = {}


def _ref(name, seed, cfg, w0):
    """the restatement on network (name, seed)'s equalised weights, computed once per configuration"""
    key = (name, seed, cfg)
    if key not in _REFS:
        bits, per_channel, signed = cfg
        out = {}
        for k, w in w0.items():
            rows = w.shape[0]
            x = w.reshape(rows, -1)
            K = int(np.prod(w.shape[2:])) if w.ndim > 2 else 1
            mins = maxs = None
            if not per_channel:
                mn, mx = row_range(x.reshape(-1))
                mins, maxs = np.full(rows, mn, F32), np.full(rows, mx, F32)
            out[k] = squant_ref(x, K, bits, signed, mins, maxs)
        _REFS[key] = out
    return _REFS[key]


@pytest.mark.parametrize('name', NAMES)
@pytest.mark.parametrize('cfg', CONFIGS)
@pytest.mark.parametrize('codes', [None, 'int32', 'int8'])
def test_batch_equals_restatement_and_twin(engine, name, cfg, codes):
    bits, per_channel, signed = cfg
    seeds = [0, 1, 2]
    nets, batch = _batch(name, seeds, engine.device)
    before = [_weights(g) for (_, g, _, _) in nets]
    bias_before = [_biases(g) for (_, g, _, _) in nets]
    plan = batch.squant_plan(bits, per_channel=per_channel, signed=signed, codes=codes)
    assert 1 <= plan.launches <= 3
    plan.run()
    _ffi.synchronize()
    for n, seed in enumerate(seeds):
        g = nets[n][1]
        want = _ref(name, seed, cfg, before[n])
        got_codes, got_ranges, got_stats = plan.codes(n), plan.ranges(n), plan.stats(n)
        twin = codes == 'int32'                        # (the twin's path has no code width: once per configuration)
        if twin:
            gt = _twin(name, seed, engine.device)
            assert all(np.array_equal(bits_of(a), bits_of(b)) for a, b in zip(_weights(gt).values(), before[n].values())), 'twin'
            out = lt.quantize_targ_layer(gt, bits, 32, TARG, return_codes=True, per_channel=per_channel, signed=signed,
                                         rounding='squant')
        for k, m in _targ(g):
            what = '{} net {} {}'.format(name, n, k)
            rows = m.weight.shape[0]
            w = m.weight.detach().cpu().numpy().reshape(rows, -1)
            assert np.array_equal(bits_of(w), bits_of(want[k]['y'])), what + ': stored weights'
            assert np.array_equal(got_stats[k].cpu().numpy(), want[k]['stats']), what + ': stats'
            assert np.abs(want[k]['stats'][:, 0]).max() <= HALF
            r = got_ranges[k].cpu().numpy()
            wr = want[k]['ranges'] if per_channel else want[k]['ranges'][0]
            assert np.array_equal(bits_of(r), bits_of(wr)), what + ': ranges'
            if codes is not None:
                c = got_codes[k]
                assert c.dtype == (torch.int32 if codes == 'int32' else (torch.int8 if signed else torch.uint8))
                assert np.array_equal(c.cpu().numpy().astype(np.int64).reshape(rows, -1), want[k]['codes']), what + ': codes'
            else:
                assert got_codes == {}
            if not twin:
                continue
            # the twin network through quantize_targ_layer(rounding='squant')
            assert np.array_equal(bits_of(gt[k].weight.detach().cpu().numpy().reshape(rows, -1)), bits_of(w)), what + ': twin weights'
            assert np.array_equal(out[1][k].cpu().numpy().astype(np.int64).reshape(rows, -1), want[k]['codes']), what + ': twin codes'
            if per_channel:
                assert np.array_equal(bits_of(out[2][k].cpu().numpy()), bits_of(wr)), what + ': twin ranges'
        # weights only: the biases are as they were
        for k, b in _biases(g).items():
            assert np.array_equal(bits_of(b), bits_of(bias_before[n][k]))
    plan.close()
    with pytest.raises(RuntimeError):
        plan.run()


@pytest.mark.parametrize('name', NAMES)
@pytest.mark.parametrize('cfg', [(4, False, False), (4, True, True)])
def test_quantize_squant_biases_are_quantize_s(engine, name, cfg):
    bits, per_channel, signed = cfg
    seeds = [0, 1, 2]
    nets, batch = _batch(name, seeds, engine.device)
    nets2, batch2 = _batch(name, seeds, engine.device)
    before = [_weights(g) for (_, g, _, _) in nets]
    codes, ranges = batch.quantize_squant(bits, 8, per_channel=per_channel, signed=signed, codes='int8')
    codes2, ranges2 = batch2.quantize(bits, 8, per_channel=per_channel, signed=signed, codes='int8')
    for n, seed in enumerate(seeds):
        want = _ref(name, seed, cfg, before[n])
        b1, b2 = _biases(nets[n][1]), _biases(nets2[n][1])
        assert sorted(b1) == sorted(b2) and b1
        for k in b1:
            assert np.array_equal(bits_of(b1[k]), bits_of(b2[k])), '{} net {} {}: bias'.format(name, n, k)
            assert np.array_equal(bits_of(ranges[n][k + '.bias'].cpu().numpy()), bits_of(ranges2[n][k + '.bias'].cpu().numpy()))
        assert sorted(ranges[n]) == sorted(ranges2[n])
        for k, m in _targ(nets[n][1]):
            rows = m.weight.shape[0]
            assert np.array_equal(bits_of(m.weight.detach().cpu().numpy().reshape(rows, -1)), bits_of(want[k]['y']))
            assert np.array_equal(codes[n][k].cpu().numpy().astype(np.int64).reshape(rows, -1), want[k]['codes'])
            assert np.array_equal(bits_of(ranges[n][k].cpu().numpy()), bits_of(ranges2[n][k].cpu().numpy()))


@pytest.mark.parametrize('per_channel', [False, True])
def test_default_rounding_is_unchanged(engine, per_channel):
    """quantize_targ_layer without `rounding`, with rounding='nearest', and the batch's quantize(): one result"""
    name, seeds = 'tiny_mobile', [1]
    nets, batch = _batch(name, seeds, engine.device)
    codes, _ = batch.quantize(4, 8, per_channel=per_channel, codes='int32')
    for n, seed in enumerate(seeds):
        ga, gb = _twin(name, seed, engine.device), _twin(name, seed, engine.device)
        for (k, m), (_, t) in zip(_targ(nets[n][1]), _targ(ga)):      # (the batch gives every equalised layer a bias)
            if m.bias is not None and t.bias is None:
                lt._ensure_bias(t)
                lt._ensure_bias(gb[k])
        oa = lt.quantize_targ_layer(ga, 4, 8, TARG, return_codes=True, per_channel=per_channel)
        ob = lt.quantize_targ_layer(gb, 4, 8, TARG, return_codes=True, per_channel=per_channel, rounding='nearest')
        for k, m in _targ(nets[n][1]):
            for other in (ga, gb):
                assert np.array_equal(bits_of(m.weight.detach().cpu().numpy()), bits_of(other[k].weight.detach().cpu().numpy())), k
                if m.bias is not None:
                    assert np.array_equal(bits_of(m.bias.detach().cpu().numpy()), bits_of(other[k].bias.detach().cpu().numpy())), k
            assert torch.equal(oa[1][k].cpu(), ob[1][k].cpu()) and torch.equal(oa[1][k].cpu(), codes[n][k].cpu()), k
    with pytest.raises(ValueError):
        lt.quantize_targ_layer(_twin(name, 0, engine.device), 4, 8, TARG, rounding='stochastic')
    with pytest.raises(ValueError):
        lt.quantize_targ_layer(_twin(name, 0, engine.device), 1, 8, TARG, rounding='squant')


def test_batch_of_one_and_released(engine):
    nets, batch = _batch('tiny_res', [3], engine.device)
    before = _weights(nets[0][1])
    codes, ranges = batch.quantize_squant(4, 32, per_channel=True, codes='int32')
    want = _ref('tiny_res', 3, (4, True, False), before)
    for k, m in _targ(nets[0][1]):
        rows = m.weight.shape[0]
        assert np.array_equal(bits_of(m.weight.detach().cpu().numpy().reshape(rows, -1)), bits_of(want[k]['y']))
        assert np.array_equal(codes[0][k].cpu().numpy().astype(np.int64).reshape(rows, -1), want[k]['codes'])
    assert not any(k.endswith('.bias') for k in ranges[0])
    with pytest.raises(ValueError):
        batch.squant_plan(17)
    with pytest.raises(ValueError):
        batch.squant_plan(9, codes='int8')
    with pytest.raises(ValueError):
        batch.squant_plan(8, codes='int16')
    plan = batch.squant_plan(8)
    batch.release()
    with pytest.raises(RuntimeError):
        plan.run()
    with pytest.raises(RuntimeError):
        batch.squant_plan(8)
    with pytest.raises(RuntimeError):
        batch.quantize_squant(8)
    plan.close()


@pytest.mark.parametrize('name', NAMES)
@pytest.mark.parametrize('cfg', [(4, True, False), (4, False, False), (4, True, True)])
def test_row_error_sums(engine, name, cfg):
    """The effect: under 'squant' the quantisation errors of every output row sum to at most half a quantum (plus the float32
    roundings between t and the stored value: four of them, each within 2^-24 of max(|l|, |h|, scale) relatively, taken as
    row_len * 2^-21 * max(|l|, |h|, scale)); under nearest rounding some row of the same networks does not.  The ranges are
    the rows' or the tensor's own, so no element is clamped."""
    bits, per_channel, signed = cfg
    seeds = [0, 1, 2]
    nets, batch = _batch(name, seeds, engine.device)
    before = [_weights(g) for (_, g, _, _) in nets]
    batch.quantize_squant(bits, 32, per_channel=per_channel, signed=signed, codes=None)
    nearest_exceeds = 0
    for n, seed in enumerate(seeds):
        want = _ref(name, seed, cfg, before[n])
        for k, m in _targ(nets[n][1]):
            rows = m.weight.shape[0]
            w0 = before[n][k].reshape(rows, -1).astype(np.float64)
            q = m.weight.detach().cpu().numpy().reshape(rows, -1).astype(np.float64)
            ref = want[k]
            for r in range(rows):
                scale = float(ref['scale'][r])
                l, h = (float(v) for v in ref['ranges'][r])
                if signed:
                    l, h = -max(abs(l), abs(h)), max(abs(l), abs(h))
                assert w0[r].min() >= l and w0[r].max() <= h            # nothing is clamped
                slack = w0.shape[1] * 2.0 ** -21 * max(abs(l), abs(h), scale)
                err = abs(math.fsum(q[r] - w0[r]))
                assert err <= 0.5 * scale + slack, '{} net {} {} row {}: {} > {} + {}'.format(name, n, k, r, err, 0.5 * scale, slack)
                # nearest rounding, on the restatement alone
                _, _, _, _, min_value = qparams(ref['ranges'][r, 0], ref['ranges'][r, 1], bits, signed)
                y0 = ((ref['c0'][r] * ref['scale'][r]).astype(F32) + min_value).astype(np.float64)
                nearest_exceeds += abs(math.fsum(y0 - w0[r])) > 0.5 * scale
    assert nearest_exceeds > 0, 'no row of these networks exceeds half a quantum under nearest rounding: the test shows nothing'
