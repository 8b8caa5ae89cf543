"""NetworkBatch.squant_plan(widths=), dfq_batch_squant_plan_set_widths and quantize_mixed(rounding='squant'): adaptive rounding
(SQuant) of a whole batch with every (network, layer) at a width of its own, read on the device.

The reference is the numpy restatement of the definition (tests/test_squant_rows.py) at each layer's own width; the
definition is integer-exact, so weights (as bit patterns), codes, ranges and stats are compared exactly.  The three
architectures hold rows of every lane class of the rows kernel (8 ... 200 weights), rows of 1600 (the long-rows kernel) and
kernels of 1, 9 and 25 elements."""
import numpy as np
import pytest
import torch

from dfq_amd import _ffi, arena, dfq

from common import TARG
from test_batch_squant import _biases, _prepared, _targ, _weights
from test_squant_rows import F32, HALF, bits_of, row_range, squant_ref

NAMES = ['tiny_mobile', 'tiny_wide', 'tiny_tail']
SEEDS = [0, 1, 2]
CONFIGS = [(False, False), (True, True), (True, False)]                     # (per_channel, signed)
NARROW, WIDE = (2, 3, 4, 6, 8), (2, 5, 8, 11, 16)                           # candidates for 'int8' codes / for 'int32' and None


def _batch(name, seeds, device):
    """(nets, batch) after merge_batchnorm.  Not equalised: rounding takes the weights as they are, and equalising tiny_wide
    takes minutes on the CPU emulation."""
    nets = [_prepared(name, s, device) for s in seeds]
    return nets, arena.NetworkBatch([(g, b, r) for (_, g, b, r) in nets], TARG)


def _twin(name, seed, device):
    return _prepared(name, seed, device)[1]


def _row_class(row_len):
    """the lanes a row of row_len weights gets: 4 ... 64 of a wave (4 slots each), 'wave', 'workgroup' (dfq_squant_batch.hip)"""
    for lanes in (4, 8, 16, 32, 64):
        if row_len <= 4 * lanes:
            return lanes
    return 'wave' if row_len <= 1536 else 'workgroup'


_REFS = {}


def _ref(name, seed, key, w, bits, per_channel, signed):
    """the restatement of one layer of network (name, seed) at `bits`, computed once"""
    at = (name, seed, key, bits, per_channel, signed, bits_of(w).tobytes())
    if at not in _REFS:
        rows = w.shape[0]
        x = w.reshape(rows, -1)
        K = int(np.prod(w.shape[2:])) if w.ndim > 2 else 1
        mins = maxs = None
        if not per_channel:
            mn, mx = row_range(x.reshape(-1))
            mins, maxs = np.full(rows, mn, F32), np.full(rows, mx, F32)
        _REFS[at] = squant_ref(x, K, bits, signed, mins, maxs)
    return _REFS[at]


def _set_bits(mixed, rows):
    """overwrite the (caller-writable) bits block of a mixed plan: rows[n][t]"""
    mixed.bits_block.copy_(torch.tensor(rows, dtype=torch.int32).to(mixed.bits_block.device))


def _allocated(batch, cands, per_channel, signed, **kw):
    """an allocating plan that has run"""
    mixed = batch.mixed_plan(cands, avg_bits=4, per_channel=per_channel, signed=signed, apply=False, **kw)
    mixed.run()
    return mixed


def _check_layer(name, seed, n, key, m, w0, plan, bits, per_channel, signed, codes):
    what = '{} net {} {} at {} bits'.format(name, n, key, bits)
    want = _ref(name, seed, key, w0, bits, per_channel, signed)
    rows = m.weight.shape[0]
    w = m.weight.detach().cpu().numpy().reshape(rows, -1)
    assert np.array_equal(bits_of(w), bits_of(want['y'])), what + ': stored weights'
    stats = plan.stats(n)[key].cpu().numpy()
    assert np.array_equal(stats, want['stats']), what + ': stats'
    assert np.abs(stats[:, 0]).max() <= HALF, what
    r = plan.ranges(n)[key].cpu().numpy()
    wr = want['ranges'] if per_channel else want['ranges'][0]
    assert np.array_equal(bits_of(r), bits_of(wr)), what + ': ranges'
    if codes is not None:
        c = plan.codes(n)[key]
        assert c.dtype == (torch.int32 if codes == 'int32' else (torch.int8 if signed else torch.uint8))
        assert np.array_equal(c.cpu().numpy().astype(np.int64).reshape(rows, -1), want['codes']), what + ': codes'
    else:
        assert plan.codes(n) == {}


# ---- 1. every class at every width, in one launch ------------------------------------------------------------------------------
# every configuration with every kind of codes for the two small architectures; tiny_wide -- 1600 rows of 70 and 9 rows of 1600,
# half a minute per case on the CPU emulation -- with every configuration and every kind of codes once
CASES = [(name, cfg, codes) for name in ('tiny_mobile', 'tiny_tail') for cfg in CONFIGS for codes in ('int8', 'int32', None)]
CASES += [('tiny_wide', cfg, codes) for cfg, codes in zip(CONFIGS, ('int8', 'int32', None))]


# the row classes and the kernel sizes each architecture brings: together every lane class, the workgroup class, K = 1, 9, 25
SHAPES = {'tiny_mobile': ({4, 8, 16, 32}, {1, 9}), 'tiny_tail': ({4, 8, 16, 64}, {1, 9}), 'tiny_wide': ({8, 32, 'workgroup'}, {1, 9, 25})}


@pytest.mark.parametrize('name,cfg,codes', CASES)
def test_every_class_at_every_width(engine, name, cfg, codes):
    per_channel, signed = cfg
    cands = NARROW if codes == 'int8' else WIDE
    nets, batch = _batch(name, SEEDS, engine.device)
    before = [_weights(g) for (_, g, _, _) in nets]
    bias_before = [_biases(g) for (_, g, _, _) in nets]
    mixed = _allocated(batch, cands, per_channel, signed)
    T, B = mixed.n_tensors, len(cands)
    table = [[cands[(n + t) % B] for t in range(T)] for n in range(len(SEEDS))]
    _set_bits(mixed, table)
    plan = batch.squant_plan(per_channel=per_channel, signed=signed, codes=codes, widths=mixed)
    uniform = batch.squant_plan(cands[0], per_channel=per_channel, signed=signed, codes=codes)
    assert plan.launches == uniform.launches and 1 <= plan.launches <= 3
    uniform.close()
    plan.run()
    _ffi.synchronize()
    seen = {}                                           # row class -> the widths it was rounded at in this run
    for n, seed in enumerate(SEEDS):
        assert plan.status(n) == 0
        for t, (key, m) in enumerate(_targ(nets[n][1])):
            assert key == mixed.keys[t]
            _check_layer(name, seed, n, key, m, before[n][key], plan, table[n][t], per_channel, signed, codes)
            seen.setdefault(_row_class(m.weight.numel() // m.weight.shape[0]), set()).add(table[n][t])
        for k, b in _biases(nets[n][1]).items():
            assert np.array_equal(bits_of(b), bits_of(bias_before[n][k]))
    assert seen and all(len(w) >= 2 for w in seen.values()), 'a row class met one width only: {}'.format(seen)
    kernels = {int(np.prod(m.weight.shape[2:])) if m.weight.dim() > 2 else 1 for _, m in _targ(nets[0][1])}
    assert (set(seen), kernels) == SHAPES[name], 'the shapes the module\'s docstring promises: {} {}'.format(seen, kernels)
    plan.close()
    mixed.close()
    with pytest.raises(RuntimeError):
        plan.run()


# ---- 2. the allocation's own widths ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,cfg', [('tiny_mobile', (False, False)), ('tiny_mobile', (True, True)), ('tiny_tail', (False, False)),
                                      ('tiny_tail', (True, True)), ('tiny_wide', (True, False))])
def test_allocation_then_squant_back_to_back(engine, name, cfg):
    per_channel, signed = cfg
    nets, batch = _batch(name, SEEDS, engine.device)
    nets2, batch2 = _batch(name, SEEDS, engine.device)
    before = [_weights(g) for (_, g, _, _) in nets]
    pin = {_targ(nets[0][1])[0][0]: 8}                  # (a small net may get one width throughout: its first layer is pinned)
    mixed = batch.mixed_plan(NARROW, avg_bits=4, per_channel=per_channel, signed=signed, apply=False, pin=pin)
    plan = batch.squant_plan(per_channel=per_channel, signed=signed, codes='int32', widths=mixed)
    mixed.run()
    plan.run()                                          # (no synchronisation in between: the widths are read on the device)
    nearest = batch2.mixed_plan(NARROW, avg_bits=4, per_channel=per_channel, signed=signed, apply=True, codes='int32', pin=pin)
    nearest.run()
    _ffi.synchronize()
    distinct = set()
    for n, seed in enumerate(SEEDS):
        assert plan.status(n) == 0
        bits = mixed.bits(n)
        assert bits == nearest.bits(n)
        distinct |= set(bits.values())
        for key, m in _targ(nets[n][1]):
            what = '{} net {} {}'.format(name, n, key)
            rows = m.weight.shape[0]
            assert np.array_equal(bits_of(plan.ranges(n)[key].cpu().numpy()), bits_of(nearest.ranges(n)[key].cpu().numpy())), what + ': ranges'
            c = plan.codes(n)[key].cpu().numpy().astype(np.int64).reshape(rows, -1)
            c0 = nearest.codes(n)[key].cpu().numpy().astype(np.int64).reshape(rows, -1)
            assert np.abs(c - c0).max() <= 1, what + ': a code further than one from nearest'
            flips = plan.stats(n)[key].cpu().numpy()[:, 1]
            assert np.array_equal(flips, (c != c0).sum(1)), what + ': the count of flips'
            w = m.weight.detach().cpu().numpy().reshape(rows, -1)
            w0 = nets2[n][1][key].weight.detach().cpu().numpy().reshape(rows, -1)
            same = flips == 0
            assert np.array_equal(bits_of(w[same]), bits_of(w0[same])), what + ': a row without flips'
            _check_layer(name, seed, n, key, m, before[n][key], plan, bits[key], per_channel, signed, 'int32')
    assert len(distinct) >= 2, 'the allocation gave one width only: the test shows nothing'
    for p in (plan, mixed, nearest):
        p.close()


# ---- 3. NULL restores; a dict is the device block ------------------------------------------------------------------------------
def _blocks(nets, plan):
    """everything a run wrote, block padding aside"""
    out = [plan.range_block.cpu().numpy().view(np.uint32), plan.stats_block.cpu().numpy()]
    for n, (_, g, _, _) in enumerate(nets):
        out += [c.cpu().numpy() for c in plan.codes(n).values()]
        out += [bits_of(w) for w in _weights(g).values()]
    return out


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize('cfg', [(False, False), (True, True)])
def test_null_restores_and_dict_is_the_block(engine, cfg):
    per_channel, signed = cfg
    name = 'tiny_tail'
    nets, batch = _batch(name, SEEDS, engine.device)
    nets2, batch2 = _batch(name, SEEDS, engine.device)
    mixed = _allocated(batch, NARROW, per_channel, signed)
    plan = batch.squant_plan(6, per_channel=per_channel, signed=signed, codes='int8')
    plan.set_widths(mixed)
    plan.set_widths(None)
    plan.run()
    fresh = batch2.squant_plan(6, per_channel=per_channel, signed=signed, codes='int8')
    fresh.run()
    _ffi.synchronize()
    assert _same(_blocks(nets, plan), _blocks(nets2, fresh)), 'set_widths(None) is not the plain plan'
    assert [plan.status(n) for n in range(3)] == [0, 0, 0]
    for p in (plan, fresh, mixed):
        p.close()
    # a dict of widths against the device block holding the same values
    nets, batch = _batch(name, SEEDS, engine.device)
    nets2, batch2 = _batch(name, SEEDS, engine.device)
    before = [_weights(g) for (_, g, _, _) in nets]
    keys = [k for k, _ in _targ(nets[0][1])]
    chosen = {k: NARROW[(2 * t + 1) % len(NARROW)] for t, k in enumerate(keys[:-1])}     # (the last layer: bit_weight)
    by_dict = batch.squant_plan(6, per_channel=per_channel, signed=signed, codes='int8', widths=chosen)
    by_dict.run()
    mixed = _allocated(batch2, NARROW, per_channel, signed)
    row = [chosen.get(k, 6) for k in keys]
    _set_bits(mixed, [row] * 3)
    by_block = batch2.squant_plan(per_channel=per_channel, signed=signed, codes='int8', widths=mixed)
    by_block.run()
    _ffi.synchronize()
    assert _same(_blocks(nets, by_dict), _blocks(nets2, by_block)), 'the dict and the device block differ'
    assert by_dict.bits_block.cpu().tolist() == [row] * 3
    # set_widths(None) on a plan made with a dict: the dict's widths again, for the run and for a pack_plan made afterwards
    stale = batch.pack_plan(by_dict)
    by_dict.set_widths(_allocated(batch, NARROW, per_channel, signed))
    assert by_dict.bits_block is not stale.bits_block
    with pytest.raises(RuntimeError):
        stale.run()                                     # (made for the widths of then)
    by_dict.set_widths(None)
    assert by_dict.bits_block.cpu().tolist() == [row] * 3 and by_dict.budget == sum(
        m.weight.numel() * b for (_, m), b in zip(_targ(nets[0][1]), row))
    assert batch.pack_plan(by_dict).widths_array().tolist() == [row] * 3
    stale.run()                                         # (the dict's block again: no longer stale)
    stale.close()
    for n, seed in enumerate(SEEDS):
        for t, (key, m) in enumerate(_targ(nets[n][1])):
            _check_layer(name, seed, n, key, m, before[n][key], by_dict, row[t], per_channel, signed, 'int8')
    for p in (by_dict, by_block, mixed):
        p.close()


# ---- 4. widths that are no widths ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,per_channel', [('tiny_wide', True), ('tiny_tail', False)])
def test_bad_widths_leave_their_tensors_alone(engine, name, per_channel):
    """Input validation: with 'int8' codes the widths 1, 17, 0 and 9 in four layers of network 1 make those (network, tensor)
    items return before they write anything.  tiny_wide: rows of the 8-lane and the 32-lane class and, with the 9, the rows of
    1600 of the long-rows kernel; tiny_tail, per tensor (the range launch in front): the 4-, 8- and 64-lane classes."""
    signed = False
    nets, batch = _batch(name, SEEDS, engine.device)
    before = [_weights(g) for (_, g, _, _) in nets]
    mixed = _allocated(batch, NARROW, per_channel, signed)
    keys = list(mixed.keys)
    T, B = len(keys), len(NARROW)
    table = [[NARROW[(n + t) % B] for t in range(T)] for n in range(3)]
    bad = dict(zip(['Conv2d_1', 'Conv2d_7', 'Conv2d_13', 'Linear_17'] if name == 'tiny_wide' else
                   ['Conv2d_1', 'Conv2d_4', 'Conv2d_7', 'Linear_14'], (1, 17, 0, 9)))
    for key, b in bad.items():
        table[1][keys.index(key)] = b
    _set_bits(mixed, table)
    plan = batch.squant_plan(per_channel=per_channel, signed=signed, codes='int8', widths=mixed)
    plan.stats_block.fill_(-77)
    plan.range_block.fill_(-77.0)
    plan.code_block.fill_(77)
    plan.run()
    _ffi.synchronize()
    assert [plan.status(n) for n in range(3)] == [0, 2, 0]
    for n, seed in enumerate(SEEDS):
        for t, (key, m) in enumerate(_targ(nets[n][1])):
            if n == 1 and key in bad:
                what = '{} net 1 {} at the width {}'.format(name, key, bad[key])
                assert np.array_equal(bits_of(m.weight.detach().cpu().numpy()), bits_of(before[n][key])), what + ': weights'
                assert (plan.stats(n)[key] == -77).all() and (plan.ranges(n)[key] == -77.0).all() and (plan.codes(n)[key] == 77).all(), what
            else:
                _check_layer(name, seed, n, key, m, before[n][key], plan, table[n][t], per_channel, signed, 'int8')
    # valid widths: the status is cleared, and the four layers -- untouched so far -- are rounded
    for key in bad:
        table[1][keys.index(key)] = 3
    _set_bits(mixed, table)
    plan.run()
    _ffi.synchronize()
    assert [plan.status(n) for n in range(3)] == [0, 0, 0]
    for key in bad:
        _check_layer(name, SEEDS[1], 1, key, nets[1][1][key], before[1][key], plan, 3, per_channel, signed, 'int8')
    plan.close()
    mixed.close()


def test_set_widths_argument_errors(engine):
    nets, batch = _batch('tiny_tail', [0], engine.device)
    lib = _ffi.lib()
    DFQ_ERR_ARG = -1
    plan = batch.squant_plan(4)
    T = len(plan.keys)
    blk = torch.full((1, T), 4, dtype=torch.int32, device=engine.device)
    status = torch.zeros((1,), dtype=torch.int32, device=engine.device)
    import ctypes
    idx = (ctypes.c_int32 * T)(*range(T))
    me = b'dfq_batch_squant_plan_set_widths'
    assert lib.dfq_batch_squant_plan_set_widths(None, None, 0, None, None) == DFQ_ERR_ARG and me in lib.dfq_last_error()
    assert lib.dfq_batch_squant_plan_set_widths(plan._plan, _ffi.ptr(blk), T, None, _ffi.ptr(status)) == DFQ_ERR_ARG
    assert lib.dfq_batch_squant_plan_set_widths(plan._plan, _ffi.ptr(blk), T, idx, None) == DFQ_ERR_ARG
    assert lib.dfq_batch_squant_plan_set_widths(plan._plan, _ffi.ptr(blk), T - 1, idx, _ffi.ptr(status)) == DFQ_ERR_ARG
    idx[0] = -1
    assert lib.dfq_batch_squant_plan_set_widths(plan._plan, _ffi.ptr(blk), T, idx, _ffi.ptr(status)) == DFQ_ERR_ARG
    idx[0] = 0
    assert lib.dfq_batch_squant_plan_set_widths(plan._plan, _ffi.ptr(blk), T, idx, _ffi.ptr(status)) == 0
    assert lib.dfq_batch_squant_plan_set_widths(plan._plan, None, 0, None, None) == 0
    plan.close()
    with pytest.raises(RuntimeError):
        plan.set_widths(None)
    for bad in ({'Conv2d_1': 1}, {'Conv2d_1': 17}, {'Conv2d_1': 4.0}, {'Conv2d_1': True}, {'nowhere': 4}, [4]):
        with pytest.raises(ValueError):
            batch.squant_plan(4, widths=bad)
    with pytest.raises(ValueError):
        batch.squant_plan(4, codes='int8', widths={'Conv2d_1': 9})


# ---- 5. the hand-over to the packing ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cfg', [(False, False), (True, True)])
def test_pack_unpack_save_load(engine, cfg, tmp_path):
    per_channel, signed = cfg
    name = 'tiny_mobile'
    nets, batch = _batch(name, SEEDS, engine.device)
    mixed = batch.mixed_plan(NARROW, avg_bits=4, per_channel=per_channel, signed=signed, apply=False)
    plan = batch.squant_plan(per_channel=per_channel, signed=signed, codes='int8', widths=mixed)
    pack = batch.pack_plan(plan)
    mixed.run()
    plan.run()
    pack.run()
    _ffi.synchronize()
    assert [pack.status(n) for n in range(3)] == [0, 0, 0]
    widths = mixed.bits_block.cpu().numpy()
    assert np.array_equal(pack.widths_array(), widths) and len(set(widths.reshape(-1).tolist())) >= 2
    stored = [_weights(g) for (_, g, _, _) in nets]
    codes = [{k: v.cpu().numpy().copy() for k, v in plan.codes(n).items()} for n in range(3)]
    with torch.no_grad():
        for (_, g, _, _) in nets:
            for _, m in _targ(g):
                m.weight.zero_()
    unpack = batch.unpack_plan(pack, weights=True, codes='int8')
    unpack.run()
    _ffi.synchronize()

    def check_back(got_nets, got_codes):
        for n in range(3):
            for key, m in _targ(got_nets[n][1]):
                if got_codes is not None:
                    assert np.array_equal(got_codes(n)[key].cpu().numpy(), codes[n][key]), key
                w, w0 = m.weight.detach().cpu().numpy(), stored[n][key]
                assert np.array_equal(w, w0), key
                assert np.array_equal(bits_of(w)[w0 != 0], bits_of(w0)[w0 != 0]), key
    check_back(nets, unpack.codes)
    path = str(tmp_path / 'squant_widths.npz')
    batch.save_packed(path, plan)
    nets2, batch2 = _batch(name, SEEDS, engine.device)
    loaded = batch2.load_packed(path)
    assert np.array_equal(loaded.widths_array(), widths)
    check_back(nets2, None)
    # a dict's widths are packed from the plan's own block
    nets3, batch3 = _batch(name, SEEDS, engine.device)
    by_dict = batch3.squant_plan(4, per_channel=per_channel, signed=signed, codes='int8', widths={'Conv2d_10': 2, 'Linear_31': 8})
    pack3 = batch3.pack_plan(by_dict)
    by_dict.run()
    pack3.run()
    _ffi.synchronize()
    assert [pack3.status(n) for n in range(3)] == [0, 0, 0]
    want = [{'Conv2d_10': 2, 'Linear_31': 8}.get(k, 4) for k in by_dict.keys]
    assert pack3.widths_array().tolist() == [want] * 3
    assert pack3.size_bits(0) == 32 * sum(arena._extent_words(m.weight.numel(), b) for (_, m), b in zip(_targ(nets3[0][1]), want))
    for p in (plan, mixed, pack, unpack, by_dict, pack3):
        p.close()


# ---- 6. the convenience paths ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cfg', [(False, False), (True, True)])
def test_quantize_mixed_squant_is_the_sequence(engine, cfg):
    per_channel, signed = cfg
    name = 'tiny_mobile'
    nets, batch = _batch(name, SEEDS, engine.device)
    nets2, batch2 = _batch(name, SEEDS, engine.device)
    nets3, batch3 = _batch(name, SEEDS, engine.device)
    codes, ranges, bits = batch.quantize_mixed(NARROW, avg_bits=4, per_channel=per_channel, signed=signed, codes='int8', bits_bias=8,
                                               rounding='squant')
    mixed = batch2.mixed_plan(NARROW, avg_bits=4, per_channel=per_channel, signed=signed, apply=False)
    plan = batch2.squant_plan(per_channel=per_channel, signed=signed, codes='int8', widths=mixed)
    mixed.run()
    plan.run()
    _ffi.synchronize()
    _, ranges3 = batch3.quantize(8, 8, per_channel=per_channel, signed=signed, codes=None)      # (the biases of quantize())
    for n in range(3):
        assert bits[n] == dict(mixed.bits(n))
        for key, m in _targ(nets[n][1]):
            m2 = nets2[n][1][key]
            assert np.array_equal(bits_of(m.weight.detach().cpu().numpy()), bits_of(m2.weight.detach().cpu().numpy())), key
            assert torch.equal(codes[n][key].cpu(), plan.codes(n)[key].cpu()), key
            assert np.array_equal(bits_of(ranges[n][key].cpu().numpy()), bits_of(plan.ranges(n)[key].cpu().numpy())), key
        b1, b3 = _biases(nets[n][1]), _biases(nets3[n][1])
        assert b1 and sorted(b1) == sorted(b3)
        for k in b1:
            assert np.array_equal(bits_of(b1[k]), bits_of(b3[k])), k
            assert np.array_equal(bits_of(ranges[n][k + '.bias'].cpu().numpy()), bits_of(ranges3[n][k + '.bias'].cpu().numpy())), k
    plan.close()
    mixed.close()


@pytest.mark.parametrize('cfg', [(False, False), (True, True)])
def test_quantize_mixed_clip_squant(engine, cfg):
    per_channel, signed = cfg
    name = 'tiny_mobile'
    nets, batch = _batch(name, SEEDS, engine.device)
    nets2, batch2 = _batch(name, SEEDS, engine.device)
    codes, ranges, bits = batch.quantize_mixed(NARROW, avg_bits=4, per_channel=per_channel, signed=signed, codes='int32', bits_bias=32,
                                               clip=8, rounding='squant')
    mixed = batch2.mixed_plan(NARROW, avg_bits=4, per_channel=per_channel, signed=signed, apply=False, clip=8)
    mixed.run(mixed.ALLOCATE | mixed.CLAMP)
    _ffi.synchronize()
    for n, seed in enumerate(SEEDS):
        assert bits[n] == dict(mixed.bits(n))
        clamped = _weights(nets2[n][1])
        for key, m in _targ(nets[n][1]):
            what = '{} net {} {}'.format(name, n, key)
            want = _ref(name + '/clip8', seed, key, clamped[key], bits[n][key], per_channel, signed)
            rows = m.weight.shape[0]
            assert np.array_equal(bits_of(m.weight.detach().cpu().numpy().reshape(rows, -1)), bits_of(want['y'])), what + ': weights'
            assert np.array_equal(codes[n][key].cpu().numpy().astype(np.int64).reshape(rows, -1), want['codes']), what + ': codes'
            assert np.array_equal(ranges[n][key].cpu().numpy(), mixed.ranges(n)[key].cpu().numpy()), what + ': ranges'
        assert not any(k.endswith('.bias') for k in ranges[n])
    mixed.close()


@pytest.mark.parametrize('clip', [None, 8])
def test_single_network_quantize_mixed_squant(engine, clip):
    name, seed = 'tiny_tail', 1
    nets, batch = _batch(name, [seed], engine.device)
    twin = _twin(name, seed, engine.device)
    assert all(np.array_equal(bits_of(a), bits_of(b)) for a, b in zip(_weights(twin).values(), _weights(nets[0][1]).values())), 'twin'
    codes, ranges, bits = batch.quantize_mixed(NARROW, avg_bits=4, per_channel=True, codes='int32', bits_bias=32, clip=clip, rounding='squant')
    out = dfq.quantize_mixed(twin, NARROW, avg_bits=4, per_channel=True, targ_type=TARG, clip=clip, rounding='squant')
    for key, m in _targ(nets[0][1]):
        assert out[key]['bits'] == bits[0][key]
        assert np.array_equal(bits_of(twin[key].weight.detach().cpu().numpy()), bits_of(m.weight.detach().cpu().numpy())), key
        assert np.array_equal(bits_of(out[key]['range']), bits_of(ranges[0][key].cpu().numpy())), key
        assert out[key]['flips'] >= 0 and set(out[key]) >= {'bits', 'err', 'range', 'flips'}
    assert sum(o['flips'] for o in out.values()) > 0
    with pytest.raises(ValueError):
        dfq.quantize_mixed(_twin(name, seed, engine.device), NARROW, avg_bits=4, targ_type=TARG, rounding='stochastic')


@pytest.mark.parametrize('clip', [None, 8])
def test_nearest_is_unchanged(engine, clip):
    name = 'tiny_mobile'
    nets, batch = _batch(name, SEEDS, engine.device)
    nets2, batch2 = _batch(name, SEEDS, engine.device)
    a = batch.quantize_mixed(NARROW, avg_bits=4, per_channel=True, codes='int8', bits_bias=8, clip=clip)
    b = batch2.quantize_mixed(NARROW, avg_bits=4, per_channel=True, codes='int8', bits_bias=8, clip=clip, rounding='nearest')
    for n in range(3):
        assert a[2][n] == b[2][n]
        assert sorted(a[0][n]) == sorted(b[0][n]) and sorted(a[1][n]) == sorted(b[1][n])
        assert all(torch.equal(a[0][n][k].cpu(), b[0][n][k].cpu()) for k in a[0][n])
        assert all(np.array_equal(bits_of(a[1][n][k].cpu().numpy()), bits_of(b[1][n][k].cpu().numpy())) for k in a[1][n])
        for (k, m), (_, m2) in zip(_targ(nets[n][1]), _targ(nets2[n][1])):
            assert np.array_equal(bits_of(m.weight.detach().cpu().numpy()), bits_of(m2.weight.detach().cpu().numpy())), k
    ga, gb = _twin(name, 0, engine.device), _twin(name, 0, engine.device)
    oa = dfq.quantize_mixed(ga, NARROW, avg_bits=4, targ_type=TARG, clip=clip)
    ob = dfq.quantize_mixed(gb, NARROW, avg_bits=4, targ_type=TARG, clip=clip, rounding='nearest')
    for k in oa:
        assert oa[k]['bits'] == ob[k]['bits'] and oa[k]['err'] == ob[k]['err'] and 'flips' not in ob[k]
        assert np.array_equal(bits_of(ga[k].weight.detach().cpu().numpy()), bits_of(gb[k].weight.detach().cpu().numpy())), k


def test_value_errors(engine):
    nets, batch = _batch('tiny_tail', [0, 1], engine.device)
    nets2, batch2 = _batch('tiny_tail', [0, 1], engine.device)
    with pytest.raises(ValueError, match='bias_correction_distill'):
        batch.quantize_mixed(NARROW, avg_bits=4, correct=True, rounding='squant')
    with pytest.raises(ValueError):
        batch.quantize_mixed(NARROW, avg_bits=4, rounding='stochastic')
    other = batch2.mixed_plan(NARROW, avg_bits=4, apply=False)
    with pytest.raises(ValueError):
        batch.squant_plan(widths=other)
    other.close()
    mine = batch.mixed_plan(NARROW, avg_bits=4, apply=False)
    with pytest.raises(ValueError):
        batch.squant_plan(per_channel=True, widths=mine)
    with pytest.raises(ValueError):
        batch.squant_plan(signed=True, widths=mine)
    plan = batch.squant_plan(widths=mine)
    with pytest.raises(ValueError):
        plan.set_widths(other)
    plan.close()
    mine.close()
    with pytest.raises(ValueError):
        batch.squant_plan(widths=mine)
    wide = batch.mixed_plan(WIDE, avg_bits=4, apply=False)
    with pytest.raises(ValueError):
        batch.squant_plan(codes='int8', widths=wide)
    ok = batch.squant_plan(codes='int32', widths=wide)
    ok.close()
    wide.close()
    # the weights of both batches are as they were: nothing above ran
    for (_, g, _, _), (_, g2, _, _) in zip(nets, nets2):
        assert all(np.array_equal(bits_of(a), bits_of(b)) for a, b in zip(_weights(g).values(), _weights(g2).values()))
