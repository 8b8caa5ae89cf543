"""Adversarial inputs for the cross-layer equalisation engines (dfq_le.hip, dfq_le_resident.hip, dfq_le_lazy.hip, dfq_le_cf.hpp)
and the stand-alone steps of dfq_prims.hip: data built against the code instead of drawn at random.

The NaN rule (include/dfq_hip.h, DESIGN.md "NaN rule of the channel ranges"): a NaN of any sign or payload, quiet or
signalling, takes no part in a channel's min / max; a channel without a non-NaN value gets S = s_hi, 1/S = inv_hi; infinities
and denormals are ordinary values.  The oracle states it as channel_ranges(..., nan='skip'); without a NaN in the data the
two oracle modes are the same function, so the other special values are checked against the unmodified ('propagate') oracle.

Channels of a pair are independent (dfq.py:50-73 is per channel), so one run plants SEVERAL cases in different channels: the
four NaN kinds of section 2 sit in four rows and four columns of one pair, the special values of section 3 in nine
channels, and the planted extrema of section 5 in EVERY row and column at once (each with its own position: a dropped
load slot, unroll slot, lane or tail loop changes some channel's answer with certainty).  Every check is bit-exact; every
engine equals the same oracle output, hence every engine equals every other.

Every case runs on the CPU emulation and, marked gpu, on the MI355X.  The C library's fminf / fmaxf return a NaN for a
signalling operand, as the raw v_min_f32 / v_max_f32 do, and the host form of quiet_nan() quiets for real, so the emulation
shows a lane that loses its accumulated extremum behind a signalling NaN wherever the loaded value reaches the min / max
unchanged (the bootstrap, the stand-alone range kernels, the bias-correction range block, LayGeneral::val).  Where the kernel
multiplies by a factor that is 1 at run time (LayFixed, LayShort, the lazy-scale passes) the host's multiplication has already
quieted the NaN, while the GPU compiler may fold the multiplication away: those sites, and the GPU's expanded 1/x and sqrtf
of the denormal cases, are judged by the GPU run only.

Trimmed on the emulation (its resident launch is slow), engines and NaN kinds untouched: the NaN positions are 'first',
'v1', 'last' and 'all' instead of all eight, and the planted extrema run two phases of positions instead of all."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import dfq_oracle as orc
from oracle import graphspec
from dfq_amd import dfq, fxgraph, prims, synthetic
from dfq_amd.utils import layer_transform as lt
from dfq_amd.utils import quantize as q
from dfq_amd.utils import relation as rel

from common import F32, LE_ENGINES, TARG, _select_le_engine, assert_bitexact, assert_close, npy, snapshot

# one engine per tile body (as test_engine_parity.test_layer_equalization_shapes)
_SHAPE_ENGINES = [e for e in LE_ENGINES if e not in ('resident-cf', 'streaming-cf2', 'streaming-bg2', 'streaming-bg4', 'streaming-bg8',
                                                     'streaming-persistent-3wg')]
PAIRS = [
    ((24, 8, 1, 1), (40, 24, 1, 1)),         # float4 rows, pointwise columns
    ((33, 7, 3, 3), (20, 33, 3, 3)),         # odd sizes: scalar tiles, 3x3 columns
    ((32, 1, 3, 3), (16, 32, 1, 1)),         # depthwise first layer
    ((16, 8, 1, 1), (16, 1, 5, 5)),          # depthwise second layer
    ((128, 12, 1, 1), (200, 128, 1, 1)),     # the bootstrap's wide-column path
]
NAN_BITS = [0x7fc00000, 0xffc00000, 0x7f800001, 0xff800001]        # +quiet, -quiet, +signalling (small payload), -signalling
NAN_POS = ['first', 'last', 'v0', 'v1', 'v2', 'v3', 'all']
FLT_MAX = float(np.finfo(F32).max)
DENORM_MIN = float(np.float32(2.0 ** -149))


def _nan(bits):
    return np.array([bits], dtype=np.uint32).view(F32)[0]


def _on_gpu(engine):
    return engine.device.type == 'cuda'


def _base(s1, s2, seed=0):
    rng = np.random.default_rng(1000 * seed + s1[0] * 7 + s2[0])
    w1 = rng.standard_normal(s1).astype(F32)
    w2 = (rng.standard_normal(s2) * 0.2).astype(F32)
    o1 = s1[0]
    return w1, w2, rng.standard_normal(o1).astype(F32), (np.abs(rng.standard_normal(o1)) + 0.1).astype(F32), rng.standard_normal(o1).astype(F32)


def _cols_view(w2, o1):
    """w2 as [G, go, I2g, khkw]: column of channel c = (g, ii) is v[g, :, ii, :] (a view: writes land in w2)"""
    i2g = w2.shape[1]
    G = o1 // i2g if o1 != i2g else 1
    return w2.reshape(G, w2.shape[0] // G, i2g, -1)


def _plant_nans(w1, w2, pos):
    """The four NaN kinds at position `pos` of four rows of W1 and of four columns of W2 (eight different channels).
    'v0'..'v3': the float4 component -- element 4m + k of a row; channel 4m + k of a pointwise column (the wide-column path
    and the float4 tiles hold four channels per register quad).  Returns the planted channels (rows, columns)."""
    o1 = w1.shape[0]
    a1 = w1.reshape(o1, -1)
    L = a1.shape[1]
    cv = _cols_view(w2, o1)
    G, go, i2g, kk = cv.shape
    k = int(pos[1]) if pos[0] == 'v' else 1
    rows, cols = [], []
    for i, bits in enumerate(NAN_BITS):
        cc = 4 * i + k                          # columns 4i + k, rows two further: eight different channels (o1 >= 16)
        rc = (cc + 2) % o1
        g, ii = cc // i2g, cc % i2g
        if pos == 'all':
            a1[rc, :] = _nan(bits)
            cv[g, :, ii, :] = _nan(bits)
        else:
            e = {'first': 0, 'last': L - 1}.get(pos, min(L - 1, 4 * ((L // 4) // 2) + k))
            a1[rc, e] = _nan(bits)
            j, t = {'first': (0, 0), 'last': (go - 1, kk - 1)}.get(pos, (go // 2, kk // 2))
            cv[g, j, ii, t] = _nan(bits)
            # the channel's extrema are the two elements in FRONT of the NaN (row order; (row j, tap) order of a column): a lane that
            # loses what it has accumulated when it meets the NaN loses the channel's range with certainty, not by the luck of the draw
            if e >= 2:
                a1[rc, e - 1], a1[rc, e - 2] = 6.0, -6.0
            m = j * kk + t
            if m >= 2:
                cv[g, (m - 1) // kk, ii, (m - 1) % kk], cv[g, (m - 2) // kk, ii, (m - 2) % kk] = 1.5, -1.5
        rows.append(rc)
        cols.append(cc)
    return rows, cols


def _run_sweeps(engine, runner, arrs, signed, eps, sweeps, nan, what):
    """`sweeps` single-pair sweeps of `runner` on copies of arrs = (w1, w2, b1, bn_weight, bn_bias), each compared bit for bit with
    the oracle's; returns the first sweep's S and the final tensors."""
    o = [a.copy() for a in arrs]
    t = [engine.to(torch.from_numpy(a.copy())) for a in arrs]
    S_first = None
    for sweep in range(sweeps):
        if runner == 'prims':
            S = prims.le_pair(t[0], t[1], t[2], t[3], t[4], signed=signed, eps=eps)
        else:
            S = dfq._layer_equalization(t[0], t[1], t[2], t[3], t[4], signed=signed, eps=eps)[3]
        S_o = orc.layer_equalization(o[0], o[1], o[2], o[3], o[4], signed=signed, eps=eps, nan=nan)
        assert_bitexact(npy(S), S_o, '{} sweep {}: S'.format(what, sweep))
        for got, want, name in zip(t, o, ('w1', 'w2', 'b1', 'bn_weight', 'bn_bias')):
            assert_bitexact(npy(got), want, '{} sweep {}: {}'.format(what, sweep, name))
        if sweep == 0:
            S_first = npy(S)
    return S_first, [npy(x) for x in t]


def _check_nan_channels(arrs, S, out, rows, cols, pos, what):
    """S = s_hi on all-NaN channels; the planted elements are still NaN and every other element of their channel is finite, i.e. was
    scaled (its value is pinned by the oracle comparison)."""
    w1, w2 = arrs[0], arrs[1]
    o1 = w1.shape[0]
    was1, now1 = np.isnan(w1.reshape(o1, -1)), np.isnan(out[0].reshape(o1, -1))
    was2, now2 = np.isnan(_cols_view(w2, o1)), np.isnan(_cols_view(out[1], o1))
    assert np.array_equal(was1, now1), what + ': the NaN pattern of W1 changed'
    assert np.array_equal(was2, now2), what + ': the NaN pattern of W2 changed'
    assert np.isfinite(out[0][~np.isnan(out[0])]).all() and np.isfinite(out[1][~np.isnan(out[1])]).all(), what
    assert not np.isnan(S).any(), what + ': a NaN reached S'
    if pos == 'all':
        for c in rows + cols:
            assert S[c] == F32(1e8), '{}: all-NaN channel {} has S = {}'.format(what, c, S[c])
    else:
        for c in rows + cols:
            assert F32(1e-8) < S[c] < F32(1e8), '{}: channel {} with one NaN has S = {}'.format(what, c, S[c])


def _positions(engine):
    return NAN_POS if _on_gpu(engine) else ['first', 'v1', 'last', 'all']


# ---------------------------------------------------------------------------------------------------------------------
# 2. NaN of every kind, every position, every engine
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('s1,s2', PAIRS)
@pytest.mark.parametrize('signed', [False, True])
@pytest.mark.parametrize('runner', _SHAPE_ENGINES + ['prims'])
def test_nan_is_skipped(engine, monkeypatch, s1, s2, signed, runner):
    """Both range modes, two sweeps, the four NaN kinds in a row of W1 and in a column of W2 at the channel's first / last element
    and in each float4 component, and whole rows / columns of NaN: S and the five tensors are the nan='skip' oracle's."""
    if runner != 'prims':
        _select_le_engine(monkeypatch, runner)
    for pos in _positions(engine):
        arrs = list(_base(s1, s2))
        rows, cols = _plant_nans(arrs[0], arrs[1], pos)
        what = '{} {}->{} signed={} NaN at {}'.format(runner, s1, s2, signed, pos)
        S, out = _run_sweeps(engine, runner, arrs, signed, 0, 2, 'skip', what)
        _check_nan_channels(arrs, S, out, rows, cols, pos, what)


@pytest.mark.parametrize('signed', [False, True])
@pytest.mark.parametrize('le_engine', ['resident', 'streaming', 'streaming-general'])
def test_one_nan_quoted_case(engine, monkeypatch, le_engine, signed):
    """The case that exposed the resident engine: (33,7,3,3)->(20,33,3,3), w1[4].flat[1] and w2[1,6,0,0] NaN (the NaN that
    inf - inf gives on x86: negative quiet).  Channel 6 must end at the NaN-skipping scale, neither at s_hi (the NaN propagated) nor
    at the scale of a range whose maximum the NaN won."""
    _select_le_engine(monkeypatch, le_engine)
    s1, s2 = (33, 7, 3, 3), (20, 33, 3, 3)
    for bits in NAN_BITS:
        arrs = list(_base(s1, s2, seed=1))
        arrs[0][4].flat[1] = _nan(bits)
        arrs[1][1, 6, 0, 0] = _nan(bits)
        S, _ = _run_sweeps(engine, le_engine, arrs, signed, 0, 2, 'skip', '{} signed={} bits={:#x}'.format(le_engine, signed, bits))
        assert F32(1e-8) < S[6] < F32(1e8) and F32(1e-8) < S[4] < F32(1e8)


class _Pair(nn.Module):
    def __init__(self, s1, s2):
        super().__init__()
        g1 = s1[0] if (s1[1] == 1 and s1[2] > 1) else 1
        g2 = s1[0] // s2[1]
        self.c1 = nn.Conv2d(s1[1] * g1, s1[0], s1[2], groups=g1)
        self.b1 = nn.BatchNorm2d(s1[0])
        self.c2 = nn.Conv2d(s2[1] * g2, s2[0], s2[2], groups=g2)

    def forward(self, x):
        return self.c2(torch.relu(self.b1(self.c1(x))))


def _pair_net(engine, s1, s2, w1, w2, seed):
    """conv - BN - ReLU - conv with the given weights, BN folded: (graph, relations) for the engines and the oracle's twin"""
    model = _Pair(s1, s2).eval()
    synthetic.init_weights(model, torch.Generator().manual_seed(seed))
    graph, bottoms = fxgraph.trace(model)
    spec = graphspec.from_torch(graph, bottoms, TARG)
    model.to(engine.device)
    lt.merge_batchnorm(model, graph, bottoms, TARG)
    orc.merge_batchnorm(spec)
    rels = rel.create_relation(graph, bottoms, TARG)
    assert len(rels) == 1
    keys = [k for k in graph if type(graph[k]) in TARG]
    with torch.no_grad():
        for k, w in zip(keys, (w1, w2)):
            graph[k].weight.copy_(torch.from_numpy(w.copy()).to(engine.device))
            spec.nodes[k].weight = w.copy()
    return graph, rels, spec


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


def _check_net(graph, rels, spec, signed, sweeps, nan, what):
    n_o, S_o = orc.cross_layer_equalization(spec, orc.create_relation(spec), signed=signed, max_sweeps=sweeps, converge_thres=-1.0,
                                            converge_count=10 ** 9, nan=nan)
    osnap, esnap = _spec_snapshot(spec), snapshot(graph)
    for k in osnap:
        assert_bitexact(esnap[k], osnap[k], '{} {}'.format(what, k))
    for r, s in zip(rels, S_o):
        assert_bitexact(npy(r.get_scale_vec()), s, what + ' cumulative S')


@pytest.mark.parametrize('s1,s2', PAIRS)
@pytest.mark.parametrize('signed', [False, True])
def test_nan_in_a_batch_leaves_the_clean_network_alone(engine, monkeypatch, s1, s2, signed):
    """A two-network batch plan (the streaming engine with its deferred stores and lazy sweeps) whose first network carries the
    NaNs and whose second is clean: the first equals the nan='skip' oracle, the second its single-network run -- both bit for bit."""
    _select_le_engine(monkeypatch, 'streaming')
    cfg = dict(signed=signed, max_sweeps=2, converge_thres=-1.0, converge_count=10 ** 9)
    for pos in _positions(engine):
        w1, w2 = _base(s1, s2)[:2]
        _plant_nans(w1, w2, pos)
        c1, c2 = _base(s1, s2, seed=2)[:2]
        dirty = _pair_net(engine, s1, s2, w1, w2, 3)
        clean = _pair_net(engine, s1, s2, c1, c2, 4)
        alone = _pair_net(engine, s1, s2, c1, c2, 4)
        plan = dfq.build_le_plan_batch([dirty[:2], clean[:2]], TARG)
        plan.run(**cfg)
        results, all_done = plan.query_all()
        plan.stage.writeback()
        plan.close()
        assert all_done and [r['sweeps'] for r in results] == [2, 2]
        single = dfq.build_le_plan(alone[0], alone[1], TARG)
        single.run(**cfg)
        single.stage.writeback()
        single.close()
        what = 'batch {}->{} signed={} NaN at {}'.format(s1, s2, signed, pos)
        _check_net(dirty[0], dirty[1], dirty[2], signed, 2, 'skip', what + ' (NaN network)')
        _check_net(clean[0], clean[1], clean[2], signed, 2, 'propagate', what + ' (clean network)')
        a, b = snapshot(clean[0]), snapshot(alone[0])
        for k in b:
            assert_bitexact(a[k], b[k], what + ': clean network vs its own run, ' + k)


@pytest.mark.parametrize('s1,s2', PAIRS)
@pytest.mark.parametrize('signed', [False, True])
def test_nan_lazy_scale_plan(engine, s1, s2, signed):
    """The lazy-scale plan (dfq_le_lazy.hip: read-only sweeps from the pristine weights and the cumulative scales).  One sweep is
    the oracle's bit for bit.  After two sweeps the cumulative S is still the oracle's bit for bit (the ranges of scaled channels
    are the scaled extrema exactly); the tensors carry ONE rounding of w0 * (s1 * s2) where the sequential loop rounds twice --
    this formulation's documented 1e-5 contract -- so they are compared within 1e-5 on the numbers and exactly on the NaN pattern."""
    for pos in _positions(engine):
        for sweeps in (1, 2):
            w1, w2 = _base(s1, s2)[:2]
            _plant_nans(w1, w2, pos)
            graph, rels, spec = _pair_net(engine, s1, s2, w1, w2, 5)
            dfq.lazy_cross_layer_equalization(graph, rels, TARG, sweeps, signed=signed)
            what = 'lazy-scale {}->{} signed={} NaN at {}, {} sweeps'.format(s1, s2, signed, pos, sweeps)
            if sweeps == 1:
                _check_net(graph, rels, spec, signed, 1, 'skip', what)
                continue
            _, S_o = orc.cross_layer_equalization(spec, orc.create_relation(spec), signed=signed, max_sweeps=2, converge_thres=-1.0,
                                                  converge_count=10 ** 9, nan='skip')
            assert_bitexact(npy(rels[0].get_scale_vec()), S_o[0], what + ' cumulative S')
            osnap, esnap = _spec_snapshot(spec), snapshot(graph)
            for k in osnap:
                assert np.array_equal(np.isnan(esnap[k]), np.isnan(osnap[k])), what + ' NaN pattern of ' + k
                assert_close(np.nan_to_num(esnap[k]), np.nan_to_num(osnap[k]), what + ' ' + k)


@pytest.mark.parametrize('path', ['resident', 'streaming', 'lazy-sweeps'])
def test_whole_loop_with_one_nan_weight(engine, monkeypatch, path):
    """tiny_mobile with one NaN weight through cross_layer_equalization: the |dW| mean of its layer is NaN in every sweep, and
    the reference's Python comparisons (dfq.py:110-115: `abs(diff - diff_tmp) > 1e-9` is False, `diff` keeps its 10) then count 20
    sweeps.  Sweep count and every tensor are the oracle's on the resident launch, the streaming launches, and a batched plan with
    lazy sweeps."""
    _select_le_engine(monkeypatch, 'resident' if path == 'resident' else 'streaming')
    nets = []
    for seed in ((0,) if path != 'lazy-sweeps' else (0, 1)):
        model, graph, bottoms = synthetic.build('tiny_mobile', seed=seed)
        spec = graphspec.from_torch(graph, bottoms, TARG)
        model.to(engine.device)
        lt.merge_batchnorm(model, graph, bottoms, TARG)
        orc.merge_batchnorm(spec)
        rels = rel.create_relation(graph, bottoms, TARG)
        kf = rels[1].get_idxs()[0]                                     # a layer in the interior of a chain
        with torch.no_grad():
            graph[kf].weight.view(-1)[5] = float('nan')
        spec.nodes[kf].weight.reshape(-1)[5] = np.nan
        nets.append((graph, rels, spec))
    if path == 'lazy-sweeps':
        plan = dfq.build_le_plan_batch([n[:2] for n in nets], TARG)
        plan.run()
        results, all_done = plan.query_all()
        plan.stage.writeback()
        plan.close()
        assert all_done
        sweeps = [r['sweeps'] for r in results]
    else:
        dfq.cross_layer_equalization(nets[0][0], nets[0][1], TARG)
        sweeps = [dfq.last_equalization['sweeps']]
    for (graph, rels, spec), n in zip(nets, sweeps):
        n_o, S_o = orc.cross_layer_equalization(spec, orc.create_relation(spec), nan='skip')
        assert n_o == 20 and n == n_o, (path, n, n_o)
        osnap, esnap = _spec_snapshot(spec), snapshot(graph)
        for k in osnap:
            assert_bitexact(esnap[k], osnap[k], '{} {}'.format(path, k))
        for r, s in zip(rels, S_o):
            assert_bitexact(npy(r.get_scale_vec()), s, path + ' cumulative S')


# ---------------------------------------------------------------------------------------------------------------------
# 3. other special values: zero, overflow, denormal, infinity, -0, FLT_MAX (no NaN in the data: the unmodified oracle)
# ---------------------------------------------------------------------------------------------------------------------
def _plant_specials(w1, w2):
    """Nine channels of one pair, one special case each (the remaining channels stay ordinary)."""
    o1 = w1.shape[0]
    a1 = w1.reshape(o1, -1)
    cv = _cols_view(w2, o1)
    i2g = cv.shape[2]

    def col(c):
        return cv[c // i2g, :, c % i2g, :]
    a1[0, :] = 0.0; col(0)[...] = 0.0                                  # both layers' channel zero
    a1[1, 0] = 3e38; col(1)[...] *= F32(1e30)                          # r1 * r2 = inf
    a1[2, :] *= F32(1e-41); col(2)[...] *= F32(1e-42)                  # denormal rows and columns (denormal * denormal = 0)
    a1[3, -1] = np.inf                                                 # a single +inf
    a1[4, 0] = np.inf; a1[4, -1] = -np.inf                             # +inf and -inf in one row
    a1[5, :] = -0.0; col(5)[...] = -0.0                                # all -0
    a1[6, 0] = FLT_MAX; col(6)[0, 0] = -FLT_MAX                        # FLT_MAX in both layers
    a1[7, :] = 0.0; a1[7, a1.shape[1] // 2] = DENORM_MIN               # a row whose range is the smallest denormal
    col(8)[-1, -1] = np.inf                                            # an infinite column
    if o1 > 9:
        a1[9, :] = -0.0; a1[9, 0] = -DENORM_MIN                        # range 2^-149 from the negative side


@pytest.mark.parametrize('s1,s2', PAIRS)
@pytest.mark.parametrize('signed', [False, True])
@pytest.mark.parametrize('runner', _SHAPE_ENGINES + ['prims'])
def test_special_values(engine, monkeypatch, s1, s2, signed, runner):
    """eps = 0 beside eps = 1e-8, two sweeps: bit-exact against the unmodified oracle.  (The denormal and overflow channels are
    where the GPU's expanded 1/x and sqrtf could differ from the host's.)"""
    if runner != 'prims':
        _select_le_engine(monkeypatch, runner)
    for eps in (0, 1e-8):
        arrs = list(_base(s1, s2, seed=3))
        _plant_specials(arrs[0], arrs[1])
        with np.errstate(all='ignore'):
            S, out = _run_sweeps(engine, runner, arrs, signed, eps, 2, 'propagate', '{} {}->{} signed={} eps={}'.format(runner, s1, s2, signed, eps))
        if eps == 0:
            assert S[0] == F32(1e8) and S[5] == F32(1e8)              # dead channels: NaN through the clamp -> s_hi
        assert np.array_equal(np.signbit(out[0].reshape(s1[0], -1)[5]), np.ones(out[0].reshape(s1[0], -1).shape[1], bool))    # -0 stays -0


# ---------------------------------------------------------------------------------------------------------------------
# 4. le_solve edge table
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('s_range', [(1e-8, 1e8), (0.5, 0.5), (2, 0.5), (1e-45, 3e38)])
@pytest.mark.parametrize('eps', [0, 1e-8])
def test_le_solve_edge_table(engine, eps, s_range):
    """r1, r2 over {0, -0, 2^-149, 1e-30, 1, 1e30, FLT_MAX, inf, -inf, NaN} squared; (2, 0.5) has hi < lo (hi_gt_lo = 0)."""
    vals = np.array([0.0, -0.0, DENORM_MIN, 1e-30, 1.0, 1e30, FLT_MAX, np.inf, -np.inf, np.nan], dtype=F32)
    r1 = np.repeat(vals, len(vals))
    r2 = np.tile(vals, len(vals))
    so, invo = orc.le_solve(r1, r2, s_range, eps)
    s, inv = prims.le_solve(engine.to(torch.from_numpy(r1.copy())), engine.to(torch.from_numpy(r2.copy())), s_range=s_range, eps=eps)
    bad = [(float(a), float(b), float(x), float(y)) for a, b, x, y in zip(r1, r2, npy(s), so)
           if not (x == y or (np.isnan(x) and np.isnan(y)))]
    assert not bad, 'S differs at (r1, r2, got, want): {}'.format(bad[:8])
    assert_bitexact(npy(s), so, 'S')
    assert_bitexact(npy(inv), invo, '1/S')
    if s_range[1] > s_range[0]:
        assert ((npy(s) >= F32(s_range[0])) & (npy(s) <= F32(s_range[1]))).all()
    # the upper end itself is NOT kept (Python's `s < hi`): where s == hi exactly the reference multiplies by float32(1 / hi)
    at_hi = np.array([1.0], dtype=F32)
    s1, inv1 = prims.le_solve(engine.to(torch.from_numpy(at_hi.copy())), engine.to(torch.from_numpy(at_hi.copy())), s_range=(1 / 3, 1.0))
    so1, invo1 = orc.le_solve(at_hi, at_hi, (1 / 3, 1.0))
    assert_bitexact(npy(s1), so1)
    assert_bitexact(npy(inv1), invo1)


def test_le_solve_boundary_uses_the_double_reciprocal(engine):
    """s == float32(s_hi) exactly is replaced by the Python float hi (`s < hi` is False), so 1/S is float32(1.0 / hi) formed in
    double from the DOUBLE hi, not the float32 reciprocal of float32(hi).  For an upper end that is no float32 number the two
    can differ in the last place; such an end is searched for, and r1 = 1, r2 = fl(h * h) lands on it (a correctly rounded sqrt
    returns h) -- `s <= s_hi` in le_solve is caught here."""
    found = None
    for m in range(1, 4000):
        hi = m / 997.0
        h32 = F32(hi)
        if F32(1.0 / hi) != F32(F32(1.0) / h32) and F32(np.sqrt(F32(h32 * h32))) == h32:
            found = hi
            break
    assert found is not None
    r1 = np.array([1.0], dtype=F32)
    r2 = np.array([F32(found) * F32(found)], dtype=F32)
    so, invo = orc.le_solve(r1, r2, (1e-8, found))
    assert so[0] == F32(found) and invo[0] == F32(1.0 / found) and invo[0] != F32(F32(1.0) / so[0])      # the case bites
    s, inv = prims.le_solve(engine.to(torch.from_numpy(r1.copy())), engine.to(torch.from_numpy(r2.copy())), s_range=(1e-8, found))
    assert_bitexact(npy(s), so)
    assert_bitexact(npy(inv), invo, '1/S at s == s_hi')


# ---------------------------------------------------------------------------------------------------------------------
# 5. planted extrema in every load tier of le_bootstrap_kernel and of the first sweep's tiles
# ---------------------------------------------------------------------------------------------------------------------
_TIER_PAIRS = [
    ((130, 8, 1, 1), (6, 130, 1, 1)),        # short rows, vector: eight rows per trip, a full and a clamped trip
    ((130, 7, 1, 1), (6, 130, 1, 1)),        # short rows, scalar
    ((5, 2052), (3, 5)),                     # long rows, vector: the 8-deep trip twice plus the clamped tail
    ((5, 2051), (3, 5)),                     # long rows, scalar
    ((128, 12, 1, 1), (200, 128, 1, 1)),     # wide columns: eight unrolled j slots and the tail loop
    ((144, 24, 1, 1), (24, 144, 1, 1)),      # wide columns, a partial block
    ((33, 7, 3, 3), (20, 33, 3, 3)),         # generic columns, khkw 9
    ((16, 8, 1, 1), (40, 16, 5, 5)),         # generic columns, khkw 25
    ((96, 12, 1, 1), (64, 48, 1, 1)),        # grouped pair: blocks straddle a group -> generic path
]
_TIER_ENGINES = ['resident', 'streaming', 'streaming-general', 'streaming-fused', 'lazy-scale']


def _row_positions(L):
    """Elements of a row where a load tier begins or ends: the float4 components, the row's first / last element, lanes 0 / 63 / 64 /
    255 of the first trip (vector index = lane), every unroll slot of the 8-deep trip (64 vectors apart), the second trip, the tail."""
    if L <= 64:
        return list(range(L))
    vec = [0, 1, 63, 64, 65, 127, 128, 191, 192, 255, 256, 319, 320, 383, 384, 447, 448, 511, 512, (L - 1) // 4 - 1, (L - 1) // 4]
    pos = set()
    for i, v in enumerate(vec):
        for k in ((0, 1, 2, 3) if i < 4 else (i % 4,)):
            pos.add(min(L - 1, 4 * v + k))
    pos.update((0, L - 1, L - 2, L - 3, L - 4))
    return sorted(pos)


def _plant_extrema(s1, s2, phase):
    """Uniform weights in [-1, 1]; EVERY row of W1 and EVERY column of W2 gets one +4 and one -4, at a position that depends on
    the channel and on `phase` -- over the phases every listed row position and every (row j, tap) of a column holds each sign once."""
    rng = np.random.default_rng(77 + phase)
    w1 = rng.uniform(-1, 1, s1).astype(F32)
    w2 = rng.uniform(-1, 1, s2).astype(F32)
    o1 = s1[0]
    a1 = w1.reshape(o1, -1)
    P = _row_positions(a1.shape[1])
    for r in range(o1):
        a1[r, P[(phase * o1 + r) % len(P)]] = 4.0
        a1[r, P[(phase * o1 + r + len(P) // 2 + 1) % len(P)]] = -4.0
    cv = _cols_view(w2, o1)
    G, go, i2g, kk = cv.shape
    n = go * kk
    for c in range(o1):
        col = cv[c // i2g, :, c % i2g, :]
        hi, lo = (phase * o1 + c) % n, (phase * o1 + c + n // 2 + 1) % n
        col[hi // kk, hi % kk] = 4.0
        col[lo // kk, lo % kk] = -4.0
    return w1, w2


def _tier_phases(s1, s2):
    o1 = s1[0]
    L = int(np.prod(s1[1:]))
    n = (s2[0] // (o1 // s2[1] if o1 != s2[1] else 1)) * int(np.prod(s2[2:]))
    return max(-(-len(_row_positions(L)) // o1), -(-n // o1))


# (the lazy-scale plan has no bootstrap, so DFQ_LE_BOOT_WORK does not reach it, and it takes its pairs from a traced network: conv
# geometries only, the default boot work only; one and two sweeps)
# boot_work 2^20: ONE workgroup per channel block -- by default the 200 rows of the wide-column pair are cut into four slices of 50,
# fewer than the 64 rows of an 8-deep trip, and only the tail loop runs
_TIER_CASES = [(s1, s2, bw, r) for r in _TIER_ENGINES for bw in (None, 40, 1 << 20) for s1, s2 in _TIER_PAIRS
               if r != 'lazy-scale' or (bw is None and len(s1) == 4)]


@pytest.mark.parametrize('s1,s2,boot_work,runner', _TIER_CASES)
def test_planted_extrema(engine, monkeypatch, s1, s2, boot_work, runner):
    """One +4 and one -4 in every channel: a dropped vector component, unroll slot, lane, clamped trip or tail loop changes a range
    with certainty.  Two sweeps, both range modes, bit-exact against the oracle; DFQ_LE_BOOT_WORK=40 makes several workgroups share
    a channel block (their statistics merge through atomicMax), 2^20 gives a block to one workgroup (the 8-deep loops run)."""
    if runner != 'lazy-scale':
        _select_le_engine(monkeypatch, runner)
    if boot_work:
        monkeypatch.setenv('DFQ_LE_BOOT_WORK', str(boot_work))
    phases = _tier_phases(s1, s2)
    if not _on_gpu(engine):
        phases = min(phases, 2)
    for phase in range(phases):
        signed = bool(phase & 1)
        w1, w2 = _plant_extrema(s1, s2, phase)
        what = '{} {}->{} phase {} boot_work={}'.format(runner, s1, s2, phase, boot_work)
        if runner == 'lazy-scale':
            for sweeps in (1, 2):          # (every S is exactly 1 here, so w0 * (s1 * s2) rounds like the sequential loop: bit-exact after two sweeps too)
                graph, rels, spec = _pair_net(engine, s1, s2, w1, w2, 6)
                dfq.lazy_cross_layer_equalization(graph, rels, TARG, sweeps, signed=signed)
                _check_net(graph, rels, spec, signed, sweeps, 'propagate', '{}, {} sweeps'.format(what, sweeps))
                assert_bitexact(npy(rels[0].get_scale_vec()), np.ones(s1[0], dtype=F32), what + ': cumulative S')
            continue
        b1 = np.linspace(-1, 1, s1[0]).astype(F32)
        S, _ = _run_sweeps(engine, runner, (w1, w2, b1, np.abs(b1) + F32(0.5), b1[::-1].copy()), signed, 0, 2, 'propagate', what)
        assert_bitexact(S, np.ones(s1[0], dtype=F32), what + ': every channel has range (-4, 4) on both sides')


# ---------------------------------------------------------------------------------------------------------------------
# 6. the same vectors through prims.row_range / prims.col_range
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('s1,s2', PAIRS)
@pytest.mark.parametrize('signed', [False, True])
def test_prims_ranges_on_the_adversarial_vectors(engine, s1, s2, signed):
    o1 = s1[0]
    cases = []
    for pos in NAN_POS:
        w1, w2 = _base(s1, s2)[:2]
        _plant_nans(w1, w2, pos)
        cases.append(('NaN at ' + pos, w1, w2, 'skip'))
    w1, w2 = _base(s1, s2, seed=3)[:2]
    _plant_specials(w1, w2)
    cases.append(('special values', w1, w2, 'propagate'))
    for what, w1, w2, nan in cases:
        cols = np.transpose(_cols_view(w2, o1), (0, 2, 1, 3)).reshape(o1, -1)
        with np.errstate(all='ignore'):
            r1o = orc.channel_ranges(w1.reshape(o1, -1), signed, nan)
            r2o = orc.channel_ranges(cols, signed, nan)
        assert_bitexact(npy(prims.row_range(engine.to(torch.from_numpy(w1.copy())), signed)), r1o, what + ': row ranges')
        assert_bitexact(npy(prims.col_range(engine.to(torch.from_numpy(w2.copy())), o1, signed)), r2o, what + ': column ranges')
        if nan == 'skip':
            assert not np.isnan(r1o).any() and not np.isnan(r2o).any()


# ---------------------------------------------------------------------------------------------------------------------
# 7. bias correction: the per-tensor (min, max) block
# ---------------------------------------------------------------------------------------------------------------------
_BC_BLOCK = 256                  # kBlock of dfq_common.hpp
_BC_CHUNK = 64 * _BC_BLOCK       # kMmChunk of dfq_bc.hip: floats per workgroup of the range pass


def _bc_schedule(n, lane):
    """bc_minmax_block restated: what lane `lane` of the workgroup of a tensor's first chunk folds into its (min, max), in order, as
    (loop, first element): 'quad' = a slot of the four-loads-per-trip loop, 'single' = the one-vector loop, 'tail' = the scalar tail."""
    e = min(n, _BC_CHUNK)
    e4 = e & ~3
    out, i = [], 4 * lane
    while i + 12 * _BC_BLOCK < e4:
        out += [('quad', i + u * 4 * _BC_BLOCK) for u in range(4)]
        i += 16 * _BC_BLOCK
    while i < e4:
        out.append(('single', i))
        i += 4 * _BC_BLOCK
    out += [('tail', j) for j in range(e4 + lane, e, _BC_BLOCK)]
    return out


def _bc_sites(n):
    """{site: (elements of the two extrema, element of the NaN)}: the NaN is component 0 of a vector (the component that meets the
    lane's accumulator directly) or a tail element, the extrema are components 1 and 2 of the vector the SAME lane folded just before."""
    sites = {}
    for lane in (3, 0):
        sch = _bc_schedule(n, lane)
        for p in range(1, len(sch)):
            kind = sch[p][0]
            if kind == 'quad':
                kind = 'quad, next slot' if p % 4 else 'quad, next trip'
            if sch[p - 1][0] != 'tail':
                sites.setdefault(kind, ((sch[p - 1][1] + 1, sch[p - 1][1] + 2), sch[p][1]))
    return sites


def _bc_net(engine, which):
    if which == 'tiny_tail':                  # its 200 x 48 pointwise layer: two trips of the four-load loop, then the one-vector loop
        model, graph, bottoms = synthetic.build('tiny_tail', seed=1)
    else:                                     # a second layer of 35 x 11 x 3 x 3 = 3465 = 4 * 866 + 1 floats: a scalar tail behind the four-load loop
        model = _Pair((11, 3, 1, 1), (35, 11, 3, 3)).eval()
        synthetic.init_weights(model, torch.Generator().manual_seed(7))
        graph, bottoms = fxgraph.trace(model)
    model.to(engine.device)
    lt.merge_batchnorm(model, graph, bottoms, TARG)
    return graph, bottoms


def test_bias_correction_range_skips_nan(engine, monkeypatch):
    """A NaN of each kind BEHIND the tensor's extrema in the lane that holds them, in every loop of bc_minmax_block: the next
    unroll slot and the next trip of the four-loads-per-trip loop, the one-vector loop and the scalar tail.  (A signalling NaN
    that meets the accumulator directly makes a raw min / max return the NaN; the following step keeps its other operand and
    the extrema are gone.  Only component 0 of a vector meets the accumulator: the other three are combined among themselves first.)
    tiny_mobile's largest tensor has 864 floats and the four-load loop needs more than 12 * 256 in a chunk, so the tensors are
    tiny_tail's 200 x 48 layer and a 35 x 11 x 3 x 3 convolution (3465 floats: a tail).  The plan does not export its (min, max);
    the quantisation-error row sums it produces are (DFQ_BC_EPS=1), and those of the rows without a NaN equal the oracle's row
    sums under the (min, max) that dfq_tensor_minmax takes of the same data -- bit for bit, which pins both ends of the range."""
    monkeypatch.setenv('DFQ_BC_EPS', '1')
    covered = set()
    for which in ('tiny_tail', 'odd conv'):
        graph, bottoms = _bc_net(engine, which)
        plan, keys = dfq.build_bc_plan(graph, bottoms, TARG)
        step = int(np.argmax([graph[k].weight.numel() for k in keys]))
        w = graph[keys[step]].weight
        flat = w.detach().view(-1)
        n = flat.numel()
        rng = np.random.default_rng(9)
        for site, ((hi, lo), at) in sorted(_bc_sites(n).items()):
            covered.add(site)
            for bits in NAN_BITS:
                data = rng.standard_normal(n).astype(F32)
                data[hi] = 7.0; data[lo] = -9.0; data[at] = _nan(bits)
                with torch.no_grad():
                    flat.copy_(torch.from_numpy(data).to(engine.device))
                mm = npy(q.tensor_minmax(flat))
                assert mm[0] == F32(-9.0) and mm[1] == F32(7.0), (which, site, hex(bits), mm)
                plan.run()
                wn = data.reshape(tuple(w.shape))
                with np.errstate(all='ignore'):
                    want = _rowsum_given_range(wn, float(mm[0]), float(mm[1]))
                got = npy(plan.eps(step)).reshape(want.shape)
                clean = ~np.isnan(want)                                # an (output row, input channel) cell without a NaN tap
                assert clean.sum() > 0 and (~clean).sum() > 0
                assert_bitexact(got[clean], want[clean], '{}, NaN {:#x} at {} ({}) behind the extrema at {}, {}: quantisation-error row '
                                'sums under the NaN-skipping range'.format(which, bits, at, site, hi, lo))
        plan.close()
    assert covered == {'quad, next slot', 'quad, next trip', 'single', 'tail'}, covered      # every loop was reached


def _rowsum_given_range(w, mn, mx):
    """orc.quant_error_rowsum (dfq.py:216-219) with the tensor's (min, max) given instead of taken with a propagating min() / max()"""
    eps = (orc.uniform_quantize(w, 8, mn, mx, False) - w).astype(F32)
    e3 = eps.reshape(w.shape[0], w.shape[1], -1)
    acc = np.zeros(e3.shape[:2], dtype=F32)
    for k in range(e3.shape[2]):                                       # fixed left-to-right float32 order
        acc = (acc + e3[:, :, k]).astype(F32)
    return acc
