"""The bias-correction chain at the edges: bc_step_body (both bodies, the per-channel body, the streaming tail), the three hand-over
protocols, the one-launch form, folded depthwise steps, merge_source and its four-at-a-time poll, relu_mean at both evaluation
sites (bc_cache_init_block, the step / folded tail) -- dfq_amd/csrc/dfq_bc.hip -- on networks whose shapes and values were chosen
to hit the work split's boundaries.  Every network is a small nn.Module traced by dfq_amd.fxgraph.trace, BN-folded by
lt.merge_batchnorm, then weights, biases and BN proxies are written directly.

Reference of one step (independent of the matvec and of the state propagation of orc.bias_correction):
  eps[o, i]  orc.quant_error_rowsum (float32 recipe, pinned bit-exactly elsewhere; test_geometry_sweep also reads it back from a
             DFQ_BC_EPS=1 plan, bit for bit); per-channel runs: the per-row quantiser's (_rowsum_per_channel of test_per_channel.py).
  E          from the proxies the run LEAVES (a BN is rewritten at most once, by a step in front of every reader, so what a step
             read is the final value): a source without ReLU is fake_bias itself (exact, no libm), merges are float32 adds in source
             order and cat appends; the sources and their order come from the oracle's walk (orc.find_prev_bn) and the merged
             vector must equal orc.bn_expectation bit for bit.  A source read through a ReLU: the float64 clipped-normal mean of
             test_act_adversarial.py (_exact_moments), with an allowance of Km u (|b| + w) + 4 eta per channel.
  S[o]       math.fsum_i(eps[o, i] * E[g n + i]), products in float64 (exact for float32 factors).  Layers of more than 512 rows (the
             8192 x 4 layer in FRONT of the layer under test) take numpy's row sum instead and add its (n - 1) 2^-53 sum|.| to the bound.
Bound, derived, not measured (u = 2^-24, eta = 2^-149, n = I / g inputs per row, A = sum_i |eps E|):
    |corr[o] - S| <= u |S| + (n + 8) 2^-53 A + eta  [+ sum_i |eps_i| (Km u (|b_i| + w_i) + 4 eta) for ReLU sources]
one float32 rounding of the row, a float64 accumulation of at most n terms and the six butterfly steps.  The suite's assert_close
allows 1e-5 max(1, |b|) on corrections of size 1e-2: three to four orders more.
Tail, bit for bit given the plan's OWN correction vector: bias_after == fl32(bias_before + (-corr)), next BN's fake_bias ==
fl32(fb_before + (-corr)); every tensor no step rewrites is unchanged (weights, fake_weight, the BNs nobody corrects).  All start
values are random and distinct per row, so a tail row taken from the wrong thread or the wrong workgroup cannot pass.

Non-finite expectations (the finding): the float64 rule -- a row is NaN iff its group holds a NaN product (a NaN factor, or
0 x inf where eps is exactly 0) or infinities of both signs, +-inf if its infinities have one sign, else finite and within the
bound; rows of other groups are untouched.  Until this file the one-group body (the default of a single network) let slots outside
the row and slots nobody owns multiply eps = 0 with a REAL element of the expectation: 0 x inf = NaN in every row of the layer,
where the general body and a batched plan of the same network left +-inf.  Fixed in bc_step_body: such slots read a word of LDS
kept at 0.0f (sh_E[kExp]).  test_nonfinite_expectation fails on the parent commit at its first variant ('default': the
one-group body); on the parent the rule holds only where the general body runs: 'general-body', 'per-position', 'safe-mode'
(a batch of three small networks still gives every wave one group of rows and runs the one-group body).

ReLU moment (section 5): Km = 3.1 = twice the error of orc.relu_mean against float64 over the input set of
test_act_adversarial.py (mode 1: grid, tails to |b / w| = 60, w = 0, w = 1e-30, the overflows), rounded up, because device and host
libm may round pdf / cdf to neighbouring floats:
    oracle vs float64   1.54 u (|b| + w)      chosen Km = 3.1      (test_oracle_relu_mean_error_is_what_the_header_says)
Planted NaN channels of the mean: (w, b) = (0, 0) and (0, -0.0) -- t = 0 / 0.  The overflow channels (1, +-2e19), (0.5, 1e30) have a
finite MEAN (their variance is what overflows) and are compared like every other channel.

Mutations of dfq_bc.hip checked on the emulation (a scratch copy of the fixed file; which tests fail):
    col_u < in  ->  <=  (either body)               geometry[pw3 g6x20x2 g9x22x3 g4x65x2 k9x65], bodies[pw3 .. pw1025, the grouped, src*,
                                                    chain3*, every merge], nonfinite[*-2-*]: bound (an element of the next group, or of the
                                                    LDS behind the expectation, counted with the row's last eps)
    group index from row / (step_o + 1)             geometry and bodies[every grouped and depthwise case], relu_moment_edges[cache-*,
                                                    tail-no-fold], nonfinite[*-2-*]: bound
    streaming tail started one element late         geometry[pw1537 pw2048 pw2049 pw4100 pw8192 g4x1600x2 k9x1537], bodies[pw1537
                                                    g4x1600x2 src2049]: bound
    cur_len not advanced by a cat                   bodies[cat3 cat7 cat-unequal]: bound
    folded tail uses nb where src_relu asks moment  relu_moment_edges[tail-default -general-body -counters -batch-3], bodies[dw9-relu]
    four-at-a-time poll without `i < s.channels`    bodies[every case] and nonfinite[*] under general-body / blocks-1 / batch-3: the slots
                                                    past the source belong to a BN a LATER step writes, or lie behind the table, and
                                                    never carry this run's epoch -- the wait is abandoned and run(check=True) raises
                                                    DFQ_ERR_ABANDONED (checked with a low DFQ_SPIN_LIMIT on the scratch copy only: at
                                                    the default limit the emulation needs minutes to give up)
    the 0 x inf behaviour itself (the parent)       nonfinite[*]: NaN in every row of the layer (rows [3, 4, 5] of a grouped one)
    bias = pre_bias - neg                           every test but the CPU one: the tail identity
    `sub < rw` dropped at the one-group store       SURVIVES on the emulation and cannot be killed there: the unowned sub-rows hold a sum
                                                    of 0.0 and land in the sh_corr entries of the NEXT wave, which the emulation runs
                                                    afterwards and which overwrites them (ordering between waves); behind the last
                                                    wave they land past the rows the tail reads.  On the device it is a race.
    `r_local < rw` dropped everywhere               equivalent, not a fault: without the filter a slot computes the row the next wave
                                                    owns, from the same weights and the same expectation, and stores the same bits
                                                    into the same entry (at most 3 rw + 63 < kBlock); the filter saves work.
NOT visible to the fiber emulation, which runs a workgroup's threads one after the other between barriers and whose atomics are
sequentially consistent: the ordering between waves and workgroups (the store filter above, a missing barrier behind a merge, a
plain load where a device-scope load is needed).  Those are what the gpu-marked runs of the same tests are for.

Found by this file besides the NaN: a folded depthwise step left -0.0 where the step on its own leaves +0.0 (eps exactly 0 and a
negative expectation: the fold's single product was not added to a sum that starts at +0.0) -- test_geometry_sweep[dw1] compares
the folded plan with DFQ_BC_FOLD=0 bit for bit.  Fixed in the folded tail.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn as nn

from dfq_amd import _ffi, dfq, fxgraph
from dfq_amd.utils import layer_transform as lt
from oracle import dfq_oracle as orc
from oracle import graphspec
from tests.common import F32, TARG, assert_bitexact, npy
from tests.test_act_adversarial import _INPUTS, _exact_moments
from tests.test_per_channel import _rowsum_per_channel

DFQ_ERR_ARG = -1                # include/dfq_hip.h
U = 2.0 ** -24
ETA = 2.0 ** -149
D = 2.0 ** -53
KM = 3.1                        # header: twice ORACLE_KM, rounded up
ORACLE_KM = 1.54                # orc.relu_mean against float64 over _INPUTS, in u (|b| + w)
FSUM_ROWS = 512                 # layers of more rows are summed by numpy (header)
_ENV = ('DFQ_BC_ONE_GROUP', 'DFQ_BC_BLOCKS', 'DFQ_BC_TAGGED', 'DFQ_BC_MERGED', 'DFQ_BC_ONE_LAUNCH', 'DFQ_BC_FOLD', 'DFQ_BC_EPS',
        'DFQ_BC_SKEW', 'DFQ_BC_MM_AHEAD', 'DFQ_BC_MM_CHUNK', 'DFQ_GRAPH')


# ---- the networks -------------------------------------------------------------------------------------------------------
class _Fan(nn.Module):
    """stem(3 -> c0) - BN0 [- ReLU] - conv1(c0 -> C, 1x1) - BN1 [- ReLU] - heads: conv(C -> O, k x k, groups) - BN each.
    The stem is fed by the data and is no step; conv1 reads a BN nobody rewrites (tag_off = -1) and rewrites BN1; every head reads
    BN1 through the slots of the launch (tag_off >= 0) and rewrites the BN behind it.  A depthwise head directly behind conv1
    with at most nine taps is folded into conv1's tail."""

    def __init__(self, C, heads, c0=4, relu0=False, relu1=False):
        super().__init__()
        self.relu0, self.relu1 = relu0, relu1
        self.stem, self.bn0 = nn.Conv2d(3, c0, 1), nn.BatchNorm2d(c0)
        self.conv1, self.bn1 = nn.Conv2d(c0, C, 1), nn.BatchNorm2d(C)
        self.heads = nn.ModuleList([nn.Conv2d(C, o, k, padding=k // 2, groups=g) for (o, k, g) in heads])
        self.tails = nn.ModuleList([nn.BatchNorm2d(o) for (o, k, g) in heads])

    def forward(self, x):
        x = self.bn0(self.stem(x))
        if self.relu0:
            x = torch.relu(x)
        x = self.bn1(self.conv1(x))
        if self.relu1:
            x = torch.relu(x)
        return tuple(bn(h(x)) for h, bn in zip(self.heads, self.tails))


class _Chain3(nn.Module):
    """stem - BN0 [ReLU] - conv1 - BN1 [ReLU] - conv2 - BN2 [ReLU] - conv3: the middle layer's source is never rewritten (read from
    memory, wait_cache under one-launch when behind a ReLU), the last two read BNs rewritten inside the launch; conv3 has no BN
    behind it (next_bn_bias null)."""

    def __init__(self, c1, c2, c3, relus=(False, False, False), c0=5):
        super().__init__()
        self.relus = relus
        self.stem, self.bn0 = nn.Conv2d(3, c0, 1), nn.BatchNorm2d(c0)
        self.conv1, self.bn1 = nn.Conv2d(c0, c1, 1), nn.BatchNorm2d(c1)
        self.conv2, self.bn2 = nn.Conv2d(c1, c2, 1), nn.BatchNorm2d(c2)
        self.conv3 = nn.Conv2d(c2, c3, 1)

    def forward(self, x):
        x = self.bn0(self.stem(x))
        if self.relus[0]:
            x = torch.relu(x)
        x = self.bn1(self.conv1(x))
        if self.relus[1]:
            x = torch.relu(x)
        x = self.bn2(self.conv2(x))
        if self.relus[2]:
            x = torch.relu(x)
        return self.conv3(x)


class _Merge(nn.Module):
    """stem - BN0 - branches conv(c0 -> n_i) - BN_i, merged by `mode`, - conv(total -> O) - BN.  Every branch BN is rewritten inside
    the launch; the last layer merges them: 'add', 'cat', 'mixed' = cat(c, a + b), 'mixed2' = c + cat(a, b).  The reference's walk
    (find_prev_bn) keeps ONE connection type per depth and sorts the sources by depth, deepest first: it reads these two as
    [a, +b, cat c] and [a, cat b, +c]; with the operands the other way round it reads an add of unequal lengths, which the
    plan refuses like the reference's own torch.add would."""

    def __init__(self, parts, mode, out=5, c0=4):
        super().__init__()
        self.mode = mode
        self.stem, self.bn0 = nn.Conv2d(3, c0, 1), nn.BatchNorm2d(c0)
        self.convs = nn.ModuleList([nn.Conv2d(c0, n, 1) for n in parts])
        self.bns = nn.ModuleList([nn.BatchNorm2d(n) for n in parts])
        total = sum(parts) if mode == 'cat' else parts[0] + parts[2] if mode == 'mixed' else parts[-1]
        self.last, self.bn_last = nn.Conv2d(total, out, 1), nn.BatchNorm2d(out)

    def forward(self, x):
        x = self.bn0(self.stem(x))
        ys = [bn(c(x)) for c, bn in zip(self.convs, self.bns)]
        if self.mode == 'add':
            y = ys[0]
            for z in ys[1:]:
                y = y + z
        elif self.mode == 'cat':
            y = torch.cat(ys, 1)
        elif self.mode == 'mixed':
            y = torch.cat([ys[2], ys[0] + ys[1]], 1)
        else:
            y = ys[-1] + torch.cat(ys[:-1], 1)
        return self.bn_last(self.last(y))


class _Direct(nn.Module):
    """stem(3 -> C) - BN0 - ReLU - depthwise(C, k x k) - BN: the ONE step reads a BN nobody rewrites through a ReLU -- its moment
    comes from bc_cache_init_block (a trailing block of the range launch, or a block of the one launch)."""

    def __init__(self, C, k):
        super().__init__()
        self.stem, self.bn0 = nn.Conv2d(3, C, 1), nn.BatchNorm2d(C)
        self.dw, self.bn1 = nn.Conv2d(C, C, k, padding=k // 2, groups=C), nn.BatchNorm2d(C)

    def forward(self, x):
        return self.bn1(self.dw(torch.relu(self.bn0(self.stem(x)))))


def _state(graph):
    out = {}
    for k, m in graph.items():
        if type(m) in TARG:
            out[k] = dict(w=npy(m.weight), b=npy(m.bias))
        elif isinstance(m, nn.BatchNorm2d) and hasattr(m, 'fake_bias'):
            out[k] = dict(fw=npy(m.fake_weight), fb=npy(m.fake_bias))
    return out


def _load(graph, state):
    with torch.no_grad():
        for k, vals in state.items():
            m = graph[k]
            for name, v in vals.items():
                t = {'w': 'weight', 'b': 'bias', 'fw': 'fake_weight', 'fb': 'fake_bias'}[name]
                getattr(m, t).copy_(torch.from_numpy(v).to(getattr(m, t).device))


def _copy(state):
    return {k: {n: v.copy() for n, v in vals.items()} for k, vals in state.items()}


class _Net:
    """One traced, BN-folded network on the engine's device with random start values, and its reference."""

    def __init__(self, engine, factory, seed, tweak=None):
        model = factory().eval()
        self.graph, self.bottoms = fxgraph.trace(model)
        model.to(engine.device)
        lt.merge_batchnorm(model, self.graph, self.bottoms, TARG)
        self.model = model
        rng = np.random.default_rng(seed)
        state = {}
        for k, m in self.graph.items():
            if type(m) in TARG:
                state[k] = dict(w=(rng.standard_normal(tuple(m.weight.shape)) * 0.3).astype(F32),
                                b=rng.standard_normal(m.weight.shape[0]).astype(F32))
            elif isinstance(m, nn.BatchNorm2d):
                n = m.weight.numel()
                state[k] = dict(fw=rng.uniform(0.5, 2.0, n).astype(F32), fb=rng.standard_normal(n).astype(F32))
        if tweak is not None:
            tweak(self, state)
        self.start = state
        _load(self.graph, state)
        # structure: the oracle's walk (dfq.py:194-270 restated in oracle/dfq_oracle.py), with the BN each step's correction goes to
        self.spec = spec = graphspec.from_torch(self.graph, self.bottoms, TARG)
        self.steps = []                     # [layer key, entries of bn_expectation, key of the next BN or None]
        bn_seen, relu_attached, pending = set(), {}, None
        for key in spec.order:
            bot = spec.bottoms[key]
            if bot is None or bot[0] == 'Data':
                continue
            node = spec.nodes[key]
            if node.kind == 'bn':
                bn_seen.add(key)
                relu_attached[key] = False
                if pending is not None:
                    self.steps[pending][2] = key
                    pending = None
                continue
            if node.kind == 'relu' and bot[0] in bn_seen:
                relu_attached[bot[0]] = True
            if node.kind == 'targ':
                bn_list, relu_list, connect_list = orc.find_prev_bn(spec, bn_seen, relu_attached, list(bot))
                self.steps.append([key, [(bn_list[i], relu_list[i], connect_list[i]) for i in range(len(bn_list))], None])
                pending = len(self.steps) - 1
        self.keys = [s[0] for s in self.steps]
        self._eps = {}

    def key_of(self, module):
        return next(k for k, m in self.graph.items() if m is module)

    def eps(self, kind):
        """row sums of the quantisation error of every corrected layer: kind 0 = per tensor (8 bit), else per-row at `kind` bits"""
        if kind not in self._eps:
            rowsum = orc.quant_error_rowsum if kind == 0 else _rowsum_per_channel(kind)
            self._eps[kind] = {k: rowsum(self.start[k]['w'], signed=False) for k in self.keys}
        return self._eps[kind]


def _expect_exact(spec, entries):
    """(float64 value, allowance) of a step's expectation vector, merged in the order of orc.bn_expectation"""
    lst = sorted(entries, key=lambda x: len(x[0][1]), reverse=True)

    def one(ent):
        (bn_key, _), use_relu, _ = ent
        n = spec.nodes[bn_key]
        fw, fb = n.fake_weight.astype(np.float64), n.fake_bias.astype(np.float64)
        if use_relu:
            with np.errstate(all='ignore'):
                return _exact_moments(1, n.fake_weight, n.fake_bias)[0], KM * U * (np.abs(fb) + fw) + 4 * ETA
        return fb, np.zeros_like(fb)

    val, err = one(lst[0])
    for ent in lst[1:]:
        v, e = one(ent)
        if ent[2] == 'cat':
            val, err = np.concatenate([val, v]), np.concatenate([err, e])
        elif not err.any() and not e.any():
            with np.errstate(all='ignore'):
                val = (val.astype(F32) + v.astype(F32)).astype(F32).astype(np.float64)         # the float32 add of the reference
        else:
            with np.errstate(all='ignore'):
                val = val + v
                err = err + e + U * np.abs(val) + ETA
    return val, err


def _verify(net, before, after, corrs, what, kind=0):
    """the assertions of the header for one run of one network; returns the worst |corr - S| / bound over the finite rows"""
    spec = net.spec
    for k, vals in after.items():
        if 'fb' in vals:
            spec.nodes[k].fake_weight, spec.nodes[k].fake_bias = vals['fw'], vals['fb']
    worst, rewritten = 0.0, set()
    for s, (key, entries, nxt) in enumerate(net.steps):
        tag = '{} step {} ({})'.format(what, s, key)
        with np.errstate(all='ignore'):
            e32 = orc.bn_expectation(spec, entries)
        val, err = _expect_exact(spec, entries)
        if not err.any():
            assert_bitexact(val.astype(F32), e32, tag + ': expectation against orc.bn_expectation')
        eps = net.eps(kind)[key]
        O, n = eps.shape
        G = len(e32) // n
        assert G * n == len(e32) and O % G == 0, tag
        gidx = np.arange(O) // (O // G)
        e64 = eps.astype(np.float64)
        corr = np.asarray(corrs[s], dtype=F32)
        assert corr.shape == (O,), tag
        with np.errstate(all='ignore'):
            P = e64 * e32.astype(np.float64).reshape(G, n)[gidx]          # IEEE products: 0 x inf and NaN factors are NaN
            want_nan = np.isnan(P).any(1) | (np.isposinf(P).any(1) & np.isneginf(P).any(1))
            want_pos, want_neg = ~want_nan & np.isposinf(P).any(1), ~want_nan & np.isneginf(P).any(1)
            Pv = e64 * val.reshape(G, n)[gidx]
            allow = (np.abs(e64) * err.reshape(G, n)[gidx]).sum(1)
        assert np.array_equal(np.isnan(corr), want_nan), '{}: NaN rows {}, the float64 rule gives {}'.format(
            tag, np.flatnonzero(np.isnan(corr)).tolist()[:12], np.flatnonzero(want_nan).tolist()[:12])
        assert np.array_equal(np.isposinf(corr), want_pos) and np.array_equal(np.isneginf(corr), want_neg), \
            '{}: +inf rows {} / -inf rows {}, the float64 rule gives {} / {}'.format(
                tag, np.flatnonzero(np.isposinf(corr)).tolist()[:12], np.flatnonzero(np.isneginf(corr)).tolist()[:12],
                np.flatnonzero(want_pos).tolist()[:12], np.flatnonzero(want_neg).tolist()[:12])
        for o in np.flatnonzero(~(want_nan | want_pos | want_neg)):
            A = float(np.abs(Pv[o]).sum())
            if O <= FSUM_ROWS:
                S, own = math.fsum(Pv[o]), 0.0
            else:
                S, own = float(Pv[o].sum()), (n - 1) * D * A
            if err.any():
                own += D * A                                              # the products eps * E64 are rounded here
            bound = U * abs(S) + (n + 8) * D * A + ETA + float(allow[o]) + own
            d = abs(float(corr[o]) - S)
            assert d <= bound, '{} row {}: corr {!r}, exact {!r}: off by {:.3e} > {:.3e}'.format(tag, o, corr[o], S, d, bound)
            if bound > 0:
                worst = max(worst, d / bound)
        with np.errstate(all='ignore'):
            neg = (-corr).astype(F32)
            assert_bitexact(after[key]['b'], (before[key]['b'] + neg).astype(F32), tag + ': bias == fl32(bias + (-corr))')
            if nxt is not None:
                assert_bitexact(after[nxt]['fb'], (before[nxt]['fb'] + neg).astype(F32), tag + ': next fake_bias == fl32(fb + (-corr))')
                rewritten.add(nxt)
    for k, vals in after.items():
        for name, v in vals.items():
            if name in ('w', 'fw') or (name == 'fb' and k not in rewritten) or (name == 'b' and k not in net.keys):
                assert_bitexact(v, before[k][name], '{}: {} of {} must not change'.format(what, name, k))
    return worst


# ---- running a plan ------------------------------------------------------------------------------------------------------
VARIANTS = {
    'default': ({}, {}),
    'general-body': ({'DFQ_BC_ONE_GROUP': '0'}, {}),
    'blocks-1': ({'DFQ_BC_BLOCKS': '1'}, {}),                    # many rows per wave, several slot groups
    'batch-3': ({}, {'batch': True}),
    'per-channel-8': ({}, {'bits': 8}),
    'per-channel-5': ({}, {'bits': 5}),
    'counters': ({'DFQ_BC_TAGGED': '0'}, {}),
    'per-position': ({'DFQ_BC_MERGED': '0'}, {}),
    'one-launch': ({'DFQ_BC_ONE_LAUNCH': '1'}, {}),
    'no-fold': ({'DFQ_BC_FOLD': '0'}, {}),
    'safe-mode': ({}, {'safe': True}),
}
PER_TENSOR = [v for v in VARIANTS if not v.startswith('per-channel')]


def _run_plan(monkeypatch, nets, variant, starts=None, repeat=2):
    """One plan under `variant` (a batch over all of `nets`, else nets[0] alone), run from every state of `starts` (of nets[0];
    default: its own start) `repeat` times -- successive tagged runs alternate parity and epoch.  Returns ([per start: per network:
    (after, corrections)], info); asserts that a repeated run repeats the first bit for bit."""
    env, opts = VARIANTS[variant]
    use = nets if opts.get('batch') else nets[:1]
    starts = [use[0].start] if starts is None else starts
    with monkeypatch.context() as mp:
        for k in _ENV:
            mp.delenv(k, raising=False)
        for k, v in env.items():
            mp.setenv(k, v)
        for net in use:
            _load(net.graph, net.start)
        if opts.get('batch'):
            plan = dfq.build_bc_plan_batch([(net.graph, net.bottoms) for net in use], TARG)
        else:
            plan, keys = dfq.build_bc_plan(use[0].graph, use[0].bottoms, TARG)
            assert keys == use[0].keys, (keys, use[0].keys)
        if opts.get('safe'):
            plan.set_safe_mode()
            assert not plan.has_waits
        kw = dict(per_channel=True, bits=opts['bits']) if 'bits' in opts else {}
        results = []
        for start in starts:
            first = None
            for rep in range(repeat):
                for i, net in enumerate(use):
                    _load(net.graph, start if i == 0 else net.start)
                plan.run(check=True, recover=False, **kw)
                res, base = [], 0
                for net in use:
                    res.append((_state(net.graph), [npy(plan.correction(base + j)) for j in range(len(net.steps))]))
                    base += len(net.steps)
                if first is None:
                    first = res
                else:
                    for (a0, c0), (a1, c1) in zip(first, res):
                        for k in a0:
                            for name in a0[k]:
                                assert_bitexact(a1[k][name], a0[k][name], '{}: run {} of the same plan, {} of {}'.format(variant, rep, name, k))
                        for j, (x, y) in enumerate(zip(c0, c1)):
                            assert_bitexact(y, x, '{}: run {} of the same plan, correction of step {}'.format(variant, rep, j))
            results.append(first)
        info = dict(folded=plan.folded_steps, chain=plan.chain_steps, tagged=plan.tagged, one_launch=plan.one_launch,
                    steps=len(use[0].steps))
        plan.close()
    return results, info


def _same(a, b, what):
    (sa, ca), (sb, cb) = a, b
    for k in sa:
        for name in sa[k]:
            assert_bitexact(sb[k][name], sa[k][name], '{}: {} of {}'.format(what, name, k))
    for j, (x, y) in enumerate(zip(ca, cb)):
        assert_bitexact(y, x, '{}: correction of step {}'.format(what, j))


def _kind(variant):
    return VARIANTS[variant][1].get('bits', 0)


# ---- the cases ------------------------------------------------------------------------------------------------------------
I_SWEEP = [1, 2, 3, 5, 9, 17, 33, 63, 64, 65, 128, 129, 512, 513, 1024, 1025, 1536, 1537, 2048, 2049, 4100, 8192]
O_SWEEP = [1, 3, 4, 5, 13]
O_LARGE = 293                   # I <= 129: 64 / lanes rows per slot, up to 256 rows per workgroup -- the last workgroup is partly filled
GROUPED = [(6, 20, 2), (9, 22, 3), (4, 65, 2), (4, 1600, 2), (8, 1024, 8)]      # (O, I, groups); the last: I g = 8192

GEOMETRY = {}
for _i in I_SWEEP:
    GEOMETRY['pw{}'.format(_i)] = (lambda i=_i: _Fan(i, [(o, 1, 1) for o in O_SWEEP + ([O_LARGE] if i <= 129 else [])]))
for _o, _i, _g in GROUPED:
    GEOMETRY['g{}x{}x{}'.format(_o, _i, _g)] = (lambda o=_o, i=_i, g=_g: _Fan(i * g, [(o, 1, g)]))
for _k in (1, 3, 5):            # khkw 1, 9, 25: 25 > kFoldTaps, that step is not folded
    GEOMETRY['dw{}'.format(_k * _k)] = (lambda k=_k: _Fan(70, [(70, k, 70)]))
for _i in (65, 1537):           # wide rows of 3 x 3 taps
    GEOMETRY['k9x{}'.format(_i)] = (lambda i=_i: _Fan(i, [(5, 3, 1)]))
FOLDED = {'dw1': 1, 'dw9': 1, 'dw25': 0, 'pw1': 1}      # (pw1: the head of ONE channel behind a layer of one channel is a depthwise layer)

BODIES = {k: GEOMETRY[k] for k in ['pw1', 'pw2', 'pw3', 'pw5', 'pw9', 'pw17', 'pw33', 'pw65', 'pw513', 'pw1025', 'pw1537',
                                   'dw1', 'dw9', 'dw25'] + ['g{}x{}x{}'.format(*g) for g in GROUPED]}
BODIES['dw9-relu'] = lambda: _Fan(70, [(70, 3, 70)], relu1=True)                 # the folded tail hands the MOMENT over
BODIES['dw25-relu'] = lambda: _Fan(70, [(70, 5, 70)], relu0=True, relu1=True)
for _c in (255, 256, 257, 1023, 1024, 1025, 2049):                               # source lengths around the strides of merge_source
    BODIES['src{}'.format(_c)] = (lambda c=_c: _Fan(c, [(3, 1, 1)]))
BODIES['chain3'] = lambda: _Chain3(40, 300, 7)
BODIES['chain3-relu'] = lambda: _Chain3(40, 300, 7, relus=(True, False, True))    # wait_cache under one-launch; a polled moment
BODIES['add2'] = lambda: _Merge([257, 257], 'add')
BODIES['cat3'] = lambda: _Merge([30, 64, 7], 'cat')
BODIES['cat7'] = lambda: _Merge([9, 16, 5, 64, 33, 1, 12], 'cat')                # more than kStepSources: the table path
BODIES['cat-unequal'] = lambda: _Merge([5, 64, 257], 'cat')
BODIES['mixed'] = lambda: _Merge([64, 64, 257], 'mixed')
BODIES['mixed2'] = lambda: _Merge([60, 70, 130], 'mixed2')


# ---- 1 / 2. geometry ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', list(GEOMETRY))
def test_geometry_sweep(engine, monkeypatch, case):
    """Every boundary of the work split under the default plan, against the bound of the header; the row sums of eps read back
    from a DFQ_BC_EPS=1 plan are the oracle's bit for bit and that plan computes the same bits; depthwise steps behind the BN
    their producer rewrites are folded by default (at most kFoldTaps taps) and not with DFQ_BC_FOLD=0."""
    net = _Net(engine, GEOMETRY[case], 0)
    (res,), info = _run_plan(monkeypatch, [net], 'default')
    after, corrs = res[0]
    worst = _verify(net, net.start, after, corrs, case)
    print('{}: worst |corr - S| / bound = {:.3f}'.format(case, worst))
    assert info['tagged'] and info['folded'] == FOLDED.get(case, 0) and info['chain'] == info['steps'] - info['folded']
    if case in FOLDED:
        (res0,), info0 = _run_plan(monkeypatch, [net], 'no-fold', repeat=1)
        assert info0['folded'] == 0 and info0['chain'] == info0['steps']
        _same(res[0], res0[0], case + ' folded against DFQ_BC_FOLD=0')
    # the materialised row sums
    with monkeypatch.context() as mp:
        for k in _ENV:
            mp.delenv(k, raising=False)
        mp.setenv('DFQ_BC_EPS', '1')
        _load(net.graph, net.start)
        plan, keys = dfq.build_bc_plan(net.graph, net.bottoms, TARG)
        plan.run(check=True, recover=False)
        for j, k in enumerate(keys):
            assert_bitexact(npy(plan.eps(j)), net.eps(0)[k], '{}: eps of {}'.format(case, k))
        _same(res[0], (_state(net.graph), [npy(plan.correction(j)) for j in range(len(keys))]), case + ' with DFQ_BC_EPS=1')
        plan.close()


def test_expectation_of_8193_channels_is_refused(engine, monkeypatch):
    """I x groups = 8193 does not fit the expectation's LDS: DFQ_ERR_ARG with the message that names the length"""
    net = _Net(engine, lambda: _Fan(8193, [(1, 1, 1)]), 0)
    with pytest.raises(_ffi.DfqError, match='expectation of 8193 channels') as exc:
        dfq.build_bc_plan(net.graph, net.bottoms, TARG)
    assert exc.value.code == DFQ_ERR_ARG


# ---- 3 / 4. bodies, protocols, sources -----------------------------------------------------------------------------------
@pytest.mark.parametrize('case', list(BODIES))
def test_bodies_and_protocols(engine, monkeypatch, case):
    """One shape per lane width, the first row past every slot boundary, the grouped and depthwise layers, source lengths around
    the strides of merge_source, a chain of three, adds and cats (seven parts: the source table) under both bodies, the
    per-channel body, every hand-over protocol, the one-launch form, without folding and in safe mode: every variant meets the
    bound, every plan repeats itself on its second run (other parity, next epoch), all per-tensor variants agree bit for bit,
    and the first network of a batch of three gets what its own plan gives it."""
    nets = [_Net(engine, BODIES[case], seed) for seed in (0, 1, 2)]
    base = None
    for variant in VARIANTS:
        (res,), info = _run_plan(monkeypatch, nets, variant)
        for i, (after, corrs) in enumerate(res):
            if variant == 'default' or variant not in PER_TENSOR or i > 0:       # (the other per-tensor results ARE the default's, below)
                _verify(nets[i], nets[i].start, after, corrs, '{} {} net {}'.format(case, variant, i), kind=_kind(variant))
        if variant == 'default':
            base = res[0]
        elif variant in PER_TENSOR:
            _same(base, res[0], '{}: {} against default'.format(case, variant))
        if variant == 'no-fold':
            assert info['folded'] == 0
        if variant in ('counters',):
            assert not info['tagged']
        if variant == 'one-launch':                              # (rows that stream from memory keep the pair of launches)
            assert info['one_launch'] == all(e.shape[1] <= 1536 for e in nets[0].eps(0).values()), (case, info)


# ---- 5. the ReLU moment at the edges -----------------------------------------------------------------------------------------
def test_oracle_relu_mean_error_is_what_the_header_says():
    """CPU only: orc.relu_mean against the float64 clipped-normal mean over the input set; its NaN channels are the planted ones"""
    w, b, _ = _INPUTS
    with np.errstate(all='ignore'):
        m = orc.relu_mean(w, b)
        em = _exact_moments(1, w, b)[0]
        d = np.maximum(np.abs(m.astype(np.float64) - em) - 4 * ETA, 0.0) / (U * (np.abs(b.astype(np.float64)) + w))
    assert np.flatnonzero(np.isnan(m)).tolist() == _planted_nan()
    keep = ~np.isnan(m)
    assert np.isfinite(m[keep]).all() and not np.isnan(d[keep]).any()
    worst = float(d[keep].max())
    print('orc.relu_mean against float64: {:.3f} u (|b| + w)'.format(worst))
    assert worst <= ORACLE_KM and 2 * worst <= KM and worst >= 0.5 * ORACLE_KM, worst


def _planted_nan():
    w, b, _ = _INPUTS
    return np.flatnonzero((w == 0) & (b == 0)).tolist()              # (0, 0) and (0, -0.0)


def _moment_tweak(site):
    w, b, _ = _INPUTS

    def tweak(net, state):
        m = net.model
        if site == 'cache':
            k = net.key_of(m.bn0)
        else:
            k = net.key_of(m.bn1)
            state[net.key_of(m.bn0)]['fb'][:] = 0.0                 # E = 0 exactly: conv1's correction is +0.0 and BN1 keeps its beta~ bit for bit
        state[k]['fw'], state[k]['fb'] = w.copy(), b.copy()
    return tweak


@pytest.mark.parametrize('site,variant', [('cache', 'default'), ('cache', 'one-launch'), ('cache', 'per-position'), ('cache', 'batch-3'),
                                          ('tail', 'default'), ('tail', 'no-fold'), ('tail', 'general-body'), ('tail', 'counters'),
                                          ('tail', 'batch-3')])
def test_relu_moment_edges(engine, monkeypatch, site, variant):
    """relu_mean where it is evaluated -- bc_cache_init_block for a BN nobody rewrites ('cache'), the step's tail and the folded
    tail for a rewritten one ('tail') -- over the input set of test_act_adversarial.py, observed through BN - ReLU - depthwise:
    corr[o] = fl32(eps[o] E[o]) with eps known bit for bit.  |corr - eps E64| <= |eps| Km u (|b| + w) + u |eps E64| + 4 eta; the NaN
    outputs are exactly the planted channels (0, +-0)."""
    w, b, _ = _INPUTS
    C = len(w)
    factory = (lambda: _Direct(C, 3)) if site == 'cache' else (lambda: _Fan(C, [(C, 3, C)], relu1=True))
    nets = [_Net(engine, factory, seed, _moment_tweak(site)) for seed in ((0, 1, 2) if variant == 'batch-3' else (0,))]
    (res,), info = _run_plan(monkeypatch, nets, variant)
    net = nets[0]
    after, corrs = res[0]
    if site == 'tail':
        assert info['folded'] == (0 if variant == 'no-fold' else len(nets)), info
        k1 = net.key_of(net.model.bn1)
        assert_bitexact(corrs[0], np.zeros(C, dtype=F32), 'the correction in front of the BN under test is +0.0')
        assert_bitexact(after[k1]['fb'], b, 'beta~ of the BN under test')
    key = net.keys[-1]
    corr, eps = corrs[-1], net.eps(0)[key][:, 0].astype(np.float64)
    with np.errstate(all='ignore'):
        e64 = _exact_moments(1, w, b)[0]
        want = eps * e64
        lim = np.abs(eps) * KM * U * (np.abs(b.astype(np.float64)) + w) + U * np.abs(want) + 4 * ETA
        d = np.abs(corr.astype(np.float64) - want)
    assert np.flatnonzero(np.isnan(corr)).tolist() == _planted_nan() == np.flatnonzero(np.isnan(orc.relu_mean(w, b))).tolist()
    keep = ~np.isnan(corr)
    assert np.isfinite(corr[keep]).all() and (eps != 0).sum() > C - 8
    bad = np.flatnonzero(keep & ~(d <= lim))
    print('{} {}: worst {:.3f} of the bound'.format(site, variant, float((d[keep] / lim[keep]).max())))
    assert bad.size == 0, 'channel {} (w {!r}, b {!r}): corr {!r}, eps E64 {!r}: off by {:.3e} > {:.3e}'.format(
        bad[0], w[bad[0]], b[bad[0]], corr[bad[0]], want[bad[0]], d[bad[0]], lim[bad[0]])
    for i, (a, c) in enumerate(res):
        _verify(nets[i], nets[i].start, a, c, '{} {} net {}'.format(site, variant, i))      # (the tail identities; the bound again)


# ---- 6. non-finite expectations ------------------------------------------------------------------------------------------------
def _nonfinite_starts(net, n, groups, relu):
    """start states of `net` with channels of the polled source BN (bn1) set to +inf, -inf or NaN, first / middle / last of
    a group; infinities of both signs in one group; and +inf on the channel whose eps is exactly 0 in one row (the tensor's minimum
    quantises to itself)"""
    k1 = net.key_of(net.model.bn1)
    head = net.keys[-1]
    starts, names = [], []
    g = groups - 1                                                   # the last group (the only one when groups == 1)
    for value in (np.inf, -np.inf, np.nan):
        for pos, i in (('first', 0), ('middle', n // 2), ('last', n - 1)):
            st = _copy(net.start)
            st[k1]['fb'][g * n + i] = value
            starts.append(st)
            names.append('{} {}'.format(value, pos))
    st = _copy(net.start)
    st[k1]['fb'][g * n + 1], st[k1]['fb'][g * n + n - 2] = np.inf, -np.inf
    starts.append(st)
    names.append('both signs')
    if not relu:
        eps = net.eps(0)[head]
        zero = np.argwhere(eps == 0)
        assert len(zero) > 0, 'no row sum of eps is exactly zero'
        o, i = zero[0]
        st = _copy(net.start)
        st[k1]['fb'][(o // (eps.shape[0] // groups)) * n + i] = np.inf
        starts.append(st)
        names.append('inf on eps == 0 (row {})'.format(o))
    return starts, names


@pytest.mark.parametrize('relu', [False, True])
@pytest.mark.parametrize('n,groups', [(40, 1), (64, 1), (100, 1), (1600, 1), (40, 2), (64, 2), (100, 2), (1600, 2)])
def test_nonfinite_expectation(engine, monkeypatch, n, groups, relu):
    """One channel of a polled source at +inf, -inf or NaN (through a ReLU: +inf, NaN, NaN), in every body and protocol: the rows of
    its group follow the float64 rule of the header, the rows of other groups are finite and within the bound.  The default
    single-network plan left NaN in every row of the layer before the one-group body took the factor of an unowned slot from
    the zero word."""
    O = 5 if groups == 1 else 6
    nets = [_Net(engine, lambda: _Fan(n * groups, [(O, 1, groups)], relu1=relu), seed) for seed in (0, 1, 2)]
    starts, names = _nonfinite_starts(nets[0], n, groups, relu)
    base = None
    for variant in VARIANTS:
        use, use_names = starts, names
        if engine.kind == 'emu' and _kind(variant) and n * groups > 200:
            # the emulation spends seconds per run in the per-row range kernel of the 1600- and 3200-row layer in FRONT of the layer under
            # test (a wave of fibers per row): the per-channel body sees one start per value there, the device sees all
            pick = [0, 4, 8, 9]
            use, use_names = [starts[i] for i in pick], [names[i] for i in pick]
        results, _ = _run_plan(monkeypatch, nets, variant, starts=use, repeat=1)
        for start, name, res in zip(use, use_names, results):
            after, corrs = res[0]
            if variant == 'default' or variant not in PER_TENSOR:               # (the other per-tensor results ARE the default's, below)
                _verify(nets[0], start, after, corrs, 'I={} g={} relu={} {}: {}'.format(n, groups, relu, variant, name), kind=_kind(variant))
            c = corrs[-1]
            if groups == 2 and 'eps == 0' not in name:
                assert np.isfinite(c[:O // 2]).all(), '{} {}: a row of the other group is not finite'.format(variant, name)
        if variant == 'default':
            base = results
        elif variant in PER_TENSOR:
            for name, r0, r1 in zip(names, base, results):
                _same(r0[0], r1[0], '{} against default, {}'.format(variant, name))
