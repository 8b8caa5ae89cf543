"""Store period of the deferred (one-way-scaled) layers of a lazy streaming plan (dfq_le.hip, "Deferred stores"): the layers are
read at the latest every defer_depth-th sweep (the verdict window, 4) but stored only every store_depth-th one
(DFQ_LE_STORE_DEPTH = 4, 8 or 16; without the switch 8 for plans with 8 Mi deferred elements or more); a reading sweep replays
up to store_depth - 1 remembered factors, the last few of them with their |dW| terms.  None of it may be visible: after every enqueue call the weights, biases, BN fakes and cumulative S are those
of the oracle stopped at that sweep, and the loop state (sweeps, diff, count, last_diff_tmp) is that of the eager engine
(DFQ_LE_LAZY_DW=0, which stores every defer_depth-th sweep) -- bit for bit, on one non-uniform batch of the tiny networks."""
import pytest
import torch

from dfq_amd import dfq, synthetic
from dfq_amd.utils import layer_transform as lt
from dfq_amd.utils import relation as rel
from oracle import dfq_oracle as orc
from oracle import graphspec

import test_verdict_launch as tvl
from common import TARG, assert_bitexact, snapshot
from test_lazy_oneway import _check_oracle, _env

CASES = (('tiny_mobile', 0), ('tiny_mobile', 1), ('tiny_cat', 3), ('tiny_tail', 1), ('tiny_res', 0))
DEFER = 4
FOREVER = dict(converge_thres=-1.0, converge_count=10 ** 9)        # no verdict ends the loop


def _build(engine, monkeypatch, lazy, store, margin=None, cases=CASES):
    _env(monkeypatch, lazy, margin)
    if store is None:
        monkeypatch.delenv('DFQ_LE_STORE_DEPTH', raising=False)
    else:
        monkeypatch.setenv('DFQ_LE_STORE_DEPTH', str(store))
    items, specs = [], []
    for name, seed in cases:
        model, graph, bottoms = synthetic.build(name, seed=seed)
        model.to(engine.device)
        spec = graphspec.from_torch(graph, bottoms, TARG)
        lt.merge_batchnorm(model, graph, bottoms, TARG)
        orc.merge_batchnorm(spec)
        items.append((graph, rel.create_relation(graph, bottoms, TARG)))
        specs.append(spec)
    plan = dfq.build_le_plan_batch(items, TARG)
    assert plan.defer_depth == DEFER and plan.lazy == lazy
    if store is not None:
        assert plan.store_depth == (store if lazy else DEFER)
    return items, specs, plan


def _calls(store):
    """1, 1, 1, 2, 3, 5, 1, 7, 2, 9 sweeps and then the shortest calls that end on the residues of the sweep count mod `store`
    still missing; at least 2 store + 3 sweeps in all."""
    calls, total, seen = [], 0, set()
    for n in (1, 1, 1, 2, 3, 5, 1, 7, 2, 9):
        calls.append(n)
        total += n
        seen.add(total % store)
    while len(seen) < store or total < 2 * store + 3:
        missing = [r for r in range(store) if r not in seen] or [(total + 1) % store]
        n = min((r - total) % store or store for r in missing)
        calls.append(n)
        total += n
        seen.add(total % store)
    return calls


_EAGER = {}


def _eager_states(engine, monkeypatch, n_sweeps):
    """Loop state of every network after 1, 2, ... sweeps of the eager engine, a sweep per call (computed once per backend)."""
    have = _EAGER.get(engine.kind, [])
    if len(have) < n_sweeps:
        _, _, plan = _build(engine, monkeypatch, False, None)
        plan.enqueue(0, restart=True, **FOREVER)
        have = []
        for _ in range(max(n_sweeps, 48)):
            plan.enqueue(1, restart=False, **FOREVER)
            have.append(plan.query_all()[0])
        plan.close()
        _EAGER[engine.kind] = have
    return have


def _deferred_sides(plan):
    """(elements of deferred first layers, of deferred second layers) from the plan's workgroup table: a row tile of 16-byte
    vectors or floats whose layer nobody column-scales (it publishes no column statistics) is a deferred W1 (rows by s), a
    column tile of those kinds that stores (its layer is nobody's first layer) a deferred W2 (columns by 1/s)."""
    w1 = w2 = 0
    for launch in range(plan.levels):
        for b in range(plan.level_info(launch)['workgroups']):
            info = plan.block_info(launch, b)
            if info['kind'] in (0, 1) and not info['publishes']:
                w1 += info['rw_elements']
            elif info['kind'] in (3, 4) and info['rw_elements'] > 0 and not info['publishes']:
                w2 += info['rw_elements']
    return w1, w2


@pytest.mark.parametrize('lazy', [True, False])
@pytest.mark.parametrize('store', [4, 8, 16])
def test_stores_are_invisible(engine, monkeypatch, store, lazy):
    """The loop, convergence disabled, cut into calls that end on every residue of the sweep count mod store_depth: every flush
    length 0 .. store_depth - 1 is exercised, the oracle and the eager loop state are checked after every call."""
    calls = _calls(store)
    ends, total = set(), 0
    for n in calls:
        total += n
        ends.add(total % store)
    assert ends == set(range(store)) and total >= 2 * store + 3
    ref = _eager_states(engine, monkeypatch, total)
    items, specs, plan = _build(engine, monkeypatch, lazy, store)
    plan.enqueue(0, restart=True, **FOREVER)
    total = 0
    for n in calls:
        plan.enqueue(n, restart=False, **FOREVER)
        total += n
        results, done = plan.query_all()
        plan.stage.writeback()
        _check_oracle(items, specs, results, total, **FOREVER)
        assert results == ref[total - 1], (store, lazy, total)
        assert not done
    stats = plan.lazy_stats()
    plan.close()
    assert (stats['lazy_sweeps'] > 0) == lazy


@pytest.mark.parametrize('store', [8, 16])
def test_stop_inside_a_store_window_through_an_undecided_verdict(engine, monkeypatch, store):
    """A threshold from the eager run's per-sweep sums that ends a network's loop at a sweep k with k % store_depth >= defer_depth
    -- remembered factors older than the window are pending -- through an undecided verdict (DFQ_LE_LAZY_MARGIN=0; looked up in
    a probe run, sweep by sweep): replay_oneway takes the stored elements through the old factors, then through the window's."""
    monkeypatch.setenv('DFQ_LE_STORE_DEPTH', str(store))
    sums = tvl._eager_sums(engine, monkeypatch)
    found = None
    for k, n, t in tvl._thresholds(sums):
        if k % store < DEFER or k % DEFER == DEFER - 1:
            continue
        rises, last = tvl._probe(engine, monkeypatch, t)
        if tvl._undecided_at(rises, last, n, k):
            found = (k, n, t)
            break
    assert found, 'no threshold puts an undecided verdict at such a sweep: {}'.format(sums)
    k, n, t = found
    _, _, plan = tvl._build(engine, monkeypatch, True)
    assert plan.store_depth == store and plan.defer_depth == DEFER
    plan.close()
    lazy, st = tvl._lazy_vs_eager(engine, monkeypatch, converge_thres=t)
    assert st['uncertain'] > 0 and lazy[0][n]['sweeps'] == k + 1 and (k % store) >= DEFER


def _put_back(items, start):
    """fresh copies of the networks, in place: the values the plan was made over, cumulative scales of 1"""
    with torch.no_grad():
        for (graph, rels), snap in zip(items, start):
            for i, (k, mod) in enumerate(graph.items()):
                for name, attr in (('w', 'weight'), ('b', 'bias'), ('fw', 'fake_weight'), ('fb', 'fake_bias')):
                    key = 'L{}.{}'.format(i, name)
                    if key in snap:
                        getattr(mod, attr).copy_(torch.from_numpy(snap[key]).to(getattr(mod, attr).device))
            for r in rels:
                r.S.fill_(1.0)


@pytest.mark.parametrize('store', [8, 16])
def test_restart_with_factors_pending(engine, monkeypatch, store):
    """A run that stops between two stores (max_sweeps), a restart over fresh copies of the networks, the same run again, and a
    longer one after another restart: each gives the bits of a first run."""
    items, specs, plan = _build(engine, monkeypatch, True, store)
    start = [snapshot(graph) for graph, _ in items]
    n1, n2 = store + DEFER + 1, 2 * store + DEFER + 2
    assert n1 % store >= DEFER and n2 % store >= DEFER
    firsts = {}
    for rnd, n in enumerate((n1, n1, n2)):
        if rnd:
            _put_back(items, start)
        plan.enqueue(0, restart=True, max_sweeps=n, **FOREVER)
        plan.enqueue(n + 3, restart=False, max_sweeps=n, **FOREVER)
        results, done = plan.query_all()
        plan.stage.writeback()
        assert done and all(r['sweeps'] == n for r in results)
        _check_oracle(items, specs, results, n, **FOREVER)
        got = (results, [snapshot(graph) for graph, _ in items])
        if n in firsts:
            assert got[0] == firsts[n][0]
            for a, b in zip(got[1], firsts[n][1]):
                for k in a:
                    assert_bitexact(a[k], b[k], 'second run of {} sweeps: {}'.format(n, k))
        firsts[n] = got
    plan.close()


def test_both_sides_are_deferred(engine, monkeypatch):
    """The batch holds a deferred first layer (rows by s) and a deferred second layer (columns by 1/s), and together they are the
    plan's deferred elements."""
    _, _, plan = _build(engine, monkeypatch, True, 16)
    w1, w2 = _deferred_sides(plan)
    assert w1 > 0 and w2 > 0 and w1 + w2 == plan.deferred_elements, (w1, w2, plan.deferred_elements)
    plan.close()


@pytest.mark.parametrize('store', [8, 16])
def test_safe_mode_runs_the_same_loop(engine, monkeypatch, store):
    """LEPlan.run() of a plan in safe mode (one launch per dependency level, every sweep reads) with store_depth > defer_depth:
    the bits of the default run."""
    out = {}
    for safe in (False, True):
        items, specs, plan = _build(engine, monkeypatch, True, store)
        if safe:
            plan.set_safe_mode()
            assert plan.store_depth == store and not plan.lazy
        plan.run()
        results, done = plan.query_all()
        plan.stage.writeback()
        assert done
        _check_oracle(items, specs, results, None)
        out[safe] = (results, [snapshot(graph) for graph, _ in items])
        plan.close()
    assert out[True][0] == out[False][0]
    for a, b in zip(out[True][1], out[False][1]):
        for k in a:
            assert_bitexact(a[k], b[k], k)


def test_getters(engine, monkeypatch):
    """store_depth follows DFQ_LE_STORE_DEPTH (lazy plans only), defer_depth stays 4, and sweep_bytes prices a lazy plan's deferred
    elements at 4 B per defer_depth sweeps read + 4 B per store_depth sweeps written."""
    seen = {}
    for store in (4, 8, 16):
        for lazy in (True, False):
            _, _, plan = _build(engine, monkeypatch, lazy, store)
            d, s, n = plan.defer_depth, plan.store_depth, plan.deferred_elements
            assert d == DEFER and s == (store if lazy else DEFER) and n > 0
            rest = 8 * plan.rw_elements + 4 * plan.ro_elements + 8.0 * plan.free_running_elements / plan.free_running_group - 8 * n
            per = 4.0 / d + 4.0 / s if lazy else 4.0 * (d + 1) / d
            assert plan.sweep_bytes == pytest.approx(rest + per * n)
            seen[(store, lazy)] = plan.sweep_bytes
            plan.close()
    assert seen[(16, True)] < seen[(8, True)] < seen[(4, True)] < seen[(4, False)] == seen[(16, False)]
    # no switch: these networks' deferred layers are far smaller than the L2s, where stores further apart gain nothing
    _, _, plan = _build(engine, monkeypatch, True, None)
    assert plan.store_depth == plan.defer_depth == DEFER and plan.deferred_elements < 8 << 20
    plan.close()


@pytest.mark.gpu
def test_default_store_depth_follows_the_deferred_size(monkeypatch):
    """Without DFQ_LE_STORE_DEPTH a lazy plan stores every 8th sweep where its deferred layers hold 8 Mi elements or more (a
    batch of 8 MobileNetV2: 8 x 1.28 M classifier weights and the first convolutions) and every defer_depth-th below that (a
    batch of 4).  Plans only: nothing runs."""
    _env(monkeypatch, True)
    monkeypatch.delenv('DFQ_LE_STORE_DEPTH', raising=False)
    dev = torch.device('cuda', 0)
    items = []
    for s in range(8):
        model, graph, bottoms = synthetic.build('mobilenet_v2', seed=s % 2)
        model.to(dev)
        lt.merge_batchnorm(model, graph, bottoms, TARG)
        items.append((graph, rel.create_relation(graph, bottoms, TARG)))
    for n, want in ((8, 8), (4, DEFER)):
        plan = dfq.build_le_plan_batch(items[:n], TARG)
        assert plan.lazy and plan.defer_depth == DEFER
        assert (plan.deferred_elements >= 8 << 20) == (want > DEFER)
        assert plan.store_depth == want, (n, plan.deferred_elements)
        plan.close()
