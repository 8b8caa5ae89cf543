"""Lazy sweeps of the deferred (one-way-scaled) layers of a batched streaming plan (dfq_le.hip, "Lazy sweeps").

A lazy sweep reads none of those layers' elements: the convergence launch decides "go on" from a lower bound of the sweep's
|dW| sum, and the missing terms are formed later, from the stored elements and the remembered factors, by the sweep that
stores them, by a sweep whose verdict needs them, or where an enqueue call ends.  None of this may be visible: weights, [O]
vectors, cumulative scales and the loop state stay those of the reference loop, bit for bit, after every call."""
import copy

import pytest

from oracle import dfq_oracle as orc
from oracle import graphspec
from dfq_amd import dfq, synthetic
from dfq_amd.utils import layer_transform as lt
from dfq_amd.utils import relation as rel

from common import TARG, assert_bitexact, npy, snapshot

CASES = [('tiny_mobile', 0), ('tiny_mobile', 1), ('tiny_cat', 3), ('tiny_tail', 1)]


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


def _env(monkeypatch, lazy, margin=None, cf=True):
    for k in ('DFQ_LE_RESIDENT', 'DFQ_LE_PERSIST', 'DFQ_LE_DEFER', 'DFQ_LE_CF', 'DFQ_LE_CF_GROUP', 'DFQ_LE_CF_BG',
              'DFQ_LE_LAZY_DW', 'DFQ_LE_LAZY_MARGIN'):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv('DFQ_LE_RESIDENT', '0')
    if not cf:
        monkeypatch.setenv('DFQ_LE_CF', '0')
    if not lazy:
        monkeypatch.setenv('DFQ_LE_LAZY_DW', '0')
    if margin is not None:
        monkeypatch.setenv('DFQ_LE_LAZY_MARGIN', margin)


def _batch(engine):
    items, specs = [], []
    for name, seed in CASES:
        model, graph, bottoms = synthetic.build(name, seed=seed)
        model.to(engine.device)
        spec = graphspec.from_torch(graph, bottoms, TARG)
        lt.merge_batchnorm(model, graph, bottoms, TARG)
        orc.merge_batchnorm(spec)
        items.append((graph, rel.create_relation(graph, bottoms, TARG)))
        specs.append(spec)
    return items, specs


def _check_oracle(items, specs, results, total=None, **kw):
    for (graph, rels), spec0, res in zip(items, specs, results):
        spec = copy.deepcopy(spec0)
        n_o, S_o = orc.cross_layer_equalization(spec, orc.create_relation(spec), max_sweeps=total, **kw)
        assert res['sweeps'] == n_o, (total, res)
        osnap, esnap = _spec_snapshot(spec), snapshot(graph)
        for k in osnap:
            assert_bitexact(esnap[k], osnap[k], '{} after {} sweeps'.format(k, total))
        for r, s in zip(rels, S_o):
            assert_bitexact(npy(r.get_scale_vec()), s, 'cumulative S after {} sweeps'.format(total))


def _state_run(engine, monkeypatch, lazy, calls=None, margin=None, cf=True, **cfg):
    """Loop states after every call (and the plan's lazy statistics at the end) of a fresh batch; the batch is checked against
    the oracle after every call."""
    _env(monkeypatch, lazy, margin, cf)
    items, specs = _batch(engine)
    plan = dfq.build_le_plan_batch(items, TARG)
    assert plan.defer_depth > 1 and plan.lazy == lazy
    states = []
    if calls is None:
        plan.run(**cfg)
        results, _ = plan.query_all()
        plan.stage.writeback()
        _check_oracle(items, specs, results, None if 'max_sweeps' not in cfg else cfg['max_sweeps'],
                      **{k: v for k, v in cfg.items() if k in ('converge_thres', 'converge_count')})
        states.append(results)
    else:
        plan.enqueue(0, restart=True, **cfg)
        total = 0
        for n in calls:
            plan.enqueue(n, restart=False, **cfg)
            total += n
            results, _ = plan.query_all()
            plan.stage.writeback()
            _check_oracle(items, specs, results, total, **{k: v for k, v in cfg.items() if k in ('converge_thres', 'converge_count')})
            states.append(results)
    stats = plan.lazy_stats()
    plan.close()
    return states, stats


@pytest.mark.parametrize('cf', [True, False])
def test_lazy_sweeps_match_eager_and_oracle(engine, monkeypatch, cf):
    """Lazy (the default) against DFQ_LE_LAZY_DW=0 and the oracle: weights, biases, BN fakes, S, and the loop state
    (sweeps, diff, count, last_diff_tmp) -- sweep count included."""
    lazy, st_l = _state_run(engine, monkeypatch, True, cf=cf)
    eager, st_e = _state_run(engine, monkeypatch, False, cf=cf)
    assert lazy == eager
    assert st_l['lazy_sweeps'] > 0 and st_e['lazy_sweeps'] == 0


def test_lazy_sweeps_cut_into_calls(engine, monkeypatch):
    """The loop cut into enqueue calls of 1, 1, 1, 2, 3, 5, ... sweeps: every call ends with the lazy sweeps resolved."""
    calls = (1, 1, 1, 2, 3, 5, 1, 2, 1000)
    lazy, st = _state_run(engine, monkeypatch, True, calls=calls)
    eager, _ = _state_run(engine, monkeypatch, False, calls=calls)
    assert lazy == eager
    assert st['lazy_sweeps'] > 0


def test_uncertain_verdicts_are_exact(engine, monkeypatch):
    """DFQ_LE_LAZY_MARGIN=0: no prediction, so the loop meets its threshold in a lazy sweep and the uncertain-verdict path reads
    the deferred layers; the results are those of the eager loop."""
    lazy, st = _state_run(engine, monkeypatch, True, margin='0')
    eager, _ = _state_run(engine, monkeypatch, False)
    assert lazy == eager
    assert st['uncertain'] > 0


def test_count_bound_and_a_count_end(engine, monkeypatch):
    """A converge_count small enough that the count bound decides the modes, and a loop that ends by `count` (threshold below
    zero: only count or max_sweeps end it)."""
    cfg = dict(converge_thres=-1.0, converge_count=3, max_sweeps=200)
    lazy, st = _state_run(engine, monkeypatch, True, **cfg)
    eager, _ = _state_run(engine, monkeypatch, False, **cfg)
    assert lazy == eager
    assert any(r['sweeps'] < 200 for r in lazy[0]), lazy     # some network ended by count
    assert st['lazy_sweeps'] > 0


@pytest.mark.parametrize('max_sweeps', [6, 10])
def test_max_sweeps_inside_a_window(engine, monkeypatch, max_sweeps):
    """A max_sweeps end on a lazy sweep (inside a window of deferred stores)."""
    lazy, _ = _state_run(engine, monkeypatch, True, max_sweeps=max_sweeps)
    eager, _ = _state_run(engine, monkeypatch, False, max_sweeps=max_sweeps)
    assert lazy == eager
    assert all(r['sweeps'] == max_sweeps for r in lazy[0])


def test_lazy_byte_accounting(engine, monkeypatch):
    """sweep_bytes: the deferred elements of a lazy plan move 8 B per defer_depth sweeps, of an eager one 4 (d + 1) / d B per sweep."""
    plans = {}
    for lazy in (True, False):
        _env(monkeypatch, lazy)
        items, _ = _batch(engine)
        plan = dfq.build_le_plan_batch(items, TARG)
        d, n = plan.defer_depth, plan.deferred_elements
        assert d > 1 and n > 0 and plan.lazy == lazy
        rest = 8 * plan.rw_elements + 4 * plan.ro_elements + 8.0 * plan.free_running_elements / plan.free_running_group - 8 * n
        per = 8.0 / d if lazy else 4.0 * (d + 1) / d
        assert plan.sweep_bytes == pytest.approx(rest + per * n)
        plans[lazy] = plan.sweep_bytes
        plan.close()
    assert plans[True] < plans[False]
