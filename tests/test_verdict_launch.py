"""One verdict launch per sweep (dfq_le.hip, le_control_kernel): a lazy sweep whose bound leaves the verdict open is decided by the
network's own workgroup of the convergence launch -- next to the clearing and the solver workgroups -- and le_resolve_kernel only
runs where an enqueue call ends.  None of it may be visible: lazy plans are compared with DFQ_LE_LAZY_DW=0 and with the oracle,
bit for bit -- weights, biases, BN fakes, cumulative S and the loop state -- on one non-uniform batch of the tiny networks.

Where an undecided verdict lands is steered with a converge_thres taken from the per-sweep |dW| sums of an eager run, and then
looked up, not assumed: a probe run of one sweep per call reads lazy_stats()['uncertain'] after every sweep, so the sweeps in
which it rises are known.  (A probe has the same undecided verdicts as the run in one call while `count` stays 0, which holds
for these inputs: two sweeps never have sums within 1e-9 of each other before the threshold is met.)"""
import os
import re
import subprocess

import pytest

from dfq_amd import dfq, synthetic
from dfq_amd.utils import layer_transform as lt
from dfq_amd.utils import relation as rel
from oracle import dfq_oracle as orc
from oracle import graphspec

from common import TARG
from test_lazy_oneway import _check_oracle, _env

CASES = (('tiny_mobile', 0), ('tiny_mobile', 1), ('tiny_cat', 3), ('tiny_tail', 1))
CASES_RES = CASES + (('tiny_res', 0),)
PROBE_SWEEPS = 24
DEFER = 4


def _build(engine, monkeypatch, lazy, cases=CASES, group=None, margin='0'):
    _env(monkeypatch, lazy, margin)
    if group is not None:
        monkeypatch.setenv('DFQ_LE_CF_GROUP', str(group))
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
    return items, specs, plan


def _run(engine, monkeypatch, lazy, cases=CASES, group=None, calls=None, stage=None, **cfg):
    """Loop states after every call of a fresh batch (checked against the oracle after every call) and the plan's lazy statistics."""
    items, specs, plan = _build(engine, monkeypatch, lazy, cases, group)
    if stage is not None:
        assert plan.set_control_stage(stage) == stage
    okw = {k: v for k, v in cfg.items() if k in ('converge_thres', 'converge_count')}
    states = []
    if calls is None:
        plan.run(**cfg)
        results, _ = plan.query_all()
        plan.stage.writeback()
        _check_oracle(items, specs, results, cfg.get('max_sweeps'), **okw)
        states.append(results)
    else:
        plan.enqueue(0, restart=True, **cfg)
        total = 0
        for n in calls:
            plan.enqueue(n, restart=False, **cfg)
            total += n
            results, _ = plan.query_all()
            plan.stage.writeback()
            _check_oracle(items, specs, results, total, **okw)
            states.append(results)
    stats = plan.lazy_stats()
    plan.close()
    return states, stats


_SUMS = {}


def _eager_sums(engine, monkeypatch, cases=CASES):
    """diff_tmp of sweep k of network n of the eager loop, [k][n] (computed once per backend)."""
    key = (engine.kind, cases)
    if key not in _SUMS:
        _, _, plan = _build(engine, monkeypatch, False, cases)
        cfg = dict(converge_thres=-1.0, converge_count=10 ** 9)
        plan.enqueue(0, restart=True, **cfg)
        sums = []
        for _ in range(PROBE_SWEEPS):
            plan.enqueue(1, restart=False, **cfg)
            sums.append([r['last_diff_tmp'] for r in plan.query_all()[0]])
        plan.close()
        _SUMS[key] = sums
    return _SUMS[key]


def _probe(engine, monkeypatch, thres, cases=CASES, group=None):
    """Sweeps (0-based) in which a lazy plan's count of undecided verdicts rises, with the rise, and each network's last sweep."""
    _, _, plan = _build(engine, monkeypatch, True, cases, group)
    cfg = dict(converge_thres=thres)
    plan.enqueue(0, restart=True, **cfg)
    rises, seen = {}, 0
    for k in range(PROBE_SWEEPS):
        plan.enqueue(1, restart=False, **cfg)
        now = plan.lazy_stats()['uncertain']
        if now > seen:
            rises[k] = now - seen
            seen = now
        res, done = plan.query_all()
        if done:
            break
    plan.close()
    return rises, [r['sweeps'] for r in res]


def _stops(sums, n, thres):
    """The sweep after which network n's loop ends by the threshold (diff follows diff_tmp: no two sums within 1e-9)."""
    for k in range(len(sums)):
        if sums[k][n] <= thres:
            return k
    return None


def _thresholds(sums):
    """Candidate thresholds: halfway between a network's sums of two sweeps, where the later sum is the smaller."""
    out = []
    for k in range(1, len(sums)):
        for n in range(len(sums[0])):
            if sums[k][n] < sums[k - 1][n]:
                t = 0.5 * (sums[k][n] + sums[k - 1][n])
                if _stops(sums, n, t) == k:
                    out.append((k, n, t))
    return out


def _undecided_at(rises, last, n, k):
    """Was network n's verdict of sweep k undecided?  It ended at sweep k by the threshold (last[n] == k + 1), so it was -- its
    bound is at most its sum, at most the threshold -- unless it had latched before, through an undecided verdict of its own.
    That is excluded when nothing was undecided before sweep k; or when every network had exactly one undecided verdict (a
    network latches at its first) and the ones before sweep k are as many as the networks whose loops ended before it."""
    if k not in rises or last[n] != k + 1:
        return False
    before = sum(r for j, r in rises.items() if j < k)
    if before == 0:
        return True
    return sum(rises.values()) == len(last) and before == sum(1 for s in last if s <= k)


def _lazy_vs_eager(engine, monkeypatch, **kw):
    lazy, st = _run(engine, monkeypatch, True, **kw)
    eager, _ = _run(engine, monkeypatch, False, **kw)
    assert lazy == eager
    return lazy, st


@pytest.mark.parametrize('group', [2, 8])
def test_undecided_verdict_next_to_the_solver_workgroups(engine, monkeypatch, group):
    """An undecided verdict in a convergence launch that also carries the solver workgroups (the last sweep of a group).

    With stores deferred over 4 sweeps, sweep k is lazy only for k % 4 != 3, and the last sweep of a group of 4 or 8 has
    k % 4 == 3: it always stores, so no threshold puts an undecided verdict there.  Groups of 2: the threshold is chosen so
    that a network stops at a sweep with k % 4 == 1, the last of its group, undecided -- looked up in a probe.  Groups of 8:
    as close as the inputs allow, an undecided verdict at k % 8 == 6; the launch of the next sweep, the group's last, then
    carries the solver workgroups next to the verdict of the latched network (a max_sweeps cut ends the run right there)."""
    sums = _eager_sums(engine, monkeypatch)
    want = (lambda k: k % 4 == 1) if group == 2 else (lambda k: k % 8 == 6)
    found = None
    for k, n, t in _thresholds(sums):
        if not want(k):
            continue
        rises, last = _probe(engine, monkeypatch, t, group=group)
        if _undecided_at(rises, last, n, k):
            found = (k, n, t)
            break
    assert found, 'no threshold puts an undecided verdict at such a sweep: {}'.format(sums)
    k, n, t = found
    lazy, st = _lazy_vs_eager(engine, monkeypatch, group=group, converge_thres=t)
    assert st['uncertain'] > 0 and lazy[0][n]['sweeps'] == k + 1
    if group == 2:
        assert (k + 1) % group == 0
    else:
        lazy, st = _lazy_vs_eager(engine, monkeypatch, group=group, converge_thres=t, max_sweeps=k + 2)
        assert st['uncertain'] > 0 and (k + 2) % group == 0 and all(r['sweeps'] <= k + 2 for r in lazy[0])


def test_go_on_after_an_undecided_verdict(engine, monkeypatch):
    """A threshold just under a network's sum of a lazy sweep: the bound (the sum without the deferred layers) is below it, the
    exact sum above -- the verdict is "go on", the network latches, keeps sweeping and stops where the eager loop stops."""
    sums = _eager_sums(engine, monkeypatch)
    found = None
    for k in range(1, PROBE_SWEEPS - 4):
        if k % DEFER == DEFER - 1:
            continue
        for n in range(len(CASES)):
            t = sums[k][n] * (1.0 - 1e-4)
            if t <= 0.0 or min(sums[j][n] for j in range(k + 1)) <= t:
                continue
            rises, last = _probe(engine, monkeypatch, t)
            # undecided at sweep k, and nobody's loop ended there: the exact answer was "go on"
            if k in rises and all(s != k + 1 for s in last) and last[n] > k + 1:
                found = (k, n, t)
                break
        if found:
            break
    assert found, 'no threshold gives an undecided verdict that goes on: {}'.format(sums)
    k, n, t = found
    lazy, st = _lazy_vs_eager(engine, monkeypatch, converge_thres=t)
    assert st['uncertain'] > 0
    assert lazy[0][n]['sweeps'] > k + 1


def test_undecided_in_different_sweeps_and_next_to_a_finished_network(engine, monkeypatch):
    """Two networks of the batch undecided in different sweeps; at the later one another network's loop is already over."""
    sums = _eager_sums(engine, monkeypatch)
    found = None
    for k, n, t in _thresholds(sums):
        rises, last = _probe(engine, monkeypatch, t)
        ks = sorted(rises)
        if len(ks) >= 2 and any(s <= ks[-1] for s in last):
            found = (t, ks, last)
            break
    assert found, 'no threshold gives undecided verdicts in two sweeps: {}'.format(sums)
    t, ks, last = found
    lazy, st = _lazy_vs_eager(engine, monkeypatch, converge_thres=t)
    assert st['uncertain'] >= 2
    assert [r['sweeps'] for r in lazy[0]] == last


def test_loop_cut_into_calls(engine, monkeypatch):
    """Calls of 1, 1, 1, 2, 3, 5, 1, 2 sweeps and the rest, no prediction: undecided verdicts are drawn inside the convergence
    launch, the lazy sweeps a call ends on are resolved by le_resolve_kernel; the oracle is checked after every call."""
    calls = (1, 1, 1, 2, 3, 5, 1, 2, 1000)
    lazy, st = _lazy_vs_eager(engine, monkeypatch, calls=calls)
    assert st['uncertain'] > 0 and st['lazy_sweeps'] > 0


@pytest.mark.parametrize('stage', [0, 8])
def test_partials_beyond_the_lds_stage(engine, monkeypatch, stage):
    """The stage of the convergence launch forced to `stage` partials (dfq_le_plan_set_ctl_stage): every network's partials
    exceed it and are read from memory.  The results are those of the plan-sized stage, and of the eager loop."""
    capped, st = _run(engine, monkeypatch, True, cases=CASES_RES, stage=stage)
    full, _ = _run(engine, monkeypatch, True, cases=CASES_RES)
    eager, _ = _run(engine, monkeypatch, False, cases=CASES_RES, stage=stage)
    assert capped == full == eager
    assert st['uncertain'] > 0


def test_control_kernel_metadata():
    """What two 16-wave workgroups of le_control_kernel per CU need (160 KB of LDS, 512 vector registers per SIMD): at most 64
    vector registers, nothing spilled, no scratch, and a static LDS part that leaves the plan-sized part room."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, 'dfq_amd', 'csrc')
    hipcc = '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    flags = ['-O3', '-std=c++17', '-fPIC', '-ffp-contract=off', '--offload-arch=gfx950', '--cuda-device-only', '-x', 'hip', '-S',
             '-Wno-unused-command-line-argument', '-o', '-']
    res = subprocess.run([hipcc] + flags + [os.path.join(csrc, 'dfq_le.hip')], capture_output=True, text=True, cwd=csrc)
    assert res.returncode == 0, res.stderr[-2000:]
    meta = {}
    for m in re.finditer(r'- \.agpr_count:.*?\.wavefront_size:\s+\d+', res.stdout, flags=re.S):
        blk = m.group(0)

        def g(k):
            return re.search(r'\.%s:\s+(\S+)' % k, blk).group(1)
        meta[g('name')] = dict(vgpr=int(g('vgpr_count')), sgpr_spill=int(g('sgpr_spill_count')), vgpr_spill=int(g('vgpr_spill_count')),
                               scratch=int(g('private_segment_fixed_size')), lds=int(g('group_segment_fixed_size')))
    ctl = [v for n, v in meta.items() if 'le_control_kernel' in n]
    lev = [v for n, v in meta.items() if 'le_level_kernelILb0' in n]
    assert len(ctl) == 1 and len(lev) == 1
    assert ctl[0]['vgpr'] <= 64, ctl
    assert ctl[0]['sgpr_spill'] == 0 and ctl[0]['vgpr_spill'] == 0 and ctl[0]['scratch'] == 0, ctl
    assert ctl[0]['lds'] <= 16 * 1024, ctl
    assert lev[0]['vgpr'] <= 80 and lev[0]['sgpr_spill'] <= 100, lev
