"""bench.py's N > 1 path (one rank per GPU, barrier + MAX over ranks, rank 0 prints the line) on two CPU
ranks over gloo, with the kernels running on the CPU emulation (tests/emu/dryrun.py).  The driver launches
the real thing as `python -m torch.distributed.run --nproc-per-node N bench.py --gpus N ...` over RCCL."""
import json
import os
import socket
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def test_two_ranks_weak_scaling_line():
    port = _free_port()
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE='2', MASTER_ADDR='127.0.0.1',
                   MASTER_PORT=str(port), PYTHONPATH=ROOT)
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, 'tests', 'emu', 'dryrun.py')], env=env, cwd=ROOT,
                                      stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    outs = [p.communicate(timeout=600) for p in procs]
    for p, (out, err) in zip(procs, outs):
        assert p.returncode == 0, err[-2000:]
    lines = [l for l in outs[0][0].splitlines() if l.startswith('{"metric"')]
    assert len(lines) == 1 and not [l for l in outs[1][0].splitlines() if l.startswith('{"metric"')]
    d = json.loads(lines[0])
    assert d['n_gpus'] == 2 and d['scaling'] == 'weak' and d['config']['networks_per_step'] == 4
    assert d['value'] > 0 and d['vs_baseline'] is None and 'cpu_baseline' not in d     # CPU baseline: N=1 only
    # config 4 as north_star splits it: both ranks on the data path, one collective per pass, strong scaling
    assert [e['net'] for e in d['sharded']] == ['tiny_mobile', 'tiny_res']
    for sh in d['sharded']:
        assert sh['world'] == 2 and sh['ranks_owning_components'] == 2 and sh['collectives_per_pass'] == 1
        assert sh['scaling'] == 'strong' and sh['sweeps_pinned'] and sh['value'] > 0 and sh['exchange_bytes_per_rank'] > 0
        # who holds what: greedy split of the components by paired elements
        assert len(sh['paired_elements_per_rank']) == 2 and all(n > 0 for n in sh['paired_elements_per_rank'])
        assert sh['components'] >= 2
        # the reference's own stopping rule across ranks: one all_reduce per sweep + the final all_gather
        assert sh['data_dependent_ms'] > 0 and sh['data_dependent_sweeps'] >= 1
        assert sh['data_dependent_collectives_per_pass'] == -(-sh['data_dependent_sweeps'] // sh['data_dependent_chunk']) + 1   # one all_reduce per chunk of sweeps (sharded.py) + the all_gather


def test_bench_line_contract_single_rank():
    """The JSON line of bench.py (dry run on the emulator, tiny net): every field the measurement contract names."""
    env = dict(os.environ, PYTHONPATH=ROOT)
    for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE'):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'emu', 'dryrun.py')], env=env, cwd=ROOT,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith('{"metric"')]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for key in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling',
                'vs_baseline', 'dtype', 'data', 'config', 'roofline', 'cpu_baseline'):
        assert key in d, key
    assert d['unit'] == 'weights/s' and d['higher_is_better'] is True and d['scaling'] == 'weak' and d['vs_baseline'] is None
    assert d['dtype'] == 'f32' and d['data'] == 'synthetic' and d['n_gpus'] == 1
    assert 'workload' in d['config'] and 'model' not in d['config']
    r = d['roofline']
    for key in ('bound', 'achieved', 'peak', 'unit', 'frac', 'traffic'):
        assert key in r, key
    assert r['bound'] == 'hbm' and r['unit'] == 'GB/s' and r['peak'] == 8000.0 and abs(r['frac'] - r['achieved'] / r['peak']) < 1e-9
    c = d['cpu_baseline']
    for key in ('value', 'unit', 'cores', 'kind', 'sample'):
        assert key in c, key
    assert c['kind'] == 'port' and c['cores'] == 1 and c['unit'] == 'weights/s'
    assert abs(d['value'] - d['config']['networks_per_step'] * 5000 / (d['ms_per_step'] * 1e-3)) < 1e-6 * d['value']
    assert 'frac_survey_8d' not in r and 'eager_formulation_equivalent_GBps' in r     # not a fraction
    lat = d['latency']
    assert lat['single_network_pass_ms'] > 0 and 0 < lat['frac_of_hbm_peak'] and lat['sweeps'] == d['config']['le_sweeps'][0]
    others = d['config']['others']
    assert [o['net'] for o in others] == ['tiny_res', 'tiny_mobile'] and others[1]['sweeps_pinned'] and others[1]['sweeps'] == 3
    assert all(o['ms'] > 0 and o['roofline_frac'] > 0 for o in others)
    act = d['config']['activation_ranges']
    assert [k['bytes'] for k in act['kernels'][:3]] == [4 * act['elements'], 8 * act['elements'], 12 * act['elements']]
    assert [e['net'] for e in d['sharded']] == ['tiny_mobile', 'tiny_res']
    assert all(e['world'] == 1 and e['scaling'] == 'strong' and e['data_dependent_ms'] > 0 for e in d['sharded'])
    # one rank, same network: the data-dependent sharded loop stops where the plain entry point's loop stops
    assert d['sharded'][0]['data_dependent_sweeps'] == d['config']['le_sweeps'][0]
    # like-for-like figure, config 5 end to end, the PCIe-inclusive drop-in pass
    assert abs(d['value_single_network'] - lat['weights_per_s']) < 1e-6 * lat['weights_per_s']
    dr = d['config']['distill_range']
    assert dr['batches'] == 2 and dr['quant_measures'] > 0 and dr['ms_per_batch'] > 0
    assert dr['quant_measure_bytes_per_batch'] == 12 * dr['elements_per_batch'] and dr['elements_per_batch'] > 0
    assert d['pcie_inclusive_ms'] == d['pcie_inclusive']['le_plus_bc_ms'] > 0
    lz = d['lazy_scale']            # the opt-in formulation: its own value and its own roofline entry, never `value`
    assert lz['sweeps'] == d['config']['le_sweeps'] and lz['sweeps_given'] and d['value_lazy_scale'] == lz['value'] > 0
    assert abs(lz['roofline']['frac'] - lz['roofline']['achieved'] / lz['roofline']['peak']) < 1e-12
    assert 'reference' in c          # the committed reference-CPU record (null for nets it was not measured on)


FULL_ONLY = ('roofline', 'latency', 'cpu_baseline', 'sharded', 'lazy_scale', 'value_lazy_scale', 'value_single_network',
             'pcie_inclusive', 'pcie_inclusive_ms')


def test_bench_plain_line_is_the_headline_alone():
    """Without --full (the default) bench.py sets up, warms up, times the steps and prints the line: the headline fields
    the measurement contract names, and none of what only --full measures."""
    env = dict(os.environ, PYTHONPATH=ROOT)
    for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE'):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'emu', 'dryrun.py'), '--no-full'], env=env, cwd=ROOT,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith('{"metric"')]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for key in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling',
                'vs_baseline', 'dtype', 'data', 'config'):
        assert key in d, key
    assert d['metric'] == 'conv weights calibrated/sec (LE+BC pass, tiny_mobile)' and d['unit'] == 'weights/s'
    assert d['higher_is_better'] is True and d['dtype'] == 'f32' and d['steps'] == 2 and d['warmup'] == 1
    assert abs(d['value'] - d['config']['networks_per_step'] * 5000 / (d['ms_per_step'] * 1e-3)) < 1e-6 * d['value']
    assert not [k for k in d if k in FULL_ONLY or k.endswith('_error')]
    assert not [k for k in ('others', 'activation_ranges', 'distill_range', 'one_unit_alone_ms', 'single_pass_latency_ms')
                if k in d['config']]
    assert 'plan_build_ms_per_unit_scattered_tensors' not in d['host_inclusive']


DUMP_FILES = {'le_sweeps', 'weights_net0', 'biases_net0', 'weights_sample', 'weights_sample_index', 'biases_sample',
              'biases_sample_index'}


def test_bench_dumps_what_its_last_timed_step_computed(tmp_path):
    """`--dump-outputs DIR` (dry run on the emulator, a batch of two tiny nets): two runs with the same arguments write the same
    arrays, float32 / float64 only, and what they hold is the calibrated batch -- weights bit-identical to the numpy oracle's
    LE + BC of the same seeds, biases within the BC tolerance."""
    import numpy as np
    import torch.nn as nn
    sys.path.insert(0, ROOT)
    from dfq_amd import synthetic
    from oracle import dfq_oracle as orc
    from oracle import graphspec

    env = dict(os.environ, PYTHONPATH=ROOT)
    for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE'):
        env.pop(k, None)
    legs_off = ['--cpu-seconds', '0', '--no-roofline', '--others', '', '--act-shape', '', '--sharded', '', '--distill', '',
                '--pcie', '', '--lazy-steps', '0', '--steps', '3']
    dirs = [str(tmp_path / d) for d in ('a', 'b')]
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, 'tests', 'emu', 'dryrun.py')] + legs_off + ['--dump-outputs', d],
                              env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for d in dirs]
    outs = [p.communicate(timeout=600) for p in procs]
    for p, (out, err) in zip(procs, outs):
        assert p.returncode == 0, err[-2000:]
    d = json.loads([l for l in outs[0][0].splitlines() if l.startswith('{"metric"')][0])
    assert d['steps'] == 3 and d['ms_per_step'] > 0

    dumps = []
    for path in dirs:
        assert {f[:-4] for f in os.listdir(path)} == DUMP_FILES
        arrays = {n: np.load(os.path.join(path, n + '.npy')) for n in DUMP_FILES}
        assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
        assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
        dumps.append(arrays)
    for n in DUMP_FILES:
        assert np.array_equal(dumps[0][n], dumps[1][n]), n
    got = dumps[0]
    assert got['le_sweeps'].tolist() == d['config']['le_sweeps']

    # the oracle on the same two networks (bench.prepare: seeds 0 and 1, BN folded, relations kept whole)
    targ = [nn.Conv2d, nn.Linear]
    want_w, want_b, sweeps = [], [], []
    for seed in (0, 1):
        _, graph, bottoms = synthetic.build('tiny_mobile', seed=seed)
        spec = graphspec.from_torch(graph, bottoms, targ)
        orc.merge_batchnorm(spec)
        n, _ = orc.cross_layer_equalization(spec, orc.create_relation(spec))
        orc.bias_correction(spec)
        sweeps.append(n)
        keys = [k for k in graph if type(graph[k]) in targ]
        want_w.append(np.concatenate([spec.nodes[k].weight.reshape(-1) for k in keys]))
        want_b.append(np.concatenate([spec.nodes[k].bias.reshape(-1) for k in keys if spec.nodes[k].bias is not None]))
    assert got['le_sweeps'].tolist() == sweeps
    # a batch of two tiny nets is smaller than the sample: the "sample" is every weight / bias of the batch, in order
    assert np.array_equal(got['weights_sample_index'], np.arange(2 * want_w[0].size))
    assert np.array_equal(got['biases_sample_index'], np.arange(2 * want_b[0].size))
    assert np.array_equal(got['weights_net0'].view(np.int32), want_w[0].astype(np.float32).view(np.int32))
    assert np.array_equal(got['weights_sample'].view(np.int32), np.concatenate(want_w).astype(np.float32).view(np.int32))
    assert np.abs(got['biases_net0'] - want_b[0]).max() <= 1e-5
    assert np.abs(got['biases_sample'] - np.concatenate(want_b)).max() <= 1e-5


def test_bench_dump_samples_a_large_batch_at_fixed_places(monkeypatch, tmp_path):
    """A batch larger than the sample: a fixed seeded set of sorted, distinct places, each holding the weight it names."""
    import numpy as np
    import torch
    import torch.nn as nn
    sys.path.insert(0, ROOT)
    import bench
    from dfq_amd import synthetic
    monkeypatch.setattr(bench, 'DUMP_SAMPLE', 1000)
    nets = [synthetic.build('tiny_mobile', seed=s) for s in range(3)]
    unit = {'nets': [(m, g, b, None) for (m, g, b) in nets]}
    flat = [torch.cat([m.weight.detach().reshape(-1) for m in g.values() if type(m) in (nn.Conv2d, nn.Linear)]).numpy()
            for (_, g, _) in nets]
    for d in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / d), unit, [1, 2, 3])
    load = lambda d, n: np.load(str(tmp_path / d / (n + '.npy')))     # noqa: E731
    for n in DUMP_FILES:
        assert np.array_equal(load('a', n), load('b', n)), n
    idx = load('a', 'weights_sample_index')
    assert 900 < idx.size <= 1000 and np.all(np.diff(idx) > 0) and idx[-1] < 3 * flat[0].size
    assert np.array_equal(load('a', 'weights_sample'), np.concatenate(flat)[idx.astype(np.int64)])
    assert np.array_equal(load('a', 'weights_net0'), flat[0]) and load('a', 'le_sweeps').tolist() == [1, 2, 3]


def test_bench_replica_is_a_deep_copy_less_the_model(engine):
    """bench.replicate, the copies every unit of work is made of: the graph, bottoms and relations copy.deepcopy would give
    (keys, module types, attributes, tensor values and types), and nothing mutable shared with the prototype."""
    import copy
    import torch
    sys.path.insert(0, ROOT)
    import bench
    proto = bench.prepare('tiny_res', 0, engine.device)
    want, got = copy.deepcopy(proto), bench.replicate(proto)
    assert got[0] is None
    assert got[2] == want[2] and got[2] is not proto[2]
    assert [vars(r) for r in got[3]] == [vars(r) for r in want[3]] and not {id(r) for r in got[3]} & {id(r) for r in proto[3]}
    assert list(got[1]) == list(want[1])
    for k, m in proto[1].items():
        a, b = want[1][k], got[1][k]
        if not isinstance(m, torch.nn.Module):
            assert a == b == m
            continue
        assert type(b) is type(a) and b is not m and list(b.__dict__) == list(a.__dict__)
        for name, v in m.__dict__.items():
            if isinstance(v, (dict, set)):
                assert b.__dict__[name] is not v and type(b.__dict__[name]) is type(a.__dict__[name])
            else:
                assert b.__dict__[name] == a.__dict__[name], (k, name)
        ta, tb, tm = ({**x._parameters, **x._buffers} for x in (a, b, m))
        assert list(tb) == list(ta)
        for n in ta:
            if ta[n] is None:
                assert tb[n] is None
                continue
            assert type(tb[n]) is type(ta[n]) and tb[n].requires_grad == ta[n].requires_grad and tb[n].dtype == ta[n].dtype
            assert tb[n].device == ta[n].device and torch.equal(tb[n], ta[n]) and tb[n].stride() == ta[n].stride()
            assert tb[n].untyped_storage().data_ptr() != tm[n].untyped_storage().data_ptr()


def test_bench_units_leave_their_prototypes_as_they_were(engine):
    """A batched unit's copies share the prototypes' storage until NetworkBatch moves them into the batch allocation: calibrating
    the unit changes its own weights and biases and leaves every tensor of the prototypes as it was."""
    import copy
    import torch
    sys.path.insert(0, ROOT)
    import bench
    protos = [bench.prepare('tiny_res', s, engine.device) for s in (0, 1)]
    before = copy.deepcopy(protos)
    unit = bench.make_unit(protos)
    assert 'batch' in unit
    unit['le'].run()
    unit['bc'].run()
    changed = 0
    for p, b, (_, g, _, _) in zip(protos, before, unit['nets']):
        for k, m in p[1].items():
            if not isinstance(m, torch.nn.Module):
                continue
            for n, t in {**m._parameters, **m._buffers}.items():
                if t is not None:
                    assert torch.equal(t, {**b[1][k]._parameters, **b[1][k]._buffers}[n]), (k, n)
            if type(m) in bench.TARG:
                changed += not torch.equal(g[k].weight, m.weight)
    assert changed > 0


def test_bench_unit_copies_compute_what_their_source_computes(engine):
    """copy_unit: a device copy of a laid-out batch with the plans moved onto it calibrates to the same bits as the batch
    itself, and running one leaves the other as it was."""
    import torch
    sys.path.insert(0, ROOT)
    import bench
    protos = [bench.prepare('tiny_res', s, engine.device) for s in (0, 1)]
    src = bench.make_unit(protos)
    cp = bench.copy_unit(src)
    bits = lambda t: t.view(torch.int32)         # noqa: E731 -- the padding between slots is never written: compare bits
    pristine = src['batch'].storage.clone()
    assert cp['storage'].data_ptr() != pristine.data_ptr() and torch.equal(bits(cp['storage']), bits(pristine))
    cp['le'].run()
    cp['bc'].run()
    assert torch.equal(bits(src['batch'].storage), bits(pristine))
    assert not torch.equal(bits(cp['storage']), bits(pristine))
    src['le'].run()
    src['bc'].run()
    assert torch.equal(bits(cp['storage']), bits(src['batch'].storage))
    assert [r['sweeps'] for r in cp['le'].query_all()[0]] == [r['sweeps'] for r in src['le'].query_all()[0]]
