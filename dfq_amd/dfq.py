"""Data-free quantisation passes on the MI355X engine, with the call surface of the reference's
``dfq.py``:

  _quantize_error            <- dfq.py:8-25
  _layer_equalization        <- dfq.py:28-75
  cross_layer_equalization   <- dfq.py:78-117
  bias_absorption            <- dfq.py:121-164
  clip_weight                <- dfq.py:167-170
  bias_correction            <- dfq.py:173-293

The Python here only walks the (graph, bottoms, relations) dictionaries to build flat work tables
(pointers + geometry); every per-channel loop of the reference runs inside libdfq_hip.so.  Callers'
``nn.Parameter`` objects are updated in place, ``Relation.S`` receives the cumulative scale vector,
missing biases are created as zero Parameters -- all as in the reference.
"""
from __future__ import annotations

import ctypes
from collections import OrderedDict

import torch
import torch.nn as nn

from . import _ffi
from .utils.layer_transform import _ensure_bias, find_prev_bn


# ------------------------------------------------------------------------------------------------
# helpers
# ------------------------------------------------------------------------------------------------
def _layer_entry(stage, weight, bias, groups=1):
    w = stage.bind(weight)
    b = stage.bind(bias)
    khkw = 1
    for d in w.shape[2:]:
        khkw *= int(d)
    return _ffi.DfqLayer(w.data_ptr(), b.data_ptr() if b is not None else None, int(w.shape[0]), int(w.shape[1]),
                         khkw, int(groups)), (w, b)


def _le_config(s_range, converge_thres, converge_count, signed, eps, max_sweeps):
    lo, hi = float(s_range[0]), float(s_range[1])
    return _ffi.DfqLeConfig(lo, hi, 1.0 / lo if lo != 0 else float('inf'), 1.0 / hi if hi != 0 else float('inf'),
                            int(hi > lo), float(eps), int(bool(signed)), float(converge_thres), int(converge_count),
                            -1 if max_sweeps is None else int(max_sweeps))


class _Snapshot:
    """A device-side copy of the tensors a plan rewrites: taken in front of a run whose launches contain in-launch waits, put
    back if a workgroup abandoned one (DFQ_ERR_ABANDONED) -- the pass is then repeated on launches that wait for nothing
    (``*_set_safe_mode``).  One flat buffer per plan, allocated at the first run; two multi-tensor copies."""

    def __init__(self, tensors):
        seen, self.src = set(), []
        for t in tensors:
            if t is not None and t.numel() > 0 and t.data_ptr() not in seen:
                seen.add(t.data_ptr())
                self.src.append(t)
        self.dst = None

    def take(self):
        if not self.src:
            return
        with torch.no_grad():
            if self.dst is None:
                flat = torch.empty(sum(t.numel() for t in self.src), dtype=self.src[0].dtype, device=self.src[0].device)
                self.dst, off = [], 0
                for t in self.src:
                    self.dst.append(flat[off:off + t.numel()].view(t.shape))
                    off += t.numel()
            torch._foreach_copy_(self.dst, self.src)

    def restore(self):
        if self.src and self.dst is not None:
            with torch.no_grad():
                torch._foreach_copy_(self.src, self.dst)


class LEPlan:
    """Device-side work list for cross-layer equalisation over a fixed set of layers/relations.

    Build once, then ``run`` (whole dfq.py:83-115 loop, synchronises once) or ``enqueue`` (fixed
    number of sweeps, asynchronous -- what bench.py times with the weights resident in HBM).
    """

    def __init__(self, layers, relations, stage=None, layer_net=None):
        """layers: list of (weight, bias|None, groups); relations: list of
        (first_idx, second_idx, bn_weight|None, bn_bias|None, scale_cum tensor [O1]).
        ``layer_net`` (optional, list of ints, non-decreasing) makes it a batched plan over several
        independent networks: every launch then covers all of them, each with its own loop state."""
        self.stage = stage or _ffi.Stage()
        self._keep = []
        self._mutable, self._snapshot, self.repeated = [], None, 0      # see run(): an abandoned in-launch wait is repeated, not raised
        if isinstance(layers, _Tables):                     # prebuilt struct arrays (build_le_plan_batch's fast path)
            t = layers
            self._keep, self.scale_cum = t.keep, t.scale_cum
            self._mutable = list(t.mutable)
            self._plan = ctypes.c_void_p()
            if t.bases is not None:                         # one network's tables + a base address per network (arena.py)
                self.n_layers, self.n_relations, self.n_nets = t.n_layers * len(t.bases), t.n_relations * len(t.bases), len(t.bases)
                _ffi.check(_ffi.lib().dfq_le_plan_create_replicated(
                    t.ptr('layers', _ffi.DfqLayer), t.n_layers, t.ptr('relations', _ffi.DfqRelation), t.n_relations,
                    t.bases.ctypes.data_as(ctypes.POINTER(ctypes.c_void_p)), len(t.bases), ctypes.byref(self._plan)))
                return
            self.n_layers, self.n_relations, self.n_nets = t.n_layers, t.n_relations, t.n_nets
            _ffi.check(_ffi.lib().dfq_le_plan_create_batch(t.ptr('layers', _ffi.DfqLayer), t.n_layers, t.ptr('layer_net', ctypes.c_int32),
                                                           t.n_nets, t.ptr('relations', _ffi.DfqRelation), t.n_relations,
                                                           ctypes.byref(self._plan)))
            return
        self.stage.prefetch([x for (w, b, g) in layers for x in (w, b)] +
                            [x for (i1, i2, bnw, bnb, scum) in relations for x in (bnw, bnb, scum)])
        entries = []
        for (w, b, g) in layers:
            e, keep = _layer_entry(self.stage, w, b, g)
            entries.append(e)
            self._keep.append(keep)
            self._mutable.extend(keep)
        rels = []
        self.scale_cum = []
        for (i1, i2, bnw, bnb, scum) in relations:
            bw, bb = self.stage.bind(bnw), self.stage.bind(bnb)
            sc = self.stage.bind(scum)
            self._keep.append((bw, bb, sc))
            self._mutable.extend((bw, bb, sc))
            self.scale_cum.append(sc)
            rels.append(_ffi.DfqRelation(int(i1), int(i2), bw.data_ptr() if bw is not None else None,
                                         bb.data_ptr() if bb is not None else None, sc.data_ptr()))
        self.n_layers, self.n_relations = len(entries), len(rels)
        larr = (_ffi.DfqLayer * len(entries))(*entries)
        rarr = (_ffi.DfqRelation * max(1, len(rels)))(*rels)
        self._plan = ctypes.c_void_p()
        if layer_net is None:
            self.n_nets = 1
            _ffi.check(_ffi.lib().dfq_le_plan_create(larr, len(entries), rarr, len(rels), ctypes.byref(self._plan)))
        else:
            self.n_nets = max(layer_net) + 1
            narr = (ctypes.c_int32 * len(entries))(*[int(v) for v in layer_net])
            _ffi.check(_ffi.lib().dfq_le_plan_create_batch(larr, len(entries), narr, self.n_nets, rarr, len(rels),
                                                           ctypes.byref(self._plan)))

    # -- introspection -----------------------------------------------------------------------
    @property
    def levels(self):
        return _ffi.lib().dfq_le_plan_levels(self._plan)

    @property
    def resident_tiles(self):
        """workgroups of the persistent whole-loop launch (weights in LDS for all sweeps), 0 if the plan streams"""
        return _ffi.lib().dfq_le_plan_resident_tiles(self._plan)

    @property
    def resident_reason(self):
        return (_ffi.lib().dfq_le_plan_resident_reason(self._plan) or b'').decode()

    @property
    def degraded(self):
        """runs of this plan that were repeated on per-level launches after the persistent launch abandoned a wait with
        nothing stored (dfq_le_plan_degraded); 0 in normal operation"""
        return _ffi.lib().dfq_le_plan_degraded(self._plan)

    @property
    def uniform(self):
        """True for a batch of like networks laid out back to back (dfq_le_plan_uniform)"""
        return bool(_ffi.lib().dfq_le_plan_uniform(self._plan))

    @property
    def depth(self):
        """dependency levels of the relation list (levels = equalisation launches per sweep: 1 unless DFQ_LE_MERGED=0)"""
        return _ffi.lib().dfq_le_plan_depth(self._plan)

    @property
    def paired_elements(self):
        return _ffi.lib().dfq_le_plan_paired_elements(self._plan)

    @property
    def rw_elements(self):
        """elements read and written per sweep (8 B each)"""
        return _ffi.lib().dfq_le_plan_rw_elements(self._plan)

    @property
    def deferred_elements(self):
        """Elements (a part of rw_elements) of layers that are scaled one way only: the streaming engine reads them every
        sweep but stores them every `defer_depth`-th one (include/dfq_hip.h)."""
        return _ffi.lib().dfq_le_plan_deferred_elements(self._plan)

    @property
    def defer_depth(self):
        return _ffi.lib().dfq_le_plan_defer_depth(self._plan)

    @property
    def store_depth(self):
        """Sweeps between two stores of the deferred elements: defer_depth, or for a lazy plan DFQ_LE_STORE_DEPTH (4, 8 or
        16, cut down to what the plan's tiles hold; include/dfq_hip.h)."""
        return _ffi.lib().dfq_le_plan_store_depth(self._plan)

    @property
    def free_running_elements(self):
        """Elements (NOT part of rw_elements) of layers whose every statistic is closed-form: the streaming engine reads and
        writes them once per `free_running_group` sweeps, in a lean launch of its own (dfq_le_cf.hpp, include/dfq_hip.h)."""
        return _ffi.lib().dfq_le_plan_free_running_elements(self._plan)

    @property
    def free_running_group(self):
        return _ffi.lib().dfq_le_plan_free_running_group(self._plan)

    @property
    def lean_background(self):
        """The lean launches of the free-running layers run on a second stream next to the sweep launches (include/dfq_hip.h)."""
        return bool(_ffi.lib().dfq_le_plan_lean_background(self._plan))

    @property
    def lean_tiles(self):
        return _ffi.lib().dfq_le_plan_lean_tiles(self._plan)

    def lean_info(self, tile):
        out = (ctypes.c_int64 * 3)()
        _ffi.check(_ffi.lib().dfq_le_plan_lean_info(self._plan, int(tile), out))
        return dict(kind=int(out[0]), rows=int(out[1]), cols=int(out[2]))

    @property
    def lazy(self):
        """The deferred layers are read only in their storing sweep and in sweeps whose verdict needs their |dW| sums
        (lazy sweeps, dfq_le.hip; batched plans with defer_depth > 1, DFQ_LE_LAZY_DW=0 turns them off)."""
        return bool(_ffi.lib().dfq_le_plan_lazy(self._plan))

    def lazy_stats(self):
        """dict(lazy_sweeps, uncertain, sweeps): lazy sweeps and uncertain verdicts since the plan was made, summed over the
        networks, and the sweeps of the current run (synchronises)."""
        out = (ctypes.c_int64 * 3)()
        _ffi.check(_ffi.lib().dfq_le_plan_lazy_stats(self._plan, _ffi.stream_arg(), out))
        return dict(lazy_sweeps=int(out[0]), uncertain=int(out[1]), sweeps=int(out[2]))

    def set_control_stage(self, n_partials):
        """Tests: lower the number of |dW| partials the convergence launch stages in LDS (what exceeds it is read from
        memory); returns the stage in force."""
        return int(_ffi.lib().dfq_le_plan_set_ctl_stage(self._plan, int(n_partials)))

    @property
    def sweep_bytes(self):
        """Bytes one sweep moves as executed (averaged over defer_depth sweeps and over a group of the free-running layers).
        A lazy plan is priced as if every sweep but a window's last were lazy: its deferred elements then move 4 B per
        defer_depth sweeps read and 4 B per store_depth sweeps written (what the always-lazy loop of a forced sweep count
        does)."""
        d, s = self.defer_depth, self.store_depth
        deferred = (8.0 - 4.0 / d - 4.0 / s) if self.lazy else 4.0 * (d - 1) / d
        return (8 * self.rw_elements + 4 * self.ro_elements - deferred * self.deferred_elements
                + 8.0 * self.free_running_elements / self.free_running_group)

    @property
    def ro_elements(self):
        """elements only read per sweep: the statistics pass over interior layers (4 B each)"""
        return _ffi.lib().dfq_le_plan_ro_elements(self._plan)

    @property
    def sweep_workgroups(self):
        """Persistent workgroups of a streaming sweep launch; 0: one workgroup per tile, or a resident plan."""
        return int(_ffi.lib().dfq_le_plan_sweep_workgroups(self._plan))

    def level_info(self, level):
        a, b, c = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int32()
        n = _ffi.lib().dfq_le_plan_level_launches(self._plan, level, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c))
        gx, gy = ctypes.c_int32(), ctypes.c_int32()
        _ffi.check(_ffi.lib().dfq_le_plan_level_grid(self._plan, level, ctypes.byref(gx), ctypes.byref(gy)))
        return dict(relations=n, rw_elements=a.value, ro_elements=b.value, workgroups=c.value,
                    grid=(gx.value, gy.value))

    # -- execution -----------------------------------------------------------------------------
    @property
    def has_waits(self):
        """True when a run of this plan can end abandoned AFTER tensors were rewritten: the streaming engine's one-launch sweep
        (dfq_le_plan_has_waits; the persistent launch of a single network stores all or nothing and repeats itself)."""
        return bool(_ffi.lib().dfq_le_plan_has_waits(self._plan))

    def set_safe_mode(self):
        """From now on one launch per dependency level: no workgroup waits for another one (dfq_le_plan_set_safe_mode)."""
        _ffi.check(_ffi.lib().dfq_le_plan_set_safe_mode(self._plan))

    def run(self, s_range=(1e-8, 1e8), converge_thres=2e-7, converge_count=20, signed=False, eps=0,
            max_sweeps=None, recover=True):
        """The whole loop of dfq.py:83-115; synchronises once.

        ``recover`` (default): a run that comes back with DFQ_ERR_ABANDONED -- a workgroup gave up a bounded in-launch wait
        (DFQ_SPIN_LIMIT: the chip was not the library's for seconds, or the dispatch order the waits count on did not hold) --
        is REPEATED instead of raised: the tensors the plan rewrites (weights, biases, BN proxies, cumulative scales: the
        caller's own tensors when they live on the device, the stage's shadows otherwise) are put back from a device-side copy
        taken in front of the run, the plan switches to one launch per dependency level for good (``set_safe_mode``: nothing
        waits, nothing can be abandoned) and the pass runs again.  ``repeated`` counts it.  The copy is only taken for plans
        whose launches contain in-launch waits and store as they go (``has_waits``); ``enqueue`` never takes one."""
        cfg = _le_config(s_range, converge_thres, converge_count, signed, eps, max_sweeps)
        res = _ffi.DfqLeResult()
        guard = recover and self.has_waits
        if guard:
            if self._snapshot is None:
                self._snapshot = _Snapshot(self._mutable)
            self._snapshot.take()
        try:
            _ffi.check(_ffi.lib().dfq_le_run(self._plan, ctypes.byref(cfg), _ffi.stream_arg(), ctypes.byref(res)))
        except _ffi.DfqError as exc:
            if not (guard and exc.code == _ffi.ERR_ABANDONED):
                raise
            self._snapshot.restore()
            self.set_safe_mode()
            self.repeated += 1
            degraded_runs['le'] += 1
            _ffi.check(_ffi.lib().dfq_le_run(self._plan, ctypes.byref(cfg), _ffi.stream_arg(), ctypes.byref(res)))
        return dict(sweeps=res.sweeps, stall_count=res.stall_count, diff=res.diff, last_diff_tmp=res.last_diff_tmp)

    def enqueue(self, n_sweeps, restart=True, s_range=(1e-8, 1e8), converge_thres=2e-7, converge_count=20,
                signed=False, eps=0, max_sweeps=None):
        cfg = _le_config(s_range, converge_thres, converge_count, signed, eps, max_sweeps)
        _ffi.check(_ffi.lib().dfq_le_enqueue(self._plan, ctypes.byref(cfg), int(n_sweeps), int(bool(restart)),
                                             _ffi.stream_arg()))

    def profile(self, n_sweeps, **kw):
        """Per-level kernel time (ms, summed over `n_sweeps` sweeps) from HIP events around each launch."""
        cfg = _le_config(kw.get('s_range', (1e-8, 1e8)), kw.get('converge_thres', 2e-7), kw.get('converge_count', 20),
                         kw.get('signed', False), kw.get('eps', 0), kw.get('max_sweeps', None))
        nl = self.levels
        level_ms = (ctypes.c_double * max(1, nl))()
        ctl = ctypes.c_double()
        nlaunch = ctypes.c_int32()
        empty = ctypes.c_double()
        lean = ctypes.c_double()
        nlean = ctypes.c_int32()
        _ffi.check(_ffi.lib().dfq_le_profile(self._plan, ctypes.byref(cfg), int(n_sweeps), _ffi.stream_arg(), level_ms,
                                             ctypes.byref(ctl), ctypes.byref(nlaunch), ctypes.byref(empty), ctypes.byref(lean),
                                             ctypes.byref(nlean)))
        return dict(level_ms=[level_ms[i] for i in range(nl)], control_ms=ctl.value, level_launches=nlaunch.value,
                    empty_bracket_ms=empty.value, lean_ms=lean.value, lean_launches=nlean.value)

    def trace(self, launch, block, **kw):
        """Shader-clock stamps of one workgroup's tile phases (tuning aid, see dfq_le_trace)."""
        cfg = _le_config(kw.get('s_range', (1e-8, 1e8)), -1.0, 10 ** 6, kw.get('signed', False), kw.get('eps', 0), None)
        out = (ctypes.c_int64 * 16)()
        _ffi.check(_ffi.lib().dfq_le_trace(self._plan, ctypes.byref(cfg), int(launch), int(block), _ffi.stream_arg(), out))
        return [int(v) for v in out]

    def block_info(self, launch, block):
        """What one workgroup of a launch does (tuning aid, see dfq_le_plan_block_info)."""
        out = (ctypes.c_int64 * 8)()
        _ffi.check(_ffi.lib().dfq_le_plan_block_info(self._plan, int(launch), int(block), out))
        return dict(kind=int(out[0]), rows=int(out[1]), cols=int(out[2]), rw_elements=int(out[3]), ro_elements=int(out[4]),
                    waits=bool(out[5]), publishes=bool(out[6]), relation=int(out[7]))

    def trace_blocks(self, launch, **kw):
        """(entry, exit, hw id) of every workgroup of one launch (tuning aid, see dfq_le_trace_blocks)."""
        cfg = _le_config(kw.get('s_range', (1e-8, 1e8)), -1.0, 10 ** 6, kw.get('signed', False), kw.get('eps', 0), None)
        gx, gy = self.level_info(launch)['grid']
        n = gx * gy
        out = (ctypes.c_int64 * (3 * n))()
        _ffi.check(_ffi.lib().dfq_le_trace_blocks(self._plan, ctypes.byref(cfg), int(launch), _ffi.stream_arg(), out, n))
        return [(int(out[3 * b]), int(out[3 * b + 1]), int(out[3 * b + 2])) for b in range(n)]

    def resident_stats(self):
        """Rollbacks of the last resident launch (dfq_le_resident_stats): dict(tiles_rolled_back, sweeps_undone, max_undone, spec, ckpt)."""
        out = (ctypes.c_int64 * 5)()
        _ffi.check(_ffi.lib().dfq_le_resident_stats(self._plan, _ffi.stream_arg(), out))
        return dict(tiles_rolled_back=int(out[0]), sweeps_undone=int(out[1]), max_undone=int(out[2]), spec=int(out[3]), ckpt=int(out[4]))

    def resident_trace(self, n_sweeps, **kw):
        """Per-workgroup phase stamps of the persistent launch (tuning aid, see dfq_le_resident_trace): list over tiles of
        dict(layer, rows, cols, stamps=[sweep][8])."""
        cfg = _le_config(kw.get('s_range', (1e-8, 1e8)), -1.0, 10 ** 9, kw.get('signed', False), kw.get('eps', 0), None)
        n = _ffi.lib().dfq_le_resident_trace_words(self._plan)
        out = (ctypes.c_int64 * n)()
        _ffi.check(_ffi.lib().dfq_le_resident_trace(self._plan, ctypes.byref(cfg), int(n_sweeps), _ffi.stream_arg(), out, n))
        tiles = []
        per = 6 * 16                                         # kTraceSweeps x kTracePoints of dfq_le_resident.hip
        for t in range(n // per):
            w = [int(out[t * per + i]) for i in range(per)]
            meta = w[7]
            tiles.append(dict(layer=meta >> 32, rows=(meta >> 16) & 0xffff, cols=meta & 0xffff,
                              stamps=[w[k * 16:k * 16 + 7] + w[k * 16 + 8:k * 16 + 16] for k in range(6)]))
        return tiles

    def query(self):
        res = _ffi.DfqLeResult()
        done = ctypes.c_int32()
        _ffi.check(_ffi.lib().dfq_le_query(self._plan, _ffi.stream_arg(), ctypes.byref(res), ctypes.byref(done)))
        return dict(sweeps=res.sweeps, stall_count=res.stall_count, diff=res.diff, last_diff_tmp=res.last_diff_tmp,
                    done=bool(done.value))

    def query_all(self):
        """Loop state of every network of a batched plan."""
        res = (_ffi.DfqLeResult * self.n_nets)()
        done = ctypes.c_int32()
        _ffi.check(_ffi.lib().dfq_le_query_all(self._plan, _ffi.stream_arg(), res, ctypes.byref(done)))
        return [dict(sweeps=r.sweeps, stall_count=r.stall_count, diff=r.diff, last_diff_tmp=r.last_diff_tmp)
                for r in res], bool(done.value)

    def close(self):
        if self._plan:
            _ffi.lib().dfq_le_plan_destroy(self._plan)
            self._plan = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- fast table building for batches -----------------------------------------------------------------------------------
# Building the descriptor tables of a batch used to cost ~3 ms of Python per network (graph walks, one ctypes structure per
# layer / relation / source, a Stage.bind per tensor): 100 ms for the benchmark's batch of 32 against 9 ms of GPU work.
# Networks of a batch are almost always the same architecture, so everything structural -- which layers, which relations,
# which BN feeds which correction step -- is derived ONCE per distinct structure (keyed on the graph's keys, node types,
# weight shapes, bottoms and relation triples) and per network only the device addresses are gathered, straight into numpy
# struct arrays laid out like the C structs of include/dfq_hip.h.
import numpy as _np

_LAYER_DT = _np.dtype({'names': ['weight', 'bias', 'out_ch', 'in_per_group', 'khkw', 'groups'],
                       'formats': ['u8', 'u8', 'i4', 'i4', 'i4', 'i4'], 'offsets': [0, 8, 16, 20, 24, 28], 'itemsize': 32})
_REL_DT = _np.dtype({'names': ['first', 'second', 'bn_weight', 'bn_bias', 'scale_cum'],
                     'formats': ['i4', 'i4', 'u8', 'u8', 'u8'], 'offsets': [0, 4, 8, 16, 24], 'itemsize': 32})
_SRC_DT = _np.dtype({'names': ['fake_weight', 'fake_bias', 'channels', 'relu', 'concat'],
                     'formats': ['u8', 'u8', 'i4', 'i4', 'i4'], 'offsets': [0, 8, 16, 20, 24], 'itemsize': 32})
_STEP_DT = _np.dtype({'names': ['layer', 'source_begin', 'source_count', 'next_bn_bias', 'net', 'reserved'],
                      'formats': ['i4', 'i4', 'i4', 'u8', 'i4', 'i4'], 'offsets': [0, 4, 8, 16, 24, 28], 'itemsize': 32})
assert (_LAYER_DT.itemsize, _REL_DT.itemsize, _SRC_DT.itemsize, _STEP_DT.itemsize) == (
    ctypes.sizeof(_ffi.DfqLayer), ctypes.sizeof(_ffi.DfqRelation), ctypes.sizeof(_ffi.DfqBcSource), ctypes.sizeof(_ffi.DfqBcStep))


def _cat(parts, dt):
    """concatenation that keeps the struct layout (numpy's own repacks a padded dtype)"""
    out = _np.zeros(sum(len(a) for a in parts), dtype=dt)
    off = 0
    for a in parts:
        out[off:off + len(a)] = a
        off += len(a)
    return out


class _Tables:
    """numpy struct arrays + what must stay alive while the plan exists"""

    def __init__(self):
        self.arrays = {}
        self.keep = []
        self.scale_cum = []
        self.mutable = []           # every tensor a run of the plan may rewrite (LEPlan / BCPlan snapshots)
        self.bases = None           # uint64 array: the tables describe the first of len(bases) networks (arena.py)

    def ptr(self, name, ctype):
        a = self.arrays[name]
        assert a.flags['C_CONTIGUOUS'] and a.dtype.itemsize == ctypes.sizeof(ctype)
        return a.ctypes.data_as(ctypes.POINTER(ctype))


_structure_cache = {}


def _dev_ptr(t, dev):
    """device address of a tensor the engine can use in place, else None (the caller falls back to the general path)"""
    if t.dtype is not torch.float32 or t.device != dev or not t.is_contiguous():
        return None
    return t.data_ptr()


_t_dev, _t_contig, _t_ptr = torch.Tensor.get_device, torch.Tensor.is_contiguous, torch.Tensor.data_ptr


def _dev_ptrs(tensors, dev):
    """_dev_ptr of a whole list (a batch of 32 MobileNetV2 has some 7 000 tensors: one pass per check, no Python per tensor
    beyond the method calls themselves) as a uint64 array, or None if one of them cannot be used in place"""
    if dev.type == 'cuda':
        idx = dev.index if dev.index is not None else torch.cuda.current_device()
    else:
        idx = -1
    f32 = torch.float32
    if not all(map(_t_contig, tensors)) or any(t.dtype is not f32 for t in tensors) or set(map(_t_dev, tensors)) - {idx}:
        return None
    return _np.fromiter(map(_t_ptr, tensors), dtype=_np.uint64, count=len(tensors))


def _le_template(graph, relations, targ_type):
    tt = tuple(targ_type)
    mods = [(k, m) for k, m in graph.items() if type(m) in tt]
    keys = [k for k, _ in mods]
    sig = ('le', tuple(keys), tuple(m._parameters['weight'].shape for _, m in mods), tuple(getattr(m, 'groups', 1) for _, m in mods),
           tuple([rr.get_idxs() for rr in relations]))
    t = _structure_cache.get(sig)
    if t is None:
        index = {k: i for i, k in enumerate(keys)}
        geo = []
        for k in keys:
            w = graph[k].weight
            khkw = 1
            for d in w.shape[2:]:
                khkw *= int(d)
            geo.append((int(w.shape[0]), int(w.shape[1]), khkw, int(getattr(graph[k], 'groups', 1))))
        rel = [(index[a], index[b], c) for (a, b, c) in (rr.get_idxs() for rr in relations)]
        t = dict(keys=keys, geo=_np.array(geo, dtype=_np.int32).reshape(len(keys), 4), rel=rel,
                 rel_idx=_np.array([(a, b) for (a, b, _) in rel], dtype=_np.int32).reshape(len(rel), 2),
                 firsts=sorted({index[rr.get_idxs()[0]] for rr in relations}),
                 o1=[int(graph[rr.get_idxs()[0]].weight.shape[0]) for rr in relations])
        _structure_cache[sig] = t
    return t


def _attr(mod, name):
    """getattr(mod, name, None) for an nn.Module without the detour through Module.__getattr__ (table building reads some
    ten thousand attributes per batch)"""
    d = mod.__dict__
    v = d.get(name)
    if v is None:
        v = d['_parameters'].get(name)
        if v is None:
            v = d['_buffers'].get(name)
    return v


def _fast_le_tables(items, targ_type, dev):
    """struct arrays for a batched LE plan, or None if some tensor needs the general (shadow-copy) path.  The structure of a
    network (geometry, relation indices) comes from a template shared by every network with the same graph; only the
    tensors' addresses are gathered per network, and those in one pass over the whole batch."""
    T = _Tables()
    geo, net_of, first, second = [], [], [], []
    fresh_scales = []                             # relations whose cumulative scale vector was created here
    tens = []                                     # every tensor whose address goes into a table ...
    w_pos, b_row, b_pos, s_pos, fw_row, fw_pos, fb_row, fb_pos = [], [], [], [], [], [], [], []   # ... and where it goes
    n_lay = n_rel = 0
    for net, (graph, relations) in enumerate(items):
        t = _le_template(graph, relations, targ_type)
        mods = [graph[k] for k in t['keys']]
        for i in t['firsts']:                                 # dfq.py:91-92
            _ensure_bias(mods[i])
        n = len(mods)
        for i, m in enumerate(mods):
            prm = m.__dict__['_parameters']
            w_pos.append(len(tens))
            tens.append(prm['weight'])
            b = prm.get('bias')
            if b is not None:
                b_row.append(n_lay + i)
                b_pos.append(len(tens))
                tens.append(b)
        geo.append(t['geo'])
        net_of.append(_np.full(n, net, dtype=_np.int32))
        # cumulative scale vectors: relations that have none yet share one flat allocation (one launch instead of one per relation)
        missing = [j for j, rr in enumerate(relations) if rr.S is None]
        if missing:
            flat = torch.ones(sum(t['o1'][j] for j in missing), dtype=torch.float32, device=dev)
            for j, v in zip(missing, flat.split([t['o1'][j] for j in missing])):
                relations[j].S = v
                fresh_scales.append(relations[j])
        for j, (rr, (i1, i2, kb)) in enumerate(zip(relations, t['rel'])):
            s_pos.append(len(tens))
            tens.append(rr.S)
            if kb is not None:
                bn = graph[kb]
                fw, fb = _attr(bn, 'fake_weight'), _attr(bn, 'fake_bias')
                if fw is not None:
                    fw_row.append(n_rel + j)
                    fw_pos.append(len(tens))
                    tens.append(fw)
                if fb is not None:
                    fb_row.append(n_rel + j)
                    fb_pos.append(len(tens))
                    tens.append(fb)
            T.scale_cum.append(rr.S)
        if t['rel']:
            ri = t['rel_idx']
            first.append(ri[:, 0] + n_lay)
            second.append(ri[:, 1] + n_lay)
        n_lay += n
        n_rel += len(relations)
        T.keep.append((mods, relations))
    ptr = _dev_ptrs(tens, dev)
    if ptr is None:
        for rr in fresh_scales:                   # the general path decides about these itself: leave no trace
            rr.S = None
        return None
    lay = _np.zeros(n_lay, dtype=_LAYER_DT)
    g = _np.concatenate(geo)
    lay['out_ch'], lay['in_per_group'], lay['khkw'], lay['groups'] = g[:, 0], g[:, 1], g[:, 2], g[:, 3]
    lay['weight'] = ptr[w_pos]
    lay['bias'][b_row] = ptr[b_pos]
    rel = _np.zeros(max(1, n_rel), dtype=_REL_DT)
    if n_rel:
        rel['first'][:n_rel], rel['second'][:n_rel] = _np.concatenate(first), _np.concatenate(second)
        rel['scale_cum'][:n_rel] = ptr[s_pos]
        rel['bn_weight'][fw_row] = ptr[fw_pos]
        rel['bn_bias'][fb_row] = ptr[fb_pos]
    T.arrays['layers'], T.arrays['relations'], T.arrays['layer_net'] = lay, rel, _np.concatenate(net_of)
    T.n_layers, T.n_relations, T.n_nets = n_lay, n_rel, len(items)
    T.mutable = tens
    return T


def _bc_template(graph, bottoms, targ_type, bn_type):
    tt = tuple(targ_type)
    mods = [(k, m) for k, m in graph.items() if type(m) in tt]
    keys = [k for k, _ in mods]
    sig = ('bc', tuple(graph.keys()), tuple(map(type, graph.values())),
           tuple([tuple(b) if isinstance(b, (list, tuple)) else b for b in bottoms.values()]),
           tuple(m._parameters['weight'].shape for _, m in mods), tuple(getattr(m, 'groups', 1) for _, m in mods))
    t = _structure_cache.get(sig)
    if t is None:
        # the general walk once, with the tensors replaced by (graph key, attribute) references
        layers, steps, _ = _bc_tables(graph, bottoms, targ_type, bn_type)
        owner = {}
        for k, m in graph.items():
            if type(m) == bn_type:
                for name in ('fake_weight', 'fake_bias'):
                    v = getattr(m, name, None)
                    if v is not None:
                        owner[id(v)] = (k, name)
        tsteps = []
        for (li, srcs, nxt, _) in steps:
            tsteps.append((li, [(owner[id(fw)] if fw is not None else None, owner[id(fb)], int(fb.numel()), bool(relu), bool(cat))
                                for (fw, fb, relu, cat) in srcs], owner[id(nxt)] if nxt is not None else None))
        geo = []
        for k in keys:
            w = graph[k].weight
            khkw = 1
            for d in w.shape[2:]:
                khkw *= int(d)
            geo.append((int(w.shape[0]), int(w.shape[1]), khkw, int(getattr(graph[k], 'groups', 1))))
        geo = _np.array(geo, dtype=_np.int32).reshape(len(keys), 4)
        # everything but the addresses: the step / source rows with network-relative indices, and which (graph key, attribute)
        # goes where
        step_arr = _np.zeros(len(tsteps), dtype=_STEP_DT)
        step_next, src_fw, src_fb, rows = [], [], [], []
        for j, (li, srcs, nxt) in enumerate(tsteps):
            step_arr['layer'][j], step_arr['source_begin'][j], step_arr['source_count'][j] = li, len(rows), len(srcs)
            if nxt is not None:
                step_next.append((j, nxt))
            for (fw, fb, ch, relu, cat) in srcs:
                if fw is not None:
                    src_fw.append((len(rows), fw))
                src_fb.append((len(rows), fb))
                rows.append((ch, int(relu), int(cat)))
        src_arr = _np.zeros(len(rows), dtype=_SRC_DT)
        if rows:
            cols = list(zip(*rows))
            src_arr['channels'], src_arr['relu'], src_arr['concat'] = cols[0], cols[1], cols[2]
        t = dict(keys=keys, geo=geo, steps=tsteps, bias_layers=sorted({li for (li, _, _) in tsteps}),
                 step_arr=step_arr, src_arr=src_arr, step_next=step_next, src_fw=src_fw, src_fb=src_fb,
                 step_out_ch=[int(geo[li, 0]) for (li, _, _) in tsteps], step_in=[int(geo[li, 1]) for (li, _, _) in tsteps])
        _structure_cache[sig] = t
    return t


def _fast_bc_tables(items, targ_type, bn_type, dev):
    T = _Tables()
    geo, steps, srcs = [], [], []
    T.step_out_ch, T.step_in, T.step_keys = [], [], []
    tens = []
    w_pos, b_row, b_pos, nx_row, nx_pos, sw_row, sw_pos, sb_row, sb_pos = [], [], [], [], [], [], [], [], []
    n_lay = n_stp = n_src = 0
    for net, (graph, bottoms) in enumerate(items):
        t = _bc_template(graph, bottoms, targ_type, bn_type)
        mods = [graph[k] for k in t['keys']]
        for li in t['bias_layers']:
            _ensure_bias(mods[li])
        for i, m in enumerate(mods):
            prm = m.__dict__['_parameters']
            w_pos.append(len(tens))
            tens.append(prm['weight'])
            b = prm.get('bias')
            if b is not None:
                b_row.append(n_lay + i)
                b_pos.append(len(tens))
                tens.append(b)
        geo.append(t['geo'])
        pos_of = {}

        def pos(ref):
            q = pos_of.get(ref)
            if q is None:
                q = pos_of[ref] = len(tens)
                tens.append(_attr(graph[ref[0]], ref[1]))
            return q
        for j, ref in t['step_next']:
            nx_row.append(n_stp + j)
            nx_pos.append(pos(ref))
        for r, ref in t['src_fw']:
            sw_row.append(n_src + r)
            sw_pos.append(pos(ref))
        for r, ref in t['src_fb']:
            sb_row.append(n_src + r)
            sb_pos.append(pos(ref))
        sa = t['step_arr'].copy()
        sa['layer'] += n_lay
        sa['source_begin'] += n_src
        sa['net'] = net
        steps.append(sa)
        srcs.append(t['src_arr'])
        T.step_out_ch.extend(t['step_out_ch'])
        T.step_in.extend(t['step_in'])
        T.step_keys.extend(t['keys'][li] for (li, _, _) in t['steps'])
        n_lay += len(mods)
        n_stp += len(sa)
        n_src += len(t['src_arr'])
        T.keep.append((mods, graph))
    ptr = _dev_ptrs(tens, dev)
    if ptr is None:
        return None
    lay = _np.zeros(n_lay, dtype=_LAYER_DT)
    g = _np.concatenate(geo)
    lay['out_ch'], lay['in_per_group'], lay['khkw'], lay['groups'] = g[:, 0], g[:, 1], g[:, 2], g[:, 3]
    lay['weight'] = ptr[w_pos]
    lay['bias'][b_row] = ptr[b_pos]
    stp, src = _cat(steps, _STEP_DT), _cat(srcs, _SRC_DT)
    stp['next_bn_bias'][nx_row] = ptr[nx_pos]
    src['fake_weight'][sw_row] = ptr[sw_pos]
    src['fake_bias'][sb_row] = ptr[sb_pos]
    T.arrays['layers'], T.arrays['steps'], T.arrays['sources'] = lay, stp, src
    T.n_layers, T.n_steps, T.n_sources = n_lay, n_stp, n_src
    weights = set(w_pos)
    T.mutable = [t for i, t in enumerate(tens) if i not in weights]      # the correction rewrites biases and BN proxies, never a weight
    return T


def build_le_plan_batch(items, targ_type, stage=None):
    """One plan over several independent networks: ``items`` is a list of (graph, relations).  The
    launches of a sweep then cover the whole batch (launch and latency costs are shared), while every
    network keeps the reference's own convergence loop."""
    stage = stage or _ffi.Stage()
    tables = _fast_le_tables(items, targ_type, stage.device)
    if tables is not None:
        return LEPlan(tables, None, stage=stage)
    layers, rels, layer_net = [], [], []
    for net, (graph, relations) in enumerate(items):
        keys = [k for k in graph if type(graph[k]) in targ_type]
        base = len(layers)
        index = {k: base + i for i, k in enumerate(keys)}
        for rr in relations:                                  # dfq.py:91-92
            _ensure_bias(graph[rr.get_idxs()[0]])
        layers += [(graph[k].weight, graph[k].bias, getattr(graph[k], 'groups', 1)) for k in keys]
        layer_net += [net] * len(keys)
        for rr in relations:
            kf, ks, kb = rr.get_idxs()
            if rr.S is None:
                rr.S = torch.ones(graph[kf].weight.size(0), dtype=torch.float32, device=stage.device)
            bn = graph[kb] if kb is not None else None
            rels.append((index[kf], index[ks], getattr(bn, 'fake_weight', None), getattr(bn, 'fake_bias', None), rr.S))
    return LEPlan(layers, rels, stage=stage, layer_net=layer_net)


def build_le_plan(graph, relations, targ_type, stage=None):
    """Work tables for ``cross_layer_equalization`` on a reference-format graph."""
    stage = stage or _ffi.Stage()
    keys = [k for k in graph if type(graph[k]) in targ_type]
    index = {k: i for i, k in enumerate(keys)}
    for rr in relations:                                  # dfq.py:91-92
        _ensure_bias(graph[rr.get_idxs()[0]])
    layers = [(graph[k].weight, graph[k].bias, getattr(graph[k], 'groups', 1)) for k in keys]
    rels = []
    missing = [rr for rr in relations if rr.S is None]        # one allocation (one fill launch) for all new scale vectors
    fresh = {}
    if missing:
        sizes = [int(graph[rr.get_idxs()[0]].weight.size(0)) for rr in missing]
        for rr, v in zip(missing, torch.ones(sum(sizes), dtype=torch.float32, device=stage.device).split(sizes)):
            fresh[id(rr)] = v
    for rr in relations:
        kf, ks, kb = rr.get_idxs()
        o1 = graph[kf].weight.size(0)
        if rr.S is None:
            scum = fresh[id(rr)]
        else:
            scum = rr.S
        bn = graph[kb] if kb is not None else None
        rels.append((index[kf], index[ks], getattr(bn, 'fake_weight', None), getattr(bn, 'fake_bias', None), scum))
    return LEPlan(layers, rels, stage=stage)


# ------------------------------------------------------------------------------------------------
# opt-in extension: lazy-scale equalisation (csrc/dfq_le_lazy.hip)
# ------------------------------------------------------------------------------------------------
class LazyLEPlan:
    """The sweeps of dfq.py:83-101 with a GIVEN sweep count per network, from the pristine weights and the cumulative scale
    vectors: a sweep only reads (4 B per paired element), the tensors are written once at the end.  Within 1e-5 of the
    sequentially rescaled result of the same number of sweeps, not bit-identical to it (the default engines are)."""

    def __init__(self, items, targ_type, stage=None):
        """items: list of (graph, relations), one per network (as for ``build_le_plan_batch``)."""
        self.stage = stage or _ffi.Stage()
        self._keep = []
        entries, rels, layer_net = [], [], []
        self.scale_cum = []
        for net, (graph, relations) in enumerate(items):
            keys = [k for k in graph if type(graph[k]) in targ_type]
            base = len(entries)
            index = {k: base + i for i, k in enumerate(keys)}
            for rr in relations:                                  # dfq.py:91-92
                _ensure_bias(graph[rr.get_idxs()[0]])
            for k in keys:
                e, keep = _layer_entry(self.stage, graph[k].weight, graph[k].bias, getattr(graph[k], 'groups', 1))
                entries.append(e)
                self._keep.append(keep)
            layer_net += [net] * len(keys)
            for rr in relations:
                kf, ks, kb = rr.get_idxs()
                if rr.S is None:
                    rr.S = torch.ones(graph[kf].weight.size(0), dtype=torch.float32, device=self.stage.device)
                bn = graph[kb] if kb is not None else None
                bw = self.stage.bind(getattr(bn, 'fake_weight', None))
                bb = self.stage.bind(getattr(bn, 'fake_bias', None))
                sc = self.stage.bind(rr.S)
                self._keep.append((bw, bb, sc))
                self.scale_cum.append(sc)
                rels.append(_ffi.DfqRelation(index[kf], index[ks], bw.data_ptr() if bw is not None else None,
                                             bb.data_ptr() if bb is not None else None, sc.data_ptr()))
        self.n_nets = len(items)
        larr = (_ffi.DfqLayer * len(entries))(*entries)
        rarr = (_ffi.DfqRelation * max(1, len(rels)))(*rels)
        narr = (ctypes.c_int32 * len(entries))(*layer_net)
        self._plan = ctypes.c_void_p()
        _ffi.check(_ffi.lib().dfq_le_lazy_plan_create(larr, len(entries), narr, self.n_nets, rarr, len(rels), ctypes.byref(self._plan)))

    @property
    def levels(self):
        return _ffi.lib().dfq_le_lazy_plan_levels(self._plan)

    @property
    def paired_elements(self):
        """elements the FIRST sweep reads (4 B each): every paired layer once per role"""
        return _ffi.lib().dfq_le_lazy_plan_paired_elements(self._plan)

    @property
    def sweep_elements(self):
        """elements every later sweep reads (4 B each): the non-depthwise layers in the interior of a chain, once per role
        (the extrema of the other passes do not change from sweep to sweep and are rescaled, not recomputed)"""
        return _ffi.lib().dfq_le_lazy_plan_sweep_elements(self._plan)

    @property
    def weight_elements(self):
        """elements of the paired tensors, written once at the end (8 B each)"""
        return _ffi.lib().dfq_le_lazy_plan_weight_elements(self._plan)

    def run(self, sweeps, s_range=(1e-8, 1e8), signed=False, eps=0):
        """Enqueue ``sweeps`` sweeps (an int, or one count per network) and the final materialisation (asynchronous)."""
        counts = [int(sweeps)] * self.n_nets if isinstance(sweeps, int) else [int(v) for v in sweeps]
        assert len(counts) == self.n_nets
        cfg = _le_config(s_range, -1.0, 10 ** 9, signed, eps, None)
        arr = (ctypes.c_int32 * self.n_nets)(*counts)
        _ffi.check(_ffi.lib().dfq_le_lazy_run(self._plan, ctypes.byref(cfg), arr, _ffi.stream_arg()))

    def close(self):
        if self._plan:
            _ffi.lib().dfq_le_lazy_plan_destroy(self._plan)
            self._plan = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def lazy_cross_layer_equalization(graph, relations, targ_type, sweeps, s_range=[1e-8, 1e8], signed=False, eps=0):
    """``cross_layer_equalization`` for a GIVEN number of sweeps in the lazy-scale formulation (see LazyLEPlan): same in-place
    update of the caller's tensors and of ``Relation.S``, within 1e-5 of what the sequential loop produces in ``sweeps`` sweeps."""
    with torch.no_grad():
        stage = _ffi.entry_stage()
        plan = LazyLEPlan([(graph, relations)], targ_type, stage=stage)
        try:
            plan.run(int(sweeps), s_range=s_range, signed=signed, eps=eps)
            _ffi.synchronize()
        finally:
            plan.close()
        stage.writeback()
        for rr, sc in zip(relations, plan.scale_cum):
            rr.S = stage.out_like(graph[rr.get_idxs()[0]].weight, sc)


# ------------------------------------------------------------------------------------------------
# dfq.py:8-25
# ------------------------------------------------------------------------------------------------
_REDUCTIONS = {None: 0, 'none': 0, 'sum': 1, 'mean': 2, 'channel': 3, 'spatial': 4}


def _quantize_error(param, num_bits=8, reduction='sum', signed=False):
    """Q(param) - param with per-tensor min/max; reduction in {'sum','mean','channel','spatial',None}."""
    mode = _REDUCTIONS.get(reduction, 0)
    lib = _ffi.lib()
    with torch.no_grad():
        stage = _ffi.Stage()
        x = stage.bind(param)
        n = x.numel()
        rows = 0
        if mode == 3:
            rows = x.shape[0]
        elif mode == 4:
            rows = x.shape[0] * x.shape[1]
        out = stage.new(x.shape) if mode == 0 else stage.new((1,))
        scratch = stage.new((int(lib.dfq_quant_error_scratch_bytes(n, rows)) // 4 + 4,), dtype=torch.int32)
        _ffi.check(lib.dfq_quant_error(_ffi.ptr(x), n, rows, int(num_bits), int(bool(signed)), mode, _ffi.ptr(out),
                                       _ffi.ptr(scratch), _ffi.stream_arg()))
        res = stage.out_like(param, out)
        return res if mode == 0 else res.reshape(())


# ------------------------------------------------------------------------------------------------
# dfq.py:28-75
# ------------------------------------------------------------------------------------------------
def _layer_equalization(weight_first, weight_second, bias_first, bn_weight=None, bn_bias=None,
                        s_range=(1e-8, 1e8), signed=False, eps=0):
    """Equalise one pair in place; returns (weight_first, weight_second, bias_first, S)."""
    with torch.no_grad():
        stage = _ffi.Stage()
        o1 = weight_first.shape[0]
        scum = torch.ones(o1, dtype=torch.float32, device=stage.device)
        plan = LEPlan([(weight_first, bias_first, 1), (weight_second, None, 1)],
                      [(0, 1, bn_weight, bn_bias, scum)], stage=stage)
        try:
            plan.run(s_range=s_range, signed=signed, eps=eps, max_sweeps=1, converge_thres=-1.0)
        finally:
            plan.close()
        stage.writeback()
        S = stage.out_like(weight_first, scum)
    return weight_first, weight_second, bias_first, S


# ------------------------------------------------------------------------------------------------
# dfq.py:78-117
# ------------------------------------------------------------------------------------------------
last_equalization = None      # result of the most recent cross_layer_equalization call


# The drop-in entry points used to build and destroy their plan on every call (descriptor tables, a dozen device
# allocations, one synchronisation: ~4-5 ms against 1 ms of GPU time for a MobileNetV2).  A caller that calibrates the same
# graph again -- the next checkpoint of a model, the second pass of main_cls.py's equalise / absorb / equalise sequence --
# now hits a small cache keyed on everything the plan depends on: device pointers and shapes of every tensor it binds, the
# relation structure, the engine-selecting environment.  Only device-resident tensors are cached (CPU tensors go through a
# per-call shadow copy whose addresses change).
# Thread safety and memory: one lock serialises the cached paths (a plan fetched by one thread must not be closed by another
# thread's eviction while it runs); a plan whose run raised is dropped (a failed in-launch wait leaves its device-side state
# and the tensors it binds undefined); every environment switch that shapes a plan is part of the key.  A cached plan pins
# its small device-side tables (LE: statistics arenas and tile tables, < 1.5 MB for a MobileNetV2; BC: descriptors and a
# correction vector per layer) until evicted: DFQ_PLAN_CACHE=n sets the number of plans kept per kind (default 8, 0 disables).
import os as _os
import threading as _threading

_PLAN_CACHE_SIZE = max(0, int(_os.environ.get('DFQ_PLAN_CACHE', '8') or 0))
_le_plan_cache = OrderedDict()
_bc_plan_cache = OrderedDict()
_cache_lock = _threading.RLock()
plan_cache_stats = {'le_hits': 0, 'le_misses': 0, 'bc_hits': 0, 'bc_misses': 0}
# Runs that were REPEATED on launches without in-launch waits after a workgroup of the one-launch kernels gave up a wait
# (DFQ_SPIN_LIMIT): LEPlan.run / BCPlan.run put the tensors back from their device-side snapshot, switch the plan to its safe mode
# (an explicit plan flag, dfq_*_plan_set_safe_mode) and run again.  0 in normal operation.
degraded_runs = {'le': 0, 'bc': 0}


# every environment switch the library reads while it CREATES a plan (tests/test_errors.py checks this list against the sources)
_PLAN_ENV = ('DFQ_LE_RESIDENT', 'DFQ_LE_MERGED', 'DFQ_LE_TILE_ELEMS', 'DFQ_LE_ROW_COLS', 'DFQ_LE_COL_COLS', 'DFQ_LE_BOOT_WORK',
             'DFQ_LE_PERSIST', 'DFQ_LE_SWEEP_WGS', 'DFQ_LE_EMIT_COLS', 'DFQ_LE_NO_SHORT', 'DFQ_LE_CHAIN_FIRST', 'DFQ_LE_POLL_NAPS',
             'DFQ_LE_DEFER', 'DFQ_LE_STORE_DEPTH', 'DFQ_LE_LAZY_DW', 'DFQ_LE_LAZY_MARGIN', 'DFQ_LE_CF', 'DFQ_LE_CF_GROUP', 'DFQ_LE_CF_BG', 'DFQ_LE_CF_BG_PRIO', 'DFQ_LE_CF_WEAVE', 'DFQ_LE_FUSE', 'DFQ_LE_UNIFORM', 'DFQ_LE_LOCAL_R1', 'DFQ_LE_LOCAL_ROW', 'DFQ_RES_EXACT_GROUPS', 'DFQ_RES_RELAXED', 'DFQ_RES_ORDER', 'DFQ_RES_SPEC', 'DFQ_RES_CKPT',
             'DFQ_RES_DIRECT', 'DFQ_RES_CF', 'DFQ_RES_SHORT_RPT', 'DFQ_RES_TILE_FLOATS', 'DFQ_BC_TAGGED', 'DFQ_BC_MERGED', 'DFQ_BC_BLOCKS', 'DFQ_BC_EPS', 'DFQ_BC_FOLD', 'DFQ_BC_MM_CHUNK', 'DFQ_BC_ONE_GROUP', 'DFQ_BC_ONE_LAUNCH', 'DFQ_BC_MM_AHEAD', 'DFQ_BC_SKEW',
             'DFQ_GRAPH', 'DFQ_COOPERATIVE', 'DFQ_HIP_LIB')
# ... and the ones it reads on every RUN (they change no plan)
_RUN_ENV = ('DFQ_SPIN_LIMIT', 'DFQ_TRACE_SWEEP', 'DFQ_PLAN_TIMING', 'DFQ_POOL_MB', 'DFQ_LE_GUARD_PER_LAUNCH')     # the last two: diagnostics / where a plan's tables are allocated


def _env_key():
    return tuple(_os.environ.get(k, '') for k in _PLAN_ENV)


def _tensor_key(t, device, stage=None):
    if t is None:
        return None
    if stage is not None:                                 # inside _ffi.staging(): the device copy the scope holds for a CPU tensor
        hit = stage._bound.get(id(t))
        if hit is not None:
            t = hit[1]
    if t.device != device or t.dtype != torch.float32 or not t.is_contiguous():
        raise _Uncacheable()
    return (t.data_ptr(), tuple(t.shape))


class _Uncacheable(Exception):
    pass


def _cache_get(cache, key):
    hit = cache.get(key)
    if hit is not None:
        cache.move_to_end(key)
    return hit


def _cache_put(cache, key, value):
    # a cached plan must not pin the caller's tensors: it is only ever used again after a key match, and the key is computed
    # from tensors that are alive at that moment (same addresses, same shapes); its own buffers stay with it
    plan = value[0]
    plan._keep = []
    if plan.stage._scoped or plan.stage._persistent:
        plan.stage = _ffi.Stage()         # the scope's (or the thread's persistent) stage is not the plan's: a private one for the helpers
    else:
        plan.stage._bound = {}
    cache[key] = value
    while len(cache) > _PLAN_CACHE_SIZE:
        _, old = cache.popitem(last=False)
        old[0].close()


def _cache_drop(cache, key):
    old = cache.pop(key, None)
    if old is not None:
        old[0].close()


def clear_plan_cache():
    with _cache_lock:
        for cache in (_le_plan_cache, _bc_plan_cache):
            while cache:
                _, old = cache.popitem()
                old[0].close()


def _le_cache_key(graph, relations, targ_type, scope=None):
    if _PLAN_CACHE_SIZE == 0:
        raise _Uncacheable()
    dev = _ffi.target_device()
    keys = [k for k in graph if type(graph[k]) in targ_type]
    if scope is not None:                                 # one packed transfer for everything the plan will bind
        scope.prefetch([x for k in keys for x in (graph[k].weight, graph[k].bias)] +
                       [getattr(graph[rr.get_idxs()[2]], n, None) for rr in relations if rr.get_idxs()[2] is not None
                        for n in ('fake_weight', 'fake_bias')])
    parts = [_env_key()]
    for k in keys:
        m = graph[k]
        parts.append((_tensor_key(m.weight, dev, scope), _tensor_key(m.bias, dev, scope), getattr(m, 'groups', 1)))
    for rr in relations:
        kf, ks, kb = rr.get_idxs()
        bn = graph[kb] if kb is not None else None
        parts.append((keys.index(kf), keys.index(ks), _tensor_key(getattr(bn, 'fake_weight', None), dev, scope),
                      _tensor_key(getattr(bn, 'fake_bias', None), dev, scope)))
    return tuple(parts)


def cross_layer_equalization(graph, relations, targ_type, s_range=[1e-8, 1e8], range_thres=0,
                             converge_thres=2e-7, converge_count=20, signed=False, eps=0,
                             visualize_state=False, max_sweeps=None):
    """Sweep the relation list until the reference's convergence test fires (dfq.py:83-115).

    ``range_thres`` and ``visualize_state`` are accepted and unused (the reference ignores
    ``range_thres`` too).  ``max_sweeps`` is an extension: an upper bound on the sweep count
    (``None`` = the reference's unbounded loop).  Returns None; see ``last_equalization``.
    """
    global last_equalization
    print("Start cross layer equalization")
    with torch.no_grad(), _cache_lock:
        for rr in relations:                                  # dfq.py:91-92 (before the cache key: biases are part of it)
            _ensure_bias(graph[rr.get_idxs()[0]])
        scope = _ffi.scoped_stage()                           # inside `with staging():` CPU tensors have stable device copies
        try:
            key = _le_cache_key(graph, relations, targ_type, scope)
        except _Uncacheable:
            key = None
        hit = _cache_get(_le_plan_cache, key) if key is not None else None
        if hit is not None:
            plan, scum, scum_flat = hit
            plan_cache_stats['le_hits'] += 1
            if all(rr.S is None for rr in relations):         # the plan accumulates into ITS buffers: start from 1 ...
                scum_flat.fill_(1.0)                          # (one launch for all of them)
            else:
                for rr, sc in zip(relations, scum):           # ... or from the caller's S
                    if rr.S is None:
                        sc.fill_(1.0)
                    else:
                        sc.copy_(rr.S)
            stage = scope or plan.stage or _ffi.Stage()
        else:
            plan_cache_stats['le_misses'] += 1
            stage = scope or _ffi.Stage()
            if key is not None:
                # cached plans own their cumulative-scale buffers (a Relation's S tensor is replaced on every call)
                saved = [rr.S for rr in relations]
                sizes = [int(graph[rr.get_idxs()[0]].weight.size(0)) for rr in relations]
                scum_flat = torch.ones(sum(sizes), dtype=torch.float32, device=stage.device)
                scum = list(scum_flat.split(sizes)) if sizes else []
                for rr, sc in zip(relations, scum):
                    if rr.S is not None:
                        sc.copy_(rr.S.detach())
                    rr.S = sc
                plan = build_le_plan(graph, relations, targ_type, stage=stage)
                for rr, s0 in zip(relations, saved):
                    rr.S = s0
                _cache_put(_le_plan_cache, key, (plan, scum, scum_flat))
            else:
                plan = build_le_plan(graph, relations, targ_type, stage=stage)
        try:
            res = plan.run(s_range=s_range, converge_thres=converge_thres, converge_count=converge_count,
                           signed=signed, eps=eps, max_sweeps=max_sweeps)
        except Exception as exc:
            if key is not None:
                _cache_drop(_le_plan_cache, key)      # an abandoned in-launch wait: the plan's state (and the device copies) are undefined
            else:
                plan.close()
            # (an abandoned in-launch wait never gets here: the persistent launch stores all or nothing and dfq_le_run repeats the
            # pass itself; the streaming engine's one-launch sweeps are repeated by LEPlan.run from its device-side snapshot)
            raise
        else:
            if key is None:
                plan.close()
        stage.writeback()
        if relations:
            first = graph[relations[0].get_idxs()[0]].weight
            outs = stage.out_like_many(first, plan.scale_cum)                    # one transfer for a host-resident model
            for rr, sc, out in zip(relations, plan.scale_cum, outs):
                rr.S = out.clone() if (key is not None and out is sc) else out    # Relation.set_scale_vec, cumulative
    last_equalization = res


# ------------------------------------------------------------------------------------------------
# dfq.py:121-164
# ------------------------------------------------------------------------------------------------
def _relu_between(graph, bottoms, layer_second, layer_first):
    key = layer_second
    while key != layer_first:
        assert len(bottoms[key]) == 1, 'graph in equalization relations should be 1-to-1 input-output'
        if type(graph[bottoms[key][0]]) == torch.nn.ReLU:
            return True
        key = bottoms[key][0]
    return False


def bias_absorption(graph, relations, bottoms, N=3):
    """Move the part of each first layer's bias that a following ReLU never clips into the second
    layer: c = max(0, beta~ - N*gamma~); b1 -= c; beta~ -= c; b2 += W2.sum(kh,kw) @ c."""
    print("Absorbing bias")
    lib = _ffi.lib()
    with torch.no_grad():
        stage = _ffi.entry_stage()
        for rr in relations:
            kf, ks, kb = rr.get_idxs()
            if not _relu_between(graph, bottoms, ks, kf):
                continue
            first, second, bn = graph[kf], graph[ks], graph[kb]
            _ensure_bias(first)
            _ensure_bias(second)
            w2 = stage.bind(second.weight)
            b1, b2 = stage.bind(first.bias), stage.bind(second.bias)
            fw, fb = stage.bind(bn.fake_weight), stage.bind(bn.fake_bias)
            khkw = w2[0, 0].numel() if w2.dim() > 2 else 1
            _ffi.check(lib.dfq_bias_absorb(_ffi.ptr(w2), w2.shape[0], w2.shape[1], khkw, first.weight.size(0),
                                           _ffi.ptr(b1), _ffi.ptr(b2), _ffi.ptr(fw), _ffi.ptr(fb),
                                           ctypes.c_float(N), _ffi.stream_arg()))
        stage.writeback()


# ------------------------------------------------------------------------------------------------
# dfq.py:167-170
# ------------------------------------------------------------------------------------------------
def clip_weight(graph, range_clip=[-15, 15], targ_type=[nn.Conv2d, nn.Linear]):
    lib = _ffi.lib()
    with torch.no_grad():
        stage = _ffi.entry_stage()
        for key in graph:
            if type(graph[key]) in targ_type:
                w = stage.bind(graph[key].weight)
                _ffi.check(lib.dfq_clamp(_ffi.ptr(w), w.numel(), ctypes.c_float(range_clip[0]),
                                         ctypes.c_float(range_clip[1]), _ffi.stream_arg()))
        stage.writeback()


# ------------------------------------------------------------------------------------------------
# extension: clip_weight with a searched bound (dfq_batch_clip_plan, include/dfq_hip.h)
# ------------------------------------------------------------------------------------------------
def _clip_config(who, bits, per_channel, signed, candidates, alpha_min, apply):
    """the arguments of the range search as a DfqBatchClipConfig, or ValueError('<who>: ...')"""
    import numbers
    ints = (int, numbers.Integral)
    if isinstance(bits, bool) or not isinstance(bits, ints) or not 2 <= bits <= 16:
        raise ValueError('{}: the bit width must be an int in [2, 16], got {!r}'.format(who, bits))
    if isinstance(candidates, bool) or not isinstance(candidates, ints) or not 1 <= candidates <= 64:
        raise ValueError('{}: candidates must be an int in [1, 64], got {!r}'.format(who, candidates))
    if isinstance(alpha_min, bool) or not isinstance(alpha_min, numbers.Real) or not 0.0 < float(alpha_min) <= 1.0:
        raise ValueError('{}: alpha_min must be a number in (0, 1], got {!r}'.format(who, alpha_min))
    return _ffi.DfqBatchClipConfig(int(bits), int(bool(signed)), int(bool(per_channel)), int(candidates), float(alpha_min),
                                   int(bool(apply)), 0)


class _ClipLayout:
    """The tensor table and the output blocks of one dfq_batch_clip_plan.  ``layers``: [(graph key, address of the weight in
    network 0, rows, row_len)].  A unit is a tensor, or an output row with ``per_row``; the blocks are torch tensors
    ``range_block`` float32 [n_nets, units, 2], ``chosen_block`` int32 [n_nets, units] and, with ``keep_errors``,
    ``error_block`` float64 [n_nets, units, K]."""

    def __init__(self, layers, n_nets, cfg, keep_errors, device):
        self.per_row, self.candidates = bool(cfg.per_row), int(cfg.candidates)
        entries, self.views, stride = [], [], 0            # (graph key, first unit, units)
        for key, address, rows, row_len in layers:
            units = rows if self.per_row else 1
            entries.append(_ffi.DfqBatchClipTensor(address, rows, row_len, stride))
            self.views.append((key, stride, units))
            stride += units
        self.stride, self.n_tensors = stride, len(entries)
        self.table = (_ffi.DfqBatchClipTensor * len(entries))(*entries)
        self.range_block = torch.zeros((n_nets, stride, 2), dtype=torch.float32, device=device)
        self.chosen_block = torch.zeros((n_nets, stride), dtype=torch.int32, device=device)
        self.error_block = torch.zeros((n_nets, stride, self.candidates), dtype=torch.float64, device=device) if keep_errors else None

    def block_args(self):
        """(ranges, chosen, errors, stride) as dfq_batch_clip_plan_create takes them"""
        return (self.range_block.data_ptr(), self.chosen_block.data_ptr(),
                None if self.error_block is None else self.error_block.data_ptr(), self.stride)

    def _views_of(self, row, tail):
        if self.per_row:
            return OrderedDict((key, row[off:off + units]) for (key, off, units) in self.views)
        return OrderedDict((key, row[off:off + 1].view(tail)) for (key, off, _) in self.views)

    def ranges(self, n):
        return self._views_of(self.range_block[n], (2,))

    def chosen(self, n):
        return self._views_of(self.chosen_block[n], ())

    def errors(self, n):
        if self.error_block is None:
            raise RuntimeError('clip_plan: the errors were not kept (keep_errors=True)')
        return self._views_of(self.error_block[n], (self.candidates,))

    def report(self, n):
        """``OrderedDict[key -> {'range', 'chosen', 'err_minmax', 'err'}]`` of network n as numpy values on the host: the chosen
        (l, h), k*, and sum e^2 of the min/max range (candidate 0) and of the chosen one; three device-to-host copies"""
        rng, cho, err = self.range_block[n].cpu().numpy(), self.chosen_block[n].cpu().numpy(), self.error_block[n].cpu().numpy()
        out = OrderedDict()
        for key, off, units in self.views:
            k = cho[off:off + units]
            e = err[off:off + units]
            best = e[range(units), k]
            if self.per_row:
                out[key] = {'range': rng[off:off + units].copy(), 'chosen': k.copy(), 'err_minmax': e[:, 0].copy(), 'err': best}
            else:
                out[key] = {'range': rng[off].copy(), 'chosen': int(k[0]), 'err_minmax': float(e[0, 0]), 'err': float(best[0])}
        return out


def clip_weight_mse(graph, bits_weight=8, per_channel=False, signed=False, candidates=32, alpha_min=0.5,
                    targ_type=[nn.Conv2d, nn.Linear]):
    """``clip_weight`` with a searched bound (extension): every ``targ_type`` weight -- every output row of it with
    ``per_channel`` -- is clamped in place to the one of ``candidates`` ranges, shrunk from its (min, max) by factors from 1
    down to ``alpha_min``, under which the ``bits_weight``-bit quantiser (``signed``: the symmetric recipe) has the least sum
    of squared errors.  The definition is the comment of dfq_batch_clip_plan_create (include/dfq_hip.h); the single-network
    form of ``NetworkBatch.clip_weight_mse``, the same plan over a batch of one.  Afterwards a weight's own (min, max) is the
    chosen range, which is what ``bias_correction``, ``quantize_targ_layer`` and the ncnn table take: call it where
    ``clip_weight`` stands, behind equalisation and absorption, in front of bias correction.  Returns
    ``OrderedDict[key -> {'range', 'chosen', 'err_minmax', 'err'}]``.  ValueError for a bit width that is not an int in
    [2, 16], ``candidates`` not an int in [1, 64], an ``alpha_min`` that is not a number in (0, 1]."""
    cfg = _clip_config('clip_weight_mse', bits_weight, per_channel, signed, candidates, alpha_min, True)
    lib = _ffi.lib()
    layers = [(key, graph[key].weight) for key in graph if type(graph[key]) in targ_type]
    if not layers:
        raise ValueError('clip_weight_mse: the graph has no {} layer'.format(tuple(targ_type)))
    with torch.no_grad():
        stage = _ffi.entry_stage()
        stage.prefetch([w for _, w in layers])
        bufs = [stage.bind(w) for _, w in layers]
        lay = _ClipLayout([(key, buf.data_ptr(), int(w.shape[0]), w.numel() // int(w.shape[0])) for (key, w), buf in zip(layers, bufs)],
                          1, cfg, True, stage.device)
        bases = (ctypes.c_void_p * 1)(bufs[0].data_ptr())
        plan = ctypes.c_void_p()
        _ffi.check(lib.dfq_batch_clip_plan_create(lay.table, lay.n_tensors, ctypes.byref(cfg), bases, 1, *lay.block_args(),
                                                  ctypes.byref(plan)))
        try:
            _ffi.check(lib.dfq_batch_clip_plan_run(plan, _ffi.stream_arg()))
            _ffi.synchronize()
            report = lay.report(0)
        finally:
            lib.dfq_batch_clip_plan_destroy(plan)
        stage.writeback()
    return report


# ------------------------------------------------------------------------------------------------
# extension: a bit width per layer under a size budget (dfq_batch_mixed_plan, include/dfq_hip.h)
# ------------------------------------------------------------------------------------------------
_MIXED_ENTRIES = 4096            # T * B the allocation's table holds
_MIXED_PAIRS = 512               # B * K a clipped plan searches


class _SquantLayout:
    """The tensor table and the output blocks of one dfq_batch_squant_plan, shared by ``NetworkBatch.squant_plan`` and
    ``quantize_mixed(rounding='squant')``.  ``layers``: [(graph key, weight)]; ``address(key, weight)`` gives the weight's device
    address in network 0; ``bits_of(key)`` the width that goes into the tensor's table entry.  The blocks are torch tensors
    [n_nets, stride]: ``range_block`` float32, ``stats_block`` int64, ``status_block`` int32 [n_nets] and, with ``codes``
    ('int32' or 'int8'), ``code_block``.  ValueError('<who>: ...') for a row longer than dfq_squant_max_row_len()."""

    def __init__(self, who, layers, address, n_nets, bits_of, per_channel, signed, codes, device):
        longest = int(_ffi.lib().dfq_squant_max_row_len())
        self.per_channel, self.signed = bool(per_channel), bool(signed)
        self.keys, self.n_nets, self.n_tensors = [key for key, _ in layers], n_nets, len(layers)
        entries, self._code_views, self._range_views, self._stats_views = [], [], [], []
        code_stride = range_stride = stats_stride = 0
        for key, w in layers:
            rows = int(w.shape[0])
            row_len = w.numel() // rows
            if row_len > longest:
                raise ValueError('{}: {}: rows of {} weights, the longest row is {}'.format(who, key, row_len, longest))
            klen = 1
            for d in w.shape[2:]:
                klen *= int(d)
            c_off = -1
            if codes is not None:
                c_off = code_stride
                self._code_views.append((key, c_off, w.numel(), tuple(w.shape)))
                code_stride += -(-w.numel() // 64) * 64
            self._range_views.append((key, range_stride, (rows, 2) if self.per_channel else (2,)))
            self._stats_views.append((key, stats_stride, rows))
            entries.append(_ffi.DfqBatchSquantTensor(address(key, w), rows, row_len, int(bits_of(key)), int(self.signed),
                                                     int(self.per_channel), 0, c_off, range_stride, klen, stats_stride))
            range_stride += 2 * rows if self.per_channel else 2
            stats_stride += 2 * rows
        self.table = (_ffi.DfqBatchSquantTensor * len(entries))(*entries)
        dtype = {None: torch.int32, 'int32': torch.int32, 'int8': torch.int8 if self.signed else torch.uint8}[codes]
        self.code_dtype = None if codes is None else dtype
        self.code_bytes = 1 if codes == 'int8' else 4
        self.code_stride, self.range_stride, self.stats_stride = code_stride, range_stride, stats_stride
        self.code_block = torch.empty((n_nets, code_stride), dtype=dtype, device=device) if codes is not None else None
        self.range_block = torch.empty((n_nets, range_stride), dtype=torch.float32, device=device)
        self.stats_block = torch.empty((n_nets, stats_stride), dtype=torch.int64, device=device)
        self.status_block = torch.zeros((n_nets,), dtype=torch.int32, device=device)

    def tables(self):
        """(tensors, n_tensors) as dfq_batch_squant_plan_create takes them in front of the bases"""
        return (self.table, self.n_tensors)

    def block_args(self):
        """(codes, code_bytes, code_stride, ranges, range_stride, stats, stats_stride) as create takes them behind the bases"""
        return (None if self.code_block is None else self.code_block.data_ptr(), self.code_bytes, self.code_stride,
                self.range_block.data_ptr(), self.range_stride, self.stats_block.data_ptr(), self.stats_stride)

    def codes(self, n):
        if self.code_block is None:
            return {}
        row = self.code_block[n]
        return {key: row[off:off + numel].view(shape) for (key, off, numel, shape) in self._code_views}

    def ranges(self, n):
        row = self.range_block[n]
        return {key: row[off:off + 2 * (shape[0] if len(shape) == 2 else 1)].view(shape) for (key, off, shape) in self._range_views}

    def stats(self, n):
        row = self.stats_block[n]
        return {key: row[off:off + 2 * rows].view(rows, 2) for (key, off, rows) in self._stats_views}


class _MixedLayout:
    """The tensor table, the configuration and the output blocks of one dfq_batch_mixed_plan; every argument is checked here,
    ValueError('<who>: ...') for what create would refuse.  ``layers``: [(graph key, weight)]; ``address(key, weight)`` gives
    the weight's device address in network 0.  The blocks are torch tensors: ``bits_block`` int32 [n_nets, T], ``error_block``
    float64 [n_nets, T, B], ``used_block`` int64 [n_nets, 2], ``cost_block`` float64 [n_nets], ``range_block`` float32
    [n_nets, range_stride] and, with ``codes``, ``code_block``."""

    def __init__(self, who, layers, address, n_nets, widths, avg_bits, budget_bits, per_channel, signed, sensitivity, pin, codes,
                 apply, device, clip=None, alpha_min=0.5):
        import math
        import numbers
        from fractions import Fraction
        ints = (int, numbers.Integral)
        try:
            widths = tuple(widths)
        except TypeError:
            raise ValueError('{}: widths must be a sequence of bit widths, got {!r}'.format(who, widths)) from None
        if not 2 <= len(widths) <= 8:
            raise ValueError('{}: 2 to 8 candidate widths, got {!r}'.format(who, widths))
        if any(isinstance(b, bool) or not isinstance(b, ints) or not 2 <= b <= 16 for b in widths):
            raise ValueError('{}: every width must be an int in [2, 16], got {!r}'.format(who, widths))
        if any(b <= a for a, b in zip(widths, widths[1:])):
            raise ValueError('{}: the widths must rise, got {!r}'.format(who, widths))
        widths = tuple(int(b) for b in widths)
        if not layers:
            raise ValueError('{}: no layer to quantise'.format(who))
        if len(layers) * len(widths) > _MIXED_ENTRIES:
            raise ValueError('{}: {} layers x {} widths, the allocation holds {} entries'.format(who, len(layers), len(widths), _MIXED_ENTRIES))
        if (avg_bits is None) == (budget_bits is None):
            raise ValueError('{}: exactly one of avg_bits and budget_bits'.format(who))
        total = sum(w.numel() for _, w in layers)
        if avg_bits is not None:
            if isinstance(avg_bits, bool) or not isinstance(avg_bits, numbers.Real) or not math.isfinite(avg_bits) or avg_bits < 0:
                raise ValueError('{}: avg_bits must be a finite number >= 0, got {!r}'.format(who, avg_bits))
            budget = int((Fraction(avg_bits) * total).__floor__())     # exact: the float's own value times an integer
        else:
            if isinstance(budget_bits, bool) or not isinstance(budget_bits, ints) or budget_bits < 0:
                raise ValueError('{}: budget_bits must be an int >= 0, got {!r}'.format(who, budget_bits))
            budget = int(budget_bits)
        if budget >= 2 ** 63:
            raise ValueError('{}: a budget of {} bits'.format(who, budget))
        if codes not in (None, 'int32', 'int8'):
            raise ValueError("{}: codes must be None, 'int32' or 'int8', got {!r}".format(who, codes))
        if codes == 'int8' and widths[-1] > 8:
            raise ValueError('{}: 1-byte codes need widths <= 8, got {!r}'.format(who, widths))
        if clip is not None:
            if isinstance(clip, bool) or not isinstance(clip, ints) or not 1 <= clip <= 64:
                raise ValueError('{}: clip must be None or an int in [1, 64] (the candidates), got {!r}'.format(who, clip))
            if isinstance(alpha_min, bool) or not isinstance(alpha_min, numbers.Real) or not 0.0 < float(alpha_min) <= 1.0:
                raise ValueError('{}: alpha_min must be a number in (0, 1], got {!r}'.format(who, alpha_min))
            if len(widths) * clip > _MIXED_PAIRS:
                raise ValueError('{}: {} widths x {} candidates, at most {} pairs'.format(who, len(widths), clip, _MIXED_PAIRS))
        keys = [key for key, _ in layers]
        sensitivity, pin = dict(sensitivity or {}), dict(pin or {})
        for name, table in (('sensitivity', sensitivity), ('pin', pin)):
            for key in table:
                if key not in keys:
                    raise ValueError('{}: {} names {!r}, which is no layer to quantise'.format(who, name, key))
        for key, s in sensitivity.items():
            if isinstance(s, bool) or not isinstance(s, numbers.Real) or not math.isfinite(s) or s < 0:
                raise ValueError('{}: the sensitivity of {!r} must be a finite number >= 0, got {!r}'.format(who, key, s))
        for key, b in pin.items():
            if isinstance(b, bool) or not isinstance(b, ints) or int(b) not in widths:
                raise ValueError('{}: {!r} is pinned to {!r}, which is none of the widths {!r}'.format(who, key, b, widths))
        self.widths, self.budget, self.total = widths, budget, total
        self.per_channel, self.signed, self.apply = bool(per_channel), bool(signed), bool(apply)
        self.keys, self.n_nets, self.n_tensors = keys, n_nets, len(layers)
        entries, self._code_views, self._range_views, self._unit_views = [], [], [], []
        code_stride = range_stride = unit_stride = 0
        for key, w in layers:
            rows = int(w.shape[0])
            self._unit_views.append((key, unit_stride, rows if self.per_channel else 1))
            unit_stride += rows if self.per_channel else 1
            c_off = -1
            if codes is not None:
                c_off = code_stride
                self._code_views.append((key, c_off, w.numel(), tuple(w.shape)))
                code_stride += -(-w.numel() // 64) * 64
            self._range_views.append((key, range_stride, (rows, 2) if self.per_channel else (2,)))
            entries.append(_ffi.DfqBatchMixedTensor(address(key, w), rows, w.numel() // rows, float(sensitivity.get(key, 1.0)),
                                                    int(pin.get(key, 0)), 0, c_off, range_stride))
            range_stride += 2 * rows if self.per_channel else 2
        self.table = (_ffi.DfqBatchMixedTensor * len(entries))(*entries)
        self.config = _ffi.DfqBatchMixedConfig((ctypes.c_int32 * 8)(*widths), len(widths), int(self.signed), int(self.per_channel),
                                               int(self.apply), {None: 0, 'int32': 4, 'int8': 1}[codes], 0, budget)
        dtype = {None: torch.int32, 'int32': torch.int32, 'int8': torch.int8 if self.signed else torch.uint8}[codes]
        self.code_dtype = None if codes is None else dtype
        self.code_stride, self.range_stride = code_stride, range_stride
        self.code_block = torch.zeros((n_nets, code_stride), dtype=dtype, device=device) if codes is not None else None
        self.range_block = torch.zeros((n_nets, range_stride), dtype=torch.float32, device=device)
        self.bits_block = torch.zeros((n_nets, len(entries)), dtype=torch.int32, device=device)
        self.error_block = torch.zeros((n_nets, len(entries), len(widths)), dtype=torch.float64, device=device)
        self.used_block = torch.zeros((n_nets, 2), dtype=torch.int64, device=device)
        self.cost_block = torch.zeros((n_nets,), dtype=torch.float64, device=device)
        self.clip = None if clip is None else int(clip)
        self.alpha_min = None if clip is None else float(alpha_min)
        self.clip_range_block = self.clip_chosen_block = self.unit_error_block = self.clip_desc = None
        if clip is not None:
            B = len(widths)
            self.unit_stride = unit_stride
            self.clip_range_block = torch.zeros((n_nets, unit_stride, B, 2), dtype=torch.float32, device=device)
            self.clip_chosen_block = torch.zeros((n_nets, unit_stride, B), dtype=torch.int32, device=device)
            self.unit_error_block = torch.zeros((n_nets, unit_stride, B), dtype=torch.float64, device=device)
            self._unit_offsets = (ctypes.c_int64 * len(entries))(*[off for _, off, _ in self._unit_views])
            self.clip_desc = _ffi.DfqBatchMixedClip(self.clip, 0, self.alpha_min, self.clip_range_block.data_ptr(),
                                                    self.clip_chosen_block.data_ptr(), self.unit_error_block.data_ptr(), unit_stride,
                                                    self._unit_offsets)

    def create(self, lib, bases, n_nets, plan):
        """the plan through today's entry point, or through dfq_batch_mixed_plan_create_clipped with ``clip``; returns the status"""
        if self.clip is None:
            return lib.dfq_batch_mixed_plan_create(*self.tables(), bases, n_nets, *self.block_args(), ctypes.byref(plan))
        return lib.dfq_batch_mixed_plan_create_clipped(*self.tables(), bases, n_nets, *self.block_args(), ctypes.byref(self.clip_desc),
                                                       ctypes.byref(plan))

    def _units(self, block, n):
        """{graph key: view [B, ...] of the tensor's unit, or [O, B, ...] of its rows} of network n's part of a clip block"""
        if block is None:
            raise RuntimeError('mixed_plan: the plan was made without clip=')
        row = block[n]
        return OrderedDict((key, row[off:off + units] if self.per_channel else row[off]) for (key, off, units) in self._unit_views)

    def clip_ranges(self, n):
        return self._units(self.clip_range_block, n)

    def clip_chosen(self, n):
        return self._units(self.clip_chosen_block, n)

    def unit_errors(self, n):
        return self._units(self.unit_error_block, n)

    def tables(self):
        """(tensors, n_tensors, config) as dfq_batch_mixed_plan_create takes them in front of the bases"""
        return (self.table, self.n_tensors, ctypes.byref(self.config))

    def block_args(self):
        """(bits, errors, used, cost, codes, code_stride, ranges, range_stride) as create takes them behind the bases"""
        return (self.bits_block.data_ptr(), self.error_block.data_ptr(), self.used_block.data_ptr(), self.cost_block.data_ptr(),
                None if self.code_block is None else self.code_block.data_ptr(), self.code_stride,
                self.range_block.data_ptr(), self.range_stride)

    def bits(self, n):
        row = self.bits_block[n].cpu().tolist()
        return OrderedDict((key, int(b)) for key, b in zip(self.keys, row))

    def errors(self, n):
        row = self.error_block[n].cpu().numpy()
        return OrderedDict((key, row[i].copy()) for i, key in enumerate(self.keys))

    def used(self, n):
        used, steps = self.used_block[n].cpu().tolist()
        return int(used), int(steps)

    def cost(self, n):
        return float(self.cost_block[n].cpu())

    def ranges(self, n):
        row = self.range_block[n]
        return OrderedDict((key, row[off:off + 2 * (shape[0] if len(shape) == 2 else 1)].view(shape)) for (key, off, shape) in self._range_views)

    def codes(self, n):
        if self.code_block is None:
            return {}
        row = self.code_block[n]
        return OrderedDict((key, row[off:off + numel].view(shape)) for (key, off, numel, shape) in self._code_views)


_NSR_MOMENTS = {'variance': 0, 'second_moment': 1}


class _NsrLayout:
    """The tensor table, the configuration and the output blocks of one dfq_batch_nsr_plan; every argument is checked here,
    ValueError('<who>: ...') for what create would refuse.  ``layers``: [(graph key, weight, groups)]; ``address(key, weight)``
    gives the weight's device address in network 0; ``sources``: the dfq_bc_source table of network 0 (numpy, _SRC_DT) and
    ``source_range[key]`` = (begin, count) in it -- a key without an entry gets ``input_moment``.  The blocks are torch tensors:
    ``moment_block`` float32 [n_nets, moment_stride], ``row_block`` float64 [n_nets, row_stride, B], ``signal_block`` float64
    [n_nets, row_stride], ``cost_block`` float64 [n_nets, T, B]."""

    def __init__(self, who, layers, address, n_nets, sources, source_range, widths, per_channel, signed, moment, input_moment, device):
        import math
        import numbers
        try:
            widths = tuple(widths)
        except TypeError:
            raise ValueError('{}: widths must be a sequence of bit widths, got {!r}'.format(who, widths)) from None
        if not 1 <= len(widths) <= 8:
            raise ValueError('{}: 1 to 8 candidate widths, got {!r}'.format(who, widths))
        if any(isinstance(b, bool) or not isinstance(b, numbers.Integral) or not 2 <= b <= 16 for b in widths):
            raise ValueError('{}: every width must be an int in [2, 16], got {!r}'.format(who, widths))
        if any(b <= a for a, b in zip(widths, widths[1:])):
            raise ValueError('{}: the widths must rise, got {!r}'.format(who, widths))
        if moment not in _NSR_MOMENTS:
            raise ValueError('{}: moment must be one of {}, got {!r}'.format(who, sorted(_NSR_MOMENTS), moment))
        if isinstance(input_moment, bool) or not isinstance(input_moment, numbers.Real) or not math.isfinite(input_moment) \
                or input_moment < 0 or float(input_moment) > 3.4028234663852886e38:
            raise ValueError('{}: input_moment must be a finite float32 >= 0, got {!r}'.format(who, input_moment))
        if not layers:
            raise ValueError('{}: no layer to look at'.format(who))
        self.widths = tuple(int(b) for b in widths)
        self.per_channel, self.signed, self.moment, self.input_moment = bool(per_channel), bool(signed), moment, float(input_moment)
        self.keys, self.n_nets, self.n_tensors = [key for key, _, _ in layers], n_nets, len(layers)
        entries, self._views = [], []
        moment_stride = row_stride = 0
        for key, w, groups in layers:
            rows = int(w.shape[0])
            row_len = w.numel() // rows
            klen = 1
            for d in w.shape[2:]:
                klen *= int(d)
            channels = row_len // klen * int(groups)
            begin, count = source_range.get(key, (0, 0))
            self._views.append((key, moment_stride, channels, row_stride, rows))
            entries.append(_ffi.DfqBatchNsrTensor(address(key, w), rows, row_len, klen, int(groups), int(begin), int(count), 0,
                                                  moment_stride, row_stride))
            moment_stride += -(-channels // 4) * 4
            row_stride += rows
        self.table = (_ffi.DfqBatchNsrTensor * len(entries))(*entries)
        self.sources = _np.ascontiguousarray(sources, dtype=_SRC_DT)
        self.config = _ffi.DfqBatchNsrConfig((ctypes.c_int32 * 8)(*self.widths), len(self.widths), int(self.signed), int(self.per_channel),
                                             _NSR_MOMENTS[moment], self.input_moment, 0)
        B = len(self.widths)
        self.moment_stride, self.row_stride = moment_stride, row_stride
        self.moment_block = torch.zeros((n_nets, moment_stride), dtype=torch.float32, device=device)
        self.row_block = torch.zeros((n_nets, row_stride, B), dtype=torch.float64, device=device)
        self.signal_block = torch.zeros((n_nets, row_stride), dtype=torch.float64, device=device)
        self.cost_block = torch.zeros((n_nets, len(entries), B), dtype=torch.float64, device=device)

    def tables(self):
        """(tensors, n_tensors, sources, n_sources, config) as dfq_batch_nsr_plan_create takes them in front of the bases"""
        return (self.table, self.n_tensors, ctypes.c_void_p(self.sources.ctypes.data if len(self.sources) else None), len(self.sources),
                ctypes.byref(self.config))

    def block_args(self):
        """(moments, moment_stride, rows, signal, row_stride, costs) as create takes them behind the bases"""
        return (self.moment_block.data_ptr(), self.moment_stride, self.row_block.data_ptr(), self.signal_block.data_ptr(),
                self.row_stride, self.cost_block.data_ptr())

    def costs(self, n):
        block = self.cost_block[n].cpu().numpy()
        return OrderedDict((key, block[i].copy()) for i, key in enumerate(self.keys))

    def rows(self, n):
        block = self.row_block[n].cpu().numpy()
        return OrderedDict((key, block[off:off + rows].copy()) for (key, _, _, off, rows) in self._views)

    def signal(self, n):
        block = self.signal_block[n].cpu().numpy()
        return OrderedDict((key, block[off:off + rows].copy()) for (key, _, _, off, rows) in self._views)

    def moments(self, n):
        block = self.moment_block[n].cpu().numpy()
        return OrderedDict((key, block[off:off + ch].copy()) for (key, off, ch, _, _) in self._views)


def _nsr_sources(graph, bottoms, targ_type, bn_type, address):
    """The dfq_bc_source table of one network for the layer sensitivities, from the bias-correction walk run WITHOUT its side
    effect (no layer gets a bias): (numpy _SRC_DT, {graph key: (begin, count)}).  ``address(tensor)``: its device address."""
    keys = [k for k in graph if type(graph[k]) in targ_type]
    _, steps, _ = _bc_tables(graph, bottoms, targ_type, bn_type, ensure_bias=False)
    rows, ranges = [], {}
    for (li, srcs, _, _) in steps:
        ranges[keys[li]] = (len(rows), len(srcs))
        for (fw, fb, relu, cat) in srcs:
            rows.append((0 if fw is None else address(fw), address(fb), int(fb.numel()), int(bool(relu)), int(bool(cat))))
    arr = _np.zeros(len(rows), dtype=_SRC_DT)
    for i, (fw, fb, ch, relu, cat) in enumerate(rows):
        arr['fake_weight'][i], arr['fake_bias'][i], arr['channels'][i], arr['relu'][i], arr['concat'][i] = fw, fb, ch, relu, cat
    return arr, ranges


def quantize_mixed(graph, widths=(2, 3, 4, 6, 8), avg_bits=None, budget_bits=None, per_channel=False, signed=False, sensitivity=None,
                   pin=None, targ_type=[nn.Conv2d, nn.Linear], cost='mse', bottoms=None, bn_type=torch.nn.BatchNorm2d,
                   moment='variance', input_moment=1.0, clip=None, alpha_min=0.5, rounding='nearest'):
    """Mixed-precision ``quantize_targ_layer`` for the weights (extension): every ``targ_type`` weight is quantised in place
    at a width of its own out of ``widths``, chosen so that the network takes at most ``budget_bits`` bits (or ``avg_bits``
    per weight on average: floor(avg_bits * number of weights)) and the sum of ``sensitivity[key]`` (default 1) times the
    layer's sum of squared quantisation errors is least -- the greedy walk the comment of dfq_batch_mixed_plan_create
    (include/dfq_hip.h) defines; ``pin[key]`` fixes a layer's width.  The single-network form of
    ``NetworkBatch.mixed_plan``, the same plan over a batch of one; it stands where ``quantize_targ_layer`` stands, behind
    equalisation, absorption and clipping.  Biases are left alone.  Returns
    ``OrderedDict[key -> {'bits', 'err', 'range'}]``: the chosen width, the sum e^2 at it, and the (min, max) the quantiser
    used ([2], or [O, 2] with ``per_channel``).  ValueError for what ``NetworkBatch.mixed_plan`` refuses.

    ``cost='nsr'`` allocates on the data-free layer sensitivities instead of the plain sum e^2 (dfq_batch_nsr_plan,
    include/dfq_hip.h: every output channel's expected noise-to-signal ratio under the BatchNorm proxies in front of the layer;
    ``NetworkBatch.nsr_plan`` for a batch of one).  It needs ``bottoms`` (ValueError without) and the proxies
    ``merge_batchnorm`` leaves on the ``bn_type`` modules; ``moment`` ('variance' or 'second_moment') and ``input_moment`` are
    ``nsr_plan``'s.  Each layer's dict then also holds ``'nsr'``, N at the chosen width.  No layer is given a bias.

    ``clip=K`` (an int in [1, 64]; ``alpha_min`` in (0, 1]) searches the MSE-optimal clip of every unit at every width, allocates
    on those errors and quantises every layer at its width's own range (dfq_batch_mixed_plan_create_clipped;
    ``NetworkBatch.mixed_plan(clip=)`` for a batch of one): ``'err'`` and ``'range'`` are then the clipped ones and the dict also
    holds ``'chosen'``, k* at the chosen width.  With ``cost='nsr'`` the costs come from the unclamped weights and the ranges are
    still the sum-e^2-optimal ones.

    ``rounding='squant'`` rounds adaptively at the allocated widths (``NetworkBatch.quantize_mixed(rounding='squant')`` for a
    batch of one): the plan only allocates (and, with ``clip``, clamps), then one adaptive-rounding plan reads the widths on the
    device (dfq_batch_squant_plan_set_widths).  ``'range'`` is then the adaptive rounding's, ``'err'`` still the sum e^2 of NEAREST
    rounding at the chosen width -- what the allocation walked on -- and the dict also holds ``'flips'``, the number of codes
    that differ from nearest.  ``'nearest'``, the default, is the path above; anything else is a ValueError."""
    lib = _ffi.lib()
    layers = [(key, graph[key].weight) for key in graph if type(graph[key]) in targ_type]
    if not layers:
        raise ValueError('quantize_mixed: the graph has no {} layer'.format(tuple(targ_type)))
    if cost not in ('mse', 'nsr'):
        raise ValueError("quantize_mixed: cost must be 'mse' or 'nsr', got {!r}".format(cost))
    if rounding not in ('nearest', 'squant'):
        raise ValueError("quantize_mixed: rounding must be 'nearest' or 'squant', got {!r}".format(rounding))
    squant = rounding == 'squant'
    if cost == 'nsr' and bottoms is None:
        raise ValueError("quantize_mixed: cost='nsr' reads the BatchNorms in front of every layer and needs `bottoms`")
    with torch.no_grad():
        stage = _ffi.entry_stage()
        proxies = []
        if cost == 'nsr':
            proxies = [t for m in graph.values() if type(m) == bn_type for t in (getattr(m, 'fake_weight', None), getattr(m, 'fake_bias', None))
                       if t is not None]
        stage.prefetch([w for _, w in layers] + proxies)
        bufs = {key: stage.bind(w) for key, w in layers}
        lay = _MixedLayout('quantize_mixed', layers, lambda key, w: bufs[key].data_ptr(), 1, widths, avg_bits, budget_bits, per_channel,
                           signed, sensitivity, pin, None, not squant, stage.device, clip, alpha_min)
        bases = (ctypes.c_void_p * 1)(bufs[layers[0][0]].data_ptr())
        plan, nsr, nlay, sq, flips = ctypes.c_void_p(), ctypes.c_void_p(), None, ctypes.c_void_p(), None
        try:
            if cost == 'nsr':
                sources, ranges_of = _nsr_sources(graph, bottoms, targ_type, bn_type, lambda t: stage.bind(t).data_ptr())
                nlay = _NsrLayout('quantize_mixed', [(key, w, getattr(graph[key], 'groups', 1)) for key, w in layers],
                                  lambda key, w: bufs[key].data_ptr(), 1, sources, ranges_of, lay.widths, per_channel, signed, moment,
                                  input_moment, stage.device)
                _ffi.check(lib.dfq_batch_nsr_plan_create(*nlay.tables(), bases, 1, *nlay.block_args(), ctypes.byref(nsr)))
                _ffi.check(lib.dfq_batch_nsr_plan_run(nsr, _ffi.stream_arg()))
            _ffi.check(lay.create(lib, bases, 1, plan))
            if nlay is not None:
                _ffi.check(lib.dfq_batch_mixed_plan_set_costs(plan, nlay.cost_block.data_ptr()))
            if squant and lay.clip is not None:
                _ffi.check(lib.dfq_batch_mixed_plan_run_stages(plan, _ffi.MIXED_ALLOCATE | _ffi.MIXED_CLAMP, _ffi.stream_arg()))
            else:
                _ffi.check(lib.dfq_batch_mixed_plan_run(plan, _ffi.stream_arg()))
            if squant:
                sl = _squant_at_widths(lib, layers, bufs, bases, lay, sq)
            _ffi.synchronize()
            bits, errors, ranges = lay.bits(0), lay.errors(0), lay.ranges(0)
            if squant:
                if int(sl.status_block[0].cpu()):
                    raise RuntimeError('quantize_mixed: the allocation left a width that is no width (status {})'.format(
                        int(sl.status_block[0].cpu())))
                ranges, flips = sl.ranges(0), sl.stats(0)
            costs = nlay.costs(0) if nlay is not None else None
            chosen = {key: v.cpu().numpy().copy() for key, v in lay.clip_chosen(0).items()} if lay.clip is not None else None
        finally:
            if sq:
                lib.dfq_batch_squant_plan_destroy(sq)
            if plan:
                lib.dfq_batch_mixed_plan_destroy(plan)
            if nsr:
                lib.dfq_batch_nsr_plan_destroy(nsr)
        stage.writeback(unchanged=proxies)
    out = OrderedDict((key, {'bits': bits[key], 'err': float(errors[key][lay.widths.index(bits[key])]),
                             'range': ranges[key].cpu().numpy().copy()}) for key in lay.keys)
    if costs is not None:
        for key in lay.keys:
            out[key]['nsr'] = float(costs[key][lay.widths.index(bits[key])])
    if chosen is not None:
        for key in lay.keys:
            out[key]['chosen'] = chosen[key][..., lay.widths.index(bits[key])]
    if flips is not None:
        for key in lay.keys:
            out[key]['flips'] = int(flips[key][:, 1].sum().cpu())
    return out


def _squant_at_widths(lib, layers, bufs, bases, lay, sq):
    """quantize_mixed(rounding='squant'): the adaptive-rounding plan of one network at the widths ``lay.bits_block`` holds on the
    device, created into ``sq`` and enqueued.  Returns its _SquantLayout, whose blocks are written once the stream has run."""
    sl = _SquantLayout('quantize_mixed', layers, lambda key, w: bufs[key].data_ptr(), 1, lambda key: lay.widths[-1], lay.per_channel,
                       lay.signed, None, lay.bits_block.device)
    _ffi.check(lib.dfq_batch_squant_plan_create(*sl.tables(), bases, 1, *sl.block_args(), ctypes.byref(sq)))
    index = (ctypes.c_int32 * sl.n_tensors)(*range(sl.n_tensors))
    _ffi.check(lib.dfq_batch_squant_plan_set_widths(sq, lay.bits_block.data_ptr(), lay.n_tensors, index, sl.status_block.data_ptr()))
    _ffi.check(lib.dfq_batch_squant_plan_run(sq, _ffi.stream_arg()))
    return sl


# ------------------------------------------------------------------------------------------------
# dfq.py:173-293
# ------------------------------------------------------------------------------------------------
class BCPlan:
    """Flat tables for the bias-correction chain of one graph (see build_bc_plan)."""

    def __init__(self, layers, steps, stage=None):
        """layers: list of (weight, bias, groups); steps: list of (layer_idx, [source,...],
        next_bn_bias|None[, net]); source = (fake_weight, fake_bias, relu, concat).  With `net` ids
        (network by network) the j-th steps of all networks share one launch."""
        self.stage = stage or _ffi.Stage()
        self._keep = []
        self._mutable, self._snapshot, self.repeated = [], None, 0      # see run(check=True)
        # run(widths=): the graph keys of the steps as created (one network's; None where the builder does not know them), how
        # many networks the plan replicates them for, and what the latest widths run must keep alive
        self.keys, self.n_nets, self._widths_keep, self._widths_map = None, 1, None, None
        if isinstance(layers, _Tables):                     # prebuilt struct arrays (build_bc_plan_batch's fast path)
            t = layers
            self._keep = t.keep
            self._mutable = list(t.mutable)
            self.n_steps = t.n_steps
            self.step_out_ch, self.step_in = t.step_out_ch, t.step_in
            self.keys = getattr(t, 'step_keys', None)
            self._created_steps = t.n_steps
            self._plan = ctypes.c_void_p()
            if t.bases is not None:                         # one network's tables + a base address per network (arena.py)
                n = self.n_nets = len(t.bases)
                self.n_steps, self.step_out_ch, self.step_in = t.n_steps * n, t.step_out_ch * n, t.step_in * n
                _ffi.check(_ffi.lib().dfq_bc_plan_create_replicated(
                    t.ptr('layers', _ffi.DfqLayer), t.n_layers, t.ptr('steps', _ffi.DfqBcStep), t.n_steps,
                    t.ptr('sources', _ffi.DfqBcSource), t.n_sources,
                    t.bases.ctypes.data_as(ctypes.POINTER(ctypes.c_void_p)), n, ctypes.byref(self._plan)))
                return
            _ffi.check(_ffi.lib().dfq_bc_plan_create(t.ptr('layers', _ffi.DfqLayer), t.n_layers, t.ptr('steps', _ffi.DfqBcStep), t.n_steps,
                                                     t.ptr('sources', _ffi.DfqBcSource), t.n_sources, ctypes.byref(self._plan)))
            return
        self.stage.prefetch([x for (w, b, g) in layers for x in (w, b)] +
                            [x for st in steps for (fw, fb, relu, concat) in st[1] for x in (fw, fb)] + [st[2] for st in steps])
        entries = []
        for (w, b, g) in layers:
            e, keep = _layer_entry(self.stage, w, b, g)
            entries.append(e)
            self._keep.append(keep)
            self._mutable.append(keep[1])
        src_arr, step_arr = [], []
        steps = [tuple(st) + (0,) if len(st) == 3 else tuple(st) for st in steps]
        for (li, srcs, nxt, net) in steps:
            begin = len(src_arr)
            for (fw, fb, relu, concat) in srcs:
                dfw, dfb = self.stage.bind(fw), self.stage.bind(fb)
                self._keep.append((dfw, dfb))
                src_arr.append(_ffi.DfqBcSource(dfw.data_ptr() if dfw is not None else None, dfb.data_ptr(),
                                                int(dfb.numel()), int(bool(relu)), int(bool(concat))))
            dn = self.stage.bind(nxt)
            self._keep.append(dn)
            self._mutable.append(dn)
            step_arr.append(_ffi.DfqBcStep(int(li), begin, len(srcs), dn.data_ptr() if dn is not None else None,
                                           int(net), 0))
        self.n_steps = self._created_steps = len(step_arr)
        self.step_out_ch = [int(layers[li][0].shape[0]) for (li, _, _, _) in steps]
        self.step_in = [int(layers[li][0].shape[1]) for (li, _, _, _) in steps]
        larr = (_ffi.DfqLayer * len(entries))(*entries)
        sarr = (_ffi.DfqBcStep * len(step_arr))(*step_arr)
        carr = (_ffi.DfqBcSource * len(src_arr))(*src_arr)
        self._plan = ctypes.c_void_p()
        _ffi.check(_ffi.lib().dfq_bc_plan_create(larr, len(entries), sarr, len(step_arr), carr, len(src_arr),
                                                 ctypes.byref(self._plan)))

    @property
    def weight_elements(self):
        return _ffi.lib().dfq_bc_plan_weight_elements(self._plan)

    @property
    def eps_elements(self):
        return _ffi.lib().dfq_bc_plan_eps_elements(self._plan)

    @property
    def has_waits(self):
        """True when the chain runs as one launch whose workgroups wait for each other (dfq_bc_plan_has_waits)."""
        return bool(_ffi.lib().dfq_bc_plan_has_waits(self._plan))

    def set_safe_mode(self):
        """From now on one launch per chain position: nothing waits, nothing can be abandoned (dfq_bc_plan_set_safe_mode)."""
        _ffi.check(_ffi.lib().dfq_bc_plan_set_safe_mode(self._plan))

    def run(self, signed=False, check=False, recover=True, per_channel=False, bits=8, widths=None):
        """Enqueue the whole correction (asynchronous).  ``check`` synchronises; with ``recover`` (default) a run in which a
        workgroup of the one-launch chain gave up its wait (DFQ_ERR_ABANDONED) is then REPEATED instead of raised: biases and BN
        proxies go back to a device-side copy taken in front of the run, the plan switches to one launch per chain position for
        good (``set_safe_mode``) and the correction runs again (``repeated`` counts it).  Without ``check`` nothing is copied
        and an abandoned run surfaces at the next ``status()``.

        ``per_channel`` (extension): the quant error of output row o is Q_o(W) - W with row o's own (min, max) at ``bits``
        bits (2..16; dfq_bc_plan_run_per_channel).  The per-tensor mode ignores ``bits`` (8, like dfq.py:218).

        ``widths`` (extension; dfq_bc_plan_run_widths holds the definition): every layer's quant error at that layer's OWN bit
        width -- per tensor, or per output row with ``per_channel`` -- the error of what ``quant_plan(bit_weight=that width)`` or
        ``mixed_plan`` will store for it.  ``None``: the behaviour above in every respect.  An ``int``: one width for every
        step (2..16), per tensor too.  A mapping ``graph key -> int``: plans that know their keys (``build_bc_plan``,
        ``NetworkBatch.bc_plan``, ``bias_correction``); every network of a batch gets the same widths.  A ``BatchMixedPlan``:
        its bits block is read on the device, where its run left it -- nothing goes to the host; its ``per_channel`` /
        ``signed`` must be the run's.  ``(tensor, width_index[, width_stride])``: a device int32 tensor, the width of step s of
        network n is ``tensor[n * width_stride + width_index[s]]`` (one index per step as created); values outside [2, 16]
        that the device reads are clamped.  ValueError for a step without a width and for a host-given width outside [2, 16].
        ``bits`` is not used by a widths run."""
        wargs = None
        if widths is not None:
            wargs = self._widths_args(widths, per_channel, signed)
        elif per_channel:
            _check_bits(bits)
        guard = check and recover and self.has_waits
        if guard:
            if self._snapshot is None:
                self._snapshot = _Snapshot(self._mutable)
            self._snapshot.take()
        self._launch(signed, per_channel, bits, wargs)
        if check:
            try:
                self.status()
            except _ffi.DfqError as exc:
                if not (guard and exc.code == _ffi.ERR_ABANDONED):
                    raise
                self._snapshot.restore()
                self.set_safe_mode()
                self.repeated += 1
                degraded_runs['bc'] += 1
                self._launch(signed, per_channel, bits, wargs)
                self.status()

    def _widths_args(self, widths, per_channel, signed):
        """(device int32 tensor or None, width_stride, host index table or None, uniform bits) of run(widths=)"""
        from collections.abc import Mapping
        if isinstance(widths, int) and not isinstance(widths, bool):
            _check_width(widths, 'every step')
            return (None, 0, None, int(widths))
        if hasattr(widths, 'bits_block') and hasattr(widths, 'keys') and not isinstance(widths, Mapping):      # a BatchMixedPlan
            if bool(widths.per_channel) != bool(per_channel) or bool(widths.signed) != bool(signed):
                raise ValueError('BCPlan.run: the mixed plan allocated for per_channel={}, signed={}, the run corrects per_channel={}, '
                                 'signed={}'.format(widths.per_channel, widths.signed, bool(per_channel), bool(signed)))
            if widths.n_nets != self.n_nets:
                raise ValueError('BCPlan.run: the mixed plan covers {} networks, this plan {}'.format(widths.n_nets, self.n_nets))
            tensor, table, stride = widths.bits_block, list(widths.keys), widths.n_tensors
        elif isinstance(widths, Mapping):
            if self.keys is None:
                raise ValueError('BCPlan.run: this plan does not know the graph keys of its steps; give (tensor, width_index)')
            missing = [key for key in self.keys if key not in widths]
            if missing:
                raise ValueError('BCPlan.run: no width for the step(s) {!r}'.format(missing))
            for key in self.keys:
                _check_width(widths[key], repr(key))
            values = tuple(int(widths[key]) for key in self.keys)
            if self._widths_map is None or self._widths_map[0] != values:      # (one upload per distinct mapping)
                self._widths_map = (values, torch.tensor(values, dtype=torch.int32, device=self.stage.device))
            tensor, stride, index, table = self._widths_map[1], 0, list(range(len(values))), None
        elif isinstance(widths, (tuple, list)) and len(widths) in (2, 3) and isinstance(widths[0], torch.Tensor):
            tensor, index = widths[0], [int(i) for i in widths[1]]
            stride = int(widths[2]) if len(widths) == 3 else 0
            table = None
        else:
            raise ValueError('BCPlan.run: widths must be None, an int, a mapping key -> int, a BatchMixedPlan or '
                             '(int32 device tensor, width_index[, width_stride]), got {!r}'.format(type(widths)))
        if table is not None:
            if self.keys is None:
                raise ValueError('BCPlan.run: this plan does not know the graph keys of its steps; give (tensor, width_index)')
            where = {key: i for i, key in enumerate(table)}
            missing = [key for key in self.keys if key not in where]
            if missing:
                raise ValueError('BCPlan.run: no width for the step(s) {!r}'.format(missing))
            index = [where[key] for key in self.keys]
        dev = self.stage.device
        same_device = tensor.device.type == dev.type and (dev.index is None or tensor.device.index == dev.index)
        if tensor.dtype is not torch.int32 or not tensor.is_contiguous() or not same_device:
            raise ValueError('BCPlan.run: the widths must be a contiguous int32 tensor on {}'.format(self.stage.device))
        if len(index) != self._created_steps:
            raise ValueError('BCPlan.run: width_index has {} entries, the plan was created with {} steps'.format(
                len(index), self._created_steps))
        if stride < 0 or min(index) < 0 or (self.n_nets - 1) * stride + max(index) >= tensor.numel():
            raise ValueError('BCPlan.run: width_index / width_stride reach outside the {} widths given'.format(tensor.numel()))
        return (tensor, stride, (ctypes.c_int32 * len(index))(*index), 0)

    def _launch(self, signed, per_channel, bits, wargs=None):
        if wargs is not None:
            tensor, stride, index, uniform = wargs
            self._widths_keep = wargs                       # (the device reads the tensor when the stream gets there)
            _ffi.check(_ffi.lib().dfq_bc_plan_run_widths(self._plan, int(bool(signed)), int(bool(per_channel)),
                                                         None if tensor is None else tensor.data_ptr(), stride, index, uniform,
                                                         _ffi.stream_arg()))
        elif per_channel:
            _ffi.check(_ffi.lib().dfq_bc_plan_run_per_channel(self._plan, int(bool(signed)), int(bits), _ffi.stream_arg()))
        else:
            _ffi.check(_ffi.lib().dfq_bc_plan_run(self._plan, int(bool(signed)), _ffi.stream_arg()))

    @property
    def tagged(self):
        """True when the one-launch chain hands values over as tagged 64-bit slots (see dfq_bc_plan_tagged)."""
        return bool(_ffi.lib().dfq_bc_plan_tagged(self._plan))

    @property
    def one_launch(self):
        """True when a tagged run is one launch: min/max blocks woven into the chain launch (dfq_bc_plan_one_launch)."""
        return bool(_ffi.lib().dfq_bc_plan_one_launch(self._plan))

    @property
    def last_run_tagged(self):
        """True when the latest run used the tagged slots (False: counters -- a recorded graph -- or no run yet)."""
        return bool(_ffi.lib().dfq_bc_plan_last_run_tagged(self._plan))

    @property
    def folded_steps(self):
        """Depthwise steps performed by the tail of the step in front of them (dfq_bc_plan_folded)."""
        return int(_ffi.lib().dfq_bc_plan_folded(self._plan))

    @property
    def chain_steps(self):
        """Dependent positions of the correction chain (dfq_bc_plan_chain_steps)."""
        return int(_ffi.lib().dfq_bc_plan_chain_steps(self._plan))

    def status(self):
        """Synchronise and raise if a workgroup of the one-launch chain abandoned its wait (nothing was stored by it)."""
        _ffi.check(_ffi.lib().dfq_bc_plan_status(self._plan, _ffi.stream_arg()))

    def _view(self, addr, n):
        """Copy n floats out of the plan's device scratch (tests / debugging)."""
        out = self.stage.new((n,))
        out.copy_(_RawDeviceBuffer(addr, n, self.stage.device).tensor())
        return out

    def eps(self, step):
        _ffi.synchronize()
        addr = _ffi.lib().dfq_bc_plan_eps(self._plan, step)
        if not addr:
            raise RuntimeError('the quant-error row sums are only materialised by plans created with DFQ_BC_EPS=1 (debug)')
        return self._view(addr, self.step_out_ch[step] * self.step_in[step]).reshape(self.step_out_ch[step], -1)

    def correction(self, step):
        _ffi.synchronize()
        addr = _ffi.lib().dfq_bc_plan_correction(self._plan, step)
        return self._view(addr, self.step_out_ch[step])

    def close(self):
        if self._plan:
            _ffi.lib().dfq_bc_plan_destroy(self._plan)
            self._plan = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _RawDeviceBuffer:
    """Wrap a raw float32 address of the engine's scratch as a torch tensor (read-only use)."""

    def __init__(self, addr, n, device):
        self.addr, self.n, self.device = addr, n, device

    def tensor(self):
        if self.device.type == 'cuda':
            iface = {'shape': (self.n,), 'typestr': '<f4', 'data': (self.addr, False), 'version': 2, 'strides': None}
            holder = type('_Holder', (), {'__cuda_array_interface__': iface})()
            return torch.as_tensor(holder, device=self.device)
        import numpy as np
        buf = (ctypes.c_float * self.n).from_address(self.addr)
        return torch.from_numpy(np.ctypeslib.as_array(buf).copy())


def build_bc_plan_batch(items, targ_type, bn_type=torch.nn.BatchNorm2d, stage=None):
    """One bias-correction plan over several independent networks: ``items`` = [(graph, bottoms), ...]."""
    stage = stage or _ffi.Stage()
    tables = _fast_bc_tables(items, targ_type, bn_type, stage.device)
    if tables is not None and tables.n_steps > 0:
        return BCPlan(tables, None, stage=stage)
    layers, steps = [], []
    for net, (graph, bottoms) in enumerate(items):
        l, s, _ = _bc_tables(graph, bottoms, targ_type, bn_type, base=len(layers), net=net)
        layers += l
        steps += s
    return BCPlan(layers, steps, stage=stage)


def build_bc_plan(graph, bottoms, targ_type, bn_type=torch.nn.BatchNorm2d, stage=None):
    """Walk the graph like dfq.py:194-293 and flatten what each layer's correction needs."""
    stage = stage or _ffi.Stage()
    layers, steps, keys = _bc_tables(graph, bottoms, targ_type, bn_type)
    plan = BCPlan(layers, steps, stage=stage)
    plan.keys = list(keys)
    return plan, keys


def _bc_tables(graph, bottoms, targ_type, bn_type, base=0, net=0, ensure_bias=True):
    """``ensure_bias=False``: the walk alone -- which BatchNorms feed each layer and how they merge -- without giving the layers
    it corrects a zero bias (the sources of the layer sensitivities, ``_nsr_sources``: that reader must not change the network)."""
    keys = [k for k in graph if type(graph[k]) in targ_type]
    index = {k: base + i for i, k in enumerate(keys)}
    bn_module, relu_attached = {}, {}
    steps = []
    pending = None                       # step whose -bias still waits for "the next BN" (bias_prev)
    for key in graph:
        bot = bottoms[key]
        if bot is None or bot[0] == 'Data':
            continue
        node = graph[key]
        if type(node) == bn_type:
            bn_module[key] = node
            relu_attached[key] = False
            if pending is not None:
                assert node.fake_bias.numel() == graph[keys[pending[0] - base]].weight.size(0), \
                    'bias correction: BN after layer has a different channel count'
                pending[2] = node.fake_bias
                pending = None
            continue
        if type(node) == torch.nn.ReLU:
            if bot[0] in bn_module:
                relu_attached[bot[0]] = True
        if type(node) in targ_type:
            bn_list, relu_list, connect_list, _ = find_prev_bn(bn_module, relu_attached, graph, bottoms, bot[:])
            branches = {}
            for i, (bn, bid) in enumerate(bn_list):
                branches.setdefault(bid[0], []).append((bn, bid, relu_list[i], connect_list[i]))
            assert len(branches) == 1, "Error while calculating expectation for bias correction"
            ordered = sorted(list(branches.values())[0], key=lambda e: len(e[1]), reverse=True)   # stable
            srcs = []
            for j, (bn, _, relu, ctype) in enumerate(ordered):
                srcs.append((bn.fake_weight, bn.fake_bias, relu, j > 0 and ctype == 'cat'))
            if ensure_bias:
                _ensure_bias(node)
            step = [index[key], srcs, None, net]
            steps.append(step)
            pending = step
    layers = [(graph[k].weight, graph[k].bias, getattr(graph[k], 'groups', 1)) for k in keys]
    return layers, [tuple(s) for s in steps], [keys[s[0] - base] for s in steps]


def _bc_tables_cached(graph, bottoms, targ_type, bn_type):
    """``_bc_tables`` of one network from the structure template of its architecture (``_bc_template``: the graph walk of
    dfq.py:194-270 done once per distinct graph, the tensors looked up by (graph key, attribute)): what a second call on the
    same architecture -- the next checkpoint, the next model of a service -- pays is the signature and ~250 attribute reads."""
    t = _bc_template(graph, bottoms, targ_type, bn_type)
    mods = [graph[k] for k in t['keys']]
    for li in t['bias_layers']:
        _ensure_bias(mods[li])
    layers = [(m.__dict__['_parameters']['weight'], m.__dict__['_parameters'].get('bias'), getattr(m, 'groups', 1)) for m in mods]

    def at(ref):
        return None if ref is None else _attr(graph[ref[0]], ref[1])
    steps = [(li, [(at(fw), at(fb), relu, cat) for (fw, fb, _, relu, cat) in srcs], at(nxt), 0) for (li, srcs, nxt) in t['steps']]
    return layers, steps, [t['keys'][li] for (li, _, _) in t['steps']]


def _check_width(bits, what):
    """A host-given width of a widths run (BCPlan.run(widths=)): an int in [2, 16]."""
    if isinstance(bits, bool) or not isinstance(bits, int) or not 2 <= bits <= 16:
        raise ValueError('bias correction: the width of {} must be an int in [2, 16], got {!r}'.format(what, bits))


def _check_bits(bits):
    """Bit widths of the per-channel quantisers: an int in [2, 16]."""
    if isinstance(bits, bool) or not isinstance(bits, int) or not 2 <= bits <= 16:
        raise ValueError('per-channel bit width must be an int in [2, 16], got {!r}'.format(bits))


def bias_correction(graph, bottoms, targ_type, bits_weight=8, bn_type=torch.nn.BatchNorm2d, signed=False, per_channel=False,
                    widths=None):
    """Analytic bias correction: b -= eps . E[x], propagated into the next BN's beta~.

    ``bits_weight`` is accepted and ignored -- the reference hard-codes 8 bits (dfq.py:218).
    ``per_channel=True`` (extension): eps is the quant error of a per-output-channel quantiser -- row o quantised with its own
    (min, max) at ``bits_weight`` bits (2..16, else ValueError) -- the error a per-channel int8 deployment makes.
    ``widths`` (extension): an int, or ``{graph key: bits}`` with a width for every corrected layer (the ``'bits'`` entries of
    ``quantize_mixed``'s result, the values of ``NetworkBatch.quantize_mixed``'s ``bits[n]``): eps is the quant error at each
    layer's OWN width, per tensor or per channel -- ``BCPlan.run(widths=)``; ``bits_weight`` is then not used.  ValueError for a
    corrected layer without a width and a width outside [2, 16].
    """
    from collections.abc import Mapping
    if widths is not None and (isinstance(widths, bool) or not isinstance(widths, (int, Mapping))):
        raise ValueError('bias_correction: widths must be None, an int or a mapping key -> int, got {!r}'.format(type(widths)))
    if per_channel and widths is None:
        _check_bits(bits_weight)
    print("Start bias correction")
    with torch.no_grad(), _cache_lock:
        layers, steps, step_keys = _bc_tables_cached(graph, bottoms, targ_type, bn_type)
        if not steps:
            return                                       # no layer behind a BN: nothing to correct (dfq.py:197-199)
        dev = _ffi.target_device()
        scope = _ffi.scoped_stage()
        try:                                             # plan cache, see cross_layer_equalization
            if _PLAN_CACHE_SIZE == 0:
                raise _Uncacheable()
            if scope is not None:
                scope.prefetch([x for (w, b, g) in layers for x in (w, b)] +
                               [x for st in steps for (fw, fb, relu, concat) in st[1] for x in (fw, fb)] + [st[2] for st in steps])
            tk = lambda t: _tensor_key(t, dev, scope)    # noqa: E731
            key = (_env_key(), ('per_channel' if per_channel else 'per_tensor') + ('' if widths is None else '+widths')) + tuple((tk(w), tk(b), g) for (w, b, g) in layers) + tuple(
                (li, tuple((tk(fw), tk(fb), bool(relu), bool(cat)) for (fw, fb, relu, cat) in srcs), tk(nxt)) for (li, srcs, nxt, _) in steps)
        except _Uncacheable:
            key = None
        hit = _cache_get(_bc_plan_cache, key) if key is not None else None
        stage = scope or _ffi.Stage()
        if hit is not None:
            plan_cache_stats['bc_hits'] += 1
            plan = hit[0]
            stage = scope or plan.stage or stage
        else:
            plan_cache_stats['bc_misses'] += 1
            plan = BCPlan(layers, steps, stage=stage)
            plan.keys = list(step_keys)
            if key is not None:
                _cache_put(_bc_plan_cache, key, (plan,))
        try:
            plan.run(signed=signed, check=True, per_channel=per_channel, bits=bits_weight if per_channel else 8, widths=widths)
        except Exception as exc:
            if key is not None:
                _cache_drop(_bc_plan_cache, key)
            else:
                plan.close()
            raise                                     # (an abandoned wait of the one-launch chain was already repeated by BCPlan.run)
        else:
            if key is None:
                plan.close()
        stage.writeback(unchanged=[w for (w, b, g) in layers])      # the correction rewrites biases and BN proxies, never a weight
