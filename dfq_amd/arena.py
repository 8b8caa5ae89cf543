"""A batch of networks of ONE architecture laid out at a fixed stride in one device allocation.

The calibration of a batch binds some 220 tensors per network (weights, biases, the BatchNorm proxies fake_weight /
fake_bias, the cumulative scale vectors): 7 000 addresses for the benchmark's batch of 32, and gathering them -- one
``data_ptr()`` / contiguity / device check per tensor, in Python -- was 20 of the 23 ms that building the two plans of a
batch cost, against 7.6 ms of GPU work for the whole calibration.  ``NetworkBatch`` moves the tensors ONCE, when the batch
is put together (model loading, not calibration), into one allocation in which network n's tensors sit at the same offsets
from ``base + n * stride``; the modules' parameters and buffers are re-pointed at those slots (views, so the models keep
working as before; ``release()`` gives them storages of their own again -- do that before saving or deep-copying a packed
model, because torch pickles and copies a view together with its whole storage).  A plan over the batch is then the tables
of the FIRST network plus one base address per network (``dfq_le_plan_create_replicated`` /
``dfq_bc_plan_create_replicated``, include/dfq_hip.h): no per-tensor host work at all.

This is the host side of the reference's per-network graph walks (dfq.py:78-82, :194-270) for a batch; the arithmetic is the
engine's, unchanged -- the plans a NetworkBatch creates are the plans ``build_le_plan_batch`` / ``build_bc_plan_batch``
would create over the same tensors (tests/test_arena.py).  ``quant_plan`` is the batch form of ``quantize_targ_layer``
(layer_transform.py:279-296, main_cls.py:178-181): one plan, one or two launches for every network of the batch, the
integer codes and ranges in two caller-visible blocks (tests/test_batch_quant.py).  ``absorb_plan`` is the batch form of the
two optional steps between equalisation and correction, ``bias_absorption`` (dfq.py:121-164) and ``clip_weight``
(dfq.py:167-170): two launches for the whole batch, every weight read once (tests/test_batch_absorb.py).
``act_range_plan`` is the batch form of ``set_quant_minmax`` (layer_transform.py:347-609, main_cls.py:188), the analytic
activation ranges: the graph walk both share (``utils.layer_transform._act_program``; this module holds no walk of its own)
is made once, on network 0, and one launch (two with a conv / linear without BatchNorm in front of a quantiser) fills one
block of packed (min, max) pairs the quantisers are then pointed at (tests/test_batch_act.py).  With them the default
calibration sequence main_cls.py:149-190 runs on a batch as le_plan -> absorb_plan -> bc_plan -> quant_plan ->
act_range_plan.  ``NetworkBatch.from_unfolded`` takes the networks as they are loaded, BatchNorm not yet folded, and
``fold_plan`` is the batch form of ``merge_batchnorm`` (layer_transform.py:231-276, main_cls.py:149): the pairs are found
once, on network 0, by the walk merge_batchnorm itself uses (``utils.layer_transform._fold_pairs``), the BatchNorm vectors get
slots behind those of the ordinary layout, and two launches fold every network (tests/test_batch_fold.py).  The sequence then
starts with fold_plan: fold_plan -> le_plan -> absorb_plan -> bc_plan -> quant_plan -> act_range_plan.
``table_plan`` is the batch form of the last step of the reference's OTHER driver, convert_ncnn.py:106-201, whose product is
the int8 calibration table ncnn2int8 takes (``ncnn_table``; convert_ncnn.py:178-201): one read of every weight of every
network gives each tensor's (min, max) and each output row's max|w|, and ``calibration_tables`` formats them, with the
activation ranges, into one table per network (tests/test_batch_table.py).  That driver then runs on a batch as
fold_plan -> le_plan().run(signed=True) -> absorb_plan(absorb=False, range_clip=...) -> bc_plan().run(signed=True) ->
act_range_plan -> calibration_tables.
``error_plan`` is the batch form of the reference's quality signal, ``_quantize_error(param, num_bits, reduction, signed)``
(dfq.py:8-25), which both of its drivers import: three launches read every weight of every network twice, write none, and
leave per weight the float64 sums of w^2 and of e, |e|, e^2 for one to four quantiser configurations, e = Q(w) - w being bit
for bit what ``quant_plan`` would store minus w; ``quantize_error`` turns them into the reference's 'sum' and 'mean', the mean
squared error and the SQNR (tests/test_batch_error.py).  It changes nothing, so it can stand anywhere in the sequence -- in
front of ``le_plan`` and behind it shows what equalisation bought.
``clip_plan`` acts on that signal: per tensor or per output row it searches the one of K ranges, shrunk from the unit's
(min, max), under which the quantiser has the least sum e^2, and clamps the weights to it -- ``clip_weight`` (dfq.py:167-170)
with a searched bound, standing where ``absorb_plan(range_clip=...)`` clips: fold_plan -> le_plan -> absorb_plan -> clip_plan
-> bc_plan -> quant_plan -> act_range_plan.  A unit's own (min, max) is then the chosen range, so the plans behind it are
unchanged (tests/test_batch_clip.py).
With a width per layer the correction has to see the widths, so the allocation comes first and the quantisation last:
fold_plan -> le_plan -> absorb_plan -> clip_plan -> mixed_plan(apply=False) -> bc_plan.run(widths=) -> mixed_plan ->
act_range_plan; ``bc_plan().run(widths=that plan)`` reads every (network, layer)'s width on the device, where the allocation
left it, and ``quantize_mixed(correct=True)`` is the three steps and the biases in one call (tests/test_bc_widths.py).
``pack_plan`` packs the codes a ``quant_plan``, ``squant_plan`` or ``mixed_plan`` wrote densely, every tensor of every network at
its own width (read on the device), ``unpack_plan`` rebuilds codes and weights from the packed words, and ``save_packed`` /
``load_packed`` put a quantised batch into one ``.npz`` and back (tests/test_batch_pack.py).
``nsr_plan`` gives the allocation a cost that knows the layer: every output channel's expected noise-to-signal ratio at every
candidate width, from the weights and the BatchNorm proxies in front of the layer (the sources of the bias-correction walk);
``mixed_plan(costs=that plan)`` and ``quantize_mixed(cost='nsr')`` allocate on it: nsr_plan -> mixed_plan(apply=False, costs=)
-> bc_plan.run(widths=) -> mixed_plan(costs=) (tests/test_batch_nsr.py).
"""
from __future__ import annotations

import ctypes
import math
from collections import OrderedDict

import numpy as np
import torch

from . import _ffi
from . import dfq as _dfq
from . import ncnn_table as _ncnn
from .utils.layer_transform import _WalkError, _act_program, _ensure_bias, _fold_pairs

_ALIGN = 64            # floats: every tensor starts on a 256-byte boundary (vector loads, the alignment hipMalloc gives)
_BN_VECTORS = ('weight', 'bias', 'running_mean', 'running_var')      # of a BatchNorm that fold_plan folds


def _rebind(mod, name, view):
    """point a module's parameter / buffer / plain tensor attribute at `view` (same values, new storage)"""
    prm = mod.__dict__['_parameters']
    if prm.get(name) is not None:
        prm[name].data = view
    elif name in mod.__dict__['_buffers']:
        mod.__dict__['_buffers'][name] = view
    else:
        setattr(mod, name, view)


class NetworkBatch:
    """``nets``: list of (graph, bottoms, relations) of networks with the same graph (keys, node types, tensor shapes,
    relation triples), BatchNorm already folded (``merge_batchnorm``) and relations created, tensors float32 on the target
    device.  After construction every tensor the equalisation and the bias correction touch lives in ``self.storage``.
    ``NetworkBatch.from_unfolded`` takes networks whose BatchNorm is still to be folded; ``self.folded`` says which state
    the batch is in, ``self.offsets`` where every slot lies."""

    def __init__(self, nets, targ_type, bn_type=torch.nn.BatchNorm2d, stage=None):
        self._layout(nets, targ_type, bn_type, stage, None)

    @classmethod
    def from_unfolded(cls, nets, targ_type, bn_type=torch.nn.BatchNorm2d, stage=None):
        """A batch of networks whose BatchNorm has NOT been folded yet: ``nets`` as for the constructor, the relations created
        on the unfolded graph (``create_relation`` reads no tensor).  The (layer, BatchNorm) pairs ``merge_batchnorm`` would
        fold are found on network 0 (``_fold_pairs``); every folded layer gets its bias, every folded BatchNorm its
        ``fake_weight`` / ``fake_bias`` buffers (contents irrelevant until the fold), the ordinary layout is made, and the
        BatchNorm vectors get slots behind it.  The batch is ``folded == False`` until ``fold_plan().run()`` /
        ``merge_batchnorm()``; the other plans raise RuntimeError until then.  ValueError, before anything is touched and
        naming the graph key: a BatchNorm that already has proxies (it has been folded: use the constructor), one without
        running statistics or affine parameters, a layer two BatchNorms claim, networks whose pairs or ``eps`` differ from
        network 0's, a tensor of a pair that is not float32 on the batch's device."""
        nets = list(nets)
        if not nets:
            raise ValueError('NetworkBatch: no networks')
        stage = stage or _ffi.Stage()
        dev = stage.device
        who = 'NetworkBatch.from_unfolded'
        g0, b0, _ = nets[0]
        pairs = _fold_pairs(g0, b0, targ_type)
        claimed = {}
        for lk, bk in pairs:
            if lk in claimed:
                raise ValueError('{}: layer {} is claimed by two BatchNorms ({} and {}): one launch cannot order two folds of '
                                 'one weight'.format(who, lk, claimed[lk], bk))
            claimed[lk] = bk
        eps0 = [g0[bk].eps for _, bk in pairs]
        for n, (graph, bottoms, _) in enumerate(nets):
            mine = _fold_pairs(graph, bottoms, targ_type) if n else pairs
            if mine != pairs:
                odd = next((q for q in mine if q not in pairs), None) or next(q for q in pairs if q not in mine)
                raise ValueError('{}: network {} does not fold the pairs of network 0 (BatchNorm {} behind layer {})'.format(
                    who, n, odd[1], odd[0]))
            for (lk, bk), eps in zip(pairs, eps0):
                layer, bn = graph[lk], graph[bk]
                if _dfq._attr(bn, 'fake_weight') is not None or _dfq._attr(bn, 'fake_bias') is not None:
                    raise ValueError('{}: BatchNorm {} of network {} already has fake_weight / fake_bias: it has been folded '
                                     '(use the constructor)'.format(who, bk, n))
                if bn.eps != eps:
                    raise ValueError('{}: BatchNorm {} of network {} has eps {!r}, network 0 has {!r}'.format(who, bk, n, bn.eps, eps))
                tensors = [(lk, 'weight', layer.weight), (lk, 'bias', layer.bias)]
                for name in _BN_VECTORS:
                    t = _dfq._attr(bn, name)
                    if t is None:
                        raise ValueError('{}: BatchNorm {} of network {} has no {} (a folded BatchNorm needs running statistics '
                                         'and affine parameters)'.format(who, bk, n, name))
                    if t.numel() != layer.weight.shape[0]:
                        raise ValueError('{}: {} of BatchNorm {} of network {} has {} channels, layer {} has {}'.format(
                            who, name, bk, n, t.numel(), lk, layer.weight.shape[0]))
                    tensors.append((bk, name, t))
                for key, name, t in tensors:
                    if t is not None and (t.dtype is not torch.float32 or t.device != dev):
                        raise ValueError('{}: {} of {} of network {} is {} on {}; the batch wants float32 on {}'.format(
                            who, name, key, n, t.dtype, t.device, dev))
        for graph, _, _ in nets:
            for lk, bk in pairs:
                _ensure_bias(graph[lk])                                 # layer_transform.py:253-254
                bn = graph[bk]
                c = bn.weight.numel()
                bn.register_buffer('fake_weight', torch.empty(c, dtype=torch.float32, device=dev))     # :264-265; filled by the fold
                bn.register_buffer('fake_bias', torch.empty(c, dtype=torch.float32, device=dev))
        self = cls.__new__(cls)
        self._layout(nets, targ_type, bn_type, stage, pairs)
        return self

    def _layout(self, nets, targ_type, bn_type, stage, fold):
        """what the constructor does; ``fold``: the (layer key, BatchNorm key) pairs of a batch that is still to be folded,
        whose BatchNorm vectors (and proxies no table refers to) get slots BEHIND the ordinary ones"""
        if not nets:
            raise ValueError('NetworkBatch: no networks')
        self.stage = stage or _ffi.Stage()
        dev = self.stage.device
        self.nets = list(nets)
        self.targ_type, self.bn_type = targ_type, bn_type
        g0, b0, r0 = self.nets[0]
        le_t = _dfq._le_template(g0, r0, targ_type)
        bc_t = _dfq._bc_template(g0, b0, targ_type, bn_type)
        need_bias = sorted(set(le_t['firsts']) | set(bc_t['bias_layers']))
        # (graph key, attribute) of every BatchNorm proxy a table refers to, in first-use order
        bn_refs, seen = [], set()

        def add(ref):
            if ref is not None and ref not in seen:
                seen.add(ref)
                bn_refs.append(ref)
        for (_, _, kb) in le_t['rel']:
            if kb is not None:
                add((kb, 'fake_weight'))
                add((kb, 'fake_bias'))
        for _, ref in bc_t['step_next']:
            add(ref)
        for _, ref in bc_t['src_fw']:
            add(ref)
        for _, ref in bc_t['src_fb']:
            add(ref)

        def slots_of(graph, bottoms, relations):
            """[(setter, tensor or None, numel)] of one network in slot order; None = a scale vector still to be created"""
            if _dfq._le_template(graph, relations, targ_type) is not le_t or _dfq._bc_template(graph, bottoms, targ_type, bn_type) is not bc_t:
                raise ValueError('NetworkBatch: the networks of a batch must share one architecture (graph keys, node types, '
                                 'tensor shapes, relations)')
            mods = [graph[k] for k in le_t['keys']]
            for i in need_bias:
                _ensure_bias(mods[i])                                   # dfq.py:91-92, layer_transform.py:253-254
            out = []
            for m in mods:
                prm = m.__dict__['_parameters']
                out.append((m, 'weight', prm['weight']))
                if prm.get('bias') is not None:
                    out.append((m, 'bias', prm['bias']))
            for (key, name) in bn_refs:
                t = _dfq._attr(graph[key], name)
                if t is not None:
                    out.append((graph[key], name, t))
            for rr, o1 in zip(relations, le_t['o1']):
                out.append((rr, 'S', rr.S if rr.S is not None else o1))
            return out

        def fold_slots_of(graph):
            """the slots of an unfolded batch behind the ordinary ones: the four vectors of every folded BatchNorm and those
            of its proxies that no LE / BC table refers to"""
            out = []
            for _, bk in fold or ():
                bn = graph[bk]
                for name in _BN_VECTORS + tuple(nm for nm in ('fake_weight', 'fake_bias') if (bk, nm) not in seen):
                    out.append((bn, name, _dfq._attr(bn, name)))
            return out

        per_net = [slots_of(*net) for net in self.nets]
        n_ordinary = len(per_net[0])
        per_net = [slots + fold_slots_of(net[0]) for slots, net in zip(per_net, self.nets)]
        numel = [t.numel() if torch.is_tensor(t) else int(t) for (_, _, t) in per_net[0]]
        for n, slots in enumerate(per_net):
            if [t.numel() if torch.is_tensor(t) else int(t) for (_, _, t) in slots] != numel:
                raise ValueError('NetworkBatch: network {} does not have the tensors of network 0'.format(n))
            for (_, name, t) in slots:
                if torch.is_tensor(t) and (t.dtype is not torch.float32 or t.device != dev):
                    raise ValueError('NetworkBatch: {} of network {} is {} on {}; the batch wants float32 on {}'.format(
                        name, n, t.dtype, t.device, dev))
        offs, total = [], 0
        for c in numel:
            offs.append(total)
            total += -(-c // _ALIGN) * _ALIGN
        self.stride = total                                            # floats per network
        self.offsets = offs                                            # of every slot, floats from a network's base
        self.storage = torch.empty(len(self.nets) * total, dtype=torch.float32, device=dev)
        rows = self.storage.view(len(self.nets), total)
        srcs, dsts = [], []
        with torch.no_grad():
            for n, slots in enumerate(per_net):
                row = rows[n]
                for (owner, name, t), off, c in zip(slots, offs, numel):
                    if torch.is_tensor(t):
                        view = row[off:off + c].view(t.shape)
                        srcs.append(t.detach())
                        dsts.append(view)
                    else:
                        view = row[off:off + c]
                        view.fill_(1.0)                                # Relation.S starts at 1 (relation.py:11)
                    if name == 'S':
                        owner.S = view
                    else:
                        _rebind(owner, name, view)
            if srcs:
                torch._foreach_copy_(dsts, srcs)
        self.slots_per_network = len(numel)
        self.bases = (np.uint64(self.storage.data_ptr()) + np.arange(len(self.nets), dtype=np.uint64) * np.uint64(4 * total))
        # the first network's tables (absolute addresses inside its slot); every plan of this batch starts from them
        self._le = _dfq._fast_le_tables([(g0, r0)], targ_type, dev)
        self._bc = _dfq._fast_bc_tables([(g0, b0)], targ_type, bn_type, dev)
        lo, hi = int(self.bases[0]), int(self.bases[0]) + 4 * total
        for T in (self._le, self._bc):
            if T is None:
                raise RuntimeError('NetworkBatch: the tables of the first network could not be built')
            for a in T.arrays.values():
                for field in (a.dtype.names or ()):
                    if a.dtype[field] == np.uint64:
                        p = a[field][a[field] != 0]
                        if len(p) and (p.min() < lo or p.max() >= hi):
                            raise RuntimeError('NetworkBatch: a table of the first network points outside its slot ({})'.format(field))
        self._base_ints = [int(v) for v in self.bases]
        self._scale_cum = [rr.S for (_, _, rels) in self.nets for rr in rels]
        # first weight, last relation of every network (None: a network without relations, ReLU6 kept, has no scale vectors)
        self._probe = [(slots[0][2], slots[n_ordinary - 1][0] if r0 else None) for slots in per_net]
        self._act_bound = {}                  # id -> (quantiser module, range block) of every BatchActRangePlan.bind_quantisers
        self._fold = fold                     # None: the networks came folded
        self.folded = not fold                # False until fold_plan().run(): the proxies hold nothing yet

    def release(self):
        """Give every tensor a storage of its own again (a copy of its slot) and drop the batch allocation.  The models' tensors
        are VIEWS of ``self.storage`` while the batch exists, and torch treats a view as its whole storage when it pickles or
        deep-copies one: ``torch.save(model.state_dict())`` / ``copy.deepcopy(model)`` of a packed model would carry all the
        batch's networks.  Call this when the calibration is done and the models go their own ways; plans created from the batch
        must not be run afterwards."""
        home = self.storage.untyped_storage().data_ptr()

        def mine(t):
            return torch.is_tensor(t) and t.untyped_storage().data_ptr() == home
        with torch.no_grad():
            for (graph, bottoms, relations) in self.nets:
                for m in graph.values():
                    if not isinstance(m, torch.nn.Module):
                        continue                                    # functional nodes of the graph are recorded by name
                    for name, t in m.__dict__['_parameters'].items():
                        if mine(t):
                            t.data = t.data.clone()
                    bufs = m.__dict__['_buffers']
                    for name in list(bufs):
                        if mine(bufs[name]):
                            bufs[name] = bufs[name].clone()
                    for name, t in list(m.__dict__.items()):
                        if mine(t):
                            m.__dict__[name] = t.clone()
                for rr in relations:
                    if mine(rr.S):
                        rr.S = rr.S.clone()
            # quantisers bound to the range block of an act_range_plan: that block is a second home allocation
            for q, block in self._act_bound.values():
                bufs = q.__dict__['_buffers']
                there = block.untyped_storage().data_ptr()
                mn, mx = bufs.get('running_min'), bufs.get('running_max')
                if not (torch.is_tensor(mn) and torch.is_tensor(mx) and mn.untyped_storage().data_ptr() == there
                        and mx.untyped_storage().data_ptr() == there):
                    continue                                        # somebody has given it other buffers since
                pair = torch.cat([mn.reshape(1), mx.reshape(1)])    # stays the packed pair QuantMeasure._packed_range looks for
                bufs['running_min'], bufs['running_max'] = pair[0:1], pair[1:2]
        self._act_bound = {}
        self._probe, self._scale_cum = [], []
        self.storage = None

    # -- plans ---------------------------------------------------------------------------------------------------------
    def _in_slot(self, key, name, t):
        """address of `t`, a tensor of network 0: a batch plan finds network n's copy at that address + bases[n] - bases[0],
        so t has to lie in network 0's slot"""
        lo, p = self._base_ints[0], t.data_ptr()
        if not (t.dtype is torch.float32 and t.is_contiguous() and lo <= p and p + 4 * t.numel() <= lo + 4 * self.stride):
            raise RuntimeError('NetworkBatch: {} of {} in network 0 no longer lives in its slot of the batch allocation'.format(
                name, key))
        return p

    def _tables(self, T):
        out = _dfq._Tables()
        out.arrays = T.arrays
        out.n_layers = T.n_layers
        out.keep = [self]
        out.bases = self.bases
        out.mutable = [self.storage]          # one allocation holds every tensor the plans rewrite: a snapshot is ONE copy
        return out

    def check(self, thorough=False):
        """Raise if a tensor has left its slot (someone assigned a new tensor to ``weight.data`` or ``Relation.S`` after the
        batch was put together).  The quick form looks at the first and the last slot of every network."""
        if self.storage is None:
            raise RuntimeError('NetworkBatch: the batch has been released')
        span = 4 * self.stride
        for n, ((w, rr), base) in enumerate(zip(self._probe, self._base_ints)):
            if w.data_ptr() != base or (rr is not None and (rr.S is None or not (base <= rr.S.data_ptr() < base + span))):
                raise RuntimeError('NetworkBatch: a tensor of network {} no longer lives in the batch allocation'.format(n))
        if thorough:
            for n, (g, b, r) in enumerate(self.nets):
                le = _dfq._fast_le_tables([(g, r)], self.targ_type, self.stage.device)
                bc = _dfq._fast_bc_tables([(g, b)], self.targ_type, self.bn_type, self.stage.device)
                for T, T0 in ((le, self._le), (bc, self._bc)):
                    for key, a in T.arrays.items():
                        for field in (a.dtype.names or ()):
                            if a.dtype[field] == np.uint64:
                                want = T0.arrays[key][field].copy()
                                want[want != 0] += self.bases[n] - self.bases[0]
                                if not np.array_equal(a[field], want):
                                    raise RuntimeError('NetworkBatch: {} of network {} is not where the batch put it'.format(field, n))

    def _ready(self, who):
        """check(), and RuntimeError for a batch from_unfolded made that has not been folded yet"""
        self.check()
        if not self.folded:
            raise RuntimeError('NetworkBatch: {} on a batch whose BatchNorm has not been folded yet (fold_plan().run() or '
                               'merge_batchnorm() first)'.format(who))

    def fold_plan(self):
        """One plan (BatchFoldPlan) for ``merge_batchnorm(model, graph, bottoms, targ_type)`` on every network of a batch
        made by ``from_unfolded``, bit for bit: two launches.  RuntimeError on a batch made by the constructor (its networks
        came folded) and for a tensor of network 0 that has left its slot.  The plan runs once: ``run()`` sets
        ``self.folded`` and raises RuntimeError on a folded batch."""
        self.check()
        if self._fold is None:
            raise RuntimeError('NetworkBatch: fold_plan on a batch of folded networks (NetworkBatch.from_unfolded takes unfolded ones)')
        return BatchFoldPlan(self)

    def merge_batchnorm(self):
        """fold_plan + run + synchronise + close, then ``eps = 1e-12`` on every folded BatchNorm (what merge_batchnorm sets,
        utils/layer_transform.py): afterwards every network is in the state ``merge_batchnorm`` leaves it in."""
        plan = self.fold_plan()
        try:
            plan.run()
            _ffi.synchronize()
        finally:
            plan.close()
        for graph, _, _ in self.nets:
            for _, bk in self._fold:
                graph[bk].eps = 1e-12

    def le_plan(self):
        """One equalisation plan over the whole batch (LEPlan): the first network's tables + a base address per network."""
        self._ready('le_plan')
        t = self._tables(self._le)
        t.n_relations, t.scale_cum = self._le.n_relations, self._scale_cum
        return _dfq.LEPlan(t, None, stage=self.stage)

    def bc_plan(self):
        """One bias-correction plan over the whole batch (BCPlan)."""
        self._ready('bc_plan')
        t = self._tables(self._bc)
        t.n_steps, t.n_sources = self._bc.n_steps, self._bc.n_sources
        t.step_out_ch, t.step_in = self._bc.step_out_ch, self._bc.step_in
        t.step_keys = list(self._bc.step_keys)               # run(widths=mixed_plan) finds every step's width by its graph key
        return _dfq.BCPlan(t, None, stage=self.stage)

    def quant_plan(self, bit_weight=8, bits_bias=16, per_channel=False, signed=False, codes=None):
        """One weight-quantisation plan over the whole batch (BatchQuantPlan): what ``quantize_targ_layer(graph, bit_weight,
        bits_bias, targ_type, per_channel=, signed=)`` does to each network -- every targ_type layer's weight (per tensor, or
        per output row with ``per_channel``; ``signed``: the symmetric recipe) and its bias unless ``bits_bias == 32`` (per
        tensor, asymmetric) -- bit for bit.  ``codes``: None, 'int32' or 'int8' (uint8 for asymmetric weights, int8 for signed
        ones; bit_weight <= 8): the weights' integer codes land in a block of the plan (``codes(n)``), every range in another
        (``ranges(n)``).  Bit widths are taken as quantize_targ_layer takes them: per tensor through ``int()`` (8.0 is 8), the
        bias skipped when ``bits_bias >= 32``; per channel integers in [2, 16] only.  Where quantize_targ_layer would fail
        inside the library (a per-tensor width outside [1, 30]) this raises ValueError up front.  Every tensor of network 0
        must still lie in its slot of the batch allocation (RuntimeError otherwise: the plan writes every network at network
        0's addresses moved by a fixed offset)."""
        self._ready('quant_plan')
        return BatchQuantPlan(self, bit_weight, bits_bias, per_channel, signed, codes)

    def quantize(self, bit_weight=8, bits_bias=16, per_channel=False, signed=False, codes='int32'):
        """quant_plan + run + synchronise: returns (codes, ranges), lists of one dict per network (``codes=None``: empty
        dicts)."""
        plan = self.quant_plan(bit_weight, bits_bias, per_channel, signed, codes)
        try:
            plan.run()
            _ffi.synchronize()
            n = len(self.nets)
            return [plan.codes(i) for i in range(n)], [plan.ranges(i) for i in range(n)]
        finally:
            plan.close()

    def squant_plan(self, bit_weight=8, per_channel=False, signed=False, codes=None, widths=None):
        """One adaptive-rounding plan over the weights of the whole batch (BatchSquantPlan; SQuant, "Adaptive rounding" in
        include/dfq_hip.h): the ranges and the quantisation grid are ``quant_plan``'s (per tensor, or per output row with
        ``per_channel``; ``signed``: the symmetric recipe), but of the roundings to nearest the few that cost least are flipped
        so that the rounding errors of every kH x kW kernel and of every output row sum to at most half a quantum -- what
        ``quantize_targ_layer(..., rounding='squant')`` does to each network, bit for bit.  Weights only; ``bit_weight`` is an
        integer in [2, 16] in both range modes.  ``codes``: None, 'int32' or 'int8' as in ``quant_plan``.  The plan exposes
        ``codes(n)``, ``ranges(n)`` and ``stats(n)``.  ValueError for a layer whose rows are longer than
        dfq_squant_max_row_len().

        ``widths``: every layer at a width of its own.  A BatchMixedPlan of this batch with the same ``per_channel`` and
        ``signed`` (ValueError otherwise, as for a closed plan, or 'int8' codes with a candidate width above 8): the width of
        every (network, layer) is read on the device from its ``bits_block`` (dfq_batch_squant_plan_set_widths), so
        ``mixed.run()`` -- or ``allocate()`` -- and ``run()`` of this plan go onto the stream back to back; ``bit_weight`` is then
        not used, and ``status(n)`` is 2 where a width on the device was no width (that layer is left as it was).  Or a dict
        ``key -> int in [2, 16]`` (ValueError for another value, an unknown key, 'int8' codes with a width above 8): the widths
        go into the plan's table, layers without an entry get ``bit_weight``.  Either way the result is, bit for bit, what
        ``squant_plan(that width)`` stores for that layer, and ``pack_plan`` packs every layer at its width.  The allocation of
        a mixed plan walks on the errors of NEAREST rounding; adaptive rounding trades a slightly larger sum e^2 for bounded
        row sums, so the widths are the nearest-rounding optimum, not this rounding's."""
        self._ready('squant_plan')
        return BatchSquantPlan(self, bit_weight, per_channel, signed, codes, widths)

    def quantize_squant(self, bit_weight=8, bits_bias=16, per_channel=False, signed=False, codes='int32'):
        """squant_plan for the weights, the nearest rounding of ``quantize`` for the biases (unless ``bits_bias >= 32``), run
        + synchronise: returns (codes, ranges) like ``quantize`` -- the biases' ranges under key + '.bias' -- and every bias
        bit for bit what ``quantize`` stores."""
        self._ready('quantize_squant')
        g0 = self.nets[0][0]
        tt = tuple(self.targ_type)
        plans = [BatchSquantPlan(self, bit_weight, per_channel, signed, codes)]
        try:
            if bits_bias < 32 and any(type(l) in tt and l.bias is not None for l in g0.values()):
                plans.append(BatchQuantPlan(self, bit_weight, bits_bias, per_channel, signed, None, _biases_only=True))
            for plan in plans:
                plan.run()
            _ffi.synchronize()
            n = len(self.nets)
            ranges = []
            for i in range(n):
                r = {}
                for plan in plans:
                    r.update({k: v.clone() for k, v in plan.ranges(i).items()})
                ranges.append(r)
            return [{k: v.clone() for k, v in plans[0].codes(i).items()} for i in range(n)], ranges
        finally:
            for plan in plans:
                plan.close()

    def mixed_plan(self, widths=(2, 3, 4, 6, 8), avg_bits=None, budget_bits=None, per_channel=False, signed=False, sensitivity=None,
                   pin=None, codes=None, apply=True, costs=None, clip=None, alpha_min=0.5):
        """One mixed-precision plan over the weights of the whole batch (BatchMixedPlan): every ``targ_type`` weight of every
        network gets a width of its own out of ``widths`` (rising ints in [2, 16], two to eight of them) so that the network
        takes at most ``budget_bits`` bits -- or, with ``avg_bits``, floor(avg_bits * number of weights), computed exactly;
        exactly one of the two is given, and the budget is the same for every network -- and the sum over the layers of
        ``sensitivity[key]`` (default 1) times the layer's sum of squared quantisation errors is least: the greedy walk the
        comment of dfq_batch_mixed_plan_create (include/dfq_hip.h) defines, run on the device per network.  ``pin[key]`` fixes
        a layer's width (one of ``widths``).  With ``apply`` every weight is then quantised in place at its width, bit for bit
        as ``quant_plan(bit_weight=that width, per_channel=, signed=)`` would; ``apply=False`` only allocates.  ``codes``:
        None, 'int32' or 'int8' (widths <= 8) as in ``quant_plan``.  The plan exposes ``bits(n)``, ``errors(n)``, ``used(n)``,
        ``cost(n)``, ``ranges(n)`` and ``codes(n)``.  Weights only.  ValueError for what create would refuse; RuntimeError
        for a weight of network 0 that has left its slot.

        ``costs``: a BatchNsrPlan of this batch with the same ``widths``, ``per_channel`` and ``signed`` (ValueError otherwise).
        The allocation then weighs ``sensitivity[key]`` times the layer's summed noise-to-signal ratio (``nsr_plan``) in place of
        its sum e^2, read on the device from that plan's ``cost_block`` -- run it first, on the same stream; ``errors(n)`` is
        still the sum e^2, ``cost(n)`` the sum of the weighed costs at the chosen widths.  A BatchMxPlan of this batch is taken
        the same way -- its ``cost_block`` holds the MX sum e^2 of every layer at every width --, and only its ``widths`` tuple is
        compared: an MX grid has no ``per_channel`` or ``signed`` (``mx_plan``, ``quantize_mx``).

        ``clip``: None for the plan above through its own entry point, or K, an int in [1, 64]: the clip-aware plan
        (dfq_batch_mixed_plan_create_clipped).  The MSE-optimal clip of every unit -- a tensor, or an output row with
        ``per_channel`` -- is searched among K candidates down to ``alpha_min`` (in (0, 1]) times the range at EVERY width, bit
        for bit what ``clip_plan(that width, ..., candidates=K, alpha_min=)`` finds; the allocation walks on the errors of the
        clipped ranges, and with ``apply`` every layer is clamped and quantised at its own width and that width's range, bit
        for bit ``clip_plan(width, apply=True)`` then ``quant_plan(width)``.  ``ranges(n)`` is then the chosen width's (l, h);
        ``clip_ranges(n)``, ``clip_chosen(n)`` and ``unit_errors(n)`` hold every width's, in ``clip_range_block`` float32
        [n_nets, units, B, 2], ``clip_chosen_block`` int32 and ``unit_error_block`` float64 [n_nets, units, B].  At most 512
        (width, candidate) pairs.  ``run(stages)`` / ``allocate()`` / ``clamp()`` / ``quantise()`` run the stages one by one."""
        self._ready('mixed_plan')
        return BatchMixedPlan(self, widths, avg_bits, budget_bits, per_channel, signed, sensitivity, pin, codes, apply, costs, clip, alpha_min)

    def nsr_plan(self, widths=(2, 3, 4, 6, 8), per_channel=False, signed=False, moment='variance', input_moment=1.0):
        """One plan (BatchNsrPlan) for the data-free sensitivities ``mixed_plan(costs=)`` allocates on: for every ``targ_type``
        weight of every network and every width of ``widths``, the sum over the output channels of the expected
        noise-to-signal power ratio -- the quantisation error e^2 and the weight w^2 of every element weighed by the moment of
        the input channel it reads, which comes from the BatchNorm proxies in front of the layer (the sources of the
        bias-correction walk; dfq_batch_nsr_plan_create in include/dfq_hip.h holds the definition).  ``moment``: 'variance'
        (what is left once bias correction has removed the mean term) or 'second_moment'; ``input_moment`` stands for the
        channels of a layer fed by the data.  Nothing of the networks is written, no layer gets a bias.  The plan exposes
        ``costs(n)``, ``rows(n)``, ``moments(n)`` and the blocks behind them."""
        self._ready('nsr_plan')
        return BatchNsrPlan(self, widths, per_channel, signed, moment, input_moment)

    def quantize_mixed(self, widths=(2, 3, 4, 6, 8), avg_bits=None, budget_bits=None, per_channel=False, signed=False, sensitivity=None,
                       pin=None, codes='int32', bits_bias=16, correct=False, cost='mse', moment='variance', input_moment=1.0,
                       clip=None, alpha_min=0.5, rounding='nearest'):
        """mixed_plan for the weights, the nearest rounding of ``quantize`` for the biases (unless ``bits_bias >= 32``), run +
        synchronise: returns (codes, ranges, bits), each a list of one dict per network -- the biases' ranges under
        key + '.bias', every bias bit for bit what ``quantize`` stores, ``bits[n][key]`` the width network n's layer got.

        ``correct=True`` puts the analytic bias correction between the allocation and the quantisation, at the widths the
        allocation chose: an allocating plan (``apply=False``), ``bc_plan().run(signed=, per_channel=, widths=that plan)`` --
        the widths are read on the device, where the allocation left them -- then the applying plan and the biases, which are
        quantised AFTER their correction, as the reference orders the two (main_cls.py:176-181).  The correction writes no
        weight, so the applying plan allocates what the first one did.  Everything stays on the stream until the one
        synchronisation at the end.

        ``cost='nsr'`` allocates on ``nsr_plan(widths, per_channel, signed, moment, input_moment)``, created and run first.  With
        ``correct`` the order is nsr -> allocation -> correction -> applying plan on the SAME cost block: the correction moves
        beta~ of later BatchNorms, so the costs are not computed again.

        ``clip=K`` (``alpha_min``): ONE clip-aware plan (``mixed_plan(clip=K, alpha_min=)``) in place of the plans above.  Without
        ``correct`` it is run, then the biases as above.  With ``correct`` its stages are run one by one: ALLOCATE, CLAMP,
        ``bc_plan().run(widths=that plan)`` -- which reads the widths on the device and sees the clamped weights, as the
        correction behind ``clip_weight`` always has --, QUANTISE, then the biases after their correction; no second
        allocation is run (it would see clamped weights and could differ).  With ``cost='nsr'`` the nsr plan runs first, on the
        unclamped weights, and the allocation walks on it; the ranges are still the sum-e^2-optimal ones.  ``clip=None`` is
        the code path above, unchanged.

        ``rounding='squant'`` rounds adaptively (``squant_plan``) at the allocated widths: the allocating plan (``apply=False``;
        with ``clip=K`` the clipped plan's ALLOCATE and CLAMP stages), then ``squant_plan(widths=that plan, codes=)``, which reads
        the widths on the device, then the biases as ``quantize_squant`` does them.  On clamped weights the squant plan's own
        (min, max) is the chosen (l, h) in value.  ``ranges`` are the squant plan's.  The allocation still walks on
        nearest-rounding errors (``squant_plan``).  ``correct=True`` is a ValueError here: the analytic correction models nearest
        rounding; correct empirically with ``bias_correction_distill``.  ``rounding='nearest'`` is the code
        path above, unchanged; anything else is a ValueError."""
        self._ready('quantize_mixed')
        if cost not in ('mse', 'nsr'):
            raise ValueError("quantize_mixed: cost must be 'mse' or 'nsr', got {!r}".format(cost))
        if rounding not in ('nearest', 'squant'):
            raise ValueError("quantize_mixed: rounding must be 'nearest' or 'squant', got {!r}".format(rounding))
        if rounding == 'squant' and correct:
            raise ValueError("quantize_mixed: correct=True models nearest rounding and does not go with rounding='squant'; "
                             'correct the rounded networks with bias_correction_distill')
        g0 = self.nets[0][0]
        tt = tuple(self.targ_type)
        plans, first = [], []
        try:
            nsr = None
            if cost == 'nsr':
                nsr = BatchNsrPlan(self, widths, per_channel, signed, moment, input_moment)
                first.append(nsr)
                nsr.run()
            if rounding == 'squant':
                first.append(BatchMixedPlan(self, widths, avg_bits, budget_bits, per_channel, signed, sensitivity, pin, None, False, nsr,
                                            clip, alpha_min))
                alloc = first[-1]
                plans.append(BatchSquantPlan(self, alloc.widths[-1], per_channel, signed, codes, alloc))
                if bits_bias < 32 and any(type(l) in tt and l.bias is not None for l in g0.values()):
                    plans.append(BatchQuantPlan(self, alloc.widths[-1], bits_bias, per_channel, signed, None, _biases_only=True))
                alloc.run(None if clip is None else BatchMixedPlan.ALLOCATE | BatchMixedPlan.CLAMP)
                for plan in plans:
                    plan.run()
                _ffi.synchronize()
                if bool(plans[0].status_block.any()):
                    raise RuntimeError('quantize_mixed: the allocation left a width that is no width (status {})'.format(
                        plans[0].status_block.cpu().tolist()))
                n = len(self.nets)
                ranges = []
                for i in range(n):
                    r = {}
                    for plan in plans:
                        r.update({k: v.clone() for k, v in plan.ranges(i).items()})
                    ranges.append(r)
                return ([{k: v.clone() for k, v in plans[0].codes(i).items()} for i in range(n)], ranges,
                        [dict(alloc.bits(i)) for i in range(n)])
            if clip is not None:
                plans.append(BatchMixedPlan(self, widths, avg_bits, budget_bits, per_channel, signed, sensitivity, pin, codes, True, nsr,
                                            clip, alpha_min))
                if bits_bias < 32 and any(type(l) in tt and l.bias is not None for l in g0.values()):
                    plans.append(BatchQuantPlan(self, plans[0].widths[-1], bits_bias, per_channel, signed, None, _biases_only=True))
                if correct:
                    first.append(self.bc_plan())
                    plans[0].run(BatchMixedPlan.ALLOCATE | BatchMixedPlan.CLAMP)
                    first[-1].run(signed=signed, per_channel=per_channel, widths=plans[0])
                    plans[0].run(BatchMixedPlan.QUANTISE)
                else:
                    plans[0].run()
                for plan in plans[1:]:
                    plan.run()
                if correct:
                    first[-1].status()
                _ffi.synchronize()
                n = len(self.nets)
                ranges = []
                for i in range(n):
                    r = {}
                    for plan in plans:
                        r.update({k: v.clone() for k, v in plan.ranges(i).items()})
                    ranges.append(r)
                return ([{k: v.clone() for k, v in plans[0].codes(i).items()} for i in range(n)], ranges,
                        [dict(plans[0].bits(i)) for i in range(n)])
            if correct:
                first += [BatchMixedPlan(self, widths, avg_bits, budget_bits, per_channel, signed, sensitivity, pin, None, False, nsr),
                          self.bc_plan()]
                first[-2].run()
                first[-1].run(signed=signed, per_channel=per_channel, widths=first[-2])
            plans.append(BatchMixedPlan(self, widths, avg_bits, budget_bits, per_channel, signed, sensitivity, pin, codes, True, nsr))
            if bits_bias < 32 and any(type(l) in tt and l.bias is not None for l in g0.values()):
                plans.append(BatchQuantPlan(self, plans[0].widths[-1], bits_bias, per_channel, signed, None, _biases_only=True))
            for plan in plans:
                plan.run()
            if correct:
                first[-1].status()             # (synchronises; an abandoned wait of the one-launch chain surfaces here)
            _ffi.synchronize()
            n = len(self.nets)
            ranges = []
            for i in range(n):
                r = {}
                for plan in plans:
                    r.update({k: v.clone() for k, v in plan.ranges(i).items()})
                ranges.append(r)
            return ([{k: v.clone() for k, v in plans[0].codes(i).items()} for i in range(n)], ranges,
                    [dict(plans[0].bits(i)) for i in range(n)])
        finally:
            for plan in plans + first:
                plan.close()

    def mx_plan(self, widths=(4, 6, 8), bit_weight=4, fp6='e2m3', fp8='e4m3', search=True, apply=True, codes=True):
        """One plan (BatchMxPlan) that turns the ``targ_type`` weights of the whole batch into the OCP MX block-scaled formats
        the f8f6f4 matrix units of the MI355X multiply natively ("MX block-scaled" in include/dfq_hip.h holds the definition):
        32 consecutive weights of a row share one power-of-two scale (an E8M0 byte), a weight becomes the nearest FP4 (E2M1),
        FP6 (``fp6``: 'e2m3' or 'e3m2') or FP8 (``fp8``: 'e4m3' or 'e5m2') code, ties to the even code, saturating.  ``widths``:
        the candidate widths, a rising subset of (4, 6, 8); the ERRORS stage leaves every layer's sum of squared errors at every
        one of them in ``error_block`` from one read of the weights.  ``search``: per block, the exponent of the OCP floor rule or
        the one above it, whichever gives the block the smaller sum e^2.  ``apply``: ``run()`` also quantises in place at
        ``bit_weight`` (one of ``widths``), or at the widths ``set_widths`` names on the device; ``codes``: keep the one-byte
        codes in ``code_block``.  The plan exposes ``codes(n)``, ``scales(n)``, ``errors(n)``, ``status(n)``, ``set_widths`` and
        ``run(stages)``; ``pack_plan`` packs its codes, ``mixed_plan(costs=)`` allocates on its errors.  Weights only: there is
        no single-network ``quantize_mx`` drop-in, bias correction keeps modelling integer grids, adaptive rounding is not
        defined on these grids, activations are not touched and nothing here multiplies matrices."""
        self._ready('mx_plan')
        return BatchMxPlan(self, widths, bit_weight, fp6, fp8, search, apply, codes)

    def quantize_mx(self, widths=(4, 6, 8), avg_bits=None, budget_bits=None, pin=None, sensitivity=None, search=True, bit_weight=None,
                    fp6='e2m3', fp8='e4m3'):
        """mx_plan, an allocation if a budget is given, run + synchronise: returns (codes, scales, bits, errors), each a list of
        one dict per network -- uint8 codes shaped like the weight, uint8 scale bytes [rows, ceil(row_len / 32)], the width the
        layer got, float64 [len(widths)] sum e^2 at every candidate width.

        With one width, or without ``avg_bits`` / ``budget_bits``, this is the plan at ``bit_weight`` (default: the first width).
        With a budget every layer of every network gets a width of its own out of ``widths``: the mx plan's ERRORS stage,
        ``mixed_plan(widths, avg_bits, budget_bits, sensitivity=, pin=, apply=False, costs=that plan).run()`` -- the greedy walk
        of dfq_batch_mixed_plan on the MX errors --, and the QUANTISE stage at the widths the walk left on the device go onto the
        stream back to back (``set_widths`` is called before the first of them: it enqueues nothing); nothing is copied to the
        host in between.

        The budget counts ELEMENT bits.  The scales come on top: 8 bits per block, 0.25 bit per weight on full blocks and more on
        short rows (a depthwise row of 9 weights carries 8 / 9 bit per weight)."""
        self._ready('quantize_mx')
        widths = tuple(widths)
        budgeted = len(widths) > 1 and (avg_bits is not None or budget_bits is not None)
        mx = BatchMxPlan(self, widths, widths[0] if bit_weight is None else bit_weight, fp6, fp8, search, True, True)
        plans = [mx]
        try:
            n = len(self.nets)
            if budgeted:
                mixed = BatchMixedPlan(self, widths, avg_bits, budget_bits, False, False, sensitivity, pin, None, False, mx)
                plans.append(mixed)
                mx.set_widths(mixed)
                mx.run(BatchMxPlan.ERRORS)
                mixed.run()
                mx.run(BatchMxPlan.QUANTISE)
            else:
                mx.run()
            _ffi.synchronize()
            if bool(mx.status_block.any()):
                raise RuntimeError('quantize_mx: the allocation left a width that is no width (status {})'.format(
                    mx.status_block.cpu().tolist()))
            bits = [dict(mixed.bits(i)) for i in range(n)] if budgeted else [{k: mx.bit_weight for k in mx.keys} for _ in range(n)]
            return ([OrderedDict((k, v.clone()) for k, v in mx.codes(i).items()) for i in range(n)],
                    [OrderedDict((k, v.clone()) for k, v in mx.scales(i).items()) for i in range(n)], bits,
                    [mx.errors(i) for i in range(n)])
        finally:
            for plan in plans:
                plan.close()

    def pack_plan(self, source, word_stride=None):
        """One plan (BatchPackPlan) that packs the integer codes of ``source`` -- a BatchQuantPlan, BatchSquantPlan or
        BatchMixedPlan of this batch created with ``codes`` -- densely, every weight of every network at its own width: the
        stream, the offsets and the status the comment of dfq_batch_pack_plan_create (include/dfq_hip.h) defines.  A mixed
        plan must have been created with ``apply=True`` (its codes are what is packed); its ``bits_block`` is read on the
        device, so ``source.run()`` and ``run()`` of this plan can be enqueued back to back.  A squant plan made with
        ``widths=`` is packed the same way, from the block its widths lie in (the mixed plan's, or the dict's); the other sources
        have one width.  ``word_stride``: uint32 words per network of the packed block; by default the exact size for one width, and
        ceil(budget / 32) + 5 T rounded up to 4 for a mixed plan -- enough whenever ``used <= budget``; ``status(n) == 1`` says so when it is
        not.  ValueError for a source without codes, a mixed plan without ``apply``, a closed source, a source of another
        batch.

        A BatchMxPlan is a source too: its one-byte codes (sign | exponent | mantissa) are packed as unsigned codes at the plan's
        own width, or at the widths of the block its ``set_widths`` named, with the default ``word_stride`` of a layered source;
        the scale bytes stay the source's ``scale_block`` (``save_packed`` writes them out)."""
        self.check()
        return BatchPackPlan(self, source, word_stride)

    def unpack_plan(self, packed, weights=True, codes=None):
        """One plan (BatchUnpackPlan) for the way back: from the words of ``packed`` -- a BatchPackPlan of this batch that
        has run, or the PackedBatch ``load_packed`` returns -- to the weights of every network, in place (``weights``), bit
        for bit what the quantiser stored (up to the sign of a zero: "zero's sign" in include/dfq_hip.h), and / or to the
        integer codes in a block of the plan (``codes``: None, 'int32' or 'int8', as in ``quant_plan``).  One launch.
        ValueError for ``weights=False`` without ``codes``, 'int8' with a width above 8, keys or shapes that are not this
        batch's.

        Words packed from a BatchMxPlan take two launches: the same unpack launch to one-byte codes (``code_block``, always
        kept; ``codes`` is None or 'int8'), then one decode launch (dfq_batch_mx_decode_plan) from the codes and the scale bytes
        to the weights, bit for bit what the quantiser stored, zero signs included -- the sign lives in the code."""
        self._ready('unpack_plan')
        return BatchUnpackPlan(self, packed, weights, codes)

    def save_packed(self, path, source):
        """pack_plan + run + synchronise, then ONE ``.npz`` (numpy only, nothing pickled): per network the packed words
        trimmed to its size (``words_<n>``, uint32), ``offsets`` int64 [n_nets, T + 1], ``widths`` int32 [n_nets, T],
        ``ranges`` float32 [n_nets, R] (the (min, max) pairs the quantiser used, in the order of ``keys``: one pair per
        tensor, or per row with ``per_channel``), ``keys``, ``shapes`` int64 [T, 8] (padded with zeros), ``per_channel``,
        ``signed``, ``version``, and the biases as float32 (``bias_keys``, ``biases`` [n_nets, B] concatenated in that
        order).  ``source`` must have run.  RuntimeError if a network did not pack (status != 0).  Returns the closed pack
        plan, whose blocks stay readable.

        An MX source (``mx_plan``) writes format ``version`` 2: no ``ranges``, but ``mx_scales`` uint8 [n_nets, S] (the scale
        bytes in the order of ``keys``), ``mx_format6``, ``mx_format8`` (the DFQ_MX_* ids of the 6- and 8-bit codes) and
        ``mx_block`` (32).  Files of the other sources keep version 1 and their keys; ``load_packed`` reads both and refuses
        every other version."""
        plan = self.pack_plan(source)
        try:
            plan.run()
            _ffi.synchronize()
        finally:
            plan.close()
        status = plan.status_block.cpu().tolist()
        if any(status):
            raise RuntimeError('save_packed: network {} did not pack (status {})'.format(
                next(n for n, s in enumerate(status) if s), next(s for s in status if s)))
        offsets = plan.offset_block.cpu().numpy()
        words = plan.packed_block.cpu().numpy().view(np.uint32)
        out = {'version': np.int64(_PACKED_VERSION if plan.mx is None else _PACKED_MX_VERSION), 'keys': np.array(plan.keys, dtype=np.str_),
               'offsets': offsets, 'widths': plan.widths_array(), 'per_channel': np.bool_(plan.per_channel), 'signed': np.bool_(plan.signed)}
        shapes = np.zeros((len(plan.keys), 8), dtype=np.int64)
        for i, (_, _, shape) in enumerate(plan._views):
            shapes[i, :len(shape)] = shape
        out['shapes'] = shapes
        if plan.mx is None:
            rng = plan.range_block.cpu().numpy()
            out['ranges'] = np.concatenate([rng[:, off:off + _range_floats(shape)] for (_, off, shape) in plan._range_views], axis=1)
        else:                                               # (an MX file: the scale bytes in the order of `keys`, no ranges)
            sc = plan.mx.scale_block.cpu().numpy()
            out['mx_scales'] = np.concatenate([sc[:, off:off + n_blk] for (_, off, n_blk, _) in plan.mx.views], axis=1)
            out['mx_format6'], out['mx_format8'] = np.int64(_MX_FP6[plan.mx.fp6]), np.int64(_MX_FP8[plan.mx.fp8])
            out['mx_block'] = np.int64(_ffi.MX_BLOCK)
        for n in range(plan.n_nets):
            out['words_{}'.format(n)] = words[n, :int(offsets[n, -1])].copy()
        bias_keys = [k for k in plan.keys if self.nets[0][0][k].bias is not None]
        out['bias_keys'] = np.array(bias_keys, dtype=np.str_)
        out['biases'] = np.stack([np.concatenate([g[k].bias.detach().cpu().numpy().reshape(-1).astype(np.float32) for k in bias_keys]
                                                 or [np.zeros(0, dtype=np.float32)]) for (g, _, _) in self.nets])
        with open(path, 'wb') as f:
            np.savez(f, **out)
        return plan

    def load_packed(self, path):
        """Read a file ``save_packed`` wrote into THIS batch: keys, shapes and the number of networks are checked against the
        batch, the words, offsets, widths and ranges uploaded, the biases copied into the networks, and one unpack launch
        rebuilds every weight in place.  Returns the PackedBatch that holds the blocks (``unpack_plan(it, ...)`` unpacks them
        again, to codes for instance).  ValueError for a file of another architecture or batch size, an unknown ``version``,
        and a file whose offsets do not fit its widths (unpack's status)."""
        self._ready('load_packed')
        packed = PackedBatch(self, path)
        plan = BatchUnpackPlan(self, packed, True, None)
        try:
            plan.run()
            _ffi.synchronize()
        finally:
            plan.close()
        status = plan.statuses()
        if any(status):
            raise ValueError('load_packed: the offsets of network {} do not fit its widths (status {})'.format(
                next(n for n, s in enumerate(status) if s), next(s for s in status if s)))
        with torch.no_grad():
            for n, (graph, _, _) in enumerate(self.nets):
                at = 0
                for k in packed._bias_keys:
                    b = graph[k].bias
                    b.copy_(torch.from_numpy(packed._biases[n, at:at + b.numel()].copy()).view(b.shape))
                    at += b.numel()
        return packed

    def absorb_plan(self, N=3, range_clip=None, absorb=True):
        """One plan (BatchAbsorbPlan) for ``bias_absorption(graph, relations, bottoms, N)`` followed, if ``range_clip`` is
        given, by ``clip_weight(graph, range_clip, targ_type)`` on every network of the batch, bit for bit.  ``absorb=False``
        with a ``range_clip`` is clip_weight alone.  Relations without a ReLU between their layers are skipped as
        bias_absorption skips them (the walk is made on network 0).  ValueError for an ``N`` that is not a finite number, a
        ``range_clip`` that is not a pair lo <= hi, and a second layer of an absorbed relation whose bias has no slot in the
        batch allocation; RuntimeError for a tensor of network 0 that has left its slot."""
        self._ready('absorb_plan')
        return BatchAbsorbPlan(self, N, range_clip, absorb)

    def absorb(self, N=3, range_clip=None, absorb=True):
        """absorb_plan + run + synchronise + close"""
        plan = self.absorb_plan(N, range_clip, absorb)
        try:
            plan.run()
            _ffi.synchronize()
        finally:
            plan.close()

    def act_range_plan(self, is_detection=False, N=6, tensor_ops=None):
        """One plan (BatchActRangePlan) for ``set_quant_minmax(graph, bottoms, is_detection, N=N)`` on every network of the
        batch, bit for bit: the analytic (min, max) of every activation quantiser from the BatchNorm proxies in front of it.
        The graph walk is made once, on network 0.  A range is computed for every layer with a ``.quant`` and for every
        ``targ_type`` layer without one (its input range, what ``ncnn_table`` asks for); ``tensor_ops = {graph key: count}``
        adds the inputs of add / cat / mean / interpolate / softmax nodes, as ``tensor_op_quant`` does for the single-network
        function.  ValueError for an ``N`` that is not a finite number, an unknown key or a non-positive count in
        ``tensor_ops``, a BatchNorm without proxies, and a graph set_quant_minmax itself would refuse; RuntimeError for a
        tensor of network 0 that has left its slot."""
        self._ready('act_range_plan')
        return BatchActRangePlan(self, is_detection, N, tensor_ops)

    def set_quant_minmax(self, is_detection=False, N=6, tensor_op_quant=None):
        """act_range_plan + run + synchronise + bind_quantisers + close: afterwards every ``layer.quant`` of every network
        holds its range, as a view of the plan's block.  ``tensor_op_quant``: one ``{graph key: [QuantMeasure, ...]}`` per
        network (the quantisers of tensor ops, as the single-network function takes them).  Returns the closed plan, whose
        ``ranges(n)`` stay readable."""
        ops = None
        if tensor_op_quant is not None:
            tensor_op_quant = list(tensor_op_quant)
            if len(tensor_op_quant) != len(self.nets):
                raise ValueError('set_quant_minmax: tensor_op_quant wants one dict per network ({}), got {}'.format(
                    len(self.nets), len(tensor_op_quant)))
            ops = OrderedDict((k, len(v)) for k, v in tensor_op_quant[0].items())
            for n, tq in enumerate(tensor_op_quant):
                if OrderedDict((k, len(v)) for k, v in tq.items()) != ops:
                    raise ValueError('set_quant_minmax: the tensor-op quantisers of network {} are not those of network 0'.format(n))
        plan = self.act_range_plan(is_detection, N, ops)
        try:
            plan.run()
            _ffi.synchronize()
            plan.bind_quantisers(tensor_op_quant)
        finally:
            plan.close()
        return plan

    def table_plan(self):
        """One plan (BatchTablePlan) for the weight statistics of the ncnn int8 calibration table (``ncnn_table``,
        convert_ncnn.py:178-201) of every network of the batch: ``run()`` reads every ``targ_type`` weight once, writes none,
        and fills one block with each tensor's (min, max) -- ``ncnn_table.weight_ranges`` -- and each output row's max|w| --
        ``prims.row_range(w, signed=True)`` -- exactly.  RuntimeError for a weight of network 0 that has left its slot."""
        self._ready('table_plan')
        return BatchTablePlan(self)

    def calibration_tables(self, act=None, names=None, per_channel=False):
        """The lines of ``model_int8_tensor.table`` of every network: a list with one list of lines per network, each equal,
        string for string, to ``ncnn_table.calibration_table(graph, targ_type, names, per_channel)`` on that network alone.
        table_plan + run + synchronise + ONE device-to-host copy of the block + close.  ``act``: a BatchActRangePlan of this
        batch that has run, open or closed (what ``set_quant_minmax()`` returns): the activation range of layer k is the one
        that plan holds for key k, read with one more copy.  ``act=None``: the quantisers ``graph[k].quant`` of every network
        are read as the single-network function reads them (min of ``running_min``, max of ``running_max``), gathered on the
        device into one tensor first.  ``names``: one list for the whole batch, the weight block's names first, then the
        activation block's (2 x layers of them, ValueError otherwise); None: the graph keys.  ZeroDivisionError, naming
        network, key and row, where the single-network function raises it: an all-zero tensor, or row with ``per_channel``,
        or an activation range of zeros."""
        self._ready('calibration_tables')
        keys = self._table_keys()
        if names is None:
            names = ['{}_param_0'.format(k) for k in keys] + [str(k) for k in keys]
        names = list(names)
        if len(names) != 2 * len(keys):
            raise ValueError('calibration_tables: need one name per layer for the weight block and one for the activation block '
                             '({}), got {}'.format(2 * len(keys), len(names)))
        return self._format_tables(names, per_channel, *self._table_statistics(act))

    def _table_keys(self):
        g0, tt = self.nets[0][0], tuple(self.targ_type)
        return [k for k in g0 if type(g0[k]) in tt]

    def _table_statistics(self, act):
        """the device side of ``calibration_tables``: (the table plan's views, its block as nested lists of Python floats, the
        (min, max) of every layer's activation range per network); two blocking copies"""
        keys, n_nets = self._table_keys(), len(self.nets)
        if act is not None:
            if not isinstance(act, BatchActRangePlan) or act._batch is not self:
                raise ValueError('calibration_tables: act is not an act_range_plan of this batch')
            at = {key: first for (key, first, _, is_op) in act._views if not is_op}
            missing = [k for k in keys if k not in at]
            if missing:
                raise ValueError('calibration_tables: the act_range_plan holds no range for {}'.format(missing[0]))
        else:
            mins, maxs = [], []
            for n, (graph, _, _) in enumerate(self.nets):
                for k in keys:
                    q = getattr(graph[k], 'quant', None)
                    if q is None:
                        raise AttributeError('calibration_tables: {} of network {} has no quantiser (.quant); pass act= an '
                                             'act_range_plan'.format(k, n))
                    lo, hi = q.running_min, q.running_max
                    mins.append(lo.reshape(1) if lo.numel() == 1 else torch.min(lo).reshape(1))
                    maxs.append(hi.reshape(1) if hi.numel() == 1 else torch.max(hi).reshape(1))
        plan = self.table_plan()
        try:
            plan.run()
            _ffi.synchronize()
            block = plan.block.cpu().tolist()                          # Python floats: str() gives the reference's digits
        finally:
            plan.close()
        if act is not None:
            pairs = act.block.cpu().tolist()
            act_of = [[tuple(pairs[n][at[k]]) for k in keys] for n in range(n_nets)]
        else:
            both = torch.stack([torch.cat(mins), torch.cat(maxs)]).cpu().tolist()       # gathered on the device: one copy
            act_of = [[(both[0][n * len(keys) + i], both[1][n * len(keys) + i]) for i in range(len(keys))] for n in range(n_nets)]
        return plan._views, block, act_of

    def error_plan(self, configs=((8, False, False),)):
        """One plan (BatchErrorPlan) for the weight quantisation error of every ``targ_type`` weight of every network under
        one to four quantiser configurations, each ``(bit_weight, per_channel, signed)`` as ``quant_plan`` takes them: the
        batch form of ``_quantize_error(param, num_bits, reduction, signed)`` (dfq.py:8-25).  ``run()`` reads every weight
        twice and writes none; ``errors(n)`` gives per weight ``sum w^2`` and, per configuration, ``sum e``, ``sum |e|`` and
        ``sum e^2`` of e = Q(w) - w, where Q(w) is bit for bit the value ``quant_plan`` with that configuration would store.
        The 'channel' and 'spatial' reductions of dfq.py:20-23 have no caller in the reference and are not offered; biases
        (16 bits per tensor, a negligible error) are not included.  ValueError for a bad configuration, RuntimeError for a
        weight of network 0 that has left its slot."""
        self._ready('error_plan')
        return BatchErrorPlan(self, configs)

    def quantize_error(self, bit_weight=8, per_channel=False, signed=False):
        """error_plan + run + synchronise + close for one configuration: one ``OrderedDict[key -> dict]`` per network with
        ``sum`` = sum |e| (``_quantize_error(w, bits, 'sum')``), ``mean`` = sum e / numel (its ``'mean'``), ``mse`` =
        sum e^2 / numel and ``sqnr_db`` = 10 log10(sum w^2 / sum e^2), ``inf`` where sum e^2 is 0; Python floats from
        float64 sums."""
        plan = self.error_plan(((bit_weight, per_channel, signed),))
        try:
            plan.run()
            _ffi.synchronize()
            block = plan.block.cpu()
        finally:
            plan.close()
        out = []
        for n in range(len(self.nets)):
            res = OrderedDict()
            for key, e in plan.errors(n, block).items():
                numel, s, s_abs, s_sq = e['numel'], float(e['sum'][0]), float(e['sum_abs'][0]), float(e['sum_sq'][0])
                if s_sq == 0:
                    sqnr = math.inf
                else:
                    ratio = e['sum_sq_w'] / s_sq
                    sqnr = 10.0 * math.log10(ratio) if ratio > 0 else (-math.inf if ratio == 0 else math.nan)
                res[key] = {'sum': s_abs, 'mean': s / numel, 'mse': s_sq / numel, 'sqnr_db': sqnr}
            out.append(res)
        return out

    def clip_plan(self, bit_weight=8, per_channel=False, signed=False, candidates=32, alpha_min=0.5, apply=True, keep_errors=False):
        """One plan (BatchClipPlan) for the MSE-optimal clipping of every ``targ_type`` weight of every network: per tensor,
        or per output row with ``per_channel``, the one of ``candidates`` ranges -- shrunk from the unit's (min, max) toward
        zero by factors from 1 down to ``alpha_min`` -- under which the ``bit_weight``-bit quantiser (``signed``: the symmetric
        recipe) has the least sum of squared errors; with ``apply`` the weights are clamped to it in place, the reference's
        ``clip_weight`` (dfq.py:167-170) with a searched bound.  The definition is the comment of dfq_batch_clip_plan_create
        (include/dfq_hip.h).  A unit's own (min, max) is then the chosen range, so ``bc_plan``, ``quant_plan``,
        ``table_plan`` and ``error_plan`` see it unchanged: the plan stands where ``absorb_plan(range_clip=...)`` clips,
        behind equalisation and absorption, in front of bias correction.  ``keep_errors``: every candidate's sum e^2 stays
        readable (``errors(n)``).  ValueError for a bit width that is not an int in [2, 16], ``candidates`` not an int in
        [1, 64], an ``alpha_min`` that is not a number in (0, 1]; RuntimeError for a weight of network 0 that has left its
        slot."""
        self._ready('clip_plan')
        return BatchClipPlan(self, bit_weight, per_channel, signed, candidates, alpha_min, apply, keep_errors)

    def clip_weight_mse(self, bit_weight=8, per_channel=False, signed=False, candidates=32, alpha_min=0.5):
        """clip_plan(apply=True, keep_errors=True) + run + synchronise + close: one
        ``OrderedDict[key -> {'range', 'chosen', 'err_minmax', 'err'}]`` per network -- the chosen (l, h), k*, and sum e^2 under
        the min/max range and under the chosen one (numpy values on the host)."""
        plan = self.clip_plan(bit_weight, per_channel, signed, candidates, alpha_min, True, True)
        try:
            plan.run()
            _ffi.synchronize()
            return [plan.report(n) for n in range(len(self.nets))]
        finally:
            plan.close()

    def _format_tables(self, names, per_channel, views, block, act_of):
        """the host side of ``calibration_tables``: the strings, by the recipe the single-network function uses"""
        tables = []
        for n in range(len(self.nets)):
            row, lines = block[n], []
            for i, (k, r_off, a_off, rows) in enumerate(views):
                if per_channel:
                    lines.append(_ncnn._table_line(names[i], [(a, a) for a in row[a_off:a_off + rows]], 1,
                                                   lambda j, n=n, k=k: 'network {}, weight of {}, row {}'.format(n, k, j)))
                else:
                    lines.append(_ncnn._table_line(names[i], [(row[r_off], row[r_off + 1])], rows,
                                                   lambda j, n=n, k=k: 'network {}, weight of {}'.format(n, k)))
            for i, (k, _, _, _) in enumerate(views):
                lines.append(_ncnn._table_line(names[len(views) + i], [act_of[n][i]], 1,
                                               lambda j, n=n, k=k: 'network {}, activation range of {}'.format(n, k)))
            tables.append(lines)
        return tables

    def write_calibration_tables(self, paths, act=None, names=None, per_channel=False):
        """``calibration_tables`` written to one file per network (``paths``: one per network, ValueError otherwise), as
        ``ncnn_table.write_calibration_table`` writes one; returns the lines.  Nothing is written if a table cannot be made."""
        paths = list(paths)
        if len(paths) != len(self.nets):
            raise ValueError('write_calibration_tables: need one path per network ({}), got {}'.format(len(self.nets), len(paths)))
        tables = self.calibration_tables(act, names, per_channel)
        for path, lines in zip(paths, tables):
            with open(path, 'w') as f:
                for line in lines:
                    f.write(line + '\n')
        return tables


def _check_bits(bits, per_channel, what):
    """a bit width as quantize_targ_layer takes it: per channel an integer in [2, 16] (_quantize_targ_layer_rows), per tensor
    whatever int() makes of it, in [1, 30] (what dfq_quant_plan_create accepts)"""
    if per_channel:
        if isinstance(bits, bool) or not isinstance(bits, (int, np.integer)) or not 2 <= bits <= 16:
            raise ValueError('quant_plan: per-channel {} {!r} outside [2, 16]'.format(what, bits))
        return int(bits)
    try:
        b = int(bits)
    except (TypeError, ValueError):
        raise ValueError('quant_plan: {} {!r} is not a bit width'.format(what, bits)) from None
    if not 1 <= b <= 30:
        raise ValueError('quant_plan: {} {!r} outside [1, 30]'.format(what, bits))
    return b


def _finite(N, who):
    """N as a float, or ValueError('<who>: N ...'): a number, finite, not a bool"""
    try:
        n_sigma = float(N)
    except (TypeError, ValueError):
        raise ValueError('{}: N {!r} is not a number'.format(who, N)) from None
    if isinstance(N, bool) or not math.isfinite(n_sigma):
        raise ValueError('{}: N {!r} is not a finite number'.format(who, N))
    return n_sigma


class _BatchPlan:
    """What the plans over a NetworkBatch share: the handle of the C plan (``_c``_create / _run / _destroy / _launches of
    include/dfq_hip.h, which all take network 0's tables and the batch's base addresses), ``launches``, ``run()`` and
    ``close()``.  A subclass builds its tables in its constructor and hands them to ``_create``."""
    _c = None                                   # 'dfq_batch_<step>_plan'

    def __init__(self, batch):
        self._batch, self._plan, self.launches = batch, None, 0

    def _create(self, tables, *rest):
        """<_c>_create(*tables, base addresses, number of networks, *rest, &plan)"""
        batch, lib = self._batch, _ffi.lib()
        self._plan = ctypes.c_void_p()
        _ffi.check(getattr(lib, self._c + '_create')(*tables, batch.bases.ctypes.data_as(ctypes.POINTER(ctypes.c_void_p)),
                                                     len(batch.nets), *rest, ctypes.byref(self._plan)))
        self.launches = int(getattr(lib, self._c + '_launches')(self._plan))

    def run(self):
        """Enqueue the plan's launches, which cover every network of the batch, on the current stream (asynchronous)."""
        if self._batch.storage is None:
            raise RuntimeError('NetworkBatch: the batch has been released')
        if not self._plan:
            raise RuntimeError('{}: the plan has been closed'.format(type(self).__name__))
        _ffi.check(getattr(_ffi.lib(), self._c + '_run')(self._plan, _ffi.stream_arg()))

    def close(self):
        if self._plan:
            getattr(_ffi.lib(), self._c + '_destroy')(self._plan)
            self._plan = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BatchQuantPlan(_BatchPlan):
    """Weight quantisation of every network of a NetworkBatch (dfq_batch_quant_plan, include/dfq_hip.h): network 0's tensor
    table plus the batch's base addresses.  ``run()`` enqueues on the current stream; the weights and biases are quantised in
    place, the codes and ranges written to blocks [n_nets, stride] the plan owns and hands out as views."""
    _c = 'dfq_batch_quant_plan'

    def __init__(self, batch, bit_weight, bits_bias, per_channel, signed, codes, _biases_only=False):
        bit_weight = _check_bits(bit_weight, per_channel, 'bit_weight')
        with_bias = bits_bias < 32                   # layer_transform.py: `bits_bias < 32` decides whether biases are quantised
        if with_bias:
            bits_bias = _check_bits(bits_bias, per_channel, 'bits_bias')
        if codes not in (None, 'int32', 'int8'):
            raise ValueError("quant_plan: codes must be None, 'int32' or 'int8', got {!r}".format(codes))
        if codes == 'int8' and bit_weight > 8:
            raise ValueError('quant_plan: 1-byte codes need bit_weight <= 8, got {}'.format(bit_weight))
        super().__init__(batch)
        self.per_channel, self.signed, self.bit_weight = bool(per_channel), bool(signed), bit_weight
        n_nets = len(batch.nets)
        dev = batch.stage.device
        g0 = batch.nets[0][0]
        tt = tuple(batch.targ_type)
        entries, self._code_views, self._range_views = [], [], []
        code_stride = range_stride = 0
        in_slot = batch._in_slot
        for key, layer in g0.items():
            if type(layer) not in tt:
                continue
            w = layer.weight
            rows = int(w.shape[0])
            c_off = -1
            if not _biases_only:                     # (quantize_squant: the weights are another plan's)
                if codes is not None:
                    c_off = code_stride
                    self._code_views.append((key, c_off, w.numel(), tuple(w.shape)))
                    code_stride += -(-w.numel() // 64) * 64
                n_rng = 2 * rows if per_channel else 2
                self._range_views.append((key, range_stride, (rows, 2) if per_channel else (2,)))
                entries.append(_ffi.DfqBatchQuantTensor(in_slot(key, 'weight', w), rows, w.numel() // rows, bit_weight, int(self.signed),
                                                        int(self.per_channel), 0, c_off, range_stride))
                range_stride += n_rng
            b = layer.bias
            if b is not None and with_bias:
                self._range_views.append((key + '.bias', range_stride, (2,)))
                entries.append(_ffi.DfqBatchQuantTensor(in_slot(key, 'bias', b), 1, b.numel(), bits_bias, 0, 0, 0, -1, range_stride))
                range_stride += 2
        if not entries:
            raise ValueError('quant_plan: the batch has no {} layer'.format(tt))
        dtype = {None: torch.int32, 'int32': torch.int32, 'int8': torch.int8 if self.signed else torch.uint8}[codes]
        self.code_dtype = None if codes is None else dtype
        self.code_block = torch.empty((n_nets, code_stride), dtype=dtype, device=dev) if codes is not None else None
        self.range_block = torch.empty((n_nets, range_stride), dtype=torch.float32, device=dev)
        self.n_nets, self.n_tensors = n_nets, len(entries)
        arr = (_ffi.DfqBatchQuantTensor * len(entries))(*entries)
        self._create((arr, len(entries)), None if self.code_block is None else self.code_block.data_ptr(),
                     1 if codes == 'int8' else 4, code_stride, self.range_block.data_ptr(), range_stride)

    def codes(self, n):
        """{graph key: integer codes of network n's weight, shaped like it} -- views of the code block"""
        if self.code_block is None:
            return {}
        row = self.code_block[n]
        return {key: row[off:off + numel].view(shape) for (key, off, numel, shape) in self._code_views}

    def ranges(self, n):
        """{graph key: float32 [O, 2] (per channel) or [2]} of network n's weights, {key + '.bias': [2]} of its biases"""
        row = self.range_block[n]
        return {key: row[off:off + 2 * (shape[0] if len(shape) == 2 else 1)].view(shape) for (key, off, shape) in self._range_views}


class BatchSquantPlan(_BatchPlan):
    """Adaptive rounding (SQuant; "Adaptive rounding" in include/dfq_hip.h) of the weights of every network of a NetworkBatch
    (dfq_batch_squant_plan): network 0's tensor table plus the batch's base addresses.  Weights only; ``run()`` enqueues on the
    current stream and quantises them in place.  The codes, ranges and per-row stats are written to blocks [n_nets, stride] the
    plan owns and hands out as views."""
    _c = 'dfq_batch_squant_plan'

    def __init__(self, batch, bit_weight, per_channel, signed, codes, widths=None):
        bit_weight = _check_bits(bit_weight, True, 'bit_weight')        # [2, 16] in both range modes
        if codes not in (None, 'int32', 'int8'):
            raise ValueError("squant_plan: codes must be None, 'int32' or 'int8', got {!r}".format(codes))
        if codes == 'int8' and bit_weight > 8:
            raise ValueError('squant_plan: 1-byte codes need bit_weight <= 8, got {}'.format(bit_weight))
        own = {}                                                        # widths known on the host: into every tensor's num_bits
        if isinstance(widths, BatchMixedPlan):
            self._check_mixed(batch, widths, per_channel, signed, codes)
        elif widths is not None:
            if not isinstance(widths, dict):
                raise ValueError('squant_plan: widths must be None, a mixed_plan of this batch or a dict key -> width, got {!r}'.format(
                    type(widths).__name__))
            keys = [key for key, layer in batch.nets[0][0].items() if type(layer) in tuple(batch.targ_type)]
            for key, b in widths.items():
                if key not in keys:
                    raise ValueError('squant_plan: widths names {!r}, which is no layer to quantise'.format(key))
                if isinstance(b, bool) or not isinstance(b, (int, np.integer)) or not 2 <= b <= 16:
                    raise ValueError('squant_plan: the width of {!r} must be an int in [2, 16], got {!r}'.format(key, b))
                if codes == 'int8' and b > 8:
                    raise ValueError('squant_plan: 1-byte codes need widths <= 8, got {} for {!r}'.format(b, key))
            own = {key: int(b) for key, b in widths.items()}
        g0 = batch.nets[0][0]
        tt = tuple(batch.targ_type)
        layers = [(key, layer.weight) for key, layer in g0.items() if type(layer) in tt]
        if not layers:
            raise ValueError('squant_plan: the batch has no {} layer'.format(tt))
        n_nets = len(batch.nets)
        lay = _dfq._SquantLayout('squant_plan', layers, lambda key, w: batch._in_slot(key, 'weight', w), n_nets,
                                 lambda key: own.get(key, bit_weight), per_channel, signed, codes, batch.stage.device)
        super().__init__(batch)
        self._lay = lay
        self.per_channel, self.signed, self.bit_weight = lay.per_channel, lay.signed, bit_weight
        self.keys, self.n_nets, self.n_tensors = lay.keys, n_nets, lay.n_tensors
        self._code_views, self._range_views, self._stats_views = lay._code_views, lay._range_views, lay._stats_views
        self.code_dtype, self.code_block, self.range_block = lay.code_dtype, lay.code_block, lay.range_block
        self.stats_block, self.status_block = lay.stats_block, lay.status_block
        self._create(lay.tables(), *lay.block_args())
        # the width of every (network, layer): one for all (``bits_block`` None), the dict's -- a block of this plan, for
        # pack_plan --, or the mixed plan's block, which every run reads on the device
        self._codes_kind = codes
        self._own_bits = self._own_budget = None
        if own:
            row = [own.get(key, bit_weight) for key in self.keys]
            self._own_bits = torch.tensor([row] * n_nets, dtype=torch.int32, device=batch.stage.device)
            self._own_budget = sum(w.numel() * b for (_, w), b in zip(layers, row))
        self.bits_block, self.budget, self._mixed = self._own_bits, self._own_budget, None
        if isinstance(widths, BatchMixedPlan):
            self.set_widths(widths)

    @staticmethod
    def _check_mixed(batch, mixed, per_channel, signed, codes):
        """the rules of mixed_plan(costs=): a live plan of this batch made for the same ranges"""
        if mixed._batch is not batch:
            raise ValueError('squant_plan: widths is a mixed_plan of another batch')
        if not mixed._plan:
            raise ValueError('squant_plan: the mixed_plan given as widths has been closed')
        if bool(per_channel) != mixed.per_channel or bool(signed) != mixed.signed:
            raise ValueError('squant_plan: the widths were allocated for per_channel {}, signed {}; the plan asks for {}, {}'.format(
                mixed.per_channel, mixed.signed, bool(per_channel), bool(signed)))
        if codes == 'int8' and mixed.widths[-1] > 8:
            raise ValueError('squant_plan: 1-byte codes need widths <= 8, got {!r}'.format(mixed.widths))

    def set_widths(self, mixed):
        """Round every layer of every network at the width ``mixed`` -- a BatchMixedPlan of this batch, checked as
        ``squant_plan(widths=)`` checks it -- leaves in its ``bits_block``, read on the device by every later run
        (dfq_batch_squant_plan_set_widths, include/dfq_hip.h); None: at the plan's own widths again -- ``bit_weight``, or the
        dict the plan was made with.  A ``pack_plan`` made of this plan before the call was made for the widths of then and
        refuses to run (RuntimeError): make a new one."""
        if not self._plan:
            raise RuntimeError('BatchSquantPlan: the plan has been closed')
        lib = _ffi.lib()
        if mixed is None:
            _ffi.check(lib.dfq_batch_squant_plan_set_widths(self._plan, None, 0, None, None))
            self.bits_block, self.budget, self._mixed = self._own_bits, self._own_budget, None      # (a dict's widths: the table's)
            return
        if not isinstance(mixed, BatchMixedPlan):
            raise ValueError('squant_plan: set_widths takes a mixed_plan of this batch or None, got {!r}'.format(type(mixed).__name__))
        self._check_mixed(self._batch, mixed, self.per_channel, self.signed, self._codes_kind)
        at = {key: i for i, key in enumerate(mixed.keys)}
        index = (ctypes.c_int32 * len(self.keys))(*[at[key] for key in self.keys])
        _ffi.check(lib.dfq_batch_squant_plan_set_widths(self._plan, mixed.bits_block.data_ptr(), mixed.bits_block.shape[1], index,
                                                        self.status_block.data_ptr()))
        self.bits_block, self.budget, self._mixed = mixed.bits_block, mixed.budget, mixed     # (kept alive while the plan reads it)

    def status(self, n):
        """0, or 2: a width network n's row of the device block held at the last run was no width (outside [2, 16], or above 8
        with 'int8' codes), and that layer was left as it was; always 0 for a plan without device widths"""
        return int(self.status_block[n].cpu())

    def codes(self, n):
        """{graph key: integer codes of network n's weight, shaped like it} -- views of the code block"""
        if self.code_block is None:
            return {}
        row = self.code_block[n]
        return {key: row[off:off + numel].view(shape) for (key, off, numel, shape) in self._code_views}

    def ranges(self, n):
        """{graph key: float32 [O, 2] (per channel) or [2]} of network n's weights"""
        row = self.range_block[n]
        return {key: row[off:off + 2 * (shape[0] if len(shape) == 2 else 1)].view(shape) for (key, off, shape) in self._range_views}

    def stats(self, n):
        """{graph key: int64 [O, 2]}: per output row (the sum of P = round(p * 2^30) it is left with, at most 2^29 in size;
        the number of codes that differ from nearest rounding)"""
        row = self.stats_block[n]
        return {key: row[off:off + 2 * rows].view(rows, 2) for (key, off, rows) in self._stats_views}


class BatchMixedPlan(_BatchPlan):
    """Mixed-precision quantisation of the weights of every network of a NetworkBatch (dfq_batch_mixed_plan, include/dfq_hip.h,
    which holds the definition): network 0's table of ``targ_type`` weights plus the batch's base addresses.  ``run()``
    enqueues on the current stream -- ranges, the errors at every width, the allocation (one workgroup per network) and, with
    ``apply``, the quantisation in place: ``launches`` of them, and nothing goes to the host in between.  The results lie in
    blocks the plan owns, torch tensors that outlive ``close()``: ``bits_block`` int32 [n_nets, T], ``error_block`` float64
    [n_nets, T, B], ``used_block`` int64 [n_nets, 2] = (used bits, steps), ``cost_block`` float64 [n_nets], ``range_block``
    and, with ``codes``, ``code_block``.  ``widths``, ``budget`` (bits per network) and ``elements`` (weights per network) are
    what the plan was made with.  Two runs of a plan without ``apply`` give bit-equal blocks, and a network's part does not
    depend on the others.  With ``clip=K`` the plan is the clip-aware one (dfq_batch_mixed_plan_create_clipped): the range
    search at every width in front of the allocation, the clamp in front of the quantisation, and the blocks
    ``clip_range_block``, ``clip_chosen_block`` and ``unit_error_block`` (None otherwise); ``run(stages)`` runs the stages of
    either kind of plan one by one."""
    _c = 'dfq_batch_mixed_plan'
    ALLOCATE, CLAMP, QUANTISE = _ffi.MIXED_ALLOCATE, _ffi.MIXED_CLAMP, _ffi.MIXED_QUANTISE

    def __init__(self, batch, widths, avg_bits, budget_bits, per_channel, signed, sensitivity, pin, codes, apply, costs=None, clip=None,
                 alpha_min=0.5):
        g0 = batch.nets[0][0]
        tt = tuple(batch.targ_type)
        layers = [(key, layer.weight) for key, layer in g0.items() if type(layer) in tt]
        if not layers:
            raise ValueError('mixed_plan: the batch has no {} layer'.format(tt))
        if costs is not None:
            if not isinstance(costs, (BatchNsrPlan, BatchMxPlan)) or costs._batch is not batch:
                raise ValueError('mixed_plan: costs must be a BatchNsrPlan (or a BatchMxPlan) of this batch')
            try:
                same = tuple(widths) == costs.widths
            except TypeError:
                same = False
            if isinstance(costs, BatchMxPlan):                  # (an MX grid has no per_channel / signed: the widths alone)
                if not same:
                    raise ValueError('mixed_plan: costs were made for widths {!r}; the plan asks for {!r}'.format(costs.widths, widths))
            elif not same or bool(per_channel) != costs.per_channel or bool(signed) != costs.signed:
                raise ValueError('mixed_plan: costs were made for widths {!r}, per_channel {}, signed {}; the plan asks for {!r}, {}, {}'.format(
                    costs.widths, costs.per_channel, costs.signed, widths, bool(per_channel), bool(signed)))
        lay = _dfq._MixedLayout('mixed_plan', layers, lambda key, w: batch._in_slot(key, 'weight', w), len(batch.nets), widths,
                                avg_bits, budget_bits, per_channel, signed, sensitivity, pin, codes, apply, batch.stage.device, clip, alpha_min)
        super().__init__(batch)
        self._lay = lay
        self.clip, self.alpha_min = lay.clip, lay.alpha_min
        self.clip_range_block, self.clip_chosen_block, self.unit_error_block = lay.clip_range_block, lay.clip_chosen_block, lay.unit_error_block
        self.widths, self.budget, self.elements = lay.widths, lay.budget, lay.total
        self.per_channel, self.signed, self.apply = lay.per_channel, lay.signed, lay.apply
        self.keys, self.n_nets, self.n_tensors = lay.keys, lay.n_nets, lay.n_tensors
        self.code_dtype = lay.code_dtype
        self.bits_block, self.error_block, self.used_block, self.cost_block = lay.bits_block, lay.error_block, lay.used_block, lay.cost_block
        self.range_block, self.code_block = lay.range_block, lay.code_block
        if lay.clip is None:
            self._create(lay.tables(), *lay.block_args())
        else:
            self._plan = ctypes.c_void_p()
            _ffi.check(lay.create(_ffi.lib(), batch.bases.ctypes.data_as(ctypes.POINTER(ctypes.c_void_p)), len(batch.nets), self._plan))
            self.launches = int(_ffi.lib().dfq_batch_mixed_plan_launches(self._plan))
        self._costs = None
        if costs is not None:
            self.set_costs(costs)

    def set_costs(self, costs):
        """Allocate on ``costs.cost_block`` (a BatchNsrPlan of the same batch, widths, per_channel and signed: the constructor
        checks that, this does not) from the next run on; None: on the plan's own errors again."""
        if not self._plan:
            raise RuntimeError('BatchMixedPlan: the plan has been closed')
        block = None if costs is None else costs.cost_block
        _ffi.check(_ffi.lib().dfq_batch_mixed_plan_set_costs(self._plan, None if block is None else block.data_ptr()))
        self._costs = block                        # (kept alive while the plan reads it)

    def run(self, stages=None):
        """Enqueue the plan on the current stream.  ``stages=None``: the whole plan (the allocation and, with ``apply``, the
        quantisation).  Else a sum of ``BatchMixedPlan.ALLOCATE``, ``CLAMP`` (plans made with ``clip=``) and ``QUANTISE``
        (dfq_batch_mixed_plan_run_stages, include/dfq_hip.h): CLAMP and QUANTISE work at the widths the plan's last ALLOCATE
        left in the plan's own state, whatever ``apply`` says."""
        if stages is None:
            return super().run()
        if self._batch.storage is None:
            raise RuntimeError('NetworkBatch: the batch has been released')
        if not self._plan:
            raise RuntimeError('BatchMixedPlan: the plan has been closed')
        _ffi.check(_ffi.lib().dfq_batch_mixed_plan_run_stages(self._plan, int(stages), _ffi.stream_arg()))

    def allocate(self):
        """``run(ALLOCATE)``: ranges, errors, allocation"""
        self.run(self.ALLOCATE)

    def clamp(self):
        """``run(CLAMP)``: every unit clamped to the range of its layer's chosen width (plans made with ``clip=``)"""
        self.run(self.CLAMP)

    def quantise(self):
        """``run(QUANTISE)``: clamp and quantise at the chosen widths"""
        self.run(self.QUANTISE)

    def clip_ranges(self, n):
        """{graph key: float32 [B, 2] (or [O, B, 2] per channel) view}: (l, h) of k* at every width; plans made with ``clip=``"""
        return self._lay.clip_ranges(n)

    def clip_chosen(self, n):
        """{graph key: int32 [B] (or [O, B]) view}: k* at every width (0 is the unit's own (min, max))"""
        return self._lay.clip_chosen(n)

    def unit_errors(self, n):
        """{graph key: float64 [B] (or [O, B]) view}: sum e^2 of the unit under k* at every width"""
        return self._lay.unit_errors(n)

    def bits(self, n):
        """``OrderedDict[graph key -> int]``: the width network n's weight got (one device-to-host copy)"""
        return self._lay.bits(n)

    def errors(self, n):
        """``OrderedDict[graph key -> float64 numpy [B]]``: sum e^2 of network n's weight at every width of ``widths``"""
        return self._lay.errors(n)

    def used(self, n):
        """(bits network n's allocation takes, steps the walk took); used > ``budget`` if the start alone exceeds it"""
        return self._lay.used(n)

    def cost(self, n):
        """sum over the layers of sensitivity * sum e^2 at the chosen widths, added in the order of ``keys``"""
        return self._lay.cost(n)

    def ranges(self, n):
        """{graph key: float32 [O, 2] (per channel) or [2]} of network n's weights: the (min, max) the quantiser used"""
        return self._lay.ranges(n)

    def codes(self, n):
        """{graph key: integer codes of network n's weight, shaped like it} -- views of the code block; {} without codes"""
        return self._lay.codes(n)


class BatchNsrPlan(_BatchPlan):
    """Data-free layer sensitivities of every network of a NetworkBatch (dfq_batch_nsr_plan, include/dfq_hip.h, which holds the
    definition): network 0's table of ``targ_type`` weights, the source table of its bias-correction walk -- the batch's own, made
    when the batch was put together -- and the batch's base addresses.  ``run()`` enqueues ``launches`` launches on the current
    stream and writes nothing but the plan's blocks, torch tensors that outlive ``close()``: ``moment_block`` float32
    [n_nets, moment_stride], ``row_block`` float64 [n_nets, row_stride, B] (R per output row), ``signal_block`` float64
    [n_nets, row_stride] (S) and ``cost_block`` float64 [n_nets, T, B] (N, what ``mixed_plan(costs=)`` reads).  Two runs give
    bit-equal blocks, and a network's part does not depend on the others."""
    _c = 'dfq_batch_nsr_plan'

    def __init__(self, batch, widths, per_channel, signed, moment, input_moment):
        g0 = batch.nets[0][0]
        tt = tuple(batch.targ_type)
        layers = [(key, layer.weight, getattr(layer, 'groups', 1)) for key, layer in g0.items() if type(layer) in tt]
        if not layers:
            raise ValueError('nsr_plan: the batch has no {} layer'.format(tt))
        steps, keys = batch._bc.arrays['steps'], [key for key, _, _ in layers]
        ranges = {keys[int(li)]: (int(b), int(c)) for li, b, c in zip(steps['layer'], steps['source_begin'], steps['source_count'])}
        lay = _dfq._NsrLayout('nsr_plan', layers, lambda key, w: batch._in_slot(key, 'weight', w), len(batch.nets),
                              batch._bc.arrays['sources'], ranges, widths, per_channel, signed, moment, input_moment, batch.stage.device)
        super().__init__(batch)
        self._lay = lay
        self.widths, self.per_channel, self.signed = lay.widths, lay.per_channel, lay.signed
        self.moment, self.input_moment = lay.moment, lay.input_moment
        self.keys, self.n_nets, self.n_tensors = lay.keys, lay.n_nets, lay.n_tensors
        self.cost_block, self.row_block, self.signal_block, self.moment_block = lay.cost_block, lay.row_block, lay.signal_block, lay.moment_block
        self._create(lay.tables(), *lay.block_args())

    def costs(self, n):
        """``OrderedDict[graph key -> float64 numpy [B]]``: N of network n's layer at every width of ``widths``"""
        return self._lay.costs(n)

    def rows(self, n):
        """``OrderedDict[graph key -> float64 numpy [O, B]]``: R, the noise-to-signal ratio of every output row"""
        return self._lay.rows(n)

    def signal(self, n):
        """``OrderedDict[graph key -> float64 numpy [O]]``: S, the weighed signal power of every output row"""
        return self._lay.signal(n)

    def moments(self, n):
        """``OrderedDict[graph key -> float32 numpy [g * I/g]]``: a, the moment of every input channel the layer reads"""
        return self._lay.moments(n)


_MX_FP6 = {'e2m3': _ffi.MX_E2M3, 'e3m2': _ffi.MX_E3M2}
_MX_FP8 = {'e4m3': _ffi.MX_E4M3, 'e5m2': _ffi.MX_E5M2}


def _mx_blocks(shape):
    """scale bytes of a weight: rows * ceil(row_len / 32)"""
    rows = int(shape[0])
    return rows * -(-(int(np.prod(shape)) // rows) // _ffi.MX_BLOCK)


class BatchMxPlan(_BatchPlan):
    """MX block-scaled FP4 / FP6 / FP8 quantisation of the weights of every network of a NetworkBatch (dfq_batch_mx_plan,
    include/dfq_hip.h, which holds the definition under "MX block-scaled"): network 0's table of ``targ_type`` weights plus the
    batch's base addresses.  The ERRORS stage (two launches) reads every weight once and writes ``error_block`` float64
    [n_nets, T, F], the sum of squared errors of every layer at every candidate width; the QUANTISE stage (one launch) writes the
    weights in place, ``code_block`` uint8 [n_nets, code_stride] (sign | exponent | mantissa in the low bits of a byte, one per
    weight) and ``scale_block`` uint8 [n_nets, scale_stride] (one E8M0 byte per 32 weights of a row; 255: the block held a NaN
    or an Inf).  ``run()`` is ERRORS and, with ``apply``, QUANTISE (``launches`` of them); ``run(stages)`` any of the two.
    ``cost_block`` is ``error_block``: what ``mixed_plan(costs=)`` allocates on.  The blocks are torch tensors that outlive
    ``close()``.  Two runs give bit-equal blocks, and a network's part does not depend on the others."""
    _c = 'dfq_batch_mx_plan'
    ERRORS, QUANTISE = _ffi.MX_ERRORS, _ffi.MX_QUANTISE

    def __init__(self, batch, widths, bit_weight, fp6, fp8, search, apply, codes):
        try:
            widths = tuple(widths)
        except TypeError:
            raise ValueError('mx_plan: widths must be a rising subset of (4, 6, 8), got {!r}'.format(widths)) from None
        if (not widths or any(isinstance(b, bool) or not isinstance(b, (int, np.integer)) or b not in (4, 6, 8) for b in widths)
                or any(b <= a for a, b in zip(widths, widths[1:]))):
            raise ValueError('mx_plan: widths must be a rising subset of (4, 6, 8), got {!r}'.format(widths))
        if fp6 not in _MX_FP6:
            raise ValueError("mx_plan: fp6 must be 'e2m3' or 'e3m2', got {!r}".format(fp6))
        if fp8 not in _MX_FP8:
            raise ValueError("mx_plan: fp8 must be 'e4m3' or 'e5m2', got {!r}".format(fp8))
        if apply and (isinstance(bit_weight, bool) or not isinstance(bit_weight, (int, np.integer)) or bit_weight not in widths):
            raise ValueError('mx_plan: bit_weight {!r} is none of the widths {!r}'.format(bit_weight, widths))
        g0 = batch.nets[0][0]
        tt = tuple(batch.targ_type)
        layers = [(key, layer.weight) for key, layer in g0.items() if type(layer) in tt]
        if not layers:
            raise ValueError('mx_plan: the batch has no {} layer'.format(tt))
        super().__init__(batch)
        self.widths, self.fp6, self.fp8, self.search, self.apply = tuple(int(b) for b in widths), fp6, fp8, bool(search), bool(apply)
        self.bit_weight = int(bit_weight) if apply else self.widths[0]
        self.per_channel, self.signed = False, False        # (what pack_plan asks of a source: one-byte unsigned codes)
        self.range_block, self._range_views = None, []
        n_nets, dev = len(batch.nets), batch.stage.device
        self.keys, self.n_nets, self.n_tensors = [key for key, _ in layers], n_nets, len(layers)
        self._sizes = OrderedDict((key, w.numel()) for key, w in layers)
        self.elements = sum(self._sizes.values())
        entries, self._code_views, self._scale_views = [], [], []
        code_stride = scale_stride = 0
        for key, w in layers:
            rows = int(w.shape[0])
            c_off = -1
            if codes:
                c_off = code_stride
                self._code_views.append((key, c_off, w.numel(), tuple(w.shape)))
                code_stride += -(-w.numel() // 64) * 64
            n_blk = _mx_blocks(w.shape)
            self._scale_views.append((key, scale_stride, n_blk, (rows, n_blk // rows)))
            entries.append(_ffi.DfqBatchMxTensor(batch._in_slot(key, 'weight', w), rows, w.numel() // rows, c_off, scale_stride))
            scale_stride += -(-n_blk // 16) * 16
        F = len(self.widths)
        self.error_block = torch.zeros((n_nets, self.n_tensors, F), dtype=torch.float64, device=dev)
        self.cost_block = self.error_block
        self.code_dtype = torch.uint8 if codes else None
        self.code_block = torch.zeros((n_nets, code_stride), dtype=torch.uint8, device=dev) if codes else None
        self.scale_block = torch.zeros((n_nets, scale_stride), dtype=torch.uint8, device=dev)
        self.status_block = torch.zeros((n_nets,), dtype=torch.int32, device=dev)
        self.bits_block, self.budget, self._mixed = None, self.elements * self.bit_weight, None
        cfg = _ffi.DfqBatchMxConfig((ctypes.c_int32 * 3)(*(list(self.widths) + [0] * (3 - F))), F, _MX_FP6[fp6], _MX_FP8[fp8],
                                    int(self.search), int(self.apply), self.bit_weight, 0)
        arr = (_ffi.DfqBatchMxTensor * len(entries))(*entries)
        self._create((arr, len(entries), ctypes.byref(cfg)), self.error_block.data_ptr(),
                     None if self.code_block is None else self.code_block.data_ptr(), code_stride, self.scale_block.data_ptr(), scale_stride)

    def run(self, stages=None):
        """Enqueue the plan on the current stream.  ``stages=None``: ERRORS and, with ``apply``, QUANTISE.  Else
        ``BatchMxPlan.ERRORS``, ``QUANTISE`` or their sum (dfq_batch_mx_plan_run_stages), whatever ``apply`` says."""
        if stages is None:
            return super().run()
        if self._batch.storage is None:
            raise RuntimeError('NetworkBatch: the batch has been released')
        if not self._plan:
            raise RuntimeError('BatchMxPlan: the plan has been closed')
        _ffi.check(_ffi.lib().dfq_batch_mx_plan_run_stages(self._plan, int(stages), _ffi.stream_arg()))

    def set_widths(self, mixed):
        """Quantise every layer of every network at the width read on the device by every later QUANTISE
        (dfq_batch_mx_plan_set_widths): ``mixed`` is a BatchMixedPlan of this batch whose widths are all candidates of this plan
        -- its ``bits_block`` is read --, or an int32 tensor [n_nets, T] on the batch's device in the order of ``keys``.  A width
        that is no candidate leaves that layer of that network untouched and makes ``status(n)`` 2.  None: at ``bit_weight``
        again.  The call synchronises; a ``pack_plan`` made of this plan before it refuses to run."""
        if not self._plan:
            raise RuntimeError('BatchMxPlan: the plan has been closed')
        lib = _ffi.lib()
        if mixed is None:
            _ffi.check(lib.dfq_batch_mx_plan_set_widths(self._plan, None, 0, None, None))
            self.bits_block, self.budget, self._mixed = None, self.elements * self.bit_weight, None
            return
        if isinstance(mixed, BatchMixedPlan):
            if mixed._batch is not self._batch:
                raise ValueError('mx_plan: set_widths got a mixed_plan of another batch')
            if not set(mixed.widths) <= set(self.widths):
                raise ValueError('mx_plan: the widths {!r} of the mixed_plan are not all among {!r}'.format(mixed.widths, self.widths))
            if list(mixed.keys) != self.keys:               # (pack_plan reads column i of the block for tensor i of this plan)
                raise ValueError('mx_plan: the layers of the mixed_plan are not this plan\'s, in its order')
            order, block, budget = list(range(self.n_tensors)), mixed.bits_block, mixed.budget
        elif isinstance(mixed, torch.Tensor):
            if mixed.dtype != torch.int32 or tuple(mixed.shape) != (self.n_nets, self.n_tensors) or not mixed.is_contiguous() \
                    or mixed.device != self.status_block.device:
                raise ValueError('mx_plan: a width block must be a contiguous int32 tensor [{}, {}] on {}'.format(
                    self.n_nets, self.n_tensors, self.status_block.device))
            order, block, budget = list(range(self.n_tensors)), mixed, self.elements * self.widths[-1]
        else:
            raise ValueError('mx_plan: set_widths takes a mixed_plan of this batch, an int32 tensor or None, got {!r}'.format(
                type(mixed).__name__))
        index = (ctypes.c_int32 * self.n_tensors)(*order)
        _ffi.check(lib.dfq_batch_mx_plan_set_widths(self._plan, block.data_ptr(), block.shape[1], index, self.status_block.data_ptr()))
        self.bits_block, self.budget, self._mixed = block, budget, mixed       # (kept alive while the plan reads it)

    def status(self, n):
        """0, or 2: a width network n's row of the device block held at the last QUANTISE was none of ``widths``, and that layer
        was left as it was; always 0 without device widths"""
        return int(self.status_block[n].cpu())

    def codes(self, n):
        """{graph key: uint8 codes of network n's weight, shaped like it} -- views of the code block; {} without codes"""
        if self.code_block is None:
            return {}
        row = self.code_block[n]
        return OrderedDict((key, row[off:off + numel].view(shape)) for (key, off, numel, shape) in self._code_views)

    def scales(self, n):
        """{graph key: uint8 [rows, ceil(row_len / 32)]}: the scale bytes of network n's weight -- views of the scale block"""
        row = self.scale_block[n]
        return OrderedDict((key, row[off:off + n_blk].view(shape)) for (key, off, n_blk, shape) in self._scale_views)

    def errors(self, n):
        """``OrderedDict[graph key -> float64 numpy [F]]``: sum e^2 of network n's weight at every width of ``widths``"""
        e = self.error_block[n].cpu().numpy()
        return OrderedDict((key, e[i].copy()) for i, key in enumerate(self.keys))


_PACKED_VERSION = 1            # of the file save_packed writes
_PACKED_MX_VERSION = 2         # of the file save_packed writes for an MX source (mx_scales, mx_format6, mx_format8, mx_block)
_PACK_MAX_BITS = 16


def _range_floats(shape):
    """floats of a range view: a pair per row ([O, 2]) or one pair ([2])"""
    return 2 * (shape[0] if len(shape) == 2 else 1)


def _extent_words(numel, bits):
    """words of one tensor's stream: ceil(numel * bits / 32) rounded up to 4 (include/dfq_hip.h)"""
    words = -(-numel * bits // 32)
    return -(-words // 4) * 4


class _MxScales:
    """What MX-packed words need besides themselves: ``scale_block`` uint8 [n_nets, scale_stride], its views
    [(key, offset, blocks, (rows, blocks per row))] and the formats of the 6- and 8-bit codes ('e2m3' / 'e3m2', 'e4m3' / 'e5m2')"""

    def __init__(self, scale_block, views, fp6, fp8):
        self.scale_block, self.views, self.fp6, self.fp8 = scale_block, list(views), fp6, fp8


class _Packed:
    """What a BatchPackPlan and a loaded PackedBatch share -- the packed words of a batch and what unpacking them needs:
    ``packed_block`` int32 [n_nets, word_stride] (the raw uint32 words), ``offset_block`` int64 [n_nets, T + 1],
    ``status_block`` int32 [n_nets], ``range_block`` float32 [n_nets, range_stride], the widths -- one for all (``bits``), or
    ``bits_block`` int32 [n_nets, T] on the device (``bits == 0``) --, ``keys``, ``per_channel`` and ``signed``.  ``mx``: None,
    or the _MxScales of words that hold MX codes (``range_block`` is then None)."""
    mx = None

    def words(self, n):
        """``OrderedDict[graph key -> int32 view]`` of network n's packed words, tensor by tensor (one device-to-host copy of
        its offsets); reinterpret as uint32 on the host (``.cpu().numpy().view(numpy.uint32)``)"""
        off = self.offset_block[n].cpu().tolist()
        row = self.packed_block[n]
        return OrderedDict((key, row[off[i]:off[i + 1]]) for i, key in enumerate(self.keys))

    def size_bits(self, n):
        """bits network n's packed words take: 32 * offset[n][T]"""
        return 32 * int(self.offset_block[n, -1].cpu())

    def status(self, n):
        """0: packed; 1: ``word_stride`` is too small (``size_bits(n)`` says what it takes); 2: a width on the device is no
        width"""
        return int(self.status_block[n].cpu())

    def widths_array(self):
        """int32 numpy [n_nets, T]: the width of every tensor of every network"""
        if self.bits:
            return np.full((self.n_nets, len(self.keys)), self.bits, dtype=np.int32)
        return self.bits_block.cpu().numpy().astype(np.int32)


class BatchPackPlan(_BatchPlan, _Packed):
    """Dense bit-packing of the codes a quant, squant or mixed plan of a NetworkBatch wrote (dfq_batch_pack_plan,
    include/dfq_hip.h, which holds the definition).  ``run()`` enqueues two launches on the current stream -- the offsets, one
    workgroup per network, then the packing -- and nothing goes to the host.  The plan owns ``packed_block``,
    ``offset_block`` and ``status_block`` (torch tensors that outlive ``close()``); the codes, the ranges and, for a mixed
    source, the widths stay the source's blocks."""
    _c = 'dfq_batch_pack_plan'

    def __init__(self, batch, source, word_stride):
        if not isinstance(source, (BatchQuantPlan, BatchSquantPlan, BatchMixedPlan, BatchMxPlan)):
            raise ValueError('pack_plan: the source must be a quant_plan, squant_plan, mixed_plan or mx_plan, got {!r}'.format(
                type(source).__name__))
        if source._batch is not batch:
            raise ValueError('pack_plan: the source is a plan of another batch')
        if not source._plan:
            raise ValueError('pack_plan: the source plan has been closed')
        if source.code_block is None:
            raise ValueError('pack_plan: the source was created without codes')
        mixed = isinstance(source, BatchMixedPlan)
        if mixed and not source.apply:
            raise ValueError('pack_plan: a mixed plan created with apply=False writes no codes')
        layered = mixed or getattr(source, 'bits_block', None) is not None       # a width per (network, layer), on the device
        views = source._lay._code_views if mixed else source._code_views
        range_views = source._lay._range_views if mixed else source._range_views
        if word_stride is not None and (isinstance(word_stride, bool) or not isinstance(word_stride, (int, np.integer)) or word_stride < 0):
            raise ValueError('pack_plan: word_stride must be an int >= 0, got {!r}'.format(word_stride))
        super().__init__(batch)
        self._source = source                                           # (its blocks are read by every run)
        self.keys = [key for (key, _, _, _) in views]
        self._views = [(key, numel, shape) for (key, _, numel, shape) in views]
        wanted = set(self.keys)
        self._range_views = [v for v in range_views if v[0] in wanted]  # (a quant plan's bias ranges are not the weights')
        self.per_channel, self.signed = source.per_channel, source.signed
        self.range_block, self.code_block, self.code_dtype = source.range_block, source.code_block, source.code_dtype
        self.n_nets, self.n_tensors = len(batch.nets), len(views)
        # an MX source: the scale bytes and the two format ids travel with the words (unpack_plan decodes with them)
        self.mx = _MxScales(source.scale_block, source._scale_views, source.fp6, source.fp8) if isinstance(source, BatchMxPlan) else None
        self.bits = 0 if layered else int(source.bit_weight)
        self.bits_block = source.bits_block if layered else None
        if not layered and not 1 <= self.bits <= _PACK_MAX_BITS:
            raise ValueError('pack_plan: codes of {} bits; the packing takes 1 to {}'.format(self.bits, _PACK_MAX_BITS))
        if word_stride is None:
            if layered:
                word_stride = -(-(-(-source.budget // 32) + 5 * self.n_tensors) // 4) * 4     # (every row on a 16-byte boundary)
            else:
                word_stride = sum(_extent_words(numel, self.bits) for (_, numel, _) in self._views)
        self.word_stride = int(word_stride)
        dev = batch.stage.device
        self.packed_block = torch.empty((self.n_nets, self.word_stride), dtype=torch.int32, device=dev)
        self.offset_block = torch.zeros((self.n_nets, self.n_tensors + 1), dtype=torch.int64, device=dev)
        self.status_block = torch.zeros((self.n_nets,), dtype=torch.int32, device=dev)
        P = _ffi.DfqBatchPackTensor
        arr = (P * self.n_tensors)(*[P(off, numel, self.bits, i, int(self.signed), 0) for i, (_, off, numel, _) in enumerate(views)])
        self._create((arr, self.n_tensors), self.code_block.data_ptr(), self.code_block.element_size(), self.code_block.shape[1],
                     None if self.bits_block is None else self.bits_block.data_ptr(), self.n_tensors,
                     self.packed_block.data_ptr(), self.word_stride, self.offset_block.data_ptr(), self.status_block.data_ptr())


    def run(self):
        """Enqueue the two launches.  RuntimeError if the source's widths have been set anew since this plan was made
        (``BatchSquantPlan.set_widths``): the plan would pack at the widths of then."""
        if getattr(self._source, 'bits_block', None) is not self.bits_block:
            raise RuntimeError('pack_plan: the widths of the source plan have changed since this plan was made; make a new pack_plan')
        super().run()


class PackedBatch(_Packed):
    """The blocks of a file ``NetworkBatch.save_packed`` wrote, uploaded for ``batch``: what ``NetworkBatch.load_packed``
    returns and ``NetworkBatch.unpack_plan`` takes.  ValueError for an unknown version and for keys, shapes or a number of
    networks that are not the batch's."""

    def __init__(self, batch, path):
        with np.load(path, allow_pickle=False) as f:
            if 'version' not in f.files or int(f['version']) not in (_PACKED_VERSION, _PACKED_MX_VERSION):
                raise ValueError('load_packed: {} has format version {}, this library reads versions {} and {} (MX)'.format(
                    path, int(f['version']) if 'version' in f.files else None, _PACKED_VERSION, _PACKED_MX_VERSION))
            is_mx = int(f['version']) == _PACKED_MX_VERSION
            need = ['keys', 'shapes', 'offsets', 'widths', 'per_channel', 'signed', 'bias_keys', 'biases']
            need += ['mx_scales', 'mx_format6', 'mx_format8', 'mx_block'] if is_mx else ['ranges']
            need += ['words_{}'.format(n) for n in range(len(batch.nets))]
            missing = [k for k in need if k not in f.files]
            if missing:
                raise ValueError('load_packed: {} is no file of save_packed (it has no {!r})'.format(path, missing[0]))
            data = {k: f[k] for k in f.files}
        g0, tt = batch.nets[0][0], tuple(batch.targ_type)
        mine = [(k, tuple(int(d) for d in m.weight.shape)) for k, m in g0.items() if type(m) in tt]
        keys = [str(k) for k in data['keys']]
        shapes = [tuple(int(d) for d in row if d) for row in data['shapes']]
        if keys != [k for k, _ in mine] or shapes != [s for _, s in mine]:
            raise ValueError('load_packed: {} holds another architecture (its keys or shapes are not this batch\'s)'.format(path))
        offsets, widths = data['offsets'].astype(np.int64), data['widths'].astype(np.int32)
        n_nets, T = len(batch.nets), len(keys)
        if offsets.shape != (n_nets, T + 1) or widths.shape != (n_nets, T):
            raise ValueError('load_packed: {} holds {} networks of {} tensors, the batch has {} of {}'.format(
                path, offsets.shape[0], offsets.shape[1] - 1, n_nets, T))
        self.keys, self.n_nets, self.n_tensors = keys, n_nets, T
        self._views = [(k, int(np.prod(s)), s) for k, s in zip(keys, shapes)]
        self.per_channel, self.signed = bool(data['per_channel']), bool(data['signed'])
        self._range_views, at = [], 0
        dev = batch.stage.device
        if is_mx:
            fp6 = {v: k for k, v in _MX_FP6.items()}.get(int(data['mx_format6']))
            fp8 = {v: k for k, v in _MX_FP8.items()}.get(int(data['mx_format8']))
            if int(data['mx_block']) != _ffi.MX_BLOCK or fp6 is None or fp8 is None:
                raise ValueError('load_packed: {}: MX block length {} or format ids ({}, {}) this library does not read'.format(
                    path, int(data['mx_block']), int(data['mx_format6']), int(data['mx_format8'])))
            views = []
            for k, s in zip(keys, shapes):
                views.append((k, at, _mx_blocks(s), (s[0], _mx_blocks(s) // s[0])))
                at += _mx_blocks(s)
            scales = np.ascontiguousarray(data['mx_scales'], dtype=np.uint8)
            if scales.shape != (n_nets, at):
                raise ValueError('load_packed: {} holds {} scale bytes per network, the batch needs {}'.format(path, scales.shape[-1], at))
            self.mx = _MxScales(torch.from_numpy(scales).to(dev), views, fp6, fp8)
            ranges = None
        else:
            for k, s in zip(keys, shapes):
                shape = (s[0], 2) if self.per_channel else (2,)
                self._range_views.append((k, at, shape))
                at += _range_floats(shape)
            ranges = np.ascontiguousarray(data['ranges'], dtype=np.float32)
            if ranges.shape != (n_nets, at):
                raise ValueError('load_packed: {} holds {} range values per network, the batch needs {}'.format(path, ranges.shape[-1], at))
        words = [np.ascontiguousarray(data['words_{}'.format(n)]).view(np.uint32) for n in range(n_nets)]
        if any(len(w) != int(offsets[n, -1]) for n, w in enumerate(words)):
            raise ValueError('load_packed: {}: a network\'s words are not as many as its offsets say'.format(path))
        self.word_stride = max(4, max(len(w) for w in words))
        host = np.zeros((n_nets, self.word_stride), dtype=np.uint32)
        for n, w in enumerate(words):
            host[n, :len(w)] = w
        self.packed_block = torch.from_numpy(host.view(np.int32)).to(dev)
        self.offset_block = torch.from_numpy(offsets).to(dev)
        self.status_block = torch.zeros((n_nets,), dtype=torch.int32, device=dev)
        self.range_block = None if ranges is None else torch.from_numpy(ranges).to(dev)
        self.bits, self.bits_block = 0, torch.from_numpy(widths).to(dev)
        self._bias_keys = [str(k) for k in data['bias_keys']]
        self._biases = np.ascontiguousarray(data['biases'], dtype=np.float32)
        want = [k for k in keys if g0[k].bias is not None]
        if self._bias_keys != want or self._biases.shape != (n_nets, sum(g0[k].bias.numel() for k in want)):
            raise ValueError('load_packed: {}: its biases are not this batch\'s'.format(path))


class BatchUnpackPlan(_BatchPlan):
    """The way back from packed words (dfq_batch_unpack_plan, include/dfq_hip.h): one launch that rebuilds, for every network
    of a NetworkBatch, the weights in place (``weights``) and / or the integer codes (``codes``: 'int32' or 'int8') in
    ``code_block``, a block the plan owns (``codes(n)``).  ``status_block`` int32 [n_nets]: 0, or why a network was skipped."""
    _c = 'dfq_batch_unpack_plan'

    def __init__(self, batch, packed, weights, codes):
        if not isinstance(packed, _Packed):
            raise ValueError('unpack_plan: packed must be a pack_plan or a loaded PackedBatch, got {!r}'.format(type(packed).__name__))
        if codes not in (None, 'int32', 'int8'):
            raise ValueError("unpack_plan: codes must be None, 'int32' or 'int8', got {!r}".format(codes))
        if not weights and codes is None:
            raise ValueError('unpack_plan: nothing to unpack to (weights=False and codes=None)')
        if codes == 'int8' and packed.bits > 8:
            raise ValueError('unpack_plan: 1-byte codes need widths <= 8, got {}'.format(packed.bits))
        g0, tt = batch.nets[0][0], tuple(batch.targ_type)
        mine = [(k, tuple(m.weight.shape)) for k, m in g0.items() if type(m) in tt]
        if [(k, tuple(s)) for (k, _, s) in packed._views] != mine:
            raise ValueError('unpack_plan: the packed keys or shapes are not this batch\'s')
        if packed.packed_block.shape[0] != len(batch.nets):
            raise ValueError('unpack_plan: packed holds {} networks, the batch has {}'.format(packed.packed_block.shape[0], len(batch.nets)))
        super().__init__(batch)
        self._packed = packed
        self.keys, self.n_nets, self.n_tensors = list(packed.keys), len(batch.nets), len(packed.keys)
        self.per_channel, self.signed = packed.per_channel, packed.signed
        self._decode = self.decode_status_block = None
        if packed.mx is not None:
            if codes == 'int32':
                raise ValueError("unpack_plan: MX codes are one byte wide (codes=None or 'int8')")
            self._init_mx(batch, packed, weights, g0)
            return
        dev = batch.stage.device
        rng = {key: off for (key, off, _) in packed._range_views}
        entries, self._code_views, code_stride = [], [], 0
        P = _ffi.DfqBatchUnpackTensor
        for i, (key, numel, shape) in enumerate(packed._views):
            w = g0[key].weight
            rows = int(shape[0])
            entries.append(P(batch._in_slot(key, 'weight', w) if weights else None, rows, numel // rows, code_stride, numel, rng[key],
                             packed.bits, i, int(self.signed), int(self.per_channel)))
            self._code_views.append((key, code_stride, numel, tuple(shape)))
            code_stride += -(-numel // 64) * 64
        dtype = {None: None, 'int32': torch.int32, 'int8': torch.int8 if self.signed else torch.uint8}[codes]
        self.code_dtype = dtype
        self.code_block = torch.empty((self.n_nets, code_stride), dtype=dtype, device=dev) if codes is not None else None
        self.status_block = torch.zeros((self.n_nets,), dtype=torch.int32, device=dev)
        arr = (P * len(entries))(*entries)
        self._create((arr, len(entries)), packed.packed_block.data_ptr(), packed.packed_block.shape[1], packed.offset_block.data_ptr(),
                     None if packed.bits_block is None else packed.bits_block.data_ptr(), self.n_tensors,
                     packed.range_block.data_ptr(), packed.range_block.shape[1],
                     None if self.code_block is None else self.code_block.data_ptr(), 1 if codes == 'int8' else 4, code_stride,
                     self.status_block.data_ptr())

    def _init_mx(self, batch, packed, weights, g0):
        """MX-packed words: the unpack launch to one-byte codes in ``code_block`` (always kept: the decode reads them), then, with
        ``weights``, one decode launch (dfq_batch_mx_decode_plan) from the codes and the scale bytes to the weights in place.
        ``decode_status_block`` is the second launch's status.  The decode launch is gated on ``status_block``: a network the
        unpack launch skipped is not decoded, its weights stay as they were, as on the integer path."""
        dev, lib = batch.stage.device, _ffi.lib()
        P, D = _ffi.DfqBatchUnpackTensor, _ffi.DfqBatchMxDecodeTensor
        scale_at = {key: off for (key, off, _, _) in packed.mx.views}
        entries, decode, self._code_views, code_stride = [], [], [], 0
        for i, (key, numel, shape) in enumerate(packed._views):
            rows = int(shape[0])
            entries.append(P(None, rows, numel // rows, code_stride, numel, -1, packed.bits, i, 0, 0))
            if weights:
                decode.append(D(batch._in_slot(key, 'weight', g0[key].weight), rows, numel // rows, code_stride, scale_at[key], packed.bits, i))
            self._code_views.append((key, code_stride, numel, tuple(shape)))
            code_stride += -(-numel // 64) * 64
        self.code_dtype = torch.uint8
        self.code_block = torch.zeros((self.n_nets, code_stride), dtype=torch.uint8, device=dev)
        self.status_block = torch.zeros((self.n_nets,), dtype=torch.int32, device=dev)
        self.decode_status_block = torch.zeros((self.n_nets,), dtype=torch.int32, device=dev)
        widths = None if packed.bits_block is None else packed.bits_block.data_ptr()
        arr = (P * len(entries))(*entries)
        self._create((arr, len(entries)), packed.packed_block.data_ptr(), packed.packed_block.shape[1], packed.offset_block.data_ptr(),
                     widths, self.n_tensors, None, 0, self.code_block.data_ptr(), 1, code_stride, self.status_block.data_ptr())
        if weights:
            darr = (D * len(decode))(*decode)
            handle = ctypes.c_void_p()
            scales = packed.mx.scale_block
            try:
                _ffi.check(lib.dfq_batch_mx_decode_plan_create(darr, len(decode), batch.bases.ctypes.data_as(ctypes.POINTER(ctypes.c_void_p)),
                                                               self.n_nets, self.code_block.data_ptr(), code_stride, scales.data_ptr(),
                                                               scales.shape[1], widths, self.n_tensors, _MX_FP6[packed.mx.fp6],
                                                               _MX_FP8[packed.mx.fp8], self.status_block.data_ptr(),
                                                               self.decode_status_block.data_ptr(), ctypes.byref(handle)))
            except Exception:
                self.close()                                # (the unpack plan made above)
                raise
            self._decode = handle
            self.launches += int(lib.dfq_batch_mx_decode_plan_launches(handle))

    def run(self):
        """Enqueue the unpack launch and, for MX-packed words with ``weights``, the decode launch behind it."""
        super().run()
        if self._decode:
            _ffi.check(_ffi.lib().dfq_batch_mx_decode_plan_run(self._decode, _ffi.stream_arg()))

    def close(self):
        if getattr(self, '_decode', None):
            _ffi.lib().dfq_batch_mx_decode_plan_destroy(self._decode)
            self._decode = None
        super().close()

    def codes(self, n):
        """{graph key: integer codes of network n's weight, shaped like it} -- views of the code block; {} without codes"""
        if self.code_block is None:
            return {}
        row = self.code_block[n]
        return OrderedDict((key, row[off:off + numel].view(shape)) for (key, off, numel, shape) in self._code_views)

    def statuses(self):
        """[n_nets] ints, one device-to-host copy: ``status(n)`` of every network"""
        block = self.status_block
        if self.decode_status_block is not None:            # (MX-packed words: the decode launch has a status of its own)
            block = torch.maximum(block, self.decode_status_block)
        return block.cpu().tolist()

    def status(self, n):
        """0, or 1 / 2: network n was skipped (its offsets do not fit its widths / a width on the device is no width)"""
        return self.statuses()[n]


def _kernel_len(w):
    """kH * kW of a convolution's weight, 1 for a Linear one"""
    k = 1
    for d in w.shape[2:]:
        k *= int(d)
    return k


class BatchFoldPlan(_BatchPlan):
    """BatchNorm folding of every network of a NetworkBatch made by ``from_unfolded`` (dfq_batch_fold_plan,
    include/dfq_hip.h): network 0's (layer, BatchNorm) pair table plus the batch's base addresses.  ``run()`` enqueues two
    launches on the current stream -- the weights, then the per-channel vectors -- and marks the batch folded; weights,
    biases, the proxies and the BatchNorm vectors change in place.  ``bn.eps`` is read here, when the plan is made, and left
    alone (``NetworkBatch.merge_batchnorm`` sets it)."""
    _c = 'dfq_batch_fold_plan'

    def __init__(self, batch):
        super().__init__(batch)
        g0 = batch.nets[0][0]

        def at(key, name):
            t = _dfq._attr(g0[key], name)
            if t is None:
                raise RuntimeError('NetworkBatch: {} of {} in network 0 no longer lives in its slot of the batch allocation'.format(
                    name, key))
            return batch._in_slot(key, name, t)
        entries = []
        for lk, bk in batch._fold:
            w = g0[lk].weight
            entries.append(_ffi.DfqBatchFoldPair(at(lk, 'weight'), at(lk, 'bias'), *[at(bk, name) for name in _BN_VECTORS],
                                                 at(bk, 'fake_weight'), at(bk, 'fake_bias'), w[0].numel(), int(w.shape[0]),
                                                 float(g0[bk].eps)))
        if not entries:
            raise ValueError('fold_plan: no BatchNorm of the batch follows a {} layer'.format(tuple(batch.targ_type)))
        self.n_nets, self.n_pairs = len(batch.nets), len(entries)
        self._create(((_ffi.DfqBatchFoldPair * len(entries))(*entries), len(entries)))
        self.elements = int(_ffi.lib().dfq_batch_fold_plan_elements(self._plan))      # folded weights per network

    def run(self):
        batch = self._batch
        if batch.storage is not None and self._plan and batch.folded:
            raise RuntimeError('BatchFoldPlan: the batch is folded already (a second fold would take the identity BatchNorms '
                               'for the real ones and overwrite the proxies with 1 and 0)')
        super().run()
        batch.folded = True


class BatchTablePlan(_BatchPlan):
    """The weight statistics of the ncnn calibration table for every network of a NetworkBatch (dfq_batch_table_plan,
    include/dfq_hip.h): network 0's table of ``targ_type`` weights plus the batch's base addresses.  ``run()`` enqueues on
    the current stream -- a clear of ``self.block`` and two launches; it reads every weight once and writes only
    ``self.block``, float32 [n_nets, stride]: per weight its (min, max), per output row its max|w|.  The block is a torch
    tensor and outlives ``close()``."""
    _c = 'dfq_batch_table_plan'

    def __init__(self, batch):
        super().__init__(batch)
        g0 = batch.nets[0][0]
        tt = tuple(batch.targ_type)
        layers = [(key, layer.weight) for key, layer in g0.items() if type(layer) in tt]
        if not layers:
            raise ValueError('table_plan: the batch has no {} layer'.format(tt))
        entries, self._views = [], []          # (graph key, offset of (min, max), offset of the rows' max|w|, rows)
        stride = 2 * len(layers)               # the pairs first, then the rows of every weight
        for i, (key, w) in enumerate(layers):
            rows = int(w.shape[0])
            entries.append(_ffi.DfqBatchTableTensor(batch._in_slot(key, 'weight', w), rows, w.numel() // rows, 2 * i, stride))
            self._views.append((key, 2 * i, stride, rows))
            stride += rows
        self.keys = [key for key, _ in layers]
        self.n_nets, self.n_tensors = len(batch.nets), len(entries)
        self.elements = sum(w.numel() for _, w in layers)               # weights per network, each read once (4 B)
        self.block = torch.zeros((self.n_nets, stride), dtype=torch.float32, device=batch.stage.device)
        self._create(((_ffi.DfqBatchTableTensor * len(entries))(*entries), len(entries)), self.block.data_ptr(), stride)

    def ranges(self, n):
        """{graph key: float32 [2] view (min, max) of network n's weight} -- what ``ncnn_table.weight_ranges`` gives"""
        row = self.block[n]
        return OrderedDict((key, row[r_off:r_off + 2]) for (key, r_off, _, _) in self._views)

    def row_absmax(self, n):
        """{graph key: float32 [O] view, max|w| of every output row of network n's weight} -- ``prims.row_range(w, signed=True)``"""
        row = self.block[n]
        return OrderedDict((key, row[a_off:a_off + rows]) for (key, _, a_off, rows) in self._views)


class BatchErrorPlan(_BatchPlan):
    """The weight quantisation error of every network of a NetworkBatch under one to four quantiser configurations
    (dfq_batch_error_plan, include/dfq_hip.h): network 0's table of ``targ_type`` weights plus the batch's base addresses.
    ``run()`` enqueues on the current stream -- a clear of the plan's range words and three launches; it reads every weight
    twice and writes only ``self.block``, float64 [n_nets, stride]: per weight ``1 + 3 * len(configs)`` sums.  Two runs give
    bit-equal blocks, and a network's part does not depend on the others.  The block is a torch tensor and outlives
    ``close()``.  ``self.configs``: the configurations as (bit_weight, per_channel, signed) with the bit width as an int."""
    _c = 'dfq_batch_error_plan'

    def __init__(self, batch, configs):
        try:
            configs = [tuple(c) for c in configs]
        except TypeError:
            raise ValueError('error_plan: configs must be a sequence of (bit_weight, per_channel, signed)') from None
        if not 1 <= len(configs) <= 4 or any(len(c) != 3 for c in configs):
            raise ValueError('error_plan: one to four configurations (bit_weight, per_channel, signed), got {!r}'.format(configs))
        checked = []
        for bits, per_channel, signed in configs:
            bits = _check_bits(bits, per_channel, 'bit_weight')
            if signed and bits == 1:
                raise ValueError('error_plan: signed with bit_weight 1 has qmax = 0')
            checked.append((bits, bool(per_channel), bool(signed)))
        super().__init__(batch)
        g0 = batch.nets[0][0]
        tt = tuple(batch.targ_type)
        layers = [(key, layer.weight) for key, layer in g0.items() if type(layer) in tt]
        if not layers:
            raise ValueError('error_plan: the batch has no {} layer'.format(tt))
        self.configs = checked
        n_vals = 1 + 3 * len(checked)
        entries, self._views = [], []          # (graph key, offset of the sums, numel)
        for i, (key, w) in enumerate(layers):
            rows = int(w.shape[0])
            entries.append(_ffi.DfqBatchErrorTensor(batch._in_slot(key, 'weight', w), rows, w.numel() // rows, n_vals * i))
            self._views.append((key, n_vals * i, w.numel()))
        stride = n_vals * len(layers)
        self.keys = [key for key, _ in layers]
        self.n_nets, self.n_tensors = len(batch.nets), len(entries)
        self.elements = sum(w.numel() for _, w in layers)               # weights per network, each read twice (8 B)
        self.block = torch.zeros((self.n_nets, stride), dtype=torch.float64, device=batch.stage.device)
        cfg = (_ffi.DfqBatchErrorConfig * len(checked))(*[_ffi.DfqBatchErrorConfig(b, int(s), int(pc), 0) for b, pc, s in checked])
        self._create(((_ffi.DfqBatchErrorTensor * len(entries))(*entries), len(entries), cfg, len(checked)),
                     self.block.data_ptr(), stride)

    def errors(self, n, block=None):
        """``OrderedDict[graph key -> dict]`` of network n: ``numel``, ``sum_sq_w`` = sum w^2 and, as float64 arrays with one
        entry per configuration, ``sum`` = sum e, ``sum_abs`` = sum |e|, ``sum_sq`` = sum e^2.  One device-to-host copy
        (of the network's part of the block); ``block``: a host copy of ``self.block`` the caller made already."""
        row = (self.block[n].cpu() if block is None else block[n]).numpy()
        out, k = OrderedDict(), len(self.configs)
        for key, off, numel in self._views:
            sums = row[off + 1:off + 1 + 3 * k].reshape(k, 3)
            out[key] = {'numel': numel, 'sum_sq_w': float(row[off]), 'sum': sums[:, 0].copy(), 'sum_abs': sums[:, 1].copy(),
                        'sum_sq': sums[:, 2].copy()}
        return out


class BatchClipPlan(_BatchPlan):
    """MSE-optimal weight clipping of every network of a NetworkBatch (dfq_batch_clip_plan, include/dfq_hip.h, which holds
    the definition): network 0's table of ``targ_type`` weights plus the batch's base addresses.  ``run()`` enqueues on the
    current stream -- one launch for the units searched in registers and the long rows, three more (four with ``apply``) for
    per-tensor tensors cut into flat pieces; with ``apply`` the weights are clamped in place, and only where the clamp
    changes them.  The results lie in blocks the plan owns, torch tensors that outlive ``close()``: ``range_block`` float32
    [n_nets, units, 2], ``chosen_block`` int32 [n_nets, units] and, with ``keep_errors``, ``error_block`` float64
    [n_nets, units, candidates]; a unit is a tensor, or an output row with ``per_channel``.  Two runs of a plan without
    ``apply`` give bit-equal blocks, and a network's part does not depend on the others."""
    _c = 'dfq_batch_clip_plan'

    def __init__(self, batch, bit_weight, per_channel, signed, candidates, alpha_min, apply, keep_errors):
        cfg = _dfq._clip_config('clip_plan', bit_weight, per_channel, signed, candidates, alpha_min, apply)
        super().__init__(batch)
        g0 = batch.nets[0][0]
        tt = tuple(batch.targ_type)
        layers = [(key, layer.weight) for key, layer in g0.items() if type(layer) in tt]
        if not layers:
            raise ValueError('clip_plan: the batch has no {} layer'.format(tt))
        self.bit_weight, self.per_channel, self.signed = int(cfg.num_bits), bool(cfg.per_row), bool(cfg.symmetric)
        self.candidates, self.alpha_min, self.apply = int(cfg.candidates), float(cfg.alpha_min), bool(cfg.apply)
        self.keys = [key for key, _ in layers]
        self.n_nets, self.n_tensors = len(batch.nets), len(layers)
        self.elements = sum(w.numel() for _, w in layers)               # weights per network
        lay = self._lay = _dfq._ClipLayout([(key, batch._in_slot(key, 'weight', w), int(w.shape[0]), w.numel() // int(w.shape[0]))
                                            for key, w in layers], self.n_nets, cfg, keep_errors, batch.stage.device)
        self.range_block, self.chosen_block, self.error_block = lay.range_block, lay.chosen_block, lay.error_block
        self._create((lay.table, len(layers), ctypes.byref(cfg)), *lay.block_args())

    def ranges(self, n):
        """{graph key: float32 [2] (or [O, 2] per channel) view, the chosen (l, h) of network n's weight}"""
        return self._lay.ranges(n)

    def chosen(self, n):
        """{graph key: int32 0-dim (or [O]) view, k* of network n's weight: 0 is the unit's own (min, max)}"""
        return self._lay.chosen(n)

    def errors(self, n):
        """{graph key: float64 [K] (or [O, K]) view, sum e^2 under every candidate}; RuntimeError without ``keep_errors``"""
        return self._lay.errors(n)

    def report(self, n):
        """``OrderedDict[key -> {'range', 'chosen', 'err_minmax', 'err'}]`` of network n (``keep_errors`` plans)"""
        if self.error_block is None:
            raise RuntimeError('clip_plan: the errors were not kept (keep_errors=True)')
        return self._lay.report(n)


class BatchAbsorbPlan(_BatchPlan):
    """Bias absorption and weight clipping of every network of a NetworkBatch (dfq_batch_absorb_plan, include/dfq_hip.h):
    network 0's relation table plus the batch's base addresses.  ``run()`` enqueues on the current stream; biases, the
    BatchNorm proxies' ``fake_bias`` and the clipped weights change in place, the shift vectors c = max(0, beta~ - N gamma~)
    every update used are kept in a block [n_nets, stride] the plan owns (``shifts(n)``)."""
    _c = 'dfq_batch_absorb_plan'

    def __init__(self, batch, N, range_clip, absorb):
        n_sigma = _finite(N, 'absorb_plan')
        lo = hi = 0.0
        if range_clip is not None:
            try:
                lo, hi = (float(v) for v in range_clip)
            except (TypeError, ValueError):
                raise ValueError('absorb_plan: range_clip {!r} is not a pair of numbers'.format(range_clip)) from None
            if not lo <= hi:
                raise ValueError('absorb_plan: range_clip {!r} is not a range lo <= hi'.format(range_clip))
        super().__init__(batch)
        n_nets = len(batch.nets)
        g0, b0, r0 = batch.nets[0]
        tt = tuple(batch.targ_type)
        in_slot = batch._in_slot
        rels, self._shift_views = [], []
        stride = 0
        for idx, rr in enumerate(r0 if absorb else ()):
            kf, ks, kb = rr.get_idxs()
            if not _dfq._relu_between(g0, b0, ks, kf):          # dfq.py:131-139
                continue
            first, second = g0[kf], g0[ks]
            for key, layer in ((ks, second), (kf, first)):
                if layer.bias is None:
                    raise ValueError('absorb_plan: layer {} of an absorbed relation has no bias in the batch allocation'.format(key))
            fw, fb = _dfq._attr(g0[kb], 'fake_weight'), _dfq._attr(g0[kb], 'fake_bias')
            if fw is None or fb is None:
                raise ValueError('absorb_plan: {} has no BatchNorm proxies (merge_batchnorm first)'.format(kb))
            w2 = second.weight
            khkw = w2[0, 0].numel() if w2.dim() > 2 else 1
            o1 = int(first.weight.size(0))
            rels.append(_ffi.DfqBatchAbsorbRelation(
                in_slot(ks, 'weight', w2), in_slot(kf, 'bias', first.bias), in_slot(ks, 'bias', second.bias),
                in_slot(kb, 'fake_weight', fw), in_slot(kb, 'fake_bias', fb), int(w2.shape[0]), int(w2.shape[1]), khkw, o1, stride))
            self._shift_views.append((idx, stride, o1))
            stride += -(-o1 // _ALIGN) * _ALIGN
        clips = []
        if range_clip is not None:
            for key, layer in g0.items():                       # dfq.py:168-170
                if type(layer) in tt:
                    clips.append(_ffi.DfqBatchAbsorbClip(in_slot(key, 'weight', layer.weight), layer.weight.numel()))
        self.n_nets, self.n_relations, self.n_clipped = n_nets, len(rels), len(clips)
        self.shift_block = torch.zeros((n_nets, stride), dtype=torch.float32, device=batch.stage.device)
        rel_arr = (_ffi.DfqBatchAbsorbRelation * len(rels))(*rels) if rels else None
        clip_arr = (_ffi.DfqBatchAbsorbClip * len(clips))(*clips) if clips else None
        self._create((rel_arr, len(rels), clip_arr, len(clips)), ctypes.c_float(n_sigma), ctypes.c_float(lo), ctypes.c_float(hi),
                     self.shift_block.data_ptr() if rels else None, stride)
        a, c = ctypes.c_int64(), ctypes.c_int64()
        _ffi.check(_ffi.lib().dfq_batch_absorb_plan_elements(self._plan, ctypes.byref(a), ctypes.byref(c)))
        self.absorbed_elements, self.clip_only_elements = a.value, c.value          # per network

    def shifts(self, n):
        """{index into the relations list: the shift vector c of network n} for the absorbed relations -- views of the block"""
        row = self.shift_block[n]
        return {idx: row[off:off + o1] for (idx, off, o1) in self._shift_views}


class BatchActRangePlan(_BatchPlan):
    """The analytic activation ranges of every network of a NetworkBatch (dfq_batch_act_plan, include/dfq_hip.h): the program
    compiled from network 0's graph plus the batch's base addresses.  ``run()`` enqueues on the current stream; it reads the
    BatchNorm proxies (and, for a conv / linear without BatchNorm in front of a quantiser, that layer's weight and bias) and
    writes only ``self.block``, float32 [n_nets, n_results, 2]: the packed (min, max) pairs in the layout ``QuantMeasure``
    keeps its range in.  The block is a torch tensor and outlives ``close()``."""
    _c = 'dfq_batch_act_plan'

    def __init__(self, batch, is_detection, N, tensor_ops):
        n_sigma = _finite(N, 'act_range_plan')
        g0, b0, _ = batch.nets[0]
        ops = OrderedDict()
        for key, count in (tensor_ops or {}).items():
            if key not in g0 or not isinstance(g0[key], str) or b0[key] is None:
                raise ValueError('act_range_plan: tensor_ops names {!r}, which is not a tensor op of the graph'.format(key))
            if isinstance(count, bool) or not isinstance(count, (int, np.integer)) or count <= 0:
                raise ValueError('act_range_plan: tensor_ops[{!r}] = {!r} is not a positive count'.format(key, count))
            ops[key] = int(count)
        super().__init__(batch)
        self.is_detection, self.n_sigma, self.eps = bool(is_detection), n_sigma, 1e-6          # eps: layer_transform.py:349
        try:
            nodes = _act_program(g0, b0, batch.bn_type, batch.targ_type, ops, self.is_detection)
        except _WalkError as e:                 # what set_quant_minmax asserts, or cannot evaluate
            raise ValueError('act_range_plan: {}: {}'.format(e.key, e)) from None
        if not nodes:
            raise ValueError('act_range_plan: the graph has no quantised node')
        key_of = {id(m): k for k, m in g0.items() if isinstance(m, torch.nn.Module)}
        in_slot = batch._in_slot

        def proxies(bn):
            key = key_of.get(id(bn), '?')
            fw, fb = _dfq._attr(bn, 'fake_weight'), _dfq._attr(bn, 'fake_bias')
            if fw is None or fb is None:
                raise ValueError('act_range_plan: {} has no BatchNorm proxies (merge_batchnorm first)'.format(key))
            if fw.numel() != fb.numel():
                raise ValueError('act_range_plan: the proxies of {} have {} and {} channels'.format(key, fw.numel(), fb.numel()))
            return key, fw, fb
        results, steps, sources = [], [], []
        self._views = []                       # (graph key, first result, number of results, is a tensor op)
        for key, _, node_results in nodes:
            self._views.append((key, len(results), len(node_results), isinstance(g0[key], str)))
            for _, prog in sorted(node_results, key=lambda r: r[0]):     # the quantisers' order; the walk gives evaluation order
                results.append(_ffi.DfqBatchActResult(len(steps), len(prog)))
                channels = None                # of the moment vectors of this result
                for (op, bn, relu, operand, through) in prog:
                    if op == _ffi.ACT_CONST:
                        steps.append(_ffi.DfqBatchActStep(None, None, op, 0, 0, 0, -1, -1, operand[0], operand[1]))
                        continue
                    if bn is None:
                        steps.append(_ffi.DfqBatchActStep(None, None, op, 0, relu, operand, -1, -1, 0.0, 0.0))
                        continue
                    bkey, fw, fb = proxies(bn)
                    if through is not None:    # case (d): both proxies through the layer, fake_bias first like set_quant_minmax
                        kind, layer = through
                        lkey = key_of.get(id(layer), '?')
                        w = layer.weight
                        khkw = w[0, 0].numel() if w.dim() == 4 else 1
                        groups = int(getattr(layer, 'groups', 1)) if kind == 'conv' else 1
                        if groups * int(w.shape[1]) != fw.numel() or int(w.shape[0]) % groups:
                            raise ValueError('act_range_plan: {} takes {} x {} channels, the BatchNorm {} in front of it has {}'.format(
                                lkey, groups, int(w.shape[1]), bkey, fw.numel()))
                        pw = in_slot(lkey, 'weight', w)
                        pb = in_slot(lkey, 'bias', layer.bias) if layer.bias is not None else None
                        for vec, name in ((fb, 'fake_bias'), (fw, 'fake_weight')):
                            sources.append(_ffi.DfqBatchActSource(pw, pb, in_slot(bkey, name, vec), int(w.shape[0]), int(w.shape[1]),
                                                                  khkw, groups))
                        steps.append(_ffi.DfqBatchActStep(None, None, op, int(w.shape[0]), relu, 0, len(sources) - 1, len(sources) - 2,
                                                          0.0, 0.0))
                        continue
                    if op in (_ffi.ACT_MOM, _ffi.ACT_MOM_ADD):
                        if channels is None:
                            channels = fw.numel()
                        elif fw.numel() != channels:
                            raise ValueError('act_range_plan: {}: {} feeds an add of {} channels with {}'.format(key, bkey, channels, fw.numel()))
                    steps.append(_ffi.DfqBatchActStep(in_slot(bkey, 'fake_weight', fw), in_slot(bkey, 'fake_bias', fb), op, fw.numel(),
                                                      relu, 0, -1, -1, 0.0, 0.0))
        self.keys = [key for (key, _, _, _) in self._views]
        self.n_nets, self.n_results, self.n_steps, self.n_sources = len(batch.nets), len(results), len(steps), len(sources)
        self.block = torch.zeros((self.n_nets, self.n_results, 2), dtype=torch.float32, device=batch.stage.device)
        res_arr = (_ffi.DfqBatchActResult * len(results))(*results)
        step_arr = (_ffi.DfqBatchActStep * len(steps))(*steps)
        src_arr = (_ffi.DfqBatchActSource * len(sources))(*sources) if sources else None
        self._create((res_arr, len(results), step_arr, len(steps), src_arr, len(sources)), ctypes.c_float(n_sigma),
                     ctypes.c_float(self.eps), self.block.data_ptr(), 2 * self.n_results)

    def ranges(self, n):
        """OrderedDict graph key -> float32 [2] view (min, max) of network n's part of the block, in set_quant_minmax's
        order; a list of such views for a tensor op (one per quantised input)"""
        rows = self.block[n]
        out = OrderedDict()
        for key, first, count, is_op in self._views:
            out[key] = [rows[first + i] for i in range(count)] if is_op else rows[first]
        return out

    def bind_quantisers(self, tensor_op_quant=None):
        """Point ``running_min`` / ``running_max`` of every quantiser module of every network at its pair in the block: no
        launch, no copy.  The two buffers become the halves of one float32[2], which is the packed pair
        ``QuantMeasure._packed_range`` looks for, so a later forward pass adopts it as it is.  ``tensor_op_quant``: one
        ``{graph key: [QuantMeasure, ...]}`` per network for the tensor ops the plan was created with.  Run (and let finish)
        the plan before anything reads the buffers; ``NetworkBatch.release()`` gives them storages of their own."""
        batch = self._batch
        if batch.storage is None:
            raise RuntimeError('NetworkBatch: the batch has been released')
        if tensor_op_quant is not None and len(tensor_op_quant) != self.n_nets:
            raise ValueError('bind_quantisers: tensor_op_quant wants one dict per network')
        for n, (graph, _, _) in enumerate(batch.nets):
            rows = self.block[n]
            for key, first, count, is_op in self._views:
                node = graph[key]
                if is_op:
                    mods = (tensor_op_quant[n].get(key) if tensor_op_quant is not None else None) or []
                else:
                    mods = [node.quant] if hasattr(node, 'quant') else []
                for i, q in enumerate(mods[:count]):
                    _rebind(q, 'running_min', rows[first + i, 0:1])
                    _rebind(q, 'running_max', rows[first + i, 1:2])
                    batch._act_bound[id(q)] = (q, self.block)
