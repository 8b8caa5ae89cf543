"""Scale folding and distilled-range calibration with the call surface of the reference's
``improve_dfq.py``:

  transform_quant_layer   <- improve_dfq.py:144-172  (+ utils/quantize.py:145-174, :269-289)
  update_quant_range      <- improve_dfq.py:280-297
  set_update_stat         <- improve_dfq.py:299-309
  bias_correction_distill <- improve_dfq.py:311-371  (ChannelSumMeter: its hook, reduced on the device)

The abandoned experiments of that file (GradHook, update_scale, kl_categorical, ...; call sites
commented out in main_cls.py:157-174,192-194) are out of scope.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _ffi
from .utils.quantize import (QConv2d, QLinear, QuantConv2d, QuantLinear, QuantMeasure, QuantNConv2d,
                             QuantNLinear)


def merge_scale_into_layer(layer):
    """QConv2d/QLinear.merge_scale_to_weight (quantize.py:145-156, :269-280) on the engine.

    scale_prev: W[o, i, :] /= scale_prev[g(o)*I/g + i]  for convs (quantize.py:158-167),
                W[o, i]    *= scale_prev[i]             for linears (quantize.py:282-283);
    scale:      W[o, ...]  *= scale[o], b[o] *= scale[o] (quantize.py:169-174).
    """
    lib = _ffi.lib()
    with torch.no_grad():
        stage = _ffi.Stage()
        w = stage.bind(layer.weight)
        is_conv = w.dim() == 4
        khkw = w[0, 0].numel() if is_conv else 1
        sp = getattr(layer, 'scale_prev', None)
        if sp is not None:
            spd = stage.bind(sp.detach().reshape(-1).contiguous())
            groups = layer.groups if is_conv else 1
            _ffi.check(lib.dfq_scale_cols(_ffi.ptr(w), w.shape[0], w.shape[1], khkw, groups, _ffi.ptr(spd),
                                          1 if is_conv else 0, _ffi.stream_arg()))
            layer.scale_prev = None
        sc = getattr(layer, 'scale', None)
        if sc is not None:
            scd = stage.bind(sc.detach().reshape(-1).contiguous())
            _ffi.check(lib.dfq_scale_rows(_ffi.ptr(w), w.shape[0], w[0].numel(), _ffi.ptr(scd), 0, _ffi.stream_arg()))
            if layer.bias is not None:
                b = stage.bind(layer.bias)
                _ffi.check(lib.dfq_vec_op(_ffi.ptr(b), _ffi.ptr(scd), b.numel(), 0, _ffi.stream_arg()))
            layer.scale = None
        stage.writeback()


def _swap_modules(model, mapping):
    """Replace every module whose exact type is a key of `mapping`, carrying parameters and the
    activation quantiser over (what the reference gets from TorchTransformer.trans_layers)."""
    swapped = {}
    for name, child in list(model.named_children()):
        new_cls = mapping.get(type(child))
        if new_cls is None:
            swapped.update(_swap_modules(child, mapping))
            continue
        if isinstance(child, nn.Conv2d):
            new = new_cls(child.in_channels, child.out_channels, child.kernel_size, child.stride, child.padding,
                          child.dilation, child.groups, child.bias is not None)
        else:
            new = new_cls(child.in_features, child.out_features, child.bias is not None)
        new.weight = child.weight
        new.bias = child.bias
        if hasattr(child, 'quant'):
            new.quant = child.quant
        for attr in ('num_bits', 'num_bits_bias'):
            if hasattr(child, attr) and hasattr(new, attr):
                setattr(new, attr, getattr(child, attr))
        new.train(child.training)
        setattr(model, name, new)
        swapped[child] = new
    return swapped


def transform_quant_layer(model, graph, res, trainable=False):
    """Fold the learned/equalisation scales into the weights of every relation's layers, drop the
    scale attributes and swap QConv2d/QLinear for their plain quantised counterparts."""
    for rr in res:
        layer_first, layer_second, _ = rr.get_idxs()
        for key in (layer_first, layer_second):
            layer = graph[key]
            merge_scale_into_layer(layer)
            for attr in ('scale', 'scale_prev'):
                if hasattr(layer, attr):
                    if attr in layer._parameters:
                        del layer._parameters[attr]
                    elif attr in layer.__dict__:
                        delattr(layer, attr)
    if trainable:
        mapping = {QConv2d: QuantConv2d, QLinear: QuantLinear}
    else:
        mapping = {QConv2d: QuantNConv2d, QLinear: QuantNLinear}
    swapped = _swap_modules(model, mapping)
    for key in graph:
        if not isinstance(graph[key], str) and graph[key] in swapped:
            graph[key] = swapped[graph[key]]
    return model


def set_update_stat(model, targ_type, update_stat):
    """Toggle ``update_stat`` on every module whose type is in ``targ_type`` (improve_dfq.py:299-309)."""
    for module in model.modules():
        if type(module) in targ_type:
            module.set_update_stat(update_stat)
    return model


def update_quant_range(model, data, graph, bottoms, is_detection=False, group=None):
    """Run the distilled batches through the model so every QuantMeasure records its range
    (improve_dfq.py:280-297); the first layer's range is pinned to the ImageNet-normalised image
    range (2.64 / -2.11790393), or +-1 for detection.

    ``group`` (extension; SURVEY 8e "C5: data-parallel over distilled batches"): a torch.distributed process group whose ranks
    each hold the same model.  Rank r then runs batches r, r + world, ... only, and ONE all_reduce merges the [modules, 2] table
    of running ranges (max of the maxima, min of the minima) at the end, so every rank ends with the same ranges.  Not
    bit-identical to the sequential pass, and it cannot be: the reference quantises every batch with the range recorded SO FAR
    (quantize.py:103-119), so what a later layer sees of batch k depends on the batches in front of it; a rank that has seen
    fewer batches quantises with a slightly narrower range.  The effect is second order -- half a quantisation step of the
    producing layer, 1/510 of its range -- tests/test_range_parity.py holds the merged ranges within 2 % of the sequential ones."""
    import torch.distributed as dist
    world = dist.get_world_size(group) if group is not None else 1
    rank = dist.get_rank(group) if group is not None else 0
    with torch.no_grad():
        for i, batch in enumerate(data):
            if i % world != rank:
                continue
            dev = next(model.parameters()).device
            model(batch.to(dev))
        if world > 1:
            measures = [m for m in model.modules() if isinstance(m, QuantMeasure)]
            if measures:
                dev = measures[0].running_max.device
                table = torch.stack([torch.cat([m.running_max.reshape(1).to(dev), -m.running_min.reshape(1).to(dev)])
                                     for m in measures])                               # max and -min: ONE reduction (MAX)
                comm = table if dist.get_backend(group) == 'nccl' else table.cpu()
                dist.all_reduce(comm, op=dist.ReduceOp.MAX, group=group)
                table = comm.to(dev)
                for m, row in zip(measures, table):
                    m.running_max.copy_(row[0:1].to(m.running_max.device))
                    m.running_min.copy_((-row[1:2]).to(m.running_min.device))
    for key in graph:
        bot = bottoms[key]
        # (the graph fxgraph.quantize_tensor_ops returns lists a layer's input quantiser as a node of its own: there the node fed
        # by 'Data' IS the QuantMeasure of the first layer)
        first = graph[key].quant if hasattr(graph[key], 'quant') else (graph[key] if isinstance(graph[key], QuantMeasure) else None)
        if bot is not None and bot[0] == 'Data' and first is not None:
            q = first
            if is_detection:
                q.running_max.fill_(1.0)
                q.running_min.fill_(-1.0)
            else:
                q.running_max.fill_(2.64)
                q.running_min.fill_(-2.11790393)
    return model


class _Scratch:
    """One device buffer for every dfq_channel_sum_accumulate call of a pass: as large as the largest output seen, regrown
    only when a larger one arrives.  All calls are enqueued on one stream, so they take turns with it."""

    def __init__(self):
        self.buf = None

    def get(self, nbytes, device):
        if self.buf is None or self.buf.numel() * 8 < nbytes or self.buf.device != device:
            self.buf = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=device)
        return self.buf


class ChannelSumMeter:
    """A forward hook that reduces what it sees instead of keeping it (the reference's ModuleHook keeps the whole output,
    improve_dfq.py:323-331, :349-355): every output [N, C, ...] is read once, by dfq_channel_sum_accumulate on the current
    stream, and ``acc[c] += weight * sum over N and the trailing dimensions of output[:, c]`` in float64 -- weight = 1 / N
    unless given, the reference's ``mean(0)``.  Nothing is kept of the output, nothing is copied to the host and nothing waits.

        meter = ChannelSumMeter()                       # or ChannelSumMeter(acc): a float64 [C] slice of a table of yours
        handle = conv.register_forward_hook(meter.hook)
        model(batch); ...; handle.remove()
        meter.acc                                       # float64 [C] on the device; meter.hw: H * W of the last output

    The sums are deterministic: the order of the additions depends on the output's shape alone.  NaN and inf in one channel
    stay in that channel.  An output that is not float32, not contiguous, on another device or not 16-byte aligned is
    copied first."""

    def __init__(self, acc=None, scratch=None):
        if acc is not None and (acc.dtype is not torch.float64 or acc.dim() != 1 or not acc.is_contiguous()):
            raise ValueError('ChannelSumMeter: acc is a contiguous float64 vector [channels]')
        self.acc = acc
        self.hw = None
        self.calls = 0
        self._scratch = scratch if scratch is not None else _Scratch()

    def hook(self, module, inputs, output):
        self.add(output)

    def add(self, x, weight=None):
        if not torch.is_tensor(x) or x.dim() < 2:
            raise TypeError('ChannelSumMeter: the hooked output is a tensor [N, C, ...], not {}'.format(
                tuple(x.shape) if torch.is_tensor(x) else type(x).__name__))
        dev = _ffi.target_device()
        n, c = int(x.shape[0]), int(x.shape[1])
        hw = 1
        for d in x.shape[2:]:
            hw *= int(d)
        if n < 1 or c < 1 or hw < 1:
            raise ValueError('ChannelSumMeter: an empty output {}'.format(tuple(x.shape)))
        if self.acc is None:
            self.acc = torch.zeros(c, dtype=torch.float64, device=dev)
        if self.acc.numel() != c or self.acc.device != dev:
            raise ValueError('ChannelSumMeter: an output of {} channels for sums of {} on {}'.format(c, self.acc.numel(), self.acc.device))
        x = x.detach()
        if x.device != dev or x.dtype is not torch.float32:
            x = x.to(device=dev, dtype=torch.float32)
        x = x.contiguous()
        if x.data_ptr() % 16:
            x = x.clone()                                   # (a view into the middle of a buffer: the kernel's loads are 16-byte)
        lib = _ffi.lib()
        scratch = self._scratch.get(int(lib.dfq_channel_sum_scratch_bytes(n, c, hw)), dev)
        _ffi.check(lib.dfq_channel_sum_accumulate(_ffi.ptr(x), n, c, hw, 1.0 / n if weight is None else float(weight), _ffi.ptr(self.acc),
                                                  _ffi.ptr(scratch), _ffi.stream_arg()))
        self.hw = hw
        self.calls += 1


def _out_channels(module):
    w = getattr(module, 'weight', None)
    if not torch.is_tensor(w) or w.dim() < 2:
        raise TypeError('bias_correction_distill: {} has no weight [out_channels, ...] to take the channel count from'.format(
            type(module).__name__))
    return int(w.shape[0])


def bias_correction_distill(qmodel, model_original, data, targ_type, targ_type_original, spatial='sum', group=None):
    """Empirical bias correction on distilled data (improve_dfq.py:311-371): every module of ``qmodel`` whose exact type is in
    ``targ_type`` gets  bias[c] -= E_q[c] - E_ref[c],  the difference between its own mean output and the mean output of its
    counterpart in ``model_original`` (exact type in ``targ_type_original``, matched by order) over the batches of ``data``.
    The only bias correction for layers the analytic one (dfq.bias_correction) cannot model: no BatchNorm in front, BatchNorms
    folded away, per-channel or low-bit weights.

    Per batch ``qmodel(batch)`` runs first, then ``model_original(batch)``; the reference's replace_op() / restore_op() around
    the first call are fxgraph.quantize_tensor_ops here, applied by the caller when the model is built -- this function does
    not patch torch.  Both models go to the engine's device and into eval(); a missing bias becomes a zero
    ``nn.Parameter(requires_grad=False)`` (:366-367), an existing one keeps its identity.

    Where the reference keeps every hooked output of both models for a whole batch and copies one [C, H, W] mean per layer,
    model and batch to the host (:349-355), the hooks here are ChannelSumMeter: an output is read once, when its hook sees it,
    and reduced into ONE float64 table [2, sum of channels] on the device.  No output is kept, and nothing is copied to the
    host or waited for until the loop is over.

    Numerics: per-channel sums over N, H and W in float64 from the first addition on (deterministic: two calls from the same
    start are bit-equal), each batch weighted 1 / N_b -- the reference's ``mean(0)``, so unequal batches weigh as they do
    there; then per channel ``(sum_q - sum_ref) * scale`` in float64, ONE rounding of that shift to float32 and ONE float32
    subtraction from the bias (:361-368).

    ``spatial``: 'sum' (the default) is the reference's ``error.view(C, -1).sum(-1)`` (:365): scale = 1 / len(data), so a conv
    layer's shift is the mean error summed over its H * W output positions -- H * W TIMES the per-position mean error.  It is
    the default only so that the function is a drop-in for the reference's.  'mean' divides by H * W as well
    (scale = 1 / (len(data) * H * W)): the estimator of the DFQ paper, E[y_q] - E[y], the shift after which the layer's mean
    output error is zero.  For a Linear layer (H * W = 1) the two coincide.

    ``group`` (extension, as update_quant_range's): a torch.distributed process group whose ranks hold the same two models.
    Rank r runs batches r, r + world, ...; ONE all_reduce(SUM) of the float64 table precedes the bias update, and the scale
    uses the global len(data), so every rank ends with the same biases.  They are not bit-identical to the sequential pass
    (another order of the float64 sums) but lie within its rounding bound."""
    import torch.distributed as dist
    if spatial not in ('sum', 'mean'):
        raise ValueError("bias_correction_distill: spatial is 'sum' or 'mean', not {!r}".format(spatial))
    n_batches = len(data)
    if n_batches < 1:
        raise ValueError('bias_correction_distill: no batches')
    dev = _ffi.target_device()
    qmodel = qmodel.to(dev).eval()
    model_original = model_original.to(dev).eval()
    mods = [m for _, m in qmodel.named_modules() if type(m) in targ_type]
    mods_original = [m for _, m in model_original.named_modules() if type(m) in targ_type_original]
    assert len(mods) == len(mods_original), "len of hooks in 2 models must be the same"
    channels = [_out_channels(m) for m in mods]
    for idx, (c, m) in enumerate(zip(channels, mods_original)):
        if _out_channels(m) != c:
            raise ValueError('bias_correction_distill: hooked module {} has {} channels in qmodel and {} in model_original'.format(
                idx, c, _out_channels(m)))
    world = dist.get_world_size(group) if group is not None else 1
    rank = dist.get_rank(group) if group is not None else 0
    offsets = [0]
    for c in channels:
        offsets.append(offsets[-1] + c)
    table = torch.zeros((2, max(offsets[-1], 1)), dtype=torch.float64, device=dev)     # half 0: qmodel, half 1: model_original
    scratch = _Scratch()
    meters = [[ChannelSumMeter(table[half, o:o + c], scratch) for o, c in zip(offsets, channels)] for half in (0, 1)]
    handles = []
    lib = _ffi.lib()
    try:
        for half, modules in enumerate((mods, mods_original)):
            for m, meter in zip(modules, meters[half]):
                handles.append(m.register_forward_hook(meter.hook))
        with torch.no_grad():
            for i, batch in enumerate(data):
                if i % world != rank:
                    continue
                batch = batch.to(dev)
                qmodel(batch)
                model_original(batch)
            if world > 1:
                comm = table if dist.get_backend(group) == 'nccl' else table.cpu()
                dist.all_reduce(comm, op=dist.ReduceOp.SUM, group=group)
                table.copy_(comm)
            stage = _ffi.Stage()
            for idx, m in enumerate(mods):
                scale = 1.0 / n_batches
                if spatial == 'mean':
                    hw = meters[0][idx].hw or meters[1][idx].hw
                    if hw is None:
                        raise RuntimeError("bias_correction_distill: spatial='mean' needs the output size of hooked module {}, "
                                           'which saw no batch on this rank'.format(idx))
                    scale = 1.0 / (n_batches * hw)
                if getattr(m, 'bias', None) is None:
                    m.bias = nn.Parameter(torch.zeros(channels[idx], device=m.weight.device), requires_grad=False)
                o, c = offsets[idx], channels[idx]
                _ffi.check(lib.dfq_bias_sub_channel_delta(_ffi.ptr(stage.bind(m.bias)), _ffi.ptr(table[0, o:o + c]), _ffi.ptr(table[1, o:o + c]),
                                                          c, scale, _ffi.stream_arg()))
            stage.writeback()
    finally:
        for h in handles:
            h.remove()
    return qmodel


class HistogramMeter:
    """A forward PRE-hook for a QuantMeasure -- it sees the quantiser's input -- that reduces what it sees instead of keeping
    it, the sibling of ChannelSumMeter.  Two phases, switched by assigning ``meter.phase``:

      'range'  folds the tensor's true (min, max) into ``range2`` (dfq_tensor_minmax, then fmin / fmax on the device: a NaN
               is skipped, the house rule of include/dfq_hip.h);
      'count'  adds the tensor's histogram over ``range2`` to ``counts`` (dfq_act_hist_accumulate; the slot rule is in
               include/dfq_hip.h).

        meter = HistogramMeter(bins=2048)               # or HistogramMeter(range2, counts): slices of tables of yours
        handle = layer.quant.register_forward_pre_hook(meter.hook)
        for b in data: model(b)
        meter.phase = 'count'
        for b in data: model(b)
        handle.remove()
        prims.hist_clip_range(meter.counts, meter.range2, num_bits=8)

    ``range2`` is a float32 [2] on the device, (+inf, -inf) before the first tensor; ``counts`` an int64 [bins + 3] (the bins,
    then below, above, nan; the library's uint64).  Nothing is kept of the activation, nothing is copied to the host and nothing
    waits.  An input that is not float32, not contiguous, on another device or not 16-byte aligned is copied first."""

    def __init__(self, range2=None, counts=None, bins=2048, phase='range', scratch=None):
        bins = int(bins)
        if not 2 <= bins <= 4096:
            raise ValueError('HistogramMeter: bins is 2 ... 4096, not {}'.format(bins))
        if range2 is not None and (range2.dtype is not torch.float32 or range2.dim() != 1 or range2.numel() != 2 or not range2.is_contiguous()):
            raise ValueError('HistogramMeter: range2 is a contiguous float32 vector [2]')
        if counts is not None and (counts.dtype is not torch.int64 or counts.dim() != 1 or counts.numel() != bins + 3
                                   or not counts.is_contiguous()):
            raise ValueError('HistogramMeter: counts is a contiguous int64 vector [bins + 3]')
        self.bins = bins
        self.range2 = range2
        self.counts = counts
        self.phase = phase
        self.calls = 0
        self._scratch = scratch          # (float32 [2], int32 [2]) of dfq_tensor_minmax, shared by the meters of one pass
        self._rows = None                # clip_quant_range: a float32 [calls, 2] table, one (min, max) per call of pass A
        self._row = 0
        self._dev = _ffi.target_device()
        self._lib = _ffi.lib()

    def hook(self, module, inputs):
        self.add(inputs[0])

    def range_rows(self, rows):
        """Pass A without a torch operation per call: the (min, max) of call i goes to rows[i] (float32 [calls, 2] on the device,
        (+inf, -inf) where nothing was written) and the caller folds the rows itself; calls beyond the table fold into
        ``range2`` as usual."""
        self._rows, self._row = rows, 0

    def add(self, x):
        if self.phase not in ('range', 'count'):
            raise ValueError("HistogramMeter: phase is 'range' or 'count', not {!r}".format(self.phase))
        if not torch.is_tensor(x):
            raise TypeError('HistogramMeter: the hooked input is a tensor, not {}'.format(type(x).__name__))
        dev = self._dev
        with torch.no_grad():
            if self.range2 is None:
                self.range2 = torch.tensor([float('inf'), float('-inf')], dtype=torch.float32).to(dev)
            if self.counts is None:
                self.counts = torch.zeros(self.bins + 3, dtype=torch.int64, device=dev)
            if self.range2.device != dev or self.counts.device != dev:
                raise ValueError('HistogramMeter: range2 and counts live on {}'.format(dev))
            if x.numel() == 0:
                return
            x = x.detach()
            if x.device != dev or x.dtype is not torch.float32:
                x = x.to(device=dev, dtype=torch.float32)
            x = x.contiguous()
            if x.data_ptr() % 16:
                x = x.clone()                               # (a view into the middle of a buffer: the kernel's loads are 16-byte)
            lib = self._lib
            if self.phase == 'range':
                if self._scratch is None or self._scratch[0].device != dev:
                    self._scratch = (torch.empty(2, dtype=torch.float32, device=dev), torch.zeros(2, dtype=torch.int32, device=dev))
                out, words = self._scratch
                if self._rows is not None and self._row < self._rows.shape[0]:
                    _ffi.check(lib.dfq_tensor_minmax(_ffi.ptr(x), x.numel(), self._rows.data_ptr() + 8 * self._row, _ffi.ptr(words),
                                                     _ffi.stream_arg()))
                    self._row += 1
                else:
                    _ffi.check(lib.dfq_tensor_minmax(_ffi.ptr(x), x.numel(), _ffi.ptr(out), _ffi.ptr(words), _ffi.stream_arg()))
                    torch.fmin(self.range2[0:1], out[0:1], out=self.range2[0:1])
                    torch.fmax(self.range2[1:2], out[1:2], out=self.range2[1:2])
            else:
                _ffi.check(lib.dfq_act_hist_accumulate(_ffi.ptr(x), x.numel(), _ffi.ptr(self.range2), self.bins, _ffi.ptr(self.counts),
                                                       _ffi.stream_arg()))
        self.calls += 1


def _data_fed_quantisers(graph, bottoms):
    """the QuantMeasure of every node fed by 'Data' (update_quant_range pins the same ones)"""
    pinned = []
    for key in graph:
        bot = bottoms[key]
        first = graph[key].quant if hasattr(graph[key], 'quant') else (graph[key] if isinstance(graph[key], QuantMeasure) else None)
        if bot is not None and bot[0] == 'Data' and first is not None:
            pinned.append(first)
    return pinned


def clip_quant_range(model, data, graph, bottoms, method='mse', percentile=0.9999, bins=2048, candidates=None, is_detection=False,
                     group=None, report=None):
    """Replace the range of every activation quantiser (QuantMeasure) of ``model`` by a CLIPPED range taken from the histogram
    of its input over the batches of ``data``: method='mse', the range of least modelled quantisation error at the quantiser's
    own ``num_bits``, or method='percentile', the central ``percentile`` of the mass on either side (the definitions:
    dfq_hist_clip_range, include/dfq_hip.h).  An extension: the reference's ranges are min / max rules (the analytic
    beta +- 6 gamma of set_quant_minmax, the running extrema of update_quant_range), which cannot trade clipping error against
    rounding error -- what counts below 8 bits and on the heavy-tailed inputs of add / cat nodes.

    Call it after update_quant_range or set_quant_minmax, with ``update_stat`` off (refused otherwise).  The model is taken as
    it stands: during both passes the activations are quantised with the ranges the model HAS, and all ranges are replaced
    together at the end.  The procedure is ONE-SHOT: the histograms are those of the inputs under the old ranges, and a second
    call would see other inputs; it is not iterated to a fixed point here.

      pass A  every batch, the hooks (HistogramMeter) in 'range': each quantiser's true (min, max), NaN skipped;
      pass B  every batch again, the hooks in 'count': the histogram of each quantiser over its own (min, max), ``bins`` bins,
              into ONE int64 table on the device;
      then ONE dfq_hist_clip_range launch for all quantisers, each with its own num_bits, and the results are copied into
      running_min / running_max on the device (the buffers keep their identity and their shape [1]).

    Nothing is kept of an activation, and nothing is copied to the host or waited for inside the loops.  The quantiser fed by
    'Data' is pinned as update_quant_range pins it (2.64 / -2.11790393, or +-1 with ``is_detection``), not searched.

    ``report``: a dict that receives, per quantiser (keyed by its module name), 'hist_range' (float32 [2]), 'counts' (int64
    [bins + 3]: the bins, below, above, nan), 'old_range' and 'new_range' -- device tensors, nothing is waited for -- and
    'pinned'; a pinned quantiser has the two ranges only.

    ``group`` (as update_quant_range's and bias_correction_distill's): a torch.distributed process group whose ranks hold the
    same model.  Rank r runs batches r, r + world, ...; ONE all_reduce (MAX of (max, -min)) of the range table follows pass A
    and ONE all_reduce(SUM) of the int64 count table pass B.  Extrema are selections and counts are integers, so -- unlike the
    two siblings -- the sharded result is BIT-IDENTICAL to the sequential one, histograms and ranges."""
    import torch.distributed as dist
    from . import prims
    if method not in prims.HIST_METHODS:
        raise ValueError("clip_quant_range: method is 'mse' or 'percentile', not {!r}".format(method))
    bins = int(bins)
    if not 2 <= bins <= prims.HIST_MAX_BINS:
        raise ValueError('clip_quant_range: bins is 2 ... {}, not {}'.format(prims.HIST_MAX_BINS, bins))
    if method == 'percentile' and not 0.5 < float(percentile) <= 1.0:
        raise ValueError('clip_quant_range: percentile is in (0.5, 1], not {}'.format(percentile))
    if method == 'mse' and candidates is not None and not 1 <= int(candidates) <= bins // 2:
        raise ValueError('clip_quant_range: candidates is 1 ... bins // 2 = {}, not {}'.format(bins // 2, candidates))
    world = dist.get_world_size(group) if group is not None else 1
    rank = dist.get_rank(group) if group is not None else 0
    dev = _ffi.target_device()
    named, seen = [], set()
    for name, m in model.named_modules():
        if isinstance(m, QuantMeasure) and id(m) not in seen:
            seen.add(id(m))
            named.append((name, m))
    pinned = _data_fed_quantisers(graph, bottoms)
    pinned_ids = {id(q) for q in pinned}
    for name, m in named:
        if m.update_stat:
            raise ValueError('clip_quant_range: {} still has update_stat on (set_update_stat(model, [QuantMeasure], False) first)'.format(name))
    searched = [(name, m) for name, m in named if id(m) not in pinned_ids]
    for name, m in searched:
        if not 2 <= int(m.num_bits) <= 16:
            raise ValueError('clip_quant_range: {} has num_bits = {} (2 ... 16)'.format(name, m.num_bits))
    n_q = len(searched)
    with torch.no_grad():
        def current(m):
            return torch.cat([m.running_min.detach().reshape(1).to(dev), m.running_max.detach().reshape(1).to(dev)])
        old = {id(m): current(m) for _, m in named}
        range_table = torch.tensor([float('inf'), float('-inf')], dtype=torch.float32).repeat(max(n_q, 1), 1).to(dev)
        count_table = torch.zeros((max(n_q, 1), bins + 3), dtype=torch.int64, device=dev)
        scratch = (torch.empty(2, dtype=torch.float32, device=dev), torch.zeros(2, dtype=torch.int32, device=dev))
        meters = [HistogramMeter(range_table[i], count_table[i], bins, 'range', scratch) for i in range(n_q)]
        try:
            n_local = len(range(rank, len(data), world))
        except TypeError:                                   # (an iterable without a length: the meters fold call by call)
            n_local = 0
        rows = torch.tensor([float('inf'), float('-inf')], dtype=torch.float32).repeat(max(n_q, 1), max(n_local, 1), 1).to(dev)
        if n_local:
            for i, meter in enumerate(meters):
                meter.range_rows(rows[i])                   # pass A: one (min, max) per batch, folded below -- no torch op per hook
        handles = []
        try:
            for (_, m), meter in zip(searched, meters):
                handles.append(m.register_forward_pre_hook(meter.hook))
            params = list(model.parameters())
            mdev = params[0].device if params else dev
            for phase in ('range', 'count'):
                for meter in meters:
                    meter.phase = phase
                for i, batch in enumerate(data):
                    if i % world != rank:
                        continue
                    model(batch.to(mdev))
                if phase == 'range' and n_q:
                    # the batches' extrema into the range table, NaN skipped (a tensor of nothing but NaN has (NaN, NaN))
                    lo, hi = rows[:, :, 0], rows[:, :, 1]
                    lo = torch.where(torch.isnan(lo), torch.full_like(lo, float('inf')), lo).amin(dim=1)
                    hi = torch.where(torch.isnan(hi), torch.full_like(hi, float('-inf')), hi).amax(dim=1)
                    range_table[:, 0].copy_(torch.fmin(range_table[:, 0], lo))
                    range_table[:, 1].copy_(torch.fmax(range_table[:, 1], hi))
                if world > 1 and n_q:
                    if phase == 'range':
                        table = torch.stack([range_table[:, 1], -range_table[:, 0]], dim=1)       # max and -min: ONE reduction (MAX)
                        comm = table if dist.get_backend(group) == 'nccl' else table.cpu()
                        dist.all_reduce(comm, op=dist.ReduceOp.MAX, group=group)
                        comm = comm.to(dev)
                        range_table[:, 1].copy_(comm[:, 0])
                        range_table[:, 0].copy_(-comm[:, 1])
                    else:
                        comm = count_table if dist.get_backend(group) == 'nccl' else count_table.cpu()
                        dist.all_reduce(comm, op=dist.ReduceOp.SUM, group=group)
                        count_table.copy_(comm)
        finally:
            for h in handles:
                h.remove()
        if n_q:
            new = prims.hist_clip_range(count_table, range_table, [int(m.num_bits) for _, m in searched], method=method,
                                        percentile=percentile, candidates=candidates)
            for i, (_, m) in enumerate(searched):
                m.running_min.copy_(new[i, 0:1].to(m.running_min.device))
                m.running_max.copy_(new[i, 1:2].to(m.running_max.device))
        for q in pinned:
            if is_detection:
                q.running_max.fill_(1.0)
                q.running_min.fill_(-1.0)
            else:
                q.running_max.fill_(2.64)
                q.running_min.fill_(-2.11790393)
        if isinstance(report, dict):
            index = {id(m): i for i, (_, m) in enumerate(searched)}
            for name, m in named:
                entry = {'old_range': old[id(m)], 'new_range': current(m), 'pinned': id(m) in pinned_ids}
                if id(m) in index:
                    entry['hist_range'] = range_table[index[id(m)]]
                    entry['counts'] = count_table[index[id(m)]]
                report[name] = entry
    return model
