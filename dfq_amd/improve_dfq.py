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
