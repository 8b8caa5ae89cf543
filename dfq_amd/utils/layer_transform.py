"""Graph-level passes around the equalisation/correction core, with the call surface of the
reference's ``utils/layer_transform.py``:

  merge_batchnorm      <- utils/layer_transform.py:231-276   (engine: dfq_fold_batchnorm; its graph walk is
                                                              ``_fold_pairs``, which ``arena.NetworkBatch.from_unfolded`` shares)
  quantize_targ_layer  <- utils/layer_transform.py:279-296   (engine: dfq_quant_plan_*)
  find_prev_bn         <- utils/layer_transform.py:299-344   (host graph walk, O(#nodes))
  set_quant_minmax     <- utils/layer_transform.py:347-609   (engine: dfq_bn_ranges, dfq_relu_moments, ...)

The graph walk of set_quant_minmax is ``_act_program``: it compiles a graph into steps, which
set_quant_minmax executes one launch at a time and ``arena.BatchActRangePlan`` hands to one plan for
a whole batch.

The graph model is the reference's: ``graph`` maps key -> nn.Module | str (tensor ops are strings whose
key contains 'add' / 'cat' / ...), ``bottoms`` maps key -> list of input keys | None.
"""
from __future__ import annotations

import ctypes

import torch
import torch.nn as nn

from .. import _ffi
from .quantize import QConv2d, QuantConv2d, QuantNConv2d, QLinear, QuantLinear, QuantNLinear

_CONV_TYPES = (nn.Conv2d, QConv2d, QuantConv2d, QuantNConv2d)
_LINEAR_TYPES = (nn.Linear, QLinear, QuantLinear, QuantNLinear)


def _ensure_bias(layer):
    """The reference adds a zero bias Parameter when a layer has none (layer_transform.py:253-254)."""
    b = layer.__dict__['_parameters'].get('bias')        # (not layer.bias: Module.__getattr__ is the slow path, and table
    if b is not None:                                     # building asks thousands of layers)
        return b
    if layer.bias is None:
        layer.bias = nn.Parameter(torch.zeros(layer.weight.size(0), dtype=torch.float32,
                                              device=layer.weight.device), requires_grad=False)
    return layer.bias


def _fold_pairs(graph, bottoms, targ_type):
    """[(layer key, BatchNorm key)] of the pairs merge_batchnorm folds, in graph order (layer_transform.py:239-244, :274): a
    node of exact type nn.BatchNorm2d with a ``targ_type`` layer among its bottoms; the first such bottom wins.  Structural:
    no tensor is read and nothing is changed.  ``merge_batchnorm`` and ``arena.NetworkBatch.from_unfolded`` share it."""
    pairs = []
    for key in graph:
        bots = bottoms[key]
        if bots is None:
            continue
        if type(graph[key]) != nn.BatchNorm2d:
            continue
        for bk in bots:
            if type(graph[bk]) not in targ_type:
                continue
            pairs.append((bk, key))
            break
    return pairs


def merge_batchnorm(model, graph, bottoms, targ_type=[QConv2d]):
    """Fold every BatchNorm2d that directly follows a targ layer into that layer.

    W <- W * gamma/sqrt(var+eps) per output channel, b <- b*gamma/sqrt(var+eps) + beta -
    gamma*mean/sqrt(var+eps); the BN keeps ``fake_weight = |gamma|`` and ``fake_bias = beta`` for the
    later passes and becomes an identity (gamma = var = 1, beta = mean = 0, eps below float32 resolution).
    """
    lib = _ffi.lib()
    with torch.no_grad():
        stage = _ffi.entry_stage()
        pairs = []
        for lk, bk in _fold_pairs(graph, bottoms, targ_type):
            _ensure_bias(graph[lk])
            pairs.append((graph[lk], graph[bk]))
        # a model that lives on the host crosses PCIe once each way: every tensor of every pair in one packed copy, the new
        # per-channel vectors of all BatchNorms in one flat buffer that comes back in one copy
        stage.prefetch([t for layer, bn in pairs for t in (layer.weight, layer.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var)])
        fake = stage.new_flat(2 * sum(bn.weight.numel() for _, bn in pairs)) if pairs else None
        outs, at = [], 0
        for layer, bn in pairs:
            w = stage.bind(layer.weight)
            b = stage.bind(layer.bias)
            gamma, beta = stage.bind(bn.weight), stage.bind(bn.bias)
            mean, var = stage.bind(bn.running_mean), stage.bind(bn.running_var)
            n = gamma.numel()
            fw, fb = fake[at:at + n], fake[at + n:at + 2 * n]
            _ffi.check(lib.dfq_fold_batchnorm(_ffi.ptr(w), _ffi.ptr(b), w.shape[0], w[0].numel(), _ffi.ptr(gamma),
                                              _ffi.ptr(beta), _ffi.ptr(mean), _ffi.ptr(var),
                                              ctypes.c_float(bn.eps), _ffi.ptr(fw), _ffi.ptr(fb),
                                              _ffi.stream_arg()))
            outs.append((bn, at, n))
            at += 2 * n
            # The reference sets eps = 0 (layer_transform.py:272); current PyTorch rejects eps <= 0 in
            # F.batch_norm.  1e-12 is absorbed by float32 rounding (1 + 1e-12 == 1): the folded BN is still an
            # exact identity and the model still runs.
            bn.eps = 1e-12
        host = {}
        for bn, o, n in outs:
            dev = bn.weight.device
            if dev == fake.device:
                src = fake
            else:                                 # ONE copy of the flat buffer per foreign device (a CPU-resident model: one D2H)
                src = host.get(dev)
                if src is None:
                    src = host[dev] = _ffi._to_host(fake) if dev.type == 'cpu' else fake.to(dev)
            bn.register_buffer('fake_weight', src[o:o + n].clone())
            bn.register_buffer('fake_bias', src[o + n:o + 2 * n].clone())
        if fake is not None and any(bn.weight.device != fake.device for bn, _, _ in outs):
            # the proxies were computed on the device: a stage whose shadows outlive the call keeps `fake` as their device copy
            stage.adopt(fake, [(t, at, t.numel()) for bn, o, n in outs
                               for t, at in ((bn.fake_weight, o), (bn.fake_bias, o + n)) if t.device.type == 'cpu'])
        stage.writeback()
    return model


def quantize_targ_layer(graph, bit_weight=8, bits_bias=16, targ_type=None, return_codes=False, per_channel=False, signed=False,
                        rounding='nearest'):
    """Per-tensor asymmetric fake-quant of every targ layer's weight (and bias unless 32 bit).

    Two launches for the whole network: one multi-tensor min/max, one multi-tensor quantise.
    ``return_codes`` (extension) additionally returns {key: int32 code tensor of the weight}.
    ``signed`` (extension): the symmetric recipe for the weights.
    ``per_channel`` (extension): every weight row (output channel) is quantised with its own (min, max); biases stay per
    tensor.  ONE launch for the whole network (dfq_row_quant_plan).  With ``return_codes`` the result is
    ``(graph, codes, ranges)``: ranges[key] = float32 [O, 2], the (min, max) each row was quantised with.
    ``rounding`` (extension): 'nearest', or 'squant' -- the same ranges and grid, but the weights' roundings are flipped where
    that costs least until the rounding errors of every kH x kW kernel and of every output row sum to at most half a quantum
    (dfq_squant_rows, "Adaptive rounding" in include/dfq_hip.h; bit_weight an integer in [2, 16]).  The biases are rounded to
    nearest as before.  Anything else: ValueError.
    """
    if rounding not in ('nearest', 'squant'):
        raise ValueError("quantize_targ_layer: rounding must be 'nearest' or 'squant', got {!r}".format(rounding))
    print("Quantizing Layer parameters")
    if bits_bias == 32:
        print("Skipping bias quantization (32 bits)")
    assert targ_type != None, "targ_type cannot be None!"
    if rounding == 'squant':
        return _quantize_targ_layer_squant(graph, bit_weight, bits_bias, targ_type, return_codes, per_channel, signed)
    if per_channel:
        return _quantize_targ_layer_rows(graph, bit_weight, bits_bias, targ_type, return_codes, signed)
    lib = _ffi.lib()
    with torch.no_grad():
        stage = _ffi.entry_stage()
        segs, keep, codes = [], [], {}
        stage.prefetch([t for layer in graph.values() if type(layer) in targ_type for t in (layer.weight, layer.bias)])
        for key in graph:
            layer = graph[key]
            if type(layer) not in targ_type:
                continue
            w = stage.bind(layer.weight)
            c = None
            if return_codes:
                c = stage.new(w.shape, dtype=torch.int32)
                codes[key] = c
            segs.append(_ffi.DfqSegment(w.data_ptr(), w.numel(), int(bit_weight), int(bool(signed)), c.data_ptr() if c is not None else None))
            keep.append(w)
            if layer.bias is not None and bits_bias < 32:
                b = stage.bind(layer.bias)
                segs.append(_ffi.DfqSegment(b.data_ptr(), b.numel(), int(bits_bias), 0, None))
                keep.append(b)
        if segs:
            arr = (_ffi.DfqSegment * len(segs))(*segs)
            plan = ctypes.c_void_p()
            _ffi.check(lib.dfq_quant_plan_create(arr, len(segs), ctypes.byref(plan)))
            try:
                _ffi.check(lib.dfq_quant_plan_run(plan, _ffi.stream_arg()))
                _ffi.synchronize()
            finally:
                lib.dfq_quant_plan_destroy(plan)
        stage.writeback()
    if return_codes:
        return graph, codes
    return graph


def _quantize_targ_layer_rows(graph, bit_weight, bits_bias, targ_type, return_codes, signed):
    """quantize_targ_layer(per_channel=True): weight rows with their own ranges, biases per tensor (a segment of one row)."""
    for bits in (bit_weight,) + ((bits_bias,) if bits_bias < 32 else ()):
        if isinstance(bits, bool) or not isinstance(bits, int) or not 2 <= bits <= 16:
            raise ValueError('per-channel quantisation needs bit widths in [2, 16], got {!r}'.format(bits))
    lib = _ffi.lib()
    with torch.no_grad():
        stage = _ffi.entry_stage()
        segs, keep, codes, ranges = [], [], {}, {}
        stage.prefetch([t for layer in graph.values() if type(layer) in targ_type for t in (layer.weight, layer.bias)])
        for key in graph:
            layer = graph[key]
            if type(layer) not in targ_type:
                continue
            w = stage.bind(layer.weight)
            rows = int(w.shape[0])
            c = r = None
            if return_codes:
                c = stage.new(w.shape, dtype=torch.int32)
                r = stage.new((rows, 2))
                codes[key], ranges[key] = c, r
            segs.append(_ffi.DfqRowSegment(w.data_ptr(), rows, w.numel() // rows, int(bit_weight), int(bool(signed)),
                                           c.data_ptr() if c is not None else None, r.data_ptr() if r is not None else None))
            keep.append(w)
            if layer.bias is not None and bits_bias < 32:
                b = stage.bind(layer.bias)
                segs.append(_ffi.DfqRowSegment(b.data_ptr(), 1, b.numel(), int(bits_bias), 0, None, None))
                keep.append(b)
        if segs:
            arr = (_ffi.DfqRowSegment * len(segs))(*segs)
            plan = ctypes.c_void_p()
            _ffi.check(lib.dfq_row_quant_plan_create(arr, len(segs), ctypes.byref(plan)))
            try:
                _ffi.check(lib.dfq_row_quant_plan_run(plan, _ffi.stream_arg()))
                _ffi.synchronize()
            finally:
                lib.dfq_row_quant_plan_destroy(plan)
        stage.writeback()
    if return_codes:
        return graph, codes, ranges
    return graph


def _quantize_targ_layer_squant(graph, bit_weight, bits_bias, targ_type, return_codes, per_channel, signed):
    """quantize_targ_layer(rounding='squant'): every weight through dfq_squant_rows -- with its rows' own ranges per channel,
    with the tensor's (min, max) for every row otherwise -- then the biases through the plan of the nearest path."""
    if isinstance(bit_weight, bool) or not isinstance(bit_weight, int) or not 2 <= bit_weight <= 16:
        raise ValueError("rounding='squant' needs bit_weight in [2, 16], got {!r}".format(bit_weight))
    lib = _ffi.lib()
    with torch.no_grad():
        stage = _ffi.entry_stage()
        codes, ranges, biases = {}, {}, {}
        stage.prefetch([t for layer in graph.values() if type(layer) in targ_type for t in (layer.weight, layer.bias)])
        for key in graph:
            layer = graph[key]
            if type(layer) not in targ_type:
                continue
            w = stage.bind(layer.weight)
            rows = int(w.shape[0])
            klen = 1
            for d in w.shape[2:]:
                klen *= int(d)
            mins = maxs = None
            if not per_channel:
                mm, words = stage.new((2,)), stage.new((2,), dtype=torch.int32)
                _ffi.check(lib.dfq_tensor_minmax(_ffi.ptr(w), w.numel(), _ffi.ptr(mm), _ffi.ptr(words), _ffi.stream_arg()))
                mins, maxs = mm[0].repeat(rows), mm[1].repeat(rows)
            c = stage.new(w.shape, dtype=torch.int32) if return_codes else None
            if return_codes and per_channel:      # the rows' ranges, by the quantisers' rule (only the ranges are kept)
                ranges[key], unused = stage.new((rows, 2)), stage.new(w.shape)
                _ffi.check(lib.dfq_fake_quant_rows(_ffi.ptr(w), _ffi.ptr(unused), rows, w.numel() // rows, None, None,
                                                   int(bit_weight), int(bool(signed)), None, _ffi.ptr(ranges[key]), _ffi.stream_arg()))
            _ffi.check(lib.dfq_squant_rows(_ffi.ptr(w), _ffi.ptr(w), rows, w.numel() // rows, klen, _ffi.ptr(mins), _ffi.ptr(maxs),
                                           int(bit_weight), int(bool(signed)), _ffi.ptr(c), None, _ffi.stream_arg()))
            if return_codes:
                codes[key] = c
            if layer.bias is not None and bits_bias < 32:
                biases[key] = layer
        if biases:                                # the nearest path, on a graph of nothing but the biases
            _quantize_biases(biases, bits_bias, per_channel, stage)
        _ffi.synchronize()
        stage.writeback()
    if return_codes:
        return (graph, codes, ranges) if per_channel else (graph, codes)
    return graph


def _quantize_biases(layers, bits_bias, per_channel, stage):
    """the biases of {key: layer} as quantize_targ_layer's nearest path quantises them: per tensor, asymmetric -- through
    dfq_quant_plan, or through dfq_row_quant_plan (a segment of one row) where the weights go per channel"""
    lib = _ffi.lib()
    if per_channel and (isinstance(bits_bias, bool) or not isinstance(bits_bias, int) or not 2 <= bits_bias <= 16):
        raise ValueError('per-channel quantisation needs bit widths in [2, 16], got {!r}'.format(bits_bias))
    bound = [stage.bind(layer.bias) for layer in layers.values()]
    plan = ctypes.c_void_p()
    if per_channel:
        arr = (_ffi.DfqRowSegment * len(bound))(*[_ffi.DfqRowSegment(b.data_ptr(), 1, b.numel(), int(bits_bias), 0, None, None)
                                                  for b in bound])
        create, run, destroy = lib.dfq_row_quant_plan_create, lib.dfq_row_quant_plan_run, lib.dfq_row_quant_plan_destroy
    else:
        arr = (_ffi.DfqSegment * len(bound))(*[_ffi.DfqSegment(b.data_ptr(), b.numel(), int(bits_bias), 0, None) for b in bound])
        create, run, destroy = lib.dfq_quant_plan_create, lib.dfq_quant_plan_run, lib.dfq_quant_plan_destroy
    _ffi.check(create(arr, len(bound), ctypes.byref(plan)))
    try:
        _ffi.check(run(plan, _ffi.stream_arg()))
        _ffi.synchronize()
    finally:
        destroy(plan)


def find_prev_bn(bn_module, relu_attached, graph, bottoms, bot):
    """Breadth-first walk upwards from ``bot`` to the nearest BatchNorm on every path.

    Returns (bn_list, relu_attach_list, connect_type_list, targ_without_bn) like
    layer_transform.py:299-344: ``bn_list`` holds (bn module, branch id) where the branch id is a
    string of length = depth of the hit; the connect type ('one' / 'add' / 'add_<flag>' / 'cat')
    is inherited from the last add/cat node passed on the way up.
    """
    frontier = [(b, str(i)) for i, b in enumerate(bot)]
    ctype = {str(i): 'one' for i in range(len(bot))}
    bn_list, relu_list, connect_list = [], [], []
    no_bn_targets = {}
    merged = False
    while frontier:
        key, bid = frontier.pop(0)
        node = graph[key]
        if isinstance(node, str):
            if 'add' in key:
                ctype[bid] = 'add_{}'.format(relu_attached[key]) if key in relu_attached else 'add'
                merged = True
            elif 'cat' in key:
                ctype[bid] = 'cat'
                merged = True
        elif not merged and type(node) in _CONV_TYPES + _LINEAR_TYPES:
            print("Warning: {} layer before first batch norm layer detected. The calculated value range might be off.".format(type(node)))
            assert bid[0] not in no_bn_targets, "Multiple conv/linear layer without batch_norm is not supported."
            no_bn_targets[bid[0]] = ("conv" if type(node) in _CONV_TYPES else "linear", node)
        if key in bn_module:
            bn_list.append((bn_module[key], bid))
            relu_list.append(relu_attached[key])
            connect_list.append(ctype[bid])
        else:
            deeper = bid + bid[0]
            frontier.extend((up, deeper) for up in bottoms[key])
            ctype[deeper] = ctype[bid]
    return bn_list, relu_list, connect_list, no_bn_targets


# ------------------------------------------------------------------------------------------------
# set_quant_minmax (layer_transform.py:347-609)
# ------------------------------------------------------------------------------------------------
_RELU_MODE = {'none': 0, 'relu': 1, 'relu6': 2}


class _WalkError(AssertionError):
    """A graph the walk of set_quant_minmax refuses: the reference's assertion text (or the walk's own) and the key of the
    node it was met at."""

    def __init__(self, key, text):
        super().__init__(text)
        self.key = key


def _act_program(graph, bottoms, bn_type, targ_type, tensor_ops, is_detection):
    """The walk of set_quant_minmax (layer_transform.py:347-609) over ONE graph, compiled: [(graph key, one to one, results)]
    in the order the reference meets the quantised nodes.  A result is (index of the node's quantiser, steps) and stands for
    one (min, max); the results of a node come in the order the reference evaluates them.  A step is (opcode of _ffi.ACT_*,
    bn or None, relu mode, operand, case-(d) layer or None) and stands for one launch of the per-network entry points
    (ACT_CONST and ACT_RANGE_DIV: none).  ``one to one`` marks the nodes of :444-474, whose single-step results the
    per-network function resolves together at the end.

    Which nodes get results: layers with a ``.quant``, layers of a type in ``targ_type`` (their input range), and the tensor
    ops in ``tensor_ops = {graph key: number of quantisers}``.  Raises _WalkError where the reference asserts, and for the
    branches it cannot evaluate (it would trip over a missing moment vector or range there)."""
    A = _ffi
    tt = tuple(targ_type)
    bn_module, relu_attached, nodes = {}, {}, []
    for key in graph:
        bot = bottoms[key]
        if bot is None:
            continue
        layer = graph[key]
        if type(layer) == bn_type:
            bn_module[key] = layer
            relu_attached[key] = 'none'
            continue
        if type(layer) == torch.nn.ReLU:
            relu_attached[bot[0]] = 'relu'
        elif type(layer) == torch.nn.ReLU6:
            relu_attached[bot[0]] = 'relu6'
        if isinstance(layer, str):
            count = tensor_ops.get(key)
        elif hasattr(layer, 'quant') or type(layer) in tt:
            count = 1
        else:
            count = None
        if count is None:
            continue
        if len(bot) == 1 and bot[0] == 'Data':                     # :443-449 (only the first quantiser of the node is set)
            lo, hi = (-1.0, 1.0) if is_detection else (-2.11790393, 2.64)   # (x - mean) / std of the data pre-processing
            nodes.append((key, False, [(0, [(A.ACT_CONST, None, 0, (lo, hi), None)])]))
            continue
        try:
            bn_list, relu_list, connect_list, no_bn = find_prev_bn(bn_module, relu_attached, graph, bottoms, bot[:])
        except AssertionError as e:
            raise _WalkError(key, str(e)) from e
        if count == len(bn_list):                                   # 1 to 1 mapping (:444-474)
            results = []
            for (bn, bid), relu in zip(bn_list, relu_list):
                if bid[0] in no_bn:                                 # case (d): no ReLU clamp in the reference
                    results.append((len(results), [(A.ACT_RANGE, bn, 0, 0, no_bn[bid[0]])]))
                else:
                    results.append((len(results), [(A.ACT_RANGE, bn, _RELU_MODE[relu], 0, None)]))
            nodes.append((key, True, results))
            continue
        # ---- 1 to many / many to many (:476-601) ----
        branches = {}
        for ent, relu, ctype in zip(bn_list, relu_list, connect_list):
            branches.setdefault(ent[1][0], []).append((ent, relu, ctype))
        compiled = {}
        for bkey, items in branches.items():
            def bad(why):
                return _WalkError(key, 'branch {} {}'.format(bkey, why))
            items = sorted(items, key=lambda x: len(x[0][1]), reverse=True)
            (bn, bid), use_relu, connect_type = items.pop(0)
            depth = len(bid)
            moments = 'add' in connect_type
            steps = [(A.ACT_MOM if moments else A.ACT_RANGE, bn, _RELU_MODE[use_relu], 0, None)]
            while items:
                bound = 0
                while bound < len(items) and len(items[bound][0][1]) == depth:
                    bound += 1
                if bound == 0:
                    depth = len(items[0][0][1])                     # cut depth
                    continue
                for (bn, bid), relu_t, connect_type in items[:bound]:
                    if 'add' in connect_type:
                        if not moments:
                            raise bad('meets an add after a cat / plain connection')
                        steps.append((A.ACT_MOM_ADD, bn, _RELU_MODE[relu_t], 0, None))
                        if 'relu6' in connect_type:
                            steps.append((A.ACT_MOM_RELU, None, 2, 0, None))
                        elif 'relu' in connect_type:
                            steps.append((A.ACT_MOM_RELU, None, 1, 0, None))
                    elif moments:
                        raise bad('meets a cat / plain connection after an add')
                    elif connect_type == 'cat':
                        steps.append((A.ACT_RANGE_CAT, bn, _RELU_MODE[relu_t], 0, None))
                    else:   # `if use_relu_tmp` of the reference is always true (a non-empty string): no ReLU mode, clamp at 0
                        steps.append((A.ACT_RANGE_ONE, bn, 0, 0, None))
                items = items[bound:]
                if connect_type == 'one':                           # (of the LAST item, as in the reference)
                    if moments:
                        raise bad('meets a cat / plain connection after an add')
                    steps.append((A.ACT_RANGE_DIV, None, 0, bound + 1, None))
            if ('add' in connect_type) != moments:
                raise bad('mixes adds with cat / plain connections')
            if moments:
                steps.append((A.ACT_MOM_RANGE, None, 0, 0, None))
            compiled[bkey] = steps
        if count == 1 and count < len(bn_list):                     # 1 to many
            if len(compiled) != 1:
                raise _WalkError(key, 'Error occurs when setting min/max, should be 1 to many')
            nodes.append((key, False, [(0, steps)]))
        elif count < len(bn_list):                                  # many to many
            if len(compiled) != count or any(str(i) not in compiled for i in range(count)):
                raise _WalkError(key, 'LENGTH NOT EQUAL {} vs {}'.format(len(compiled), count))
            nodes.append((key, False, [(int(bkey), steps) for bkey, steps in compiled.items()]))
        else:
            raise _WalkError(key, 'Unknown error occured while setting min/max')
    return nodes


class _Moments:
    """(mean, var) channel vectors of one branch, living on the device (layer_transform.py:494-540)."""

    def __init__(self, stage, n):
        self.stage = stage
        self.n = n
        self.mean = stage.new((n,))
        self.var = stage.new((n,))

    def add_source(self, bn, relu_mode, accumulate):
        lib = _ffi.lib()
        w, b = self.stage.bind(bn.fake_weight), self.stage.bind(bn.fake_bias)
        _ffi.check(lib.dfq_relu_moments(_ffi.ptr(w), _ffi.ptr(b), self.n, relu_mode, _ffi.ptr(self.mean),
                                        _ffi.ptr(self.var), int(accumulate), _ffi.stream_arg()))

    def relu_after_add(self, mode, eps):
        _ffi.check(_ffi.lib().dfq_moments_after_add(_ffi.ptr(self.mean), _ffi.ptr(self.var), self.n, mode, eps,
                                                    _ffi.stream_arg()))

    def value_range(self, eps, n_sigma):
        out = self.stage.new((2,))
        _ffi.check(_ffi.lib().dfq_moment_range(_ffi.ptr(self.mean), _ffi.ptr(self.var), self.n, eps, float(n_sigma),
                                               _ffi.ptr(out), _ffi.stream_arg()))
        lo, hi = out.tolist()
        return lo, hi


def _bn_ranges(stage, reqs, n_sigma):
    """[(fake_weight, fake_bias, relu mode)] -> [(min, max)] with the ReLU clamps: ONE launch, one read-back."""
    if not reqs:
        return []
    lib = _ffi.lib()
    arr = (_ffi.DfqBnRangeReq * len(reqs))()
    keep = []
    for i, (fw, fb, relu_mode) in enumerate(reqs):
        w, b = stage.bind(fw).reshape(-1), stage.bind(fb).reshape(-1)
        keep.append((w, b))
        arr[i] = _ffi.DfqBnRangeReq(w.data_ptr(), b.data_ptr(), w.numel(), relu_mode)
    out = stage.new((len(reqs), 2))
    scratch = stage.new((int(lib.dfq_bn_ranges_scratch_bytes(len(reqs))) // 4 + 1,), dtype=torch.int32)
    _ffi.check(lib.dfq_bn_ranges(arr, len(reqs), float(n_sigma), _ffi.ptr(out), _ffi.ptr(scratch), _ffi.stream_arg()))
    return [tuple(r) for r in out.tolist()]


def _through_layer(stage, layer, kind, vec):
    """A BN proxy vector through a conv / linear layer that has no BN of its own (case d, :455-463)."""
    lib = _ffi.lib()
    w = stage.bind(layer.weight)
    khkw = w[0, 0].numel() if w.dim() == 4 else 1
    out = stage.new((w.shape[0],))
    _ffi.check(lib.dfq_bn_through_layer(_ffi.ptr(w), w.shape[0], w.shape[1], khkw, getattr(layer, 'groups', 1) if kind == 'conv' else 1,
                                        _ffi.ptr(stage.bind(layer.bias)), _ffi.ptr(stage.bind(vec).reshape(-1)), _ffi.ptr(out),
                                        _ffi.stream_arg()))
    return out


def set_quant_minmax(graph, bottoms, is_detection=False, bn_type=torch.nn.BatchNorm2d, N=6, verbose=True,
                     tensor_op_quant=None):
    """Set ``running_min`` / ``running_max`` of every activation quantiser from the statistics of the
    BatchNorm layers in front of it (layer_transform.py:347-609); no data involved.

    Quantisers are the ``.quant`` modules of the Q*Conv2d / Q*Linear layers.  The reference additionally
    serves quantisers of tensor ops (QuantAdd, ...) that its ``replace_op`` registers in a module global
    of the PyTransformer machinery; a caller that has such modules passes them as
    ``tensor_op_quant = {graph key of the op: [QuantMeasure, ...]}``.  Same cases as the reference:
    1 BN -> 1 quantiser (:444-474), 1 quantiser fed by several BNs through add / cat (:476-580), several
    quantisers of one tensor op (:582-601), and a conv / linear without BN in between (case d).

    The walk is ``_act_program``; this function executes its steps, one launch each, except that the
    1-to-1 results of the whole graph share ONE launch at the end.
    """
    if verbose:
        print("SET QUANT MIN MAX")
    A = _ffi
    eps = 1e-6
    stage = _ffi.entry_stage()
    op_quant = {k: v for k, v in (tensor_op_quant or {}).items() if v is not None}
    one_to_one = []          # (quantiser, fake_weight, fake_bias, relu mode) resolved with one launch at the end

    def fill(q, lo, hi):
        q.running_max.fill_(hi)
        q.running_min.fill_(lo)
    with torch.no_grad():
        for key, is_one_to_one, results in _act_program(graph, bottoms, bn_type, (), {k: len(v) for k, v in op_quant.items()},
                                                        is_detection):
            quant_module = op_quant[key] if isinstance(graph[key], str) else [graph[key].quant]
            values = {}
            for idx, steps in results:
                mom = lo = hi = None
                for op, bn, relu, operand, through in steps:
                    if op == A.ACT_CONST:
                        lo, hi = operand
                    elif is_one_to_one:
                        fw, fb = bn.fake_weight, bn.fake_bias
                        if through is not None:                     # case (d)
                            kind, obj = through
                            fb = _through_layer(stage, obj, kind, bn.fake_bias)
                            fw = _through_layer(stage, obj, kind, bn.fake_weight)
                        one_to_one.append((quant_module[idx], fw, fb, relu))
                    elif op == A.ACT_MOM:
                        mom = _Moments(stage, bn.fake_bias.numel())
                        mom.add_source(bn, relu, accumulate=False)
                    elif op == A.ACT_MOM_ADD:
                        mom.add_source(bn, relu, accumulate=True)
                    elif op == A.ACT_MOM_RELU:
                        mom.relu_after_add(relu, eps)
                    elif op == A.ACT_MOM_RANGE:
                        lo, hi = mom.value_range(eps, N)
                    elif op == A.ACT_RANGE_DIV:
                        lo /= operand
                        hi /= operand
                    else:
                        (r_lo, r_hi), = _bn_ranges(stage, [(bn.fake_weight, bn.fake_bias, relu)], N)
                        if op == A.ACT_RANGE:
                            lo, hi = r_lo, r_hi
                        elif op == A.ACT_RANGE_CAT:
                            lo, hi = min(lo, r_lo), max(hi, r_hi)
                        else:                                       # ACT_RANGE_ONE
                            lo += max(0., r_lo)
                            hi += r_hi
                if lo is not None:
                    values[idx] = (lo, hi)
            for idx in sorted(values):
                fill(quant_module[idx], *values[idx])
        ranges = _bn_ranges(stage, [(fw, fb, relu) for (_, fw, fb, relu) in one_to_one], N)
        for (q, _, _, _), (lo, hi) in zip(one_to_one, ranges):
            fill(q, lo, hi)
