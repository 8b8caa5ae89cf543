"""Stand-alone steps of the calibration path (C ABI section "Stand-alone steps").

Thin ctypes wrappers: every function stages its tensor arguments on the GPU (in place when they already
live there), calls ONE entry point of libdfq_hip.so and returns device-side results moved back to the
caller's device.  The plans in dfq_amd.dfq are the fast path; these exist so that a caller can drive the
reference's algorithm step by step (dfq.py:28-75, :105-108, :281-287) and for the per-channel quantiser.
"""
from __future__ import annotations

import torch

from . import _ffi


def _weight_geometry(w):
    out_ch = w.shape[0]
    in_per_group = w.shape[1]
    khkw = w[0, 0].numel() if w.dim() > 2 else 1
    return out_ch, in_per_group, khkw


def row_range(weight, signed=False):
    """range of every output row of `weight` (dfq.py:50-55 on the first layer) -> float32 [O]."""
    lib = _ffi.lib()
    with torch.no_grad():
        stage = _ffi.Stage()
        w = stage.bind(weight)
        out = stage.new((w.shape[0],))
        _ffi.check(lib.dfq_row_range(_ffi.ptr(w), w.shape[0], w[0].numel(), int(bool(signed)), _ffi.ptr(out),
                                     _ffi.stream_arg()))
        return stage.out_like(weight, out)


def col_range(weight_second, first_out_channels, signed=False):
    """range of every paired input channel of the second layer (the view of dfq.py:41-46) -> float32 [O1]."""
    lib = _ffi.lib()
    with torch.no_grad():
        stage = _ffi.Stage()
        w = stage.bind(weight_second)
        o2, i2g, khkw = _weight_geometry(w)
        groups = first_out_channels // i2g if first_out_channels != i2g else 1
        out = stage.new((groups * i2g,))
        _ffi.check(lib.dfq_col_range(_ffi.ptr(w), o2, i2g, khkw, groups, int(bool(signed)), _ffi.ptr(out),
                                     _ffi.stream_arg()))
        return stage.out_like(weight_second, out)


def le_solve(r1, r2, s_range=(1e-8, 1e8), eps=0):
    """(S, 1/S as the reference applies it) from the two range vectors (dfq.py:58-59, :73)."""
    lib = _ffi.lib()
    with torch.no_grad():
        stage = _ffi.Stage()
        a, b = stage.bind(r1), stage.bind(r2)
        s, inv = stage.new(a.shape), stage.new(a.shape)
        _ffi.check(lib.dfq_le_solve(_ffi.ptr(a), _ffi.ptr(b), a.numel(), float(eps), float(s_range[0]), float(s_range[1]),
                                    _ffi.ptr(s), _ffi.ptr(inv), _ffi.stream_arg()))
        return stage.out_like(r1, s), stage.out_like(r1, inv)


def le_apply(weight_first, weight_second, bias_first, bn_weight, bn_bias, S, Sinv):
    """In place: W1 rows, b1, BN proxies *= S; W2 input channels *= Sinv (dfq.py:62-73)."""
    lib = _ffi.lib()
    with torch.no_grad():
        stage = _ffi.Stage()
        w1, w2 = stage.bind(weight_first), stage.bind(weight_second)
        o2, i2g, khkw = _weight_geometry(w2)
        _ffi.check(lib.dfq_le_apply(_ffi.ptr(w1), w1.shape[0], w1[0].numel(), _ffi.ptr(w2), o2, i2g, khkw,
                                    _ffi.ptr(stage.bind(bias_first)), _ffi.ptr(stage.bind(bn_weight)),
                                    _ffi.ptr(stage.bind(bn_bias)), _ffi.ptr(stage.bind(S)), _ffi.ptr(stage.bind(Sinv)),
                                    _ffi.stream_arg()))
        stage.writeback()


def le_pair(weight_first, weight_second, bias_first, bn_weight=None, bn_bias=None, s_range=(1e-8, 1e8),
            signed=False, eps=0):
    """_layer_equalization (dfq.py:28-75) through the stand-alone steps; returns S."""
    lib = _ffi.lib()
    with torch.no_grad():
        stage = _ffi.Stage()
        w1, w2 = stage.bind(weight_first), stage.bind(weight_second)
        o2, i2g, khkw = _weight_geometry(w2)
        o1 = w1.shape[0]
        S = stage.new((o1,))
        work = stage.new((3 * o1,))
        _ffi.check(lib.dfq_le_pair(_ffi.ptr(w1), o1, w1[0].numel(), _ffi.ptr(w2), o2, i2g, khkw,
                                   _ffi.ptr(stage.bind(bias_first)), _ffi.ptr(stage.bind(bn_weight)),
                                   _ffi.ptr(stage.bind(bn_bias)), float(s_range[0]), float(s_range[1]),
                                   int(bool(signed)), float(eps), _ffi.ptr(S), _ffi.ptr(work), _ffi.stream_arg()))
        stage.writeback()
        return stage.out_like(weight_first, S)


def absdiff_mean(weight, prev):
    """float(torch.mean(torch.abs(weight - prev))) of dfq.py:108 as a Python float."""
    lib = _ffi.lib()
    with torch.no_grad():
        stage = _ffi.Stage()
        a, b = stage.bind(weight), stage.bind(prev)
        n = a.numel()
        out = stage.new((1,))
        scratch = stage.new((int(lib.dfq_absdiff_mean_scratch_bytes(n)) // 8 + 1,), dtype=torch.float64)
        _ffi.check(lib.dfq_absdiff_mean(_ffi.ptr(a), _ffi.ptr(b), n, _ffi.ptr(out), _ffi.ptr(scratch), _ffi.stream_arg()))
        return float(out.item())


def fake_quant_rows(x, num_bits=8, min_values=None, max_values=None, symmetric=False, return_codes=False):
    """Per-output-channel fake-quant: row r of `x` (first dimension) with its own (min, max)."""
    lib = _ffi.lib()
    with torch.no_grad():
        stage = _ffi.Stage()
        xx = stage.bind(x)
        rows, row_len = xx.shape[0], xx[0].numel()
        y = stage.new(xx.shape)
        codes = stage.new(xx.shape) if return_codes else None
        mm = stage.new((rows, 2))
        _ffi.check(lib.dfq_fake_quant_rows(_ffi.ptr(xx), _ffi.ptr(y), rows, row_len, _ffi.ptr(stage.bind(min_values)),
                                           _ffi.ptr(stage.bind(max_values)), int(num_bits), int(bool(symmetric)),
                                           _ffi.ptr(codes), _ffi.ptr(mm), _ffi.stream_arg()))
        res = stage.out_like(x, y)
        if return_codes:
            return res, stage.out_like(x, codes), stage.out_like(x, mm)
        return res


def squant_rows(x, kernel_len=1, num_bits=8, min_values=None, max_values=None, symmetric=False, return_codes=False,
                return_stats=False):
    """Adaptive rounding (SQuant; dfq_squant_rows, "Adaptive rounding" in include/dfq_hip.h) of the rows of `x` (first
    dimension): the grid of fake_quant_rows -- each row's own (min, max), or the given ones -- but the roundings that cost least
    are flipped until the rounding errors of every run of `kernel_len` elements and of every row sum to at most half a quantum.
    Returns the quantised tensor, then the int32 codes (``return_codes``), then int64 [rows, 2] = (the row's remaining error
    sum in units of 2^-30 quanta, the number of flipped codes) (``return_stats``)."""
    lib = _ffi.lib()
    with torch.no_grad():
        stage = _ffi.Stage()
        xx = stage.bind(x)
        rows, row_len = xx.shape[0], xx[0].numel()
        y = stage.new(xx.shape)
        codes = stage.new(xx.shape, dtype=torch.int32) if return_codes else None
        stats = stage.new((rows, 2), dtype=torch.int64) if return_stats else None
        _ffi.check(lib.dfq_squant_rows(_ffi.ptr(xx), _ffi.ptr(y), rows, row_len, int(kernel_len), _ffi.ptr(stage.bind(min_values)),
                                       _ffi.ptr(stage.bind(max_values)), int(num_bits), int(bool(symmetric)), _ffi.ptr(codes),
                                       _ffi.ptr(stats), _ffi.stream_arg()))
        res = [stage.out_like(x, y)]
        if return_codes:
            res.append(stage.out_like(x, codes))
        if return_stats:
            res.append(stage.out_like(x, stats))
        return res[0] if len(res) == 1 else tuple(res)


MX_FORMATS = {'e2m1': _ffi.MX_E2M1, 'e2m3': _ffi.MX_E2M3, 'e3m2': _ffi.MX_E3M2, 'e4m3': _ffi.MX_E4M3, 'e5m2': _ffi.MX_E5M2}


def mx_rows(x, format='e2m1', search=True):
    """MX block-scaled quantisation (dfq_mx_rows, "MX block-scaled" in include/dfq_hip.h) of the rows of `x` (first dimension):
    every run of 32 consecutive elements of a row -- the last one of a row may be short -- shares one power-of-two scale, and
    an element becomes the nearest code of `format` ('e2m1', 'e2m3', 'e3m2', 'e4m3' or 'e5m2'; ties to the even code,
    saturating).  ``search`` chooses between the floor exponent and the one above it by the block's own sum of squared errors.
    Returns (the stored weights shaped like `x`, uint8 codes shaped like `x`, uint8 scale bytes [rows, ceil(row_len / 32)],
    float64 block errors of the same shape).  One launch."""
    if format not in MX_FORMATS:
        raise ValueError('mx_rows: format must be one of {}, got {!r}'.format(sorted(MX_FORMATS), format))
    lib = _ffi.lib()
    with torch.no_grad():
        stage = _ffi.Stage()
        xx = stage.bind(x)
        rows, row_len = xx.shape[0], xx[0].numel()
        bpr = -(-row_len // _ffi.MX_BLOCK)
        y = stage.new(xx.shape)
        codes = stage.new(xx.shape, dtype=torch.uint8)
        scales = stage.new((rows, bpr), dtype=torch.uint8)
        err = stage.new((rows, bpr), dtype=torch.float64)
        _ffi.check(lib.dfq_mx_rows(_ffi.ptr(xx), _ffi.ptr(y), rows, row_len, MX_FORMATS[format], int(bool(search)), _ffi.ptr(codes),
                                   _ffi.ptr(scales), _ffi.ptr(err), _ffi.stream_arg()))
        return tuple(stage.out_like(x, t) for t in (y, codes, scales, err))


def _mx_axis_geometry(who, x, axis, format):
    """(format id, axis >= 0, outer, len, inner) of `x` cut along `axis`, or the ValueError"""
    if format not in MX_FORMATS:
        raise ValueError('{}: format must be one of {}, got {!r}'.format(who, sorted(MX_FORMATS), format))
    if not isinstance(axis, int) or isinstance(axis, bool) or not -x.dim() <= axis < x.dim():
        raise ValueError('{}: axis {!r} is outside a tensor of {} dimensions'.format(who, axis, x.dim()))
    axis %= x.dim()
    outer = 1
    for n in x.shape[:axis]:
        outer *= int(n)
    inner = 1
    for n in x.shape[axis + 1:]:
        inner *= int(n)
    return MX_FORMATS[format], axis, outer, int(x.shape[axis]), inner


def mx_axis(x, axis=1, format='e4m3', search=False, outputs=('y', 'codes', 'scales', 'err')):
    """MX block-scaled quantisation (dfq_mx_axis, "MX block-scaled" in include/dfq_hip.h) of `x` along `axis` (negative axes
    count from the end): every run of 32 consecutive elements along that axis -- the last run may be short -- shares one
    power-of-two scale, all other indices fixed.  Channel blocks of an NCHW activation are ``axis=1``; a 2-D tensor with
    ``axis=1`` (or any tensor with the last axis) is the row case of mx_rows.  The result is exactly mx_rows on the tensor with
    the axis moved last, moved back, without the two transposes.  ``search`` as in mx_rows (activations: off by default).
    Returns (the stored values shaped like `x`, uint8 codes shaped like `x`, uint8 scale bytes and float64 block errors shaped
    like `x` with `axis` reduced to ceil(len / 32)).  ``outputs`` names the ones that are wanted; the others are not computed
    and come back as None.  A non-contiguous `x` is made contiguous first.  One launch."""
    fmt, axis, outer, length, inner = _mx_axis_geometry('mx_axis', x, axis, format)
    lib = _ffi.lib()
    with torch.no_grad():
        stage = _ffi.Stage()
        xx = stage.bind(x)
        small = tuple(xx.shape[:axis]) + (-(-length // _ffi.MX_BLOCK),) + tuple(xx.shape[axis + 1:])
        y = stage.new(xx.shape) if 'y' in outputs else None
        codes = stage.new(xx.shape, dtype=torch.uint8) if 'codes' in outputs else None
        scales = stage.new(small, dtype=torch.uint8) if 'scales' in outputs else None
        err = stage.new(small, dtype=torch.float64) if 'err' in outputs else None
        _ffi.check(lib.dfq_mx_axis(_ffi.ptr(xx), _ffi.ptr(y), outer, length, inner, fmt, int(bool(search)), _ffi.ptr(codes),
                                   _ffi.ptr(scales), _ffi.ptr(err), _ffi.stream_arg()))
        return tuple(None if t is None else stage.out_like(x, t) for t in (y, codes, scales, err))


def zeroq_quant_rows(x, num_bits=8, min_values=None, max_values=None, return_codes=False):
    """ZeroQ's per-output-channel asymmetric quantiser (quant_utils.py:85-135 via quant_modules.py:161-171)."""
    lib = _ffi.lib()
    with torch.no_grad():
        stage = _ffi.Stage()
        xx = stage.bind(x)
        rows, row_len = xx.shape[0], xx[0].numel()
        y = stage.new(xx.shape)
        codes = stage.new(xx.shape) if return_codes else None
        _ffi.check(lib.dfq_zeroq_quant_rows(_ffi.ptr(xx), _ffi.ptr(y), rows, row_len, _ffi.ptr(stage.bind(min_values)),
                                            _ffi.ptr(stage.bind(max_values)), int(num_bits), _ffi.ptr(codes), None,
                                            _ffi.stream_arg()))
        res = stage.out_like(x, y)
        return (res, stage.out_like(x, codes)) if return_codes else res


def grouped_matvec(eps, expect, groups=1):
    """bias[o] = eps[o, :] . expect[group(o)] (dfq.py:281-287) -> float32 [O]."""
    lib = _ffi.lib()
    with torch.no_grad():
        stage = _ffi.Stage()
        e, x = stage.bind(eps), stage.bind(expect)
        out = stage.new((e.shape[0],))
        _ffi.check(lib.dfq_grouped_matvec(_ffi.ptr(e), _ffi.ptr(x), e.shape[0], e.shape[1], int(groups), _ffi.ptr(out),
                                          _ffi.stream_arg()))
        return stage.out_like(eps, out)


HIST_MAX_BINS = 4096          # kHistMaxBins of dfq_act_hist.hip
HIST_METHODS = {'percentile': 0, 'mse': 1}


def _device_f32(t, dev):
    """float32, contiguous, on the engine's device -- the tensor itself when it already is"""
    if not torch.is_tensor(t):
        t = torch.tensor(t, dtype=torch.float32)
    t = t.detach()
    if t.device != dev or t.dtype is not torch.float32:
        t = t.to(device=dev, dtype=torch.float32)
    return t.contiguous()


def act_histogram(x, range2, bins=2048, counts=None):
    """counts[slot] += 1 for every element of `x` over the range (lo, hi) = `range2`, by dfq_act_hist_accumulate (the slot
    rule: include/dfq_hip.h) -> int64 [bins + 3] on the engine's device: the bins, then below, above, nan.  The counts are the
    library's uint64 (torch reduces and communicates int64; a count stays far below 2^63).

    ``range2``: a float32 [2] tensor -- read on the device, nothing waits for it -- or a pair of numbers.  ``counts``: a
    contiguous int64 [bins + 3] tensor on the engine's device to add to (a slice of a table of yours); None makes a zeroed one.
    An `x` that is not float32, not contiguous, on another device or not 16-byte aligned is copied first."""
    bins = int(bins)
    if not 2 <= bins <= HIST_MAX_BINS:
        raise ValueError('act_histogram: bins is 2 ... {}, not {}'.format(HIST_MAX_BINS, bins))
    lib = _ffi.lib()
    dev = _ffi.target_device()
    with torch.no_grad():
        if counts is None:
            counts = torch.zeros(bins + 3, dtype=torch.int64, device=dev)
        if (counts.dtype is not torch.int64 or counts.dim() != 1 or counts.numel() != bins + 3 or not counts.is_contiguous()
                or counts.device != dev):
            raise ValueError('act_histogram: counts is a contiguous int64 vector [bins + 3] on {}'.format(dev))
        r = _device_f32(range2, dev).reshape(-1)
        if r.numel() != 2:
            raise ValueError('act_histogram: range2 is (lo, hi)')
        xx = _device_f32(x, dev)
        if xx.data_ptr() % 16:
            xx = xx.clone()                                 # (a view into the middle of a buffer: the kernel's loads are 16-byte)
        _ffi.check(lib.dfq_act_hist_accumulate(_ffi.ptr(xx), xx.numel(), _ffi.ptr(r), bins, _ffi.ptr(counts), _ffi.stream_arg()))
    return counts


def hist_clip_range(counts, range2, num_bits=8, method='mse', percentile=0.9999, candidates=None):
    """The clipped range of one histogram ([bins + 3] counts, [2] range -> float32 [2]) or of several in ONE launch
    ([n, bins + 3], [n, 2] -> [n, 2]) by dfq_hist_clip_range; the definitions are in include/dfq_hip.h.

    ``method``: 'mse' searches ``candidates`` (default bins // 2) edges from each end for the range of least modelled
    quantisation error at ``num_bits``; 'percentile' keeps the central ``percentile`` of the mass on either side.
    ``num_bits``: one width in [2, 16] for all histograms, or one per histogram (a sequence or an integer tensor; a tensor on
    the engine's device is validated by the caller, not here: reading it would wait for the device)."""
    if method not in HIST_METHODS:
        raise ValueError("hist_clip_range: method is 'mse' or 'percentile', not {!r}".format(method))
    lib = _ffi.lib()
    dev = _ffi.target_device()
    with torch.no_grad():
        single = counts.dim() == 1
        c = counts.detach()
        if c.dtype is not torch.int64:
            raise ValueError('hist_clip_range: counts is int64 (the table act_histogram fills)')
        c = c.to(dev).contiguous().reshape(1 if single else c.shape[0], -1)
        n_hist, bins = int(c.shape[0]), int(c.shape[1]) - 3
        if not 2 <= bins <= HIST_MAX_BINS:
            raise ValueError('hist_clip_range: counts is [..., bins + 3] with 2 ... {} bins'.format(HIST_MAX_BINS))
        r = _device_f32(range2, dev).reshape(-1, 2)
        if r.shape[0] != n_hist:
            raise ValueError('hist_clip_range: {} ranges for {} histograms'.format(r.shape[0], n_hist))
        if torch.is_tensor(num_bits) and num_bits.device == dev and dev.type == 'cuda':
            bits = num_bits.to(torch.int32).contiguous().reshape(-1)
        else:
            if torch.is_tensor(num_bits):
                num_bits = num_bits.reshape(-1).tolist()
            host = [int(b) for b in num_bits] if hasattr(num_bits, '__len__') else [int(num_bits)]
            if len(host) == 1:
                host = host * n_hist
            if any(b < 2 or b > 16 for b in host):
                raise ValueError('hist_clip_range: num_bits is 2 ... 16, not {}'.format(sorted(set(host))))
            bits = torch.tensor(host, dtype=torch.int32).to(dev)
        if bits.numel() != n_hist:
            raise ValueError('hist_clip_range: {} bit widths for {} histograms'.format(bits.numel(), n_hist))
        if candidates is None:
            candidates = bins // 2
        out = torch.empty((n_hist, 2), dtype=torch.float32, device=dev)
        _ffi.check(lib.dfq_hist_clip_range(_ffi.ptr(c), _ffi.ptr(r), n_hist, bins, _ffi.ptr(bits), HIST_METHODS[method],
                                           float(percentile), int(candidates), _ffi.ptr(out), _ffi.stream_arg()))
        out = out.to(counts.device) if out.device != counts.device else out
    return out[0] if single else out
