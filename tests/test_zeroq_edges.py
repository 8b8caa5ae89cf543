"""Row f2 at the edges: the BatchNorm-statistics loss kernels (dfq_amd/csrc/dfq_zeroq.hip) on degenerate and
ill-conditioned rows, at every launch shape, through every entry point.

Reference: the float64 oracle (oracle.dfq_oracle.bn_stat_losses / bn_stat_rows).  Next to it run the reference's own
torch expressions (distill_data.py:172-196) with autograd: in float64 to validate the oracle on every case (1e-10), in
float32 to measure what any float32 evaluation loses on the ill-conditioned ones.  Every case calls the C ABI directly
with guard elements around each buffer, so row_mean / row_std are compared as well and a stray write is seen.

Tolerances: losses, row_mean, row_std |got - ref| <= 1e-5 max(1, |ref|) (tests.common.assert_close) on EVERY case;
gradients rtol 1e-4 / atol 1e-6 against the oracle on the well-conditioned ones.  Ill-conditioned gradients (a large offset
with a small spread, one element 1 ulp off): (x + eps) - mean loses digits in ANY float32 evaluation, so the error is taken
in the max norm relative to max|grad_f64|, measured for the reference's float32 autograd in the same way, and the engine
must stay within max(1e-4, 2 x the reference's error) -- 2 for the differing summation order of two float32 evaluations;
a cancellation defect misses it by orders of magnitude.

Measured pairs "engine, reference float32" (max norm relative to max|grad_f64|; printed by every run with -s):

    case                                               emulation
    1 ulp off, base 0.37, hw 49                        2.1e-02, 1.0e+00
    1 ulp off, base 0.37, hw 1025                      9.8e-04, 9.8e-04
    1 ulp off, base -5, hw 49                          1.7e-02, 8.3e-01
    1 ulp off, base -5, hw 1025                        9.3e-04, 9.5e-01
    1 ulp off, base 3e4, hw 49                         1.3e-05, 1.3e-05
    1 ulp off, base 3e4, hw 1025                       2.9e-06, 2.8e-06
    1e3 + randn, 7x7                                   1.5e-07, 3.1e-07
    1e3 + randn, 112x112                               1.3e-07, 1.6e-07
    3e4 + 0.01 randn, 7x7                              6.4e-06, 1.1e-05
    3e4 + 0.01 randn, 112x112                          5.2e-07, 5.2e-07
    -3e4 + 0.01 randn, 7x7                             6.5e-06, 1.1e-05
    -3e4 + 0.01 randn, 112x112                         4.5e-07, 4.7e-07
    1e3 + randn, matching statistics, hw 49            8.0e-06, 4.7e-05
    1e3 + randn, matching statistics, hw 12544         7.0e-06, 2.0e-05
    +-3e4 + 0.01 randn, matching statistics, hw 49     7.5e-02, 8.5e-02
    +-3e4 + 0.01 randn, matching statistics, hw 12544  3.7e-03, 3.7e-03
(MI355X: not measured yet -- the gpu cases print the same lines.  With the default statistics the mean term,
2 (offset - bn_mean) / (C HW), dominates max|grad|; "matching statistics" puts bn_mean at the offset and bn_std at the
spread, so the std term is what is measured.)
"""
import numpy as np
import pytest
import torch

from dfq_amd import _ffi, zeroq
from oracle import dfq_oracle as orc
from tests.common import F32, assert_bitexact, assert_close, npy
from tests.test_zeroq import _reference_losses

GUARD = 16                      # elements in front of and behind every buffer handed to the library
SENTINEL = -777.25
W_MEAN, W_STD = 0.7, 1.3        # upstream gradients of the two losses


# ---- the reference's own expressions ------------------------------------------------------------------------------
def _reference_expr(x, bn_mean, bn_std, eps, denom):
    """distill_data.py:172-190 (`_reference_losses`), its H*W == 1 branch (:181-182) and, with `denom`, the input-batch
    term of :192-196 (statistics first, so own_loss divides by the batch size)."""
    own_loss = lambda A, B: (A - B).norm() ** 2 / A.size(0)
    n, c = x.shape[:2]
    if denom is not None:
        assert denom == n
        tmp_mean = torch.mean(x.view(n, c, -1), dim=2)
        tmp_std = torch.std(x.view(n, c, -1) + eps, dim=2)
        return own_loss(tmp_mean, bn_mean.view(1, c)), own_loss(tmp_std, bn_std.view(1, c))
    if x[0, 0].numel() == 1:
        tmp_mean = torch.mean(x.view(n, c, -1), dim=2)
        tmp_std = torch.std(x.view(c, -1) + eps, dim=1)
        return own_loss(bn_mean, tmp_mean), own_loss(bn_std, tmp_std)
    return _reference_losses(x, bn_mean, bn_std, eps)


def _reference_f32(x, bn_mean, bn_std, eps, denom):
    xr = x.clone().requires_grad_(True)
    ml, sl = _reference_expr(xr, bn_mean, bn_std, eps, denom)
    (ml * W_MEAN + sl * W_STD).backward()
    return float(ml.detach()), float(sl.detach()), xr.grad.numpy().astype(np.float64)


def _reference_f64(x, bn_mean, bn_std, eps, denom, shift):
    """The same expressions in float64.  x + eps is rounded in float32 by reference and engine alike, so the std term is
    taken over e = float32(x + eps) (with eps = 0 from there on) and the mean term over x; d/dx = d/de.  `shift`: a row
    whose spread is at the float32 rounding level (constant, one element 1 ulp off) is beyond float64's own 2^-53 / 2^-24
    resolution, so each std row is first centred on its first element -- exact in float64, and std does not see a shift."""
    x64 = x.double().requires_grad_(True)
    e = (x + torch.tensor(eps, dtype=torch.float32)).double()
    if shift:
        n, c = x.shape[:2]
        rows = e.view(c, -1) if x[0, 0].numel() == 1 else e.view(n * c, -1)
        e = (rows - rows[:, :1]).view(x.shape)
    e64 = e.clone().requires_grad_(True)
    bm, bs = bn_mean.double(), bn_std.double()
    ml = _reference_expr(x64, bm, bs, 0.0, denom)[0]
    sl = _reference_expr(e64, bm, bs, 0.0, denom)[1]
    (ml * W_MEAN + sl * W_STD).backward()
    return float(ml.detach()), float(sl.detach()), (x64.grad + e64.grad).numpy()


# ---- the C ABI with guard elements --------------------------------------------------------------------------------
class _Guarded:
    def __init__(self, engine, n, init=None, dtype=torch.float32):
        self.n = n
        host = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype)
        if init is not None:
            host[GUARD:GUARD + n] = init.reshape(-1).to(dtype)
        self.host0 = host.clone()
        self.buf = engine.to(host)
        self.view = self.buf[GUARD:GUARD + n]

    def ptr(self):
        return _ffi.ptr(self.view)

    def check_guards(self, what):
        got = self.buf.cpu()
        assert torch.equal(got[:GUARD], self.host0[:GUARD]) and torch.equal(got[GUARD + self.n:], self.host0[GUARD + self.n:]), \
            '{}: a guard element was written'.format(what)

    def check_unchanged(self, what):
        got, want = self.buf.cpu(), self.host0
        same = (got == want) | (torch.isnan(got) & torch.isnan(want))
        assert bool(same.all()), '{}: an input buffer was written'.format(what)

    def numpy(self):
        return self.view.cpu().numpy().copy()


def _direct(engine, x, bn_mean, bn_std, eps=1e-6, denom=None, entry='dev', accumulate=0, prefill=None):
    """forward + backward through the C ABI; returns row_mean [N*C], row_std [N*C, or C for H*W == 1], loss2, grad_x."""
    lib = _ffi.lib()
    n, c = x.shape[:2]
    hw = x[0, 0].numel()
    rows = n * c
    denom = float(c if denom is None else denom)
    xs, ms, ss = _Guarded(engine, rows * hw, x), _Guarded(engine, c, bn_mean), _Guarded(engine, c, bn_std)
    rm, rs, l2 = _Guarded(engine, rows), _Guarded(engine, rows), _Guarded(engine, 2)
    gx = _Guarded(engine, rows * hw, prefill)
    pair = _Guarded(engine, 2, torch.tensor([W_MEAN, W_STD]))
    scratch_bytes = int(lib.dfq_bn_stat_loss_scratch_bytes(rows))
    assert scratch_bytes % 8 == 0
    scratch = _Guarded(engine, scratch_bytes // 8, dtype=torch.float64)
    _ffi.check(lib.dfq_bn_stat_loss_forward(xs.ptr(), rows, hw, c, ms.ptr(), ss.ptr(), float(eps), denom, rm.ptr(), rs.ptr(),
                                            l2.ptr(), scratch.ptr(), _ffi.stream_arg()))
    if entry == 'dev':
        _ffi.check(lib.dfq_bn_stat_loss_backward_dev(xs.ptr(), rows, hw, c, ms.ptr(), ss.ptr(), float(eps), denom, rm.ptr(),
                                                     rs.ptr(), pair.ptr(), gx.ptr(), int(accumulate), _ffi.stream_arg()))
    else:
        _ffi.check(lib.dfq_bn_stat_loss_backward(xs.ptr(), rows, hw, c, ms.ptr(), ss.ptr(), float(eps), denom, rm.ptr(), rs.ptr(),
                                                 W_MEAN, W_STD, gx.ptr(), int(accumulate), _ffi.stream_arg()))
    _ffi.synchronize()
    for name, b in (('x', xs), ('bn_mean', ms), ('bn_std', ss), ('grad_pair', pair)):
        b.check_unchanged(name)
    for name, b in (('row_mean', rm), ('row_std', rs), ('loss2', l2), ('grad_x', gx), ('scratch', scratch)):
        b.check_guards(name)
    row_std = rs.numpy()
    if hw == 1:
        assert (row_std[c:] == F32(SENTINEL)).all(), 'H*W == 1: row_std holds C entries, the rest is not written'
        row_std = row_std[:c]
    return {'row_mean': rm.numpy(), 'row_std': row_std, 'loss': l2.numpy(), 'grad': gx.numpy().reshape(x.shape)}


def _maxnorm(g, ref):
    return float(np.abs(np.asarray(g, dtype=np.float64) - ref).max() / np.abs(ref).max())


def _report(case, engine, pair):
    print('PAIR {} [{}]: engine {:.1e}, reference float32 {:.1e}'.format(case, engine.kind, *pair))


def _check(engine, x, bn_mean, bn_std, eps=1e-6, denom=None, ill=None, shift=False, ref32=True, constant_rows=None):
    """One case against the oracle.  `ill`: the name of an ill-conditioned case (gradient bound relative to the
    reference's own float32 error); `shift`: see _reference_f64; `ref32`: the float32 reference can evaluate the case;
    `constant_rows`: boolean [N, C] (or [1, C] view rows for H*W == 1) of the rows that are spatially constant."""
    xn, bmn, bsn = x.numpy(), bn_mean.numpy(), bn_std.numpy()
    ml_o, sl_o, gm_o, gs_o = orc.bn_stat_losses(xn, bmn, bsn, eps, denom)
    mean_o, std_o, _, _ = orc.bn_stat_rows(xn, eps)
    grad_o = W_MEAN * gm_o + W_STD * gs_o
    # the oracle itself, against float64 autograd of the reference's expressions (CPU only, before anything relies on it)
    ml_d, sl_d, grad_d = _reference_f64(x, bn_mean, bn_std, eps, denom, shift)
    assert abs(ml_o - ml_d) <= 1e-10 * max(1.0, abs(ml_d)) and abs(sl_o - sl_d) <= 1e-10 * max(1.0, abs(sl_d)), (ml_o, ml_d, sl_o, sl_d)
    assert _maxnorm(grad_o, grad_d) <= 1e-10, _maxnorm(grad_o, grad_d)

    got = _direct(engine, x, bn_mean, bn_std, eps, denom)
    assert_close(got['loss'][0], ml_o, 'mean loss')
    assert_close(got['loss'][1], sl_o, 'std loss')
    assert_close(got['row_mean'], mean_o.reshape(-1), 'row_mean')
    assert_close(got['row_std'], std_o.reshape(-1), 'row_std')
    if ill is None:
        np.testing.assert_allclose(got['grad'], grad_o, rtol=1e-4, atol=1e-6)
    if ref32:
        ml_r, sl_r, grad_r = _reference_f32(x, bn_mean, bn_std, eps, denom)
        if ill is None and constant_rows is None:       # as loose as tests/test_zeroq.py: the reference's float32 reductions
            assert abs(got['loss'][0] - ml_r) <= 1e-4 * max(1.0, abs(ml_r)) and abs(got['loss'][1] - sl_r) <= 1e-4 * max(1.0, abs(sl_r))
            np.testing.assert_allclose(got['grad'], grad_r, rtol=2e-3, atol=1e-5)
        if ill is not None:
            pair = (_maxnorm(got['grad'], grad_o), _maxnorm(grad_r, grad_o))
            _report(ill, engine, pair)
            assert np.isfinite(got['grad']).all()
            assert pair[0] <= max(1e-4, 2.0 * pair[1]), pair
    if constant_rows is not None:
        n, c = x.shape[:2]
        hw = x[0, 0].numel()
        assert np.isfinite(got['grad']).all(), '{} non-finite gradient elements'.format(int((~np.isfinite(got['grad'])).sum()))
        assert np.isfinite(got['row_std']).all() and (got['row_std'] >= 0).all()
        mask = np.asarray(constant_rows, dtype=bool)
        elems = (np.broadcast_to(mask.reshape(c, 1), (c, n)) if hw == 1 else np.broadcast_to(mask.reshape(n, c, 1), (n, c, hw))).reshape(x.shape)
        assert (gs_o[elems] == 0).all() and (std_o.reshape(mask.shape)[mask] == 0).all()
        np.testing.assert_allclose(got['grad'][elems], (W_MEAN * gm_o)[elems], rtol=1e-4, atol=1e-6)   # the mean term alone
    # the product path (autograd node) runs the same kernels
    xe = engine.to(x.clone()).requires_grad_(True)
    ml, sl = zeroq.bn_stat_losses(xe, engine.to(bn_mean), engine.to(bn_std), eps, denom)
    (ml * W_MEAN + sl * W_STD).backward()
    assert_bitexact(npy(xe.grad), got['grad'], 'autograd node vs C ABI')
    assert_bitexact([float(ml.detach()), float(sl.detach())], got['loss'], 'autograd node vs C ABI, losses')
    return got


def _stats(gen, c):
    return torch.randn(c, generator=gen), torch.rand(c, generator=gen) + 0.5


def _randn64(gen, shape):
    return torch.randn(*shape, generator=gen, dtype=torch.float64)


# ---- every launch shape ---------------------------------------------------------------------------------------------
# hw: the wave-per-row template (< 1024, with lanes that have no element and rows shorter / longer than a wave), the
# workgroup-per-row template (>= 1024); N*C: dead waves in the last workgroup (1, 5, 7), more rows than one pass of the
# reduce kernel's 256 threads (300), channels = 1, N = 1
SHAPES = [(1, 1, 2), (1, 5, 3), (7, 1, 63), (1, 7, 64), (5, 1, 65), (1, 1, 255), (1, 5, 255), (7, 1, 1023), (1, 7, 1024),
          (5, 1, 1025), (1, 1, 12544), (5, 1, 12544), (3, 100, 2), (300, 1, 64), (1, 300, 65), (100, 3, 1024), (2, 150, 1025)]


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_every_launch_shape(engine, shape):
    n, c, hw = shape
    g = torch.Generator().manual_seed(n * 1000003 + c * 1009 + hw)
    x = torch.randn(n, c, hw, 1, generator=g) * 1.5 + 0.3
    bn_mean, bn_std = _stats(g, c)
    _check(engine, x, bn_mean, bn_std)


# ---- spatially constant rows ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('hw', [49, 1025, 12544])
@pytest.mark.parametrize('value', [0.0, 0.37, -5.0, 1e-30, 3e4])
def test_constant_rows_get_the_mean_term_only(engine, value, hw):
    """A dead filter: channel 1 of every sample is one value.  torch's std backward masks std == 0 to a zero gradient."""
    g = torch.Generator().manual_seed(hw)
    x = torch.randn(2, 3, hw, 1, generator=g) * 1.5 + 0.3
    x[:, 1] = value
    bn_mean, bn_std = _stats(g, 3)
    const = np.zeros((2, 3), dtype=bool)
    const[:, 1] = True
    _check(engine, x, bn_mean, bn_std, shift=True, constant_rows=const)


@pytest.mark.parametrize('shape', [(2, 3, 49), (1, 5, 1025)], ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('value', [0.0, 0.37, 3e4])
def test_whole_tensor_constant(engine, value, shape):
    n, c, hw = shape
    g = torch.Generator().manual_seed(11)
    x = torch.full((n, c, hw, 1), value)
    bn_mean, bn_std = _stats(g, c)
    _check(engine, x, bn_mean, bn_std, shift=True, constant_rows=np.ones((n, c), dtype=bool))


@pytest.mark.parametrize('eps', [1e-6, 0.0])
def test_constant_rows_of_the_input_batch_term(engine, eps):
    g = torch.Generator().manual_seed(12)
    x = torch.randn(4, 3, 65, 1, generator=g)
    x[2, 0] = 0.37
    const = np.zeros((4, 3), dtype=bool)
    const[2, 0] = True
    _check(engine, x, torch.zeros(3), torch.ones(3), eps=eps, denom=4, shift=True, constant_rows=const)


# ---- ill-conditioned rows ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('hw', [49, 1025])
@pytest.mark.parametrize('base', [0.37, -5.0, 3e4])
def test_one_element_one_ulp_off(engine, base, hw):
    """Every row is one value except for a single element 1 ulp above it: the first, the last, or one in between."""
    g = torch.Generator().manual_seed(13)
    x = np.full((2, 3, hw), base, dtype=F32)
    for r in range(6):
        pos = 0 if r == 0 else hw - 1 if r == 1 else (r * 17) % hw
        x[r // 3, r % 3, pos] = np.nextafter(F32(base), F32(np.inf))
    bn_mean, bn_std = _stats(g, 3)
    _check(engine, torch.from_numpy(x.reshape(2, 3, hw, 1)), bn_mean, bn_std, shift=True, ill='1 ulp off, base {:g}, hw {}'.format(base, hw))


@pytest.mark.parametrize('hw', [(7, 7), (112, 112)], ids=['7x7', '112x112'])
@pytest.mark.parametrize('offset,spread', [(1e3, 1.0), (3e4, 0.01), (-3e4, 0.01)])
def test_large_offset_small_spread(engine, offset, spread, hw):
    """|mean| >> std: a one-pass sum of squares cancels (3e4 + 0.01 randn at 112x112: a std loss of 2.930002 against
    2.929918 in float64, 2.9e-5, before the sums were shifted)."""
    g = torch.Generator().manual_seed(14)
    x = (offset + spread * _randn64(g, (2, 3) + hw)).float()
    bn_mean, bn_std = _stats(g, 3)
    _check(engine, x, bn_mean, bn_std, ill='offset {:g} + {:g} randn, {}x{}'.format(offset, spread, *hw))


@pytest.mark.parametrize('hw', [49, 12544])
@pytest.mark.parametrize('offset,spread', [(1e3, 1.0), (3e4, 0.01), (-3e4, 0.01)])
def test_large_offset_with_matching_statistics(engine, offset, spread, hw):
    """The same rows against BN statistics of their own size (bn_mean near the offset, bn_std near the spread), so that the
    std term is not hidden behind a mean term of 2 (offset - bn_mean) / (C HW)."""
    g = torch.Generator().manual_seed(15)
    x = (offset + spread * _randn64(g, (2, 3, hw, 1))).float()
    bn_mean = (offset + spread * _randn64(g, (3,))).float()
    bn_std = (spread * (torch.rand(3, generator=g, dtype=torch.float64) + 0.5)).float()
    _check(engine, x, bn_mean, bn_std, shift=True, ill='offset {:g} + {:g} randn, matching statistics, hw {}'.format(offset, spread, hw))


# ---- the ends of the float32 range -----------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(2, 3, 63), (1, 2, 1025)], ids=lambda s: 'x'.join(map(str, s)))
def test_magnitude_1e18(engine, shape):
    """float32 squares overflow (the reference's own float32 evaluation is inf), the kernel's float64 ones do not."""
    n, c, hw = shape
    g = torch.Generator().manual_seed(16)
    x = (1e18 * _randn64(g, (n, c, hw, 1))).float()
    bn_mean, bn_std = _stats(g, c)
    got = _check(engine, x, bn_mean, bn_std, ref32=False)
    assert np.isfinite(got['loss']).all() and np.isfinite(got['grad']).all()


@pytest.mark.parametrize('eps', [0.0, 1e-6])
@pytest.mark.parametrize('shape', [(2, 3, 63), (1, 2, 1025)], ids=lambda s: 'x'.join(map(str, s)))
def test_denormal_range(engine, shape, eps):
    """Every element is a float32 denormal.  eps = 0: statistics and gradient factors stay in the denormal range (row_std
    about 1e-39; HW >= 63 keeps 2 g (std - bn_std) / (C (HW - 1) std) below the float32 maximum).  eps = 1e-6: x + eps
    rounds to eps in every element, so every row is constant after the shift."""
    n, c, hw = shape
    g = torch.Generator().manual_seed(17)
    x = torch.from_numpy((1e-39 * _randn64(g, (n, c, hw, 1))).numpy().astype(F32))
    assert float(x.abs().max()) < 1.17549435e-38 and float(x.abs().max()) > 0
    bn_mean, bn_std = _stats(g, c)
    if eps == 0.0:
        _check(engine, x, bn_mean, bn_std, eps=eps, ref32=False)
    else:
        _check(engine, x, bn_mean, bn_std, eps=eps, shift=True, ref32=False, constant_rows=np.ones((n, c), dtype=bool))


# ---- particular arguments -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('hw', [64, 1025])
def test_bn_std_equal_to_the_row_std(engine, hw):
    g = torch.Generator().manual_seed(18)
    x = torch.randn(1, 5, hw, 1, generator=g) * 1.5 + 0.3
    bn_mean = torch.randn(5, generator=g)
    bn_std = torch.from_numpy(orc.bn_stat_rows(x.numpy())[1].reshape(5).astype(F32))
    got = _check(engine, x, bn_mean, bn_std)
    assert got['loss'][1] <= 1e-12           # five terms of (float32 rounding of a std of about 1.5)^2 / 5


@pytest.mark.parametrize('shape', [(4, 3, 256), (5, 3, 1025), (2, 1, 3)], ids=lambda s: 'x'.join(map(str, s)))
def test_input_batch_term_eps_zero_denom_override(engine, shape):
    """distill_data.py:192-196: no eps, own_loss divides by the batch size."""
    n, c, hw = shape
    g = torch.Generator().manual_seed(19)
    x = torch.randn(n, c, hw, 1, generator=g)
    _check(engine, x, torch.zeros(c), torch.ones(c), eps=0.0, denom=n)


# ---- H*W == 1 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,c,constant', [(2, 4, False), (5, 4, False), (1030, 3, False), (2, 1, False), (5, 4, True), (1030, 3, True)])
def test_single_pixel_branch(engine, n, c, constant):
    """The std term over the [N, C] block viewed as [C, N]: N = 1030 sends those rows through the workgroup-per-row
    template.  `constant`: one row of that view is a single value (and gets the mean term only)."""
    g = torch.Generator().manual_seed(n + c)
    x = torch.randn(n, c, 1, 1, generator=g)
    bn_mean, bn_std = _stats(g, c)
    const = None
    if constant:
        x.view(c, n)[1] = 0.37
        const = np.zeros((1, c), dtype=bool)
        const[0, 1] = True
    _check(engine, x, bn_mean, bn_std, shift=constant, constant_rows=const)


# ---- entry points ---------------------------------------------------------------------------------------------------------
ENTRY_SHAPES = [(2, 3, 49, 1), (1, 5, 1025, 1), (5, 4, 1, 1), (1030, 3, 1, 1)]


@pytest.mark.parametrize('shape', ENTRY_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_host_scalar_backward_is_bit_identical_to_dev(engine, shape):
    g = torch.Generator().manual_seed(21)
    x = torch.randn(*shape, generator=g) * 1.5 + 0.3
    bn_mean, bn_std = _stats(g, shape[1])
    dev = _direct(engine, x, bn_mean, bn_std, entry='dev')
    host = _direct(engine, x, bn_mean, bn_std, entry='host')
    assert np.isfinite(dev['grad']).all()
    for k in dev:
        assert_bitexact(host[k], dev[k], k)


@pytest.mark.parametrize('entry', ['dev', 'host'])
@pytest.mark.parametrize('shape', ENTRY_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_accumulate_adds_into_grad_x(engine, shape, entry):
    g = torch.Generator().manual_seed(22)
    x = torch.randn(*shape, generator=g) * 1.5 + 0.3
    bn_mean, bn_std = _stats(g, shape[1])
    prefill = torch.randn(*shape, generator=g)
    plain = _direct(engine, x, bn_mean, bn_std, entry=entry, accumulate=0, prefill=prefill)['grad']
    added = _direct(engine, x, bn_mean, bn_std, entry=entry, accumulate=1, prefill=prefill)['grad']
    want = prefill.numpy() + plain              # one float32 addition per element
    if x[0, 0].numel() > 1:
        assert_bitexact(added, want, 'accumulate')
    else:
        # H*W == 1 adds the two terms in two launches: (prefill + mean term) + std term against prefill + (mean term + std
        # term), two float32 additions in another order -- at most an ulp of the largest partial sum each
        np.testing.assert_allclose(added, want, rtol=0, atol=2 * 2.0 ** -23 * float(np.abs(want).max() + np.abs(plain).max()))


# ---- isolation ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('inf', [np.inf, -np.inf])
@pytest.mark.parametrize('hw', [63, 1025])
def test_a_poisoned_row_stays_in_its_row(engine, hw, inf):
    """One NaN and one inf in row 4: its statistics and the losses may be anything, every other row is untouched."""
    g = torch.Generator().manual_seed(23)
    x = torch.randn(2, 3, hw, 1, generator=g) * 1.5 + 0.3
    bn_mean, bn_std = _stats(g, 3)
    clean = _direct(engine, x, bn_mean, bn_std)
    bad = x.clone()
    bad[1, 1, 5] = float('nan')
    bad[1, 1, hw - 2] = float(inf)
    got = _direct(engine, bad, bn_mean, bn_std)
    others = np.arange(6) != 4
    assert np.isfinite(clean['grad']).all()
    assert_bitexact(got['row_mean'][others], clean['row_mean'][others], 'row_mean')
    assert_bitexact(got['row_std'][others], clean['row_std'][others], 'row_std')
    assert_bitexact(got['grad'].reshape(6, hw)[others], clean['grad'].reshape(6, hw)[others], 'grad_x')
