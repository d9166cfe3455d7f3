"""fp64 conv oracle + per-element comparator with a derived error bound.

``tests/test_ops_gpu.py::_cmp`` accepts ``err <= atol + rtol * max|ref|`` over
the whole tensor, which for a 3x3x128 conv is an allowance of several
individual products (see ``tests/test_oracle_selftest.py``). This helper
instead bounds every output element by the rounding a correct kernel is
entitled to:

    bf16 outputs:  |got - ref| <= 2^-8 * |ref| + c * n * 2^-24 * mag
    fp32 outputs:  |got - ref| <=                c * n * 2^-24 * mag

* ``ref`` is the operation in fp64 on the bf16-quantized inputs (products of
  two bf16 values are exact in fp32 and fp64, so ``ref`` is exact to ~1e-16).
* ``mag`` is the same operation on ``|a|`` and ``|b|``: the sum of the
  magnitudes of the products that feed this output element.
* ``n`` is the number of products that really feed the element (padding and
  stride holes contribute exact zeros, which round nothing), plus the number
  of split-K slabs where a slab reduce follows.
* ``2^-8 * |ref|`` is half a bf16 ulp (8 significand bits, round to nearest
  even in ``f2bf``); ``n * 2^-24 * mag`` is the classic running-sum bound
  ``gamma_n * sum|a_i b_i|`` for fp32 with unit roundoff 2^-24, valid for any
  summation order. ``c = 2`` covers an accumulator that truncates instead of
  rounding to nearest (unit roundoff 2^-23) — the MFMA's internal summation
  rounding is not documented as nearest-even.

Calibration record (rule: if an already-validated route exceeds c = 2, set c
to the next power of two above twice the measured need, never above 16; never
calibrate on the routes under test): measured on MI355X over the routes the
existing suite validates (every geometry of ``test_conv_fwd_bwd`` and
``test_conv_shape_fuzz``, forward / dx / dW, unit-magnitude inputs), the
largest needed c — max over elements of
``(err - 2^-8|ref|) / (n * 2^-24 * mag)`` — was 0.0000 on every route
(fwd v2_bn64 / v1_bk32, dx v1_bk32 / v1_bk64, dW v2 / v1_generic): products
of 8-bit significands are exact in fp32 and these partial sums stay below
2^24 ulps of the smallest product, so the accumulation rounds (almost)
nothing and the whole error is the final bf16 rounding; fp32 dW came out
bit-equal to the rounded fp64 reference. The derived ``c = 2`` stands.

Test inputs come from ``signed_unit``: ``|v|`` in [0.5, 1] with a random sign,
so every single product is at least 0.25 — one dropped or misplaced product
is then far outside the bound — and the data is asymmetric (a transposed
C-write or swapped operand cannot pass).

Layouts are cilfw's: activations NHWC, weights (R, S, C, K).
"""

import torch
import torch.nn.functional as F
from torch.nn import grad as G

U_F32 = 2.0 ** -24        # fp32 unit roundoff (round to nearest)
HALF_ULP_BF16 = 2.0 ** -8  # relative half-ulp of bf16
C_SUM = 2.0               # see module docstring


def signed_unit(shape, gen, dtype=torch.bfloat16):
    """|v| in [0.5, 1], random sign (quantized to ``dtype``)."""
    mag = 0.5 + 0.5 * torch.rand(shape, generator=gen)
    sign = torch.randint(0, 2, shape, generator=gen).float() * 2 - 1
    return (mag * sign).to(dtype)


def _nchw(t):
    return t.detach().cpu().permute(0, 3, 1, 2).double().contiguous()


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _kcrs(w):
    return w.detach().cpu().permute(3, 2, 0, 1).double().contiguous()


def _ones(*shape):
    return torch.ones(*shape, dtype=torch.float64)


def conv_fwd_ref(x, w, stride, pad):
    """-> (ref, mag, n): fp64 NHWC y, its magnitude sum, and the per-pixel
    product count (broadcastable to y)."""
    xf, wf = _nchw(x), _kcrs(w)
    ref = F.conv2d(xf, wf, stride=stride, padding=pad)
    mag = F.conv2d(xf.abs(), wf.abs(), stride=stride, padding=pad)
    _, C, H, W = xf.shape
    R, S = wf.shape[2], wf.shape[3]
    n = F.conv2d(_ones(1, 1, H, W), _ones(1, 1, R, S), stride=stride,
                 padding=pad) * C
    return _nhwc(ref), _nhwc(mag), _nhwc(n)


def conv_dx_ref(dy, w, stride, pad, H, W):
    """-> (ref, mag, n) for dx (N, H, W, C), fp64 ``conv2d_input``."""
    dyf, wf = _nchw(dy), _kcrs(w)
    N, K, Ho, Wo = dyf.shape
    C, R, S = wf.shape[1], wf.shape[2], wf.shape[3]
    ref = G.conv2d_input((N, C, H, W), wf, dyf, stride=stride, padding=pad)
    mag = G.conv2d_input((N, C, H, W), wf.abs(), dyf.abs(), stride=stride,
                         padding=pad)
    n = G.conv2d_input((1, 1, H, W), _ones(1, 1, R, S),
                       _ones(1, 1, Ho, Wo), stride=stride, padding=pad) * K
    return _nhwc(ref), _nhwc(mag), _nhwc(n)


def conv_dw_ref(dy, x, stride, pad, R, S):
    """-> (ref, mag, n) for dW (R, S, C, K), fp64 ``conv2d_weight``."""
    dyf, xf = _nchw(dy), _nchw(x)
    N, C, H, W = xf.shape
    K, Ho, Wo = dyf.shape[1], dyf.shape[2], dyf.shape[3]
    ref = G.conv2d_weight(xf, (K, C, R, S), dyf, stride=stride, padding=pad)
    mag = G.conv2d_weight(xf.abs(), (K, C, R, S), dyf.abs(), stride=stride,
                          padding=pad)
    n = G.conv2d_weight(_ones(1, 1, H, W), (1, 1, R, S),
                        _ones(1, 1, Ho, Wo), stride=stride, padding=pad) * N

    def rsck(t):
        return t.permute(2, 3, 1, 0).contiguous()
    return rsck(ref), rsck(mag), rsck(n)


def bound(ref, mag, n, bf16_out, c=C_SUM, extra=None):
    """Per-element allowance (fp64 tensor shaped like ``ref``)."""
    b = c * U_F32 * (mag * n)
    if bf16_out:
        b = b + HALF_ULP_BF16 * ref.abs()
    if extra is not None:
        b = b + extra
    return b


def worst(got, ref, mag, n, bf16_out, c=C_SUM, extra=None):
    """-> (max err/bound, flat index of it). A non-finite output, or any
    error where the bound is zero, gives inf."""
    g = got.detach().double().cpu().reshape(ref.shape)
    b = bound(ref, mag, n, bf16_out, c, extra)
    err = (g - ref).abs()
    ratio = err / b.clamp_min(1e-300)
    ratio = torch.where((err == 0) & (b == 0), torch.zeros_like(ratio), ratio)
    ratio = torch.where(torch.isfinite(g), ratio,
                        torch.full_like(ratio, float("inf")))
    r, i = ratio.reshape(-1).max(0)
    return r.item(), i.item()


def needed_c(got, ref, mag, n, bf16_out):
    """Smallest ``c`` under which ``got`` would pass (calibration figure)."""
    g = got.detach().double().cpu().reshape(ref.shape)
    err = (g - ref).abs()
    if bf16_out:
        err = (err - HALF_ULP_BF16 * ref.abs()).clamp_min(0)
    denom = (U_F32 * (mag * n)).clamp_min(1e-300)
    return (err / denom).max().item()


def accepts(got, ref, mag, n, bf16_out, c=C_SUM, extra=None):
    return worst(got, ref, mag, n, bf16_out, c, extra)[0] <= 1.0


def check(got, ref, mag, n, bf16_out, what, c=C_SUM, extra=None):
    """Assert every element of ``got`` is within its bound; prints the worst
    err/bound first so a log shows the margin."""
    assert tuple(got.shape) == tuple(ref.shape), \
        f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    r, i = worst(got, ref, mag, n, bf16_out, c, extra)
    print(f"{what}: max err/bound = {r:.4f} (c={c})")
    if r > 1.0:
        idx = tuple(int(v) for v in torch.unravel_index(
            torch.tensor(i), ref.shape))
        g = got.detach().double().cpu().reshape(ref.shape)
        raise AssertionError(
            f"{what}: element {idx} got {g[idx].item():.9g} ref "
            f"{ref[idx].item():.9g} (err/bound {r:.3g}, c={c})")
