"""fp64 references and derived allowances for the kernels of csrc/norm.hip:
BN statistics / apply / backward, add+ReLU, DownsampleA, global average pool
and max pool (tests/test_norm_gpu.py, tests/test_norm_oracle_selftest.py).

Every reference works in fp64 on the same bf16-quantised inputs the kernel
gets. Every allowance is counted from the fp32 operations the kernel really
performs; none is fitted to a kernel's output.

Notation. ``u = 2^-24`` is the fp32 unit roundoff (one rounding to nearest).
``g(k) = k*u / (1 - k*u)`` bounds the relative error of a quantity that went
through ``k`` successive fp32 roundings, and of a sum of ``k + 1`` terms in
any order against the sum of their magnitudes (the running-sum bound the
other oracles of this project use). A bf16 store rounds to nearest even: it
moves the kernel's own fp32 value ``v`` by at most half a bf16 ulp,
``2^-8 * |v|``, and ``|v| <= |ref| + e`` where ``e`` is the fp32 allowance, so

    bf16 outputs:  tol = e + 2^-8 * (|ref| + e)
    fp32 outputs:  tol = e

A fused multiply-add only removes roundings, so the compiler's contraction of
``a * b + c`` stays inside every count below.

Batch statistics (bn_sums -> slab reduce -> bn_finalize, or the fused
bn_reduce_finalize). ``gy = ceil(M / 256)`` row blocks; ``n = M + gy``.
  mean   s/M. The M values of a channel are summed in some fixed tree: M - 1
         additions of non-zero terms (adding the zero accumulators rounds
         nothing), then one correctly rounded division by (float)M. That is
         at most M roundings <= n:   tol = g(n) * sum|x| / M.
  var    q/M - mu^2, one pass. x*x is exact in fp32 for bf16 x (16-bit
         product). E[x^2] as for the mean: g(n) * sum(x^2)/M. mu^2 carries
         the error of mu, (2|mu| + tol_mu) * tol_mu, one rounding of the
         product and one of the subtraction:
           tol = g(n)*sum(x^2)/M + (2|mu| + tol_mu)*tol_mu
                 + u*(|mu| + tol_mu)^2 + u*(E[x^2] + g(n)E[x^2] + (|mu|+tol_mu)^2)
         The fmaxf(., 0) clamp moves towards the true (non-negative) value.
         With |mean| >> std the middle term dominates: this IS the
         cancellation of the one-pass formula, allowed because the issue
         only measures it (see "offset mean" below).
  invstd rsqrtf(var + eps): the sum rounds once (u*(var + eps)), the result
         is propagated exactly through v -> v^-1/2 over [v - d, v + d]
         (lower end clamped at eps, which var_hat >= 0 guarantees), plus the
         error of rsqrtf itself. HIP's math-API table lists rsqrtf at 1 ulp
         (2^-23 relative); the ROCm documentation installed next to the
         compiler used for this project does not carry that table, so the
         figure is SUPPOSED, not looked up (RSQRT_ULPS).
  running_mean  (1 - m)*rm + m*mu with m and 1 - m the fp32 values the kernel
         forms: two products and one sum, each term sees two roundings:
           tol = m*tol_mu + g(2)*(|(1-m) rm| + m*(|mu| + tol_mu))
  running_var   unbiased = var*M/(M-1) left to right is two roundings (M - 1
         clamped to 1), then as running_mean:
           tol_unb = f*tol_var + g(2)*f*(var + tol_var),  f = M/max(M-1, 1)
           tol = m*tol_unb + g(2)*(|(1-m) rv| + m*(unb + tol_unb))

BN forward output. The kernel folds to x*sc + sh, sc = gamma*invstd,
sh = beta - mean*sc (+ res). Roundings seen by each term: |x*sc| 4 (sc, the
product, the sum, the residual sum), |mean*sc| 5 (sc, the product, the
subtraction, the two sums), |beta| 3, |res| 1, so
    e = prop + g(5) * (|x*sc| + |mean*sc| + |beta| + |res|)
    prop = |gamma| * (|x - mean|*tol_invstd + (invstd + tol_invstd)*tol_mean)
``prop`` is the propagated allowance of the kernel's own (mean, invstd):
the reference uses the fp64 statistics. ReLU is 1-Lipschitz, so the output
is compared on EVERY element under the allowance of its pre-activation. Only
the ReLU mask (y > 0, which the backward consumes) is compared away from the
band |pre| <= e, where fp32 rounding may legitimately decide the sign; the
band's share must stay below RELU_BAND_CAP.

BN backward takes the kernel's own saved (mean, invstd, y) as exact inputs.
  dbeta   sum of g (dy, ReLU-masked by y > 0):  g(n) * sum|g|
  dgamma  sum of g*(x - mean)*invstd: each term is rounded three times before
          it is summed:  g(n + 3) * sum|g*(x - mean)*invstd|
  dx      training: P*g + Q*x + R, P = gamma*invstd, A = P*(1/M),
          Q = -A*dgamma*invstd, R = A*(dgamma*invstd*mean - dbeta).
          Roundings per term: P*g 4 (P, product, two sums); Q*x 8 (A has 3:
          P, 1/M, product; Q two more; product; two sums); A*dgamma*invstd*
          mean 8 (two products, subtraction, A's 3, the product with A, the
          last sum); A*dbeta 6:
            e = prop + g(8) * (|P g| + |Q x| + |A dgamma invstd mean| + |A dbeta|)
            prop = |A invstd (x - mean)|*tol_dgamma + |A|*tol_dbeta
          (the kernel uses its own dgamma/dbeta, the reference the fp64 ones).
          |Q x| and the mean part of R cancel when |mean| >> std; both stay
          in the magnitude sum, which is what a correct kernel is entitled to.
          eval: dx = P*g, two roundings: e = g(2)*|P g|.
  dres    the masked dy, bit-equal.

add_relu forward: fl32(a + b) is exact when the exponents of a and b are
within 16 of each other (asserted on the inputs), so the only rounding is
the bf16 store: half a bf16 ulp of the fp64 sum. Backward: bit-exact.

gap_fwd: serial sum of HW values, times fl(1/HW): HW - 1 + 2 roundings, but
partial sum i only carries the first i values. For |x| in [0.5, 1] and
HW = 1 (nothing rounds) or HW >= 7 the total is within
HW * u * sum|x|/HW (sum_i |s_i| + 2|s| <= HW*sum|x| needs
sum|x| <= sum_j (j-2)|x_j|, true from HW = 7 on for such data); asserted.
gap_bwd: dy/(float)HW is one division, allowed one fp32 ulp (2^-23).

downsample_a: pure data movement, bit-exact against an index loop; extent
ceil(H/2) x ceil(W/2) (AvgPool2d(1, 2) keeps the last row / column of an odd
extent).

maxpool: explicit scan loop; the first maximum in (r, s) order wins; y and
idx exact. Backward: sum of dy over the w windows that selected the element,
w - 1 additions: e = (w - 1) * 2^-23 * sum|dy|.

Offset-mean record (x = 8 + 0.25*signed_unit, M = 293, C = 8, |mean|/std
~ 43): the derived one-pass allowance of invstd is 5.2 % of invstd there.
Measured on MI355X (tests/test_norm_gpu.py::test_bn_offset_mean): invstd
err/tol = 0.0016, largest relative error of invstd 7.6e-5 (about 640 fp32
ulps; the same kernel stays within a few ulps on zero-mean data). The
one-pass formula does lose ~9 bits here, far inside what the derivation
allows; OFFSET_MEAN_RECORD keeps the figures.
"""

import numpy as np
import torch

import _oracle as O

U = O.U_F32
HB = O.HALF_ULP_BF16
ULP32 = 2.0 ** -23
RSQRT_ULPS = 1            # supposed: see module docstring
ROWS_PER_BLK = 256        # BN_ROWS_PER_BLK of csrc/norm.hip
WAVE = 64
RELU_BAND_CAP = 0.01
MOMENTUM, EPS = 0.1, 1e-5

# offset-mean case measured on MI355X (a record, not a bound: nothing asserts
# against it)
OFFSET_MEAN_RECORD = dict(invstd_err_over_tol=0.001605,
                          invstd_max_rel_err=7.632e-05,
                          invstd_tol_over_value=5.171e-02)

BN_SHAPES = [(1, 8), (293, 8), (293, 72), (293, 136), (293, 520), (16643, 8)]
BN_MODES = ["plain", "relu", "res_relu"]
BN_EVAL_SHAPE = (147, 72)
SLAB_CONST = 4.0          # added to the rows of slab 64 onward at M = 16643
ADD_RELU_TOTALS = [8, 2048 * 3 + 8]
ADD_RELU_MIXED = 2048 + 5
GAP_SHAPES = [(3, 49, 264), (2, 64, 64), (1, 1, 8)]       # (N, HW, C)
DS_SHAPES = [(2, 8, 8, 16), (2, 15, 15, 8), (1, 7, 9, 24), (1, 1, 1, 8)]
# (N, H, W, C, kernel, stride, pad)
POOL_CASES = [(2, 7, 9, 8, 3, 2, 1), (1, 16, 16, 64, 3, 2, 1),
              (1, 8, 8, 16, 2, 2, 0), (2, 7, 9, 12, 3, 2, 1)]
POOL_VALUES = (0.0, 0.5, 1.0, -0.5, 1.5)


def g(k):
    return k * U / (1.0 - k * U)


def gy_of(M):
    return -(-M // ROWS_PER_BLK)


def f32(v):
    """The fp32 value of a Python float, as a Python float."""
    return float(np.float32(v))


# ------------------------------------------------------------------ comparing

def worst(got, ref, tol):
    """max err/tol. inf for a shape mismatch, a non-finite output, or any
    error where the allowance is zero (the exact comparisons pass tol = 0)."""
    if tuple(got.shape) != tuple(ref.shape):
        return float("inf")
    gd = got.detach().double().cpu()
    ref = ref.double()
    tol = torch.as_tensor(tol, dtype=torch.float64).expand_as(ref)
    err = (gd - ref).abs()
    ratio = err / tol.clamp_min(1e-300)
    ratio = torch.where(tol == 0, torch.where(
        err == 0, torch.zeros_like(ratio),
        torch.full_like(ratio, float("inf"))), ratio)
    ratio = torch.where(torch.isfinite(gd), ratio,
                        torch.full_like(ratio, float("inf")))
    return ratio.max().item() if ratio.numel() else 0.0


def check(got, ref, tol, what):
    r = worst(got, ref, tol)
    print(f"{what}: max err/tol = {r:.4f}")
    assert r <= 1.0, f"{what}: err/tol {r:.3g}"
    return r


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def check_bits(got, ref, what):
    assert tuple(got.shape) == tuple(ref.shape), \
        f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    assert got.dtype == ref.dtype, f"{what}: {got.dtype} vs {ref.dtype}"
    bad = (bits(got) != bits(ref)).sum().item()
    print(f"{what}: max err/tol = {0.0 if bad == 0 else float('inf')} "
          f"(bit-exact, {bad} differ)")
    assert bad == 0, f"{what}: {bad} elements differ"


def bf16_tol(ref, e):
    return e + HB * (ref.abs() + e)


# ------------------------------------------------------------------------- BN

def bn_inputs(M, C, offset_mean=False):
    """-> dict of CPU tensors: x, res, dy (M, 1, 1, C) bf16; gamma, beta,
    rm0, rv0 fp32. At M > 64 slabs the rows from slab 64 onward carry
    SLAB_CONST, so a reduce that stops after 64 slabs moves the mean."""
    gen = torch.Generator().manual_seed(7000 + 13 * M + C + (5 if offset_mean
                                                            else 0))
    shape = (M, 1, 1, C)
    if offset_mean:
        x = (8.0 + 0.25 * O.signed_unit(shape, gen).float()).bfloat16()
    else:
        x = O.signed_unit(shape, gen).float()
        if M > WAVE * ROWS_PER_BLK:
            x[WAVE * ROWS_PER_BLK:] += SLAB_CONST
        x = x.bfloat16()
    return dict(
        x=x, res=O.signed_unit(shape, gen), dy=O.signed_unit(shape, gen),
        gamma=(torch.rand(C, generator=gen) + 0.5),
        beta=O.signed_unit((C,), gen, torch.float32),
        rm0=O.signed_unit((C,), gen, torch.float32) * 0.3,
        rv0=torch.rand(C, generator=gen) + 0.5)


def _invstd(var, tol_var, eps32):
    v = var + eps32
    d = tol_var + U * (v + tol_var)
    lo = (v - d).clamp_min(eps32)
    hi = v + d
    inv = v.rsqrt()
    tol = torch.maximum(lo.rsqrt() - inv, inv - hi.rsqrt()) \
        + RSQRT_ULPS * ULP32 * lo.rsqrt()
    return inv, tol


def bn_stats_ref(x, rm0, rv0, momentum=MOMENTUM, eps=EPS, rows=None):
    """Training statistics -> {name: (ref, tol)} for mean, var, invstd,
    running_mean, running_var. ``rows`` restricts the reduction (fault
    seeding only); the allowances always belong to the full reduction."""
    C = x.shape[-1]
    x64 = x.double().reshape(-1, C)
    M = x64.shape[0]
    n = M + gy_of(M)
    xs = x64 if rows is None else x64[rows]
    mean = xs.sum(0) / M
    ex2 = (xs * xs).sum(0) / M
    var = ((x64 - mean) ** 2).mean(0) if rows is None else ex2 - mean * mean
    amean = x64.abs().mean(0)
    ex2_full = (x64 * x64).mean(0)
    t_mu = g(n) * amean
    t_q = g(n) * ex2_full
    mu_hi = mean.abs() + t_mu
    t_var = t_q + (2 * mean.abs() + t_mu) * t_mu + U * mu_hi ** 2 \
        + U * (ex2_full + t_q + mu_hi ** 2)
    eps32 = f32(eps)
    inv, t_inv = _invstd(var, t_var, eps32)
    m32 = f32(momentum)
    c1 = float(np.float32(1.0) - np.float32(momentum))
    a = c1 * rm0.double()
    rm = a + m32 * mean
    t_rm = m32 * t_mu + g(2) * (a.abs() + m32 * mu_hi)
    f = M / max(M - 1, 1)
    unb = var * f
    t_unb = f * t_var + g(2) * f * (var + t_var)
    a = c1 * rv0.double()
    rv = a + m32 * unb
    t_rv = m32 * t_unb + g(2) * (a.abs() + m32 * (unb + t_unb))
    return dict(mean=(mean, t_mu), var=(var, t_var), invstd=(inv, t_inv),
                running_mean=(rm, t_rm), running_var=(rv, t_rv))


def bn_eval_stats_ref(rm, rv, eps=EPS):
    """Eval mode: mean = running_mean exactly, invstd = rsqrtf(rv + eps)."""
    mean = rm.double()
    inv, t_inv = _invstd(rv.double(), torch.zeros_like(mean), f32(eps))
    return dict(mean=(mean, torch.zeros_like(mean)), invstd=(inv, t_inv))


def bn_y_ref(x, gamma, beta, stats, res=None, relu=False):
    """-> (ref, tol, pre, band): the bf16 output's reference and allowance,
    the fp64 pre-activation and the mask of elements whose ReLU decision is
    within the fp32 allowance of zero."""
    C = x.shape[-1]
    x64 = x.double().reshape(-1, C)
    (mean, t_mu), (inv, t_inv) = stats["mean"], stats["invstd"]
    ga, be = gamma.double(), beta.double()
    pre = (x64 - mean) * inv * ga + be
    prop = ga.abs() * ((x64 - mean).abs() * t_inv + (inv + t_inv) * t_mu)
    mag = (x64.abs() + mean.abs() + t_mu) * ga.abs() * (inv + t_inv) \
        + be.abs()
    if res is not None:
        r64 = res.double().reshape(-1, C)
        pre = pre + r64
        mag = mag + r64.abs()
    e = prop + g(5) * mag
    ref = pre.clamp_min(0) if relu else pre
    band = (pre.abs() <= e) if relu else torch.zeros_like(pre, dtype=bool)
    return ref, bf16_tol(ref, e), pre, band


def check_relu_mask(y, pre, band, what):
    """y > 0 exactly where the fp64 pre-activation is positive, outside the
    band; the band's share is capped."""
    share = band.double().mean().item()
    print(f"{what}: ReLU band share = {share:.5f}")
    assert share < RELU_BAND_CAP, f"{what}: band share {share:.4f}"
    got = y.detach().cpu().double().reshape(pre.shape) > 0
    bad = ((got != (pre > 0)) & ~band).sum().item()
    assert bad == 0, f"{what}: {bad} ReLU decisions differ outside the band"


def bn_bwd_ref(dy, x, gamma, mean_k, invstd_k, y_k, relu, training,
               mask=True, with_q=True, with_dbeta=True):
    """(mean_k, invstd_k, y_k) are the kernel's own saved tensors, taken as
    exact. -> dict: dgamma, dbeta, dx as (ref, tol); dres as the bf16 tensor
    the kernel must reproduce bit for bit. ``mask`` / ``with_q`` /
    ``with_dbeta`` seed faults."""
    C = x.shape[-1]
    x64 = x.double().reshape(-1, C)
    M = x64.shape[0]
    n = M + gy_of(M)
    mu = mean_k.detach().double().cpu()
    inv = invstd_k.detach().double().cpu()
    ga = gamma.double()
    dyc = dy.detach().cpu().reshape(-1, C)
    keep = (y_k.detach().cpu().double().reshape(-1, C) > 0) if relu \
        else torch.ones_like(x64, dtype=bool)
    gm = dyc.double() * keep
    d = x64 - mu
    t = (gm if mask else dyc.double()) * d * inv
    dgamma = t.sum(0)
    t_dg = g(n + 3) * (gm * d * inv).abs().sum(0)
    dbeta = gm.sum(0)
    t_db = g(n) * gm.abs().sum(0)
    P = ga * inv
    T1 = P * gm
    if training:
        A = P / M
        T2 = A * dgamma * inv * x64
        T3 = A * dgamma * inv * mu
        T4 = A * dbeta
        ref = T1.clone()
        if with_q:
            ref = ref - T2
        ref = ref + T3
        if with_dbeta:
            ref = ref - T4
        dg_hi, db_hi = dgamma.abs() + t_dg, dbeta.abs() + t_db
        prop = (A * inv * d).abs() * t_dg + A.abs() * t_db
        e = prop + g(8) * (T1.abs() + (A * inv).abs() * dg_hi
                           * (x64.abs() + mu.abs()) + A.abs() * db_hi)
    else:
        ref = T1
        e = g(2) * T1.abs()
    dres = torch.where(keep, dyc, torch.zeros_like(dyc))
    return dict(dgamma=(dgamma, t_dg), dbeta=(dbeta, t_db),
                dx=(ref, bf16_tol(ref, e)), dres=dres)


# ------------------------------------------------------------------- add_relu

def add_relu_inputs(total, mixed=False):
    """(a, b, dy), shape (1, 1, 1, total). ``mixed``: values from a small
    set so that a + b hits exact zeros and both signs."""
    gen = torch.Generator().manual_seed(8100 + total)
    shape = (1, 1, 1, total)
    if mixed:
        vals = torch.tensor([-1.0, -0.5, 0.5, 1.0, 0.75, -0.75])
        a = vals[torch.randint(0, 6, shape, generator=gen)].bfloat16()
        b = vals[torch.randint(0, 6, shape, generator=gen)].bfloat16()
    else:
        a, b = O.signed_unit(shape, gen), O.signed_unit(shape, gen)
    return a, b, O.signed_unit(shape, gen)


def add_relu_ref(a, b, dy):
    """-> (y_ref, y_tol, da): da is the bf16 tensor add_relu_bwd must give
    bit for bit when handed the correctly rounded y."""
    s = a.double() + b.double()
    assert torch.equal(s.float().double(), s), "a + b must be exact in fp32"
    ref = s.clamp_min(0)
    da = torch.where(ref.to(torch.bfloat16) > 0, dy, torch.zeros_like(dy))
    return ref, HB * ref.abs(), da


# ------------------------------------------------------------------------ gap

def gap_inputs(N, HW, C):
    gen = torch.Generator().manual_seed(8200 + HW + C)
    H = {49: 7, 64: 8, 1: 1}[HW]
    return (O.signed_unit((N, H, HW // H, C), gen),
            O.signed_unit((N, C), gen))


def gap_ref(x, dy):
    """-> (y_ref, y_tol, dx_ref, dx_tol)."""
    N, H, W, C = x.shape
    HW = H * W
    x64 = x.double().reshape(N, HW, C)
    assert HW == 1 or HW >= 7
    assert (x64.abs() >= 0.5).all() and (x64.abs() <= 1).all()
    ref = x64.mean(1)
    e = HW * U * x64.abs().mean(1)
    dref = (dy.double() / HW).reshape(N, 1, 1, C).expand(N, H, W, C)
    return ref, bf16_tol(ref, e), dref, bf16_tol(dref, ULP32 * dref.abs())


# ---------------------------------------------------------------- DownsampleA

def ds_inputs(N, H, W, C):
    gen = torch.Generator().manual_seed(8300 + H * 31 + W)
    Ho, Wo = -(-H // 2), -(-W // 2)
    return (O.signed_unit((N, H, W, C), gen),
            O.signed_unit((N, Ho, Wo, 2 * C), gen))


def ds_ref(x, dy, origin=0, floor=False):
    """Plain index loops -> (y, dx), bf16, to be matched bit for bit.
    ``origin`` / ``floor`` seed faults."""
    N, H, W, C = x.shape
    Ho, Wo = (H // 2, W // 2) if floor else (-(-H // 2), -(-W // 2))
    y = torch.zeros(N, Ho, Wo, 2 * C, dtype=x.dtype)
    dx = torch.zeros(N, H, W, C, dtype=x.dtype)
    for ho in range(Ho):
        for wo in range(Wo):
            h, w = 2 * ho + origin, 2 * wo + origin
            if h < H and w < W:
                y[:, ho, wo, :C] = x[:, h, w, :]
                if ho < dy.shape[1] and wo < dy.shape[2]:
                    dx[:, h, w, :] = dy[:, ho, wo, :C]
    return y, dx


# -------------------------------------------------------------------- maxpool

def pool_inputs(N, H, W, C, k, st, pad):
    """x from the five-value set POOL_VALUES (zero included): the nine taps
    of a 3x3 window cannot all differ."""
    gen = torch.Generator().manual_seed(8400 + H * 17 + C + k)
    vals = torch.tensor(POOL_VALUES)
    x = vals[torch.randint(0, len(POOL_VALUES), (N, H, W, C),
                           generator=gen)].bfloat16()
    Ho = (H + 2 * pad - k) // st + 1
    Wo = (W + 2 * pad - k) // st + 1
    return x, O.signed_unit((N, Ho, Wo, C), gen)


def pool_ref(x, dy, k, st, pad, last_wins=False, credit_all=False):
    """Explicit scan -> (y bf16, idx int32, dx_ref, dx_tol). The first
    maximum in (r, s) order wins. ``last_wins`` / ``credit_all`` seed
    faults."""
    N, H, W, C = x.shape
    Ho = (H + 2 * pad - k) // st + 1
    Wo = (W + 2 * pad - k) // st + 1
    x64 = x.double()
    best = torch.full((N, Ho, Wo, C), -float("inf"), dtype=torch.float64)
    idx = torch.zeros(N, Ho, Wo, C, dtype=torch.int32)
    for ho in range(Ho):
        for wo in range(Wo):
            for r in range(k):
                hi = ho * st - pad + r
                if hi < 0 or hi >= H:
                    continue
                for s in range(k):
                    wi = wo * st - pad + s
                    if wi < 0 or wi >= W:
                        continue
                    v = x64[:, hi, wi, :]
                    cur = best[:, ho, wo, :]
                    take = (v >= cur) if last_wins else (v > cur)
                    best[:, ho, wo, :] = torch.where(take, v, cur)
                    idx[:, ho, wo, :] = torch.where(
                        take, torch.full_like(idx[:, ho, wo, :], hi * W + wi),
                        idx[:, ho, wo, :])
    y = best.to(torch.bfloat16)
    dy64 = dy.double()
    dx = torch.zeros(N, H, W, C, dtype=torch.float64)
    mag = torch.zeros_like(dx)
    cnt = torch.zeros_like(dx)
    for ho in range(Ho):
        for wo in range(Wo):
            for r in range(k):
                hi = ho * st - pad + r
                if hi < 0 or hi >= H:
                    continue
                for s in range(k):
                    wi = wo * st - pad + s
                    if wi < 0 or wi >= W:
                        continue
                    if credit_all:
                        sel = x64[:, hi, wi, :] == best[:, ho, wo, :]
                    else:
                        sel = idx[:, ho, wo, :] == hi * W + wi
                    sel = sel.double()
                    dx[:, hi, wi, :] += sel * dy64[:, ho, wo, :]
                    mag[:, hi, wi, :] += sel * dy64[:, ho, wo, :].abs()
                    cnt[:, hi, wi, :] += sel
    e = (cnt - 1).clamp_min(0) * ULP32 * mag
    return y, idx, dx, bf16_tol(dx, e)
