"""fp64 references and per-element allowances for the classifier head and the
losses: the three ``gemm_kernel`` modes of csrc/gemm.hip, ``wa_loss_*``,
``ce_*``, ``kd_*``, ``loss_mean*`` and ``topk_kernel`` of csrc/loss.hip.
Shared by test_head_oracle_selftest.py (CPU) and test_head_gpu.py.

Linear
------
``x (M,K)``, ``w (N,K)``, ``bias (N)``, ``dy (M,N)``: bf16 values from
``_oracle.signed_unit`` (|v| in [0.5, 1], random sign), so one dropped or
misplaced product is at least 0.25. References in fp64 on those values:
``y = x w^T + b``, ``dx = dy w``, ``dW = dy^T x``, ``db = dy.sum(0)``; ``mag``
is the same operation on absolute values. Allowance ``_oracle.bound`` with
``c = C_SUM``: ``n`` = reduction length + the split factor that launch uses
(one more fp32 add per slab in the reduce), ``bf16_out`` for ``y`` and ``dx``,
fp32 for ``dW`` and ``db`` (``n = M``, ``mag = |dy|.sum(0)``). The bias is one
more fp32 add: ``extra = 2 * 2^-24 * (mag + |b|)``.

Losses
------
``log_softmax`` in fp64 on the bf16 (WA) or fp32 (CE, KD) inputs;
``total = [ce] CE + lam KD`` with CE = label-smoothed cross entropy over all
``C`` columns and KD = ``T^2/M sum pt (log pt - log ps)`` over the first
``Ck``. The gradient reference is what fp64 autograd gives for ``total * up``.

Per-element allowance for dlogits, with ``p``, ``ps``, ``pt`` the fp64
softmaxes, ``u = 2^-24``, columns >= Ck taking only the CE terms::

    rel_s = 2 eps + 4 u (|s| + max_row|s|) + C u
    rel_t = 2 eps + 4 u (|t| + max_row|t|) / T + Ck u
    err   = p rel_s + [c < Ck] lam T (ps rel_s + pt rel_t)
    mag   = p + smooth/C + onehot (1 - smooth) + [c < Ck] lam T (ps + pt)
    allow = |up| / M * (err + 4 u mag)   (+ 2^-8 |ref| for bf16 dlogits)

* ``eps = 2^-21`` for ``__expf`` / ``__logf`` is derived, not measured: a
  hardware transcendental good to 1 ulp (2^-23), one fp32 scaling multiply
  (the base-2 conversion), doubled as ``C_SUM`` doubles the unit roundoff.
  ``2 eps`` because a softmax entry is ``exp(s - lse)`` with ``lse`` itself
  from one ``exp`` sum and one ``log``.
* ``4 u (|s| + max_row|s|)``: ``exp`` amplifies the absolute rounding error of
  its argument ``s - lse`` (``|lse| <= max|s| + log C``; the subtraction, the
  ``lse = log(se) + mx`` add and, for KD, the division by ``T`` each round
  once) into a relative error of the result.
* ``C u`` is the running sum of ``C`` non-negative terms in ``se``.
* ``4 u mag``: the few fp32 operations that combine the terms (subtract
  ``smooth/C`` and the one-hot, ``lam*T*(ps-pt)``, ``* up``, ``/ M``), each
  relative to the magnitudes that enter.
* ``2^-8 |ref|``: half a bf16 ulp of the result (``wa_loss`` only).
* underflow, a term the issue's formula lacks and that the relative
  allowances above cannot express (observed: without it the project's fp32
  CPU path came out at 253 times the bound at (37, 300, 257), scale 30,
  smooth 0, on an element whose reference is 1.4e-41 and which fp32 returns
  as 0; the term was added before the first GPU run, so no GPU figure
  without it exists): fp32 and
  bf16 share the exponent range, and a result below the smallest normal
  number 2^-126 may be flushed to zero (at logit scale 30 the far tail of a
  softmax is ~1e-40). Each softmax that enters (``p``; ``ps`` and ``pt``
  weighted ``lam T``) may lose up to 2^-126 before the ``|up|/M`` scaling and
  the result once more after it: ``+ 2^-126 (1 + |up|/M (1 + 2 lam T))``.
  The smallest seeded fault is > 1e-9, thirty orders of magnitude above it.

Scalar losses (``total``, ``ce``, ``kd``)::

    allow = (M + C + 8) u * sum_rows|row terms| / M + 2 eps (mean|lse| + 1)

``|row terms|`` of CE is ``(1-smooth)(|lse| + |s_y|) + smooth (mean|s| +
|lse|)``, of KD ``T^2 sum pt (|log pt| + |log ps|)`` (and ``lse`` there are
the two log-sum-exps of ``s/T`` and ``t/T``); ``M + C + 8`` counts the adds of
the column sum, the row mean (``loss_mean*``) and the handful of scalar
operations; ``total`` gets ``[ce] allow_ce + lam allow_kd``.

Top-k is exact: rank of the target = number of columns with a larger value,
plus columns with an equal value and a lower index; ``counts[k-1]`` = rows
with rank < k, compared as integers.

Calibration record
------------------
No constant was calibrated: ``eps`` stands at its derived 2^-21 and ``c`` at
``C_SUM``. Largest ``max err/bound`` printed per family (every smooth /
upstream / bias combination of the shapes above):

CPU, the project's fp32 path with bf16 dlogits (test_head_oracle_selftest):
wa_loss dlogits 0.9939 at (37, 300, 257) (0.9852 / 0.9939 / 0.9846 at scales
1 / 8 / 30), scalars <= 0.0182; ce dlogits 0.5597, kd dlogits 0.2159,
their losses <= 0.0044; linear 0.9958 (dx of (5,3,2057), the bf16 rounding).

MI355X (test_head_gpu.py):

* linear y: 0.9714 (70,67,40), 0.2963 (1,1,33), 0.7762 (37,13,520; split 4),
  0.9688 (37,300,72), 0.9624 (300,13,72), 0.2285 (5,3,2057; split 16),
  0.0458 (3,5,8200; split 32). dx: 0.9749, 0.8448, 0.9907, 0.8829 (split 2),
  0.9893, 0.9958, 0.9955. dW and db: 0.0000 everywhere, split 2 included -
  sums of products of 8-bit significands stay exact in fp32 at these
  lengths, as ``_oracle`` found for the convs; y and dx are the final bf16
  rounding alone.
* wa_loss dlogits / total / ce / kd: (37,300,257) 0.9939 / 0.0025 / 0.0014 /
  0.0026; (300,10,0) 0.9934 / 0.0029 / 0.0029 / 0; (5,64,64) 0.9734 /
  0.0331 / 0.0109 / 0.0627 (scale 30); (1,2,1) 0.8436 / 0.0118 / 0.0182 / 0.
  The bf16 half-ulp dominates dlogits; at scales 1 and 8 the figures equal
  the CPU path's to four digits.
* cross_entropy (fp32 dlogits / loss): 0.5210 / 0.0026 at (37,300), 0.5128 /
  0.0033 at (300,10), 0 / 0 at (1,1).
* kd_loss (fp32 dlogits / loss): 0.2130 / 0.0045 at (37,300), 0.3585 /
  0.0029 at (300,10), 0 / 0 at (1,1).
* top-k: counts equal as integers in every case; the expected counts are
  [8, 15, 18, 25, 27] of 33 at C = 1000, [1, 3, 3, 5, 5] of 7 at C = 257,
  [2, 3, 3, 5, 6, 7, 7, 9] of 9 at C = 300 / maxk = 8, [2, 3, 4, 5, 5],
  [2, 3, 4] and [1] in the small cases.
"""

import torch

from _oracle import (U_F32, HALF_ULP_BF16, C_SUM, signed_unit, bound, worst,
                     check)

EPS_TRANS = 2.0 ** -21   # __expf / __logf, see module docstring (cap 2^-19)
F32_MIN_NORMAL = 2.0 ** -126   # below it fp32 / bf16 results may flush to 0

# (M, N, K) -> (fwd, dx, dW) split factors cilfw_linear_ksplit gives; each the
# smallest shape that reaches its code
LINEAR_SHAPES = [
    ((70, 67, 40), (1, 1, 1)),     # two blocks each way, ragged M, N and K
    ((1, 1, 33), (1, 1, 1)),       # degenerate, odd K
    ((37, 13, 520), (4, 1, 1)),    # ragged last K-slice (17 steps over 4)
    ((37, 300, 72), (1, 2, 1)),    # dx split-K, reduce_slabs_bf16
    ((300, 13, 72), (1, 1, 2)),    # dW split-K, reduce_slabs_f32
    ((5, 3, 2057), (16, 1, 1)),    # rn50 feature width + 9
    ((3, 5, 8200), (32, 1, 1)),    # the cap
]
LINEAR_IDS = ["x".join(map(str, s)) for s, _ in LINEAR_SHAPES]

# (M, C, Ck) of the WA loss; (M, C) of CE / KD
WA_SHAPES = [(37, 300, 257),   # strided loops run twice
             (300, 10, 0),     # t_logits=None, loss_mean3 strided
             (5, 64, 64),      # Ck = C
             (1, 2, 1)]
WA_IDS = ["x".join(map(str, s)) for s in WA_SHAPES]
CE_SHAPES = [(37, 300), (300, 10), (1, 1)]
SCALES = [1, 8, 30]
T_KD, LAM = 2.0, 0.5

# (M, C, maxk) of the top-k cases
TOPK_CASES = [(33, 1000, 5), (7, 257, 5), (5, 5, 5), (4, 3, 3), (1, 100, 1),
              (9, 300, 8)]


# --------------------------------------------------------------------- linear

def linear_inputs(M, N, K, seed=0):
    """-> x (M,K) bf16, w (N,K) bf16, bias (N) fp32 (bf16-valued), dy (M,N)
    bf16, all from signed_unit."""
    g = torch.Generator().manual_seed(104729 + 31 * M + 7 * N + K + seed)
    x = signed_unit((M, K), g)
    w = signed_unit((N, K), g)
    b = signed_unit((N,), g).float()
    dy = signed_unit((M, N), g)
    return x, w, b, dy


def linear_ref(x, w, b, dy, splits):
    """-> {name: (ref, mag, n, bf16_out, extra)} for y, dx, dw, db. ``b`` may
    be None (then no db entry and no bias term)."""
    x64, w64, dy64 = (t.detach().cpu().double() for t in (x, w, dy))
    M, K = x64.shape
    N = w64.shape[0]
    ks_f, ks_dx, ks_dw = splits
    out = {}
    ref, mag = x64 @ w64.t(), x64.abs() @ w64.abs().t()
    extra = None
    if b is not None:
        b64 = b.detach().cpu().double()
        ref = ref + b64
        extra = 2 * U_F32 * (mag + b64.abs())
    out["y"] = (ref, mag, float(K + ks_f), True, extra)
    out["dx"] = (dy64 @ w64, dy64.abs() @ w64.abs(), float(N + ks_dx), True,
                 None)
    out["dw"] = (dy64.t() @ x64, dy64.abs().t() @ x64.abs(),
                 float(M + ks_dw), False, None)
    if b is not None:
        out["db"] = (dy64.sum(0), dy64.abs().sum(0), float(M), False, None)
    return out


def linear_worst(got, entry):
    ref, mag, n, bf16_out, extra = entry
    assert tuple(got.shape) == tuple(ref.shape), \
        f"shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    return worst(got, ref, mag, n, bf16_out, C_SUM, extra)[0]


def linear_check(got, entry, what):
    ref, mag, n, bf16_out, extra = entry
    check(got, ref, mag, n, bf16_out, what, C_SUM, extra)


# --------------------------------------------------------------------- losses

def forced_targets(M, C, Ck, gen):
    """Random targets with the first rows forced onto columns 0, Ck-1, Ck and
    C-1 (those that exist), the last row first when M is short."""
    y = torch.randint(0, C, (M,), generator=gen)
    cols = [c for c in (C - 1, Ck, Ck - 1, 0) if 0 <= c < C]
    for i, c in enumerate(cols[:M]):
        y[i] = c
    return y


def loss_inputs(M, C, Ck, scale, dtype, seed=0):
    """-> s (M,C), t (M,Ck) or None, targets; ``dtype`` values, randn*scale."""
    g = torch.Generator().manual_seed(7907 + 13 * M + 5 * C + Ck + 101 * scale
                                      + seed)
    s = (torch.randn(M, C, generator=g) * scale).to(dtype)
    t = (torch.randn(M, Ck, generator=g) * scale).to(dtype) if Ck > 0 else None
    return s, t, forced_targets(M, C, Ck, g)


def loss_ref(s, t, targets, smooth, T, lam, up=1.0, ce=True, bf16_grad=True):
    """fp64 reference and allowances -> dict(total, ce, kd, allow_total,
    allow_ce, allow_kd (floats), grad, grad_allow (M,C) fp64).
    ``ce=False``: the KD term alone (``kd_loss``)."""
    s64 = s.detach().cpu().double().requires_grad_(True)
    M, C = s64.shape
    Ck = 0 if t is None else t.shape[1]
    y = targets.detach().cpu().view(-1, 1)
    u, eps = U_F32, EPS_TRANS
    n_s = float(M + C + 8)

    lse = torch.logsumexp(s64, 1, keepdim=True)
    logp = s64 - lse
    ce_row = (1 - smooth) * (-logp.gather(1, y)) \
        - smooth * logp.mean(1, keepdim=True)
    ce_val = ce_row.sum() / M
    sd = s64.detach()
    ce_mag = (1 - smooth) * (lse.detach().abs() + sd.gather(1, y).abs()) \
        + smooth * (sd.abs().mean(1, keepdim=True) + lse.detach().abs())
    allow_ce = n_s * u * ce_mag.sum().item() / M \
        + 2 * eps * (lse.detach().abs().mean().item() + 1)

    if Ck > 0:
        t64 = t.detach().cpu().double()
        sk, tk = s64[:, :Ck] / T, t64 / T
        lse_s = torch.logsumexp(sk, 1, keepdim=True)
        lse_t = torch.logsumexp(tk, 1, keepdim=True)
        logps, logpt = sk - lse_s, tk - lse_t
        pt = logpt.exp()
        kd_val = (pt * (logpt - logps)).sum() * (T * T) / M
        kd_mag = (T * T) * (pt * (logpt.abs() + logps.detach().abs())).sum(
            1, keepdim=True)
        allow_kd = n_s * u * kd_mag.sum().item() / M + 2 * eps * (
            (lse_s.detach().abs() + lse_t.abs()).mean().item() + 1)
    else:
        kd_val = torch.zeros((), dtype=torch.float64)
        allow_kd = 2 * eps
    total = (ce_val if ce else 0.0) + lam * kd_val
    allow_total = (allow_ce if ce else 0.0) + lam * allow_kd
    (total * up).backward()
    grad = s64.grad

    p = logp.detach().exp()
    rel_s = 2 * eps + 4 * u * (sd.abs() + sd.abs().amax(1, keepdim=True)) \
        + C * u
    onehot = torch.zeros_like(p).scatter_(1, y, 1.0)
    err = torch.zeros_like(p)
    mag = torch.zeros_like(p)
    if ce:
        err += p * rel_s
        mag += p + smooth / C + onehot * (1 - smooth)
    if Ck > 0:
        ps = logps.detach().exp()
        rel_t = 2 * eps + 4 * u * (t64.abs()
                                   + t64.abs().amax(1, keepdim=True)) / T \
            + Ck * u
        err[:, :Ck] += lam * T * (ps * rel_s[:, :Ck] + pt * rel_t)
        mag[:, :Ck] += lam * T * (ps + pt)
    flush = (1.0 if ce else 0.0) + (2 * lam * T if Ck > 0 else 0.0)
    allow = abs(up) / M * (err + 4 * u * mag + F32_MIN_NORMAL * flush) \
        + F32_MIN_NORMAL
    if bf16_grad:
        allow = allow + HALF_ULP_BF16 * grad.abs()
    return dict(total=total.detach().item(), ce=ce_val.detach().item(),
                kd=kd_val.detach().item(),
                allow_total=allow_total, allow_ce=allow_ce,
                allow_kd=allow_kd, grad=grad, grad_allow=allow)


def _ratio(got, ref, allow):
    """max |got - ref| / allow through ``_oracle.worst`` (inf for a
    non-finite output or an error where the allowance is zero): with
    ``mag = allow`` and ``n = 1 / (C_SUM * U_F32)``, a power of two, its bound
    ``C_SUM * U_F32 * mag * n`` is ``allow`` exactly."""
    return worst(got, ref, allow, 1.0 / (C_SUM * U_F32), False)[0]


def grad_worst(got, ref):
    """max err/allowance over every dlogits element."""
    assert tuple(got.shape) == tuple(ref["grad"].shape), \
        f"dlogits shape {tuple(got.shape)} vs {tuple(ref['grad'].shape)}"
    return _ratio(got, ref["grad"], ref["grad_allow"])


def scalar_worst(got, ref, which):
    """err/allowance of one scalar loss, ``which`` in total / ce / kd."""
    r = torch.tensor([ref[which]], dtype=torch.float64)
    a = torch.tensor([ref["allow_" + which]], dtype=torch.float64)
    return _ratio(got.reshape(1), r, a)


def loss_check(scalars, grad, ref, what):
    """Assert the scalar losses (dict which -> 0-d tensor) and dlogits are
    within their allowances; prints every err/bound first."""
    rs = {k: scalar_worst(v, ref, k) for k, v in scalars.items()}
    rg = grad_worst(grad, ref)
    print(f"{what}: max err/bound = {rg:.4f} (dlogits) "
          + " ".join(f"{r:.4f} ({k})" for k, r in rs.items()))
    for k, r in rs.items():
        assert r <= 1.0, \
            f"{what}: {k} got {scalars[k].item():.9g} ref {ref[k]:.9g} " \
            f"(err/bound {r:.3g})"
    assert rg <= 1.0, f"{what}: dlogits err/bound {rg:.3g}"


# ---------------------------------------------------------------------- top-k

def tied_logits(M, C, gen):
    """bf16-valued fp32 logits in which every row has ties: multiples of 1/8
    from randn, clamped to [-2, 2] (33 levels) at C >= 100, two levels below."""
    if C >= 100:
        v = ((torch.randn(M, C, generator=gen) * 8).round() / 8).clamp(-2, 2)
    else:
        v = torch.randint(0, 2, (M, C), generator=gen).float() - 0.5
    out = v.to(torch.bfloat16).float()
    assert torch.equal(out, v)
    return out


def rows_with_ties(logits):
    s = logits.sort(dim=1).values
    if s.shape[1] < 2:
        return 0
    return int((s[:, 1:] == s[:, :-1]).any(dim=1).sum())


def topk_case(M, C, maxk):
    """-> (logits (M, C) bf16-valued fp32, targets): data on which a wrong
    top-k shows. Random targets at C >= 100 are almost never within the top
    8, so the targets are picked from each row's ranking instead: row i takes
    the column at rank 0, 0, 1, 2, ..., maxk in turn (a hit at every k and a
    miss; rank 0 twice, so that no tie group has all its members as targets
    equally often - otherwise swapping the winners within each group would
    leave the counts as they are).

    At C >= 100 the head of each row is planted above the tied background:
    ``maxk + 3`` columns at random indices carry the values 6, 6, 5.5, 5.5,
    5, ... in random order, so every target is tied with a partner, on either
    side of it, and which of the two ranks first is decided by the index
    alone. At C > 256 half of the planted columns lie at indices >= 256 (the
    second trip of the kernel's strided loop) and every odd row's target is
    one of them."""
    gen = torch.Generator().manual_seed(M * 1009 + C)
    lg = tied_logits(M, C, gen)
    npl = maxk + 3
    y = torch.empty(M, dtype=torch.long)
    for i in range(M):
        r = min(max(i % (maxk + 2) - 1, 0), C - 1)
        hi = None
        if C >= 100:
            if C > 256:
                nhi = min(npl - npl // 2, C - 256)
                hi = 256 + torch.randperm(C - 256, generator=gen)[:nhi]
                lo = torch.randperm(256, generator=gen)[:npl - nhi]
                cols = torch.cat([lo, hi])
            else:
                cols = torch.randperm(C, generator=gen)[:npl]
            vals = 6.0 - 0.5 * (torch.arange(npl) // 2).float()
            lg[i, cols] = vals[torch.randperm(npl, generator=gen)]
        order = lg[i].sort(descending=True, stable=True).indices
        y[i] = order[r]
        if hi is not None and i % 2 == 1 and y[i] < 256:
            # hand the target's value to a planted column >= 256
            a, b = int(y[i]), int(hi[i % len(hi)])
            va, vb = lg[i, a].item(), lg[i, b].item()
            lg[i, a], lg[i, b] = vb, va
            y[i] = b
    return lg, y


def topk_ref(logits, targets, maxk, higher_wins=False, ncols=None):
    """Exact counts (maxk,) int64: descending order, lower index wins ties;
    the target counts for k when its rank is below k. The keyword arguments
    give the counts of two wrong kernels, for the tests that show the data
    tells them apart: ties going to the higher index, and only the first
    ``ncols`` columns read."""
    lf = logits.detach().cpu().double()
    y = targets.detach().cpu().view(-1, 1)
    vt = lf.gather(1, y)
    idx = torch.arange(lf.shape[1]).view(1, -1)
    first = (idx > y) if higher_wins else (idx < y)
    ahead = (lf > vt) | ((lf == vt) & first)
    rank = ahead.sum(1)
    seen = torch.ones_like(rank, dtype=torch.bool)
    if ncols is not None:
        rank = (ahead & (idx < ncols)).sum(1)
        seen = y.view(-1) < ncols
    return torch.stack([((rank < k) & seen).sum()
                        for k in range(1, maxk + 1)])


def topk_case_is_telling(logits, targets, maxk):
    """What makes a top-k case worth running: ties in at least half of the
    rows, expected counts that are neither all zero nor (with more than one
    row) all M, counts that differ when ties go to the higher index, and at
    C > 256 counts that differ when only the first 256 columns are read."""
    M, C = logits.shape
    want = topk_ref(logits, targets, maxk)
    assert 2 * rows_with_ties(logits) >= M
    assert want.max() > 0 and (M == 1 or want.min() < M), want.tolist()
    assert want.tolist() != topk_ref(logits, targets, maxk,
                                     higher_wins=True).tolist()
    if C > 256:
        assert want.tolist() != topk_ref(logits, targets, maxk,
                                         ncols=256).tolist()
        hit = topk_ref(logits[targets >= 256], targets[targets >= 256], maxk)
        assert hit[-1] > 0, "no target at an index >= 256 is within top-k"
    return want


def topk_constructed():
    """Four rows with known outcome at maxk = 5 -> (logits (4, 12) fp32,
    targets, counts (5,))."""
    C = 12
    lg = torch.arange(C, dtype=torch.float32).neg().repeat(4, 1) * 0.25 - 3
    lg[0] = 1.5                       # all equal, target 0: counts at k = 1
    lg[1] = 1.5                       # all equal, target 6: misses at k = 5
    lg[2, [1, 3, 4, 7, 9]] = 2.0      # target 9 tied with 4 lower: rank 4
    lg[3, [2, 5, 6, 8, 11]] = 2.0     # target 2 tied with 4 higher: rank 0
    y = torch.tensor([0, 6, 9, 2])
    return lg, y, torch.tensor([2, 2, 2, 2, 3])
