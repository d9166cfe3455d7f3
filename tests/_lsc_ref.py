"""fp64 oracle, seeded inputs and allowances for PODNet's local similarity
classifier and NCA loss (cilfw/ops/lsc.py, csrc/lsc.hip), shared by
test_lsc_nca.py and test_lsc_nca_gpu.py.

Definitions (ops/lsc.py). ``lsc_reduce``: ``a_k = softmax_k(gamma s_k)`` over
the K proxies of a class, ``yhat = sum_k a_k s_k``, ``logits = sigma yhat``;
``dsims = sigma g a_k (1 + gamma (s_k - yhat))``, ``dsigma = sum g yhat``.
``nca_loss``: a row with a target outside 0..C-1 is skipped; otherwise
``sm = fp32(sigma margin)``, ``mx = max_{i != y} l_i``, ``S = sum_{i != y}
exp(l_i - mx)``, ``lse = mx + log S``, ``h = lse - (l_y - sm)``, active iff
``h > 0``, ``loss = (1/M) sum_m max(h_m, 0)``; ``dlogits[i] = (g/M) exp(l_i -
lse)`` (``i != y``), ``dlogits[y] = -g/M`` on active rows, 0 elsewhere;
``dsigma = (g/M) margin A``.

The oracle works in fp64 from the inputs as given (bf16-rounded for the
kernels), the fp32 value of sigma and the fp32 values of gamma and margin.
``sm`` is the fp32 product of two fp32 numbers, which fp64 reproduces exactly
and then rounds once, so oracle and implementation share the same ``sm``.

Allowances in the form of ``_oracle.bound``: ``c n u mag + extra (+ e |ref|
for a bf16 result)`` with ``u = 2^-24``, ``c = C_SUM = 2``, ``e = 2^-8`` and
``eps = EPS_TRANS = 2^-21`` of ``_head_ref`` for each ``exp`` / ``log``.
``mag`` is the reference formula with absolute values in place of every
subtraction and signed sum; ``n`` counts the fp32 roundings; ``extra``
carries what is not a rounding of the result's own terms (the
transcendentals and the amplified error of an ``exp`` argument).

lsc_reduce, per class, ``S = max_k |s_k|``:

* ``e_k = exp(gamma s_k - mx)``: the product (error ``u gamma S``), the
  maximum (one of those products: ``u gamma S``) and the subtraction
  (``|.| <= 2 gamma S``: ``2 u gamma S``) leave the argument off by at most
  ``4 u gamma S``, which ``exp`` turns into a relative error; with its own
  ``eps``: ``rel_e = eps + 4 c u gamma S``.
* ``yhat`` is a mean of the ``s_k`` under weights each off by ``rel_e``
  relatively: to first order it moves by at most ``2 rel_e sum_k a_k |s_k -
  yhat|`` (``extra``). Roundings: each term of the numerator goes through
  its weight (the division by Z, or none when the division comes last), its
  product and at most ``K - 1`` adds (``K + 1``), the sum Z through
  ``K - 1`` adds and the final division (``K``, rounded up to ``K + 1``):
  ``n = 2 K + 2`` against ``mag = sum_k a_k |s_k|``.
* ``logits``: one more product: ``n = 2 K + 3`` against ``|sigma| mag``,
  ``|sigma| extra``, plus half a bf16 ulp.
* ``dsims``: Z and the division (``K + 1``), ``s_k - yhat``, ``gamma (.)``,
  ``1 + (.)`` (3), the products ``sigma g``, ``(.) a_k`` and ``(.) w`` (3):
  ``n = K + 7`` against ``mag = |sigma g| a_k (1 + gamma (|s_k| +
  |yhat|))``; ``extra = |sigma g| a_k (2 rel_e (1 + gamma (|s_k| + |yhat|))
  + gamma d_yhat)``, ``d_yhat`` the whole fp32 allowance of ``yhat`` (the
  backward reads the saved fp32 ``yhat``); plus half a bf16 ulp.
* ``dsigma``: the product ``g yhat`` (1), the sum over a row's classes in
  any order (strided chains and the 6-level butterfly, or torch's sum: at
  most ``C + 6``), the sum over the rows (cos_sum's chains and 8-level tree:
  at most ``M + 8``) and its scale (1): ``n = C + M + 16`` against ``mag =
  sum |g| sum_k a_k |s_k|``; ``extra = sum |g| d_yhat``.

nca_loss, per row, ``L = max_i |l_i|``:

* ``exp(l_i - mx)``: the subtraction (``|.| <= 2 L``) rounds once: relative
  ``eps + 2 c u L``; ``S`` sums ``C - 1`` non-negative terms in any order
  (relative ``c C u``); ``log S`` is off by that relative error of ``S`` plus
  ``eps |log S|``; ``lse = mx + log S`` rounds once:
  ``d_lse = c u (|lse| + 2 L + C) + eps (1 + |log S|)``.
* ``h``: the three roundings of ``mx + log S``, ``l_y - sm`` and ``lse -
  (.)``, each at most ``u hmag`` with ``hmag = |mx| + |log S| + |l_y| +
  |sm|``: ``d_h = c u (3 hmag + 2 L + C) + eps (1 + |log S|)``; 0 for a
  skipped row, whose ``h`` is exactly 0.
* ``loss``: the sum over the rows in any order (``M + 9``, as in
  ``_mr_ref``), ``1/M`` and the product (2): ``n = M + 11`` against ``mag =
  (1/M) sum_active hmag``; ``extra = (1/M) sum_active d_h``.
* ``dlogits`` of an active row, ``i != y``: ``l_i - lse`` rounds once
  (``u (L + |lse|)``) and inherits ``d_lse``; ``exp`` makes both relative
  and adds ``eps``: ``extra = |ref| (eps + d_lse + c u (L + |lse|))``;
  ``1/M``, ``g (1/M)`` and the product (3): ``n = 3`` against ``|ref|``, plus
  half a bf16 ulp. At the target ``-g/M``: ``n = 2``, no ``extra``. Where the
  oracle is exactly 0 (every element of an inactive or skipped row) the
  bound is 0 (``_oracle.worst`` gives inf for any error where the bound is
  zero, and for a non-finite value).
* ``dsigma``: ``margin A`` (A an exact fp32 integer), ``1/M``, their product
  and ``g (.)``: ``n = 4`` against ``|ref|``.
* The active set is compared exactly. ``d_h`` is below 2e-4 for every
  fixture (its ``c C u`` term at C = 1100), so with every ``|h_m| >=
  MIN_ABS_H = 1e-3`` in the oracle the set is unambiguous; test_lsc_nca.py
  asserts both of every fixture.

Inputs. ``make_lsc``: sims uniform in [-1, 1] rounded to bf16 (spread
proxies: the softmax weights of a class differ by up to e^(2 gamma)), the
upstream from ``_oracle.signed_unit``, ``sigma = 3.7``. ``make_nca``:
``sigma = 8``, ``margin = 0.6``, cosines ``0.1 randn``; odd rows are shifted
by -0.6 and get a target cosine in [0.9, 1) (inactive), even rows a target
cosine in [-0.2, 0.7); ``logits = bf16(sigma cos)``. One seeded CPU
generator per shape; the seeds of ``NCA_SEEDS`` were picked on the oracle
alone: the first under which the shape meets the fixture conditions of
test_lsc_nca.py (every multi-row shape holds an active and an inactive row,
every ``|h_m| >= MIN_ABS_H``). No element or row is excluded from any
comparison.

Calibration record: no constant was calibrated; ``eps`` stands at its
derived 2^-21 and ``c`` at ``C_SUM``. Largest err/allowance over every shape,
gamma and upstream. The project's fp32 CPU path (fp32 results,
test_lsc_nca.py): logits 0.1913, dsims 0.0780, lsc dsigma 0.0017; loss
0.0145, h 0.0390, dlogits 0.1875, nca dsigma 0.0574. MI355X (bf16 results,
whose half ulp is the first term of the allowance; profiles/lsc_nca.md):
logits 0.9943, dsims 0.9907, lsc dsigma 0.0030; loss 0.0034, h 0.0485,
dlogits 0.9822, nca dsigma 0.1982. The CPU path's results rounded to bf16
read logits 0.9943, dsims 0.9907, dlogits 0.9822 as well.
"""

import numpy as np
import torch

import _oracle
from _oracle import U_F32 as U, C_SUM
from _head_ref import EPS_TRANS as EPS

MIN_ABS_H = 1e-3
LSC_SIGMA = 3.7   # rounded to fp32 by make_lsc
NCA_SIGMA = 8.0
MARGIN = 0.6

# (M, C, K)
LSC_SHAPES = {
    "one": (1, 1, 1),          # smallest possible
    "podnet": (5, 10, 10),     # one full 4-row block + 1 row, 20-byte stride
    "odd": (70, 67, 3),        # odd row stride 201
    "kmax": (9, 5, 16),        # K at its maximum
    "wide": (7, 1100, 2),      # several sweeps per lane
}
LSC_IDS = list(LSC_SHAPES)
GAMMAS = [1.0, 4.0]

# (M, C)
NCA_SHAPES = {
    "degenerate": (1, 2),
    "small": (5, 10),
    "ragged": (70, 67),
    "wide": (7, 1100),
}
NCA_IDS = list(NCA_SHAPES)
NCA_SEEDS = {"degenerate": 0, "small": 0, "ragged": 0, "wide": 0}


def _gen(salt, index, seed):
    return torch.Generator().manual_seed(salt * (index + 1) + seed)


def _f32(v):
    return float(np.float32(v))


# ------------------------------------------------------------------ lsc_reduce

def make_lsc(name, seed=0):
    """-> sims (M, C K) bf16, sigma (1,) fp32, K, upstream g (M, C) bf16."""
    M, C, K = LSC_SHAPES[name]
    g = _gen(7907, LSC_IDS.index(name), seed)
    sims = (2 * torch.rand(M, C * K, generator=g) - 1).to(torch.bfloat16)
    up = _oracle.signed_unit((M, C), g)
    return sims, torch.tensor([LSC_SIGMA], dtype=torch.float32), K, up


def lsc_ref(sims, sigma, K, gamma, g):
    """fp64 oracle -> dict of references, magnitudes, counts and extras."""
    M, CK = sims.shape
    C = CK // K
    s = sims.detach().cpu().double().reshape(M, C, K)
    gg = g.detach().cpu().double().reshape(M, C)
    sg = _f32(sigma.detach().cpu().float().reshape(-1)[0].item())
    gm = _f32(gamma)
    a = torch.softmax(gm * s, dim=2)
    yhat = (a * s).sum(dim=2)
    ymag = (a * s.abs()).sum(dim=2)
    spread = (a * (s - yhat[:, :, None]).abs()).sum(dim=2)
    rel_e = EPS + 4 * C_SUM * U * gm * s.abs().amax(dim=2)
    y_extra = 2 * rel_e * spread
    d_yhat = _oracle.bound(yhat, ymag, 2.0 * K + 2, False, extra=y_extra)
    wmag = 1 + gm * (s.abs() + yhat.abs()[:, :, None])
    sgg = (abs(sg) * gg.abs())[:, :, None]
    return dict(
        M=M, C=C, K=K, a=a,
        yhat=yhat, yhat_mag=ymag, yhat_extra=y_extra,
        logits=sg * yhat, logits_mag=abs(sg) * ymag,
        logits_extra=abs(sg) * y_extra,
        dsims=((sg * gg)[:, :, None] * a
               * (1 + gm * (s - yhat[:, :, None]))).reshape(M, CK),
        dsims_mag=(sgg * a * wmag).reshape(M, CK),
        dsims_extra=(sgg * a * (2 * rel_e[:, :, None] * wmag
                                + gm * d_yhat[:, :, None])).reshape(M, CK),
        dsigma=(gg * yhat).sum().reshape(1),
        dsigma_mag=(gg.abs() * ymag).sum().reshape(1),
        dsigma_extra=(gg.abs() * d_yhat).sum().reshape(1))


def worst_yhat(got, ref):
    return _oracle.worst(got, ref["yhat"], ref["yhat_mag"],
                         2.0 * ref["K"] + 2, False,
                         extra=ref["yhat_extra"])[0]


def worst_logits(got, ref):
    assert tuple(got.shape) == tuple(ref["logits"].shape), \
        f"logits: shape {tuple(got.shape)} vs {tuple(ref['logits'].shape)}"
    return _oracle.worst(got, ref["logits"], ref["logits_mag"],
                         2.0 * ref["K"] + 3, got.dtype == torch.bfloat16,
                         extra=ref["logits_extra"])[0]


def worst_dsims(got, ref):
    assert tuple(got.shape) == tuple(ref["dsims"].shape), \
        f"dsims: shape {tuple(got.shape)} vs {tuple(ref['dsims'].shape)}"
    return _oracle.worst(got, ref["dsims"], ref["dsims_mag"],
                         ref["K"] + 7.0, got.dtype == torch.bfloat16,
                         extra=ref["dsims_extra"])[0]


def worst_lsc_dsigma(got, ref):
    return _oracle.worst(got.reshape(1), ref["dsigma"], ref["dsigma_mag"],
                         ref["C"] + ref["M"] + 16.0, False,
                         extra=ref["dsigma_extra"])[0]


def bound_lsc_dsigma(ref):
    return _oracle.bound(ref["dsigma"], ref["dsigma_mag"],
                         ref["C"] + ref["M"] + 16.0, False,
                         extra=ref["dsigma_extra"])


# -------------------------------------------------------------------- nca_loss

def make_nca(name, seed=None):
    """-> logits (M, C) bf16, targets (M,) int64, sigma (1,) fp32, margin."""
    M, C = NCA_SHAPES[name]
    g = _gen(7919, NCA_IDS.index(name), NCA_SEEDS[name] if seed is None
             else seed)
    cos = 0.1 * torch.randn(M, C, generator=g)
    rows = torch.arange(M)
    odd = rows % 2 == 1
    cos[odd] -= 0.6
    targets = torch.randint(0, C, (M,), generator=g)
    conf = 0.9 + 0.1 * torch.rand(M, generator=g)
    weak = -0.2 + 0.9 * torch.rand(M, generator=g)
    cos[rows, targets] = torch.where(odd, conf, weak)
    sigma = torch.tensor([NCA_SIGMA], dtype=torch.float32)
    logits = (sigma * cos.clamp(-1, 1)).to(torch.bfloat16)
    return logits, targets, sigma, MARGIN


def with_invalid_targets(targets, C):
    """Rows 0 and 2 (where present) get targets -1 and C: skipped rows."""
    t = targets.clone()
    t[0] = -1
    if t.numel() > 2:
        t[2] = C
    return t


def nca_ref(logits, targets, sigma, margin, up=1.0):
    """fp64 oracle for upstream ``up`` -> dict of references, magnitudes and
    allowances."""
    L = logits.detach().cpu().double()
    t = targets.detach().cpu().long()
    M, C = L.shape
    sg32 = np.float32(sigma.detach().cpu().float().reshape(-1)[0].item())
    mg32 = np.float32(margin)
    sm = float(np.float32(sg32 * mg32))
    valid = (t >= 0) & (t < C)
    y = t.clamp(0, C - 1)[:, None]
    pos = torch.zeros(M, C, dtype=torch.bool).scatter_(1, y, True)
    neg = L.masked_fill(pos, float("-inf"))
    mx = neg.amax(dim=1)
    logS = torch.log(torch.exp(neg - mx[:, None]).sum(dim=1))
    lse = mx + logS
    ly = L.gather(1, y)[:, 0]
    zero = torch.zeros(M, dtype=torch.float64)
    h = torch.where(valid, lse - (ly - sm), zero)
    active = (h > 0) & valid
    act = active.double()
    Lmax = L.abs().amax(dim=1)
    hmag = mx.abs() + logS.abs() + ly.abs() + abs(sm)
    d_h = torch.where(valid, C_SUM * U * (3 * hmag + 2 * Lmax + C)
                      + EPS * (1 + logS.abs()), zero)
    d_lse = C_SUM * U * (lse.abs() + 2 * Lmax + C) + EPS * (1 + logS.abs())
    dl = (up / M) * torch.exp(neg - lse[:, None]).masked_fill(pos, -1.0) \
        * act[:, None]
    rel = EPS + d_lse + C_SUM * U * (Lmax + lse.abs())
    dl_extra = (dl.abs() * rel[:, None]).masked_fill(pos, 0.0)
    dl_n = torch.full((M, C), 3.0, dtype=torch.float64).masked_fill(pos, 2.0)
    A = int(active.sum())
    h_valid = h[valid]
    return dict(
        M=M, C=C, A=A, sm=sm, valid=valid, active=active,
        h=h, h_allow=d_h,
        loss=((h * act).sum() / M).reshape(1),
        loss_mag=((hmag * act).sum() / M).reshape(1),
        loss_extra=((d_h * act).sum() / M).reshape(1),
        dlogits=dl, dlogits_extra=dl_extra, dlogits_n=dl_n,
        dsigma=torch.tensor([up * float(mg32) * A / M], dtype=torch.float64),
        min_abs_h=(h_valid.abs().min().item() if h_valid.numel()
                   else float("inf")),
        n_active=A, n_inactive=int((~active & valid).sum()))


def worst_h(got, ref):
    """``d_h`` is a finished allowance: ``mag = d_h`` with ``n = 1 / (c u)``,
    a power of two, makes ``_oracle.bound`` return it exactly."""
    return _oracle.worst(got, ref["h"], ref["h_allow"], 1.0 / (C_SUM * U),
                         False)[0]


def worst_loss(got, ref):
    return _oracle.worst(got.reshape(1), ref["loss"], ref["loss_mag"],
                         ref["M"] + 11.0, False, extra=ref["loss_extra"])[0]


def worst_dlogits(got, ref):
    assert tuple(got.shape) == tuple(ref["dlogits"].shape), \
        f"dlogits: shape {tuple(got.shape)} vs {tuple(ref['dlogits'].shape)}"
    return _oracle.worst(got, ref["dlogits"], ref["dlogits"].abs(),
                         ref["dlogits_n"], got.dtype == torch.bfloat16,
                         extra=ref["dlogits_extra"])[0]


def worst_nca_dsigma(got, ref):
    return _oracle.worst(got.reshape(1), ref["dsigma"], ref["dsigma"].abs(),
                         4.0, False)[0]


def bound_nca_dsigma(ref):
    return _oracle.bound(ref["dsigma"], ref["dsigma"].abs(), 4.0, False)


def worst_total_dsigma(got, lref, nref):
    """sigma.grad of ``lsc_reduce -> nca_loss``: autograd adds the two
    contributions (one more rounding, at most ``c u (|a| + |b|)``), so the
    allowance is the sum of the two allowances plus that."""
    ref = lref["dsigma"] + nref["dsigma"]
    allow = bound_lsc_dsigma(lref) + bound_nca_dsigma(nref) \
        + C_SUM * U * (lref["dsigma"].abs() + nref["dsigma"].abs())
    return _oracle.worst(got.reshape(1), ref, allow, 1.0 / (C_SUM * U),
                         False)[0]


def same_active(got, ref):
    g = got.detach().cpu()
    return g.dtype == torch.int32 and tuple(g.shape) == (ref["M"],) \
        and torch.equal(g.bool(), ref["active"]) \
        and bool(((g == 0) | (g == 1)).all())
