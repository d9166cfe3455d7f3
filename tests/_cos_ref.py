"""fp64 oracle, seeded inputs and allowances for the cosine head and the
embedding distillation (cilfw/ops/cosine.py, csrc/cosine.hip), shared by
test_cosine_head.py and test_cosine_head_gpu.py.

Definitions. ``r(x) = 1/|x|`` if ``|x| > 0`` else 0; ``x^ = x r(x)``,
``w^ = w r(w)``, ``z = x^ w^T``; ``logits = s z`` (``s`` = sigma); with
``g = dlogits``: ``G = g w^``, ``H = g^T x^``, ``dsigma = sum g z``,
``dx = s r(x) (G - x^ (x^ . G))``, ``dw = s r(w) (H - w^ (w^ . H))``.
Flat: ``u = s^ - t^``, ``l_m = |u_m|^2 / 2``, ``loss = mean l``,
``ds = (g/M) r(s) (u - s^ (s^ . u))``.

The oracle works in fp64 from the bf16-rounded features, the fp32 weights and
the fp32 value of sigma. Allowances in the form of ``_oracle``
(``u = 2^-24``, ``c = C_SUM = 2``, ``e = 2^-8`` half a bf16 ulp):
``c n u mag (+ e |ref| for a bf16 result) + extra``. ``mag`` is always the
reference formula with absolute values in place of every subtraction and
every signed sum. They follow the roundings the implementation makes
(docs/kernels.md, "Cosine head / flat"): sigma is folded into the normalised
features, ``xs = bf16(s x^)``, ``wn = bf16(w^)``, the three GEMMs of
csrc/gemm.hip run on (xs, wn, g), ``G`` comes out of its GEMM in bf16, the
rest is fp32.

* An inverse norm: the sum of D squares (all >= 0, one rounding each through
  the fma) is relative ``D u``, halved by the square root, plus the root and
  the division: ``n = D/2 + 2``, ``mag = |ref|``. A normalised bf16 row
  ``s x^``: two more products, ``n = D/2 + 4``, plus its half ulp.
* A logit ``bf16(sum_k xs_k wn_k)``: half an ulp of the result; the bf16
  rounding of each of the two operands, which acts on every product and so
  counts against ``mag = s sum_k |x^_k w^_k| <= s``, not against ``|ref|``:
  ``extra = ((1+e)^3 - 1 - e) mag`` (the two operand roundings and their
  interplay with the last one); fp32: the two inverse norms and the operand
  products (``D + 10``), the sum over D and the split-K slabs (at most
  ``MAX_SPLIT = 32``, the cap of ``cilfw_linear_ksplit``):
  ``n = 2 D + 10 + MAX_SPLIT``.
* ``dx`` (bf16): ``G`` carries the rounding of ``wn`` and its own bf16
  rounding, both against ``mag_G = |g| |w^|``; they pass through the
  projection as ``mag_dx = s r(x) (mag_G + |x^| (|x^| . mag_G))``:
  ``extra = ((1+e)^3 - 1 - e) mag_dx``; fp32: the GEMM sum over C and its
  slabs, ``w^`` and ``x^`` (``D + 10``), the sum ``x^ . G`` over D, a few
  products: ``n = C + MAX_SPLIT + 2 D + 16``.
* ``dw`` (fp32): the one bf16 rounding is that of ``xs`` in
  ``s H = g^T xs``: ``extra = e mag_dw``,
  ``mag_dw = s r(w) (mag_H + |w^| (|w^| . mag_H))``, ``mag_H = |g|^T |x^|``;
  ``n = M + MAX_SPLIT + 2 D + 16``.
* ``dsigma`` (fp32) ``= sum_m x^_m . G_m``: the two roundings in ``G``,
  ``extra = ((1+e)^2 - 1) mag``, ``mag = sum |g| (|x^| |w^|^T)``;
  ``n = C + MAX_SPLIT + 2 D + M + 16``.
* Flat, all fp32 from bf16 inputs: an element of ``u`` is off by
  ``(D/2 + 6) u (|s^| + |t^|)``; ``l`` doubles it through the square and adds
  the sum over D: ``n = 2 D + 16`` against
  ``mag_l = sum_k (|s^_k| + |t^_k|)^2 / 2 <= 2``; the loss adds the mean over
  M. ``ds`` (bf16): ``n = 3 D + 16`` (``u``, ``s^ . u``, the products)
  against ``mag_ds = (|g|/M) r(s) (|s^| + |t^| + |s^| (|s^| . (|s^| + |t^|)))``.

A zero row has ``mag = 0`` everywhere it enters alone: its logits and its
gradient must then be exactly 0 (``_oracle.worst`` gives inf for any error
where the bound is zero, and for a non-finite value).

Inputs: features ``|randn| + 0.1`` rounded to bf16 (post-ReLU pooled features
are >= 0), weights ``+-(0.3 |randn| + 0.05)`` in full fp32 precision, upstream
``dlogits`` from ``_oracle.signed_unit``; one seeded CPU generator per shape.
No entry is zero, so a dropped term shows. No element, row or class is
excluded from a comparison.

Calibration record: no constant was calibrated. Largest err/allowance on
MI355X over the five shapes (profiles/cosine_head.md): inverse norms 0.11,
the bf16 unit rows 0.98 (their half ulp), logits 0.25, dx 0.58, dw 0.78,
dsigma 0.15, flat rows and loss 0.003, ds 0.96 (its half ulp).
"""

import torch

import _oracle
from _oracle import HALF_ULP_BF16 as E

MAX_SPLIT = 32.0
E2 = (1 + E) ** 2 - 1
E3 = (1 + E) ** 3 - 1 - E

# (M, C, D), each the smallest at which a distinct thing can go wrong
SHAPES = {
    "degenerate": (1, 1, 8),
    "cifar64": (5, 3, 64),       # CIFAR width; one full 4-row block + 1
    "ragged40": (70, 67, 40),    # D below one 512-element sweep; ragged tiles
    "sweep520": (37, 13, 520),   # one lane past a full sweep; fwd split-4
    "wide2048": (7, 300, 2048),  # widest D, C > 256
}
SHAPE_IDS = list(SHAPES)
SIGMA = 3.7  # rounded to fp32 by make_head


def _gen(name, seed):
    return torch.Generator().manual_seed(
        6151 * (SHAPE_IDS.index(name) + 1) + seed)


def make_head(name, seed=0):
    """-> x (M, D) bf16, w (C, D) fp32, sigma (1,) fp32, dy (M, C) bf16."""
    M, C, D = SHAPES[name]
    g = _gen(name, seed)
    x = (torch.randn(M, D, generator=g).abs() + 0.1).to(torch.bfloat16)
    sign = torch.randint(0, 2, (C, D), generator=g).float() * 2 - 1
    w = sign * (0.3 * torch.randn(C, D, generator=g).abs() + 0.05)
    dy = _oracle.signed_unit((M, C), g)
    return x, w, torch.tensor([SIGMA], dtype=torch.float32), dy


def make_feats(name, seed=0):
    """-> student, teacher (M, D) bf16, drawn independently."""
    M, _, D = SHAPES[name]
    g = _gen(name, seed + 1000)
    s = (torch.randn(M, D, generator=g).abs() + 0.1).to(torch.bfloat16)
    t = (torch.randn(M, D, generator=g).abs() + 0.1).to(torch.bfloat16)
    return s, t


def _d(t):
    return t.detach().cpu().double()


def rinv64(a):
    n = a.norm(dim=1, keepdim=True)
    return torch.where(n > 0, 1.0 / torch.where(n > 0, n, torch.ones_like(n)),
                       torch.zeros_like(n))


def _proj(v, G):
    return G - v * (v * G).sum(dim=1, keepdim=True)


def _proj_mag(v, Gm):
    return Gm + v.abs() * (v.abs() * Gm).sum(dim=1, keepdim=True)


def head_ref(x, w, sigma, g):
    """fp64 oracle of cosine_linear and its backward for dlogits ``g`` ->
    dict of references, magnitudes and the shape."""
    x64, w64, g64 = _d(x), _d(w), _d(g)
    s = float(_d(sigma).reshape(-1)[0])
    M, D = x64.shape
    C = w64.shape[0]
    rx, rw = rinv64(x64), rinv64(w64)
    xh, wh = x64 * rx, w64 * rw
    z, zm = xh @ wh.t(), xh.abs() @ wh.abs().t()
    G, Gm = g64 @ wh, g64.abs() @ wh.abs()
    H, Hm = g64.t() @ xh, g64.abs().t() @ xh.abs()
    return dict(
        M=M, C=C, D=D, sigma=s, rx=rx.reshape(M), rw=rw.reshape(C),
        xs=s * xh, wn=wh,
        logits=s * z, logits_mag=abs(s) * zm,
        dx=s * rx * _proj(xh, G), dx_mag=abs(s) * rx * _proj_mag(xh, Gm),
        dw=s * rw * _proj(wh, H), dw_mag=abs(s) * rw * _proj_mag(wh, Hm),
        dsigma=(g64 * z).sum().reshape(1),
        dsigma_mag=(g64.abs() * zm).sum().reshape(1))


def flat_ref(s, t):
    """fp64 oracle of flat_loss for upstream 1 -> dict."""
    s64, t64 = _d(s), _d(t)
    M, D = s64.shape
    rs = rinv64(s64)
    sh, th = s64 * rs, t64 * rinv64(t64)
    u, um = sh - th, sh.abs() + th.abs()
    l, lm = 0.5 * (u * u).sum(dim=1), 0.5 * (um * um).sum(dim=1)
    return dict(M=M, D=D, l=l, l_mag=lm, loss=(l.sum() / M).reshape(1),
                loss_mag=(lm.sum() / M).reshape(1),
                ds=rs * _proj(sh, u) / M, ds_mag=rs * _proj_mag(sh, um) / M)


# ---------------------------------------------------------------- comparators
# each -> max err/allowance over every element

def _same_shape(got, ref, what):
    assert tuple(got.shape) == tuple(ref.shape), \
        f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"


def worst_rinv(got, ref_r, D):
    _same_shape(got, ref_r, "rinv")
    return _oracle.worst(got, ref_r, ref_r.abs(), D / 2 + 2.0, False)[0]


def worst_unit(got, ref_rows, D):
    """A normalised (and scaled) bf16 row matrix."""
    _same_shape(got, ref_rows, "unit rows")
    return _oracle.worst(got, ref_rows, ref_rows.abs(), D / 2 + 4.0, True)[0]


def worst_logits(got, ref):
    _same_shape(got, ref["logits"], "logits")
    mag = ref["logits_mag"]
    return _oracle.worst(got, ref["logits"], mag,
                         2.0 * ref["D"] + 10 + MAX_SPLIT, True,
                         extra=E3 * mag)[0]


def worst_dx(got, ref):
    _same_shape(got, ref["dx"], "dx")
    mag = ref["dx_mag"]
    return _oracle.worst(got, ref["dx"], mag,
                         ref["C"] + MAX_SPLIT + 2.0 * ref["D"] + 16, True,
                         extra=E3 * mag)[0]


def worst_dw(got, ref):
    _same_shape(got, ref["dw"], "dw")
    mag = ref["dw_mag"]
    return _oracle.worst(got, ref["dw"], mag,
                         ref["M"] + MAX_SPLIT + 2.0 * ref["D"] + 16, False,
                         extra=E * mag)[0]


def worst_dsigma(got, ref):
    mag = ref["dsigma_mag"]
    return _oracle.worst(got.reshape(1), ref["dsigma"], mag,
                         ref["C"] + MAX_SPLIT + 2.0 * ref["D"] + ref["M"] + 16,
                         False, extra=E2 * mag)[0]


def worst_flat_rows(got_l, ref):
    _same_shape(got_l, ref["l"], "l")
    return _oracle.worst(got_l, ref["l"], ref["l_mag"],
                         2.0 * ref["D"] + 16, False)[0]


def worst_flat_loss(got_loss, ref):
    return _oracle.worst(got_loss.reshape(1), ref["loss"], ref["loss_mag"],
                         2.0 * ref["D"] + 16 + ref["M"], False)[0]


def worst_flat_grad(got_ds, ref, scale=1.0):
    """``scale``: the upstream factor the oracle (upstream 1) is multiplied
    by."""
    _same_shape(got_ds, ref["ds"], "ds")
    return _oracle.worst(got_ds, ref["ds"] * scale,
                         ref["ds_mag"] * abs(scale), 3.0 * ref["D"] + 16,
                         True)[0]
