"""fp64 oracle, seeded inputs and allowances for LUCIR's margin-ranking loss
(cilfw/ops/margin.py, csrc/mrank.hip), shared by test_margin_rank.py and
test_margin_rank_gpu.py.

Definition (ops/margin.py). ``s = 1/sigma`` for ``sigma > 0`` else 0; row m is
an old row iff ``0 <= targets[m] < known``; ``a = logits[m, targets[m]]``;
``n_1..n_k`` at classes ``c_1..c_k``: the k largest of ``logits[m, known:C]``,
descending, ties to the lower class; ``sm = fp32(sigma margin)``;
``v_j = sm - (a - n_j)``; active iff ``v_j > 0``; ``rho_m = sum_j max(v_j,
0)``; ``N`` old rows; ``q = s / (k max(N, 1))``; ``loss = q sum_m rho_m``;
for upstream g: ``dlogits[m, c_j] = g q`` (active), ``dlogits[m, targets[m]]
= -g q A_m``, 0 elsewhere; ``dsigma = g s q sum_active (a - n_j)``.

The oracle works in fp64 from the logits as given (bf16-rounded for the
kernels) and the fp32 value of sigma. ``sm`` is the fp32 product of the fp32
sigma and the fp32 margin, which fp64 reproduces exactly (the product of two
fp32 numbers is exact in fp64 and is then rounded once to fp32), so the
oracle and the implementation share the very same ``sm``.

Allowances in the form of ``_oracle`` (``u = 2^-24``, ``c = C_SUM = 2``,
``e = 2^-8`` half a bf16 ulp): ``c n u mag (+ e |ref| for a bf16 result)``.
``mag`` is the reference formula with absolute values in place of every
subtraction and every signed sum; ``n`` counts the fp32 roundings:

* ``loss``: ``a - n_j`` and ``sm - (.)`` (2), the sum over the k pairs of the
  row (k), the sum over the rows in any order (strided chains and the 8-level
  tree of mrank_finalize, or torch's sum: at most ``M + 9``), ``1/sigma``,
  the division by ``k max(N, 1)`` (an exact fp32 integer) and the last
  product (3): ``n = k + M + 14`` against
  ``mag = q sum_active (|sm| + |a| + |n_j|)``.
* ``dsigma``: ``a - n_j`` (1), the two sums (``k + M + 9``), ``q`` (2), the
  products ``s q``, ``(s q) sum`` and ``g (.)`` (3), ``s`` (1):
  ``n = k + M + 16`` against ``mag = |g| s q sum_active (|a| + |n_j|)``.
* ``dlogits``: ``q`` (3 roundings with ``s``), ``g q`` and ``(g q) A_m`` (2):
  ``n = 5`` against ``mag = |ref|``, plus half a bf16 ulp for the kernel's
  bf16 result. Where the reference is 0 the bound is 0: every element outside
  the at most ``k + 1`` entries of a row must be exactly 0 (``_oracle.worst``
  gives inf for any error where the bound is zero, and for a non-finite
  value).
* The selected set ``sel`` is compared exactly. The fp32 evaluation of
  ``v_j`` from exact bf16 inputs errs by about ``2 u max(|sm|, |a - n_j|)``
  (< 1e-6 here), so with every ``|v_j| >= MIN_ABS_V = 1e-4`` in the oracle the
  active set is unambiguous; test_margin_rank.py asserts that of every
  fixture.

Inputs (``make_case``): cosines ``0.1 randn`` for every class; the target
cosine of an old row is "confident" (uniform in [0.9, 1)) or "weak" (uniform
in [-0.2, 0.75)) in turn, so that with margin 0.5 active and inactive
pairs occur, within one row too; every third row is a new-class row.
``logits = bf16(fp32(sigma) cos)``. One seeded CPU generator per shape; the
seeds of ``SEEDS`` were picked on the oracle alone: the first under which the
shape meets the fixture conditions of test_margin_rank.py and, where one of
the first four does, holds a row with some but not all pairs active ("lucir",
"ragged", "k8"). No element, row or pair is excluded from a comparison.

Calibration record: no constant was calibrated. Largest err/allowance on
MI355X over the five shapes and both upstreams (profiles/margin_rank.md):
loss 0.022, dlogits 0.87 (its half ulp), dsigma 0.014; the total sigma.grad
through cosine_linear 0.005 of the two summed allowances.
"""

import numpy as np
import torch

import _oracle

MIN_ABS_V = 1e-4
SIGMA = 3.7  # rounded to fp32 by make_case
MARGIN = 0.5

# (M, C, known, k)
SHAPES = {
    "degenerate": (1, 2, 1, 1),     # one old row, one new class
    "lucir": (5, 10, 5, 2),         # one full 4-row block + 1 row
    "ragged": (70, 67, 31, 2),      # odd row stride, odd known
    "k8": (9, 40, 32, 8),           # k = C - known = 8: every new class
    "wide": (7, 1100, 100, 3),      # several sweeps per lane
}
SHAPE_IDS = list(SHAPES)
SEEDS = {"degenerate": 0, "lucir": 0, "ragged": 0, "k8": 3, "wide": 0}


def _gen(name, seed):
    return torch.Generator().manual_seed(
        7919 * (SHAPE_IDS.index(name) + 1) + seed)


def make_case(name, seed=None):
    """-> logits (M, C) bf16, targets (M,) int64, sigma (1,) fp32, known, k,
    margin."""
    M, C, known, k = SHAPES[name]
    g = _gen(name, SEEDS[name] if seed is None else seed)
    cos = 0.1 * torch.randn(M, C, generator=g)
    rows = torch.arange(M)
    is_new = rows % 3 == 2
    t_old = torch.randint(0, known, (M,), generator=g)
    t_new = torch.randint(known, C, (M,), generator=g)
    targets = torch.where(is_new, t_new, t_old)
    conf = 0.9 + 0.1 * torch.rand(M, generator=g)
    weak = -0.2 + 0.95 * torch.rand(M, generator=g)
    a = torch.where(rows % 3 == 0, conf, weak)
    cos[rows[~is_new], targets[~is_new]] = a[~is_new]
    sigma = torch.tensor([SIGMA], dtype=torch.float32)
    logits = (sigma * cos.clamp(-1, 1)).to(torch.bfloat16)
    return logits, targets, sigma, known, k, MARGIN


def tie_case(dtype=torch.float32):
    """Row 0 (old): equal maxima at known + 1 and known + 65."""
    M, C, known = 2, 80, 10
    logits = torch.full((M, C), -1.0)
    logits[:, 0] = 0.5
    logits[0, known + 1] = logits[0, known + 65] = 2.0
    logits[1, known + 7] = 2.0
    logits[1, known + 3] = 1.0
    return logits.to(dtype), torch.tensor([0, 0]), \
        torch.tensor([2.0], dtype=torch.float32), known


def mr_ref(logits, targets, sigma, known, k, margin, up=1.0):
    """fp64 oracle for upstream ``up`` -> dict of references, magnitudes and
    the shape."""
    L = logits.detach().cpu().double()
    t = targets.detach().cpu().long()
    M, C = L.shape
    sg32 = np.float32(sigma.detach().cpu().float().reshape(-1)[0].item())
    sg = float(sg32)
    sm = float(np.float32(sg32 * np.float32(margin)))
    s = 1.0 / sg if sg > 0 else 0.0
    old = (t >= 0) & (t < known)
    a = L.gather(1, t.clamp(0, C - 1)[:, None])
    n, idx = torch.sort(L[:, known:], dim=1, descending=True, stable=True)
    n, cls = n[:, :k], idx[:, :k] + known
    diff = a - n
    v = sm - diff
    active = (v > 0) & old[:, None]
    act = active.double()
    N = int(old.sum())
    q = s / (k * max(N, 1))
    vmag = abs(sm) + a.abs() + n.abs()
    dmag = a.abs() + n.abs()
    dl = torch.zeros(M, C, dtype=torch.float64)
    dl.scatter_(1, cls, up * q * act)
    dl.scatter_add_(1, t.clamp(0, C - 1)[:, None],
                    -up * q * act.sum(dim=1, keepdim=True))
    v_old = v[old]
    return dict(
        M=M, C=C, k=k, N=N, q=q, s=s, sm=sm, old=old, active=active,
        sel=torch.where(active, cls, torch.full_like(cls, -1)
                        ).to(torch.int32),
        loss=(q * (v * act).sum()).reshape(1),
        loss_mag=(q * (vmag * act).sum()).reshape(1),
        dsigma=(up * s * q * (diff * act).sum()).reshape(1),
        dsigma_mag=(abs(up) * s * q * (dmag * act).sum()).reshape(1),
        dlogits=dl,
        min_abs_v=(v_old.abs().min().item() if v_old.numel() else
                   float("inf")),
        n_active=int(active.sum()), n_inactive=int((~active)[old].sum()),
        n_partial=int(((act.sum(dim=1) > 0) & (act.sum(dim=1) < k)).sum()))


# ---------------------------------------------------------------- comparators
# each -> max err/allowance over every element

def n_loss(ref):
    return ref["k"] + ref["M"] + 14.0


def n_dsigma(ref):
    return ref["k"] + ref["M"] + 16.0


N_DLOGITS = 5.0


def worst_loss(got, ref):
    return _oracle.worst(got.reshape(1), ref["loss"], ref["loss_mag"],
                         n_loss(ref), False)[0]


def worst_dsigma(got, ref):
    return _oracle.worst(got.reshape(1), ref["dsigma"], ref["dsigma_mag"],
                         n_dsigma(ref), False)[0]


def bound_dsigma(ref):
    return _oracle.bound(ref["dsigma"], ref["dsigma_mag"], n_dsigma(ref),
                         False)


def worst_dlogits(got, ref):
    assert tuple(got.shape) == tuple(ref["dlogits"].shape), \
        f"dlogits: shape {tuple(got.shape)} vs {tuple(ref['dlogits'].shape)}"
    return _oracle.worst(got, ref["dlogits"], ref["dlogits"].abs(),
                         N_DLOGITS, got.dtype == torch.bfloat16)[0]


def same_sel(got, ref):
    g = got.detach().cpu()
    return g.dtype == torch.int32 and tuple(g.shape) == tuple(
        ref["sel"].shape) and torch.equal(g, ref["sel"])
