"""K-means initialisation of the proxies of a multi-proxy cosine head
(PODNet's LSC): the K proxies of a new class start at the K k-means centres
of that class's unit features.

Definition (shared by csrc/kmeans.hip, the CPU path below, tests/_kmeans_ref.py
and docs/kernels.md), with ``x^ = x / max(|x|_2, 1e-12)``. Per class with rows
``f_0..f_{n-1}`` (n >= K), on the unit rows, squared Euclidean distance:

* seeding (deterministic maximin, no random numbers): centre 0 is the row
  nearest to the mean of the unit rows; centre j is the row whose smallest
  squared distance to centres 0..j-1 is largest; every tie goes to the lower
  row index. Before the first pass only the K seed rows are assigned, each to
  its own centre (a row seeded twice keeps the later centre); every other row
  is unassigned, which differs from every centre.
* Lloyd iteration: assign each row to its nearest centre (ties to the lower
  centre index); each centre with members becomes their mean, summed in
  ascending row order; a centre that has lost all its members keeps its
  previous value. Stop after the first iteration whose assignment pass
  changed no row, or after ``max_iter`` iterations; ``iters`` counts the
  assignment passes run. (So n = K gives iters = 1: every row is its own
  centre.)
* output: ``proxies (C K, D)`` fp32, class-major, each row its centre divided
  by ``max(|centre|, 1e-12)``; ``assign (n,)`` int32, class-local centre index
  of every row; ``iters (C,)`` int32.

The distance is evaluated as ``|c_k|^2 - 2 x^ . c_k + |x^|^2`` (clamped at 0).
On a GPU the HIP kernel is the only path (one launch for all classes, no
ATen fallback); CPU tensors use the torch fp32 implementation below: the same
tie rules, and a row's distances are computed by the same operations wherever
the row sits, so identical rows tie exactly. Its D- and n-term sums run in
torch's order, not the kernel's.
"""

import numpy as np
import torch

from ._backend import use_hip, ext
from .nme import EPS, _f32, _unit_rows

MAX_PROXY = 16
MAX_KD = 16000          # (K, D) fp32 centres in the kernel's LDS
MAX_ABS = 2.0 ** 48


def kmeans_supported(n, D, K):
    """The shape rule of ``cilfw_kmeans_supported`` (csrc/kmeans.hip); ``n`` is
    the smallest class."""
    return D % 4 == 0 and 4 <= D <= 4096 and 1 <= K <= MAX_PROXY \
        and K * D <= MAX_KD and n >= K


def _first_min(v):
    """Index of the first minimum along the last dim (lowest index on ties)."""
    m = v.min(dim=-1, keepdim=True).values
    idx = torch.arange(v.shape[-1]).expand_as(v)
    return torch.where(v == m, idx, v.shape[-1]).min(dim=-1).values


def _dist(X, xx, cen):
    """(n, D), (n,), (K, D) -> (n, K) squared distances, the kernel's
    formula."""
    c2 = (cen * cen).sum(dim=1)
    step = max(1, (1 << 24) // max(cen.numel(), 1))
    dots = torch.cat([(X[r:r + step, None, :] * cen[None]).sum(dim=2)
                      for r in range(0, X.shape[0], step)])
    return (c2[None] - 2.0 * dots + xx[:, None]).clamp_min(0.0)


def _kmeans_class(X, K, max_iter):
    """One class on its unit rows X (n, D) fp32 -> (centres, assign, iters)."""
    n, D = X.shape
    xx = (X * X).sum(dim=1)
    mean = X.sum(dim=0) / n
    row = int(_first_min(_dist(X, xx, mean[None])[:, 0]))
    cen = torch.empty(K, D)
    assign = torch.full((n,), -1, dtype=torch.int64)
    dmin = None
    for j in range(K):
        cen[j] = X[row]
        assign[row] = j
        if j + 1 < K:
            d = _dist(X, xx, cen[j:j + 1])[:, 0]
            dmin = d if dmin is None else torch.minimum(dmin, d)
            row = int(_first_min(-dmin))
    it = 0
    while it < max_iter:
        it += 1
        new = _first_min(_dist(X, xx, cen))
        changed = bool((new != assign).any())
        assign = new
        cnt = torch.bincount(assign, minlength=K)
        sums = torch.zeros(K, D).index_add_(0, assign, X)
        has = cnt > 0
        cen[has] = sums[has] / cnt[has, None].to(torch.float32)
        if not changed:
            break
    return cen, assign, it


def kmeans_proxies(feats, seg_off, nb_proxy, max_iter=100):
    """feats (n, D), rows grouped by class; seg_off (C+1,) row offsets of the
    class segments (tensor, array or list; read on the host) -> (proxies
    (C nb_proxy, D) fp32 unit rows, assign (n,) int32, iters (C,) int32).
    A class with fewer than ``nb_proxy`` rows and non-finite features raise
    ValueError."""
    feats = _f32(feats)
    if feats.dim() != 2:
        raise ValueError("kmeans_proxies: features must be a 2-d tensor (n, D)")
    n, D = feats.shape
    K, max_iter = int(nb_proxy), int(max_iter)
    if max_iter < 1:
        raise ValueError(
            f"kmeans_proxies: max_iter must be >= 1 (got {max_iter})")
    if not 1 <= K <= MAX_PROXY:
        raise ValueError(
            f"kmeans_proxies: nb_proxy must be in 1..{MAX_PROXY} (got {K})")
    if torch.is_tensor(seg_off):
        seg_off = seg_off.detach().cpu().numpy()
    off = np.asarray(seg_off, dtype=np.int64).reshape(-1)
    assert off.size >= 2 and off[0] == 0 and off[-1] == n \
        and (np.diff(off) >= 0).all(), \
        f"kmeans_proxies: seg_off must run from 0 to n = {n} (got {off})"
    q = np.diff(off)
    if (q < K).any():
        raise ValueError(
            f"kmeans_proxies: class segment(s) {np.where(q < K)[0].tolist()} "
            f"hold fewer than nb_proxy = {K} rows")
    if not kmeans_supported(int(q.min()), D, K):
        raise ValueError(
            f"kmeans_proxies: unsupported shape (D, nb_proxy) = ({D}, {K}): "
            f"needs D % 4 == 0, 4 <= D <= 4096 and nb_proxy * D <= {MAX_KD} "
            f"(the kernel keeps the centres in LDS)")
    if use_hip(feats):
        so = torch.from_numpy(off.astype(np.int32)).to(feats.device)
        return ext().kmeans_proxies(feats, so, K, max_iter)
    a = feats.abs().amax().item() if feats.numel() else 0.0
    if not (a <= MAX_ABS):  # written so that NaN fails
        raise ValueError(
            f"kmeans_proxies: features must be finite with max|f| <= 2^48 "
            f"(got max|f| = {a}); a diverged run cannot be clustered")
    xh = _unit_rows(feats)
    cens, assigns, iters = [], [], []
    for a, b in zip(off[:-1], off[1:]):
        cen, asg, it = _kmeans_class(xh[a:b], K, max_iter)
        cens.append(cen / cen.norm(dim=1, keepdim=True).clamp_min(EPS))
        assigns.append(asg.to(torch.int32))
        iters.append(it)
    return torch.cat(cens), torch.cat(assigns), \
        torch.tensor(iters, dtype=torch.int32)
