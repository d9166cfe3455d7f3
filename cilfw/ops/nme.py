"""Nearest-mean-of-exemplars (NME) classifier ops — iCaRL's rule.

Definition (shared by csrc/nme.hip, the CPU path below and the tests), with
``x^ = x / max(|x|_2, 1e-12)``:

* prototype of class c with exemplar features f_1..f_q (q >= 1):
  ``m = (1/q) sum_i f^_i``, ``p_c = m / max(|m|_2, 1e-12)``;
* score of a feature x for class c: ``s(x, c) = x^ . p_c`` — with unit
  vectors this ranks exactly like ``-|x^ - p_c|^2``: larger = nearer;
* top-k: the k classes with the largest scores, descending; ties go to the
  lower class index.

On a GPU the fused HIP kernels are the only path (no ATen fallback); CPU
tensors use the torch implementation of the same definition.
"""

import numpy as np
import torch

from ._backend import use_hip, ext

EPS = 1e-12


def _f32(t):
    return t.detach().to(torch.float32).contiguous()


def _unit_rows(x):
    return x / x.norm(dim=1, keepdim=True).clamp_min(EPS)


def _check_width(D, what):
    assert D % 4 == 0 and 4 <= D <= 4096, \
        f"{what}: nme ops support feature widths D % 4 == 0, 4 <= D <= 4096 " \
        f"(got D = {D})"


def nme_prototypes(feats, seg_off):
    """feats (n, D), rows grouped by class; seg_off (C+1,) row offsets of the
    class segments (tensor, array or list; read on the host). -> (C, D) fp32
    unit-norm prototypes. An empty class segment raises ValueError."""
    feats = _f32(feats)
    assert feats.dim() == 2
    n, D = feats.shape
    _check_width(D, "nme_prototypes")
    if torch.is_tensor(seg_off):
        seg_off = seg_off.detach().cpu().numpy()
    off = np.asarray(seg_off, dtype=np.int64).reshape(-1)
    assert off.size >= 2 and off[0] == 0 and off[-1] == n, \
        f"nme_prototypes: seg_off must run from 0 to n = {n} (got {off})"
    q = np.diff(off)
    if (q <= 0).any():
        raise ValueError(
            f"nme_prototypes: class segment(s) {np.where(q <= 0)[0].tolist()} "
            f"hold no exemplar")
    if use_hip(feats):
        so = torch.from_numpy(off.astype(np.int32)).to(feats.device)
        return ext().nme_prototypes(feats, so)
    fh = _unit_rows(feats)
    m = torch.stack([fh[a:b].mean(dim=0) for a, b in zip(off[:-1], off[1:])])
    return _unit_rows(m)


def nme_topk(feats, protos, maxk, targets=None):
    """-> (idx int32 (N, maxk), score fp32 (N, maxk), counts int64 (maxk,) |
    None). counts[k-1] = number of rows whose target is within the top-k
    (only with ``targets``)."""
    feats, protos = _f32(feats), _f32(protos)
    assert feats.dim() == 2 and protos.dim() == 2 \
        and feats.shape[1] == protos.shape[1]
    N, D = feats.shape
    C = protos.shape[0]
    _check_width(D, "nme_topk")
    maxk = int(maxk)
    assert 1 <= maxk <= min(8, C), \
        f"nme_topk: maxk must be in 1..min(8, C) (got maxk={maxk}, C={C})"
    if targets is not None:
        targets = targets.to(feats.device, torch.int64).contiguous()
        assert targets.shape == (N,)
    if use_hip(feats):
        return ext().nme_topk(feats, protos, maxk, targets)
    xh = _unit_rows(feats)
    # broadcast product + sum over D, not a BLAS matmul: the summation order
    # of a (row, class) pair must not depend on where the class sits, so that
    # bitwise-equal prototypes tie exactly
    step = max(1, (1 << 24) // max(C * D, 1))
    scores = torch.cat([(xh[r:r + step, None, :] * protos[None]).sum(dim=2)
                        for r in range(0, N, step)]) if N else \
        torch.empty(0, C)
    # stable descending sort: equal scores stay in ascending class order
    s, i = torch.sort(scores, dim=1, descending=True, stable=True)
    s, i = s[:, :maxk].contiguous(), i[:, :maxk].contiguous()
    counts = None
    if targets is not None:
        hit = (i == targets[:, None]).cumsum(dim=1) > 0
        counts = hit.sum(dim=0).to(torch.int64)
    return i.to(torch.int32), s, counts
