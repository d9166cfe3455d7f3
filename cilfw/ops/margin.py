"""LUCIR's margin-ranking loss over the cosine head's logits (Hou et al., CVPR
2019): each old-class sample's ground-truth cosine must beat its ``k`` hardest
new-class cosines by ``margin``.

Definition (shared by csrc/mrank.hip, the CPU path below and the tests) of
``margin_rank_loss(logits, targets, sigma, known, k=2, margin=0.5)``.

* ``logits (M, C)`` are the cosine head's output ``sigma z`` (bf16 on a GPU,
  fp32 or fp64 on the CPU), ``targets (M,)`` int64, ``sigma`` the head's
  1-element parameter on the same device (fp32 on a GPU; the kernels read it
  from device memory, like ``rownorm_fwd``). ``known``, ``k`` and ``margin``
  are host scalars, ``1 <= known < C``, ``1 <= k <= min(8, C - known)``,
  ``margin >= 0``.
* ``s = 1/sigma`` if ``sigma > 0``, else 0: for ``sigma <= 0`` the loss and
  every gradient are exactly 0 and finite.
* Row ``m`` is an *old row* iff ``targets[m] < known``. For an old row
  ``a = logits[m, targets[m]]`` and the negatives ``n_1..n_k`` at classes
  ``c_1..c_k`` are the ``k`` largest of ``logits[m, known:C]``, descending by
  value, ties going to the lower class index (the rule of ``ops.nme_topk``).
* ``v_j = fp32(sigma margin) - (a - n_j)``, in fp32 (fp64 for fp64 input);
  pair ``j`` is *active* iff ``v_j > 0``; ``rho_m = sum_j max(v_j, 0)``.
* ``N`` = number of old rows, ``q = s / (k max(N, 1))``,
  ``loss = q sum_m rho_m``: LUCIR's ``MarginRankingLoss(margin)`` on the
  cosines ``z``, a mean over the ``N k`` (ground truth, hard negative) pairs.
  With no old row the loss is exactly 0.
* Gradients for upstream ``g``: ``dlogits[m, c_j] = +g q`` for each active
  pair, ``dlogits[m, targets[m]] = -g q A_m`` (``A_m`` = active pairs of the
  row), every other element exactly 0;
  ``dsigma = g (s q) sum_active (a - n_j)``, the explicit dependence on
  ``sigma``. It cancels the gradient that reaches ``sigma`` through
  ``cosine_linear`` (the loss is a function of ``z`` alone), so it is
  returned, never dropped. ``targets``, ``known``, ``k`` and ``margin`` get
  no gradient.

On a GPU the logits must be bf16 and the HIP kernels are the only path (no
ATen fallback): no allocation depends on the data, nothing is read on the
host, so the term sits inside a captured step and replays with the current
``sigma``, ``targets`` and upstream (docs/kernels.md, "Margin ranking"). CPU
tensors use the torch implementation below, in fp64 for fp64 logits.
"""

import torch

from ._backend import use_hip, ext

MAX_K = 8


def _check_args(logits, targets, sigma, known, k, margin):
    assert logits.dim() == 2, "margin_rank_loss: logits are (M, C)"
    M, C = logits.shape
    known, k, margin = int(known), int(k), float(margin)
    assert M >= 1 and C >= 2, \
        f"margin_rank_loss: needs M >= 1 rows and C >= 2 classes " \
        f"(got {M} x {C})"
    assert 1 <= known < C, \
        f"margin_rank_loss: known must be in 1..C-1 (got known={known}, " \
        f"C={C})"
    assert 1 <= k <= min(MAX_K, C - known), \
        f"margin_rank_loss: k must be in 1..min({MAX_K}, C - known) " \
        f"(got k={k}, C - known = {C - known})"
    assert margin >= 0.0, \
        f"margin_rank_loss: margin must be >= 0 (got {margin})"
    assert targets.shape == (M,) and targets.dtype == torch.int64 \
        and targets.device == logits.device, \
        "margin_rank_loss: targets are an int64 (M,) tensor on the device " \
        "of the logits"
    assert sigma.numel() == 1 and sigma.device == logits.device, \
        "margin_rank_loss: sigma is a 1-element tensor on the device of " \
        "the logits"
    return known, k, margin


def _mrank_torch(L, t, sg, known, k, margin):
    """The definition in the dtype of ``L`` (fp32 or fp64), ``sg`` 0-d in
    that dtype. -> (loss, sel int32 (M, k), dlogits and dsigma for upstream
    1)."""
    M, C = L.shape
    zero = torch.zeros((), dtype=L.dtype)
    s = torch.where(sg > 0, 1.0 / torch.where(sg > 0, sg, zero + 1), zero)
    old = (t >= 0) & (t < known)
    a = L.gather(1, t.clamp(0, C - 1)[:, None])
    # stable descending sort: equal values stay in ascending class order
    n, idx = torch.sort(L[:, known:], dim=1, descending=True, stable=True)
    n, cls = n[:, :k], idx[:, :k] + known
    diff = a - n
    v = sg * margin - diff
    active = (v > 0) & old[:, None]
    N = int(old.sum())
    q = s / (k * max(N, 1))
    loss = q * torch.where(active, v, zero).sum(dim=1).sum()
    sel = torch.where(active, cls, torch.full_like(cls, -1)).to(torch.int32)
    act = active.to(L.dtype)
    dl = torch.zeros_like(L)
    dl.scatter_(1, cls, q * act)
    dl.scatter_add_(1, t.clamp(0, C - 1)[:, None],
                    -q * act.sum(dim=1, keepdim=True))
    dsig = (s * q) * torch.where(active, diff, zero).sum(dim=1).sum()
    return loss, sel, dl, dsig


class MarginRank(torch.autograd.Function):
    """``q sum_m rho_m``. HIP: saves the selected classes and the scalars of
    mrank_finalize; the backward reads them and the upstream on the
    device."""

    @staticmethod
    def forward(ctx, logits, targets, sigma, known, k, margin):
        known, k, margin = _check_args(logits, targets, sigma, known, k,
                                       margin)
        ctx.sigma_shape, ctx.sigma_dtype = sigma.shape, sigma.dtype
        ctx.shape = (logits.shape[1], known)
        logits = logits.detach().contiguous()
        targets = targets.contiguous()
        ctx.hip = use_hip(logits)
        if ctx.hip:
            e = ext()
            e._bf16(logits, "margin_rank_loss.logits")
            sg = sigma.detach()
            assert sg.dtype == torch.float32, \
                "margin_rank_loss: sigma is a 1-element fp32 tensor on the " \
                "device of the logits (the kernels read it there)"
            loss, sel, fin = e.mrank_fwd(logits, targets, sg.reshape(1),
                                         known, k, margin)[:3]
            ctx.save_for_backward(sel, targets, fin)
            ctx.mark_non_differentiable(sel)
            return loss, sel
        assert logits.dtype in (torch.float32, torch.float64), \
            f"margin_rank_loss: CPU logits are fp32 or fp64 " \
            f"(got {logits.dtype})"
        sg = sigma.detach().to(logits.dtype).reshape(())
        loss, sel, dl, dsig = _mrank_torch(logits, targets, sg, known, k,
                                           margin)
        ctx.save_for_backward(dl, dsig)
        ctx.mark_non_differentiable(sel)
        return loss, sel

    @staticmethod
    def backward(ctx, dloss, _dsel):
        if ctx.hip:
            sel, targets, fin = ctx.saved_tensors
            C, known = ctx.shape
            up = dloss.detach().float().reshape(1).contiguous()
            dl, dsig = ext().mrank_bwd(sel, targets, fin, up, C, known)
            return dl, None, dsig.reshape(ctx.sigma_shape), None, None, None
        dl, dsig = ctx.saved_tensors
        g = dloss.to(dl.dtype)
        return dl * g, None, \
            (dsig * g).reshape(ctx.sigma_shape).to(ctx.sigma_dtype), \
            None, None, None


def margin_rank_loss(logits, targets, sigma, known, k=2, margin=0.5):
    """LUCIR's margin-ranking loss (module docstring) -> 0-d loss."""
    return MarginRank.apply(logits, targets, sigma, known, k, margin)[0]


def margin_rank_select(logits, targets, sigma, known, k=2, margin=0.5):
    """The selected set ``sel (M, k)`` int32 (no autograd): the class index
    of each active pair in rank order, -1 for an inactive pair and for every
    pair of a row that is not an old row."""
    with torch.no_grad():
        return MarginRank.apply(logits, targets, sigma, known, k, margin)[1]
