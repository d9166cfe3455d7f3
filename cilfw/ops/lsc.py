"""PODNet's local similarity classifier (LSC: several proxies per class on a
cosine head) and the NCA loss it is trained with (Douillard et al., ECCV
2020, eq. 8-10).

Definitions (shared by csrc/lsc.hip, the CPU path below and the tests).

``lsc_reduce(sims, sigma, nb_proxy, gamma=1.0) -> logits``

* ``sims (M, C K)`` are pure cosines (``cosine_linear`` at scale 1); class
  ``c``'s proxies sit at columns ``c K .. c K + K - 1``. ``K = nb_proxy`` is a
  host int in 1..16, ``gamma`` a host float ``>= 0``, ``sigma`` a 1-element
  tensor on the device of ``sims`` (fp32 on a GPU, where the kernels read
  it).
* Per row and class: ``a_k = softmax_k(gamma s_{c,k})``, computed
  max-subtracted in fp32 (fp64 for fp64 input); ``yhat_c = sum_k a_k
  s_{c,k}``; ``logits[m, c] = sigma yhat_c``, in the dtype of ``sims``.
* Backward for upstream ``g (M, C)``: ``dsims[m, c, k] = sigma g_c a_k (1 +
  gamma (s_k - yhat_c))``; ``dsigma = sum_{m,c} g_{mc} yhat_{mc}``.
* ``K = 1`` gives ``logits = sigma sims``.

``nca_loss(logits, targets, sigma, margin=0.6) -> 0-d loss``

* ``logits (M, C)`` with ``C >= 2``, ``targets (M,)`` int64, ``sigma`` as
  above, ``margin`` a host float ``>= 0``.
* A row whose target lies outside ``0..C-1`` is skipped: nothing is read at
  its target column, it contributes 0 (``h_m = 0``, not active), its
  gradient row is exactly 0, and ``M`` stays the divisor.
* Otherwise, with ``y = targets[m]``: ``sm = fp32(sigma margin)`` rounded on
  its own; ``mx = max_{i != y} l_i``; ``lse = mx + log sum_{i != y} exp(l_i -
  mx)`` (the positive is excluded from the denominator, eq. 10);
  ``h_m = lse - (l_y - sm)``; the row is *active* iff ``h_m > 0``;
  ``loss = (1/M) sum_m max(h_m, 0)``.
* Gradients for upstream ``g``: ``dlogits[m, i] = (g/M) exp(l_i - lse)`` for
  ``i != y`` of an active row, ``dlogits[m, y] = -g/M``; the whole row of an
  inactive or skipped row is exactly 0; ``dsigma = (g/M) margin A`` with
  ``A`` the number of active rows, the explicit dependence through ``sm``. It
  is returned, never dropped. ``targets`` and ``margin`` get no gradient.
* For ``sigma <= 0`` nothing special happens: ``sm <= 0`` and every result
  is finite.

``nca_rows(logits, targets, sigma, margin) -> (h (M,) fp32, active (M,)
int32)`` without autograd.

On a GPU the inputs must be bf16 and the HIP kernels are the only path (no
ATen fallback): no allocation depends on the data, nothing is read on the
host, so both ops sit inside a captured step and replay with the current
``sigma``, ``targets`` and upstream (docs/kernels.md, "LSC / NCA"). CPU
tensors use the torch implementation below, in fp64 for fp64 input.
"""

import torch

from ._backend import use_hip, ext

MAX_PROXY = 16


def _sigma_f32(sigma, name):
    sg = sigma.detach()
    assert sg.dtype == torch.float32, \
        f"{name}: sigma is a 1-element fp32 tensor on the device of the " \
        f"input (the kernels read it there)"
    return sg.reshape(1)


# ------------------------------------------------------------------ lsc_reduce

def _check_lsc(sims, sigma, nb_proxy, gamma):
    assert sims.dim() == 2, "lsc_reduce: sims are (M, C * nb_proxy)"
    K, gamma = int(nb_proxy), float(gamma)
    assert 1 <= K <= MAX_PROXY, \
        f"lsc_reduce: nb_proxy must be in 1..{MAX_PROXY} (got {K})"
    M, CK = sims.shape
    assert M >= 1 and CK >= 1 and CK % K == 0, \
        f"lsc_reduce: sims (M, C * nb_proxy) need M >= 1 and a column " \
        f"count that is a multiple of nb_proxy = {K} (got {M} x {CK})"
    assert gamma >= 0.0, f"lsc_reduce: gamma must be >= 0 (got {gamma})"
    assert sigma.numel() == 1 and sigma.device == sims.device, \
        "lsc_reduce: sigma is a 1-element tensor on the device of the sims"
    return K, gamma


def _lsc_torch(s3, gamma):
    """``s3 (M, C, K)`` fp32 or fp64 -> (a (M, C, K), yhat (M, C))."""
    x = gamma * s3
    e = torch.exp(x - x.amax(dim=2, keepdim=True))
    a = e / e.sum(dim=2, keepdim=True)
    return a, (a * s3).sum(dim=2)


class LscReduce(torch.autograd.Function):
    """``sigma sum_k softmax_k(gamma s_k) s_k`` per class. HIP: saves the
    sims and yhat; the backward recomputes the softmax weights."""

    @staticmethod
    def forward(ctx, sims, sigma, nb_proxy, gamma):
        K, gamma = _check_lsc(sims, sigma, nb_proxy, gamma)
        ctx.sigma_shape, ctx.sigma_dtype = sigma.shape, sigma.dtype
        ctx.args = (K, gamma)
        sims = sims.detach().contiguous()
        ctx.hip = use_hip(sims)
        if ctx.hip:
            e = ext()
            e._bf16(sims, "lsc_reduce.sims")
            sg = _sigma_f32(sigma, "lsc_reduce")
            logits, yhat = e.lsc_reduce_fwd(sims, sg, K, gamma)
            ctx.save_for_backward(sims, yhat, sg)
            return logits
        assert sims.dtype in (torch.float32, torch.float64), \
            f"lsc_reduce: CPU sims are fp32 or fp64 (got {sims.dtype})"
        M, CK = sims.shape
        sg = sigma.detach().to(sims.dtype).reshape(())
        s3 = sims.reshape(M, CK // K, K)
        a, yhat = _lsc_torch(s3, gamma)
        ctx.save_for_backward(s3, a, yhat, sg)
        return sg * yhat

    @staticmethod
    def backward(ctx, g):
        K, gamma = ctx.args
        if ctx.hip:
            e = ext()
            sims, yhat, sg = ctx.saved_tensors
            dsims, rows = e.lsc_reduce_bwd(sims, yhat, g.contiguous(), sg, K,
                                           gamma)
            return dsims, e.cos_sum(rows).reshape(ctx.sigma_shape), None, None
        s3, a, yhat, sg = ctx.saved_tensors
        g = g.to(s3.dtype)
        ds = (sg * g)[:, :, None] * a * (1.0 + gamma * (s3 - yhat[:, :, None]))
        dsig = (g * yhat).sum(dim=1).sum()
        return ds.reshape(s3.shape[0], -1), \
            dsig.reshape(ctx.sigma_shape).to(ctx.sigma_dtype), None, None


def lsc_reduce(sims, sigma, nb_proxy, gamma=1.0):
    """The K proxies of each class reduced to one logit (module docstring):
    ``sims (M, C * nb_proxy)`` -> ``(M, C)`` in the dtype of ``sims``."""
    return LscReduce.apply(sims, sigma, nb_proxy, gamma)


# -------------------------------------------------------------------- nca_loss

def _check_nca(logits, targets, sigma, margin):
    assert logits.dim() == 2, "nca_loss: logits are (M, C)"
    M, C = logits.shape
    margin = float(margin)
    assert M >= 1 and C >= 2, \
        f"nca_loss: needs M >= 1 rows and C >= 2 classes (got {M} x {C})"
    assert margin >= 0.0, f"nca_loss: margin must be >= 0 (got {margin})"
    assert targets.shape == (M,) and targets.dtype == torch.int64 \
        and targets.device == logits.device, \
        "nca_loss: targets are an int64 (M,) tensor on the device of the " \
        "logits"
    assert sigma.numel() == 1 and sigma.device == logits.device, \
        "nca_loss: sigma is a 1-element tensor on the device of the logits"
    return margin


def _nca_torch(L, t, sg, margin):
    """The definition in the dtype of ``L`` (fp32 or fp64), ``sg`` 0-d in
    that dtype. -> (loss, h (M,), active bool (M,), dlogits and dsigma for
    upstream 1)."""
    M, C = L.shape
    zero = torch.zeros((), dtype=L.dtype, device=L.device)
    valid = (t >= 0) & (t < C)
    y = t.clamp(0, C - 1)[:, None]
    pos = torch.zeros(M, C, dtype=torch.bool, device=L.device).scatter_(
        1, y, True)
    neg = L.masked_fill(pos, float("-inf"))
    mx = neg.amax(dim=1, keepdim=True)
    lse = mx + torch.log(torch.exp(neg - mx).sum(dim=1, keepdim=True))
    h = lse - (L.gather(1, y) - sg * margin)
    h = torch.where(valid[:, None], h, zero)
    active = h > 0
    loss = torch.where(active, h, zero).sum() / M
    dl = torch.exp(neg - lse).masked_fill(pos, -1.0) / M
    dl = torch.where(active, dl, zero)
    dsig = margin * active.sum().to(L.dtype) / M
    return loss, h[:, 0], active[:, 0], dl, dsig


class NcaLoss(torch.autograd.Function):
    """``(1/M) sum_m max(h_m, 0)``. HIP: saves the logits, the per-row
    log-sum-exp and active flags and the scalars of nca_finalize; the
    backward reads them and the upstream on the device."""

    @staticmethod
    def forward(ctx, logits, targets, sigma, margin):
        margin = _check_nca(logits, targets, sigma, margin)
        ctx.sigma_shape, ctx.sigma_dtype = sigma.shape, sigma.dtype
        logits = logits.detach().contiguous()
        targets = targets.contiguous()
        ctx.hip = use_hip(logits)
        if ctx.hip:
            e = ext()
            e._bf16(logits, "nca_loss.logits")
            sg = _sigma_f32(sigma, "nca_loss")
            loss, h, active, lse, fin, _ = e.nca_fwd(logits, targets, sg,
                                                     margin)
            ctx.save_for_backward(logits, targets, lse, active, fin)
            ctx.mark_non_differentiable(h, active)
            return loss, h, active
        assert logits.dtype in (torch.float32, torch.float64), \
            f"nca_loss: CPU logits are fp32 or fp64 (got {logits.dtype})"
        sg = sigma.detach().to(logits.dtype).reshape(())
        loss, h, active, dl, dsig = _nca_torch(logits, targets, sg, margin)
        h, active = h.float(), active.to(torch.int32)
        ctx.save_for_backward(dl, dsig)
        ctx.mark_non_differentiable(h, active)
        return loss, h, active

    @staticmethod
    def backward(ctx, dloss, _dh, _dactive):
        if ctx.hip:
            logits, targets, lse, active, fin = ctx.saved_tensors
            up = dloss.detach().float().reshape(1).contiguous()
            dl, dsig = ext().nca_bwd(logits, targets, lse, active, fin, up)
            return dl, None, dsig.reshape(ctx.sigma_shape), None
        dl, dsig = ctx.saved_tensors
        g = dloss.to(dl.dtype)
        return dl * g, None, \
            (dsig * g).reshape(ctx.sigma_shape).to(ctx.sigma_dtype), None


def nca_loss(logits, targets, sigma, margin=0.6):
    """PODNet's NCA loss (module docstring) -> 0-d loss."""
    return NcaLoss.apply(logits, targets, sigma, margin)[0]


def nca_rows(logits, targets, sigma, margin=0.6):
    """Per-row ``h (M,)`` fp32 and ``active (M,)`` int32 (no autograd): 0 and
    not active for a skipped row."""
    with torch.no_grad():
        return NcaLoss.apply(logits, targets, sigma, margin)[1:]
