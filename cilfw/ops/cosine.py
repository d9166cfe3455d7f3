"""Cosine-normalised classifier head (LUCIR, Hou et al., CVPR 2019; PODNet's
LSC head with one proxy per class) and the distillation of the final
embedding that both papers pair with it ("less-forget" / POD-flat).

Definitions (shared by csrc/cosine.hip, the CPU path below and the tests).

* Inverse norm of a row ``x``: ``r(x) = 1/|x|_2`` if ``|x|_2 > 0``, else 0: a
  zero row gives a zero unit vector and an exactly zero gradient.
* ``cosine_linear(x, w, sigma)``: features ``x (M, D)``, class weights
  ``w (C, D)`` (the fp32 masters), one scalar ``sigma``:
  ``logits[m, c] = sigma (x_m . w_c) r(x_m) r(w_c)``, in the dtype of ``x``.
  With ``g = dlogits``, ``x^ = x r(x)``, ``w^ = w r(w)``, ``z = x^ w^T``:
  ``dsigma = sum g z``;
  ``dx_m = sigma r(x_m) (G_m - x^_m (x^_m . G_m))``, ``G = g w^``;
  ``dw_c = sigma r(w_c) (H_c - w^_c (w^_c . H_c))``, ``H = g^T x^``.
* ``flat_loss(s, t)``: ``u_m = s^_m - t^_m``, ``l_m = |u_m|^2 / 2`` (``1 -
  cos`` for non-zero rows), ``loss = mean_m l_m``; gradient to the student
  only: ``ds_m = (g/M) r(s_m) (u_m - s^_m (s^_m . u_m))``.

On a GPU the features must be bf16 and the HIP kernels are the only path (no
ATen fallback): ``sigma`` folds into the normalised features, the ``(M, C)``
products run on the head GEMMs of csrc/gemm.hip, and ``sigma`` and the
upstream scalar are read from device memory by the kernels, so a captured
step replays with their current values (docs/kernels.md, "Cosine head /
flat"). CPU tensors use the torch implementation of the same definitions, in
fp64 when the features are fp64.
"""

import torch

from ._backend import use_hip, ext


def _acc_dtype(x):
    return torch.float64 if x.dtype == torch.float64 else torch.float32


def _rinv(x):
    n = x.norm(dim=1, keepdim=True)
    return torch.where(n > 0, 1.0 / torch.where(n > 0, n, torch.ones_like(n)),
                       torch.zeros_like(n))


def _check_feats(x, name):
    assert x.dim() == 2, f"{name}: features are (M, D)"


def _w_f32(w):
    """The fp32 masters as one contiguous, 16-byte aligned matrix."""
    assert w.dtype == torch.float32, \
        f"cosine_linear: class weights are the fp32 masters (got {w.dtype})"
    w = w.contiguous()
    return w if w.data_ptr() % 16 == 0 else w.clone()


def _sigma_dev(sigma, ref):
    s = sigma.detach()
    assert s.numel() == 1, "cosine_linear: sigma is one scalar"
    assert s.dtype == torch.float32 and s.device == ref.device, \
        "cosine_linear: sigma is a 1-element fp32 tensor on the device of " \
        "the features (the kernels read it there)"
    return s.reshape(1)


class CosineLinear(torch.autograd.Function):
    """``sigma cos(x_m, w_c)``. HIP: saves the rows, their inverse norms and
    the two normalised bf16 GEMM operands."""

    @staticmethod
    def forward(ctx, x, w, sigma):
        _check_feats(x, "cosine_linear")
        assert w.dim() == 2 and w.shape[1] == x.shape[1], \
            f"cosine_linear: features {tuple(x.shape)} vs class weights " \
            f"{tuple(w.shape)}"
        assert w.device == x.device and sigma.numel() == 1
        ctx.sigma_shape = sigma.shape
        x = x.contiguous()
        if use_hip(x):
            e = ext()
            e._bf16(x, "cosine_linear.x")
            wf, sg = _w_f32(w.detach()), _sigma_dev(sigma, x)
            xs, rx = e.rownorm_fwd(x, sg)
            wn, rw = e.rownorm_fwd(wf)
            ctx.save_for_backward(x, wf, sg, rx, rw, xs, wn)
            return e.linear_fwd(xs, wn, None)
        acc = _acc_dtype(x)
        xa, wa, sa = x.to(acc), w.detach().to(acc), sigma.detach().to(acc)
        rx, rw = _rinv(xa), _rinv(wa)
        ctx.save_for_backward(xa, wa, sa, rx, rw)
        ctx.dtypes = (x.dtype, w.dtype, sigma.dtype)
        return (sa.reshape(()) * ((xa * rx) @ (wa * rw).t())).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        if use_hip(g):
            e = ext()
            x, wf, sg, rx, rw, xs, wn = ctx.saved_tensors
            # G = g w^ (bf16) and sigma H = g^T (sigma x^) (fp32)
            G, sH, _ = e.linear_bwd(g, xs, wn, False)
            dx, dsr = e.rownorm_bwd(x, rx, G, sg, want_dsig=True)
            dw, _ = e.rownorm_bwd(wf, rw, sH)
            return dx, dw, e.cos_sum(dsr).reshape(ctx.sigma_shape)
        xa, wa, sa, rx, rw = ctx.saved_tensors
        dt_x, dt_w, dt_s = ctx.dtypes
        ga = g.to(xa.dtype)
        xh, wh, s = xa * rx, wa * rw, sa.reshape(())
        G, H = ga @ wh, ga.t() @ xh
        dsig = (xh * G).sum()
        dx = s * rx * (G - xh * (xh * G).sum(dim=1, keepdim=True))
        dw = s * rw * (H - wh * (wh * H).sum(dim=1, keepdim=True))
        return dx.to(dt_x), dw.to(dt_w), \
            dsig.reshape(ctx.sigma_shape).to(dt_s)


def cosine_linear(x, w, sigma):
    """Cosine logits ``sigma cos(x_m, w_c)``: features ``x (M, D)``, class
    weights ``w (C, D)``, scalar ``sigma`` (1 element). -> (M, C) in the
    dtype of ``x``."""
    return CosineLinear.apply(x, w, sigma)


@torch.no_grad()
def cosine_normalize_weights(w):
    """Unit rows of ``w (C, D)`` as the GEMM operand a frozen head caches:
    bf16 on a GPU (one rownorm_fwd), the dtype of ``w`` on the CPU."""
    if use_hip(w):
        return ext().rownorm_fwd(_w_f32(w.detach().float()))[0]
    wa = w.detach().to(_acc_dtype(w))
    return (wa * _rinv(wa)).to(w.dtype)


@torch.no_grad()
def cosine_linear_frozen(x, wn, sigma):
    """Cosine logits against rows already normalised by
    ``cosine_normalize_weights`` (a frozen teacher's head): one rownorm_fwd
    on the features plus the GEMM. No autograd."""
    _check_feats(x, "cosine_linear_frozen")
    x = x.contiguous()
    if use_hip(x):
        e = ext()
        e._bf16(x, "cosine_linear_frozen.x")
        return e.linear_fwd(e.rownorm_fwd(x, _sigma_dev(sigma, x))[0], wn,
                            None)
    acc = _acc_dtype(x)
    xa = x.to(acc)
    return (sigma.to(acc).reshape(()) * ((xa * _rinv(xa)) @ wn.to(acc).t())
            ).to(x.dtype)


def _flat_torch(s, t):
    """-> (loss, l (M,), gs (M, D) for upstream 1), in the dtype of s, t."""
    M = s.shape[0]
    rs = _rinv(s)
    # s r(s) and t r(t) are each rounded on their own: equal rows give u == 0
    sh = s * rs
    u = sh - t * _rinv(t)
    l = 0.5 * (u * u).sum(dim=1)
    gs = rs * (u - sh * (sh * u).sum(dim=1, keepdim=True)) / M
    return l.sum() / M, l, gs


def _check_pair(s, t):
    _check_feats(s, "flat_loss")
    assert s.shape == t.shape, \
        f"flat_loss: student features {tuple(s.shape)} vs teacher " \
        f"{tuple(t.shape)}"
    assert s.device == t.device


class FlatDistill(torch.autograd.Function):
    """``mean_m |s^_m - t^_m|^2 / 2``. Saves the gradient for upstream 1; the
    teacher gets no gradient."""

    @staticmethod
    def forward(ctx, s, t):
        _check_pair(s, t)
        s, t = s.contiguous(), t.detach().contiguous()
        if use_hip(s):
            loss, _l, gs = ext().flat_dist(s, t)
        else:
            assert s.dtype == t.dtype
            acc = _acc_dtype(s)
            loss, _l, gs = _flat_torch(s.to(acc), t.to(acc))
        ctx.save_for_backward(gs)
        ctx.s_dtype = s.dtype
        return loss

    @staticmethod
    def backward(ctx, dloss):
        gs, = ctx.saved_tensors
        if use_hip(gs):
            up = dloss.detach().float().reshape(1).contiguous()
            return ext().flat_bwd(gs, up), None
        return (gs * dloss.to(gs.dtype)).to(ctx.s_dtype), None


def flat_loss(feat_s, feat_t):
    """Embedding distillation: student features ``feat_s``, teacher features
    ``feat_t`` (no gradient), both (M, D). -> 0-d loss."""
    return FlatDistill.apply(feat_s, feat_t)


def flat_dist(feat_s, feat_t):
    """Per-row ``l_m = |s^_m - t^_m|^2 / 2`` (M,) (no autograd)."""
    _check_pair(feat_s, feat_t)
    s, t = feat_s.detach().contiguous(), feat_t.detach().contiguous()
    if use_hip(s):
        return ext().flat_dist(s, t)[1]
    assert s.dtype == t.dtype
    acc = _acc_dtype(s)
    return _flat_torch(s.to(acc), t.to(acc))[1]
