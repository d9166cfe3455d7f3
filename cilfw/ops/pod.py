"""Pooled-outputs distillation — PODNet's POD-spatial loss (Douillard et al.,
ECCV 2020) over the backbone's stage outputs.

Definition (shared by csrc/pod.hip, the CPU path below and the tests). For
one stage, student map ``a`` and teacher map ``b``, both ``(N, H, W, C)``:

* pooled vector of sample n, ``v(a)_n`` of length ``(H+W) C``, stored as
  ``(N, H+W, C)`` fp32, the r rows first:
  ``r[h, c] = sum_w a[n, h, w, c]^2``, then ``q[w, c] = sum_h a[n, h, w, c]^2``;
* ``v^ = v / max(|v|_2, 1e-12)``, ``d_n = |v^(a)_n - v^(b)_n|_2``,
  stage loss ``= (1/N) sum_n d_n``;
* ``pod_loss`` is the mean of the stage losses over the stages.

Gradient of a stage loss with upstream scalar g — student only:
``u = v^_s - v^_t``; ``g^ = (g/N) u / d`` (exactly 0 when ``d == 0``);
``g_v = (g^ - v^_s (v^_s . g^)) / max(|v_s|, 1e-12)``;
``da[n, h, w, c] = 2 a[n, h, w, c] (g_v.r[h, c] + g_v.q[w, c])`` in the dtype
of ``a``.

The maps are whatever the backbones' ``return_maps`` gives: by default the
post-ReLU stage outputs (their last ReLU is fused into
``batchnorm_add_relu``); with ``pod_tap="pre"`` (``--pod_tap pre``) the paper's
tap, each stage's sum before its last ReLU (``ops.add_relu_tap``). Nothing
here assumes a sign: the pooled terms are squares.

On a GPU the maps must be bf16 and the fused HIP kernels are the only path
(no ATen fallback); CPU tensors use the torch implementation of the same
definition.
"""

import torch

from ._backend import use_hip, ext

EPS = 1e-12


def _acc_dtype(a):
    return torch.float64 if a.dtype == torch.float64 else torch.float32


def _check_maps(a, b=None):
    assert a.dim() == 4, "pod: maps are (N, H, W, C)"
    if b is not None:
        assert a.shape == b.shape, \
            f"pod: student map {tuple(a.shape)} vs teacher {tuple(b.shape)}"
        assert a.device == b.device


def _pool_torch(a):
    sq = a.to(_acc_dtype(a)) ** 2
    return torch.cat([sq.sum(dim=2), sq.sum(dim=1)], dim=1)


def _dist_torch(vs, vt):
    """-> (loss, d (N,), g_v (N, H+W, C) for upstream 1)."""
    N = vs.shape[0]
    fs, ft = vs.reshape(N, -1), vt.reshape(N, -1)
    ns = fs.norm(dim=1, keepdim=True).clamp_min(EPS)
    nt = ft.norm(dim=1, keepdim=True).clamp_min(EPS)
    sh = fs / ns
    u = sh - ft / nt
    d = u.norm(dim=1, keepdim=True)
    safe = torch.where(d > 0, d, torch.ones_like(d))
    gh = torch.where(d > 0, u / (safe * N), torch.zeros_like(u))
    gv = (gh - sh * (sh * gh).sum(dim=1, keepdim=True)) / ns
    return d.sum() / N, d.reshape(N), gv.reshape(vs.shape)


def _bwd_torch(a, gv, up):
    H = a.shape[1]
    t = gv[:, :H, None, :] + gv[:, None, H:, :]
    return (2 * a.to(gv.dtype) * t * up.to(gv.dtype)).to(a.dtype)


def pod_pool(a):
    """(N, H, W, C) -> (N, H+W, C) fp32 pooled sums of squares (fp64 for an
    fp64 CPU map), r rows first."""
    _check_maps(a)
    a = a.detach().contiguous()
    if use_hip(a):
        return ext().pod_pool(a)
    return _pool_torch(a)


class PodSpatial(torch.autograd.Function):
    """Stage loss of one (student, teacher) map pair. Saves ``a`` and
    ``g_v``; the teacher gets no gradient."""

    @staticmethod
    def forward(ctx, a, b):
        _check_maps(a, b)
        a, b = a.contiguous(), b.detach().contiguous()
        if use_hip(a):
            e = ext()
            loss, _dist, gv = e.pod_dist(e.pod_pool(a), e.pod_pool(b))
        else:
            assert a.dtype == b.dtype
            loss, _dist, gv = _dist_torch(_pool_torch(a), _pool_torch(b))
        ctx.save_for_backward(a, gv)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        a, gv = ctx.saved_tensors
        if use_hip(a):
            up = dloss.detach().float().reshape(1).contiguous()
            return ext().pod_bwd(a, gv, up), None
        return _bwd_torch(a, gv, dloss), None


def pod_spatial(a, b):
    """POD-spatial loss of one stage: student map ``a``, teacher map ``b``
    (no gradient), both (N, H, W, C). -> 0-d loss."""
    return PodSpatial.apply(a, b)


def pod_dist(a, b):
    """Per-sample distances ``d_n`` (N,) of one stage (no autograd)."""
    _check_maps(a, b)
    a, b = a.detach().contiguous(), b.detach().contiguous()
    if use_hip(a):
        e = ext()
        return e.pod_dist(e.pod_pool(a), e.pod_pool(b))[1]
    return _dist_torch(_pool_torch(a), _pool_torch(b))[1]


def pod_loss(maps_s, maps_t):
    """Mean over the stages of the POD-spatial stage losses."""
    assert len(maps_s) == len(maps_t) and len(maps_s) > 0, \
        f"pod_loss: {len(maps_s)} student maps vs {len(maps_t)} teacher maps"
    total = pod_spatial(maps_s[0], maps_t[0])
    for a, b in zip(maps_s[1:], maps_t[1:]):
        total = total + pod_spatial(a, b)
    return total / len(maps_s)
