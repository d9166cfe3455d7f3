"""fp64 oracle, seeded inputs and allowances for the POD-spatial ops
(cilfw/ops/pod.py, csrc/pod.hip), shared by test_pod.py and test_pod_gpu.py.

Definition, one stage, maps (N, H, W, C): pooled ``v = [r | q]`` stored
(N, H+W, C), ``r[h,c] = sum_w a^2``, ``q[w,c] = sum_h a^2``;
``v^ = v / max(|v|, 1e-12)``; ``d_n = |v^_s - v^_t|``; loss = mean_n d_n;
``u = v^_s - v^_t``, ``g^ = (g/N) u/d``,
``g_v = (g^ - v^_s (v^_s . g^)) / max(|v_s|, 1e-12)``,
``da = 2 a (g_v.r[h,c] + g_v.q[w,c])``.

The oracle works in fp64 from the bf16-rounded inputs. Allowances in the form
of ``_oracle`` (u = 2^-24, c = ``_oracle.C_SUM`` = 2):

* pooled element: ``2 max(H,W) u |ref|`` — every term is >= 0, so the
  running-sum bound is relative (squares of bf16 values are exact in fp32);
* d_n and the stage loss: ``2 n u * 2`` with ``n = max(H,W) + (H+W) C`` —
  the pooling sums followed by the sums over the pooled vector, on unit
  vectors whose difference has norm <= 2;
* da: ``2^-8 |ref| + 2 n u mag / min(d_n, 1)`` — half a bf16 ulp of the
  result plus the fp32 sums, amplified by the division by d; ``mag`` is the
  gradient formula with absolute values in place of every subtraction.

Inputs: ``|randn| + 0.1`` rounded to bf16, student and teacher drawn
independently from one seeded CPU generator — no entry is zero, so a dropped
term always shows. No element and no sample is excluded from a comparison.
"""

import torch

import _oracle

EPS = 1e-12

# (N, H, W, C), each the smallest at which a distinct thing can go wrong
SHAPES = {
    "degenerate": (1, 1, 1, 8),
    "odd_hw": (3, 5, 7, 8),          # H != W, odd sizes
    "many_groups": (2, 4, 4, 512),   # many channel groups on a tiny map
    "c72": (5, 8, 8, 72),            # C no multiple of 64
    "cifar_s1": (2, 32, 32, 16),     # CIFAR stage-1 shape
    "long_ragged": (2, 56, 56, 40),  # long reduction, ragged tiles
}
SHAPE_IDS = list(SHAPES)


def make_maps(name, seed=0):
    """-> (a, b) bf16 CPU maps of SHAPES[name]."""
    shape = SHAPES[name]
    g = torch.Generator().manual_seed(7919 * (SHAPE_IDS.index(name) + 1)
                                      + seed)
    a = (torch.randn(shape, generator=g).abs() + 0.1).to(torch.bfloat16)
    b = (torch.randn(shape, generator=g).abs() + 0.1).to(torch.bfloat16)
    return a, b


def n_sum(H, W, C):
    return float(max(H, W) + (H + W) * C)


def pooled_ref(a):
    """-> fp64 (N, H+W, C), r rows first."""
    sq = a.detach().cpu().double() ** 2
    return torch.cat([sq.sum(dim=2), sq.sum(dim=1)], dim=1)


def stage_ref(a, b, g=1.0):
    """fp64 oracle of one stage -> dict(pooled_s, pooled_t, d (N,), loss,
    da (N,H,W,C), mag (N,H,W,C), n)."""
    a64 = a.detach().cpu().double()
    N, H, W, C = a64.shape
    vs, vt = pooled_ref(a), pooled_ref(b)
    fs, ft = vs.reshape(N, -1), vt.reshape(N, -1)
    ns = fs.norm(dim=1, keepdim=True).clamp_min(EPS)
    nt = ft.norm(dim=1, keepdim=True).clamp_min(EPS)
    sh, th = fs / ns, ft / nt
    u = sh - th
    d = u.norm(dim=1, keepdim=True)
    safe = torch.where(d > 0, d, torch.ones_like(d))
    gh = torch.where(d > 0, (g / N) * u / safe, torch.zeros_like(u))
    gv = (gh - sh * (sh * gh).sum(dim=1, keepdim=True)) / ns
    # the same with |.| in place of every subtraction
    gh_m = torch.where(d > 0, (abs(g) / N) * (sh + th) / safe,
                       torch.zeros_like(u))
    gv_m = (gh_m + sh * (sh * gh_m).sum(dim=1, keepdim=True)) / ns

    def spread(x):
        x = x.reshape(N, H + W, C)
        return x[:, :H, None, :] + x[:, None, H:, :]
    return dict(pooled_s=vs, pooled_t=vt, d=d.reshape(N),
                loss=d.sum() / N, da=2 * a64 * spread(gv),
                mag=2 * a64.abs() * spread(gv_m), n=n_sum(H, W, C))


def worst_pooled(got, a):
    """max err/allowance of a pooled tensor against the oracle."""
    ref = pooled_ref(a)
    _, H, W, _ = a.shape
    assert tuple(got.shape) == tuple(ref.shape), \
        f"pooled shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    return _oracle.worst(got, ref, ref.abs(), float(max(H, W)), False)[0]


def worst_dist(got_d, got_loss, ref):
    """max err/allowance over every d_n and the stage loss."""
    two = torch.full_like(ref["d"], 2.0)
    r_d = _oracle.worst(got_d, ref["d"], two, ref["n"], False)[0]
    r_l = _oracle.worst(got_loss.reshape(1), ref["loss"].reshape(1),
                        two[:1], ref["n"], False)[0]
    return max(r_d, r_l)


def grad_sum_share(got_da, ref):
    """Share of da's summation allowance ``2 n u mag / min(d, 1)`` that the
    error needs once the half bf16 ulp is taken off (``_oracle.needed_c`` /
    c). A correctly rounded bf16 result alone brings ``worst_grad`` close to
    1 (half an ulp is up to 2^-8 |ref|), so the calibration of ``n`` and
    ``mag`` reads this figure, not ``worst_grad``."""
    dmin = ref["d"].clamp(max=1.0).reshape(-1, 1, 1, 1)
    return _oracle.needed_c(got_da, ref["da"], ref["mag"] / dmin, ref["n"],
                            True) / _oracle.C_SUM


def worst_grad(got_da, ref, scale=1.0):
    """max err/allowance of da; ``scale``: the upstream factor the oracle
    (computed for upstream 1) is multiplied by."""
    dmin = ref["d"].clamp(max=1.0).reshape(-1, 1, 1, 1)
    return _oracle.worst(got_da, ref["da"] * scale,
                         ref["mag"] * abs(scale) / dmin, ref["n"], True)[0]
