"""Conv kernels on the routes the default training step really takes, each
compared element by element with the fp64 oracle of ``tests/_oracle.py``
(run on MI355X: pytest -m gpu).

Every test first asserts the route its shape was chosen for (the launchers in
csrc/conv.hip branch on the same predicates), so retuning a threshold makes
the test fail loudly instead of quietly testing another kernel.
"""

import os
import subprocess
import sys
import textwrap

import pytest
import torch

import _oracle as O
import cilfw.ops.functional as CF

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(),
                                 reason="needs GPU")]

U = O.U_F32


def _H():
    from cilfw import _hip_ops
    return _hip_ops


def _xw(N, H, W, C, K, k, seed):
    gen = torch.Generator().manual_seed(seed)
    return O.signed_unit((N, H, W, C), gen), O.signed_unit((k, k, C, K), gen)


def _dy(x, k, stride, pad, K, seed):
    N, H, W, _ = x.shape
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    return O.signed_unit((N, Ho, Wo, K), torch.Generator().manual_seed(seed))


# ------------------------------------------------- forward 128-wide N tile

@pytest.mark.parametrize("N,hw,C,K,ks", [
    (17, 31, 64, 256, 1),   # M = 16337: ragged last M block
    (9, 30, 512, 128, 4),   # M = 8100: slab reduce on the 128-wide tile
])
def test_fwd_bn128_tile_1x1(N, hw, C, K, ks):
    H = _H()
    assert H.conv2d_fwd_route(N, hw, hw, C, K, 1, 1, 1, 0) == ("v2_bn128", ks)
    x, w = _xw(N, hw, hw, C, K, 1, seed=11)
    dy = _dy(x, 1, 1, 0, K, seed=12)
    xg = x.cuda().requires_grad_()
    wg = w.float().cuda().requires_grad_()
    y = CF.conv2d(xg, wg, 1, 0)
    ref, mag, n = O.conv_fwd_ref(x, w, 1, 0)
    O.check(y, ref, mag, n + (ks if ks > 1 else 0), True, "fwd bn128")
    y.backward(dy.cuda())
    _, dks = H.conv2d_bwd_data_route(N, hw, hw, C, K, 1, 1, 1)
    ref, mag, n = O.conv_dx_ref(dy, w, 1, 0, hw, hw)
    O.check(xg.grad, ref, mag, n + (dks if dks > 1 else 0), True, "dx")
    route, ns = H.conv2d_bwd_weight_route(N, C, K, 1, 1, hw, hw)
    assert route == "v2"
    ref, mag, n = O.conv_dw_ref(dy, x, 1, 0, 1, 1)
    O.check(wg.grad, ref, mag, n + ns, False, "dW")


# ------------------------------------------------ BN-statistics epilogue

BN_PARTS_SHAPES = [
    # N, H, W, C, K, k, stride, pad, route
    (3, 7, 7, 16, 24, 3, 1, 1, "v2_bn64"),     # M=147: 19-row block; K tail
    (5, 9, 9, 24, 72, 3, 2, 1, "v2_bn64"),     # M=125 ragged; 2 col tiles
    (2, 11, 11, 64, 136, 1, 1, 0, "v2_bn64"),  # K tail after 2 full tiles
    (17, 31, 31, 64, 256, 1, 1, 0, "v2_bn128"),  # 128-wide tile's epilogue
    (64, 32, 32, 64, 64, 3, 1, 1, "v2_bn64"),  # ksplit=1 through a full grid
]


def _bn_ref(y64, gamma, beta, rm0, rv0, momentum, eps, relu):
    """fp64 training BN over rows of y64 (M, K) + first-order error budgets
    for fp32 sum / sum-of-squares statistics."""
    M = y64.shape[0]
    mu = y64.mean(0)
    q = (y64 * y64).mean(0)
    var = (q - mu * mu).clamp_min(0)
    inv = torch.rsqrt(var + eps)
    d_mu = (M + 2) * U * y64.abs().mean(0)
    d_var = (M + 4) * U * (q + mu * mu) + 2 * mu.abs() * d_mu
    d_inv = inv * (0.5 * d_var / (var + eps) + 4 * U)
    unb = var * M / max(M - 1, 1)
    rm = (1 - momentum) * rm0 + momentum * mu
    rv = (1 - momentum) * rv0 + momentum * unb
    d_rm = momentum * d_mu + 4 * U * (rm0.abs() + mu.abs())
    d_rv = momentum * d_var * M / max(M - 1, 1) + 4 * U * (rv0.abs() + unb)
    out = (y64 - mu) * inv * gamma + beta
    sc = (inv * gamma).abs()
    d_out = ((y64 - mu).abs() * gamma.abs() * d_inv + sc * d_mu
             + 4 * U * (y64.abs() * sc + mu.abs() * sc + beta.abs()))
    if relu:
        out = out.clamp_min(0)
    return dict(mean=(mu, d_mu), invstd=(inv, d_inv), rm=(rm, d_rm),
                rv=(rv, d_rv), out=(out, d_out + O.HALF_ULP_BF16 * out.abs()))


def _within(got, ref_tol, what):
    ref, tol = ref_tol
    err = (got.detach().double().cpu().reshape(ref.shape) - ref).abs()
    r = (err / tol.clamp_min(1e-300)).max().item()
    print(f"{what}: max err/tol = {r:.4f}")
    assert r <= 1.0, f"{what}: err/tol {r:.3g}"


@pytest.mark.parametrize("N,H,W,C,K,k,st,pd,route", BN_PARTS_SHAPES)
def test_conv_fwd_bn_stats_epilogue(N, H, W, C, K, k, st, pd, route):
    Hop = _H()
    assert Hop.conv2d_fwd_route(N, H, W, C, K, k, k, st, pd) == (route, 1)
    x, w = _xw(N, H, W, C, K, k, seed=21)
    y, parts = Hop.conv2d_fwd(x.cuda(), w.cuda(), st, pd, want_bn_parts=True)
    assert parts is not None, "BN-statistics epilogue did not engage"
    ref, mag, n = O.conv_fwd_ref(x, w, st, pd)
    O.check(y, ref, mag, n, True, "fwd (bn_parts launch)")
    y_plain, none = Hop.conv2d_fwd(x.cuda(), w.cuda(), st, pd)
    assert none is None and torch.equal(y_plain, y), \
        "y changed under the BN epilogue"

    # the kernel sums the bf16-rounded stored y: independent of conv accuracy
    M = y.numel() // K
    gy = parts.shape[0]
    assert parts.shape == (gy, 2, K)
    y64 = y.double().cpu().view(M, K)
    got = parts.double().cpu().sum(0)
    _within(got[0], (y64.sum(0), M * U * y64.abs().sum(0)), "parts sum")
    _within(got[1], ((y64 * y64).sum(0), M * U * (y64 * y64).sum(0)),
            "parts sumsq")

    gen = torch.Generator().manual_seed(22)
    gamma = (torch.rand(K, generator=gen) + 0.5)
    beta = torch.randn(K, generator=gen)
    rm0 = torch.randn(K, generator=gen) * 0.1
    rv0 = torch.rand(K, generator=gen) + 0.5
    want = _bn_ref(y64, gamma.double(), beta.double(), rm0.double(),
                   rv0.double(), 0.1, 1e-5, True)
    for tag, kw in (("ext_parts", dict(ext_parts=parts)),
                    ("own sums", {})):
        rm, rv = rm0.clone().cuda(), rv0.clone().cuda()
        out, mean, invstd = Hop.bn_fwd(y, gamma.cuda(), beta.cuda(), rm, rv,
                                       0.1, 1e-5, True, True, **kw)
        _within(mean, want["mean"], f"{tag} mean")
        _within(invstd, want["invstd"], f"{tag} invstd")
        _within(rm, want["rm"], f"{tag} running_mean")
        _within(rv, want["rv"], f"{tag} running_var")
        _within(out.view(M, K), want["out"], f"{tag} bn output")


def test_conv_fwd_bn_stats_declined_under_split_k():
    """ksplit > 1 writes fp32 slabs, so no epilogue: parts must be None and
    y still correct."""
    Hop = _H()
    N, H, W, C, K, k, st, pd = 4, 6, 6, 128, 72, 3, 1, 1
    route, ks = Hop.conv2d_fwd_route(N, H, W, C, K, k, k, st, pd)
    assert route == "v2_bn64" and ks > 1
    x, w = _xw(N, H, W, C, K, k, seed=23)
    y, parts = Hop.conv2d_fwd(x.cuda(), w.cuda(), st, pd, want_bn_parts=True)
    assert parts is None
    ref, mag, n = O.conv_fwd_ref(x, w, st, pd)
    O.check(y, ref, mag, n + ks, True, "fwd split-K")


# ------------------------------------------------------------ bwd-data

def _bwd_data_nan_prefilled(Hop, dy, w, stride, pad, H, W):
    """conv2d_bwd_data with its ``torch.empty`` dx pre-filled with NaN, so an
    input position that no block (or parity class) writes stays NaN."""
    real_empty = torch.empty

    def nan_empty(*a, **kw):
        t = real_empty(*a, **kw)
        return t.fill_(float("nan")) if t.is_floating_point() else t
    Hop.torch.empty = nan_empty
    try:
        return Hop.conv2d_bwd_data(dy, w, stride, pad, H, W)
    finally:
        Hop.torch.empty = real_empty


def _check_bwd_data(Hop, N, H, W, C, K, k, st, pd, route, seed):
    got_route, ks = Hop.conv2d_bwd_data_route(N, H, W, C, K, k, k, st)
    assert got_route == route, f"routes to {got_route}, wanted {route}"
    x, w = _xw(N, H, W, C, K, k, seed=seed)
    dy = _dy(x, k, st, pd, K, seed=seed + 1)
    dx = _bwd_data_nan_prefilled(Hop, dy.cuda(), w.cuda(), st, pd, H, W)
    ref, mag, n = O.conv_dx_ref(dy, w, st, pd, H, W)
    slabs = ks if (ks > 1 and route != "s2_fused") else 0
    O.check(dx, ref, mag, n + slabs, True,
            f"dx {route} {N}x{H}x{W}x{C}<-{K} k{k}s{st}")


@pytest.mark.parametrize("N,hw,C,K,k", [
    (32, 31, 128, 32, 3),   # odd size: the 4 parity classes differ in extent
    (32, 32, 128, 16, 3),
    (22, 31, 136, 16, 3),   # C tail
    (32, 31, 128, 16, 5),   # any R*S > 1 routes here
])
def test_bwd_data_s2_fused(N, hw, C, K, k):
    _check_bwd_data(_H(), N, hw, hw, C, K, k, 2, k // 2, "s2_fused", seed=31)


@pytest.mark.parametrize("N,hw,C,K,k,st", [
    (3, 224, 16, 16, 3, 1),
    (13, 108, 24, 40, 3, 1),   # ragged M, C tail, K % 16 != 0
    (13, 110, 32, 24, 3, 2),   # K % 16 != 0 keeps it off the fused route
    (13, 108, 64, 64, 1, 1),
])
def test_bwd_data_v2_at_real_threshold(N, hw, C, K, k, st):
    assert N * hw * hw >= 150000
    _check_bwd_data(_H(), N, hw, hw, C, K, k, st, k // 2, "v2", seed=41)


# geometry list of test_ops_gpu.py::test_conv_shape_fuzz + a stride-2 3x3
# with K = 128 (B, H, W, Cin, Cout, k, stride, pad)
FUZZ = [(3, 7, 7, 16, 16, 3, 1, 1), (5, 9, 9, 32, 48, 3, 2, 1),
        (2, 11, 11, 64, 24, 1, 1, 0), (7, 5, 5, 24, 64, 3, 1, 1),
        (1, 17, 17, 16, 40, 5, 2, 2), (4, 6, 6, 128, 72, 3, 1, 1),
        (2, 14, 14, 40, 16, 7, 2, 3), (4, 16, 16, 64, 128, 3, 2, 1)]

_CHILD = textwrap.dedent("""
    import sys
    sys.path.insert(0, {tests!r})
    import torch
    import _oracle as O
    from cilfw import _hip_ops as H
    import test_conv_routes_gpu as T
    mode = {mode!r}
    split = 0
    ran_bwd, ran_fwd = set(), set()  # (route, FAST instantiation) launched
    for i, (N, Hh, W, C, K, k, st, pd) in enumerate(
            T.FUZZ if mode != "bnp" else ()):
        route, ks = H.conv2d_bwd_data_route(N, Hh, W, C, K, k, k, st)
        if mode == "v2":
            assert route == "v2", (route, T.FUZZ[i])
            split += ks > 1
        else:
            assert route in ("v1_bk32", "v1_bk64"), (route, T.FUZZ[i])
        T._check_bwd_data(H, N, Hh, W, C, K, k, st, pd, route, seed=50 + i)
        ran_bwd.add((route, K % 16 == 0 and st <= 2))
        if mode == "v1":
            froute, fks = H.conv2d_fwd_route(N, Hh, W, C, K, k, k, st, pd)
            assert froute in ("v1_bk32", "v1_bk64"), (froute, T.FUZZ[i])
            x, w = T._xw(N, Hh, W, C, K, k, seed=70 + i)
            y, _ = H.conv2d_fwd(x.cuda(), w.cuda(), st, pd)
            ref, mag, n = O.conv_fwd_ref(x, w, st, pd)
            O.check(y, ref, mag, n + (fks if fks > 1 else 0), True,
                    "fwd " + froute)
            ran_fwd.add((froute, C % 16 == 0))
    assert mode != "v2" or split >= 2, "no split-K geometry reached v2"
    if mode == "v1":
        every = {{(r, f) for r in ("v1_bk32", "v1_bk64")
                 for f in (True, False)}}
        assert ran_bwd == every, ("bwd-data", sorted(every - ran_bwd))
        assert ran_fwd == every, ("forward", sorted(every - ran_fwd))
    for i, (N, Hh, W, C, K, route, fast) in enumerate(
            T.BNP_SHAPES if mode == "bnp" else ()):
        assert H.conv2d_bwd_data_route(N, Hh, W, C, K, 3, 3, 1) == (route, 1)
        assert (K % 16 == 0) == fast
        # ksplit == 1 store of the plain kernel against the fp64 oracle
        T._check_bwd_data(H, N, Hh, W, C, K, 3, 1, 1, route, seed=90 + i)
        torch.manual_seed(i)
        dev = "cuda"
        dy = torch.randn(N, Hh, W, K, device=dev).bfloat16() * 0.1
        w = torch.randn(3, 3, C, K, device=dev).bfloat16() * 0.05
        bn_x = torch.randn(N, Hh, W, C, device=dev).bfloat16()
        bn_y = torch.randn(N, Hh, W, C, device=dev).bfloat16()  # ~half <= 0
        mean = torch.randn(C, device=dev)
        invstd = torch.rand(C, device=dev) + 0.5
        gamma = torch.randn(C, device=dev)
        dx0 = H.conv2d_bwd_data(dy, w, 1, 1, Hh, W)
        dx1, parts = H.conv2d_bwd_data(dy, w, 1, 1, Hh, W,
                                       bn_meta=(bn_y, bn_x, mean, invstd, 1))
        assert parts is not None, "fusion did not engage"
        assert parts.shape == (2, 2, C)  # ragged second row block
        assert torch.equal(dx0, dx1), "dx changed under the BN epilogue"
        a = H.bn_bwd(dx0, bn_x, gamma, mean, invstd, bn_y, True, True)
        b = H.bn_bwd(dx0, bn_x, gamma, mean, invstd, bn_y, True, True,
                     ext_parts=parts)
        torch.cuda.synchronize()
        for j in (1, 2):  # dgamma, dbeta
            torch.testing.assert_close(a[j], b[j], rtol=2e-4, atol=2e-3)
    torch.cuda.synchronize()
    print("routes-child-ok")
""")


def _run_child(mode, env_extra):
    tests = os.path.dirname(os.path.abspath(__file__))
    code = _CHILD.format(tests=tests, mode=mode)
    env = dict(os.environ, **env_extra)
    p = subprocess.run([sys.executable, "-c", code], env=env,
                       capture_output=True, text=True, timeout=280,
                       cwd=os.path.dirname(tests))
    assert p.returncode == 0 and "routes-child-ok" in p.stdout, \
        p.stdout[-3000:] + p.stderr[-3000:]


@pytest.mark.timeout(300)
def test_bwd_data_v2_small_shapes_and_split_k():
    """CILFW_CONV_V2_BWD_MINM=1 sends every K%8==0 geometry to the all-glds
    bwd-data kernel — the only way to reach it with ksplit > 1. Subprocess
    (a fresh child) because the C-side threshold is a per-process static."""
    _run_child("v2", {"CILFW_CONV_V2_BWD_MINM": "1"})


@pytest.mark.timeout(300)
def test_v1_kernels_forward_and_bwd_data():
    """CILFW_CONV_V2=0: the v1 fast / generic and BK64 kernels — what a
    launch falls back to when the zero page is missing — forward and
    bwd-data over the same geometries."""
    _run_child("v1", {"CILFW_CONV_V2": "0"})


# bwd-data with the BN-backward epilogue, one shape per instantiation of
# conv2d_bwd_data_kernel<BKT, FAST, true> (3x3, stride 1, pad 1). M is 147,
# 147, 175, 144: two row blocks each, the second ragged.
BNP_SHAPES = [
    # N, H, W, C, K, route, FAST
    (3, 7, 7, 16, 16, "v1_bk32", True),
    (3, 7, 7, 16, 24, "v1_bk32", False),    # K % 16 != 0
    (7, 5, 5, 24, 64, "v1_bk64", True),     # RSK = 576
    (4, 6, 6, 128, 72, "v1_bk64", False),   # RSK = 648, two C tiles
]


@pytest.mark.timeout(300)
def test_bwd_data_bn_epilogue_every_instantiation():
    """CILFW_BNBWD_FUSE=1 with CILFW_CONV_KSPLIT_TARGET=1 (ksplit == 1
    everywhere): each BKT x FAST kernel with the epilogue gives the dx of
    the plain kernel bit for bit, and partials that reduce to the BN grads
    of the standalone sums pass (assertions and tolerances of
    test_ops_gpu.py::test_bnbwd_fuse_partials_match_sums_pass)."""
    _run_child("bnp", {"CILFW_BNBWD_FUSE": "1",
                       "CILFW_CONV_KSPLIT_TARGET": "1"})


# ------------------------------------------------- bwd-weight delivery

DW_GEOMS = FUZZ[:4] + [
    (4, 8, 8, 64, 128, 1, 2, 0),   # 1x1 stride-2 projection (gathered x)
    (2, 32, 32, 3, 64, 7, 2, 3),   # 7x7 stem: padded-im2col route
]


@pytest.mark.parametrize("N,H,W,C,K,k,st,pd", DW_GEOMS)
def test_bwd_weight_slot_delivery(N, H, W, C, K, k, st, pd):
    Hop = _H()
    x, w = _xw(N, H, W, C, K, k, seed=61)
    dy = _dy(x, k, st, pd, K, seed=62)
    Ho, Wo = dy.shape[1], dy.shape[2]
    plain = (N, H, W, C, K, k, st, pd) in FUZZ
    ref, mag, n = O.conv_dw_ref(dy, x, st, pd, k, k)

    route, ns = Hop.conv2d_bwd_weight_route(N, C, K, k, k, Ho, Wo, False)
    assert route == "v2"
    out = torch.full((k, k, C, K), float("nan"), device="cuda")
    got = Hop.conv2d_bwd_weight(dy.cuda(), x.cuda(), st, pd, k, k, out=out,
                                accum=False)
    assert got.data_ptr() == out.data_ptr()
    O.check(out, ref, mag, n + ns, False, f"dW out= ({route})")

    route, ns = Hop.conv2d_bwd_weight_route(N, C, K, k, k, Ho, Wo, True)
    if plain or k == 1:
        assert route == "v1_fast"
    pre = torch.randn(k, k, C, K, generator=torch.Generator().manual_seed(63))
    out = pre.clone().cuda()
    Hop.conv2d_bwd_weight(dy.cuda(), x.cuda(), st, pd, k, k, out=out,
                          accum=True)
    want = pre.double() + ref
    O.check(out, want, mag, n + ns, False, f"dW accum ({route})",
            extra=2.0 ** -23 * want.abs())
