"""CPU self-test of the BN / residual / pooling / DownsampleA oracle in
``tests/_norm_ref.py``.

The project's fp32 CPU path of every ``CF`` op must be accepted at every
shape tests/test_norm_gpu.py uses, and "wrong kernels" built from the fp64
reference with one seeded fault each, rounded like the kernel's output, must
be rejected by more than 10x the allowance. No GPU involved.
"""

import pytest
import torch
import torch.nn.functional as F

import _norm_ref as R
import cilfw.ops.functional as CF
from test_ops_gpu import _cmp

BF = torch.bfloat16


def _bn_ids(s):
    return f"{s[0]}x{s[1]}"


# ----------------------------------------------------------- CPU path accepted

def _cpu_bn(inp, mode, training=True):
    C = inp["x"].shape[-1]
    x = inp["x"].clone().requires_grad_(True)
    gamma = inp["gamma"].clone().requires_grad_(True)
    beta = inp["beta"].clone().requires_grad_(True)
    rm, rv = inp["rm0"].clone(), inp["rv0"].clone()
    res = None
    if mode == "res_relu":
        res = inp["res"].clone().requires_grad_(True)
        y = CF.batchnorm_add_relu(x, res, gamma, beta, rm, rv, R.MOMENTUM,
                                  R.EPS, training)
    else:
        y = CF.batchnorm_act(x, gamma, beta, rm, rv, R.MOMENTUM, R.EPS,
                             training, relu=(mode == "relu"))
    y.backward(inp["dy"])
    # the statistics the CPU path saved for its backward (same fp32 ops)
    if training:
        xf = inp["x"].float().reshape(-1, C)
        mean, var = xf.mean(0), xf.var(0, unbiased=False)
    else:
        mean, var = rm.float(), rv.float()
    return dict(y=y.detach(), rm=rm, rv=rv, mean=mean,
                invstd=torch.rsqrt(var + R.EPS), dx=x.grad,
                dgamma=gamma.grad, dbeta=beta.grad,
                dres=None if res is None else res.grad)


def _check_bn(out, inp, mode, training, what):
    relu = mode != "plain"
    res = inp["res"] if mode == "res_relu" else None
    if training:
        st = R.bn_stats_ref(inp["x"], inp["rm0"], inp["rv0"])
        R.check(out["rm"], *st["running_mean"], f"{what} running_mean")
        R.check(out["rv"], *st["running_var"], f"{what} running_var")
    else:
        st = R.bn_eval_stats_ref(inp["rm0"], inp["rv0"])
        assert torch.equal(out["rm"], inp["rm0"])
        assert torch.equal(out["rv"], inp["rv0"])
    R.check(out["mean"], *st["mean"], f"{what} mean")
    R.check(out["invstd"], *st["invstd"], f"{what} invstd")
    ref, tol, pre, band = R.bn_y_ref(inp["x"], inp["gamma"], inp["beta"], st,
                                     res, relu)
    R.check(out["y"].reshape(ref.shape), ref, tol, f"{what} y")
    if relu:
        R.check_relu_mask(out["y"], pre, band, what)
    b = R.bn_bwd_ref(inp["dy"], inp["x"], inp["gamma"], out["mean"],
                     out["invstd"], out["y"], relu, training)
    R.check(out["dgamma"], *b["dgamma"], f"{what} dgamma")
    R.check(out["dbeta"], *b["dbeta"], f"{what} dbeta")
    R.check(out["dx"].reshape(b["dx"][0].shape), *b["dx"], f"{what} dx")
    return b


@pytest.mark.parametrize("mode", R.BN_MODES)
@pytest.mark.parametrize("shape", R.BN_SHAPES, ids=_bn_ids)
def test_bn_cpu_path_accepted(shape, mode):
    inp = R.bn_inputs(*shape)
    out = _cpu_bn(inp, mode)
    b = _check_bn(out, inp, mode, True, f"cpu bn {shape} {mode}")
    if mode == "res_relu":          # values (the CPU mask leaves -0.0)
        assert R.worst(out["dres"].reshape(b["dres"].shape), b["dres"],
                       0.0) == 0.0


def test_bn_cpu_path_accepted_offset_mean_and_eval():
    inp = R.bn_inputs(293, 8, offset_mean=True)
    x64 = inp["x"].double().reshape(-1, 8)
    assert (x64.mean(0).abs() / x64.std(0)).min() > 30
    # plain mode only: the one-pass variance allowance (5 % of invstd here)
    # propagates into the pre-activation, and the ReLU band it opens holds
    # 3.7 % of the elements, above the cap
    _check_bn(_cpu_bn(inp, "plain"), inp, "plain", True,
              "cpu bn offset-mean plain")
    inp = R.bn_inputs(*R.BN_EVAL_SHAPE)
    for mode in R.BN_MODES:
        _check_bn(_cpu_bn(inp, mode, training=False), inp, mode, False,
                  f"cpu bn eval {mode}")


def test_elementwise_cpu_paths_accepted():
    for total, mixed in [(t, False) for t in R.ADD_RELU_TOTALS] \
            + [(R.ADD_RELU_MIXED, True)]:
        a, b, dy = R.add_relu_inputs(total, mixed)
        ref, tol, da = R.add_relu_ref(a, b, dy)
        if mixed:
            assert (ref == 0).any() and (a.double() + b.double() < 0).any() \
                and (ref > 0).any()
        ag = a.clone().requires_grad_(True)
        y = CF.add_relu(ag, b)
        y.backward(dy)
        R.check(y, ref, tol, f"cpu add_relu {total}")
        assert R.worst(ag.grad, da, 0.0) == 0.0
    for shape in R.GAP_SHAPES:
        x, dy = R.gap_inputs(*shape)
        yref, ytol, dref, dtol = R.gap_ref(x, dy)
        xg = x.clone().requires_grad_(True)
        y = CF.global_avg_pool(xg)
        y.backward(dy)
        R.check(y, yref, ytol, f"cpu gap {shape} y")
        R.check(xg.grad, dref, dtol, f"cpu gap {shape} dx")


@pytest.mark.parametrize("case", R.POOL_CASES, ids=str)
def test_maxpool_cpu_path_accepted_faults_rejected(case):
    N, H, W, C, k, st, pad = case
    x, dy = R.pool_inputs(*case)
    y, idx, dref, dtol = R.pool_ref(x, dy, k, st, pad)
    xg = x.clone().requires_grad_(True)
    yc = CF.max_pool(xg, k, st, pad)
    yc.backward(dy)
    R.check_bits(yc.detach(), y, f"cpu maxpool {case} y")
    R.check(xg.grad, dref, dtol, f"cpu maxpool {case} dx")
    # ties of the maximum exist, so the scan order matters
    y2, idx2, d2, _ = R.pool_ref(x, dy, k, st, pad, last_wins=True)
    assert torch.equal(y2, y)
    assert R.worst(idx2, idx, 0.0) == float("inf"), "no tied maximum"
    assert R.worst(d2.to(BF), dref, dtol) > 10.0
    d3 = R.pool_ref(x, dy, k, st, pad, credit_all=True)[2]
    assert R.worst(d3.to(BF), dref, dtol) > 10.0
    assert R.worst(dref.to(BF), dref, dtol) <= 1.0


# ---------------------------------------------------------------- DownsampleA

def _ds_torch(x):
    """The reference module: AvgPool2d(1, 2) + zero-channel concat (NCHW)."""
    p = F.avg_pool2d(x.permute(0, 3, 1, 2), 1, 2)
    return torch.cat([p, torch.zeros_like(p)], 1).permute(0, 2, 3, 1)


@pytest.mark.parametrize("H", [15, 8, 7, 1])
@pytest.mark.parametrize("W", [15, 8, 7, 1])
def test_downsample_a_cpu_matches_avgpool(H, W):
    gen = torch.Generator().manual_seed(H * 16 + W)
    x = torch.randn(2, H, W, 8, generator=gen)
    a = x.clone().requires_grad_(True)
    b = x.clone().requires_grad_(True)
    ya, yb = CF.downsample_a(a), _ds_torch(b)
    assert ya.shape == yb.shape == (2, -(-H // 2), -(-W // 2), 16)
    assert torch.equal(ya, yb)
    dy = torch.randn(ya.shape, generator=gen)
    ya.backward(dy)
    yb.backward(dy)
    assert torch.equal(a.grad, b.grad)


@pytest.mark.parametrize("shape", R.DS_SHAPES, ids=str)
def test_downsample_a_reference_and_faults(shape):
    x, dy = R.ds_inputs(*shape)
    y, dx = R.ds_ref(x, dy)
    xg = x.clone().requires_grad_(True)
    yc = CF.downsample_a(xg)
    yc.backward(dy)
    R.check_bits(yc.detach(), y, f"cpu downsample_a {shape} y")
    R.check_bits(xg.grad, dx, f"cpu downsample_a {shape} dx")
    N, H, W, C = shape
    if H > 1:
        yb, dxb = R.ds_ref(x, dy, origin=1)
        assert R.worst(yb, y, 0.0) == float("inf")
        assert R.worst(dxb, dx, 0.0) == float("inf")
    if H % 2:
        yb, dxb = R.ds_ref(x, dy, floor=True)
        assert R.worst(yb, y, 0.0) == float("inf")       # extent differs
        if H > 1:
            assert R.worst(dxb, dx, 0.0) == float("inf")


# ------------------------------------------------------------- seeded BN faults

def _kernel_like(inp, mode):
    """The fp64 reference rounded like the kernel's outputs."""
    relu = mode != "plain"
    res = inp["res"] if mode == "res_relu" else None
    st = R.bn_stats_ref(inp["x"], inp["rm0"], inp["rv0"])
    ref, tol, _, _ = R.bn_y_ref(inp["x"], inp["gamma"], inp["beta"], st, res,
                                relu)
    mean, inv = st["mean"][0].float(), st["invstd"][0].float()
    y = ref.to(BF)
    b = R.bn_bwd_ref(inp["dy"], inp["x"], inp["gamma"], mean, inv, y, relu,
                     True)
    return st, (ref, tol), mean, inv, y, b


def test_slab_fault_rejected():
    """Statistics reduced over the first 64 slabs only, at the shape whose
    rows from slab 64 onward carry a constant."""
    M, C = 16643, 8
    assert R.gy_of(M) == 66 and M % R.ROWS_PER_BLK != 0
    inp = R.bn_inputs(M, C)
    st = R.bn_stats_ref(inp["x"], inp["rm0"], inp["rv0"])
    bad = R.bn_stats_ref(inp["x"], inp["rm0"], inp["rv0"],
                         rows=slice(0, R.WAVE * R.ROWS_PER_BLK))
    for k in ("mean", "invstd", "running_mean", "running_var"):
        assert R.worst(st[k][0].float(), *st[k]) <= 1.0
        r = R.worst(bad[k][0].float(), *st[k])
        print(f"first 64 slabs only, {k}: err/tol = {r:.1f}")
        assert r > 10.0, f"{k}: {r:.3g}"
    # the backward sums: dbeta / dgamma over the first 64 slabs only
    _, _, mean, inv, y, b = _kernel_like(inp, "relu")
    keep = torch.zeros(M, 1, 1, 1)
    keep[:R.WAVE * R.ROWS_PER_BLK] = 1
    bb = R.bn_bwd_ref((inp["dy"].float() * keep).to(BF), inp["x"],
                      inp["gamma"], mean, inv, y, True, True)
    for k in ("dgamma", "dbeta"):
        assert R.worst(b[k][0].float(), *b[k]) <= 1.0
        assert R.worst(bb[k][0].float(), *b[k]) > 10.0, k


def test_bn_faults_rejected():
    M, C = 293, 72
    inp = R.bn_inputs(M, C)
    st, (yref, ytol), mean, inv, y, b = _kernel_like(inp, "res_relu")
    f = M / (M - 1)
    m32, c1 = R.f32(R.MOMENTUM), 1.0 - R.f32(R.MOMENTUM)
    var = st["var"][0]
    bad = {}
    # biased variance written to running_var
    bad["rv_biased"] = ((c1 * inp["rv0"].double() + m32 * var).float(),
                        st["running_var"])
    # ... and the unbiased one used for normalisation
    bad["invstd_unbiased"] = ((var * f + R.f32(R.EPS)).rsqrt().float(),
                              st["invstd"])
    # a channel group shifted by 8
    bad["y_group_shift"] = (torch.roll(yref, 8, 1).to(BF), (yref, ytol))
    bad["y_no_residual"] = (R.bn_y_ref(inp["x"], inp["gamma"], inp["beta"],
                                       st, None, True)[0].to(BF),
                            (yref, ytol))
    kw = dict(dy=inp["dy"], x=inp["x"], gamma=inp["gamma"], mean_k=mean,
              invstd_k=inv, y_k=y, relu=True, training=True)
    bad["dgamma_unmasked"] = (R.bn_bwd_ref(mask=False, **kw)["dgamma"][0]
                              .float(), b["dgamma"])
    bad["dx_no_Qx"] = (R.bn_bwd_ref(with_q=False, **kw)["dx"][0].to(BF),
                       b["dx"])
    bad["dx_no_dbeta"] = (R.bn_bwd_ref(with_dbeta=False, **kw)["dx"][0]
                          .to(BF), b["dx"])
    bad["dx_eval_formula"] = (R.bn_bwd_ref(**dict(kw, training=False))["dx"]
                              [0].to(BF), b["dx"])
    bad["dx_group_shift"] = (torch.roll(b["dx"][0], 8, 1).to(BF), b["dx"])
    bad["dres_unmasked"] = (inp["dy"].reshape(M, C), (b["dres"], 0.0))
    # the correctly rounded reference passes each of these comparisons
    assert R.worst(yref.to(BF), yref, ytol) <= 1.0
    assert R.worst(b["dx"][0].to(BF), *b["dx"]) <= 1.0
    assert R.worst(st["running_var"][0].float(), *st["running_var"]) <= 1.0
    for name, (got, (ref, tol)) in bad.items():
        r = R.worst(got, ref, tol)
        print(f"{name}: err/tol = {r:.1f}")
        assert r > 10.0, f"{name}: fault accepted or too close ({r:.3g})"


def test_gap_scale_fault():
    """gap scaled by 1/(HW + 1). Half a bf16 ulp is 1/256 of the value, so
    at HW = 49 / 64 this fault is only ~5 / ~4 allowances away (no bound on
    a bf16 output can separate it further); at HW = 1 it is 128."""
    rs = {}
    for shape in R.GAP_SHAPES:
        N, HW, C = shape
        x, dy = R.gap_inputs(*shape)
        yref, ytol, dref, dtol = R.gap_ref(x, dy)
        rs[HW] = R.worst((yref * HW / (HW + 1)).to(BF), yref, ytol)
        assert rs[HW] > 3.0, shape
        assert R.worst((dref * HW / (HW + 1)).to(BF), dref, dtol) > 3.0
        assert R.worst(yref.to(BF), yref, ytol) <= 1.0
    assert rs[1] > 10.0


def _cmp_accepts(got, ref):
    try:
        _cmp(got, ref)
    except AssertionError:
        return False
    return True


def test_whole_tensor_cmp_accepts_seeded_faults():
    """Why this file exists: ``_cmp`` with the tolerances of
    tests/test_ops_gpu.py (0.02 + 0.02 * max|ref|) accepts a running_var fed
    the biased variance, an invstd from the unbiased one and a gap divided
    by HW + 1; the per-element allowances reject each (asserted above and
    again here)."""
    M, C = 293, 72
    inp = R.bn_inputs(M, C)
    st = R.bn_stats_ref(inp["x"], inp["rm0"], inp["rv0"])
    var = st["var"][0]
    m32, c1 = R.f32(R.MOMENTUM), 1.0 - R.f32(R.MOMENTUM)
    pairs = {
        "rv_biased": ((c1 * inp["rv0"].double() + m32 * var).float(),
                      st["running_var"]),
        "invstd_unbiased": ((var * M / (M - 1) + R.f32(R.EPS)).rsqrt()
                            .float(), st["invstd"]),
    }
    x, dy = R.gap_inputs(3, 49, 264)
    yref, ytol, _, _ = R.gap_ref(x, dy)
    pairs["gap_hw_plus_1"] = ((yref * 49 / 50).to(BF), (yref, ytol))
    for name, (got, (ref, tol)) in pairs.items():
        assert _cmp_accepts(got, ref.float()), f"_cmp rejected {name}"
        assert R.worst(got, ref, tol) > 1.0, f"{name} accepted"
