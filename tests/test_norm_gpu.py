"""The kernels of csrc/norm.hip against the fp64 references and derived
allowances of ``tests/_norm_ref.py`` (run on MI355X: pytest -m gpu). The
comparator itself is tested on the CPU in test_norm_oracle_selftest.py.
"""

import pytest
import torch

import _norm_ref as R

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(),
                                 reason="needs GPU")]


def _H():
    from cilfw import _hip_ops
    return _hip_ops


def _ids(s):
    return "x".join(str(v) for v in s)


# ------------------------------------------------------------------------- BN

def _run_bn(inp, mode, training=True, ext_parts=None):
    Hop = _H()
    relu = mode != "plain"
    x, dy, gamma = inp["x"].cuda(), inp["dy"].cuda(), inp["gamma"].cuda()
    res = inp["res"].cuda() if mode == "res_relu" else None
    rm, rv = inp["rm0"].cuda(), inp["rv0"].cuda()
    y, mean, invstd = Hop.bn_fwd(x, gamma, inp["beta"].cuda(), rm, rv,
                                 R.MOMENTUM, R.EPS, training, relu,
                                 residual=res, ext_parts=ext_parts)
    dx, dgamma, dbeta, dres = Hop.bn_bwd(dy, x, gamma, mean, invstd, y, relu,
                                         training,
                                         want_dres=(mode == "res_relu"))
    torch.cuda.synchronize()
    return dict(y=y, mean=mean, invstd=invstd, rm=rm, rv=rv, dx=dx,
                dgamma=dgamma, dbeta=dbeta, dres=dres)


def _check_bn(out, inp, mode, training, what, backward=True):
    relu = mode != "plain"
    res = inp["res"] if mode == "res_relu" else None
    assert torch.isfinite(out["y"]).all() and torch.isfinite(out["dx"]).all()
    if training:
        st = R.bn_stats_ref(inp["x"], inp["rm0"], inp["rv0"])
        R.check(out["rm"], *st["running_mean"], f"{what} running_mean")
        R.check(out["rv"], *st["running_var"], f"{what} running_var")
        R.check(out["mean"], *st["mean"], f"{what} mean")
    else:
        st = R.bn_eval_stats_ref(inp["rm0"], inp["rv0"])
        R.check_bits(out["rm"], inp["rm0"], f"{what} running_mean kept")
        R.check_bits(out["rv"], inp["rv0"], f"{what} running_var kept")
        R.check_bits(out["mean"], inp["rm0"], f"{what} mean")
    r_inv = R.check(out["invstd"], *st["invstd"], f"{what} invstd")
    ref, tol, pre, band = R.bn_y_ref(inp["x"], inp["gamma"], inp["beta"], st,
                                     res, relu)
    R.check(out["y"].reshape(ref.shape), ref, tol, f"{what} y")
    if relu:
        R.check_relu_mask(out["y"], pre, band, what)
    if not backward:
        return r_inv
    b = R.bn_bwd_ref(inp["dy"], inp["x"], inp["gamma"], out["mean"],
                     out["invstd"], out["y"], relu, training)
    R.check(out["dgamma"], *b["dgamma"], f"{what} dgamma")
    R.check(out["dbeta"], *b["dbeta"], f"{what} dbeta")
    R.check(out["dx"].reshape(b["dx"][0].shape), *b["dx"], f"{what} dx")
    if mode == "res_relu":
        R.check_bits(out["dres"].reshape(b["dres"].shape), b["dres"],
                     f"{what} dres")
    else:
        assert out["dres"] is None
    return r_inv


@pytest.mark.parametrize("mode", R.BN_MODES)
@pytest.mark.parametrize("shape", R.BN_SHAPES, ids=_ids)
def test_bn_train_fwd_bwd(shape, mode):
    """Training forward (statistics, running statistics, output, ReLU mask)
    and backward (dgamma, dbeta, dx, dres) at the widths and row counts of
    _norm_ref.BN_SHAPES; (16643, 8) takes two trips of the slab loops, with
    a constant on the rows of the second trip, and must be bit-identical
    across two runs."""
    M, C = shape
    inp = R.bn_inputs(M, C)
    out = _run_bn(inp, mode)
    _check_bn(out, inp, mode, True, f"bn {shape} {mode}")
    if M > R.WAVE * R.ROWS_PER_BLK:
        assert _H()._lib.cilfw_bn_sums_gy(M) == R.gy_of(M) == 66
        again = _run_bn(inp, mode)
        for k, v in out.items():
            if v is not None:
                R.check_bits(again[k], v, f"bn {shape} {mode} rerun {k}")


def test_bn_fused_reduce_finalize_two_trips():
    """bn_reduce_finalize_kernel (statistics from per-row-block partials, as
    a producing conv hands them over) with gy = 66: two trips of its slab
    loop. The partials are the fp64 block sums rounded to fp32, one more
    rounding per block than the allowance's M - 1 additions need."""
    M, C = 16643, 8
    inp = R.bn_inputs(M, C)
    x64 = inp["x"].double().reshape(M, C)
    gy = R.gy_of(M)
    parts = torch.zeros(gy, 2, C, dtype=torch.float64)
    for b in range(gy):
        blk = x64[b * R.ROWS_PER_BLK:(b + 1) * R.ROWS_PER_BLK]
        parts[b, 0], parts[b, 1] = blk.sum(0), (blk * blk).sum(0)
    out = _run_bn(inp, "relu", ext_parts=parts.float().cuda())
    _check_bn(out, inp, "relu", True, "bn fused reduce (16643, 8)")


def test_bn_offset_mean():
    """x = 8 + 0.25 * signed_unit (|mean|/std ~ 43): the one-pass variance
    q/M - mu^2 and the Q*x + R fold of dx both cancel. Asserted under the
    derived allowances; the measured err/tol of invstd is printed (recorded
    in _norm_ref.OFFSET_MEAN_RECORD and COVERAGE.md). Plain mode: see the
    self-test for why the ReLU band cap excludes the other two."""
    inp = R.bn_inputs(293, 8, offset_mean=True)
    out = _run_bn(inp, "plain")
    r = _check_bn(out, inp, "plain", True, "bn offset-mean (293, 8)")
    ref, tol = R.bn_stats_ref(inp["x"], inp["rm0"], inp["rv0"])["invstd"]
    rel = ((out["invstd"].double().cpu() - ref).abs() / ref).max().item()
    print(f"offset-mean invstd: err/tol = {r:.6f}, max relative error = "
          f"{rel:.3e}, allowance/invstd = {(tol / ref).max().item():.3e}")


@pytest.mark.parametrize("mode", R.BN_MODES)
def test_bn_eval_fwd_bwd(mode):
    """Eval mode on the non-frozen path: mean is running_mean bit for bit,
    invstd = rsqrtf(running_var + eps), running statistics untouched;
    backward with training = 0 is dx = P * g."""
    inp = R.bn_inputs(*R.BN_EVAL_SHAPE)
    out = _run_bn(inp, mode, training=False)
    _check_bn(out, inp, mode, False, f"bn eval {R.BN_EVAL_SHAPE} {mode}")


# ------------------------------------------------------------------ elementwise

@pytest.mark.parametrize("total,mixed", [(t, False)
                                         for t in R.ADD_RELU_TOTALS]
                         + [(R.ADD_RELU_MIXED, True)])
def test_add_relu(total, mixed):
    Hop = _H()
    a, b, dy = R.add_relu_inputs(total, mixed)
    ref, tol, da = R.add_relu_ref(a, b, dy)
    y = Hop.add_relu_fwd(a.cuda(), b.cuda())
    R.check(y, ref, tol, f"add_relu {total} y")
    assert torch.equal(y.cpu() > 0, ref > 0)
    R.check_bits(Hop.add_relu_bwd(dy.cuda(), y), da, f"add_relu {total} da")


@pytest.mark.parametrize("shape", R.GAP_SHAPES, ids=_ids)
def test_gap(shape):
    Hop = _H()
    x, dy = R.gap_inputs(*shape)
    yref, ytol, dref, dtol = R.gap_ref(x, dy)
    R.check(Hop.gap_fwd(x.cuda()), yref, ytol, f"gap {shape} y")
    R.check(Hop.gap_bwd(dy.cuda(), x.shape[1], x.shape[2]), dref, dtol,
            f"gap {shape} dx")


@pytest.mark.parametrize("shape", R.DS_SHAPES, ids=_ids)
def test_downsample_a(shape):
    Hop = _H()
    x, dy = R.ds_inputs(*shape)
    y, dx = R.ds_ref(x, dy)
    R.check_bits(Hop.downsample_a_fwd(x.cuda()), y, f"downsample_a {shape} y")
    R.check_bits(Hop.downsample_a_bwd(dy.cuda(), shape[1], shape[2]), dx,
                 f"downsample_a {shape} dx")


@pytest.mark.parametrize("case", R.POOL_CASES, ids=_ids)
def test_maxpool(case):
    """Ties in every 3x3 window: the first maximum in scan order wins, idx
    exact, y bit-exact; C = 12 takes the scalar backward kernel."""
    Hop = _H()
    N, H, W, C, k, st, pad = case
    x, dy = R.pool_inputs(*case)
    y, idx, dref, dtol = R.pool_ref(x, dy, k, st, pad)
    yg, ig = Hop.maxpool_fwd(x.cuda(), k, st, pad)
    R.check_bits(yg, y, f"maxpool {case} y")
    R.check_bits(ig, idx, f"maxpool {case} idx")
    R.check(Hop.maxpool_bwd(dy.cuda(), ig, H, W, k, st, pad), dref, dtol,
            f"maxpool {case} dx")


# -------------------------------------------------------------------- refusals

def test_refusals():
    """Each raised by the wrapper before any launch."""
    Hop = _H()
    dev = "cuda"

    def bf(*shape):
        return torch.zeros(*shape, dtype=torch.bfloat16, device=dev)

    def f32(n, v=0.0):
        return torch.full((n,), v, dtype=torch.float32, device=dev)

    x, small = bf(2, 8, 8, 16), bf(2, 7, 7, 16)
    gam, bet, rm, rv = f32(16, 1.0), f32(16), f32(16), f32(16, 1.0)
    with pytest.raises(AssertionError, match="residual"):
        Hop.bn_fwd(x, gam, bet, rm, rv, 0.1, 1e-5, True, True, residual=small)
    frm = rm.clone()
    frm._cilfw_frozen = (rm.clone(), rv.clone())
    with pytest.raises(AssertionError, match="residual"):
        Hop.bn_fwd(x, gam, bet, frm, rv, 0.1, 1e-5, False, True,
                   residual=small)
    x12 = bf(2, 4, 4, 12)
    g12, r12 = f32(12, 1.0), f32(12)
    r12._cilfw_frozen = (f32(12), f32(12, 1.0))
    with pytest.raises(AssertionError, match="C%8"):
        Hop.bn_fwd(x12, g12, f32(12), r12, f32(12, 1.0), 0.1, 1e-5, False,
                   False)
    with pytest.raises(AssertionError, match="C%8"):
        Hop.bn_bwd(x12, x12, g12, f32(12), f32(12, 1.0), x12, False, True)
    with pytest.raises(AssertionError, match="bn_bwd"):
        Hop.bn_bwd(small, x, gam, rm, rv, x, True, True)
    with pytest.raises(AssertionError, match="add_relu"):
        Hop.add_relu_fwd(x, small)
    with pytest.raises(AssertionError, match="add_relu_bwd"):
        Hop.add_relu_bwd(small, x)
    with pytest.raises(AssertionError, match="downsample_a_bwd"):
        Hop.downsample_a_bwd(bf(2, 7, 7, 16), 15, 15)      # floor extent
    with pytest.raises(AssertionError, match="gap_bwd"):
        Hop.gap_bwd(bf(2, 1, 1, 16), 7, 7)
    idx = torch.zeros(2, 4, 4, 16, dtype=torch.int32, device=dev)
    with pytest.raises(AssertionError, match="maxpool_bwd"):
        Hop.maxpool_bwd(bf(2, 3, 3, 16), idx, 8, 8, 3, 2, 1)
    with pytest.raises(AssertionError, match="maxpool_bwd"):
        Hop.maxpool_bwd(bf(2, 4, 4, 16), idx[:, :3], 8, 8, 3, 2, 1)
    torch.cuda.synchronize()
