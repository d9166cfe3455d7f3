"""Cosine head and embedding distillation HIP kernels (csrc/cosine.hip)
against the fp64 oracle of _cos_ref, sigma read on the device under graph
replay, the wrapper refusals, and --gpu_data engine runs with --head cosine
--lambda_flat (pytest -m gpu). Shapes, inputs and allowances are those of
_cos_ref; no element, row or class is excluded."""

import contextlib
import io
import math
import re

import pytest
import torch

import _cos_ref as R
from cilfw import ops
from cilfw.config import parse_args

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(),
                                 reason="needs GPU")]

DEV = "cuda:0"
BF = torch.bfloat16
UPS = [1.0, 0.37]
_CACHE = {}


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def _head_fwd_bwd(xd, wd, sd, g):
    x = xd.clone().requires_grad_(True)
    w = wd.clone().requires_grad_(True)
    s = sd.clone().requires_grad_(True)
    logits = ops.cosine_linear(x, w, s)
    logits.backward(g)
    return logits.detach(), x.grad, w.grad, s.grad


def _flat_fwd_bwd(sd, td, scale=1.0):
    s = sd.clone().requires_grad_(True)
    loss = ops.flat_loss(s, td)
    (loss * scale).backward()
    return loss.detach(), s.grad


def _case(name):
    """Oracles and one device forward + backward per shape and upstream,
    computed once and shared (read-only) by the tests."""
    if name not in _CACHE:
        x, w, sigma, dy = R.make_head(name)
        xd, wd, sd = x.to(DEV), w.to(DEV), sigma.to(DEV)
        c = dict(x=x, w=w, sigma=sigma, xd=xd, wd=wd, sd=sd, head={})
        for up in UPS:
            # the upstream dlogits is a bf16 tensor: the oracle takes the
            # rounded product
            g = (dy.float() * up).to(BF)
            c["head"][up] = dict(g=g.to(DEV), ref=R.head_ref(x, w, sigma, g),
                                 out=_head_fwd_bwd(xd, wd, sd, g.to(DEV)))
        s, t = R.make_feats(name)
        sdv, tdv = s.to(DEV), t.to(DEV)
        c.update(s=s, t=t, sdv=sdv, tdv=tdv, flat_ref=R.flat_ref(s, t),
                 flat={up: _flat_fwd_bwd(sdv, tdv, up) for up in UPS},
                 l=ops.flat_dist(sdv, tdv))
        torch.cuda.synchronize()
        _CACHE[name] = c
    return _CACHE[name]


@pytest.mark.parametrize("name", R.SHAPE_IDS)
def test_rownorm(name):
    """rownorm_fwd on features (scaled by sigma) and on fp32 weights, into
    NaN-prefilled outputs."""
    from cilfw import _hip_ops as H
    c = _case(name)
    ref = c["head"][1.0]["ref"]
    M, C, D = ref["M"], ref["C"], ref["D"]
    xs, rx = H.rownorm_fwd(c["xd"], c["sd"], out=_nan(M, D, dtype=BF),
                           rinv=_nan(M))
    wn, rw = H.rownorm_fwd(c["wd"], None, out=_nan(C, D, dtype=BF),
                           rinv=_nan(C))
    rs = dict(rx=R.worst_rinv(rx, ref["rx"], D),
              rw=R.worst_rinv(rw, ref["rw"], D),
              xs=R.worst_unit(xs, ref["xs"], D),
              wn=R.worst_unit(wn, ref["wn"], D))
    print(f"{name}: err/allowance " + " ".join(
        f"{k} {v:.4f}" for k, v in rs.items()))
    assert all(v <= 1.0 for v in rs.values()), rs


@pytest.mark.parametrize("name", R.SHAPE_IDS)
def test_logits(name):
    c = _case(name)
    h = c["head"][1.0]
    logits = h["out"][0]
    assert logits.dtype == BF \
        and logits.shape == (h["ref"]["M"], h["ref"]["C"])
    r = R.worst_logits(logits, h["ref"])
    print(f"{name}: logits err/allowance {r:.4f}")
    assert r <= 1.0


@pytest.mark.parametrize("up", UPS)
@pytest.mark.parametrize("name", R.SHAPE_IDS)
def test_head_gradients(name, up):
    from cilfw import _hip_ops as H
    c = _case(name)
    h = c["head"][up]
    ref = h["ref"]
    _, dx, dw, ds = h["out"]
    assert dx.dtype == BF and dw.dtype == torch.float32 and ds.shape == (1,)
    rs = dict(dx=R.worst_dx(dx, ref), dw=R.worst_dw(dw, ref),
              dsigma=R.worst_dsigma(ds, ref))
    print(f"{name} upstream {up}: err/allowance " + " ".join(
        f"{k} {v:.4f}" for k, v in rs.items()))
    assert all(v <= 1.0 for v in rs.values()), rs
    # the projection kernels write every element: NaN-prefilled outputs
    xs, rx = H.rownorm_fwd(c["xd"], c["sd"])
    wn, rw = H.rownorm_fwd(c["wd"])
    G, sH, _ = H.linear_bwd(h["g"], xs, wn, False)
    dx2, _ = H.rownorm_bwd(c["xd"], rx, G, c["sd"], want_dsig=True,
                           out=_nan(*dx.shape, dtype=BF))
    dw2, _ = H.rownorm_bwd(c["wd"], rw, sH, out=_nan(*dw.shape))
    assert torch.equal(dx2, dx) and torch.equal(dw2, dw)
    if up != 1.0:
        # the upstream is not ignored: the result fails the upstream-1 oracle
        ref1 = c["head"][1.0]["ref"]
        assert R.worst_dx(dx, ref1) > 1.0 and R.worst_dw(dw, ref1) > 1.0
        # dsigma = sum g z cancels with signed g: where the scaled oracle
        # itself lies within the upstream-1 allowance, no result can fail
        # it; test_dsigma_upstream_without_cancellation covers the scalar
        if R.worst_dsigma((UPS[1] * ref1["dsigma"]).float(), ref1) > 1.0:
            assert R.worst_dsigma(ds, ref1) > 1.0


def test_dsigma_upstream_without_cancellation():
    """|w| and |dlogits|: every term of dsigma is positive, so a dropped
    upstream factor shows in the scalar too."""
    x, w, sigma, dy = R.make_head("cifar64")
    w, dy = w.abs(), dy.abs()
    g = (dy.float() * UPS[1]).to(BF)
    ds = _head_fwd_bwd(x.to(DEV), w.to(DEV), sigma.to(DEV), g.to(DEV))[3]
    r = R.worst_dsigma(ds, R.head_ref(x, w, sigma, g))
    print(f"dsigma, unsigned data, upstream {UPS[1]}: err/allowance {r:.4f}")
    assert r <= 1.0
    assert R.worst_dsigma(ds, R.head_ref(x, w, sigma, dy)) > 1.0


@pytest.mark.parametrize("name", R.SHAPE_IDS)
def test_flat(name):
    from cilfw import _hip_ops as H
    c = _case(name)
    ref = c["flat_ref"]
    loss, ds = c["flat"][1.0]
    assert ds.dtype == BF and ds.shape == c["s"].shape
    assert c["l"].dtype == torch.float32
    M, D = ref["M"], ref["D"]
    loss2, l2, gs = H.flat_dist(c["sdv"], c["tdv"], out=_nan(M, D),
                                rows_out=_nan(M))
    assert torch.equal(loss2, loss) and torch.equal(l2, c["l"])
    ds2 = H.flat_bwd(gs, torch.ones(1, device=DEV),
                     out=_nan(M, D, dtype=BF))
    assert torch.equal(ds2, ds)  # NaN prefill fully overwritten
    up = float(torch.tensor(UPS[1], dtype=torch.float32))
    ds37 = c["flat"][UPS[1]][1]
    rs = dict(l=R.worst_flat_rows(c["l"], ref),
              loss=R.worst_flat_loss(loss, ref),
              ds=R.worst_flat_grad(ds, ref),
              ds37=R.worst_flat_grad(ds37, ref, scale=up))
    print(f"{name}: err/allowance " + " ".join(
        f"{k} {v:.4f}" for k, v in rs.items()))
    assert all(v <= 1.0 for v in rs.values()), rs
    assert R.worst_flat_grad(ds37, ref, scale=1.0) > 1.0


@pytest.mark.parametrize("name", R.SHAPE_IDS)
def test_two_launches_bit_identical(name):
    c = _case(name)
    h = c["head"][UPS[1]]
    again = _head_fwd_bwd(c["xd"], c["wd"], c["sd"], h["g"])
    assert all(torch.equal(a, b) for a, b in zip(again, h["out"]))
    loss, ds = _flat_fwd_bwd(c["sdv"], c["tdv"], UPS[1])
    assert torch.equal(loss, c["flat"][UPS[1]][0])
    assert torch.equal(ds, c["flat"][UPS[1]][1])
    assert torch.equal(ops.flat_dist(c["sdv"], c["tdv"]), c["l"])


def test_zero_rows():
    """One feature row and one weight row all zero: their logits and
    gradients are exactly 0 and finite; every other row stays within its
    allowance (the oracle's bound is 0 on the zero rows, so the comparators
    ask for exact zeros there too)."""
    x, w, sigma, dy = R.make_head("ragged40")
    x[5] = 0
    w[66] = 0
    ref = R.head_ref(x, w, sigma, dy)
    logits, dx, dw, ds = _head_fwd_bwd(x.to(DEV), w.to(DEV), sigma.to(DEV),
                                       dy.to(DEV))
    assert (logits[5] == 0).all() and (logits[:, 66] == 0).all()
    assert (dx[5] == 0).all() and (dw[66] == 0).all()
    for t in (logits, dx, dw, ds):
        assert torch.isfinite(t.float()).all()
    rs = dict(logits=R.worst_logits(logits, ref), dx=R.worst_dx(dx, ref),
              dw=R.worst_dw(dw, ref), dsigma=R.worst_dsigma(ds, ref))
    print("zero rows: err/allowance " + " ".join(
        f"{k} {v:.4f}" for k, v in rs.items()))
    assert all(v <= 1.0 for v in rs.values()), rs


def test_flat_equal_features():
    """Bitwise-equal student and teacher: loss == 0.0 and gradient == 0
    everywhere, with and without a zero row."""
    for name in ("cifar64", "sweep520"):
        for zero_row in (False, True):
            s = R.make_feats(name)[0]
            if zero_row:
                s[s.shape[0] // 2] = 0
            sd = s.to(DEV)
            loss, ds = _flat_fwd_bwd(sd, sd.clone())
            assert loss.item() == 0.0
            assert torch.isfinite(ds.float()).all() and (ds == 0).all()
            assert (ops.flat_dist(sd, sd.clone()) == 0).all()


def test_sigma_is_read_on_the_device():
    """cosine_linear forward + backward captured once; sigma changed in place
    between two replays: the second replay computes with the new value."""
    x, w, sigma, dy = R.make_head("cifar64")
    xd = x.to(DEV).requires_grad_(True)
    wd = w.to(DEV).requires_grad_(True)
    sd = sigma.to(DEV).requires_grad_(True)
    g = dy.to(DEV)

    def step():
        logits = ops.cosine_linear(xd, wd, sd)
        return (logits,) + torch.autograd.grad(logits, (xd, wd, sd), g)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    graph.replay()
    torch.cuda.synchronize()
    ref_old = R.head_ref(x, w, sigma, dy)
    assert R.worst_logits(out[0], ref_old) <= 1.0
    assert R.worst_dsigma(out[3], ref_old) <= 1.0
    with torch.no_grad():
        sd.fill_(1.25)
    graph.replay()
    torch.cuda.synchronize()
    ref_new = R.head_ref(x, w, torch.tensor([1.25]), dy)
    rs = dict(logits=R.worst_logits(out[0], ref_new),
              dx=R.worst_dx(out[1], ref_new), dw=R.worst_dw(out[2], ref_new),
              dsigma=R.worst_dsigma(out[3], ref_new))
    print("after sigma.fill_: err/allowance " + " ".join(
        f"{k} {v:.4f}" for k, v in rs.items()))
    assert all(v <= 1.0 for v in rs.values()), rs
    assert R.worst_logits(out[0], ref_old) > 1.0
    assert R.worst_dx(out[1], ref_old) > 1.0


def test_wrapper_refusals():
    """Refused by the wrappers before any launch."""
    sg = torch.ones(1, device=DEV)
    x12 = torch.ones(2, 12, device=DEV, dtype=BF)
    w12 = torch.ones(3, 12, device=DEV)
    with pytest.raises(AssertionError, match="D % 8 == 0"):
        ops.cosine_linear(x12, w12, sg)
    with pytest.raises(AssertionError, match="D % 8 == 0"):
        ops.flat_loss(x12, x12)
    f32 = torch.ones(2, 16, device=DEV)
    with pytest.raises(AssertionError, match="bf16"):
        ops.cosine_linear(f32, torch.ones(3, 16, device=DEV), sg)
    with pytest.raises(AssertionError, match="bf16"):
        ops.flat_loss(f32, f32)
    wide = torch.ones(1, 2056, device=DEV, dtype=BF)
    with pytest.raises(AssertionError, match="D <= 2048"):
        ops.cosine_linear(wide, torch.ones(2, 2056, device=DEV), sg)
    with pytest.raises(AssertionError, match="D <= 2048"):
        ops.flat_dist(wide, wide)
    a = torch.ones(4, 16, device=DEV, dtype=BF)
    with pytest.raises(AssertionError, match="student features"):
        ops.flat_loss(a, a[:, :8].contiguous())
    with pytest.raises(AssertionError, match="student features"):
        ops.flat_dist(a, a[:2])
    from cilfw import _hip_ops as H
    lib = H._lib
    assert lib.cilfw_cosine_supported(4, 16, 0) == 1
    assert lib.cilfw_cosine_supported(4, 12, 0) == 0
    assert lib.cilfw_cosine_supported(4, 12, 1) == 1
    assert lib.cilfw_cosine_supported(4, 2056, 0) == 0
    assert lib.cilfw_cosine_supported(0, 16, 0) == 0


def _engine_run(extra=()):
    from cilfw.engine import run
    args = parse_args([
        "--data_set", "synthetic", "--backbone", "resnet20",
        "--synthetic_classes", "10", "--num_bases", "5", "--increment", "5",
        "--num_epochs", "1", "--batch_size", "32", "--workers", "0",
        "--synthetic_train_size", "640", "--memory_size", "40",
        "--eval_every_epoch", "0", "--input_size", "32", "--no_aug",
        "--lr", "0.05", "--seed", "3", "--dtype", "bf16", "--gpu_data",
        "--head", "cosine", "--lambda_flat", "1"] + list(extra))
    sigmas = []
    from cilfw.models import CilModel
    orig = CilModel.after_model_adaption

    def spy(self, nb_classes, a=None):
        sigmas.append(self.fc.sigma.item())
        return orig(self, nb_classes, a)

    CilModel.after_model_adaption = spy
    out = io.StringIO()
    try:
        with contextlib.redirect_stdout(out):
            accs = run(args)
    finally:
        CilModel.after_model_adaption = orig
    return accs, out.getvalue(), sigmas


@pytest.mark.parametrize("extra", [(), ("--lambda_pod", "3")],
                         ids=["flat", "flat_pod"])
def test_engine_cosine_flat_captures_and_repeats(extra):
    """--gpu_data --head cosine --lambda_flat 1 (and with --lambda_pod 3):
    the run completes with the head and the flat term inside the captured
    step graph, the flat meter is finite on task 1 only, WA is skipped,
    sigma is trained, and a second identical run repeats it bit for bit."""
    accs, out, sigmas = _engine_run(extra)
    assert len(accs) == 2
    assert "capture failed" not in out
    assert "weight aligning skipped" in out
    t0 = re.findall(r"^task 0 epoch \d+: .*$", out, re.M)
    t1 = re.findall(r"^task 1 epoch \d+: .*$", out, re.M)
    assert len(t0) == 1 and len(t1) == 1 and "flat:" not in t0[0]
    pat = r"  flat: (\S+) \((\S+)\)"
    m = re.search(pat, t1[0])
    assert m, t1[0]
    assert all(math.isfinite(float(v)) for v in m.groups())
    assert ("  pod: " in t1[0]) == bool(extra)
    assert len(sigmas) == 2 and sigmas[0] != 1.0  # sigma after task 0
    accs2, out2, sigmas2 = _engine_run(extra)
    assert accs2 == accs and sigmas2 == sigmas

    def meters(line):
        return re.sub(r"imgs/s \d+", "", line)
    for task in (0, 1):
        a = re.findall(rf"^task {task} epoch \d+: .*$", out, re.M)
        b = re.findall(rf"^task {task} epoch \d+: .*$", out2, re.M)
        assert [meters(v) for v in a] == [meters(v) for v in b]
