"""POD-spatial distillation on the CPU: the ops against the fp64 oracle of
_pod_ref (the fp32 torch path is the calibration of its allowances), the
hand-written backward against torch autograd, the comparator self-test, the
backbones' return_maps, the CLI flag and the engine wiring."""

import contextlib
import io
import math
import re

import pytest
import torch
import torch.nn.functional as F

import _pod_ref as R
from cilfw import ops
from cilfw.config import parse_args
from cilfw.engine import run
from cilfw.models import CilModel


def _fwd_bwd(a, b, scale=1.0):
    a = a.clone().requires_grad_(True)
    loss = ops.pod_spatial(a, b)
    (loss * scale).backward()
    return loss.detach(), a.grad


# ----------------------------------------------------------------- ops vs fp64

@pytest.mark.parametrize("name", R.SHAPE_IDS)
def test_cpu_path_within_allowances(name):
    """The fp32 torch path (bf16 maps in, bf16 da out) is accepted by every
    comparator; the printed err/allowance figures are the calibration record
    of profiles/pod_loss.md."""
    a, b = R.make_maps(name)
    N, H, W, C = a.shape
    ref = R.stage_ref(a, b)
    pooled = ops.pod_pool(a)
    assert pooled.shape == (N, H + W, C) and pooled.dtype == torch.float32
    loss, da = _fwd_bwd(a, b)
    d = ops.pod_dist(a, b)
    assert da.dtype == torch.bfloat16 and da.shape == a.shape
    r_pool = max(R.worst_pooled(pooled, a),
                 R.worst_pooled(ops.pod_pool(b), b))
    r_dist = R.worst_dist(d, loss, ref)
    r_grad = R.worst_grad(da, ref)
    share = R.grad_sum_share(da, ref)
    print(f"{name}: err/allowance pooled {r_pool:.4f} dist {r_dist:.4f} "
          f"da {r_grad:.4f} (da summation share {share:.4f})")
    assert r_pool <= 1.0 and r_dist <= 1.0 and r_grad <= 1.0
    # calibration rule: the fp32 path stays under half of every fp32
    # allowance (da: of its summation term; the rest is the bf16 half ulp)
    assert r_pool <= 0.5 and r_dist <= 0.5 and share <= 0.5


def test_upstream_scale_cpu():
    a, b = R.make_maps("odd_hw")
    ref = R.stage_ref(a, b)
    _, da = _fwd_bwd(a, b, scale=0.37)
    assert R.worst_grad(da, ref, scale=0.37) <= 1.0
    assert R.worst_grad(da, ref, scale=1.0) > 1.0  # the scale is not ignored


def _composition(a, b):
    """The definition as a literal torch composition (autograd reference)."""
    def pooled(x):
        sq = x.pow(2)
        return torch.cat([sq.sum(dim=2), sq.sum(dim=1)], dim=1).reshape(
            x.shape[0], -1)
    va = F.normalize(pooled(a), dim=1, eps=1e-12)
    vb = F.normalize(pooled(b), dim=1, eps=1e-12)
    return (va - vb).norm(dim=1).mean()


@pytest.mark.parametrize("name", ["odd_hw", "c72", "cifar_s1"])
def test_backward_matches_autograd_fp64(name):
    """ops.pod_spatial's hand-written backward == torch autograd through the
    literal composition, in fp64, also under a non-unit upstream; the teacher
    gets no gradient."""
    a, b = (t.double() for t in R.make_maps(name))
    a1 = a.clone().requires_grad_(True)
    b1 = b.clone().requires_grad_(True)
    loss = ops.pod_spatial(a1, b1)
    assert loss.dtype == torch.float64
    (0.37 * loss).backward()
    assert b1.grad is None
    a2 = a.clone().requires_grad_(True)
    want = _composition(a2, b)
    (0.37 * want).backward()
    assert abs(loss.item() - want.item()) <= 1e-13
    scale = a2.grad.abs().max().item()
    assert (a1.grad - a2.grad).abs().max().item() <= 1e-12 * scale


def test_pod_loss_is_mean_over_stages():
    pairs = [R.make_maps(n) for n in ("odd_hw", "c72", "degenerate")]
    maps_s = [p[0].double().requires_grad_(True) for p in pairs]
    maps_t = [p[1].double() for p in pairs]
    total = ops.pod_loss(maps_s, maps_t)
    want = sum(_composition(a, b) for a, b in zip(maps_s, maps_t)) / 3
    assert abs(total.item() - want.item()) <= 1e-13
    total.backward()
    one = maps_s[1].detach().clone().requires_grad_(True)
    (_composition(one, maps_t[1]) / 3).backward()
    assert torch.allclose(maps_s[1].grad, one.grad, rtol=1e-10, atol=0)
    with pytest.raises(AssertionError, match="student maps"):
        ops.pod_loss(maps_s, maps_t[:2])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_zero_distance(dtype):
    """a == b bitwise: loss 0 and an all-zero, finite gradient — also with one
    sample that is all zeros."""
    a, _ = R.make_maps("odd_hw")
    a = a.to(dtype)
    for zero_sample in (False, True):
        x = a.clone()
        if zero_sample:
            x[1] = 0
        loss, da = _fwd_bwd(x, x.clone())
        assert loss.item() == 0.0
        assert torch.isfinite(da.float()).all() and (da == 0).all()


# --------------------------------------------------------- comparator self-test

def _gv_from_pooled(vs, vt, projection=True):
    N = vs.shape[0]
    fs, ft = vs.reshape(N, -1), vt.reshape(N, -1)
    ns = fs.norm(dim=1, keepdim=True)
    sh = fs / ns
    u = sh - ft / ft.norm(dim=1, keepdim=True)
    gh = u / (N * u.norm(dim=1, keepdim=True))
    if projection:
        gh = gh - sh * (sh * gh).sum(dim=1, keepdim=True)
    return (gh / ns).reshape(vs.shape)


def _da_from_gv(a, gv, factor=2.0):
    H = a.shape[1]
    t = gv[:, :H, None, :] + gv[:, None, H:, :]
    return (factor * a.double() * t).to(torch.bfloat16)


@pytest.mark.parametrize("name", ["odd_hw", "c72"])
def test_comparators_reject_seeded_faults(name):
    """"Wrong kernels" built on the CPU from the fp64 oracle, each with one
    seeded fault and rounded like a real kernel's output. Faults 1, 2 and 5
    change the pooled tensor and must be rejected by the pooled comparator;
    faults 3, 4 and 5 change da and must be rejected by the gradient
    comparator. The correctly rounded oracle is accepted by both."""
    a, b = R.make_maps(name)
    N, H, W, C = a.shape
    assert name != "odd_hw" or H != W  # fault 2 runs on this shape
    ref = R.stage_ref(a, b)
    good_pool = ref["pooled_s"].float()
    assert R.worst_pooled(good_pool, a) <= 1.0
    good_gv = _gv_from_pooled(ref["pooled_s"], ref["pooled_t"])
    assert R.worst_grad(_da_from_gv(a, good_gv), ref) <= 1.0

    sq = a.double() ** 2
    # 1: one pixel dropped from one row sum
    p1 = ref["pooled_s"].clone()
    p1[N - 1, H // 2] -= sq[N - 1, H // 2, W - 1]
    assert R.worst_pooled(p1.float(), a) > 1.0, "fault 1 accepted"
    # 2: r and q swapped (only distinguishable layouts: H != W)
    if H != W:
        p2 = torch.cat([sq.sum(dim=1), sq.sum(dim=2)], dim=1)
        assert R.worst_pooled(p2.float(), a) > 1.0, "fault 2 accepted"
    # 3: the factor 2 missing
    assert R.worst_grad(_da_from_gv(a, good_gv, factor=1.0), ref) > 1.0, \
        "fault 3 accepted"
    # 4: the projection term v^ (v^ . g^) missing
    gv4 = _gv_from_pooled(ref["pooled_s"], ref["pooled_t"], projection=False)
    assert R.worst_grad(_da_from_gv(a, gv4), ref) > 1.0, "fault 4 accepted"
    # 5: the last 8-channel group left unwritten (zero- and NaN-prefilled)
    for fill in (0.0, float("nan")):
        p5 = good_pool.clone()
        p5[..., C - 8:] = fill
        assert R.worst_pooled(p5, a) > 1.0, "fault 5 (pooled) accepted"
        d5 = _da_from_gv(a, good_gv)
        d5[..., C - 8:] = fill
        assert R.worst_grad(d5, ref) > 1.0, "fault 5 (da) accepted"


# ----------------------------------------------------------------------- models

@pytest.mark.parametrize("backbone,shapes", [
    ("resnet20", [(2, 16, 16, 16), (2, 8, 8, 32), (2, 4, 4, 64)]),
    ("resnet18", [(2, 16, 16, 64), (2, 8, 8, 128), (2, 4, 4, 256),
                  (2, 2, 2, 512)]),
])
def test_return_maps(backbone, shapes):
    torch.manual_seed(0)
    model = CilModel(backbone, 16)
    model.prev_model_adaption(5)
    model.eval()
    x = torch.randn(2, 16, 16, 3)
    with torch.no_grad():
        plain = model(x)
        logits, feats, maps = model(x, return_maps=True)
        bb = model.backbone(x)
        bb_feats, bb_maps = model.backbone(x, return_maps=True)
    assert isinstance(plain, tuple) and len(plain) == 2
    assert torch.equal(plain[0], logits) and torch.equal(plain[1], feats)
    assert torch.is_tensor(bb) and torch.equal(bb, bb_feats)
    assert [tuple(m.shape) for m in maps] == shapes
    assert [tuple(m.shape) for m in bb_maps] == shapes
    assert all((m >= 0).all() for m in maps)  # post-ReLU stage outputs


# ------------------------------------------------------------------------ engine

def test_cli_flag():
    assert parse_args([]).lambda_pod == 0.0
    assert parse_args(["--lambda_pod", "3"]).lambda_pod == 3.0


def _run(extra, monkeypatch_forward):
    args = parse_args([
        "--data_set", "synthetic", "--backbone", "resnet20",
        "--synthetic_classes", "10", "--num_bases", "5", "--increment", "5",
        "--num_epochs", "1", "--batch_size", "32", "--workers", "0",
        "--synthetic_train_size", "320", "--memory_size", "20",
        "--eval_every_epoch", "0", "--input_size", "16", "--no_aug",
        "--lr", "0.05", "--seed", "3", "--dtype", "fp32", "--device", "cpu",
    ] + list(extra))
    requests = []
    orig = CilModel.forward

    def spy(self, x, return_maps=False):
        requests.append((bool(return_maps), self.training))
        return orig(self, x, return_maps=return_maps)

    monkeypatch_forward(spy)
    out = io.StringIO()
    try:
        with contextlib.redirect_stdout(out):
            accs = run(args)
    finally:
        monkeypatch_forward(orig)
    return accs, out.getvalue(), requests


@pytest.fixture(scope="module")
def runs():
    def setter(fn):
        CilModel.forward = fn
    return dict(plain=_run([], setter),
                pod=_run(["--lambda_pod", "3"], setter),
                pod_only=_run(["--lambda_pod", "3", "--lambda_kd", "0"],
                              setter))


def _epoch_lines(out, task):
    return re.findall(rf"^task {task} epoch \d+: .*$", out, re.M)


def test_engine_default_requests_no_map(runs):
    accs, out, requests = runs["plain"]
    assert len(accs) == 2 and requests
    assert not any(r[0] for r in requests), "a map was requested"
    assert "pod" not in out


def test_engine_pod_meter_on_task1_only(runs):
    accs, out, requests = runs["pod"]
    assert len(accs) == 2
    t0, t1 = _epoch_lines(out, 0), _epoch_lines(out, 1)
    assert len(t0) == 1 and len(t1) == 1
    assert "pod:" not in t0[0]
    m = re.search(r"  pod: (\S+) \((\S+)\)", t1[0])
    assert m, t1[0]
    vals = [float(m.group(1)), float(m.group(2))]
    assert all(math.isfinite(v) and 0.0 < v <= 2.0 for v in vals)
    # task 1: the student (train mode) and the teacher (eval mode) are both
    # asked for maps on every step; nothing else is
    with_maps = [r for r in requests if r[0]]
    assert with_maps and sum(r[1] for r in with_maps) * 2 == len(with_maps)


def test_engine_pod_without_logit_kd(runs):
    accs, out, _ = runs["pod_only"]
    assert len(accs) == 2
    t1 = _epoch_lines(out, 1)
    assert re.search(r"  pod: (\S+) \((\S+)\)", t1[0])
    assert accs[0] == runs["pod"][0][0]  # task 0 does not depend on either
