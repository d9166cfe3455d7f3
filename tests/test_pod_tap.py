"""The pre-ReLU POD tap on the CPU: the --pod_tap flag, ops.add_relu_tap
(two differentiable outputs, one merged gradient), the backbones' "pre" mode
against their default mode on the same weights, the number of tap launches,
and one two-task engine run."""

import contextlib
import copy
import io
import math
import re

import pytest
import torch

import _pod_ref as R
import _pod_tap_ref as T
from cilfw import ops
from cilfw.config import parse_args
from cilfw.engine import run
from cilfw.models import CilModel
from cilfw.ops import functional as CF


# -------------------------------------------------------------------------- CLI

def test_cli_flag():
    assert parse_args([]).pod_tap == "post"
    args = parse_args(["--pod_tap", "pre", "--lambda_pod", "3"])
    assert args.pod_tap == "pre" and args.lambda_pod == 3.0
    assert parse_args(["--pod_tap", "post"]).pod_tap == "post"


def test_cli_refuses_pre_without_pod(capsys):
    with pytest.raises(SystemExit):
        parse_args(["--pod_tap", "pre"])
    assert "--pod_tap pre needs --lambda_pod" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        parse_args(["--pod_tap", "pre", "--lambda_pod", "0"])
    with pytest.raises(SystemExit):
        parse_args(["--pod_tap", "both", "--lambda_pod", "3"])


def test_model_refuses_unknown_tap():
    with pytest.raises(ValueError, match="pod_tap"):
        CilModel("resnet20", 16, pod_tap="both")


# --------------------------------------------------------------------------- op

def _signed(shape, seed, dtype=torch.float64):
    """(a, b) with |a + b| >= 0.1 and both signs of the sum present."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(shape, generator=g, dtype=torch.float64)
    s = torch.randn(shape, generator=g, dtype=torch.float64)
    s = s + 0.1 * torch.where(s >= 0, 1.0, -1.0)
    assert (s > 0).any() and (s < 0).any() and s.abs().min() >= 0.1
    return a.to(dtype), (s - a).to(dtype)


def test_forward_definition():
    a, b = _signed((2, 3, 3, 8), 0, torch.float32)
    y, z = ops.add_relu_tap(a, b)
    assert torch.equal(z, a + b)
    assert torch.equal(y, (a + b).clamp_min(0))
    assert torch.equal(y, ops.add_relu(a, b))
    a16, b16 = a.to(torch.bfloat16), b.to(torch.bfloat16)
    y16, z16 = ops.add_relu_tap(a16, b16)
    assert y16.dtype == z16.dtype == torch.bfloat16
    assert torch.equal(z16, (a16.float() + b16.float()).to(torch.bfloat16))
    assert torch.equal(y16, ops.add_relu(a16, b16))


def test_gradcheck_fp64():
    a, b = _signed((2, 3, 3, 8), 1)
    a.requires_grad_(True)
    b.requires_grad_(True)
    assert torch.autograd.gradcheck(ops.add_relu_tap, (a, b))


def test_merged_gradient():
    a, b = _signed((2, 3, 3, 8), 2)
    g = torch.Generator().manual_seed(5)
    w1 = torch.randn(a.shape, generator=g, dtype=torch.float64)
    w2 = torch.randn(a.shape, generator=g, dtype=torch.float64)
    a1 = a.clone().requires_grad_(True)
    b1 = b.clone().requires_grad_(True)
    y, z = ops.add_relu_tap(a1, b1)
    ((y * w1).sum() + (z * w2).sum()).backward()
    assert torch.equal(a1.grad, b1.grad)
    assert torch.equal(a1.grad, w2 + torch.where(a + b > 0, w1,
                                                 torch.zeros_like(w1)))


def test_y_alone_is_add_relu():
    a, b = _signed((2, 3, 3, 8), 3)
    w = torch.randn(a.shape, dtype=torch.float64,
                    generator=torch.Generator().manual_seed(6))
    grads = []
    for fn in (lambda p, q: ops.add_relu_tap(p, q)[0], ops.add_relu):
        a1 = a.clone().requires_grad_(True)
        b1 = b.clone().requires_grad_(True)
        (fn(a1, b1) * w).sum().backward()
        grads.append((a1.grad, b1.grad))
    assert torch.equal(grads[0][0], grads[1][0])
    assert torch.equal(grads[0][1], grads[1][1])
    assert (grads[0][0] == 0).any() and (grads[0][0] != 0).any()


def test_z_alone_returns_dz():
    a, b = _signed((2, 3, 3, 8), 4)
    w = torch.randn(a.shape, dtype=torch.float64,
                    generator=torch.Generator().manual_seed(7))
    a1 = a.clone().requires_grad_(True)
    b1 = b.clone().requires_grad_(True)
    _, z = ops.add_relu_tap(a1, b1)
    (z * w).sum().backward()
    assert torch.equal(a1.grad, w) and torch.equal(b1.grad, w)


@pytest.mark.parametrize("shape", T.TAP_SHAPES, ids=T.TAP_IDS)
def test_bf16_cpu_path_is_the_definition(shape):
    """The op's CPU path on the GPU tests' inputs (planted zero sums, tiny
    negative sums and RNE ties) == the literal definition of _pod_tap_ref."""
    a, b, dy, dz = T.tap_inputs(shape)
    y_ref, z_ref = T.tap_fwd_ref(a, b)
    a1 = a.clone().requires_grad_(True)
    b1 = b.clone().requires_grad_(True)
    y, z = ops.add_relu_tap(a1, b1)
    assert torch.equal(y, y_ref) and torch.equal(z, z_ref)
    assert torch.equal(y, ops.add_relu(a, b))
    torch.autograd.backward([y, z], [dy, dz])
    assert torch.equal(a1.grad, T.tap_bwd_ref(dy, dz, z_ref))
    assert torch.equal(b1.grad, a1.grad)
    for grads, want in (((dy, None), T.tap_bwd_ref(dy, None, z_ref)),
                        ((None, dz), dz)):
        a2 = a.clone().requires_grad_(True)
        y2, z2 = ops.add_relu_tap(a2, b)
        out, g = (y2, grads[0]) if grads[1] is None else (z2, grads[1])
        out.backward(g)
        assert torch.equal(a2.grad, want)


# ------------------------------------------------- POD torch path, signed maps

@pytest.mark.parametrize("name", R.SHAPE_IDS)
def test_pod_cpu_path_on_signed_maps(name):
    """The maps of a "pre" run are signed. _pod_ref's allowances hold as
    written for them (squares in the pooled terms, absolute values in the
    gradient allowance): the fp32 torch path of ops/pod.py stays within every
    one, no element excluded."""
    a, b = T.signed_maps(name)
    ref = R.stage_ref(a, b)
    x = a.clone().requires_grad_(True)
    loss = ops.pod_spatial(x, b)
    loss.backward()
    r_pool = max(R.worst_pooled(ops.pod_pool(a), a),
                 R.worst_pooled(ops.pod_pool(b), b))
    r_dist = R.worst_dist(ops.pod_dist(a, b), loss.detach(), ref)
    r_grad = R.worst_grad(x.grad, ref)
    print(f"{name} signed: err/allowance pooled {r_pool:.4f} dist "
          f"{r_dist:.4f} da {r_grad:.4f} (da summation share "
          f"{R.grad_sum_share(x.grad, ref):.4f})")
    assert r_pool <= 1.0 and r_dist <= 1.0 and r_grad <= 1.0


# -------------------------------------------------------------------- backbones

def _pair(backbone, train):
    """The same weights in the default and the "pre" mode."""
    torch.manual_seed(0)
    post = CilModel(backbone, 16)
    post.prev_model_adaption(5)
    pre = copy.deepcopy(post)
    pre.backbone.pod_tap = "pre"
    assert post.backbone.pod_tap == "post"
    for m in (post, pre):
        m.train(train)
    return post, pre


def _stem_weight(model):
    bb = model.backbone
    return (bb.conv_1_3x3 if hasattr(bb, "conv_1_3x3") else bb.stem).weight


@pytest.mark.parametrize("backbone,stages", [("resnet20", 3), ("resnet18", 4)])
def test_pre_maps_against_post(backbone, stages):
    post, pre = _pair(backbone, train=True)
    x = torch.randn(2, 16, 16, 3, generator=torch.Generator().manual_seed(1))
    lo, fo, mo = post(x, return_maps=True)
    lp, fp, mp = pre(x, return_maps=True)
    assert len(mo) == len(mp) == stages
    for zo, zp in zip(mo, mp):
        assert zo.shape == zp.shape
        assert (zp < 0).any(), "a pre-ReLU map without a negative entry"
        assert torch.equal(zp.clamp_min(0), zo)
    # in fp32 both tails perform the same operations
    assert torch.equal(fo, fp) and torch.equal(lo, lp)
    lo.sum().backward()
    lp.sum().backward()
    go, gp = _stem_weight(post).grad, _stem_weight(pre).grad
    assert go.abs().max() > 0
    assert torch.equal(go, gp)
    # the plain forward takes the tap path too and computes the same
    lp2, fp2 = pre(x)
    assert torch.equal(fp2, fp) and torch.equal(lp2, lp)


@pytest.mark.parametrize("backbone", ["resnet20", "resnet18"])
def test_pre_map_carries_gradient_below_zero(backbone):
    """A loss on the maps alone reaches the pre-activations the ReLU cuts: in
    eval mode BN is elementwise, so the gradient at the last BN's input is
    non-zero wherever z < 0 in "pre" mode and exactly zero there in the
    default mode."""
    post, pre = _pair(backbone, train=False)
    x = torch.randn(2, 16, 16, 3, generator=torch.Generator().manual_seed(2))
    grads, zmaps = [], []
    for model in (post, pre):
        bb = model.backbone
        last = list(bb.stage_3 if hasattr(bb, "stage_3") else bb.layer4)[-1]
        bn = last.bn_b if hasattr(last, "bn_b") else last.bn2
        seen = []

        def hook(mod, inputs):
            inputs[0].retain_grad()
            seen.append(inputs[0])

        h = bn.register_forward_pre_hook(hook)
        _, maps = bb(x, return_maps=True)
        h.remove()
        (maps[-1] ** 2).sum().backward()
        grads.append(seen[0].grad)
        zmaps.append(maps[-1].detach())
    cut = zmaps[1] < 0
    assert cut.any() and torch.equal(zmaps[0] == 0, zmaps[1] <= 0)
    assert (grads[0][cut] == 0).all()
    assert (grads[1][cut] != 0).all()


# ----------------------------------------------------------------- launch counts

@pytest.mark.parametrize("backbone,stages", [
    ("resnet20", 3), ("resnet32", 3), ("resnet18", 4), ("resnet50", 4)])
def test_tap_launches(backbone, stages, monkeypatch):
    calls = []
    orig = CF.add_relu_tap

    def spy(a, b):
        calls.append(tuple(a.shape))
        return orig(a, b)

    monkeypatch.setattr(CF, "add_relu_tap", spy)
    torch.manual_seed(0)
    model = CilModel(backbone, 32)
    model.prev_model_adaption(5)
    model.eval()
    x = torch.randn(2, 32, 32, 3)
    with torch.no_grad():
        model(x, return_maps=True)
        model(x)
    assert calls == [], "the default mode launched the tap"
    model.backbone.pod_tap = "pre"
    with torch.no_grad():
        _, _, maps = model(x, return_maps=True)
    assert len(calls) == stages == len(maps)
    assert calls == [tuple(m.shape) for m in maps]
    del calls[:]
    with torch.no_grad():
        model(x)
        model.extract_vector(x)
    assert len(calls) == 2 * stages
    # the frozen copy that teaches the next task inherits the mode
    teacher = model.copy()
    teacher.freeze()
    assert teacher.backbone.pod_tap == "pre"


def test_cil_model_sets_the_attribute():
    assert CilModel("resnet20", 16).backbone.pod_tap == "post"
    assert CilModel("resnet20", 16, pod_tap="pre").backbone.pod_tap == "pre"
    assert CilModel("resnet18", 16, pod_tap="pre").backbone.pod_tap == "pre"


# ------------------------------------------------------------------------ engine

def test_engine_pre_tap(monkeypatch):
    """Two synthetic tasks with --lambda_pod 3 --pod_tap pre on the CPU: the
    run completes, the pod meter is finite on task 1 only, student and teacher
    are both asked for maps, and the tap runs in every pass."""
    args = parse_args([
        "--data_set", "synthetic", "--backbone", "resnet20",
        "--synthetic_classes", "10", "--num_bases", "5", "--increment", "5",
        "--num_epochs", "1", "--batch_size", "32", "--workers", "0",
        "--synthetic_train_size", "320", "--memory_size", "20",
        "--eval_every_epoch", "0", "--input_size", "16", "--no_aug",
        "--lr", "0.05", "--seed", "3", "--dtype", "fp32", "--device", "cpu",
        "--lambda_pod", "3", "--pod_tap", "pre"])
    requests, taps, signed = [], [], []
    orig_fwd, orig_tap = CilModel.forward, CF.add_relu_tap

    def fwd_spy(self, x, return_maps=False):
        assert self.backbone.pod_tap == "pre"
        requests.append((bool(return_maps), self.training))
        out = orig_fwd(self, x, return_maps=return_maps)
        if return_maps:
            signed.append(all(bool((m < 0).any()) for m in out[2]))
        return out

    def tap_spy(a, b):
        taps.append(1)
        return orig_tap(a, b)

    monkeypatch.setattr(CilModel, "forward", fwd_spy)
    monkeypatch.setattr(CF, "add_relu_tap", tap_spy)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        accs = run(args)
    out = out.getvalue()
    assert len(accs) == 2
    t0 = re.findall(r"^task 0 epoch \d+: .*$", out, re.M)
    t1 = re.findall(r"^task 1 epoch \d+: .*$", out, re.M)
    assert len(t0) == 1 and len(t1) == 1 and "pod:" not in t0[0]
    m = re.search(r"  pod: (\S+) \((\S+)\)", t1[0])
    assert m, t1[0]
    assert all(math.isfinite(float(v)) and 0.0 < float(v) <= 2.0
               for v in m.groups())
    with_maps = [r for r in requests if r[0]]
    # the student (train mode) and the teacher (eval mode), on every step
    assert with_maps and sum(r[1] for r in with_maps) * 2 == len(with_maps)
    assert signed and all(signed)
    # three taps per backbone pass, task 0 and evaluation included
    assert len(taps) >= 3 * len(requests) and len(taps) % 3 == 0
