"""The pre-ReLU POD tap on the GPU (pytest -m gpu): add_relu_tap_fwd / _bwd
(csrc/norm.hip) against their exact definitions, the tapped block tail
against the existing ops, the POD kernels on signed maps against the fp64
oracle of _pod_ref, and --gpu_data engine runs with --pod_tap pre. Every
kernel value is defined exactly: no tolerance outside the POD comparators."""

import contextlib
import io
import math
import re

import pytest
import torch

import _pod_ref as R
import _pod_tap_ref as T
from cilfw import ops
from cilfw.config import parse_args
from cilfw.ops import functional as CF

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(),
                                 reason="needs GPU")]

DEV = "cuda:0"
BF = torch.bfloat16
_CACHE = {}


def _nan_like(t):
    return torch.full_like(t, float("nan"))


def _case(i):
    """Inputs, CPU definitions and one NaN-prefilled device forward and
    backward per shape, computed once and shared (read-only) by the tests."""
    if i not in _CACHE:
        from cilfw import _hip_ops as H
        a, b, dy, dz = T.tap_inputs(T.TAP_SHAPES[i])
        y_ref, z_ref = T.tap_fwd_ref(a, b)
        ad, bd, dyd, dzd = (t.to(DEV) for t in (a, b, dy, dz))
        y, z = H.add_relu_tap_fwd(ad, bd, out=(_nan_like(ad), _nan_like(ad)))
        g = H.add_relu_tap_bwd(dyd, dzd, z, out=_nan_like(ad))
        g_dy = H.add_relu_tap_bwd(dyd, None, z, out=_nan_like(ad))
        g_dz = H.add_relu_tap_bwd(None, dzd, z, out=_nan_like(ad))
        torch.cuda.synchronize()
        _CACHE[i] = dict(a=a, b=b, dy=dy, dz=dz, ad=ad, bd=bd, dyd=dyd,
                         dzd=dzd, y_ref=y_ref, z_ref=z_ref, y=y, z=z, g=g,
                         g_dy=g_dy, g_dz=g_dz)
    return _CACHE[i]


_SHAPE_PARAMS = pytest.mark.parametrize("i", range(len(T.TAP_SHAPES)),
                                        ids=T.TAP_IDS)


@_SHAPE_PARAMS
def test_forward_exact(i):
    from cilfw import _hip_ops as H
    c = _case(i)
    assert c["y"].shape == c["a"].shape and c["y"].dtype == BF
    assert torch.equal(c["z"].cpu(), c["z_ref"])
    assert torch.equal(c["y"].cpu(), c["y_ref"])
    assert torch.equal(c["y"], H.add_relu_fwd(c["ad"], c["bd"]))
    # the CPU path of the op is the same definition
    y_cpu, z_cpu = ops.add_relu_tap(c["a"], c["b"])
    assert torch.equal(y_cpu, c["y_ref"]) and torch.equal(z_cpu, c["z_ref"])


@_SHAPE_PARAMS
def test_backward_exact(i):
    from cilfw import _hip_ops as H
    c = _case(i)
    z = c["z_ref"]
    assert torch.equal(c["g"].cpu(), T.tap_bwd_ref(c["dy"], c["dz"], z))
    assert torch.equal(c["g_dy"].cpu(), T.tap_bwd_ref(c["dy"], None, z))
    assert torch.equal(c["g_dy"], H.add_relu_bwd(c["dyd"], c["y"]))
    assert torch.equal(c["g_dz"], c["dzd"])


@_SHAPE_PARAMS
def test_autograd_merges_both_gradients(i):
    c = _case(i)
    a = c["ad"].clone().requires_grad_(True)
    b = c["bd"].clone().requires_grad_(True)
    y, z = ops.add_relu_tap(a, b)
    assert torch.equal(y, c["y"]) and torch.equal(z, c["z"])
    # d/dy = w1 = dy and d/dz = w2 = dz, exactly
    ((y * c["dyd"]).sum() + (z * c["dzd"]).sum()).backward()
    assert torch.equal(a.grad, c["g"]) and torch.equal(b.grad, c["g"])
    # one output alone: the other gradient reaches the kernel as a null
    a2 = c["ad"].clone().requires_grad_(True)
    y2, _ = ops.add_relu_tap(a2, c["bd"])
    (y2 * c["dyd"]).sum().backward()
    assert torch.equal(a2.grad, c["g_dy"])
    a3 = c["ad"].clone().requires_grad_(True)
    _, z3 = ops.add_relu_tap(a3, c["bd"])
    (z3 * c["dzd"]).sum().backward()
    assert torch.equal(a3.grad, c["dzd"])


@_SHAPE_PARAMS
def test_two_launches_bit_identical(i):
    from cilfw import _hip_ops as H
    c = _case(i)
    y, z = H.add_relu_tap_fwd(c["ad"], c["bd"])
    assert torch.equal(y, c["y"]) and torch.equal(z, c["z"])
    assert torch.equal(H.add_relu_tap_bwd(c["dyd"], c["dzd"], z), c["g"])


def test_wrapper_refusals():
    from cilfw import _hip_ops as H
    a = torch.ones(2, 4, 4, 8, device=DEV, dtype=BF)
    with pytest.raises(AssertionError, match="bf16"):
        H.add_relu_tap_fwd(a.float(), a.float())
    with pytest.raises(AssertionError, match="add_relu_tap.b"):
        H.add_relu_tap_fwd(a, a[:1])
    with pytest.raises(AssertionError, match="needs dy or dz"):
        H.add_relu_tap_bwd(None, None, a)
    with pytest.raises(AssertionError, match="add_relu_tap_bwd.dz"):
        H.add_relu_tap_bwd(a, a[:1], a)
    with pytest.raises(AssertionError, match="16-byte"):
        H.add_relu_tap_fwd(a.reshape(-1)[1:9], a.reshape(-1)[1:9])


# ----------------------------------------------------------------- block identity

def _blocks():
    from cilfw.models.resnet import BasicBlockB, Bottleneck
    from cilfw.models.resnet_cifar import BasicBlockA
    return {
        "basic_a": (lambda: BasicBlockA(16, 16, 1), 16, "bn_b"),
        "basic_a_down": (lambda: BasicBlockA(16, 32, 2), 16, "bn_b"),
        "basic_b_proj": (lambda: BasicBlockB(64, 128, 2), 64, "bn2"),
        "bottleneck": (lambda: Bottleneck(64, 64, 1), 64, "bn3"),
    }


@pytest.mark.parametrize("name", ["basic_a", "basic_a_down", "basic_b_proj",
                                  "bottleneck"])
def test_block_tail_identity(name):
    """The tapped tail of a block in train mode == add_relu(batchnorm_act(
    conv_out, relu=False), residual) from the existing ops; z is that sum
    before the ReLU, recomputed on the CPU from the bf16 operands."""
    make, cin, bn_name = _blocks()[name]
    torch.manual_seed(0)
    block = make().to(DEV).train()
    x = torch.randn(2, 8, 8, cin, device=DEV).to(BF)
    bn = getattr(block, bn_name)
    seen = []
    h = bn.register_forward_pre_hook(lambda m, inp: seen.append(inp))
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
    y, z = block(x, tap=True)
    h.remove()
    conv_out, residual = seen[0][0], seen[0][1]
    bn_out = CF.batchnorm_act(conv_out, bn.weight, bn.bias, rm0, rv0,
                              bn.momentum, bn.eps, True, relu=False,
                              fuse_bwd=False)
    assert torch.equal(rm0, bn.running_mean) \
        and torch.equal(rv0, bn.running_var)
    assert torch.equal(y, CF.add_relu(bn_out, residual))
    z_cpu = (bn_out.cpu().float() + residual.cpu().float()).to(BF)
    assert (z_cpu < 0).any() and (z_cpu > 0).any()
    assert torch.equal(z.cpu(), z_cpu)
    assert torch.equal(z.clamp_min(0), y)


# ------------------------------------------------------- POD kernels, signed maps

_POD = {}


def _pod_case(name):
    if name not in _POD:
        from cilfw import _hip_ops as H
        a, b = T.signed_maps(name)
        ref = R.stage_ref(a, b)
        ad, bd = a.to(DEV), b.to(DEV)
        N, Hh, W, C = a.shape
        pooled = H.pod_pool(ad, out=torch.full((N, Hh + W, C), float("nan"),
                                               device=DEV))
        x = ad.clone().requires_grad_(True)
        loss = ops.pod_spatial(x, bd)
        loss.backward()
        _POD[name] = dict(a=a, b=b, ad=ad, bd=bd, ref=ref, pooled=pooled,
                          loss=loss.detach(), dist=ops.pod_dist(ad, bd),
                          da=x.grad)
    return _POD[name]


@pytest.mark.parametrize("name", R.SHAPE_IDS)
def test_pod_kernels_on_signed_maps(name):
    """The maps a --pod_tap pre run pools are signed; _pod_ref's allowances
    hold as written (the pooled terms are squares, the gradient allowance
    takes absolute values) and no element is excluded."""
    c = _pod_case(name)
    r_pool = max(R.worst_pooled(c["pooled"], c["a"]),
                 R.worst_pooled(ops.pod_pool(c["bd"]), c["b"]))
    r_dist = R.worst_dist(c["dist"], c["loss"], c["ref"])
    r_grad = R.worst_grad(c["da"], c["ref"])
    print(f"{name} signed: err/allowance pooled {r_pool:.4f} dist "
          f"{r_dist:.4f} da {r_grad:.4f} (da summation share "
          f"{R.grad_sum_share(c['da'], c['ref']):.4f})")
    assert c["da"].dtype == BF and c["da"].shape == c["a"].shape
    assert r_pool <= 1.0 and r_dist <= 1.0 and r_grad <= 1.0


# ------------------------------------------------------------------------ engine

_RUNS = {}


def _engine_run(tap, again=False):
    """test_pod_gpu.py's engine configuration plus --pod_tap; the first run
    of each mode is kept."""
    if tap in _RUNS and not again:
        return _RUNS[tap]
    from cilfw.engine import run
    args = parse_args([
        "--data_set", "synthetic", "--backbone", "resnet20",
        "--synthetic_classes", "10", "--num_bases", "5", "--increment", "5",
        "--num_epochs", "1", "--batch_size", "32", "--workers", "0",
        "--synthetic_train_size", "640", "--memory_size", "40",
        "--eval_every_epoch", "0", "--input_size", "32", "--no_aug",
        "--lr", "0.05", "--seed", "3", "--dtype", "bf16", "--gpu_data",
        "--lambda_pod", "3", "--pod_tap", tap])
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        accs = run(args)
    return _RUNS.setdefault(tap, (accs, out.getvalue()))


def _pod_meter(out):
    t1 = re.findall(r"^task 1 epoch \d+: .*$", out, re.M)
    assert len(t1) == 1
    m = re.search(r"  pod: (\S+) \((\S+)\)", t1[0])
    assert m, t1[0]
    return m.groups()


def test_engine_pre_tap_captures():
    accs, out = _engine_run("pre")
    assert len(accs) == 2
    assert "capture failed" not in out
    t0 = re.findall(r"^task 0 epoch \d+: .*$", out, re.M)
    assert len(t0) == 1 and "pod:" not in t0[0]
    assert all(math.isfinite(float(v)) for v in _pod_meter(out))


def test_engine_pre_tap_repeats():
    accs, out = _engine_run("pre")
    accs2, out2 = _engine_run("pre", again=True)
    assert accs2 == accs
    assert _pod_meter(out2) == _pod_meter(out)


def test_engine_pre_differs_from_post():
    _, out = _engine_run("pre")
    _, out_post = _engine_run("post")
    assert "capture failed" not in out_post
    assert _pod_meter(out_post) != _pod_meter(out)
