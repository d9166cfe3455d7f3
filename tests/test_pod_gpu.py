"""POD-spatial HIP kernels (csrc/pod.hip) against the fp64 oracle of _pod_ref,
and one --gpu_data engine run with --lambda_pod (pytest -m gpu). Shapes,
inputs and allowances are those of _pod_ref; no element is excluded."""

import contextlib
import io
import math
import re

import pytest
import torch

import _pod_ref as R
from cilfw import ops
from cilfw.config import parse_args

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(),
                                 reason="needs GPU")]

DEV = "cuda:0"
_CACHE = {}


def _case(name):
    """Oracle and one device forward + backward per shape, computed once and
    shared (read-only) by the tests."""
    if name not in _CACHE:
        from cilfw import _hip_ops as H
        a, b = R.make_maps(name)
        ref = R.stage_ref(a, b)
        ad, bd = a.to(DEV), b.to(DEV)
        N, Hh, W, C = a.shape
        # NaN-prefilled outputs: an unwritten element shows
        nan32 = torch.full((N, Hh + W, C), float("nan"), device=DEV)
        pooled = H.pod_pool(ad, out=nan32)
        x = ad.clone().requires_grad_(True)
        loss = ops.pod_spatial(x, bd)
        loss.backward()
        loss1, dist, gv = H.pod_dist(pooled, H.pod_pool(bd))
        up = torch.ones(1, device=DEV)
        da_nan = H.pod_bwd(ad, gv, up, out=torch.full_like(ad, float("nan")))
        torch.cuda.synchronize()
        _CACHE[name] = dict(a=a, b=b, ad=ad, bd=bd, ref=ref, pooled=pooled,
                            loss=loss.detach(), loss1=loss1, dist=dist,
                            gv=gv, da=x.grad, da_nan=da_nan)
    return _CACHE[name]


@pytest.mark.parametrize("name", R.SHAPE_IDS)
def test_pool(name):
    c = _case(name)
    N, H, W, C = c["a"].shape
    assert c["pooled"].shape == (N, H + W, C) \
        and c["pooled"].dtype == torch.float32
    r = max(R.worst_pooled(c["pooled"], c["a"]),
            R.worst_pooled(ops.pod_pool(c["bd"]), c["b"]))
    print(f"{name}: pooled err/allowance {r:.4f}")
    assert r <= 1.0


@pytest.mark.parametrize("name", R.SHAPE_IDS)
def test_distance_and_loss(name):
    c = _case(name)
    assert torch.equal(c["loss"], c["loss1"])
    assert torch.equal(ops.pod_dist(c["ad"], c["bd"]), c["dist"])
    r = R.worst_dist(c["dist"], c["loss"], c["ref"])
    print(f"{name}: dist/loss err/allowance {r:.4f}")
    assert r <= 1.0


@pytest.mark.parametrize("name", R.SHAPE_IDS)
def test_gradient(name):
    c = _case(name)
    assert c["da"].dtype == torch.bfloat16 and c["da"].shape == c["a"].shape
    assert torch.equal(c["da"], c["da_nan"])  # NaN prefill fully overwritten
    r = R.worst_grad(c["da"], c["ref"])
    print(f"{name}: da err/allowance {r:.4f} "
          f"(summation share {R.grad_sum_share(c['da'], c['ref']):.4f})")
    assert r <= 1.0


@pytest.mark.parametrize("name", R.SHAPE_IDS)
def test_two_launches_bit_identical(name):
    c = _case(name)
    x = c["ad"].clone().requires_grad_(True)
    loss = ops.pod_spatial(x, c["bd"])
    loss.backward()
    assert torch.equal(ops.pod_pool(c["ad"]), c["pooled"])
    assert torch.equal(loss.detach(), c["loss"])
    assert torch.equal(x.grad, c["da"])


def test_zero_distance():
    """a == b bitwise: loss and gradient exactly zero, also when one sample
    is all zeros."""
    a, _ = R.make_maps("c72")
    for zero_sample in (False, True):
        x = a.clone()
        if zero_sample:
            x[2] = 0
        x = x.to(DEV).requires_grad_(True)
        loss = ops.pod_spatial(x, x.detach().clone())
        loss.backward()
        assert loss.item() == 0.0
        assert torch.isfinite(x.grad.float()).all() and (x.grad == 0).all()
        assert (ops.pod_dist(x, x.detach().clone()) == 0).all()


def test_wrapper_refusals():
    a12 = torch.ones(2, 4, 4, 12, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(AssertionError, match="C % 8 == 0"):
        ops.pod_pool(a12)
    with pytest.raises(AssertionError, match="C % 8 == 0"):
        ops.pod_spatial(a12, a12)
    f32 = torch.ones(2, 4, 4, 16, device=DEV)
    with pytest.raises(AssertionError, match="bf16"):
        ops.pod_pool(f32)
    with pytest.raises(AssertionError, match="bf16"):
        ops.pod_spatial(f32, f32)
    wide = torch.ones(1, 1, 257, 8, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(AssertionError, match="H, W <= 256"):
        ops.pod_pool(wide)


def test_upstream_scaling():
    c = _case("odd_hw")
    x = c["ad"].clone().requires_grad_(True)
    (0.37 * ops.pod_spatial(x, c["bd"])).backward()
    r = R.worst_grad(x.grad, c["ref"], scale=0.37)
    print(f"upstream 0.37: da err/allowance {r:.4f}")
    assert r <= 1.0
    assert R.worst_grad(x.grad, c["ref"], scale=1.0) > 1.0


def _engine_run():
    from cilfw.engine import run
    args = parse_args([
        "--data_set", "synthetic", "--backbone", "resnet20",
        "--synthetic_classes", "10", "--num_bases", "5", "--increment", "5",
        "--num_epochs", "1", "--batch_size", "32", "--workers", "0",
        "--synthetic_train_size", "640", "--memory_size", "40",
        "--eval_every_epoch", "0", "--input_size", "32", "--no_aug",
        "--lr", "0.05", "--seed", "3", "--dtype", "bf16", "--gpu_data",
        "--lambda_pod", "3"])
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        accs = run(args)
    return accs, out.getvalue()


def test_engine_gpu_data_pod_captures_and_repeats():
    """--gpu_data --lambda_pod 3: the run completes with the POD term inside
    the captured step graph, the pod meter is finite on task 1 only, and a
    second identical run repeats it bit for bit."""
    accs, out = _engine_run()
    assert len(accs) == 2
    assert "capture failed" not in out
    t0 = re.findall(r"^task 0 epoch \d+: .*$", out, re.M)
    t1 = re.findall(r"^task 1 epoch \d+: .*$", out, re.M)
    assert len(t0) == 1 and len(t1) == 1 and "pod:" not in t0[0]
    m = re.search(r"  pod: (\S+) \((\S+)\)", t1[0])
    assert m, t1[0]
    assert all(math.isfinite(float(v)) for v in m.groups())
    accs2, out2 = _engine_run()
    assert accs2 == accs
    t1b = re.findall(r"^task 1 epoch \d+: .*$", out2, re.M)
    assert re.search(r"  pod: (\S+) \((\S+)\)", t1b[0]).groups() == m.groups()
