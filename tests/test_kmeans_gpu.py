"""``kmeans_proxy_kernel`` (csrc/kmeans.hip) against the fp64 reference of
``tests/_kmeans_ref.py`` (run on MI355X: pytest -m gpu).

Every input has a decisive reference (gap / allowance >= 10 at every seeding
step and every assignment, asserted on the CPU in
test_kmeans_oracle_selftest.py), so ``assign`` and ``iters`` must equal the
reference exactly and every proxy element lies within the derived bound.
Outputs are prefilled with NaN / -1; each test prints the largest proxy
err / bound and the smallest reference gap / allowance.

The issue's shape ([7, 40, 257, 600]; 64; 10) contradicts its own rule
n >= K; it is asserted to be refused, and both halves run: K = 10 with the
smallest class at 10 rows, and the listed sizes at K = 7.
"""

import contextlib
import io
import math
import re

import numpy as np
import pytest
import torch

import _kmeans_ref as R
from cilfw import ops
from cilfw.config import parse_args

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(),
                                 reason="needs GPU")]

DEV = "cuda"


def _H():
    from cilfw.ops._backend import ext
    return ext()


def _raw(f, sizes, K, max_iter):
    """The raw launch on prefilled outputs -> CPU (proxies, assign, iters)."""
    fd = f.to(DEV).contiguous()
    so = torch.tensor(R.seg_offsets(sizes), dtype=torch.int32, device=DEV)
    n, D, C = f.shape[0], f.shape[1], len(sizes)
    out = (torch.full((C * K, D), float("nan"), device=DEV),
           torch.full((n,), -1, dtype=torch.int32, device=DEV),
           torch.full((C,), -1, dtype=torch.int32, device=DEV))
    got = _H().kmeans_proxies(fd, so, K, max_iter, out=out)
    assert all(a is b for a, b in zip(got, out))
    return tuple(t.cpu() for t in got)


@pytest.mark.parametrize("name", list(R.CASES))
def test_launch_vs_fp64(name):
    f, sizes, K, max_iter, refs = R.case(name)
    out = _raw(f, sizes, K, max_iter)
    R.check(refs, sizes, K, out, f"kmeans_proxies {name}")
    norms = out[0].double().norm(dim=1)
    assert (norms - 1).abs().max().item() <= 2 * R.U * (R.depth(f.shape[1])
                                                         + 4)
    # the public op on device features: the same launch
    pub = ops.kmeans_proxies(f.to(DEV), R.seg_offsets(sizes), K, max_iter)
    assert all(t.device.type == "cuda" for t in pub)
    assert all(torch.equal(a.cpu(), b) for a, b in zip(pub, out))
    # a rerun is bit-identical
    again = _raw(f, sizes, K, max_iter)
    assert all(torch.equal(a, b) for a, b in zip(again, out)), "rerun differs"


def test_n_equals_K_and_iteration_limits():
    for name in ("1x4x1", "5x4x5"):
        f, sizes, K, max_iter, refs = R.case(name)
        _, assign, iters = _raw(f, sizes, K, max_iter)
        assert iters.tolist() == [1]
        assert sorted(assign.tolist()) == list(range(K))
    assert [r["iters"] for r in R.case("iter1")[4]] == [1, 1, 1, 1]
    assert max(r["iters"] for r in R.case("iter2")[4]) == 2
    assert max(r["iters"] for r in R.case("batch_D64_K7")[4]) > 2


def test_emptied_centre_keeps_its_value():
    f, sizes, K, max_iter, refs = R.case("3x4x3_dup_empty")
    assert refs[0]["emptied"]
    prox, assign, iters = _raw(f, sizes, K, max_iter)
    assert assign.tolist() == [0, 0, 1] and iters.tolist() == [2]
    assert torch.equal(prox[2], prox[0])  # both are bit copies of row A


@pytest.mark.parametrize("name", ["batch_D64_K10", "batch_D64_K7", "D300_K6"])
def test_class_alone_equals_class_in_batch(name):
    f, sizes, K, max_iter, _ = R.case(name)
    prox, assign, iters = _raw(f, sizes, K, max_iter)
    o = 0
    for c, n in enumerate(sizes):
        p1, a1, i1 = _raw(f[o:o + n], [n], K, max_iter)
        assert torch.equal(p1, prox[c * K:(c + 1) * K]), f"class {c}"
        assert torch.equal(a1, assign[o:o + n]), f"class {c}"
        assert i1.item() == iters[c].item(), f"class {c}"
        o += n


class _CountingLib:
    """Stands in for ``_hip_ops._lib``: the shape queries go to the real
    library, every other entry point counts its calls and does nothing."""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        if name.endswith("_supported"):
            return getattr(self.real, name)

        def fn(*a):
            self.calls.append(name)
            return 0
        return fn


def test_refusals_launch_nothing(monkeypatch):
    H = _H()
    lib = _CountingLib(H._lib)
    monkeypatch.setattr(H, "_lib", lib)
    f = R.blobs(24, 8, 3, 77).to(DEV)
    so = torch.tensor([0, 10, 24], dtype=torch.int32, device=DEV)

    for bad in (float("nan"), float("inf"), -float("inf"), 2.0 ** 49):
        g = f.clone()
        g[13, 5] = bad
        with pytest.raises(ValueError, match="finite"):
            H.kmeans_proxies(g, so, 3, 10)
        with pytest.raises(ValueError, match="finite"):
            ops.kmeans_proxies(g, [0, 10, 24], 3)
    with pytest.raises(ValueError, match=r"segment\(s\) \[0\] hold fewer"):
        H.kmeans_proxies(f, so, 11, 10)
    with pytest.raises(ValueError, match=r"segment\(s\) \[0\] hold fewer"):
        ops.kmeans_proxies(f, [0, 10, 24], 11)
    # the issue's shape: a 7-row class cannot give 10 centres
    f7, sizes7 = R.case("batch_D64_K7")[:2]
    with pytest.raises(ValueError, match=r"segment\(s\) \[0\] hold fewer"):
        ops.kmeans_proxies(f7.to(DEV), R.seg_offsets(sizes7), 10)
    with pytest.raises(ValueError, match="kmeans_supported"):
        H.kmeans_proxies(f, so, 17, 10)
    with pytest.raises(ValueError, match="kmeans_supported"):
        H.kmeans_proxies(f[:, :6].contiguous(), so, 3, 10)      # D % 4
    big = torch.ones(32, 1004, device=DEV)
    with pytest.raises(ValueError, match="kmeans_supported"):
        H.kmeans_proxies(big, torch.tensor([0, 32], dtype=torch.int32,
                                           device=DEV), 16, 10)  # K D
    with pytest.raises(ValueError, match="max_iter"):
        H.kmeans_proxies(f, so, 3, 0)
    with pytest.raises(ValueError, match="fp32"):
        H.kmeans_proxies(f.double(), so, 3, 10)
    with pytest.raises(ValueError, match="contiguous"):
        H.kmeans_proxies(f.t().contiguous().t(), so, 3, 10)
    with pytest.raises(ValueError, match="on the GPU"):
        H.kmeans_proxies(f.cpu(), so.cpu(), 3, 10)
    with pytest.raises(ValueError, match="seg_off"):
        H.kmeans_proxies(f, so.long(), 3, 10)
    with pytest.raises(ValueError, match="from 0 to n"):
        H.kmeans_proxies(f, torch.tensor([0, 10, 25], dtype=torch.int32,
                                         device=DEV), 3, 10)
    with pytest.raises(ValueError, match="from 0 to n"):
        H.kmeans_proxies(f, torch.tensor([0, 30, 24], dtype=torch.int32,
                                         device=DEV), 3, 10)
    with pytest.raises(ValueError, match="out must hold"):
        H.kmeans_proxies(f, so, 3, 10, out=(torch.empty(6, 8, device=DEV),
                                            torch.empty(24, device=DEV),
                                            torch.empty(2, device=DEV)))
    assert lib.calls == [], f"launched: {lib.calls}"
    # and the stand-in does count: valid input reaches the entry point
    H.kmeans_proxies(f, so, 3, 10)
    assert lib.calls == ["cilfw_kmeans_proxies"]


# ---------------------------------------------------------------------- engine

def _engine_run(extra=()):
    from cilfw.engine import run
    args = parse_args([
        "--data_set", "synthetic", "--backbone", "resnet20",
        "--synthetic_classes", "10", "--num_bases", "5", "--increment", "5",
        "--num_epochs", "1", "--batch_size", "32", "--workers", "0",
        "--synthetic_train_size", "640", "--memory_size", "40",
        "--eval_every_epoch", "0", "--input_size", "32", "--no_aug",
        "--lr", "0.05", "--seed", "3", "--dtype", "bf16", "--gpu_data",
        "--head", "cosine", "--nb_proxy", "3", "--cls_loss", "nca",
        "--lambda_kd", "0", "--lambda_pod", "3", "--lambda_flat", "1",
        "--proxy_init", "kmeans", *extra])
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        accs = run(args)
    return accs, out.getvalue()


def test_engine_podnet_with_kmeans_init_repeats():
    """--gpu_data with the PODNet flag set and --proxy_init kmeans: two tasks
    complete, the second task's proxies come from the kernel (one line
    says so), the meters are finite and a second run repeats them bit for
    bit."""
    accs, out = _engine_run()
    assert len(accs) == 2
    init = re.findall(r"^proxy init: task (\d+): (\d+) new head rows set to "
                      r"k-means centres, mean old norm (\S+), iterations "
                      r"(\d+)\.\.(\d+)$", out, re.M)
    assert len(init) == 1 and init[0][:2] == ("1", "15")
    assert math.isfinite(float(init[0][2])) and float(init[0][2]) > 0
    assert 1 <= int(init[0][3]) <= int(init[0][4]) <= 100
    lines = re.findall(r"^task \d+ epoch \d+: .*$", out, re.M)
    assert len(lines) == 2
    for line in lines:
        m = re.search(r"  nca: (\S+) \((\S+)\)", line)
        assert m and all(math.isfinite(float(v)) for v in m.groups()), line
    accs2, out2 = _engine_run()
    assert accs2 == accs

    def meters(text):
        keep = re.findall(r"^(?:task \d+ epoch \d+|proxy init): .*$", text,
                          re.M)
        return [re.sub(r"imgs/s \d+", "", v) for v in keep]
    assert meters(out) == meters(out2)
