"""Measurements of profiles/pod_loss.md (needs a GPU).

(a) Forward + backward of ops.pod_spatial on the stage shapes of resnet18 at
32 px / batch 128 and resnet50 at 224 px / batch 64: the HIP path against the
same definition in torch ops on the device (CILFW_FORCE_TORCH=1), the two
alternating in one process, device events around REPS back-to-back
forward+backward calls, 3 warm-up calls each. Outputs of the two paths are
compared on the timed inputs.
(b) Each kernel alone (pod_pool, pod_dist, pod_bwd): device events around
REPS back-to-back launches; the bytes the kernel has to move, computed from
the shape, over that time, as a fraction of the 6.29 TB/s copy rate.
(c) --engine: imgs/s of task 1 of a --gpu_data synthetic resnet18 run with
--lambda_pod 0 and --lambda_pod 3, alternating, as the engine prints them
(epoch 0 of the task holds the graph capture and is left out).
(d) --tap-kernels: add_relu_tap_fwd / _bwd (the pre-ReLU tap of --pod_tap
pre) next to add_relu_fwd / _bwd on the maps the tap really runs on: the
CIFAR-ResNet stages and the resnet18 small-input stages at batch 128. The
four alternate in one process; per kernel the median, the least and the most
of ROUNDS timings of REPS back-to-back launches, the bytes it has to move and
the time ratio tap / plain next to the byte ratio (4/3 both ways).
(e) --engine --pod_tap pre: as (c), but --lambda_pod 3 in both runs and
--pod_tap post against --pod_tap pre, alternating.

Prints one JSON line per measurement.

    python tools/podbench.py                          # (a) and (b)
    python tools/podbench.py --engine                 # (c)
    python tools/podbench.py --tap-kernels            # (d)
    python tools/podbench.py --engine --pod_tap pre   # (e)
"""
import contextlib
import io
import json
import os
import re
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cilfw import ops  # noqa: E402

dev = "cuda:0"
COPY_RATE = 6.29e12  # B/s, achievable HBM copy rate of the MI355X
REPS = 50
ROUNDS = 7

SHAPES = [("rn18/32px/b128 s1", (128, 32, 32, 64)),
          ("rn18/32px/b128 s2", (128, 16, 16, 128)),
          ("rn18/32px/b128 s3", (128, 8, 8, 256)),
          ("rn18/32px/b128 s4", (128, 4, 4, 512)),
          ("rn50/224px/b64 s1", (64, 56, 56, 256)),
          ("rn50/224px/b64 s2", (64, 28, 28, 512)),
          ("rn50/224px/b64 s3", (64, 14, 14, 1024)),
          ("rn50/224px/b64 s4", (64, 7, 7, 2048))]


def ev_time(fn, reps):
    """ms per call over ``reps`` back-to-back calls."""
    a, b = torch.cuda.Event(True), torch.cuda.Event(True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def median(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2]


@contextlib.contextmanager
def force_torch(on):
    old = os.environ.pop("CILFW_FORCE_TORCH", None)
    if on:
        os.environ["CILFW_FORCE_TORCH"] = "1"
    try:
        yield
    finally:
        os.environ.pop("CILFW_FORCE_TORCH", None)
        if old is not None:
            os.environ["CILFW_FORCE_TORCH"] = old


def bench_shape(name, shape):
    from cilfw import _hip_ops as H
    N, Hh, W, C = shape
    g = torch.Generator(device=dev).manual_seed(1)
    a = (torch.randn(shape, device=dev, generator=g).abs() + 0.1
         ).to(torch.bfloat16).requires_grad_(True)
    b = (torch.randn(shape, device=dev, generator=g).abs() + 0.1
         ).to(torch.bfloat16)

    def fwd_bwd():
        a.grad = None
        loss = ops.pod_spatial(a, b)
        loss.backward()
        return loss.detach(), a.grad

    def run(torch_path):
        with force_torch(torch_path):
            return fwd_bwd()

    for _ in range(3):
        run(False), run(True)
    torch.cuda.synchronize()
    th, tt = [], []
    for _ in range(ROUNDS):  # alternate the two
        th.append(ev_time(lambda: run(False), REPS))
        tt.append(ev_time(lambda: run(True), REPS))
    lh, gh = run(False)
    lt, gt = run(True)
    gdiff = (gh.float() - gt.float()).abs().max().item() \
        / gt.float().abs().max().item()

    # kernels alone
    map_b = N * Hh * W * C * 2
    pool_b = N * (Hh + W) * C * 4
    ad = a.detach()
    vs, vt = H.pod_pool(ad), H.pod_pool(b)
    gv = H.pod_dist(vs, vt)[2]
    up = torch.ones(1, device=dev)
    da = torch.empty_like(ad)
    kern = {"pod_pool": (lambda: H.pod_pool(ad, out=vs), map_b + pool_b),
            "pod_dist": (lambda: H.pod_dist(vs, vt), 3 * pool_b),
            "pod_bwd": (lambda: H.pod_bwd(ad, gv, up, out=da),
                        2 * map_b + pool_b)}
    kres = {}
    for kname, (fn, nbytes) in kern.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        t = median([ev_time(fn, REPS) for _ in range(ROUNDS)])
        kres[kname] = dict(us=t * 1e3, bytes=nbytes,
                           frac_of_copy_rate=nbytes / (t * 1e-3) / COPY_RATE)
    print(json.dumps(dict(
        shape=name, nhwc=shape, groups_per_block=H.pod_pool_groups(W, C),
        hip_us_median=median(th) * 1e3, hip_us_min=min(th) * 1e3,
        torch_us_median=median(tt) * 1e3, torch_us_min=min(tt) * 1e3,
        speedup_median=median(tt) / median(th),
        loss_hip=lh.item(), loss_torch=lt.item(), grad_rel_maxdiff=gdiff,
        kernels=kres, reps=REPS, rounds=ROUNDS)), flush=True)


TAP_SHAPES = [("cifar/b128 s1", (128, 32, 32, 16)),
              ("cifar/b128 s2", (128, 16, 16, 32)),
              ("cifar/b128 s3", (128, 8, 8, 64)),
              ("rn18/32px/b128 s1", (128, 32, 32, 64)),
              ("rn18/32px/b128 s2", (128, 16, 16, 128)),
              ("rn18/32px/b128 s3", (128, 8, 8, 256)),
              ("rn18/32px/b128 s4", (128, 4, 4, 512))]


def bench_tap(name, shape):
    from cilfw import _hip_ops as H
    g = torch.Generator(device=dev).manual_seed(2)
    a, b, dy, dz = (torch.randn(shape, device=dev, generator=g
                                ).to(torch.bfloat16) for _ in range(4))
    y, z = H.add_relu_tap_fwd(a, b)
    assert torch.equal(y, H.add_relu_fwd(a, b))
    assert torch.equal(H.add_relu_tap_bwd(dy, None, z),
                       H.add_relu_bwd(dy, y))
    out2, out1 = (torch.empty_like(a), torch.empty_like(a)), \
        torch.empty_like(a)
    map_b = a.numel() * 2
    kern = {"add_relu_fwd": (lambda: H.add_relu_fwd(a, b), 3 * map_b),
            "add_relu_tap_fwd": (lambda: H.add_relu_tap_fwd(a, b, out=out2),
                                 4 * map_b),
            "add_relu_bwd": (lambda: H.add_relu_bwd(dy, y), 3 * map_b),
            "add_relu_tap_bwd": (lambda: H.add_relu_tap_bwd(dy, dz, z,
                                                            out=out1),
                                 4 * map_b)}
    for fn, _ in kern.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in kern}
    for _ in range(ROUNDS):  # alternate the four
        for k, (fn, _) in kern.items():
            ts[k].append(ev_time(fn, REPS))
    res = {k: dict(us_median=median(t) * 1e3, us_min=min(t) * 1e3,
                   us_max=max(t) * 1e3, bytes=kern[k][1],
                   frac_of_copy_rate=kern[k][1] / (median(t) * 1e-3)
                   / COPY_RATE) for k, t in ts.items()}
    print(json.dumps(dict(
        shape=name, nhwc=shape, kernels=res, byte_ratio=4 / 3,
        fwd_time_ratio=median(ts["add_relu_tap_fwd"])
        / median(ts["add_relu_fwd"]),
        bwd_time_ratio=median(ts["add_relu_tap_bwd"])
        / median(ts["add_relu_bwd"]),
        reps=REPS, rounds=ROUNDS)), flush=True)


def engine_ips(lambda_pod, epochs=4, pod_tap=None):
    """imgs/s of the task-1 epochs after the first, as the engine prints."""
    from cilfw.config import parse_args
    from cilfw.engine import run
    argv = ["--data_set", "synthetic", "--backbone", "resnet18",
            "--synthetic_classes", "100", "--num_bases", "50",
            "--increment", "50", "--synthetic_train_size", "10000",
            "--num_epochs", str(epochs), "--batch_size", "128",
            "--workers", "0", "--memory_size", "2000",
            "--eval_every_epoch", "0", "--no_aug", "--seed", "0",
            "--gpu_data", "--max_tasks", "2"]
    if lambda_pod:
        argv += ["--lambda_pod", str(lambda_pod)]
    if pod_tap is not None:
        argv += ["--pod_tap", pod_tap]
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        run(parse_args(argv))
    out = out.getvalue()
    assert "capture failed" not in out, out
    ips = [float(v) for v in re.findall(
        r"^task 1 epoch [1-9]\d*: .*imgs/s (\d+)$", out, re.M)]
    return dict(lambda_pod=lambda_pod, pod_tap=pod_tap or "post",
                task1_imgs_per_s=ips,
                pod_meter=bool(re.search(r"^task 1 .*  pod: ", out, re.M)))


if __name__ == "__main__":
    assert torch.cuda.is_available(), "podbench needs a GPU"
    if "--pod_tap" in sys.argv:
        tap = sys.argv[sys.argv.index("--pod_tap") + 1]
        assert tap in ("post", "pre") and "--engine" in sys.argv, \
            "--pod_tap post|pre goes with --engine"
        other = "post" if tap == "pre" else "pre"
        for t in (other, tap, other, tap):
            print(json.dumps(engine_ips(3, pod_tap=t)), flush=True)
    elif "--engine" in sys.argv:
        for lam in (0, 3, 0, 3):
            print(json.dumps(engine_ips(lam)), flush=True)
    elif "--tap-kernels" in sys.argv:
        for name, shape in TAP_SHAPES:
            bench_tap(name, shape)
    else:
        for name, shape in SHAPES:
            bench_shape(name, shape)
