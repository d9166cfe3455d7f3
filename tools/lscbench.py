"""Measurements of profiles/lsc_nca.md (needs a GPU).

(a) The kernels of csrc/lsc.hip at (M, C, K) = (128, 100, 10): device events
around REPS back-to-back launches, median of ROUNDS, for lsc_reduce_fwd,
lsc_reduce_bwd, nca_fwd + nca_finalize (one wrapper call) and nca_bwd, and for
ops.lsc_reduce -> ops.nca_loss forward + backward. The baseline is the torch
composition of the same two ops (softmax over the proxies, logsumexp over the
negatives, autograd backward) on the same device and the same cosines.
(b) --engine: imgs/s of task 1 of a --gpu_data synthetic resnet18 run as the
engine prints them (epoch 0 of the task holds the graph capture and is left
out). One run per process; flags for the run follow ``--``, so that a job
script can alternate the PODNet flag set with ``--head cosine`` and cross
entropy on the same build.

Prints one JSON line per measurement.

    python tools/lscbench.py
    python tools/lscbench.py --engine -- --head cosine --nb_proxy 10 \\
        --cls_loss nca --lambda_kd 0 --lambda_pod 3 --lambda_flat 1
    python tools/lscbench.py --engine -- --head cosine
"""
import contextlib
import io
import json
import os
import re
import sys
import time

import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

dev = "cuda:0"
REPS = 50
ROUNDS = 7
SHAPES = ((128, 100, 10),)  # (M, C, K)
GAMMA = 1.0
MARGIN = 0.6


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


def timed(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    return median([ev_time(fn, REPS) for _ in range(ROUNDS)]) * 1e3  # us


def torch_lsc_nca(sims, targets, sigma, K, gamma, margin):
    """The same two ops as a torch composition."""
    M, CK = sims.shape
    s = sims.float().reshape(M, CK // K, K)
    logits = sigma * (torch.softmax(gamma * s, dim=2) * s).sum(dim=2)
    pos = torch.zeros_like(logits, dtype=torch.bool).scatter_(
        1, targets[:, None], True)
    lse = torch.logsumexp(logits.masked_fill(pos, float("-inf")), dim=1)
    h = lse - (logits.gather(1, targets[:, None])[:, 0] - sigma * margin)
    return h.clamp_min(0).sum() / M


def bench_shape(M, C, K):
    from cilfw import ops
    from cilfw import _hip_ops as H
    g = torch.Generator(device=dev).manual_seed(1)
    sg = torch.full((1,), 8.0, device=dev)
    sims = (2 * torch.rand(M, C * K, device=dev, generator=g) - 1
            ).to(torch.bfloat16)
    targets = torch.randint(0, C, (M,), device=dev, generator=g)
    up = torch.ones(1, device=dev)

    logits, yhat = H.lsc_reduce_fwd(sims, sg, K, GAMMA)
    out = H.nca_fwd(logits, targets, sg, MARGIN)
    bufs = dict(h=out[1], active=out[2], lse=out[3], fin=out[4], nact=out[5])
    dl, ds = H.nca_bwd(logits, targets, out[3], out[2], out[4], up)
    dsims, rows = H.lsc_reduce_bwd(sims, yhat, dl, sg, K, GAMMA)
    kres = {}
    for name, fn in {
            "lsc_reduce_fwd": lambda: H.lsc_reduce_fwd(
                sims, sg, K, GAMMA, out=logits, yhat=yhat),
            "lsc_reduce_bwd": lambda: H.lsc_reduce_bwd(
                sims, yhat, dl, sg, K, GAMMA, out=dsims, rows=rows),
            "nca_fwd+finalize": lambda: H.nca_fwd(
                logits, targets, sg, MARGIN, out=bufs),
            "nca_bwd": lambda: H.nca_bwd(
                logits, targets, out[3], out[2], out[4], up, out=dl, dsig=ds),
    }.items():
        kres[name] = round(timed(fn), 2)

    xr = sims.clone().requires_grad_(True)
    sr = sg.clone().requires_grad_(True)

    def hip():
        xr.grad = sr.grad = None
        ops.nca_loss(ops.lsc_reduce(xr, sr, K, GAMMA), targets, sr,
                     MARGIN).backward()

    def composed():
        xr.grad = sr.grad = None
        torch_lsc_nca(xr, targets, sr, K, GAMMA, MARGIN).backward()

    print(json.dumps(dict(
        M=M, C=C, K=K, kernels_us=kres,
        lsc_reduce_nca_loss_fwd_bwd_us=round(timed(hip), 2),
        torch_composition_fwd_bwd_us=round(timed(composed), 2),
        reps=REPS, rounds=ROUNDS)), flush=True)


def engine_ips(flags, epochs=4):
    """imgs/s of the task-1 epochs after the first, as the engine prints."""
    from cilfw.config import parse_args
    from cilfw import engine
    argv = ["--data_set", "synthetic", "--backbone", "resnet18",
            "--synthetic_classes", "100", "--num_bases", "50",
            "--increment", "50", "--synthetic_train_size", "10000",
            "--num_epochs", str(epochs), "--batch_size", "128",
            "--workers", "0", "--memory_size", "2000",
            "--eval_every_epoch", "0", "--no_aug", "--seed", "0",
            "--gpu_data", "--max_tasks", "2"] + list(flags)
    out = io.StringIO()
    t0 = time.time()
    with contextlib.redirect_stdout(out):
        accs = engine.run(parse_args(argv))
    wall = time.time() - t0
    out = out.getvalue()
    assert "capture failed" not in out, out
    ips = [float(v) for v in re.findall(
        r"^task 1 epoch [1-9]\d*: .*imgs/s (\d+)$", out, re.M)]
    return dict(flags=list(flags), task1_imgs_per_s=ips,
                task1_step_ms=[round(128e3 / v, 3) for v in ips],
                acc1s=accs, run_wall_s=round(wall, 2),
                nca_meter=bool(re.search(r"^task 1 .*  nca: ", out, re.M)))


if __name__ == "__main__":
    argv = sys.argv[1:]
    flags = []
    if "--" in argv:
        flags = argv[argv.index("--") + 1:]
        argv = argv[:argv.index("--")]
    sys.path.insert(0, HERE)
    assert torch.cuda.is_available(), "lscbench needs a GPU"
    if "--engine" in argv:
        print(json.dumps(engine_ips(flags)), flush=True)
    else:
        for shape in SHAPES:
            bench_shape(*shape)
