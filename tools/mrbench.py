"""Measurements of profiles/margin_rank.md (needs a GPU).

(a) The kernels of csrc/mrank.hip at batch 128 with 100 and 1000 classes, of
which 90 and 900 known, k = 2: device events around REPS back-to-back
launches, median of ROUNDS, for mrank_fwd + mrank_finalize (one wrapper call)
and mrank_bwd, and for ops.margin_rank_loss forward + backward. The baseline
is the torch composition of the same loss (topk + gather + clamp, autograd
backward) on the same device and the same logits.
(b) --engine: imgs/s of task 1 of a --gpu_data synthetic resnet18 run as the
engine prints them (epoch 0 of the task holds the graph capture and is left
out), and the wall time of the imprint pass where --imprint is among the
flags. One run per process; flags for the run follow ``--``, and ``--tree
DIR`` imports cilfw from another checkout (a build of the parent commit), so
that a job script can alternate the two.

Prints one JSON line per measurement.

    python tools/mrbench.py
    python tools/mrbench.py --engine [--tree DIR] [-- --head cosine ...]
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
SHAPES = ((128, 100, 90, 2), (128, 1000, 900, 2))  # (M, C, known, k)
MARGIN = 0.5


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


def torch_margin_rank(logits, targets, sigma, known, k, margin):
    """The same loss as a torch composition: syncs the host to pick the old
    rows, allocates by their count, tie order unspecified."""
    z = logits.float() / sigma
    old = targets < known
    zo = z[old]
    a = zo.gather(1, targets[old][:, None])
    n = zo[:, known:].topk(k, dim=1).values
    return (margin - (a - n)).clamp_min(0).sum() / max(zo.shape[0] * k, 1)


def bench_shape(M, C, known, k):
    from cilfw import ops
    from cilfw import _hip_ops as H
    g = torch.Generator(device=dev).manual_seed(1)
    sg = torch.full((1,), 3.0, device=dev)
    logits = (3.0 * (2 * torch.rand(M, C, device=dev, generator=g) - 1)
              ).to(torch.bfloat16)
    targets = torch.randint(0, C, (M,), device=dev, generator=g)
    up = torch.ones(1, device=dev)

    out = H.mrank_fwd(logits, targets, sg, known, k, MARGIN)
    bufs = dict(sel=out[1], fin=out[2], nold=out[3], rho=out[4], dsum=out[5],
                old=out[6])
    dl, ds = H.mrank_bwd(out[1], targets, out[2], up, C, known)
    kres = {}
    for name, fn in {
            "mrank_fwd+finalize": lambda: H.mrank_fwd(
                logits, targets, sg, known, k, MARGIN, out=bufs),
            "mrank_bwd": lambda: H.mrank_bwd(
                out[1], targets, out[2], up, C, known, out=dl, dsig=ds),
    }.items():
        kres[name] = round(timed(fn), 2)

    lr = logits.clone().requires_grad_(True)
    sr = sg.clone().requires_grad_(True)

    def hip():
        lr.grad = sr.grad = None
        ops.margin_rank_loss(lr, targets, sr, known, k, MARGIN).backward()

    def composed():
        lr.grad = sr.grad = None
        torch_margin_rank(lr, targets, sr, known, k, MARGIN).backward()

    print(json.dumps(dict(
        M=M, C=C, known=known, k=k, kernels_us=kres,
        margin_rank_loss_fwd_bwd_us=round(timed(hip), 2),
        torch_composition_fwd_bwd_us=round(timed(composed), 2),
        reps=REPS, rounds=ROUNDS)), flush=True)


def engine_ips(flags, epochs=4):
    """imgs/s of the task-1 epochs after the first, as the engine prints, and
    the wall time of the imprint pass (None without --imprint)."""
    from cilfw.config import parse_args
    from cilfw import engine
    argv = ["--data_set", "synthetic", "--backbone", "resnet18",
            "--synthetic_classes", "100", "--num_bases", "50",
            "--increment", "50", "--synthetic_train_size", "10000",
            "--num_epochs", str(epochs), "--batch_size", "128",
            "--workers", "0", "--memory_size", "2000",
            "--eval_every_epoch", "0", "--no_aug", "--seed", "0",
            "--gpu_data", "--max_tasks", "2"] + list(flags)
    imprint_s = []
    orig = getattr(engine, "imprint_new_classes", None)
    if orig is not None:
        def timed_imprint(*a, **kw):
            torch.cuda.synchronize()
            t0 = time.time()
            r = orig(*a, **kw)
            torch.cuda.synchronize()
            imprint_s.append(round(time.time() - t0, 4))
            return r
        engine.imprint_new_classes = timed_imprint
    out = io.StringIO()
    t0 = time.time()
    with contextlib.redirect_stdout(out):
        accs = engine.run(parse_args(argv))
    wall = time.time() - t0
    out = out.getvalue()
    assert "capture failed" not in out, out
    ips = [float(v) for v in re.findall(
        r"^task 1 epoch [1-9]\d*: .*imgs/s (\d+)$", out, re.M)]
    return dict(flags=list(flags), task1_imgs_per_s=ips, acc1s=accs,
                run_wall_s=round(wall, 2), imprint_pass_s=imprint_s or None,
                mr_meter=bool(re.search(r"^task 1 .*  mr: ", out, re.M)))


if __name__ == "__main__":
    argv = sys.argv[1:]
    flags = []
    if "--" in argv:
        flags = argv[argv.index("--") + 1:]
        argv = argv[:argv.index("--")]
    tree = HERE
    if "--tree" in argv:
        tree = os.path.abspath(argv[argv.index("--tree") + 1])
    sys.path.insert(0, tree)
    assert torch.cuda.is_available(), "mrbench needs a GPU"
    if "--engine" in argv:
        print(json.dumps(dict(tree=os.path.relpath(tree, HERE),
                              **engine_ips(flags))), flush=True)
    else:
        for shape in SHAPES:
            bench_shape(*shape)
