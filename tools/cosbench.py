"""Measurements of profiles/cosine_head.md (needs a GPU).

(a) Each kernel of csrc/cosine.hip alone at the three feature widths of the
project (64, 512, 2048), batch 128, with 100 and 1000 classes: device events
around REPS back-to-back launches, median of ROUNDS; the bytes the kernel has
to move, computed from the shape, over that time as a fraction of the
6.29 TB/s copy rate. Next to them ops.cosine_linear and ops.flat_loss,
forward + backward, with the GEMMs of the head included.
(b) --engine: imgs/s of task 1 of a --gpu_data synthetic resnet18 run as the
engine prints them (epoch 0 of the task holds the graph capture and is left
out). One run per process; flags for the run follow ``--``, and ``--tree
DIR`` imports cilfw from another checkout (a build of the parent commit), so
that a job script can alternate the two.

Prints one JSON line per measurement.

    python tools/cosbench.py
    python tools/cosbench.py --engine [--tree DIR] [-- --head cosine ...]
"""
import contextlib
import io
import json
import os
import re
import sys

import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

dev = "cuda:0"
COPY_RATE = 6.29e12  # B/s, achievable HBM copy rate of the MI355X
REPS = 50
ROUNDS = 7
BATCH = 128
WIDTHS = (64, 512, 2048)
CLASSES = (100, 1000)


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


def bench_shape(M, C, D):
    from cilfw import ops
    from cilfw import _hip_ops as H
    g = torch.Generator(device=dev).manual_seed(1)
    x = (torch.randn(M, D, device=dev, generator=g).abs() + 0.1
         ).to(torch.bfloat16)
    t = (torch.randn(M, D, device=dev, generator=g).abs() + 0.1
         ).to(torch.bfloat16)
    w = torch.randn(C, D, device=dev, generator=g)
    sg = torch.full((1,), 3.0, device=dev)
    dy = torch.randn(M, C, device=dev, generator=g).to(torch.bfloat16)
    up = torch.ones(1, device=dev)

    xs, rx = H.rownorm_fwd(x, sg)
    wn, rw = H.rownorm_fwd(w)
    G, sH, _ = H.linear_bwd(dy, xs, wn, False)
    dx, dsr = H.rownorm_bwd(x, rx, G, sg, want_dsig=True)
    dw, _ = H.rownorm_bwd(w, rw, sH)
    _, l, gs = H.flat_dist(x, t)
    ds = H.flat_bwd(gs, up)

    fb, wb = M * D * 2, C * D * 4  # bytes of the features / the weights
    kern = {
        "rownorm_fwd feat": (lambda: H.rownorm_fwd(x, sg, out=xs, rinv=rx),
                             2 * fb),
        "rownorm_fwd w": (lambda: H.rownorm_fwd(w, out=wn, rinv=rw),
                          wb + wb // 2),
        "rownorm_bwd feat": (lambda: H.rownorm_bwd(x, rx, G, sg,
                                                   want_dsig=True, out=dx),
                             3 * fb),
        "rownorm_bwd w": (lambda: H.rownorm_bwd(w, rw, sH, out=dw), 3 * wb),
        "cos_sum": (lambda: H.cos_sum(dsr), M * 4),
        "flat_dist+mean": (lambda: H.flat_dist(x, t, out=gs, rows_out=l),
                           2 * fb + M * D * 4),
        "flat_bwd": (lambda: H.flat_bwd(gs, up, out=ds), M * D * 4 + fb),
    }
    kres = {}
    for name, (fn, nbytes) in kern.items():
        us = timed(fn)
        kres[name] = dict(us=round(us, 2), bytes=nbytes,
                          frac_of_copy_rate=round(
                              nbytes / (us * 1e-6) / COPY_RATE, 4))

    xr = x.clone().requires_grad_(True)
    wr = w.clone().requires_grad_(True)
    sr = sg.clone().requires_grad_(True)

    def head():
        xr.grad = wr.grad = sr.grad = None
        ops.cosine_linear(xr, wr, sr).backward(dy)

    def linear():
        xr.grad = wr.grad = None
        ops.linear(xr, wr).backward(dy)

    def flat():
        xr.grad = None
        ops.flat_loss(xr, t).backward()

    print(json.dumps(dict(
        M=M, C=C, D=D, kernels=kres,
        cosine_linear_fwd_bwd_us=round(timed(head), 2),
        linear_fwd_bwd_us=round(timed(linear), 2),
        flat_loss_fwd_bwd_us=round(timed(flat), 2),
        reps=REPS, rounds=ROUNDS)), flush=True)


def engine_ips(flags, epochs=4):
    """imgs/s of the task-1 epochs after the first, as the engine prints."""
    from cilfw.config import parse_args
    from cilfw.engine import run
    argv = ["--data_set", "synthetic", "--backbone", "resnet18",
            "--synthetic_classes", "100", "--num_bases", "50",
            "--increment", "50", "--synthetic_train_size", "10000",
            "--num_epochs", str(epochs), "--batch_size", "128",
            "--workers", "0", "--memory_size", "2000",
            "--eval_every_epoch", "0", "--no_aug", "--seed", "0",
            "--gpu_data", "--max_tasks", "2"] + list(flags)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        accs = run(parse_args(argv))
    out = out.getvalue()
    assert "capture failed" not in out, out
    ips = [float(v) for v in re.findall(
        r"^task 1 epoch [1-9]\d*: .*imgs/s (\d+)$", out, re.M)]
    return dict(flags=list(flags), task1_imgs_per_s=ips, acc1s=accs,
                flat_meter=bool(re.search(r"^task 1 .*  flat: ", out, re.M)))


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
    assert torch.cuda.is_available(), "cosbench needs a GPU"
    if "--engine" in argv:
        print(json.dumps(dict(tree=os.path.relpath(tree, HERE),
                              **engine_ips(flags))), flush=True)
    else:
        for D in WIDTHS:
            for C in CLASSES:
                bench_shape(BATCH, C, D)
