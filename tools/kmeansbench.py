"""Measurements of profiles/kmeans_init.md (needs a GPU).

(a) ``ops.kmeans_proxies``: the one launch (device events around the raw
wrapper's call into preallocated outputs, 2 warm-up launches, median and
minimum of 7) next to the project's CPU path on the same input (host clock,
one run), at the CIFAR shape (10 classes x 500 rows x 512, K = 10) and the
ImageNet-100 shape (100 x 1300 x 512, K = 10). The rows are rectified noise
around 20 directions per class, so that ten centres do not fit at once and
Lloyd runs for tens of iterations.

(b) ``--engine``: full PODNet on synthetic_hard, 50 -> 100 classes in steps
of 10, ``--proxy_init random`` against ``kmeans``, same seed, one child
process per arm; prints each arm's per-task accuracy, its first-epoch nca
meter of every task and its "proxy init" lines.

    python tools/kmeansbench.py
    python tools/kmeansbench.py --engine [--epochs 3]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from cilfw import ops  # noqa: E402

dev = "cuda:0"


def rows(C, n, D, ndir, seed):
    g = torch.Generator().manual_seed(seed)
    dirs = torch.relu(torch.randn(C, ndir, D, generator=g))
    which = torch.randint(0, ndir, (C, n), generator=g)
    x = dirs[torch.arange(C)[:, None], which] \
        + 0.5 * torch.randn(C, n, D, generator=g)
    return (torch.relu(x) + 0.01).reshape(C * n, D)


def part_a(C, n, D, K, max_iter=100):
    from cilfw.ops._backend import ext
    H = ext()
    f = rows(C, n, D, 20, 1)
    fd = f.to(dev)
    off = list(range(0, C * n + 1, n))
    so = torch.tensor(off, dtype=torch.int32, device=dev)
    out = (torch.empty(C * K, D, device=dev),
           torch.empty(C * n, dtype=torch.int32, device=dev),
           torch.empty(C, dtype=torch.int32, device=dev))
    for _ in range(2):
        H.kmeans_proxies(fd, so, K, max_iter, out=out)
    torch.cuda.synchronize()
    ts = []
    for _ in range(7):
        a, b = torch.cuda.Event(True), torch.cuda.Event(True)
        a.record()
        H.kmeans_proxies(fd, so, K, max_iter, out=out)
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    t0 = time.perf_counter()
    cp, ca, ci = ops.kmeans_proxies(f, off, K, max_iter)
    cpu_s = time.perf_counter() - t0
    it = out[2].cpu()
    print(json.dumps(dict(
        shape=[C, n, D, K], gpu_ms_median=ts[len(ts) // 2], gpu_ms_min=ts[0],
        cpu_path_s=cpu_s, iters_min=int(it.min()), iters_max=int(it.max()),
        iters_mean=float(it.float().mean()),
        assign_agree_with_cpu_path=(out[1].cpu() == ca).float().mean().item(),
        iters_equal_cpu_path=bool(torch.equal(it, ci)))), flush=True)


BASE = [
    "--data_set", "synthetic_hard", "--backbone", "resnet32",
    "--synthetic_classes", "100", "--num_bases", "50", "--increment", "10",
    "--batch_size", "128", "--workers", "0",
    "--synthetic_train_size", "50000", "--memory_size", "2000",
    "--eval_every_epoch", "0", "--input_size", "32", "--gpu_data",
    "--seed", "0", "--no_aug",
    "--head", "cosine", "--nb_proxy", "10", "--cls_loss", "nca",
    "--lambda_kd", "0", "--lambda_pod", "3", "--lambda_flat", "1"]


def part_b(epochs):
    for arm in ("random", "kmeans"):
        cmd = [sys.executable, os.path.join(REPO, "template.py"), *BASE,
               "--num_epochs", str(epochs), "--proxy_init", arm]
        p = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True)
        out = p.stdout
        accs = re.findall(r"^task id = \d+  @Acc1 = (\S+),", out, re.M)
        first = re.findall(r"^task (\d+) epoch 0: .*?  nca: (\S+) ", out, re.M)
        init = re.findall(r"^proxy init: .*$", out, re.M)
        print(json.dumps(dict(arm=arm, rc=p.returncode, epochs=epochs,
                              acc1=[float(a) for a in accs],
                              first_epoch_nca=first, proxy_init=init)),
              flush=True)
        if p.returncode != 0:
            print(out[-3000:], p.stderr[-3000:], flush=True)
            sys.exit(p.returncode)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--engine", action="store_true")
    ap.add_argument("--epochs", type=int, default=3)
    o = ap.parse_args()
    if o.engine:
        part_b(o.epochs)
    else:
        part_a(10, 500, 512, 10)
        part_a(100, 1300, 512, 10)
