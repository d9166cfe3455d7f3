#!/usr/bin/env python3
"""GpuTaskLoader feed-rate microbench (GPU): iterates the device loader with
no model behind it and prints imgs/s per crop mode, plus the crop_resize
kernel's own time and achieved bytes/s against the streaming roofline.

  pad   zero-pad + random crop + flip at the stored size (small-input path;
        measured here at --out_size so the three rows move the same output)
  rrc   RandomResizedCrop + flip   (one ops.crop_resize launch per batch)
  eval  resize + center-crop       (one ops.crop_resize launch per batch)

--impl torch runs rrc/eval through the pure-torch reference implementation on
the same cuda tensors (CILFW_FORCE_TORCH=1): the "plain torch ops" baseline.

Usage: python tools/loaderbench.py [--src 256] [--out_size 224] [--batch 128]
           [--images 2048] [--epochs 5] [--modes pad,rrc,eval]
           [--impl hip,torch] [--dtype bf16]
"""

import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from cilfw.data.gpu_pipeline import GpuTaskLoader  # noqa: E402
from cilfw.data.scenario import TaskSet  # noqa: E402

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
HBM_STREAM = 6.29e12  # measured float4-copy bandwidth of the MI355X, B/s


def _taskset(n, size):
    rng = np.random.default_rng(0)
    x = rng.integers(0, 256, (n, size, size, 3), dtype=np.uint8)
    return TaskSet(x, np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64))


def loader_rate(mode, impl, args, dtype):
    """imgs/s of full epochs (host clock around a device synchronize);
    epoch 0 is warm-up, the rest are reported min / median / max."""
    src = args.out_size if mode == "pad" else args.src
    kw = {} if mode == "pad" else dict(crop_mode=mode, out_size=args.out_size)
    ld = GpuTaskLoader(_taskset(args.images, src), args.batch, "cuda", MEAN,
                       STD, seed=1, augment=mode != "eval", dtype=dtype, **kw)
    if impl == "torch":
        os.environ["CILFW_FORCE_TORCH"] = "1"
    try:
        rates = []
        for ep in range(args.epochs + 1):
            ld.set_epoch(ep)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = 0
            for imgs, _labels, _ in ld:
                n += imgs.shape[0]
            torch.cuda.synchronize()
            if ep > 0:
                rates.append(n / (time.perf_counter() - t0))
    finally:
        os.environ.pop("CILFW_FORCE_TORCH", None)
    assert imgs.shape == (args.batch, args.out_size, args.out_size, 3)
    return sorted(rates)


def kernel_rate(mode, args, dtype, iters=50):
    """Device-event time of the crop_resize launch alone, one batch, and the
    bytes it has to move: the output it writes plus the source box it reads."""
    from cilfw.data.device_augment import eval_params, rrc_params
    from cilfw.ops import crop_resize
    S, B = args.out_size, args.batch
    g = torch.Generator(device="cuda").manual_seed(0)
    src = torch.randint(0, 256, (args.images, args.src, args.src, 3),
                        dtype=torch.uint8, device="cuda", generator=g)
    idx = torch.randperm(args.images, device="cuda", generator=g)[:B]
    if mode == "rrc":
        params, flip = rrc_params(B, args.src, args.src, S, g, "cuda")
    else:
        params, flip = eval_params(B, args.src, args.src, S, "cuda")
    mean = torch.tensor(MEAN, device="cuda") * 255
    std = torch.tensor(STD, device="cuda") * 255

    def fn():
        return crop_resize(src, idx, params, flip, S, mean, std, dtype)

    for _ in range(5):
        out = fn()
    torch.cuda.synchronize()
    t0 = torch.cuda.Event(enable_timing=True)
    t1 = torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    sec = t0.elapsed_time(t1) / iters * 1e-3
    box = (params[:, 2] * (S - 1) + 1) * (params[:, 3] * (S - 1) + 1) * 3
    nbytes = out.numel() * out.element_size() + float(box.sum().item())
    return sec, nbytes


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--src", type=int, default=256, help="stored image side")
    ap.add_argument("--out_size", type=int, default=224)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--images", type=int, default=2048)
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--modes", default="pad,rrc,eval")
    ap.add_argument("--impl", default="hip,torch")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    args = ap.parse_args()
    assert torch.cuda.is_available(), "loaderbench measures on a GPU"
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    print(f"batch {args.batch}, source {args.src}x{args.src} -> "
          f"{args.out_size}x{args.out_size}, {args.dtype}, {args.images} "
          f"images/epoch, {args.epochs} timed epochs (min/median/max)")
    for mode in args.modes.split(","):
        for impl in args.impl.split(","):
            if mode == "pad" and impl != "hip":
                continue  # pad-crop has one implementation (torch index ops)
            r = loader_rate(mode, impl, args, dtype)
            name = "torch-index" if mode == "pad" else impl
            print(f"loader {mode:4s} {name:11s}: {r[0]:9.0f} / "
                  f"{r[len(r) // 2]:9.0f} / {r[-1]:9.0f} imgs/s", flush=True)
    for mode in args.modes.split(","):
        if mode == "pad" or "hip" not in args.impl.split(","):
            continue
        sec, nbytes = kernel_rate(mode, args, dtype)
        print(f"kernel {mode:4s}: {sec * 1e6:8.1f} us/batch  "
              f"{args.batch / sec:10.0f} imgs/s  {nbytes / 1e6:6.1f} MB  "
              f"{nbytes / sec / 1e12:5.2f} TB/s  "
              f"({100 * nbytes / sec / HBM_STREAM:4.1f}% of the 6.29 TB/s "
              f"streaming roofline)", flush=True)
