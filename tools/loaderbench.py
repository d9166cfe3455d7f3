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

--ragged measures the path-backed route instead: a RaggedImageStore of
--images random images whose (H, W) follow a fixed seeded ImageNet-like
spread around 375x500 (built on the device, no files), the loader's rrc /
eval rates from it, the crop_resize_ragged kernel alone, and beside both the
DENSE loader and kernel on 375x500 sources in the same process. --ingest N
adds the one-time ingest cost: N generated PNG files (PNG, not JPEG) decoded
and uploaded by RaggedImageStore.from_paths with --workers threads.

Usage: python tools/loaderbench.py [--src 256] [--out_size 224] [--batch 128]
           [--images 2048] [--epochs 5] [--modes pad,rrc,eval]
           [--impl hip,torch] [--dtype bf16]
           [--ragged [--ingest 300] [--workers 16]]
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
    h, w = size if isinstance(size, tuple) else (size, size)
    x = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    return TaskSet(x, np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64))


def loader_rate(mode, impl, args, dtype, loader=None):
    """imgs/s of full epochs (host clock around a device synchronize);
    epoch 0 is warm-up, the rest are reported min / median / max."""
    src = args.out_size if mode == "pad" else args.src
    kw = {} if mode == "pad" else dict(crop_mode=mode, out_size=args.out_size)
    ld = loader if loader is not None else GpuTaskLoader(
        _taskset(args.images, src), args.batch, "cuda", MEAN,
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


def kernel_rate(mode, args, dtype, iters=50, hw=None, store=None):
    """Device-event time of the crop_resize launch alone, one batch, and the
    bytes it has to move: the output it writes plus the source box it reads.
    ``hw``: dense source (Hs, Ws) instead of the square --src; ``store``: a
    RaggedImageStore, timing crop_resize_ragged."""
    from cilfw.data.device_augment import (eval_params, eval_params_ragged,
                                           rrc_params, rrc_params_ragged)
    from cilfw.ops import crop_resize, crop_resize_ragged
    S, B = args.out_size, args.batch
    g = torch.Generator(device="cuda").manual_seed(0)
    Hs, Ws = hw if hw is not None else (args.src, args.src)
    mean = torch.tensor(MEAN, device="cuda") * 255
    std = torch.tensor(STD, device="cuda") * 255
    if store is not None:
        idx = torch.randperm(len(store), device="cuda", generator=g)[:B]
        if mode == "rrc":
            params, flip = rrc_params_ragged(store.hw[idx], S, g)
        else:
            params, flip = eval_params_ragged(store.hw[idx], S)

        def fn():
            return crop_resize_ragged(store.pool, store.offsets, store.hw,
                                      store.channels, idx, params, flip, S,
                                      mean, std, dtype)
    else:
        src = torch.randint(0, 256, (args.images, Hs, Ws, 3),
                            dtype=torch.uint8, device="cuda", generator=g)
        idx = torch.randperm(args.images, device="cuda", generator=g)[:B]
        if mode == "rrc":
            params, flip = rrc_params(B, Hs, Ws, S, g, "cuda")
        else:
            params, flip = eval_params(B, Hs, Ws, S, "cuda")

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


def ragged_sizes(n, seed=0):
    """(n,2) (H, W): a fixed ImageNet-like spread around 375x500 - 70%
    landscape, 30% portrait, side scale uniform in [0.7, 1.3], aspect jitter
    uniform in [0.9, 1.1]."""
    rng = np.random.default_rng(seed)
    f = rng.uniform(0.7, 1.3, n)
    a = rng.uniform(0.9, 1.1, n)
    h = np.rint(375 * f * a).astype(np.int64)
    w = np.rint(500 * f / a).astype(np.int64)
    portrait = rng.random(n) < 0.3
    return np.where(portrait[:, None], np.stack([w, h], 1),
                    np.stack([h, w], 1))


def ragged_store(n):
    """Random-content store with ragged_sizes geometry, filled on the device."""
    from cilfw.data.ragged_store import RaggedImageStore
    hw = ragged_sizes(n)
    sizes = hw[:, 0] * hw[:, 1] * 3
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    g = torch.Generator(device="cuda").manual_seed(0)
    pool = torch.randint(0, 256, (int(sizes.sum()),), dtype=torch.uint8,
                         device="cuda", generator=g)
    return RaggedImageStore(pool, offsets, hw, 3)


def _path_taskset(n):
    names = np.asarray([f"resident/{i}" for i in range(n)], dtype=object)
    return TaskSet(names, np.zeros(n, dtype=np.int64),
                   np.zeros(n, dtype=np.int64))


def _print_loader(tag, r):
    print(f"loader {tag}: {r[0]:9.0f} / {r[len(r) // 2]:9.0f} / "
          f"{r[-1]:9.0f} imgs/s", flush=True)


def _print_kernel(tag, sec, nbytes, batch):
    print(f"kernel {tag}: {sec * 1e6:8.1f} us/batch  "
          f"{batch / sec:10.0f} imgs/s  {nbytes / 1e6:6.1f} MB  "
          f"{nbytes / sec / 1e12:5.2f} TB/s  "
          f"({100 * nbytes / sec / HBM_STREAM:4.1f}% of the 6.29 TB/s "
          f"streaming roofline)", flush=True)


def ingest_rate(n, workers):
    """Decode + upload imgs/s of RaggedImageStore.from_paths on n generated
    PNG files (random content, ragged_sizes geometry) in a temp directory."""
    import tempfile
    from PIL import Image
    from cilfw.data.ragged_store import RaggedImageStore
    rng = np.random.default_rng(1)
    with tempfile.TemporaryDirectory() as d:
        paths = []
        for i, (h, w) in enumerate(ragged_sizes(n, seed=1)):
            p = os.path.join(d, f"{i:05d}.png")
            Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
                            ).save(p, compress_level=1)
            paths.append(p)
        RaggedImageStore.from_paths(paths[:8], "cuda", workers, log=False)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        store = RaggedImageStore.from_paths(paths, "cuda", workers)
        torch.cuda.synchronize()
        sec = time.perf_counter() - t0
    return n / sec, store.nbytes / sec


def run_ragged(args, dtype):
    modes = [m for m in args.modes.split(",") if m != "pad"]
    store = ragged_store(args.images)
    hw = store.hw_host
    print(f"ragged store: {len(store)} images, {store.nbytes / 1e9:.2f} GB, "
          f"H {hw[:, 0].min()}..{hw[:, 0].max()} W {hw[:, 1].min()}.."
          f"{hw[:, 1].max()}, mean {hw[:, 0].mean():.0f}x"
          f"{hw[:, 1].mean():.0f}; dense comparison: 375x500")
    for mode in modes:
        ld = GpuTaskLoader(_path_taskset(args.images), args.batch, "cuda",
                           MEAN, STD, seed=1, augment=mode != "eval",
                           dtype=dtype, crop_mode=mode,
                           out_size=args.out_size, store=store)
        _print_loader(f"{mode:4s} ragged     ",
                      loader_rate(mode, "hip", args, dtype, loader=ld))
    args.src = (375, 500)
    for mode in modes:
        _print_loader(f"{mode:4s} dense375x500",
                      loader_rate(mode, "hip", args, dtype))
    for mode in modes:
        sec, nbytes = kernel_rate(mode, args, dtype, store=store)
        _print_kernel(f"{mode:4s} ragged     ", sec, nbytes, args.batch)
        sec, nbytes = kernel_rate(mode, args, dtype, hw=(375, 500))
        _print_kernel(f"{mode:4s} dense375x500", sec, nbytes, args.batch)
    if args.ingest:
        ips, bps = ingest_rate(args.ingest, args.workers)
        print(f"ingest (PNG files, {args.workers} decode threads, "
              f"{args.ingest} files): {ips:8.0f} imgs/s  "
              f"{bps / 1e6:7.1f} MB/s decoded", flush=True)


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
    ap.add_argument("--ragged", action="store_true",
                    help="measure the ragged-store (path-backed) route")
    ap.add_argument("--ingest", type=int, default=0,
                    help="with --ragged: also time from_paths on N PNG files")
    ap.add_argument("--workers", type=int, default=16,
                    help="decode threads for --ingest")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "loaderbench measures on a GPU"
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    if args.ragged:
        print(f"batch {args.batch}, ragged sources -> {args.out_size}x"
              f"{args.out_size}, {args.dtype}, {args.images} images/epoch, "
              f"{args.epochs} timed epochs (min/median/max)")
        run_ragged(args, dtype)
        sys.exit(0)
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
