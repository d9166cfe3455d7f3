"""Shared fixtures of the ragged-store tests: lossless PNG files of differing
sizes (so a decode is exact and ``load_image`` is the oracle), and a tiny
ImageFolder tree of them."""

import os

import numpy as np
from PIL import Image

# (H, W) of the stored files: none equal, both orientations, one square pair
SIZES = [(40, 56), (64, 48), (33, 71), (96, 96), (120, 80), (110, 110)]


def write_png(path, h, w, rng, mode="RGB"):
    c = {"L": 1, "RGB": 3, "RGBA": 4}[mode]
    a = rng.integers(0, 256, (h, w, c), dtype=np.uint8)
    im = Image.fromarray(a[:, :, 0] if c == 1 else a)
    assert im.mode == mode
    im.save(path)
    return path


def write_files(root, sizes=SIZES, seed=0, odd_modes=True):
    """One PNG per (H, W) in ``root``; with ``odd_modes`` the second file is
    mode L and the third RGBA (load_image converts both to RGB)."""
    rng = np.random.default_rng(seed)
    os.makedirs(root, exist_ok=True)
    paths = []
    for k, (h, w) in enumerate(sizes):
        mode = {1: "L", 2: "RGBA"}.get(k, "RGB") if odd_modes else "RGB"
        paths.append(write_png(os.path.join(root, f"img{k:03d}.png"), h, w,
                               rng, mode))
    return paths


def write_tree(root, classes=4, per_class=8, val_per_class=3, seed=0):
    """<root>/{train,val}/c<k>/*.png, sizes cycling through SIZES."""
    rng = np.random.default_rng(seed)
    k = 0
    for split, n in (("train", per_class), ("val", val_per_class)):
        for c in range(classes):
            d = os.path.join(root, split, f"c{c}")
            os.makedirs(d, exist_ok=True)
            for i in range(n):
                h, w = SIZES[k % len(SIZES)]
                k += 1
                # class-dependent brightness so the task is learnable at all
                a = rng.integers(0, 128, (h, w, 3), dtype=np.uint8) + 32 * c
                Image.fromarray(a.astype(np.uint8)).save(
                    os.path.join(d, f"{i:03d}.png"))
    return root
