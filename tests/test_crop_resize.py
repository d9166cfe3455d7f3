"""ops.crop_resize (CPU reference path), its parameter samplers, and the
GpuTaskLoader / engine wiring of the large-input crop modes.

The oracle for the resampling is the HOST pipeline: transforms._resize
(scipy.ndimage.zoom order=1, then clip + uint8 truncation). The two agree
except on floor ties: the host interpolates in double, the op in fp32, and
where the exact value is an integer one of them can land a hair below it.
That is at most ONE level on a small share of pixels; a wrong coordinate map
shows up as differences of many levels.
"""

import numpy as np
import pytest
import torch

from cilfw.data import transforms as T
from cilfw.data.device_augment import eval_params, rrc_params
from cilfw.data.gpu_pipeline import GpuTaskLoader
from cilfw.data.scenario import TaskSet
from cilfw.ops import crop_resize

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)


def _box_row(y, x, h, w, S):
    return [float(y), float(x), (h - 1) / (S - 1), (w - 1) / (S - 1)]


def _host_overshoots(n, S):
    """scipy's zoom walks coordinate j*((n-1)/(S-1)) in double; for a few
    (n, S) the last one rounds to just ABOVE n-1, which zoom treats as outside
    the image and fills with 0 (a black last row/column in the host output).
    That is the oracle's own error, so such extents are not drawn."""
    return (S - 1) * ((n - 1) / (S - 1)) > n - 1


def _levels_close(got, want):
    d = (got.astype(np.int64) - want.astype(np.int64))
    return int(np.abs(d).max()), float((d != 0).mean())


def test_matches_host_resize_on_random_boxes():
    rng = np.random.default_rng(11)
    worst, ndiff, ntot = 0, 0, 0
    for k in range(60):
        S = (8, 16, 24, 33)[k % 4]
        Hs, Ws = int(rng.integers(9, 41)), int(rng.integers(9, 41))
        if Hs == Ws:
            Ws = Ws + 1 if Ws < 40 else Ws - 1
        img = rng.integers(0, 256, (Hs, Ws, 3), dtype=np.uint8)
        if k % 5 == 0:
            img[:] = rng.integers(0, 256)
        while True:
            h, w = int(rng.integers(2, Hs + 1)), int(rng.integers(2, Ws + 1))
            if not (_host_overshoots(h, S) or _host_overshoots(w, S)):
                break
        y, x = int(rng.integers(0, Hs - h + 1)), int(rng.integers(0, Ws - w + 1))
        want = T._resize(img[y:y + h, x:x + w], S)
        got = crop_resize(torch.from_numpy(img)[None], None,
                          torch.tensor([_box_row(y, x, h, w, S)]),
                          torch.zeros(1, dtype=torch.uint8), S)[0].numpy()
        assert got.shape == want.shape == (S, S, 3) and got.dtype == np.uint8
        if k % 5 == 0:  # constant image: a + t*(b - a) is exact
            assert np.array_equal(got, want)
        d = np.abs(got.astype(np.int64) - want.astype(np.int64))
        worst = max(worst, int(d.max()))
        ndiff += int((d != 0).sum())
        ntot += d.size
    print(f"worst {worst} level(s), {100.0 * ndiff / ntot:.3f}% of "
          f"{ntot} pixels differ")
    assert worst <= 1
    assert ndiff / ntot <= 0.02


def _random_case(seed=3, M=5, Hs=20, Ws=28, S=16, C=3):
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(0, 256, (M, Hs, Ws, C), dtype=torch.uint8, generator=g)
    params, _ = rrc_params(M, Hs, Ws, S, g, "cpu")
    return src, params


def test_flip_reverses_width_exactly():
    src, params = _random_case()
    n = src.shape[0]
    plain = crop_resize(src, None, params, torch.zeros(n, dtype=torch.uint8),
                        16)
    flipped = crop_resize(src, None, params, torch.ones(n, dtype=torch.uint8),
                          16)
    assert torch.equal(flipped, plain.flip(2))
    mixed = crop_resize(src, None, params,
                        torch.tensor([0, 1, 0, 1, 1], dtype=torch.uint8), 16)
    assert torch.equal(mixed[0], plain[0]) and torch.equal(mixed[1],
                                                           flipped[1])


def test_identity_scale_returns_the_crop():
    src, _ = _random_case()
    S = 16
    params = torch.tensor([[2.0, 7.0, 1.0, 1.0], [4.0, 12.0, 1.0, 1.0],
                           [0.0, 0.0, 1.0, 1.0]])
    idx = torch.tensor([4, 0, 4])
    out = crop_resize(src, idx, params, torch.zeros(3, dtype=torch.uint8), S)
    assert torch.equal(out[0], src[4, 2:18, 7:23])
    assert torch.equal(out[1], src[0, 4:20, 12:28])
    assert torch.equal(out[2], src[4, 0:16, 0:16])


def _args(size):
    class A:
        input_size = size
    return A()


@pytest.mark.parametrize("Hs,Ws", [(40, 40), (36, 48)])
def test_eval_params_match_eval_transform(Hs, Ws):
    S = 28  # R = int(256/224*28) = 32
    rng = np.random.default_rng(Hs + Ws)
    img = rng.integers(0, 256, (Hs, Ws, 3), dtype=np.uint8)
    host = T.EvalTransform(_args(S), "imagenet")
    host.small = False  # the large-input branch, at a test-sized S
    want = host(img)  # normalized fp32 (S,S,3)
    want_u8 = torch.round(want * host.std * 255 + host.mean * 255).numpy()
    params, flip = eval_params(1, Hs, Ws, S, "cpu")
    got = crop_resize(torch.from_numpy(img)[None], None, params, flip,
                      S)[0].numpy()
    worst, share = _levels_close(got, want_u8)
    print(f"eval {Hs}x{Ws}: worst {worst}, {100 * share:.3f}% differ")
    assert worst <= 1 and share <= 0.02


def test_eval_params_short_side_already_r_is_exact():
    S, R = 28, 32
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (R, 45, 3), dtype=np.uint8)
    params, flip = eval_params(2, R, 45, S, "cpu")
    assert torch.equal(params[0, 2:], torch.tensor([1.0, 1.0]))
    got = crop_resize(torch.from_numpy(img)[None], torch.tensor([0, 0]),
                      params, flip, S)
    want = torch.from_numpy(T._center_crop(img, S).copy())
    assert torch.equal(got[0], want) and torch.equal(got[1], want)


def test_normalized_mode_is_the_loader_expression():
    src, params = _random_case()
    n = src.shape[0]
    flip = torch.tensor([0, 1, 0, 1, 1], dtype=torch.uint8)
    mean255 = torch.tensor(MEAN) * 255.0
    std255 = torch.tensor(STD) * 255.0
    u8 = crop_resize(src, None, params, flip, 16)
    f32 = crop_resize(src, None, params, flip, 16, mean255, std255,
                      torch.float32)
    assert f32.dtype == torch.float32 and f32.shape == (n, 16, 16, 3)
    assert torch.equal(f32, (u8.float() - mean255) / std255)
    bf = crop_resize(src, None, params, flip, 16, mean255, std255,
                     torch.bfloat16)
    assert bf.dtype == torch.bfloat16 and torch.equal(bf, f32.bfloat16())


def test_single_and_four_channel_sources():
    g = torch.Generator().manual_seed(1)
    for C in (1, 4):
        src = torch.randint(0, 256, (2, 12, 15, C), dtype=torch.uint8,
                            generator=g)
        params = torch.tensor([[1.0, 2.0, 1.0, 1.0], [0.0, 0.0, 1.0, 1.0]])
        out = crop_resize(src, None, params,
                          torch.zeros(2, dtype=torch.uint8), 9)
        assert torch.equal(out[0], src[0, 1:10, 2:11])
        assert torch.equal(out[1], src[1, 0:9, 0:9])


# ------------------------------------------------------------- rrc_params

def _boxes(params, S):
    y, x = params[:, 0], params[:, 1]
    h = params[:, 2] * (S - 1) + 1
    w = params[:, 3] * (S - 1) + 1
    return y, x, h, w


def test_rrc_boxes_lie_inside_the_source():
    g = torch.Generator().manual_seed(0)
    for Hs, Ws in ((20, 28), (37, 23), (9, 13)):
        params, flip = rrc_params(2048, Hs, Ws, 16, g, "cpu")
        assert params.shape == (2048, 4) and params.dtype == torch.float32
        assert flip.shape == (2048,) and flip.dtype == torch.uint8
        y, x, h, w = _boxes(params, 16)
        assert torch.equal(y, y.floor()) and torch.equal(x, x.floor())
        assert (y >= 0).all() and (x >= 0).all()
        assert (h >= 1 - 1e-4).all() and (w >= 1 - 1e-4).all()
        assert (y + h <= Hs + 1e-3).all() and (x + w <= Ws + 1e-3).all()
        # the sampler is not degenerate: boxes vary in size and position
        assert h.round().unique().numel() > 3 and y.unique().numel() > 3


def test_rrc_full_scale_unit_ratio_is_the_full_image():
    g = torch.Generator().manual_seed(0)
    params, _ = rrc_params(64, 20, 20, 16, g, "cpu", scale=(1.0, 1.0),
                           ratio=(1.0, 1.0))
    want = torch.tensor([0.0, 0.0, 19 / 15, 19 / 15]).expand(64, 4)
    assert torch.equal(params, want)


def test_rrc_never_fitting_falls_back_to_center_crop():
    g = torch.Generator().manual_seed(0)
    params, _ = rrc_params(64, 20, 28, 16, g, "cpu", scale=(4.0, 4.0))
    want = torch.tensor([0.0, 4.0, 19 / 15, 19 / 15]).expand(64, 4)
    assert torch.equal(params, want)
    params, _ = rrc_params(8, 37, 23, 16, g, "cpu", scale=(4.0, 4.0))
    assert torch.equal(params, torch.tensor([7.0, 0.0, 22 / 15, 22 / 15])
                       .expand(8, 4))


def test_rrc_flip_rate_and_seed_determinism():
    g = torch.Generator().manual_seed(7)
    p1, f1 = rrc_params(4096, 20, 28, 16, g, "cpu")
    assert abs(f1.float().mean().item() - 0.5) <= 0.05
    g.manual_seed(7)
    p2, f2 = rrc_params(4096, 20, 28, 16, g, "cpu")
    assert torch.equal(p1, p2) and torch.equal(f1, f2)


# ------------------------------------------------------------------ loader

def _taskset(n=40, H=20, W=28):
    rng = np.random.default_rng(0)
    x = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    y = rng.integers(0, 5, n).astype(np.int64)
    return TaskSet(x, y, np.zeros(n, dtype=np.int64))


def test_loader_rrc_shapes_and_epoch_determinism():
    ld = GpuTaskLoader(_taskset(), 8, "cpu", MEAN, STD, seed=2,
                       dtype=torch.float32, crop_mode="rrc", out_size=16)
    ld.set_epoch(0)
    a = [(i.clone(), l.clone()) for i, l, _ in ld]
    b = [(i.clone(), l.clone()) for i, l, _ in ld]
    assert len(a) == 5
    for (ia, la), (ib, lb) in zip(a, b):
        assert ia.shape == (8, 16, 16, 3) and ia.dtype == torch.float32
        assert torch.isfinite(ia).all()
        assert torch.equal(ia, ib) and torch.equal(la, lb)
    ld.set_epoch(1)
    c = [i for i, _, _ in ld]
    assert not torch.equal(torch.cat(c), torch.cat([i for i, _ in a]))


def test_loader_eval_mode_is_resize_center_crop():
    ts = _taskset(n=10, H=40, W=40)
    ld = GpuTaskLoader(ts, 4, "cpu", MEAN, STD, shuffle=False, augment=False,
                       drop_last=False, dtype=torch.float32,
                       crop_mode="eval", out_size=28)
    imgs = torch.cat([i for i, _, _ in ld])
    assert imgs.shape == (10, 28, 28, 3)
    params, flip = eval_params(10, 40, 40, 28, "cpu")
    want = crop_resize(torch.from_numpy(ts.x), None, params, flip, 28,
                       torch.tensor(MEAN) * 255, torch.tensor(STD) * 255,
                       torch.float32)
    assert torch.equal(imgs, want)


def test_loader_rrc_with_augment_pipeline_crops_first():
    """RandAugment/jitter run on the already cropped out_size images (host
    order), erasing after the normalize."""
    from cilfw.data.device_augment import DeviceAugment
    seen = []

    class Spy(DeviceAugment):
        def __call__(self, imgs, g):
            seen.append((tuple(imgs.shape), imgs.dtype))
            return super().__call__(imgs, g)

    aug = Spy(aa_policy="rand-m9-mstd0.5-inc1", color_jitter=0.4,
              reprob=0.25)
    ld = GpuTaskLoader(_taskset(), 8, "cpu", MEAN, STD, seed=2,
                       dtype=torch.float32, crop_mode="rrc", out_size=16,
                       aug_pipeline=aug)
    batches = [i for i, _, _ in ld]
    assert seen == [((40, 16, 16, 3), torch.uint8)]
    assert len(batches) == 5
    assert all(b.shape == (8, 16, 16, 3) and torch.isfinite(b).all()
               for b in batches)


def test_loader_pad_mode_is_the_default_bit_for_bit():
    ts = _taskset(n=40, H=16, W=16)
    for augment in (True, False):
        old = GpuTaskLoader(ts, 8, "cpu", MEAN, STD, seed=4, augment=augment,
                            dtype=torch.float32)
        new = GpuTaskLoader(ts, 8, "cpu", MEAN, STD, seed=4, augment=augment,
                            dtype=torch.float32, crop_mode="pad",
                            out_size=None)
        for (ia, la, _), (ib, lb, _) in zip(old, new):
            assert torch.equal(ia, ib) and torch.equal(la, lb)


# ------------------------------------------------------------------ engine

@pytest.mark.timeout(300)
def test_engine_large_input_gpu_data_on_cpu(monkeypatch):
    """--gpu_data --input_size 72: train (rrc), val and feature-extraction
    (eval) loaders all go through crop_resize; the run completes with finite
    accuracies."""
    import cilfw.data.gpu_pipeline as gp
    from cilfw import ops
    from cilfw.config import parse_args
    from cilfw.engine import run
    monkeypatch.setenv("CILFW_GPU_DATA_ON_CPU", "1")
    modes = []
    real = ops.crop_resize

    def spy(src, idx, params, flip, out_size, *a, **k):
        modes.append((tuple(src.shape[1:3]), out_size))
        return real(src, idx, params, flip, out_size, *a, **k)

    monkeypatch.setattr(ops, "crop_resize", spy)
    made = []
    real_init = gp.GpuTaskLoader.__init__

    def init_spy(self, *a, **k):
        made.append((k.get("crop_mode"), k.get("out_size")))
        real_init(self, *a, **k)

    monkeypatch.setattr(gp.GpuTaskLoader, "__init__", init_spy)
    args = parse_args([
        "--data_set", "synthetic", "--backbone", "resnet18",
        "--synthetic_classes", "4", "--num_bases", "2", "--increment", "2",
        "--num_epochs", "1", "--batch_size", "8", "--workers", "0",
        "--synthetic_train_size", "32", "--memory_size", "8",
        "--eval_every_epoch", "0", "--input_size", "72", "--gpu_data",
        "--lr", "0.01", "--seed", "1",
    ])
    accs = run(args)
    assert len(accs) == 2 and all(np.isfinite(a) for a in accs)
    assert ("rrc", 72) in made and ("eval", 72) in made
    assert ("pad", 72) not in made and (None, None) not in made
    assert modes and all(m == ((72, 72), 72) for m in modes)
