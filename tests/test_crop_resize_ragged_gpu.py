"""HIP crop_resize_ragged kernel (csrc/data.hip) against its CPU oracle
(ops.crop_resize_ragged on CPU tensors), against the dense kernel on uniform
sizes, the ragged loader on the GPU, and one path-backed engine run
(pytest -m gpu).

Tolerances are those of tests/test_crop_resize_gpu.py, for the same reason:
the kernel and the oracle evaluate the same fp32 expression, so the only
licensed difference is a floor tie moved by a differently rounded product,
i.e. ONE level on a small share of pixels:
  uint8 mode         max |diff| <= 1 level, <= 2% of pixels differ
  fp32 normalized    the same after de-normalizing (out*std255 + mean255),
                     with 1e-3 slack for that fp32 round trip
  bf16 normalized    de-normalized |diff| <= 1.6 levels (1 for the tie plus
                     half a bf16 ulp at |x| < 4 times the largest std255)

The pool holds six images of different sizes between 64 guard bytes of 255 on
either side (offsets[0] = 64). At S=5 a sample is 75 (C=3), 25 (C=1) or 100
(C=4) elements; the lanes own 16 / 8 / 4 of them (u8 / bf16 / fp32), so in
nearly every mode lanes straddle two samples of different H, W and base, and
the last vector is partial.
"""

import numpy as np
import pytest
import torch

import _ragged_tree as RT
from cilfw.data.device_augment import eval_params_ragged, rrc_params_ragged
from cilfw.data.gpu_pipeline import GpuTaskLoader
from cilfw.data.scenario import TaskSet
from cilfw.ops import crop_resize, crop_resize_ragged

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(),
                                 reason="needs GPU")]

MEAN = (0.5071, 0.4865, 0.4409)
STD = (0.2673, 0.2564, 0.2761)
SIZES = [(9, 13), (37, 23), (1, 7), (5, 1), (21, 18), (2, 2)]
IDX = [3, 0, 5, 4, 1, 1, 2]
FLIP = [0, 1, 1, 0, 1, 0, 1]
# (y, x, h, w) per output sample, inside image IDX[n]: whole images, a 2x2
# box, h=1 and w=1 boxes, boxes touching the far borders
BOXES = [(0, 0, 5, 1),      # 5x1   whole image (w=1)
         (0, 0, 9, 13),     # 9x13  whole image
         (0, 0, 2, 2),      # 2x2   whole image = a 2x2 box
         (19, 16, 2, 2),    # 21x18 2x2 box in the far corner
         (30, 0, 7, 23),    # 37x23 bottom band
         (5, 3, 1, 17),     # 37x23 h=1 box
         (0, 0, 1, 7)]      # 1x7   whole image (h=1)
GUARD = 64
N = len(IDX)


def _box(y, x, h, w, S):
    return [float(y), float(x), (h - 1) / (S - 1), (w - 1) / (S - 1)]


def _pool(sizes, C, seed):
    g = torch.Generator().manual_seed(seed)
    imgs = [torch.randint(0, 256, (h, w, C), dtype=torch.uint8, generator=g)
            for h, w in sizes]
    guard = torch.full((GUARD,), 255, dtype=torch.uint8)
    pool = torch.cat([guard] + [i.reshape(-1) for i in imgs] + [guard])
    lens = [i.numel() for i in imgs]
    offs = torch.tensor([GUARD + sum(lens[:m]) for m in range(len(imgs))],
                        dtype=torch.int64)
    hw = torch.tensor(sizes, dtype=torch.int32)
    return imgs, pool, offs, hw


_cache = {}


def _inputs_and_oracle(C, S, sizes=None):
    """CPU inputs + the u8 oracle levels, computed once per case."""
    key = (C, S, sizes is None)
    if key not in _cache:
        sz = SIZES if sizes is None else sizes
        imgs, pool, offs, hw = _pool(sz, C, seed=100 * C + S)
        assert offs[0] == GUARD
        if sizes is None:
            boxes = BOXES
        else:  # uniform 21x18 sources: the dense test's boxes
            boxes = [(0, 0, 21, 18), (2, 3, 9, 14), (11, 1, 10, 17),
                     (0, 9, 21, 9), (19, 16, 2, 2), (4, 4, 13, 13),
                     (1, 0, 19, 18)]
        params = torch.tensor([_box(*b, S) for b in boxes])
        idx = torch.tensor(IDX)
        flip = torch.tensor(FLIP, dtype=torch.uint8)
        mean255 = torch.tensor(MEAN[:C] if C <= 3 else MEAN + (0.5,)) * 255
        std255 = torch.tensor(STD[:C] if C <= 3 else STD + (0.25,)) * 255
        want = crop_resize_ragged(pool, offs, hw, C, idx, params, flip, S)
        _cache[key] = (imgs, pool, offs, hw, idx, params, flip, mean255,
                       std255, want)
    return _cache[key]


def _dev(*ts):
    return tuple(t.cuda() for t in ts)


CASES = [(3, 5), (3, 16), (3, 33), (1, 5), (4, 5)]


@pytest.mark.parametrize("C,S", CASES)
def test_kernel_matches_cpu_oracle(C, S):
    (_, pool, offs, hw, idx, params, flip, mean255, std255,
     want) = _inputs_and_oracle(C, S)
    a = _dev(pool, offs, hw) + (C,) + _dev(idx, params, flip) + (S,)

    got = crop_resize_ragged(*a)
    assert got.dtype == torch.uint8 and got.shape == (N, S, S, C)
    d = (got.cpu().int() - want.int()).abs()
    print(f"C={C} S={S} u8: worst {int(d.max())}, "
          f"{100 * (d != 0).float().mean():.3f}% differ")
    assert d.max() <= 1 and (d != 0).float().mean() <= 0.02

    levels = want.float()
    m, s = _dev(mean255, std255)
    got = crop_resize_ragged(*a, m, s, torch.float32)
    assert got.dtype == torch.float32 and got.shape == (N, S, S, C)
    d = (got.cpu() * std255 + mean255 - levels).abs()
    print(f"C={C} S={S} f32: worst {float(d.max()):.5f}")
    assert d.max() <= 1 + 1e-3 and (d > 1e-3).float().mean() <= 0.02

    got = crop_resize_ragged(*a, m, s, torch.bfloat16)
    assert got.dtype == torch.bfloat16 and got.shape == (N, S, S, C)
    d = (got.cpu().float() * std255 + mean255 - levels).abs()
    print(f"C={C} S={S} bf16: worst {float(d.max()):.5f}")
    assert d.max() <= 1.6


def test_guard_bytes_are_never_sampled():
    """All-zero images between 255 guards: any read outside an image's own
    bytes (a stale row stride, clamp limit or base after a sample change)
    shows as a non-zero output."""
    S, C = 5, 3
    _, pool, offs, hw, idx, params, flip, _, _, _ = _inputs_and_oracle(C, S)
    pool = pool.clone()
    pool[GUARD:-GUARD] = 0
    got = crop_resize_ragged(*_dev(pool, offs, hw), C,
                             *_dev(idx, params, flip), S)
    assert int(got.max()) == 0


def test_out_of_range_idx_is_clamped_like_the_dense_kernel():
    S, C = 16, 3
    _, pool, offs, hw, _, _, flip, _, _, _ = _inputs_and_oracle(C, S)
    M = len(SIZES)
    bad = torch.tensor([M, -1, 5, 10 ** 12, -10 ** 12, 0, M + 3])
    ok = bad.clamp(0, M - 1)
    params, _ = eval_params_ragged(hw[ok], S)
    dp, do, dh, df, dpar = _dev(pool, offs, hw, flip, params)
    got = crop_resize_ragged(dp, do, dh, C, bad.cuda(), dpar, df, S)
    want = crop_resize_ragged(dp, do, dh, C, ok.cuda(), dpar, df, S)
    assert torch.equal(got, want)
    # ... which is what the dense kernel does with the same indices
    src = torch.randint(0, 256, (M, 8, 9, C), dtype=torch.uint8).cuda()
    assert torch.equal(crop_resize(src, bad.cuda(), dpar, df, S),
                       crop_resize(src, ok.cuda(), dpar, df, S))


def test_two_launches_are_bit_identical():
    S, C = 33, 3
    (_, pool, offs, hw, idx, params, flip, mean255, std255,
     _) = _inputs_and_oracle(C, S)
    a = _dev(pool, offs, hw) + (C,) + _dev(idx, params, flip) + (S,)
    n = _dev(mean255, std255) + (torch.bfloat16,)
    one, two = crop_resize_ragged(*a, *n), crop_resize_ragged(*a, *n)
    assert torch.equal(one.view(torch.int16), two.view(torch.int16))
    assert torch.equal(crop_resize_ragged(*a), crop_resize_ragged(*a))


@pytest.mark.parametrize("S", [5, 33])
def test_uniform_sizes_are_bit_identical_to_the_dense_kernel(S):
    C = 3
    (imgs, pool, offs, hw, idx, params, flip, mean255, std255,
     _) = _inputs_and_oracle(C, S, sizes=[(21, 18)] * 6)
    src = torch.stack(imgs).cuda()
    a = _dev(pool, offs, hw) + (C,) + _dev(idx, params, flip) + (S,)
    b = (src,) + _dev(idx, params, flip) + (S,)
    m, s = _dev(mean255, std255)
    assert torch.equal(crop_resize_ragged(*a), crop_resize(*b))
    assert torch.equal(crop_resize_ragged(*a, m, s, torch.float32),
                       crop_resize(*b, m, s, torch.float32))
    assert torch.equal(
        crop_resize_ragged(*a, m, s, torch.bfloat16).view(torch.int16),
        crop_resize(*b, m, s, torch.bfloat16).view(torch.int16))


def test_ragged_loader_matches_cpu_through_the_oracle(tmp_path):
    """The loader's rrc / eval batches from a mixed-size PNG tree are
    crop_resize_ragged of its store with its own parameter rows: copy the
    rows sampled on the device to the CPU and replay them through the
    oracle (device and CPU generators are different streams)."""
    from cilfw.data.ragged_store import RaggedImageStore
    paths = RT.write_files(str(tmp_path), sizes=RT.SIZES * 4)
    n = len(paths)
    ts = TaskSet(np.asarray(paths, dtype=object),
                 np.arange(n, dtype=np.int64) % 5, np.zeros(n, np.int64))
    cpu = RaggedImageStore.from_paths(paths, "cpu", workers=4, log=False)
    mean255, std255 = torch.tensor(MEAN) * 255, torch.tensor(STD) * 255
    for mode in ("rrc", "eval"):
        ld = GpuTaskLoader(ts, 8, "cuda", MEAN, STD, seed=5, shuffle=False,
                           augment=mode == "rrc", dtype=torch.bfloat16,
                           crop_mode=mode, out_size=16, workers=4)
        assert torch.equal(ld.images.pool.cpu(), cpu.pool)
        g = torch.Generator(device="cuda")
        g.manual_seed(ld.seed * 1000003 + ld.epoch * 131 + ld.rank)
        batches = list(ld)
        assert len(batches) == 3
        for b, (imgs, labels, _) in enumerate(batches):
            assert imgs.shape == (8, 16, 16, 3)
            assert imgs.dtype == torch.bfloat16 and imgs.is_cuda
            idx = torch.arange(b * 8, b * 8 + 8)
            hw = ld.images.hw[idx.cuda()]
            if mode == "rrc":
                params, flip = rrc_params_ragged(hw, 16, g)
            else:
                params, flip = eval_params_ragged(hw, 16)
            levels = crop_resize_ragged(cpu.pool, cpu.offsets, cpu.hw, 3,
                                        idx, params.cpu(), flip.cpu(),
                                        16).float()
            d = (imgs.cpu().float() * std255 + mean255 - levels).abs()
            assert d.max() <= 1.6, (mode, b, float(d.max()))
            assert torch.equal(labels.cpu(),
                               torch.from_numpy(ts.y[idx.numpy()]))


@pytest.mark.timeout(300)
def test_engine_path_backed_gpu_data_run(tmp_path, capsys):
    """--gpu_data --input_size 96 on an ImageFolder tree of mixed-size PNGs,
    end to end on the HIP path (bf16). The store lines show that the device
    path engaged, not the host-loader fallback."""
    from cilfw.config import parse_args
    from cilfw.engine import run
    RT.write_tree(str(tmp_path))
    args = parse_args([
        "--data_set", "imagenet100", "--data_path", str(tmp_path),
        "--backbone", "resnet18", "--num_bases", "2", "--increment", "2",
        "--num_epochs", "1", "--batch_size", "8", "--workers", "2",
        "--memory_size", "8", "--eval_every_epoch", "0",
        "--input_size", "96", "--gpu_data", "--lr", "0.01", "--seed", "1",
        "--dtype", "bf16",
    ])
    accs = run(args)
    assert len(accs) == 2 and all(np.isfinite(a) for a in accs)
    log = capsys.readouterr().out
    assert "loss:" in log and "nan" not in log.lower(), log
    lines = [ln for ln in log.splitlines()
             if ln.startswith("[gpu_data] ragged store:")]
    assert [ln.split()[3] for ln in lines] == ["16", "6", "24", "12"], log
    assert all("(cuda" in ln for ln in lines)
