"""HIP crop_resize kernel (csrc/data.hip) against its CPU oracle
(ops.crop_resize on CPU tensors), the loader's crop modes on the GPU, and one
large-input engine run (pytest -m gpu).

Tolerances. The kernel and the oracle evaluate the same fp32 expression; the
only licensed difference is a floor tie moved by a differently rounded
product, i.e. ONE level on a small share of pixels:
  uint8 mode         max |diff| <= 1 level, <= 2% of pixels differ
  fp32 normalized    the same after de-normalizing (out*std255 + mean255),
                     with 1e-3 slack for that fp32 round trip
  bf16 normalized    de-normalized |diff| <= 1.6 levels: 1 for the tie plus
                     0.54 = half an ulp of bf16 at |x| < 4 (2^-7) times the
                     largest std255 (0.2761 * 255)
"""

import numpy as np
import pytest
import torch

from cilfw.data.device_augment import eval_params, rrc_params
from cilfw.data.gpu_pipeline import GpuTaskLoader
from cilfw.data.scenario import TaskSet
from cilfw.ops import crop_resize

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(),
                                 reason="needs GPU")]

MEAN = (0.5071, 0.4865, 0.4409)
STD = (0.2673, 0.2564, 0.2761)
N = 7


def _box(y, x, h, w, S):
    return [float(y), float(x), (h - 1) / (S - 1), (w - 1) / (S - 1)]


def _case(name, S):
    """(src uint8 CPU, idx, params, flip) - N=7 output samples each."""
    g = torch.Generator().manual_seed(len(name) * 100 + S)

    def src(M, Hs, Ws, C=3):
        return torch.randint(0, 256, (M, Hs, Ws, C), dtype=torch.uint8,
                             generator=g)

    flip = torch.tensor([0, 1, 1, 0, 1, 0, 1], dtype=torch.uint8)
    idx = torch.tensor([3, 0, 3, 4, 1, 1, 2])  # repeats, out of order
    if name == "upsample_9x13":  # source smaller than S
        boxes = [(0, 0, 9, 13), (1, 2, 7, 9), (0, 5, 9, 8), (4, 0, 5, 13),
                 (3, 3, 2, 2), (0, 0, 4, 6), (2, 1, 6, 11)]
        return src(5, 9, 13), idx, boxes, flip
    if name == "borders_37x23":  # boxes touching every border, and h=w=2
        boxes = [(0, 0, 37, 23), (0, 4, 20, 19), (17, 0, 20, 11),
                 (30, 16, 7, 7), (35, 21, 2, 2), (0, 0, 2, 2), (5, 3, 29, 17)]
        return src(5, 37, 23), idx, boxes, flip
    if name == "c4":
        boxes = [(0, 0, 21, 18), (2, 3, 9, 14), (11, 1, 10, 17),
                 (0, 9, 21, 9), (19, 16, 2, 2), (4, 4, 13, 13), (1, 0, 19, 18)]
        return src(5, 21, 18, 4), idx, boxes, flip
    if name == "c1_identity_idx":  # idx=None: identity gather, N == M
        boxes = [(0, 0, 21, 18), (2, 3, 9, 14), (11, 1, 10, 17),
                 (0, 9, 21, 9), (19, 16, 2, 2), (4, 4, 13, 13), (1, 0, 19, 18)]
        return src(N, 21, 18, 1), None, boxes, flip
    raise KeyError(name)


CASES = [(n, S) for n in ("upsample_9x13", "borders_37x23")
         for S in (16, 33)] + [("c4", 33), ("c1_identity_idx", 16)]

_oracle_cache = {}


def _inputs_and_oracle(name, S):
    """CPU inputs + the three oracle outputs, computed once per case."""
    key = (name, S)
    if key not in _oracle_cache:
        src, idx, boxes, flip = _case(name, S)
        params = torch.tensor([_box(*b, S) for b in boxes])
        C = src.shape[-1]
        mean255 = torch.tensor(MEAN[:C] if C <= 3 else MEAN + (0.5,)) * 255
        std255 = torch.tensor(STD[:C] if C <= 3 else STD + (0.25,)) * 255
        want = {
            "u8": crop_resize(src, idx, params, flip, S),
            "f32": crop_resize(src, idx, params, flip, S, mean255, std255,
                               torch.float32),
        }
        _oracle_cache[key] = (src, idx, params, flip, mean255, std255, want)
    return _oracle_cache[key]


def _dev(t):
    return None if t is None else t.cuda()


@pytest.mark.parametrize("name,S", CASES)
def test_kernel_matches_cpu_op(name, S):
    src, idx, params, flip, mean255, std255, want = _inputs_and_oracle(name, S)
    a = (_dev(src), _dev(idx), _dev(params), _dev(flip), S)
    C = src.shape[-1]

    got = crop_resize(*a)
    assert got.dtype == torch.uint8 and got.shape == (N, S, S, C)
    d = (got.cpu().int() - want["u8"].int()).abs()
    print(f"{name} S={S} u8: worst {int(d.max())}, "
          f"{100 * (d != 0).float().mean():.3f}% differ")
    assert d.max() <= 1 and (d != 0).float().mean() <= 0.02

    levels = want["u8"].float()
    got = crop_resize(*a, _dev(mean255), _dev(std255), torch.float32)
    assert got.dtype == torch.float32
    d = (got.cpu() * std255 + mean255 - levels).abs()
    print(f"{name} S={S} f32: worst {float(d.max()):.5f}")
    assert d.max() <= 1 + 1e-3 and (d > 1e-3).float().mean() <= 0.02

    got = crop_resize(*a, _dev(mean255), _dev(std255), torch.bfloat16)
    assert got.dtype == torch.bfloat16 and got.shape == (N, S, S, C)
    d = (got.cpu().float() * std255 + mean255 - levels).abs()
    print(f"{name} S={S} bf16: worst {float(d.max()):.5f}")
    assert d.max() <= 1.6


def test_two_launches_are_bit_identical():
    src, idx, params, flip, mean255, std255, _ = _inputs_and_oracle(
        "borders_37x23", 33)
    a = (_dev(src), _dev(idx), _dev(params), _dev(flip), 33, _dev(mean255),
         _dev(std255), torch.bfloat16)
    one, two = crop_resize(*a), crop_resize(*a)
    assert torch.equal(one.view(torch.int16), two.view(torch.int16))
    assert torch.equal(crop_resize(*a[:5]), crop_resize(*a[:5]))


def test_loader_crop_modes_match_cpu_through_crop_resize():
    """The loader's rrc / eval batches are crop_resize of the resident tensor
    with the loader's own parameter rows: replay those rows on CPU. (Device
    and CPU generators are different streams, so the rows sampled on the
    device are copied over, not re-sampled.)"""
    rng = np.random.default_rng(0)
    x = rng.integers(0, 256, (24, 20, 28, 3), dtype=np.uint8)
    ts = TaskSet(x, rng.integers(0, 5, 24).astype(np.int64),
                 np.zeros(24, dtype=np.int64))
    mean255, std255 = torch.tensor(MEAN) * 255, torch.tensor(STD) * 255
    for mode in ("rrc", "eval"):
        ld = GpuTaskLoader(ts, 8, "cuda", MEAN, STD, seed=5, shuffle=False,
                           augment=mode == "rrc", dtype=torch.bfloat16,
                           crop_mode=mode, out_size=16)
        g = torch.Generator(device="cuda")
        g.manual_seed(ld.seed * 1000003 + ld.epoch * 131 + ld.rank)
        batches = list(ld)
        assert len(batches) == 3
        for b, (imgs, labels, _) in enumerate(batches):
            assert imgs.shape == (8, 16, 16, 3)
            assert imgs.dtype == torch.bfloat16 and imgs.is_cuda
            if mode == "rrc":
                params, flip = rrc_params(8, 20, 28, 16, g, "cuda")
            else:
                params, flip = eval_params(8, 20, 28, 16, "cuda")
            idx = torch.arange(b * 8, b * 8 + 8)
            levels = crop_resize(torch.from_numpy(x), idx, params.cpu(),
                                 flip.cpu(), 16).float()
            d = (imgs.cpu().float() * std255 + mean255 - levels).abs()
            assert d.max() <= 1.6, (mode, b, float(d.max()))
            assert torch.equal(labels.cpu(),
                               torch.from_numpy(ts.y[idx.numpy()]))


@pytest.mark.timeout(300)
def test_engine_large_input_gpu_data_run(capsys):
    """--gpu_data --input_size 96 end to end on the HIP path (bf16): rrc
    train loader, eval val / feature loaders."""
    from cilfw.config import parse_args
    from cilfw.engine import run
    args = parse_args([
        "--data_set", "synthetic", "--backbone", "resnet18",
        "--synthetic_classes", "4", "--num_bases", "2", "--increment", "2",
        "--num_epochs", "1", "--batch_size", "16", "--workers", "0",
        "--synthetic_train_size", "64", "--memory_size", "8",
        "--eval_every_epoch", "0", "--input_size", "96", "--gpu_data",
        "--lr", "0.01", "--seed", "1", "--dtype", "bf16",
    ])
    accs = run(args)
    assert len(accs) == 2 and all(np.isfinite(a) for a in accs)
    log = capsys.readouterr().out
    assert "loss:" in log and "nan" not in log.lower(), log
