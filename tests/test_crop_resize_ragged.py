"""ops.crop_resize_ragged on the CPU (its pure-torch oracle), the per-image
parameter samplers, and the GpuTaskLoader / engine wiring for path-backed
datasets (CILFW_GPU_DATA_ON_CPU=1).

The ragged oracle is, by construction, the dense oracle applied per image, so
these comparisons are exact (torch.equal); only the comparison against the
HOST EvalTransform carries the floor-tie allowance documented in
tests/test_crop_resize.py (double vs fp32 interpolation: at most one level on
at most 2% of pixels).
"""

import numpy as np
import pytest
import torch

import _ragged_tree as RT
from cilfw.data import transforms as T
from cilfw.data.datasets import load_image
from cilfw.data.device_augment import (eval_params, eval_params_ragged,
                                       resize_params, resize_params_ragged,
                                       rrc_params, rrc_params_ragged)
from cilfw.data.gpu_pipeline import GpuTaskLoader
from cilfw.data.ragged_store import RaggedImageStore
from cilfw.data.scenario import TaskSet
from cilfw.ops import (crop_resize, crop_resize_ragged,
                       crop_resize_ragged_reference)
from cilfw.ops.functional import crop_resize_reference

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
# the sizes the issue pins at S=96 (R = int(256/224*96) = 109), plus two with
# short == R so the no-resize branch of the eval rule is really taken
SIZES_96 = RT.SIZES + [(109, 109), (109, 130), (150, 109)]


def _pack(images, guard=0):
    """Flat pool + tables of uint8 HWC arrays, ``guard`` bytes of 255 before
    the first and after the last image."""
    C = images[0].shape[2]
    parts, offs, at = [np.full(guard, 255, np.uint8)], [], guard
    for a in images:
        offs.append(at)
        parts.append(a.reshape(-1))
        at += a.size
    parts.append(np.full(guard, 255, np.uint8))
    return (torch.from_numpy(np.concatenate(parts)),
            torch.tensor(offs, dtype=torch.int64),
            torch.tensor([a.shape[:2] for a in images], dtype=torch.int32), C)


def _rand_images(sizes, C=3, seed=0):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, C), dtype=np.uint8) for h, w in sizes]


# ------------------------------------------------------------------ oracle

def test_uniform_sizes_equal_the_dense_oracle_exactly():
    imgs = _rand_images([(20, 28)] * 5)
    pool, offs, hw, C = _pack(imgs, guard=7)
    g = torch.Generator().manual_seed(3)
    idx = torch.tensor([4, 0, 4, 2, 1, 3, 3])
    params, flip = rrc_params(7, 20, 28, 16, g, "cpu")
    src = torch.from_numpy(np.stack(imgs))
    mean255, std255 = torch.tensor(MEAN) * 255, torch.tensor(STD) * 255
    for norm in ((), (mean255, std255, torch.float32),
                 (mean255, std255, torch.bfloat16)):
        got = crop_resize_ragged(pool, offs, hw, C, idx, params, flip, 16,
                                 *norm)
        want = crop_resize_reference(src, idx, params, flip, 16, *norm)
        assert got.dtype == want.dtype and torch.equal(got, want)
    assert torch.equal(
        crop_resize_ragged(pool, offs, hw, C, idx, params, flip, 16),
        crop_resize_ragged_reference(pool, offs, hw, C, idx, params, flip,
                                     16))


def test_mixed_sizes_equal_the_per_image_dense_oracle():
    sizes = [(9, 13), (37, 23), (1, 7), (5, 1), (21, 18), (2, 2)]
    for C in (1, 3, 4):
        imgs = _rand_images(sizes, C=C, seed=C)
        pool, offs, hw, _ = _pack(imgs, guard=64)
        g = torch.Generator().manual_seed(C)
        idx = torch.tensor([3, 0, 5, 4, 1, 1, 2, 9, -4])  # last two clamp
        params, flip = rrc_params_ragged(hw[idx.clamp(0, 5)], 11, g)
        got = crop_resize_ragged(pool, offs, hw, C, idx, params, flip, 11)
        assert got.shape == (9, 11, 11, C) and got.dtype == torch.uint8
        for n, m in enumerate(idx.clamp(0, 5).tolist()):
            want = crop_resize(torch.from_numpy(imgs[m])[None], None,
                               params[n:n + 1], flip[n:n + 1], 11)[0]
            assert torch.equal(got[n], want), (C, n, m)


def test_offsets_are_honoured_not_assumed_cumulative():
    imgs = _rand_images([(6, 9), (11, 4), (3, 3)])
    pool, offs, hw, C = _pack(imgs)
    # same bytes, stored back to front with gaps
    rev = torch.full((pool.numel() + 30,), 255, dtype=torch.uint8)
    at, new = 5, []
    for m in (2, 1, 0):
        n = imgs[m].size
        rev[at:at + n] = pool[offs[m]:offs[m] + n]
        new.append(at)
        at += n + 10
    offs2 = torch.tensor(new[::-1], dtype=torch.int64)
    idx = torch.tensor([0, 1, 2, 1])
    params, flip = resize_params_ragged(hw[idx], 8)
    assert torch.equal(
        crop_resize_ragged(pool, offs, hw, C, idx, params, flip, 8),
        crop_resize_ragged(rev, offs2, hw, C, idx, params, flip, 8))


# -------------------------------------------------------------- parameters

def test_eval_and_resize_rows_are_bitwise_the_scalar_rules():
    S = 96
    hw = torch.tensor(SIZES_96, dtype=torch.int32)
    ep, ef = eval_params_ragged(hw, S)
    rp, rf = resize_params_ragged(hw, S)
    assert ep.dtype == rp.dtype == torch.float32 and ep.shape == (len(hw), 4)
    assert ef.dtype == torch.uint8 and not ef.any() and not rf.any()
    for n, (H, W) in enumerate(SIZES_96):
        want = eval_params(1, H, W, S, "cpu")[0][0]
        assert torch.equal(ep[n].view(torch.int32),
                           want.view(torch.int32)), (H, W)
        want = resize_params(1, H, W, S, "cpu")[0][0]
        assert torch.equal(rp[n].view(torch.int32),
                           want.view(torch.int32)), (H, W)
    # the short == R rows took the no-resize branch: scale exactly 1
    assert torch.equal(ep[len(RT.SIZES):, 2:], torch.ones(3, 2))
    # other output sizes, including one where (110,110) is short == R
    for S2 in (28, 72, 97, 224):
        ep, _ = eval_params_ragged(hw, S2)
        for n, (H, W) in enumerate(SIZES_96):
            assert torch.equal(ep[n], eval_params(1, H, W, S2, "cpu")[0][0])


def test_rrc_ragged_equals_rrc_on_uniform_sizes():
    for Hs, Ws, S in ((20, 28, 16), (37, 23, 16), (375, 500, 224)):
        g1 = torch.Generator().manual_seed(9)
        g2 = torch.Generator().manual_seed(9)
        hw = torch.tensor([[Hs, Ws]] * 512, dtype=torch.int32)
        p1, f1 = rrc_params(512, Hs, Ws, S, g1, "cpu")
        p2, f2 = rrc_params_ragged(hw, S, g2)
        assert torch.equal(p1, p2) and torch.equal(f1, f2)
        # the generators are left in the same state: same number of draws
        assert torch.equal(torch.rand(4, generator=g1),
                           torch.rand(4, generator=g2))
    # never fitting -> the centred square of side min(H, W)
    g1, g2 = torch.Generator().manual_seed(1), torch.Generator().manual_seed(1)
    p1, _ = rrc_params(8, 37, 23, 16, g1, "cpu", scale=(4.0, 4.0))
    p2, _ = rrc_params_ragged(torch.tensor([[37, 23]] * 8), 16, g2,
                              scale=(4.0, 4.0))
    assert torch.equal(p1, p2)


def test_rrc_ragged_boxes_lie_inside_their_own_image():
    S = 16
    g = torch.Generator().manual_seed(0)
    sizes = torch.tensor(SIZES_96 + [(9, 13), (1, 7), (5, 1), (2, 2)],
                         dtype=torch.int32)
    hw = sizes[torch.randint(0, len(sizes), (4096,), generator=g)]
    params, flip = rrc_params_ragged(hw, S, g)
    assert params.shape == (4096, 4) and flip.dtype == torch.uint8
    y, x = params[:, 0], params[:, 1]
    h = params[:, 2] * (S - 1) + 1
    w = params[:, 3] * (S - 1) + 1
    assert torch.equal(y, y.floor()) and torch.equal(x, x.floor())
    assert (y >= 0).all() and (x >= 0).all()
    assert (h >= 1 - 1e-4).all() and (w >= 1 - 1e-4).all()
    assert (y + h <= hw[:, 0] + 1e-3).all()
    assert (x + w <= hw[:, 1] + 1e-3).all()
    assert abs(flip.float().mean().item() - 0.5) <= 0.05


# ------------------------------------------------------------------ loader

def _path_taskset(root, sizes=RT.SIZES + [(82, 100), (130, 82)]):
    paths = RT.write_files(str(root), sizes=sizes, odd_modes=False)
    n = len(paths)
    return TaskSet(np.asarray(paths, dtype=object),
                   np.arange(n, dtype=np.int64) % 3,
                   np.zeros(n, dtype=np.int64)), paths


def test_ragged_loader_eval_matches_host_eval_transform(tmp_path):
    """The mixed sizes at S=72, the input size of the engine run below
    (R = int(256/224*72) = 82; the last two files have short == R). Bound: the
    one of test_crop_resize.py::test_eval_params_match_eval_transform.

    S is not that test's 28 on purpose: 64x48 at S=28 resizes by exactly
    sy = 63/42 = 3/2, so every other output row is an exact half-sum and the
    true value is an integer on a large share of pixels - a tie-dense map on
    which the DENSE oracle itself differs from the host (double vs fp32) on
    2.4% of pixels, by one level. That is the oracle pair's own error at that
    geometry, not something this loader adds; S=72 has no such step."""
    S = 72
    ts, paths = _path_taskset(tmp_path)
    ld = GpuTaskLoader(ts, 3, "cpu", MEAN, STD, shuffle=False, augment=False,
                       drop_last=False, dtype=torch.float32,
                       crop_mode="eval", out_size=S)
    assert isinstance(ld.images, RaggedImageStore) and ld.n_task == len(paths)
    batches = list(ld)
    got = torch.cat([i for i, _, _ in batches])
    assert got.shape == (len(paths), S, S, 3) and got.dtype == torch.float32
    assert torch.equal(torch.cat([l for _, l, _ in batches]),
                       torch.from_numpy(ts.y))

    class A:
        input_size = S
    host = T.EvalTransform(A(), "imagenet")
    host.small = False
    mean255, std255 = torch.tensor(MEAN) * 255, torch.tensor(STD) * 255
    for m, p in enumerate(paths):
        want = torch.round(host(load_image(p)) * host.std * 255
                           + host.mean * 255)
        lev = torch.round(got[m] * std255 + mean255)
        d = (lev - want).abs()
        print(f"{p[-10:]}: worst {int(d.max())}, "
              f"{100 * float((d != 0).float().mean()):.3f}% differ")
        assert d.max() <= 1 and (d != 0).float().mean() <= 0.02, p


def test_ragged_loader_rrc_replays_through_the_oracle(tmp_path):
    ts, paths = _path_taskset(tmp_path)
    ld = GpuTaskLoader(ts, 4, "cpu", MEAN, STD, seed=5, shuffle=False,
                       dtype=torch.float32, crop_mode="rrc", out_size=16)
    a = [i.clone() for i, _, _ in ld]
    b = [i.clone() for i, _, _ in ld]
    assert len(a) == 2 and all(torch.equal(x, y) for x, y in zip(a, b))
    g = torch.Generator().manual_seed(ld.seed * 1000003)
    st = ld.images
    mean255, std255 = torch.tensor(MEAN) * 255, torch.tensor(STD) * 255
    for bi, imgs in enumerate(a):
        idx = torch.arange(bi * 4, bi * 4 + 4)
        params, flip = rrc_params_ragged(st.hw[idx], 16, g)
        for n, m in enumerate(idx.tolist()):
            want = crop_resize(torch.tensor(load_image(paths[m]))[None],
                               None, params[n:n + 1], flip[n:n + 1], 16,
                               mean255, std255, torch.float32)[0]
            assert torch.equal(imgs[n], want)


def test_ragged_loader_rejects_pad_and_takes_a_store_as_extra(tmp_path):
    ts, paths = _path_taskset(tmp_path)
    with pytest.raises(ValueError, match="crop_mode"):
        GpuTaskLoader(ts, 4, "cpu", MEAN, STD)
    with pytest.raises(ValueError, match="crop_mode"):
        GpuTaskLoader(ts, 4, "cpu", MEAN, STD, crop_mode="pad", out_size=16)
    extra = RaggedImageStore.from_paths(paths[:2], "cpu", log=False)
    ld = GpuTaskLoader(ts, 5, "cpu", MEAN, STD, shuffle=False, augment=False,
                       drop_last=False, dtype=torch.float32,
                       crop_mode="resize", out_size=12,
                       extra=(extra, torch.tensor([7, 8]),
                              torch.tensor([0, 0])))
    assert len(ld.images) == len(paths) + 2 and ld.n_task == len(paths)
    imgs = torch.cat([i for i, _, _ in ld])
    labels = torch.cat([l for _, l, _ in ld])
    assert imgs.shape[0] == len(paths) + 2
    assert labels[-2:].tolist() == [7, 8]
    assert torch.equal(imgs[-2:], imgs[:2])  # the exemplars ARE files 0, 1
    # the task prefix the replay mirror gathers from
    pre = ld.images[:ld.n_task]
    assert len(pre) == len(paths)
    assert np.array_equal(pre.image(3).numpy(), load_image(paths[3]))


def test_ragged_loader_with_augment_pipeline_crops_first(tmp_path):
    from cilfw.data.device_augment import DeviceAugment
    ts, _ = _path_taskset(tmp_path)
    seen = []

    class Spy(DeviceAugment):
        def __call__(self, imgs, g):
            seen.append((tuple(imgs.shape), imgs.dtype))
            return super().__call__(imgs, g)

    ld = GpuTaskLoader(ts, 4, "cpu", MEAN, STD, seed=2, dtype=torch.float32,
                       crop_mode="rrc", out_size=16,
                       aug_pipeline=Spy(color_jitter=0.4, aa_policy=""))
    batches = [i for i, _, _ in ld]
    assert seen == [((8, 16, 16, 3), torch.uint8)]
    assert len(batches) == 2 and all(torch.isfinite(b).all() for b in batches)


# ------------------------------------------------------------------ mirror

def test_replay_mirror_tracks_a_path_backed_memory(tmp_path):
    from cilfw.cil import RehearsalMemory
    from cilfw.cil.replay_gpu import DeviceReplayMirror
    paths = RT.write_files(str(tmp_path), sizes=RT.SIZES * 2,
                           odd_modes=False)
    x = np.asarray(paths, dtype=object)
    store = RaggedImageStore.from_paths(paths, "cpu", log=False)
    memory = RehearsalMemory(8, "barycenter")
    mirror = DeviceReplayMirror("cpu")
    feats = torch.randn(12, 5, generator=torch.Generator().manual_seed(0))

    def check(m):
        mx, my, mt = memory.get()
        st, labels, tasks = m.get()
        assert len(m) == len(memory) == len(st)
        assert labels.tolist() == my.tolist() and tasks.tolist() == mt.tolist()
        for k, p in enumerate(mx):
            assert np.array_equal(st.image(k).numpy(), load_image(p))
        assert st.pool.numel() == st.nbytes  # compact: nothing kept alive
        return st

    y0 = np.array([0, 1] * 3)
    memory.add(x[:6], y0, np.zeros(6, np.int64), feats[:6])
    mirror.update(memory, task_images=store[:6])
    check(mirror)
    y1 = np.array([2, 3] * 3)
    memory.add(x[6:], y1, np.ones(6, np.int64), feats[6:])
    mirror.update(memory, task_images=store[6:])
    check(mirror)  # quota shrank 4 -> 2: old classes trimmed AND compacted
    for c, s in mirror._imgs.items():
        assert len(s) == 2 and s.pool.numel() == s.nbytes
        assert s.pool.data_ptr() != store.pool.data_ptr()
    # resume: rebuilt from the memory's paths
    check(DeviceReplayMirror.from_memory(memory, "cpu"))
    # no resident task store at hand: decode the selected paths
    m2 = DeviceReplayMirror("cpu")
    mem2 = RehearsalMemory(8, "barycenter")
    mem2.add(x[:6], y0, np.zeros(6, np.int64), feats[:6])
    m2.update(mem2)
    st, _, _ = m2.get()
    assert np.array_equal(st.image(0).numpy(), load_image(mem2.get()[0][0]))


# ------------------------------------------------------------------ engine

def _engine_args(root, extra=()):
    from cilfw.config import parse_args
    return parse_args([
        "--data_set", "imagenet100", "--data_path", str(root),
        "--backbone", "resnet18", "--num_bases", "2", "--increment", "2",
        "--num_epochs", "1", "--batch_size", "8", "--workers", "2",
        "--memory_size", "8", "--eval_every_epoch", "0",
        "--input_size", "72", "--gpu_data", "--lr", "0.01", "--seed", "1",
        *extra])


@pytest.mark.timeout(300)
def test_engine_path_backed_gpu_data_on_cpu(tmp_path, monkeypatch, capsys):
    """--gpu_data on an ImageFolder tree of mixed-size PNGs: every loader is
    built on a RaggedImageStore (the store line), batches come from
    crop_resize_ragged, and task 1 replays from the device mirror."""
    import cilfw.data.gpu_pipeline as gp
    from cilfw import ops
    from cilfw.engine import run
    RT.write_tree(str(tmp_path))
    monkeypatch.setenv("CILFW_GPU_DATA_ON_CPU", "1")
    calls = []
    real = ops.crop_resize_ragged

    def spy(pool, offsets, hw, channels, idx, params, flip, out_size, *a,
            **k):
        calls.append(out_size)
        return real(pool, offsets, hw, channels, idx, params, flip, out_size,
                    *a, **k)

    monkeypatch.setattr(ops, "crop_resize_ragged", spy)
    made = []
    real_init = gp.GpuTaskLoader.__init__

    def init_spy(self, taskset, *a, **k):
        real_init(self, taskset, *a, **k)
        made.append((k.get("crop_mode"), self.ragged, len(self.images),
                     self.n_task, k.get("extra") is not None))

    monkeypatch.setattr(gp.GpuTaskLoader, "__init__", init_spy)
    accs = run(_engine_args(tmp_path))
    assert len(accs) == 2 and all(np.isfinite(a) for a in accs)
    log = capsys.readouterr().out
    # task 0: train (16 files) + val (6); task 1: train (16 + 8 exemplars)
    # + cumulative val (12). Feature passes reuse the train loader's store.
    lines = [ln for ln in log.splitlines()
             if ln.startswith("[gpu_data] ragged store:")]
    assert [ln.split()[3] for ln in lines] == ["16", "6", "24", "12"], lines
    assert all(m[1] for m in made) and all(c == 72 for c in calls) and calls
    train = [m for m in made if m[0] == "rrc"]
    assert train == [("rrc", True, 16, 16, False), ("rrc", True, 24, 16, True)]
    assert "nan" not in log.lower()


def test_engine_path_backed_opt_out_keeps_the_host_loader(tmp_path,
                                                          monkeypatch):
    """CILFW_GPU_DATA_PATHS=0 and small inputs: the host DataLoader."""
    from cilfw.engine import _gpu_data_active
    monkeypatch.setenv("CILFW_GPU_DATA_ON_CPU", "1")
    args = _engine_args(tmp_path)
    ds = TaskSet(np.asarray(["a.png"], dtype=object), [0], [0])
    assert _gpu_data_active(args, "cpu", ds)
    args.input_size = 64
    assert not _gpu_data_active(args, "cpu", ds)
    args.input_size = 72
    monkeypatch.setenv("CILFW_GPU_DATA_PATHS", "0")
    assert not _gpu_data_active(args, "cpu", ds)
    args.gpu_data = False
    monkeypatch.delenv("CILFW_GPU_DATA_PATHS")
    assert not _gpu_data_active(args, "cpu", ds)
