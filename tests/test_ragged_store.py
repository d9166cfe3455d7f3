"""RaggedImageStore on the CPU: what it holds is exactly what
``datasets.load_image`` decodes (lossless PNGs, so byte equality), and its
views / gathers / concats keep that property."""

import numpy as np
import pytest
import torch

import _ragged_tree as RT
from cilfw.data import ragged_store as RS
from cilfw.data.datasets import load_image
from cilfw.data.ragged_store import RaggedImageStore


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    paths = RT.write_files(str(tmp_path_factory.mktemp("png")))
    want = [load_image(p) for p in paths]
    store = RaggedImageStore.from_paths(paths, "cpu", workers=3)
    return paths, want, store


def _same(store, want):
    assert len(store) == len(want)
    assert store.nbytes == sum(w.size for w in want)
    assert store.offsets.dtype == torch.int64
    assert store.hw.dtype == torch.int32 and store.hw.shape == (len(want), 2)
    assert np.array_equal(store.offsets.numpy(), store.offsets_host)
    assert np.array_equal(store.hw.numpy(), store.hw_host)
    for m, w in enumerate(want):
        assert tuple(store.hw_host[m]) == w.shape[:2]
        assert np.array_equal(store.image(m).numpy(), w), m


def test_modes_l_and_rgba_are_present_and_converted(built):
    from PIL import Image
    paths, want, _ = built
    modes = [Image.open(p).mode for p in paths]
    assert "L" in modes and "RGBA" in modes
    assert all(w.shape[2] == 3 and w.dtype == np.uint8 for w in want)


def test_every_stored_image_is_load_image(built, capsys):
    paths, want, store = built
    _same(store, want)
    assert store.channels == 3 and store.pool.dtype == torch.uint8
    assert store.pool.numel() == store.nbytes  # packed, nothing between
    # offsets are the running sum of the sizes
    sizes = np.array([w.size for w in want])
    assert np.array_equal(store.offsets_host,
                          np.concatenate([[0], np.cumsum(sizes)[:-1]]))


def test_building_prints_the_store_line(tmp_path, capsys):
    paths = RT.write_files(str(tmp_path), sizes=RT.SIZES[:2])
    store = RaggedImageStore.from_paths(paths, "cpu")
    out = capsys.readouterr().out
    mb = store.nbytes / 1e6
    assert out.count("[gpu_data] ragged store:") == 1
    assert f"[gpu_data] ragged store: 2 images, {mb:.1f} MB resident (cpu)" \
        in out


def test_small_staging_chunks_upload_the_same_bytes(built, monkeypatch):
    paths, want, _ = built
    # smaller than most single images: every chunk path is taken
    monkeypatch.setattr(RS, "STAGING_BYTES", 10_000)
    _same(RaggedImageStore.from_paths(paths, "cpu", workers=2, log=False),
          want)


def test_prefix_view_shares_the_pool(built):
    _, want, store = built
    for n in (0, 1, 4, len(want)):
        v = store[:n]
        assert v.pool.data_ptr() == store.pool.data_ptr()
        _same(v, want[:n])
    with pytest.raises(TypeError):
        store[2]


def test_gather_builds_a_compact_copy(built):
    _, want, store = built
    idx = np.array([4, 0, 1, 2, 5, 5])  # out of order, an adjacent run, a repeat
    g = store.gather(idx)
    _same(g, [want[i] for i in idx])
    assert g.pool.data_ptr() != store.pool.data_ptr()
    assert g.pool.numel() == g.nbytes
    # gathering from a view indexes the view
    _same(store[:3].gather([2, 0]), [want[2], want[0]])
    _same(store.gather([]), [])


def test_concat_and_empty_sides(built):
    _, want, store = built
    a, b = store.gather([1, 3]), store.gather([0])
    _same(RaggedImageStore.concat(a, b), [want[1], want[3], want[0]])
    empty = RaggedImageStore.from_paths([], "cpu", log=False)
    assert len(empty) == 0 and empty.nbytes == 0
    assert empty.hw.shape == (0, 2) and empty.offsets.shape == (0,)
    _same(RaggedImageStore.concat(empty, a), [want[1], want[3]])
    _same(RaggedImageStore.concat(a, empty), [want[1], want[3]])
    _same(RaggedImageStore.concat(empty, empty), [])
    _same(RaggedImageStore.concat_all([b, empty, a, store[:2]]),
          [want[0], want[1], want[3], want[0], want[1]])


def test_append_lands_behind_the_decoded_images(built):
    paths, want, store = built
    tail = store.gather([5, 2])
    s = RaggedImageStore.from_paths(paths[:3], "cpu", append=tail, log=False)
    _same(s, want[:3] + [want[5], want[2]])
    _same(RaggedImageStore.from_paths([], "cpu", append=tail, log=False),
          [want[5], want[2]])


def test_from_arrays_matches_from_paths(built):
    _, want, store = built
    s = RaggedImageStore.from_arrays(want, "cpu", log=False)
    _same(s, want)
    assert torch.equal(s.pool, store.pool)


def test_construction_rejects_an_oversize_image(built, monkeypatch):
    paths, want, _ = built
    biggest = max(w.size for w in want)
    monkeypatch.setattr(RS, "MAX_IMAGE_BYTES", biggest)  # limit is exclusive
    with pytest.raises(ValueError, match="bytes"):
        RaggedImageStore.from_paths(paths, "cpu", log=False)
    monkeypatch.setattr(RS, "MAX_IMAGE_BYTES", biggest + 1)
    _same(RaggedImageStore.from_paths(paths, "cpu", log=False), want)


def test_construction_rejects_offsets_outside_the_pool():
    pool = torch.zeros(100, dtype=torch.uint8)
    RaggedImageStore(pool, [0, 52], [[4, 4], [4, 4]], 3)
    with pytest.raises(ValueError, match="outside"):
        RaggedImageStore(pool, [0, 53], [[4, 4], [4, 4]], 3)
    with pytest.raises(ValueError, match="outside"):
        RaggedImageStore(pool, [-1], [[4, 4]], 3)


def test_decode_thread_pool_is_bounded(built, monkeypatch):
    """workers=64 still decodes with at most 16 threads."""
    paths, want, _ = built
    seen = []
    real = RS.ThreadPoolExecutor

    def spy(max_workers=None, **k):
        seen.append(max_workers)
        return real(max_workers=max_workers, **k)

    monkeypatch.setattr(RS, "ThreadPoolExecutor", spy)
    _same(RaggedImageStore.from_paths(paths, "cpu", workers=64, log=False),
          want)
    RaggedImageStore.from_paths(paths[:1], "cpu", workers=0, log=False)
    assert seen == [16, 1]
