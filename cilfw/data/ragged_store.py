"""Packed, ragged, device-resident image store - the ``--gpu_data`` source for
path-backed datasets (ImageFolder trees: ImageNet-100/1000, CUB-200).

An image tree has a different (H, W) per file, so it cannot be one dense
[M,Hs,Ws,C] tensor. The store decodes every file ONCE, at its full stored
resolution, into one flat uint8 byte pool on the device plus two tables:

    offsets int64 [M]    byte offset of image m in the pool
    hw      int32 [M,2]  its (H, W)

image m is H*W*C contiguous HWC bytes at ``pool[offsets[m]:]`` (C uniform).
``ops.crop_resize_ragged`` (csrc/data.hip) samples batches straight from it.
A host numpy mirror of both tables makes slicing / gathering sync-free.

The kernel trusts the tables, so the bounds it relies on are checked here,
once, when a store is built: every image has H*W*C < 2**31 bytes and lies
inside the pool.
"""

from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

MAX_IMAGE_BYTES = 2 ** 31      # the kernel indexes inside an image with int32
STAGING_BYTES = 256 << 20      # host staging per upload chunk
MAX_DECODE_THREADS = 16


def _announce(store):
    print(f"[gpu_data] ragged store: {len(store)} images, "
          f"{store.nbytes / 1e6:.1f} MB resident ({store.device})", flush=True)


def _check_sizes(hw, channels):
    """Per-image byte sizes (int64) of an (M,2) (H, W) table, validated."""
    hw = np.asarray(hw, dtype=np.int64).reshape(-1, 2)
    if hw.size and hw.min() < 1:
        raise ValueError("ragged store: image with an empty side")
    sizes = hw[:, 0] * hw[:, 1] * int(channels)
    if sizes.size and sizes.max() >= MAX_IMAGE_BYTES:
        m = int(sizes.argmax())
        raise ValueError(
            f"ragged store: image {m} is {hw[m, 0]}x{hw[m, 1]}x{channels} = "
            f"{int(sizes[m])} bytes; the limit is {MAX_IMAGE_BYTES} - 1")
    return sizes


class RaggedImageStore:
    def __init__(self, pool, offsets, hw, channels=3, _trusted=False):
        """pool: flat uint8 tensor (on the store's device); offsets / hw:
        HOST arrays (M,), (M,2). Offsets are honoured as given (they need not
        be cumulative, and several stores may share one pool)."""
        assert pool.dtype == torch.uint8 and pool.dim() == 1 \
            and pool.is_contiguous()
        assert 1 <= int(channels) <= 4
        self.pool = pool
        self.channels = int(channels)
        self.offsets_host = np.ascontiguousarray(offsets,
                                                 dtype=np.int64).reshape(-1)
        self.hw_host = np.ascontiguousarray(hw, dtype=np.int32).reshape(-1, 2)
        assert self.offsets_host.shape[0] == self.hw_host.shape[0]
        if not _trusted:
            sizes = _check_sizes(self.hw_host, self.channels)
            if sizes.size and (self.offsets_host.min() < 0 or
                               (self.offsets_host + sizes).max()
                               > pool.numel()):
                raise ValueError("ragged store: image outside the pool")
        self.offsets = torch.from_numpy(self.offsets_host).to(pool.device)
        self.hw = torch.from_numpy(self.hw_host).to(pool.device)

    # ------------------------------------------------------------- building

    @classmethod
    def empty(cls, device, channels=3):
        return cls(torch.empty(0, dtype=torch.uint8, device=device),
                   np.zeros(0, np.int64), np.zeros((0, 2), np.int32),
                   channels)

    @classmethod
    def from_paths(cls, paths, device, workers=0, append=None, log=True):
        """Decode image files into a new store. Pass one reads the sizes from
        the file headers only and allocates the pool once; pass two decodes
        (datasets.load_image: RGB) in a small thread pool and uploads in
        bounded chunks, so the host never holds the whole decoded set.
        ``append``: an existing store whose images are copied (device to
        device) behind the decoded ones, into the same allocation."""
        from .datasets import Image, load_image
        paths = [str(p) for p in paths]
        C = 3
        if append is not None:
            assert append.channels == C
        if paths and Image is None:
            raise RuntimeError("ragged store: decoding image files needs PIL")
        threads = max(1, min(int(workers or 1), MAX_DECODE_THREADS))

        def header(p):
            with Image.open(p) as im:
                w, h = im.size
            return h, w

        with ThreadPoolExecutor(max_workers=threads) as ex:
            hw = np.asarray(list(ex.map(header, paths)),
                            dtype=np.int64).reshape(-1, 2)
            sizes = _check_sizes(hw, C)
            offsets = np.zeros(len(paths), dtype=np.int64)
            if len(paths) > 1:
                np.cumsum(sizes[:-1], out=offsets[1:])
            task_bytes = int(sizes.sum())
            tail = append.nbytes if append is not None else 0
            pool = torch.empty(task_bytes + tail, dtype=torch.uint8,
                               device=device)

            # pass two: chunks of at most STAGING_BYTES (one image if larger)
            staging = np.empty(min(max(task_bytes, 1), STAGING_BYTES),
                               dtype=np.uint8)
            lo = 0
            while lo < len(paths):
                hi, nb = lo, 0
                while hi < len(paths) and (hi == lo or nb + int(sizes[hi])
                                           <= STAGING_BYTES):
                    nb += int(sizes[hi])
                    hi += 1
                if nb > staging.size:
                    staging = np.empty(nb, dtype=np.uint8)
                base = int(offsets[lo])

                def decode(m, base=base, staging=staging):
                    img = load_image(paths[m])
                    if img.shape != (hw[m, 0], hw[m, 1], C):
                        raise ValueError(
                            f"{paths[m]}: decoded shape {img.shape} differs "
                            f"from its header {tuple(hw[m])}")
                    o = int(offsets[m]) - base
                    staging[o:o + int(sizes[m])] = img.reshape(-1)

                list(ex.map(decode, range(lo, hi)))
                pool[base:base + nb].copy_(torch.from_numpy(staging[:nb]))
                lo = hi
        if append is not None and len(append):
            dst = cls(pool, np.zeros(0, np.int64), np.zeros((0, 2), np.int32),
                      C)
            app_off = dst._copy_in(task_bytes, [append])
            offsets = np.concatenate([offsets, app_off])
            hw = np.concatenate([hw, append.hw_host.astype(np.int64)])
        store = cls(pool, offsets, hw, C)
        if log:
            _announce(store)
        return store

    @classmethod
    def from_arrays(cls, images, device, log=True):
        """Store of in-memory uint8 HWC arrays (all with the same C)."""
        images = [np.ascontiguousarray(a, dtype=np.uint8) for a in images]
        C = images[0].shape[2] if images else 3
        assert all(a.ndim == 3 and a.shape[2] == C for a in images)
        hw = np.asarray([a.shape[:2] for a in images],
                        dtype=np.int64).reshape(-1, 2)
        sizes = _check_sizes(hw, C)
        offsets = np.zeros(len(images), dtype=np.int64)
        if len(images) > 1:
            np.cumsum(sizes[:-1], out=offsets[1:])
        pool = torch.empty(int(sizes.sum()), dtype=torch.uint8, device=device)
        lo = 0
        while lo < len(images):  # bounded staging, as in from_paths
            hi, nb = lo, 0
            while hi < len(images) and (hi == lo or nb + int(sizes[hi])
                                        <= STAGING_BYTES):
                nb += int(sizes[hi])
                hi += 1
            flat = np.concatenate([a.reshape(-1) for a in images[lo:hi]])
            base = int(offsets[lo])
            pool[base:base + nb].copy_(torch.from_numpy(flat))
            lo = hi
        store = cls(pool, offsets, hw, C)
        if log:
            _announce(store)
        return store

    # ------------------------------------------------------------ accessors

    def __len__(self):
        return self.offsets_host.shape[0]

    @property
    def device(self):
        return self.pool.device

    @property
    def sizes_host(self):
        return (self.hw_host[:, 0].astype(np.int64) * self.hw_host[:, 1]
                * self.channels)

    @property
    def nbytes(self):
        """Bytes of this store's images (a view counts only its own)."""
        return int(self.sizes_host.sum())

    def __getitem__(self, key):
        """store[:n] (any unit-step slice): a view sharing the pool."""
        if not isinstance(key, slice) or key.step not in (None, 1):
            raise TypeError("RaggedImageStore supports store[a:b] views; "
                            "use gather(idx) for an index selection")
        return RaggedImageStore(self.pool, self.offsets_host[key],
                                self.hw_host[key], self.channels,
                                _trusted=True)

    def image(self, m):
        """Image m as an (H, W, C) uint8 view of the pool."""
        h, w = (int(v) for v in self.hw_host[m])
        o = int(self.offsets_host[m])
        return self.pool[o:o + h * w * self.channels].view(h, w,
                                                           self.channels)

    # ---------------------------------------------------- gather and concat

    def _copy_in(self, at, segments):
        """Copy the images of ``segments`` (stores, in order) into self.pool
        from byte ``at`` on, device to device, merging runs that are already
        adjacent in their source pool. Returns the new byte offsets."""
        new_off = []
        for s in segments:
            off, sizes = s.offsets_host, s.sizes_host
            k, n = 0, len(s)
            while k < n:
                start = int(off[k])
                end = start + int(sizes[k])
                new_off.append(at)
                run = k + 1
                while run < n and int(off[run]) == end:
                    new_off.append(at + end - start)
                    end += int(sizes[run])
                    run += 1
                self.pool[at:at + end - start].copy_(s.pool[start:end])
                at += end - start
                k = run
        return np.asarray(new_off, dtype=np.int64)

    @classmethod
    def concat_all(cls, stores, device=None):
        """A new compact store of all images of ``stores``, in order."""
        stores = list(stores)
        assert stores, "concat_all needs at least one store"
        C = stores[0].channels
        assert all(s.channels == C for s in stores)
        device = device if device is not None else stores[0].device
        total = sum(s.nbytes for s in stores)
        out = cls(torch.empty(total, dtype=torch.uint8, device=device),
                  np.zeros(0, np.int64), np.zeros((0, 2), np.int32), C)
        offsets = out._copy_in(0, stores)
        hw = np.concatenate([s.hw_host for s in stores])
        return cls(out.pool, offsets, hw, C)

    @classmethod
    def concat(cls, a, b):
        return cls.concat_all([a, b])

    def gather(self, idx):
        """A new compact store of images ``idx`` (a HOST index array), built
        by device-to-device slice copies; it does not share this pool."""
        idx = np.asarray(idx, dtype=np.int64).reshape(-1)
        sel = RaggedImageStore(self.pool, self.offsets_host[idx],
                               self.hw_host[idx], self.channels,
                               _trusted=True)
        return RaggedImageStore.concat_all([sel])
