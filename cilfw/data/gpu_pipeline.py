"""Device-resident data pipeline — feeds the HIP training step at full rate.

A Python-side DataLoader tops out far below the ~20k imgs/s the MI355X step
consumes at CIFAR scale. When the task's images are array-backed (CIFAR /
synthetic; not lazy ImageFolder paths), cilfw uploads the task set ONCE as
uint8 (CIFAR-100 full train split = 150 MB — nothing against 288 GB HBM) and
assembles every batch on-device: gather -> random crop(+pad) -> horizontal
flip -> [RandAugment / color-jitter / random-erasing, see device_augment.py]
-> normalize -> bf16, all torch index ops on the GPU.

Large inputs (``--input_size > 64``) use the resampling crop modes instead
(``crop_mode`` "rrc" / "eval" / "resize"): RandomResizedCrop + flip for
training, resize + center-crop for evaluation, exactly the host transform
contract, from sources of any stored size. Those are ONE fused HIP launch per
batch (``ops.crop_resize``, csrc/data.hip): gather -> bilinear resample ->
flip -> quantize -> normalize straight from the resident uint8 tensor.

Path-backed tasksets (ImageFolder trees; ``x`` is an object array of file
paths) take the resampling modes too: the files are decoded once into a
``RaggedImageStore`` (ragged_store.py: flat uint8 pool + per-image offset /
size tables, full stored resolution) and every batch is one
``ops.crop_resize_ragged`` launch with per-image geometry. ``crop_mode="pad"``
needs a common stored size and is refused for them.

Sharding is the torch-DistributedSampler contract via the single shared
implementation ``cilfw.data.sampler.compute_shard`` (same seed+epoch
permutation on every rank, pad-by-repetition, rank-strided slice).

``extra`` accepts already-device-resident (images_u8, labels, task_ids)
tensors — the DeviceReplayMirror replay path (cilfw/cil/replay_gpu.py):
exemplars are concatenated after the task tensor exactly like the
reference's TaskSet.add_samples appends them (template.py:230-231), so the
epoch shuffle sees an identically-ordered index space.
"""

import numpy as np
import torch

from .sampler import compute_shard


class GpuTaskLoader:
    def __init__(self, taskset, batch_size, device, mean, std, world=1, rank=0,
                 shuffle=True, seed=0, augment=True, drop_last=True,
                 dtype=torch.bfloat16, pad=4, extra=None, aug_pipeline=None,
                 crop_mode="pad", out_size=None, workers=0, store=None):
        # path-backed taskset (ImageFolder trees): the images are decoded
        # once into a RaggedImageStore (ragged_store.py) and every batch is
        # ops.crop_resize_ragged of it. ``store`` hands in an already built
        # store of exactly taskset's images instead of decoding them again.
        self.ragged = taskset.x.dtype == object
        assert self.ragged or taskset.x.dtype == np.uint8, \
            "GpuTaskLoader needs uint8 array-backed images or image paths"
        labels = torch.from_numpy(
            np.ascontiguousarray(taskset.y).astype(np.int64)).to(device)
        if self.ragged:
            from .ragged_store import RaggedImageStore
            if crop_mode not in ("rrc", "eval", "resize"):
                raise ValueError(
                    f"GpuTaskLoader: path-backed images have no common "
                    f"stored size, so crop_mode must be 'rrc', 'eval' or "
                    f"'resize' (got {crop_mode!r}); 'pad' needs an "
                    f"array-backed dataset")
            assert out_size is not None, "path-backed images need out_size"
            ex_store = None
            if extra is not None:
                ex_store = extra[0]
                assert isinstance(ex_store, RaggedImageStore), \
                    "replay for a path-backed taskset is a RaggedImageStore"
            if store is not None:
                assert len(store) == len(taskset.x)
                images = store if ex_store is None else \
                    RaggedImageStore.concat(store, ex_store)
            else:
                images = RaggedImageStore.from_paths(
                    taskset.x, device, workers, append=ex_store)
            self.n_task = len(taskset.x)
            if extra is not None:
                labels = torch.cat([labels, extra[1].to(device, torch.int64)])
        else:
            images = torch.from_numpy(
                np.ascontiguousarray(taskset.x)).to(device)
            self.n_task = images.shape[0]
            if extra is not None:
                ex_imgs, ex_labels = extra[0], extra[1]
                assert ex_imgs.dtype == torch.uint8
                images = torch.cat([images, ex_imgs.to(device)])
                labels = torch.cat([labels, ex_labels.to(device,
                                                         torch.int64)])
        self.images = images
        self.labels = labels
        self.batch_size = batch_size
        self.device = device
        self.world, self.rank = world, rank
        self.shuffle, self.seed = shuffle, seed
        self.augment = augment
        self.aug_pipeline = aug_pipeline  # optional DeviceAugment (RandAugment etc.)
        self.drop_last = drop_last
        self.dtype = dtype
        self.pad = pad
        # crop_mode: "pad" = zero-pad + random crop at the stored size (small
        # inputs, the default); "rrc" = RandomResizedCrop + flip; "eval" =
        # resize + center-crop; "resize" = plain resize. The last three go
        # through ops.crop_resize and produce out_size x out_size batches
        # from sources of any stored size.
        assert crop_mode in ("pad", "rrc", "eval", "resize"), crop_mode
        self.crop_mode = crop_mode
        self.out_size = int(out_size if out_size is not None
                            else images.shape[1])
        self._param_cache = {}
        self.epoch = 0
        self.mean = (torch.tensor(mean, device=device).view(1, 1, 1, -1)
                     * 255.0)
        self.std = (torch.tensor(std, device=device).view(1, 1, 1, -1)
                    * 255.0)
        n = len(self.labels)
        import math
        if drop_last and n % world != 0:
            self.num_samples = n // world
        else:
            self.num_samples = math.ceil(n / world)

    def set_epoch(self, epoch):
        self.epoch = epoch

    def __len__(self):
        if self.drop_last:
            return self.num_samples // self.batch_size
        return (self.num_samples + self.batch_size - 1) // self.batch_size

    def _shard_indices(self):
        shard = compute_shard(len(self.labels), self.world, self.rank,
                              self.shuffle, self.seed, self.epoch,
                              self.drop_last)
        return shard.to(self.device)

    def _resample_params(self, n, g):
        """(params, flip) rows for ops.crop_resize, per crop mode."""
        from .device_augment import eval_params, resize_params, rrc_params
        Hs, Ws = self.images.shape[1], self.images.shape[2]
        mode = self.crop_mode
        if mode == "rrc" and not self.augment:
            mode = "eval"
        if mode == "rrc":
            return rrc_params(n, Hs, Ws, self.out_size, g, self.device)
        key = (mode, n)  # eval / resize rows are constants: build once
        if key not in self._param_cache:
            fn = eval_params if mode == "eval" else resize_params
            self._param_cache[key] = fn(n, Hs, Ws, self.out_size,
                                        self.device)
        return self._param_cache[key]

    def _resample_params_ragged(self, idx, g):
        """(params, flip) rows for ops.crop_resize_ragged: the same rules
        with each sample's own (H, W), gathered from the store's table on the
        device. The generator draws are those of _resample_params."""
        from .device_augment import (eval_params_ragged,
                                     resize_params_ragged, rrc_params_ragged)
        mode = self.crop_mode
        if mode == "rrc" and not self.augment:
            mode = "eval"
        if mode == "rrc":
            return rrc_params_ragged(self.images.hw[idx], self.out_size, g)
        if mode not in self._param_cache:  # constant per image: build once
            fn = eval_params_ragged if mode == "eval" else \
                resize_params_ragged
            self._param_cache[mode] = fn(self.images.hw, self.out_size)[0]
        return (self._param_cache[mode][idx],
                torch.zeros(idx.shape[0], dtype=torch.uint8,
                            device=self.device))

    def _crop_resize(self, idx, g, *norm):
        """One fused launch for samples ``idx``: dense or ragged source."""
        if self.ragged:
            from ..ops import crop_resize_ragged
            params, flip = self._resample_params_ragged(idx, g)
            st = self.images
            return crop_resize_ragged(st.pool, st.offsets, st.hw,
                                      st.channels, idx, params, flip,
                                      self.out_size, *norm)
        from ..ops import crop_resize
        params, flip = self._resample_params(idx.shape[0], g)
        return crop_resize(self.images, idx, params, flip, self.out_size,
                           *norm)

    def __iter__(self):
        shard = self._shard_indices()
        g = torch.Generator(device=self.device)
        g.manual_seed(self.seed * 1000003 + self.epoch * 131 + self.rank)
        nb = len(self)
        aug = self.aug_pipeline if self.augment else None
        resample = self.crop_mode != "pad"
        aug_imgs = None
        if aug is not None and (aug.enabled or aug.color_jitter > 0):
            # EPOCH-level batched RandAugment + jitter over the whole shard:
            # per-batch application is host-sync/launch-bound (~200 launches
            # + op-subset syncs per 128-batch cost 2/3 of step throughput);
            # one pass per epoch amortizes that ~40x. Results are integral
            # 0..255 so they round-trip through uint8 exactly.
            # Order: the resampling modes (crop_mode rrc/eval/resize, large
            # inputs) crop+flip FIRST, in uint8, then RA/jitter run on the
            # crops - the host order crop -> flip -> RA -> jitter ->
            # normalize -> erase. The small-input crop_mode="pad" path keeps
            # its documented deviation: RA/jitter run before the per-batch
            # pad-crop/flip instead of after.
            outs = []
            for c0 in range(0, shard.shape[0], 4096):
                if resample:
                    chunk = self._crop_resize(shard[c0:c0 + 4096], g)
                else:
                    chunk = self.images[shard[c0:c0 + 4096]]
                outs.append(aug(chunk, g).to(torch.uint8))
            aug_imgs = torch.cat(outs)
            del outs
        for b in range(nb):
            idx = shard[b * self.batch_size:(b + 1) * self.batch_size]
            if resample and aug_imgs is None:
                # one fused launch: resident uint8 -> normalized dtype
                imgs = self._crop_resize(idx, g, self.mean.view(-1),
                                         self.std.view(-1), self.dtype)
            else:
                if aug_imgs is not None:
                    imgs = aug_imgs[b * self.batch_size:
                                    (b + 1) * self.batch_size].float()
                else:
                    imgs = self.images[idx].float()
                if self.augment and not resample:
                    imgs = self._crop_flip(imgs, g)
                imgs = ((imgs - self.mean) / self.std).to(self.dtype)
            if aug is not None and aug.reprob > 0:
                imgs = aug.erase(imgs, g)
            yield imgs, self.labels[idx], None

    def _crop_flip(self, imgs, g):
        N, H, W, C = imgs.shape
        p = self.pad
        padded = torch.zeros(N, H + 2 * p, W + 2 * p, C, device=self.device)
        padded[:, p:p + H, p:p + W] = imgs
        oy = torch.randint(0, 2 * p + 1, (N,), device=self.device,
                           generator=g)
        ox = torch.randint(0, 2 * p + 1, (N,), device=self.device,
                           generator=g)
        rows = oy.view(N, 1) + torch.arange(H, device=self.device)
        cols = ox.view(N, 1) + torch.arange(W, device=self.device)
        imgs = padded[torch.arange(N, device=self.device).view(N, 1, 1),
                      rows.view(N, H, 1), cols.view(N, 1, W)]
        flip = torch.rand(N, device=self.device, generator=g) < 0.5
        imgs[flip] = imgs[flip].flip(2)
        return imgs
