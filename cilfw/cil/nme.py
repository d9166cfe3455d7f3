"""Nearest-mean-of-exemplars (NME) evaluation — iCaRL's classifier on top of
the herded rehearsal memory (``--nme_eval``).

After each task the engine builds one unit-norm prototype per seen class from
the CURRENT model's features of the memory's exemplars (``build_prototypes``)
and classifies the cumulative validation set by the nearest prototype
(``evaluate_nme``). Next to the linear head's "CNN" accuracy this is the
standard control for head bias: an NME curve well above the CNN curve means
weight aligning has not removed the old/new bias.

Features are ``model.extract_vector`` in eval mode on un-augmented images
(eval crop mode at large inputs). iCaRL's extra averaging of each exemplar
with its horizontally flipped copy is deliberately NOT done (TODO.md).
Neither function consumes random numbers: a run with ``--nme_eval`` trains
exactly like one without.
"""

import contextlib

import numpy as np
import torch

from .. import ops
from ..utils.metrics import MetricLogger


@contextlib.contextmanager
def _torch_rng_kept():
    """A host DataLoader draws its base seed from the global torch generator
    every time it is iterated; put the state back so the extra passes leave
    the training stream untouched."""
    state = torch.get_rng_state()
    try:
        yield
    finally:
        torch.set_rng_state(state)


class _Resident:
    """Stand-in taskset that lets GpuTaskLoader serve already resident
    images: ``x`` only tells it the kind and count of images."""

    def __init__(self, x, y):
        self.x, self.y = x, y


def _resident_loader(images, labels, device, args):
    """Unshuffled, un-augmented GpuTaskLoader over device-resident exemplars
    (uint8 tensor or RaggedImageStore): nothing is uploaded or decoded."""
    from ..data import DATASET_STATS
    from ..data.gpu_pipeline import GpuTaskLoader
    from ..engine import _crop_modes, compute_dtype
    mean, std = DATASET_STATS[getattr(args, "_stats_key", "synthetic")]
    kw = dict(shuffle=False, augment=False, drop_last=False,
              dtype=compute_dtype(args), workers=args.workers,
              **_crop_modes(args)[1])
    if torch.is_tensor(images):
        # an empty task part + the resident tensor as the "replay" part
        empty = _Resident(np.empty((0,) + tuple(images.shape[1:]), np.uint8),
                          np.empty(0, np.int64))
        return GpuTaskLoader(empty, args.batch_size, device, mean, std,
                             extra=(images, labels), **kw)
    ts = _Resident(np.empty(len(images), dtype=object),
                   labels.cpu().numpy())
    return GpuTaskLoader(ts, args.batch_size, device, mean, std,
                         store=images, **kw)


def memory_segments(memory, nb_seen):
    """Row offsets (nb_seen + 1,) of the class segments of ``memory.get()``
    (sorted classes, herding rank). Every seen class needs an exemplar."""
    counts = [len(memory._y[c]) if c in memory._y else 0
              for c in range(nb_seen)]
    if set(memory._y) - set(range(nb_seen)) or min(counts, default=0) < 1:
        missing = [c for c, k in enumerate(counts) if k < 1]
        raise ValueError(
            f"--nme_eval needs at least one exemplar of each of the "
            f"{nb_seen} seen classes, but the rehearsal memory holds none "
            f"for classes {missing[:10]}{'...' if len(missing) > 10 else ''}"
            f" (memory classes: {len(memory._y)}): raise --memory_size to "
            f"at least the number of classes "
            f"(--memory_size {memory.memory_size})")
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


@torch.no_grad()
def build_prototypes(model, memory, device, args, mirror=None):
    """(C, D) fp32 unit-norm class prototypes from the current model's
    features of the memory's exemplars, C = classes seen so far. With a
    DeviceReplayMirror the resident exemplar images are read in place;
    without one the exemplars take the loader extract_task_features picks.
    Replicated on every rank, like herding."""
    from ..engine import extract_task_features
    seg_off = memory_segments(memory, model.fc.nb_classes)
    with _torch_rng_kept():
        if mirror is not None:
            images, labels, _tasks = mirror.get()
            assert len(labels) == seg_off[-1], \
                "device replay mirror out of sync with rehearsal memory"
            model.eval()
            feats = [model.extract_vector(inputs).float() for inputs, _y, _t
                     in _resident_loader(images, labels, device, args)]
            model.train()
            feats = torch.cat(feats)
        else:
            from ..data.scenario import TaskSet
            feats = extract_task_features(model, TaskSet(*memory.get()),
                                          device, args)
    return ops.nme_prototypes(feats, seg_off)


def _shard_size(loader):
    """Samples this rank's pass over ``loader`` yields, or None."""
    n = getattr(loader, "num_samples", None)  # GpuTaskLoader
    if n is None and getattr(loader, "sampler", None) is not None \
            and not getattr(loader, "drop_last", False):
        n = len(loader.sampler)
    return n


@torch.no_grad()
def evaluate_nme(model, protos, loader, device, args):
    """One backbone-only pass over the rank's validation shard into a single
    fp32 feature buffer, then ONE fused ops.nme_topk launch over it.
    Cross-rank sample-weighted means as in engine.evaluate. -> (nme1, nme5)."""
    from ..engine import _to_device, compute_dtype
    model.eval()
    dtype = compute_dtype(args)
    dev = torch.device(device)
    C, D = protos.shape
    kmax = min(5, C)
    n = _shard_size(loader)
    with _torch_rng_kept():
        if n is None:
            fl, tl = [], []
        else:
            feats = torch.empty(n, D, dtype=torch.float32, device=dev)
            tgts = torch.empty(n, dtype=torch.int64, device=dev)
        o = 0
        for inputs, targets, _tids in loader:
            inputs, targets = _to_device(inputs, targets, device, dtype)
            f = model.extract_vector(inputs)
            b = f.shape[0]
            if n is None:
                fl.append(f.float())
                tl.append(targets)
            else:
                feats[o:o + b] = f
                tgts[o:o + b] = targets
            o += b
        if n is None:
            feats = torch.cat(fl) if fl else torch.empty(0, D, device=dev)
            tgts = torch.cat(tl) if tl else \
                torch.empty(0, dtype=torch.int64, device=dev)
        assert o == feats.shape[0], \
            f"validation pass yielded {o} samples, expected {feats.shape[0]}"
    _idx, _score, counts = ops.nme_topk(feats, protos, kmax, tgts)
    counts = counts.tolist()  # the one host sync
    metric_logger = MetricLogger()
    metric_logger.update_n(n=o, nme1=counts[0] * 100.0 / max(o, 1))
    metric_logger.update_n(n=o, nme5=counts[kmax - 1] * 100.0 / max(o, 1))
    metric_logger.synchronize_between_processes(device=dev)
    nme1 = metric_logger.meters["nme1"].global_avg
    nme5 = metric_logger.meters["nme5"].global_avg
    print(f"* NME Acc@1 {nme1:.3f} Acc@5 {nme5:.3f}")
    model.train()
    return nme1, nme5
