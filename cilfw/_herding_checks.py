"""Input checks of herding exemplar selection, shared by ``cil/memory.py``
(torch path) and the HIP wrappers in ``_hip_ops.py``. Pure torch: importable
without the built kernel library.

Why the value bound exists. ``herding_kernel`` / ``herding_batch_kernel``
(csrc/loss.hip) take the candidate with the smallest fp32 squared distance
``d2 = sum_d t_d^2``, ``t_d = (sum_sel_d + f_d) / (k + 1) - mu_d``, and a
candidate wins only through ``d2 < best``. With a NaN or inf feature, or with
finite features so large that ``d2`` overflows, every comparison is false, no
candidate wins, and the kernel would index with its "none yet" sentinel. The
torch path degrades differently (``argmin`` over an all-inf row returns index 0
again: duplicate picks). Both are refused here instead, before any launch.

The bound ``max|f| <= 2^48`` is derived, not measured: ``sum_sel`` holds k
selected rows, so ``|(sum_sel + f) / (k + 1)| <= max|f|`` and, ``mu`` being a
mean of the rows (the raw wrapper checks a caller's ``mu`` against the same
bound), ``|t| <= 2 max|f|`` and ``d2 <= 4 D max|f|^2``. The kernels hold
``n + D <= 15000`` floats of LDS, so ``D <= 15000`` and
``d2 <= 4 * 15000 * 2^96 < 4.8e33``, five orders of magnitude under FLT_MAX
(3.4e38) - room for every rounding on the way. ``sum_sel`` itself stays below
``m * max|f| <= 15000 * 2^48 < 2^62``.

Cost: one device reduction and one host sync per call. Herding runs once per
task (not per step), so the sync is acceptable.
"""

import torch

HERDING_MAX_ABS = 2.0 ** 48
LDS_BYTES = 60_000          # dynamic LDS the wrappers allow: (n + D) * 4


def _bad(a):
    # written so that NaN fails: NaN <= x is False
    return not (a <= HERDING_MAX_ABS)


def check_values(what, *tensors):
    """ValueError unless every element of every tensor is finite and within
    ``HERDING_MAX_ABS``. One sync (``amax`` and ``maximum`` propagate NaN)."""
    a = None
    for t in tensors:
        if t.numel() == 0:
            continue
        b = t.detach().abs().amax()
        a = b if a is None else torch.maximum(a, b)
    if a is None:
        return
    a = a.item()
    if _bad(a):
        raise ValueError(
            f"{what}: features must be finite with max|f| <= 2^48 (got "
            f"max|f| = {a}); a diverged run cannot be herded")


def check_values_batch(flat, sizes, what):
    """As ``check_values`` on the concatenated rows of a batched call; the
    message names the position (in the list) of the first offending class.
    The per-class search only runs on the error path."""
    if flat.numel() == 0:
        return
    a = flat.detach().abs().amax().item()
    if not _bad(a):
        return
    o = 0
    for pos, n in enumerate(sizes):
        rows = flat[o:o + n]
        o += n
        if rows.numel() and _bad(rows.detach().abs().amax().item()):
            raise ValueError(
                f"{what}: class at list position {pos}: features must be "
                f"finite with max|f| <= 2^48; a diverged run cannot be herded")
    raise ValueError(f"{what}: non-finite or oversized features")


def check_select_args(f, mu, m, what="herding_select"):
    """Argument checks of the raw single-class wrapper (no value is read)."""
    if not (torch.is_tensor(f) and f.dim() == 2):
        raise ValueError(f"{what}: features must be a 2-d tensor (n, D)")
    if f.dtype != torch.float32:
        raise ValueError(f"{what}: features must be fp32 (got {f.dtype})")
    if not f.is_contiguous():
        raise ValueError(f"{what}: features must be contiguous")
    n, D = f.shape
    if not (torch.is_tensor(mu) and tuple(mu.shape) == (D,)):
        raise ValueError(
            f"{what}: mu must have shape ({D},) (got "
            f"{tuple(mu.shape) if torch.is_tensor(mu) else type(mu)})")
    if mu.dtype != torch.float32 or not mu.is_contiguous() \
            or mu.device != f.device:
        raise ValueError(
            f"{what}: mu must be a contiguous fp32 tensor on the device of "
            f"the features")
    m = int(m)
    if not 0 <= m <= n:
        raise ValueError(f"{what}: need 0 <= m <= n (got m = {m}, n = {n})")
    return n, D, m


def check_batch_args(feats_list, m_list, what="herding_select_batch"):
    """Argument checks of the batched wrapper -> (sizes, D, device)."""
    feats_list, m_list = list(feats_list), list(m_list)
    if not feats_list:
        raise ValueError(f"{what}: empty class list")
    if len(m_list) != len(feats_list):
        raise ValueError(
            f"{what}: {len(m_list)} quotas for {len(feats_list)} classes")
    f0 = feats_list[0]
    if not (torch.is_tensor(f0) and f0.dim() == 2):
        raise ValueError(
            f"{what}: class at list position 0: features must be a 2-d "
            f"tensor (n, D)")
    D, device = f0.shape[1], f0.device
    for pos, (f, m) in enumerate(zip(feats_list, m_list)):
        if not (torch.is_tensor(f) and f.dim() == 2):
            raise ValueError(
                f"{what}: class at list position {pos}: features must be a "
                f"2-d tensor (n, D)")
        if f.shape[1] != D:
            raise ValueError(
                f"{what}: class at list position {pos}: feature width "
                f"{f.shape[1]} != {D}")
        if f.device != device:
            raise ValueError(
                f"{what}: class at list position {pos}: on {f.device}, the "
                f"first class on {device}")
        if not f.dtype.is_floating_point:
            raise ValueError(
                f"{what}: class at list position {pos}: features must be "
                f"floating point (got {f.dtype})")
        if int(m) < 0:
            raise ValueError(
                f"{what}: class at list position {pos}: negative quota {m}")
    return [int(f.shape[0]) for f in feats_list], int(D), device
