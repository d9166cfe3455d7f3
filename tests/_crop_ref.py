"""fp64 reference, per-pixel comparator, fp32 kernel model and test inputs for
``crop_resize_kernel`` / ``crop_resize_ragged_kernel`` of csrc/data.hip
(tests/test_crop_resize_oracle_gpu.py,
tests/test_crop_resize_oracle_selftest.py). Numpy only; nothing here imports
``cilfw.ops``.

Reference
---------
The docstring of ``ops.functional.crop_resize_reference`` in fp64. The
parameter rows are read as the fp32 numbers they are; output pixel (i, j) of
sample n, from image ``idx[n]`` (clamped to [0, M-1]) of size (H, W):

    jj = S-1-j if flip[n] else j
    fy = oy + i*sy ; fx = ox + jj*sx
    y0 = clamp(floor(fy), 0, H-1) ; y1 = min(y0+1, H-1) ; ty = fy - y0
    (same in x; t comes from the CLAMPED cell, so below 0 it is negative and
    the lerp extrapolates from cell 0, past the far border y1 == y0 and it
    replicates)
    top = a + tx*(b-a) ; bot = d + tx*(e-d) ; v = top + ty*(bot-top)

``i*sy`` has at most 6 + 24 bits and the sums stay far inside fp64, so the
fp64 coordinates are the exact ones. ``reference`` returns the unfloored
``clamp(v, 0, 255)`` together with the allowance and the admissible levels.

Allowance A (levels, per pixel)
-------------------------------
Counted from the kernel's fp32 arithmetic, nothing fitted to its output.
``u = 2^-24``; a rounding of a result whose exact value is x costs ``u|x|``,
and costs NOTHING where its operands are exact and x is an fp32 number
(checked by casting x to fp32 and back). So A is exactly 0 wherever every
intermediate is fp32-exact: dyadic scales, t = 0, four equal taps.

* coordinates: ``fl(o + fl(i*s))``: ``df = rnd(i*s) + rnd(o + i*s)``.
  ``t = f - y0`` is exact in fp32 (y0 is an integer no larger than |f| on the
  same side of 0, or 0), so ``dt = df``.
* v is continuous and piecewise bilinear in (fx, fy), across cell borders and
  across both clamps, so moving the coordinates by (dfx, dfy) moves v by at
  most ``gx*dfx + gy*dfy`` with the slopes taken from the actual taps,
  ``gx = |1-ty||b-a| + |ty||e-d|``, ``gy = |1-tx||d-a| + |tx||e-b|``: a
  ``floor`` that flips in fp32 is inside this term. A flipped floor means the
  kernel evaluates in the neighbouring cell, so slopes and the roundings below
  are the largest of the nine points (fy + {-dfy, 0, dfy}, fx + {-dfx, 0, dfx}).
* the three lerps, ``b-a`` being exact (integers):
      e_top = rnd(tx(b-a)) + rnd(top)          (e_bot alike)
      e_dbt = e_top + e_bot + rnd(bot-top)
      e_p   = |ty| e_dbt + rnd(ty(bot-top))
      A_rnd = e_top + e_p + rnd(v)
  An inexact t times a zero tap difference, and an exact t = 0 times an
  inexact difference, are exactly 0 and cost nothing.
* ``A = (gx dfx + gy dfy + A_rnd) (1 + 2^-16)``; the factor holds the
  second-order terms (roundings of perturbed values, slopes at perturbed t:
  relative 1e-5 at the most with |f| < 2^7 and taps <= 255).

Judgement
---------
uint8   level in [floor(clamp(v-A)), floor(clamp(v+A))]; where the ends agree
        (a DECIDED pixel) that is equality. The ends never differ by more
        than one level (asserted for every input).
fp32    the kernel forms ``fl(fl(l - m) / s)`` with l an admissible level and
        m, s the fp32 ``mean255[c]``, ``std255[c]``. With q = (l - m)/s in
        fp64: ``fl(l - m) = (l - m)(1 + e1)``, the correctly rounded divide
        adds (1 + e2), |e| <= u, so ``|out - q| <= (2u + u^2)|q|``. With
        2^E <= |q| < 2^(E+1), ulp(q) = 2^(E-23) and u|q| < 2^(E-23): one
        rounding is less than one ulp of q, two of them (the u^2 term is
        far below the slack) less than two: ``|out - q| <= 2 ulp(q)``.
bf16    the kernel rounds that fp32 value to nearest-even. Rounding is
        monotone, so the output must lie between the RNE bf16 of the smallest
        and of the largest fp32 number within 2 ulp(q) of q: one value, or two
        neighbours where a bf16 tie lies within 2 fp32 ulps of q.
``judge`` returns the share of UNDECIDED pixels with its verdict; it is a
property of the inputs and the reference alone and the tests cap it per tier.

Inputs
------
``tier1_cases`` (exact: share 0 asserted), ``tier2_cases`` (generic scales)
and the builders of the two > 2^31-byte cases. The RandomResizedCrop rows of
tier 2 were sampled once with a device generator on an MI355X and are kept in
tests/golden/crop_rrc_rows.npz so that the CPU self-test judges exactly the
rows the GPU test uses (device and CPU generators are different streams).
"""

import os

import numpy as np
import torch

U = 2.0 ** -24
SECOND_ORDER = 1.0 + 2.0 ** -16

MEAN = (0.5071, 0.4865, 0.4409, 0.5)
STD = (0.2673, 0.2564, 0.2761, 0.25)
MODES = ("u8", "f32", "bf16")
VEC = {"u8": 16, "f32": 4, "bf16": 8}     # elements per 16-byte lane
BLOCK = 256                                # DNT of csrc/data.hip
PREFILL_U8 = 0xA5
BF16_NAN = 0x7FC0


def stats(C):
    """fp32 (mean255, std255) as the project's callers form them."""
    m = (torch.tensor(MEAN[:C]) * 255).numpy()
    s = (torch.tensor(STD[:C]) * 255).numpy()
    return m, s


# ---------------------------------------------------------------- reference

def _rep32(x):
    return x.astype(np.float32).astype(np.float64) == x


def _rnd(x, dirty):
    """Cost of rounding a result whose exact value is ``x`` to fp32; nothing
    where the operands are exact (not ``dirty``) and x is an fp32 number."""
    return np.where(dirty | ~_rep32(x), U * np.abs(x), 0.0)


def _coords(o, s, k):
    p = k * s
    f = o + p
    dp = _rnd(p, np.zeros(p.shape, bool))
    return f, dp + _rnd(f, dp > 0)


def _cell(f, n):
    i0 = np.clip(np.floor(f), 0, n - 1)
    i1 = np.minimum(i0 + 1, n - 1)
    return i0.astype(np.int64), i1.astype(np.int64), f - i0


def _eval(img, fy, fx, dirty_y, dirty_x):
    """Bilinear value, slope bounds and lerp roundings at (fy[:, None],
    fx[None, :]) -> four (S, S, C) arrays."""
    H, W, _ = img.shape
    y0, y1, ty = _cell(fy, H)
    x0, x1, tx = _cell(fx, W)
    a, b = img[y0][:, x0], img[y0][:, x1]
    d, e = img[y1][:, x0], img[y1][:, x1]
    ty, tx = ty[:, None, None], tx[None, :, None]
    dy = np.broadcast_to(dirty_y[:, None, None], a.shape)
    dx = np.broadcast_to(dirty_x[None, :, None], a.shape)
    p1, p2 = tx * (b - a), tx * (e - d)
    top, bot = a + p1, d + p2
    dbt = bot - top
    p3 = ty * dbt
    v = top + p3
    gx = np.abs(1 - ty) * np.abs(b - a) + np.abs(ty) * np.abs(e - d)
    gy = np.abs(1 - tx) * np.abs(d - a) + np.abs(tx) * np.abs(e - b)
    # i_*: the kernel's value may differ from the exact one (an inexact t
    # times a zero tap difference is still exactly 0)
    i_p1, i_p2 = dx & (b != a), dx & (e != d)
    r1, r2 = _rnd(p1, i_p1), _rnd(p2, i_p2)
    e_top = r1 + _rnd(top, i_p1 | (r1 > 0))
    e_bot = r2 + _rnd(bot, i_p2 | (r2 > 0))
    i_dbt = i_p1 | i_p2 | (e_top > 0) | (e_bot > 0)
    e_dbt = e_top + e_bot + _rnd(dbt, i_dbt)
    t0 = ~dy & (ty == 0)          # an exact zero weight: the product is 0
    i_p3 = ((i_dbt | (e_dbt > 0)) & ~t0) | (dy & (dbt != 0))
    e_p = np.abs(ty) * e_dbt + _rnd(p3, i_p3)
    i_v = i_p1 | (e_top > 0) | i_p3 | (e_p > 0)
    a_rnd = e_top + e_p + _rnd(v, i_v)
    return v, gx, gy, a_rnd


def _sample(img, row, fl, S):
    oy, ox, sy, sx = (float(np.float32(r)) for r in row)
    k = np.arange(S, dtype=np.float64)
    fy, dfy = _coords(oy, sy, k)
    fx, dfx = _coords(ox, sx, (S - 1) - k if fl else k)
    img = img.astype(np.float64)
    dirty_y, dirty_x = dfy > 0, dfx > 0
    v, gx, gy, a_rnd = _eval(img, fy, fx, dirty_y, dirty_x)
    if dirty_y.any() or dirty_x.any():
        for sgy in (-1, 0, 1):
            for sgx in (-1, 0, 1):
                if sgy == 0 and sgx == 0:
                    continue
                _, gx2, gy2, a2 = _eval(img, fy + sgy * dfy, fx + sgx * dfx,
                                        dirty_y, dirty_x)
                gx, gy = np.maximum(gx, gx2), np.maximum(gy, gy2)
                a_rnd = np.maximum(a_rnd, a2)
    geo = gx * dfx[None, :, None] + gy * dfy[:, None, None]
    return v, (geo + a_rnd) * SECOND_ORDER


class Ref:
    """v: clamp(value, 0, 255) unfloored; A: allowance; lo, hi: the
    admissible levels (int64); all (N, S, S, C)."""

    def __init__(self, raw, A):
        self.v = np.clip(raw, 0.0, 255.0)
        self.A = A
        self.lo = np.floor(np.clip(raw - A, 0.0, 255.0)).astype(np.int64)
        self.hi = np.floor(np.clip(raw + A, 0.0, 255.0)).astype(np.int64)

    @property
    def undecided(self):
        return float((self.lo != self.hi).mean())


def reference(images, idx, params, flip, S):
    """images: list of (H, W, C) uint8 arrays; idx: N ints (clamped to
    [0, M-1]) or None (identity); params (N, 4) fp32; flip (N,) -> Ref."""
    M = len(images)
    params = np.asarray(params, dtype=np.float32)
    N = params.shape[0]
    ms = range(N) if idx is None else [min(max(int(m), 0), M - 1) for m in idx]
    raw, A = [], []
    for n, m in enumerate(ms):
        v, a = _sample(np.asarray(images[m]), params[n], int(flip[n]) != 0, S)
        raw.append(v)
        A.append(a)
    return Ref(np.stack(raw), np.stack(A))


# --------------------------------------------------------------- comparator

def rne_bf16(x32):
    """fp32 array -> uint16 bf16 bits, round to nearest even (finite input)."""
    b = np.ascontiguousarray(x32, dtype=np.float32).view(np.uint32)
    return ((b + np.uint32(0x7FFF) + ((b >> np.uint32(16)) & np.uint32(1)))
            >> np.uint32(16)).astype(np.uint16)


def bf16_value(bits):
    return (np.ascontiguousarray(bits, dtype=np.uint16).astype(np.uint32)
            << np.uint32(16)).view(np.float32)


def _ulp32(q):
    """ulp of the fp32 binade that holds |q| (fp64 in, fp64 out; 0 at 0)."""
    _, ex = np.frexp(np.abs(q))            # |q| = m 2^ex, m in [0.5, 1)
    return np.where(q == 0, 0.0, np.ldexp(1.0, np.maximum(ex - 1, -126) - 23))


def _f32_interval(q):
    """Smallest and largest fp32 numbers within 2 ulp(q) of q."""
    w = 2 * _ulp32(q)
    lo = (q - w).astype(np.float32)
    lo = np.where(lo.astype(np.float64) < q - w,
                  np.nextafter(lo, np.float32(np.inf)), lo)
    hi = (q + w).astype(np.float32)
    hi = np.where(hi.astype(np.float64) > q + w,
                  np.nextafter(hi, np.float32(-np.inf)), hi)
    return lo.astype(np.float32), hi.astype(np.float32)


def to_numpy(out):
    """torch output of either kernel -> numpy (bf16 as uint16 bits)."""
    if torch.is_tensor(out):
        out = out.detach().cpu()
        if out.dtype == torch.bfloat16:
            return out.contiguous().view(torch.int16).numpy().view(np.uint16)
        return out.numpy()
    return np.asarray(out)


def judge(ref, out, mode, mean255=None, std255=None):
    """-> (reason or None, share of undecided pixels). ``out``: uint8 levels,
    fp32 values or bf16 bits (uint16 / torch.bfloat16), shaped like ref.v."""
    out = to_numpy(out)
    share = ref.undecided
    if out.shape != ref.v.shape:
        return f"shape {out.shape}, expected {ref.v.shape}", share
    if (ref.hi - ref.lo).max() > 1:
        return "the allowance spans more than two levels", share
    if mode == "u8":
        if out.dtype != np.uint8:
            return f"dtype {out.dtype}", share
        o = out.astype(np.int64)
        ok = (o >= ref.lo) & (o <= ref.hi)
    else:
        C = ref.v.shape[-1]
        m = np.asarray(mean255, dtype=np.float32).astype(np.float64)
        s = np.asarray(std255, dtype=np.float32).astype(np.float64)
        assert m.shape == (C,) and s.shape == (C,)
        ok = np.zeros(ref.v.shape, bool)
        for lev in (ref.lo, ref.hi):
            q = (lev - m) / s
            if mode == "f32":
                if out.dtype != np.float32:
                    return f"dtype {out.dtype}", share
                ok |= np.abs(out.astype(np.float64) - q) <= 2 * _ulp32(q)
            else:
                if out.dtype != np.uint16:
                    return f"dtype {out.dtype}", share
                lo32, hi32 = _f32_interval(q)
                val = bf16_value(out)
                ok |= (val >= bf16_value(rne_bf16(lo32))) \
                    & (val <= bf16_value(rne_bf16(hi32)))
    if ok.all():
        return None, share
    n, i, j, c = (int(k) for k in np.argwhere(~ok)[0])
    got = out[n, i, j, c]
    if mode == "bf16":
        got = f"{float(bf16_value(np.array([got]))[0])!r} (0x{int(got):04x})"
    return (f"{int((~ok).sum())} of {ok.size} elements outside the band, "
            f"first at (n, i, j, c) = {(n, i, j, c)}: got {got}, v = "
            f"{ref.v[n, i, j, c]!r} +- {ref.A[n, i, j, c]:.3g}, levels "
            f"[{ref.lo[n, i, j, c]}, {ref.hi[n, i, j, c]}]"), share


def check(ref, out, mode, what, mean255=None, std255=None, cap=None):
    """Assert ``out`` inside the band and the undecided share <= cap (None:
    recorded only); prints the figures first -> share."""
    why, share = judge(ref, out, mode, mean255, std255)
    print(f"{what} {mode}: undecided {100 * share:.3f}%"
          f"{'' if cap is None else f' (cap {100 * cap:g}%)'}")
    assert why is None, f"{what} {mode}: {why}"
    assert cap is None or share <= cap, \
        f"{what}: undecided share {share:.4f} above the cap {cap}"
    return share


def old_band_accepts(got, want_levels, mode, mean255=None, std255=None):
    """The band of test_crop_resize_gpu.py / test_crop_resize_ragged_gpu.py
    (their assertions, copied): <= 1 level on <= 2 % of pixels; fp32 the same
    after de-normalising with 1e-3 slack; bf16 <= 1.6 levels."""
    got = torch.as_tensor(got)
    want = torch.as_tensor(want_levels)
    if mode == "u8":
        d = (got.int() - want.int()).abs()
        return bool(d.max() <= 1 and (d != 0).float().mean() <= 0.02)
    m, s = torch.as_tensor(mean255), torch.as_tensor(std255)
    d = (got.float() * s + m - want.float()).abs()
    if mode == "f32":
        return bool(d.max() <= 1 + 1e-3 and (d > 1e-3).float().mean() <= 0.02)
    return bool(d.max() <= 1.6)


# ------------------------------------------- fp32 model of the kernel + faults

FAULTS = (
    "mirror_S_minus_j", "stale_flip", "stale_row_stride", "stale_clamp",
    "x1_unclamped", "y1_clamp_H", "t_swapped", "tx_unflipped",
    "t_before_clamp", "round_not_floor", "channel_not_reset",
    "stats_next_channel", "bf16_truncation", "no_partial_vector",
    "two_samples_per_lane", "offset_32bit", "idx_unclamped",
)


class Pool:
    """Flat byte source of the model: ``data`` lives at byte ``base`` of a
    virtual pool; any other byte reads as ``fill`` (so a 2^31-byte pool needs
    no memory, and a read outside the pool is visible instead of fatal)."""

    def __init__(self, data, base=0, fill=0xEE):
        self.data = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
        self.base, self.fill = int(base), fill

    def take(self, ix):
        k = ix - self.base
        ok = (k >= 0) & (k < self.data.size)
        return np.where(ok, self.data[np.where(ok, k, 0)],
                        np.uint8(self.fill))


def kernel_model(pool, offsets, hw, C, idx, params, flip, S, mode,
                 mean255=None, std255=None, fault=None):
    """The walk of ``crop_resize_body`` in numpy fp32, element by element of
    the flat output, with the lane structure (16 bytes per lane) explicit so
    that per-lane faults can be seeded. ``pool``: Pool or uint8 array;
    offsets (M,), hw (M, 2): a dense source is the uniform special case.
    ``fault``: one of FAULTS. -> (N, S, S, C) uint8 / fp32 / uint16 bf16 bits;
    elements the (faulty) kernel leaves unwritten hold the tests' prefill."""
    assert fault is None or fault in FAULTS
    f32 = np.float32
    if not isinstance(pool, Pool):
        pool = Pool(pool)
    offsets = np.asarray(offsets, dtype=np.int64)
    hw = np.asarray(hw, dtype=np.int64)
    M = offsets.shape[0]
    params = np.asarray(params, dtype=f32)
    N = params.shape[0]
    flip = np.asarray(flip)
    idx = np.arange(N) if idx is None else np.asarray(idx, dtype=np.int64)
    V = VEC[mode]
    total = N * S * S * C
    e = np.arange(total, dtype=np.int64)
    per, rowlen = S * S * C, S * C
    n = e // per
    i = (e % per) // rowlen
    j = (e % rowlen) // C
    c = e % C
    e0 = e // V * V
    n0 = e0 // per
    prev = np.where(n > n0, n - 1, n)      # the sample before a change
    n_flip = n_stride = n_clamp = n_all = n
    if fault == "stale_flip":
        n_flip = prev
    if fault == "stale_row_stride":
        n_stride = prev
    if fault == "stale_clamp":
        n_clamp = prev
    if fault == "two_samples_per_lane":
        n_all = np.minimum(n, n0 + 1)
        n_flip = n_stride = n_clamp = n_all

    def src_of(ns):
        m = idx[ns]
        if fault == "idx_unclamped":
            bad = (m < 0) | (m >= M)       # reads past the tables: garbage
            mm = np.clip(m, 0, M - 1)
            off = np.where(bad, np.int64(-10 ** 15), offsets[mm])
            return off, hw[mm, 0], hw[mm, 1]
        mm = np.clip(m, 0, M - 1)
        return offsets[mm], hw[mm, 0], hw[mm, 1]

    base, _, _ = src_of(n_all)
    if fault == "offset_32bit":
        base = (base + 2 ** 31) % 2 ** 32 - 2 ** 31
    _, Hc, Wc = src_of(n_clamp)
    _, _, Wr = src_of(n_stride)
    row_elems = Wr * C
    oy, ox, sy, sx = (params[n_all, k] for k in range(4))
    fl = flip[n_flip] != 0

    mirror = S - j if fault == "mirror_S_minus_j" else S - 1 - j
    jj = np.where(fl, mirror, j)
    fy = oy + i.astype(f32) * sy
    fx = ox + jj.astype(f32) * sx
    ymax, xmax = (Hc - 1).astype(f32), (Wc - 1).astype(f32)
    y0f = np.maximum(np.minimum(np.floor(fy), ymax), f32(0))
    x0f = np.maximum(np.minimum(np.floor(fx), xmax), f32(0))
    y0, x0 = y0f.astype(np.int64), x0f.astype(np.int64)
    y1 = np.minimum(y0 + 1, Hc if fault == "y1_clamp_H" else Hc - 1)
    x1 = x0 + 1 if fault == "x1_unclamped" else np.minimum(x0 + 1, Wc - 1)
    ty, tx = fy - y0f, fx - x0f
    if fault == "t_before_clamp":
        ty, tx = fy - np.floor(fy), fx - np.floor(fx)
    if fault == "tx_unflipped":
        fxu = ox + j.astype(f32) * sx
        tx = fxu - np.maximum(np.minimum(np.floor(fxu), xmax), f32(0))
    if fault == "t_swapped":
        ty, tx = tx, ty
    assert ty.dtype == f32 and tx.dtype == f32
    cc = c
    if fault == "channel_not_reset":
        cc = (e0 % C) + (e - e0)           # keeps counting within the lane

    def tap(y, x):
        return pool.take(base + y * row_elems + x * C + cc).astype(f32)

    a, b, d, g = tap(y0, x0), tap(y0, x1), tap(y1, x0), tap(y1, x1)
    top = a + tx * (b - a)
    bot = d + tx * (g - d)
    v = top + ty * (bot - top)
    v = np.minimum(np.maximum(v, f32(0)), f32(255))
    v = np.floor(v + f32(0.5)) if fault == "round_not_floor" else np.floor(v)
    v = np.minimum(v, f32(255))
    assert v.dtype == f32
    if mode == "u8":
        out = v.astype(np.uint8)
        fill = np.uint8(PREFILL_U8)
    else:
        cs = cc % C
        if fault == "stats_next_channel":
            cs = (c + 1) % C
        m32 = np.asarray(mean255, dtype=f32)
        s32 = np.asarray(std255, dtype=f32)
        out = (v - m32[cs]) / s32[cs]
        assert out.dtype == f32
        fill = f32(np.nan)
        if mode == "bf16":
            fill = np.uint16(BF16_NAN)
            if fault == "bf16_truncation":
                out = (out.view(np.uint32) >> np.uint32(16)).astype(np.uint16)
            else:
                out = rne_bf16(out)
    if fault == "no_partial_vector" and total % V:
        out = out.copy()
        out[total // V * V:] = fill
    return out.reshape(N, S, S, C)


# ------------------------------------------------------------------- inputs

SIZES = [(9, 13), (37, 23), (1, 7), (5, 1), (21, 18), (2, 2)]
GUARD = 64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "crop_rrc_rows.npz")


def box(y, x, h, w, S):
    d = float(max(S - 1, 1))
    return [float(y), float(x), (h - 1) / d, (w - 1) / d]


class Case:
    """One input of either kernel. ``images``: list of (H, W, C) uint8
    arrays, what the reference sees. ``dense``: the kernel source is their
    stack (M, H, W, C); else the guarded pool + offsets + hw. idx None: the
    dense kernel's identity gather."""

    def __init__(self, name, images, dense, idx, params, flip, S, cap,
                 old=None):
        self.name, self.images, self.dense = name, images, dense
        self.C = images[0].shape[2]
        self.S = S
        self.idx = None if idx is None else np.asarray(idx, dtype=np.int64)
        self.params = np.asarray(params, dtype=np.float32)
        self.flip = np.asarray(flip, dtype=np.uint8)
        self.N = self.params.shape[0]
        self.cap = cap        # undecided-share cap; None: recorded only
        self.old = old        # an input of the two older GPU tests
        self.mean255, self.std255 = stats(self.C)
        flat = [im.reshape(-1) for im in images]
        guard = np.full(GUARD, 255, np.uint8)
        self.pool = np.concatenate([guard] + flat + [guard])
        lens = [f.size for f in flat]
        self.offsets = np.array([GUARD + sum(lens[:m])
                                 for m in range(len(flat))], dtype=np.int64)
        self.hw = np.array([im.shape[:2] for im in images], dtype=np.int32)
        self._ref = None

    @property
    def total(self):
        return self.N * self.S * self.S * self.C

    @property
    def ref(self):
        if self._ref is None:
            self._ref = reference(self.images, self.idx, self.params,
                                  self.flip, self.S)
        return self._ref

    def model(self, mode, fault=None):
        """kernel_model on this case (the dense layout is the pool with
        uniform sizes: same bytes, same arithmetic)."""
        return kernel_model(self.pool, self.offsets, self.hw, self.C,
                            self.idx, self.params, self.flip, self.S, mode,
                            self.mean255, self.std255, fault)


def _images(sizes, C, seed, zero=False):
    rng = np.random.default_rng(seed)
    return [np.zeros((h, w, C), np.uint8) if zero else
            rng.integers(0, 256, (h, w, C), dtype=np.uint8)
            for h, w in sizes]


# ragged tier 1: (image, box, flip) per output sample; images 7 and -1 clamp
# to 5 and 0. Whole images, 2x2 corners, h = 1, w = 1, every border touched.
_T1_RAGGED = [
    (3, (0, 0, 5, 1), 0),     # 5x1   whole image (w = 1)
    (0, (0, 0, 9, 13), 1),    # 9x13  whole image
    (5, (0, 0, 2, 2), 1),     # 2x2   whole image
    (4, (19, 16, 2, 2), 0),   # 21x18 2x2 far corner
    (1, (30, 0, 7, 23), 1),   # 37x23 bottom band, left to right border
    (1, (5, 3, 1, 17), 0),    # 37x23 h = 1
    (2, (0, 0, 1, 7), 1),     # 1x7   whole image (h = 1)
    (4, (0, 0, 2, 2), 1),     # 21x18 2x2 near corner
    (0, (2, 12, 5, 1), 0),    # 9x13  w = 1 on the right border
    (1, (0, 4, 20, 19), 0),   # 37x23 top and right border
    (7, (0, 0, 2, 2), 1),     # idx >= M: the 2x2 image
    (-1, (4, 0, 5, 13), 0),   # idx < 0: 9x13, bottom and left border
]
# dense tier 1: 21x18 sources, the boxes of the older tests plus the corners
_T1_DENSE = [
    (3, (0, 0, 21, 18), 0), (0, (2, 3, 9, 14), 1), (3, (11, 1, 10, 17), 1),
    (4, (0, 9, 21, 9), 0), (1, (19, 16, 2, 2), 1), (1, (4, 4, 1, 13), 0),
    (2, (1, 0, 19, 1), 1), (9, (0, 0, 2, 2), 1), (-3, (20, 0, 1, 18), 0),
]


def _boxed(name, images, dense, rows, S, cap=0.0):
    return Case(name, images, dense, [r[0] for r in rows],
                [box(*r[1], S) for r in rows], [r[2] for r in rows], S, cap)


def _multi_sample_lane(dense, S, C):
    """N = 37 samples of S*S*C <= 9 bytes: a uint8 lane spans up to 16 of
    them, each with its own (H, W, base, params, flip), and the last vector
    is partial (except C = 4 / S = 2 in fp32, where a lane is whole
    samples). S = 1: rows written directly, dyadic fractions."""
    sizes = [(21, 18)] * 6 if dense else SIZES
    images = _images(sizes, C, 7000 + 10 * S + C + 100 * dense)
    N = 37
    idx = [(5 * n + 1) % 6 for n in range(N)]
    flip = [(n * n + n // 3) % 2 for n in range(N)]
    if S == 1:
        rows = []
        for n in range(N):
            h, w = sizes[idx[n]]
            rows.append([(n * 7 % (4 * h - 3)) / 4.0 if h > 1 else 0.0,
                         (n * 5 % (4 * w - 3)) / 4.0 if w > 1 else 0.0,
                         0.5, 0.25])
    else:
        rows = [box(0, 0, *sizes[idx[n]], S) for n in range(N)]
    kind = "dense" if dense else "ragged"
    return Case(f"{kind}-lane-S{S}-C{C}-N37", images, dense, idx, rows, flip,
                S, 0.0)


def _out_of_range(dense, C, zero):
    """Origins below 0 (the lerp extrapolates from cell 0 with t < 0, then
    the clamp to [0, 255]) and past the far border (replicates); steps of
    1/2 and 1/4 keep everything exact."""
    sizes = [(21, 18)] * 6 if dense else SIZES
    images = _images(sizes, C, 8100 + C + 10 * dense, zero)
    idx = [3, 0, 5, 4, 1, 1, 2, 4]
    flip = [0, 1, 1, 0, 1, 0, 1, 0]
    rows = []
    for n, m in enumerate(idx):
        h, w = sizes[m]
        rows.append([[-1.5, -2.0, 0.5, 0.5],
                     [h - 2.0, w - 1.5, 0.5, 0.25],
                     [-1.5, w - 2.0, 0.25, 0.5],
                     [h + 3.0, -2.0, 0.5, 0.5]][n % 4])
    kind = "dense" if dense else "ragged"
    return Case(f"{kind}-out-of-range-C{C}{'-zero' if zero else ''}", images,
                dense, idx, rows, flip, 9, 0.0)


_cache = {}


def tier1_cases():
    """name -> Case; every one fp32-exact (undecided share 0 asserted)."""
    if "t1" in _cache:
        return _cache["t1"]
    cases = []
    for C in (1, 3, 4):
        for S in (2, 3, 5, 9, 17, 33):
            cases.append(_boxed(f"ragged-S{S}-C{C}",
                                _images(SIZES, C, 100 * C + S), False,
                                _T1_RAGGED, S))
            cases.append(_boxed(f"dense-S{S}-C{C}",
                                _images([(21, 18)] * 5, C, 5000 + 100 * C + S),
                                True, _T1_DENSE, S))
        for S in (1, 2, 3):
            if S == 1 or C == 1:
                cases.append(_multi_sample_lane(False, S, C))
                cases.append(_multi_sample_lane(True, S, C))
        cases.append(_out_of_range(False, C, False))
        cases.append(_out_of_range(True, C, False))
    cases.append(_out_of_range(False, 3, True))
    cases.append(_out_of_range(True, 3, True))
    # identity gather (idx None, N == M) of the dense kernel
    ims = _images([(21, 18)] * 7, 3, 5909)
    c = Case("dense-identity-S9-C3", ims, True, None,
             [box(*r[1], 9) for r in _T1_DENSE[:7]],
             [r[2] for r in _T1_DENSE[:7]], 9, 0.0)
    cases.append(c)
    # partial vector in a block beyond the first: S = 17, C = 3, N = 5 is
    # 4335 elements = 4096 + 239 (uint8: second block, 15 left over),
    # 2 * 2048 + 239 (bf16: third block, 7 left over), 4 * 1024 + 239 (fp32:
    # fifth block, 3 left over) - one N serves the three modes.
    for dense in (False, True):
        rows = (_T1_DENSE if dense else _T1_RAGGED)[:5]
        ims = _images([(21, 18)] * 5 if dense else SIZES, 3, 6000 + dense)
        cases.append(_boxed(f"{'dense' if dense else 'ragged'}-block-"
                            f"boundary-S17-C3-N5", ims, dense, rows, 17))
    for mode in MODES:
        t = 5 * 17 * 17 * 3
        assert t > BLOCK * VEC[mode] and 0 < t % VEC[mode]
    _cache["t1"] = {c.name: c for c in cases}
    assert len(_cache["t1"]) == len(cases)
    return _cache["t1"]


def _golden():
    if "golden" not in _cache:
        with np.load(GOLDEN) as z:
            _cache["golden"] = {k: z[k] for k in z.files}
    return _cache["golden"]


# Tier 2 gathers: the rrc rows were recorded for T2_IDX (a row's box lies
# inside its own image). The deterministic eval / resize rows of the ragged
# sizes are split: the 2-D images under the cap, and the 1-D ones (1x7, 5x1)
# recorded without one. Where one axis is not interpolated (h = 1, w = 1, or
# a scale of exactly 1 as in resize 20x28 -> 20) the value is a 1-D lerp
# a + (m/(S-1)) k (b-a) and sits on an integer, up to the fp32 error of the
# row itself, whenever (S-1) divides m k (b-a): 5 - 29 % of the pixels are
# knife edges by arithmetic, whatever the seed. They are still judged pixel
# by pixel; only the share is not capped.
T2_IDX = [3, 0, 5, 4, 1, 1, 2, 4]
T2_IDX_2D = [0, 5, 4, 1, 1, 4, 0, 1]
T2_IDX_1D = [3, 2, 3, 2]


def tier2_cases():
    """name -> Case; generic scales. The parameter rows come from the
    project's builders (cilfw.data.device_augment): eval / resize rows are
    deterministic, the rrc rows are the recorded device samples (the seed of
    each is in the file; chosen on the CPU, from the reference alone, as the
    one of six with the smallest undecided share)."""
    if "t2" in _cache:
        return _cache["t2"]
    from cilfw.data.device_augment import (eval_params, eval_params_ragged,
                                           resize_params,
                                           resize_params_ragged)
    gold = _golden()
    cases = []
    for S in (14, 20, 24):
        for Hs, Ws in ((37, 23), (20, 28)):
            ims = _images([(Hs, Ws)] * 6, 3, 9000 + S + Hs)
            rows = {
                "rrc": (gold[f"dense_{Hs}x{Ws}_S{S}_params"],
                        gold[f"dense_{Hs}x{Ws}_S{S}_flip"]),
                "eval": eval_params(8, Hs, Ws, S, "cpu"),
                "resize": resize_params(8, Hs, Ws, S, "cpu"),
            }
            for kind, (p, f) in rows.items():
                # a scale of exactly 1 (Hs == S) leaves a 1-D lerp: below
                cap = None if kind == "resize" and S in (Hs, Ws) else 0.05
                cases.append(Case(f"dense-{kind}-{Hs}x{Ws}-S{S}", ims, True,
                                  T2_IDX, np.asarray(p), np.asarray(f), S,
                                  cap))
        ims = _images(SIZES, 3, 9500 + S)
        cases.append(Case(f"ragged-rrc-S{S}", ims, False, T2_IDX,
                          gold[f"ragged_S{S}_params"],
                          gold[f"ragged_S{S}_flip"], S, 0.05))
        for kind, fn in (("eval", eval_params_ragged),
                         ("resize", resize_params_ragged)):
            for tag, idx, cap in (("", T2_IDX_2D, 0.05),
                                  ("-1d", T2_IDX_1D, None)):
                hw_rows = torch.tensor([SIZES[m] for m in idx],
                                       dtype=torch.int32)
                p, f = fn(hw_rows, S)
                cases.append(Case(f"ragged-{kind}{tag}-S{S}", ims, False,
                                  idx, p.numpy(), f.numpy(), S, cap))
    cases += _old_s16_cases()
    _cache["t2"] = {c.name: c for c in cases}
    assert len(_cache["t2"]) == len(cases)
    return _cache["t2"]


def _old_s16_cases():
    """The S = 16 inputs of test_crop_resize_gpu.py and
    test_crop_resize_ragged_gpu.py, taken from those modules: rich in knife
    edges (the last row and column of a corner-to-corner box, and every i
    with i (h-1)/15 an integer, hit integer source coordinates), so the
    share is recorded, not capped."""
    import test_crop_resize_gpu as D
    import test_crop_resize_ragged_gpu as R
    out = []
    for name in ("upsample_9x13", "borders_37x23", "c1_identity_idx"):
        src, idx, boxes, flip = D._case(name, 16)
        params = torch.tensor([D._box(*b, 16) for b in boxes])
        out.append(Case(f"old-dense-{name}-S16", list(src.numpy()), True,
                        None if idx is None else idx.numpy(), params.numpy(),
                        flip.numpy(), 16, None, old="dense"))
    imgs, pool, offs, hw, idx, params, flip, _, _, _ = \
        R._inputs_and_oracle(3, 16)
    c = Case("old-ragged-C3-S16", [i.numpy() for i in imgs], False,
             idx.numpy(), params.numpy(), flip.numpy(), 16, None,
             old="ragged")
    assert np.array_equal(c.pool, pool.numpy()) \
        and np.array_equal(c.offsets, offs.numpy())
    out.append(c)
    return out


# ---------------------------------------------------- past 2^31 bytes, inputs

BIG_POOL_BYTES = 2 ** 31 + 2 ** 20
BIG_DENSE_SHAPE = (70000, 64, 128, 4)      # 2 293 760 000 bytes
BIG_S = 9


def big_ragged():
    """Three small images placed past byte 2^31 of a 2^31 + 2^20-byte pool.
    -> (Case over the three images alone, their byte offsets in the big
    pool). The Case's own compact pool is what the CPU path and the model
    see; the offsets are what the GPU test and the 32-bit fault use."""
    if "big_ragged" not in _cache:
        sizes = [(9, 13), (5, 1), (21, 18)]
        ims = _images(sizes, 3, 31337)
        rows = [(2, (0, 0, 21, 18), 0), (0, (0, 0, 9, 13), 1),
                (1, (0, 0, 5, 1), 1), (2, (19, 16, 2, 2), 0),
                (0, (4, 0, 5, 13), 1), (5, (2, 3, 9, 14), 0)]
        case = _boxed("ragged-past-2^31", ims, False, rows, BIG_S)
        offs, o = [], 2 ** 31 + 12345
        for im in ims:
            offs.append(o)
            o += im.size + 1000
        assert o < BIG_POOL_BYTES
        _cache["big_ragged"] = (case, np.array(offs, dtype=np.int64))
    return _cache["big_ragged"]


def big_dense():
    """The last three images of a (70000, 64, 128, 4) source; idx selects
    them (70000 + 5 clamps to the last). -> (Case over the three images with
    idx 0..2, the idx into the big tensor)."""
    if "big_dense" not in _cache:
        M, H, W, C = BIG_DENSE_SHAPE
        ims = _images([(H, W)] * 3, C, 4242)
        rows = [(2, (0, 0, 64, 128), 0), (0, (0, 0, 64, 64), 1),
                (1, (31, 96, 33, 32), 1), (2, (62, 126, 2, 2), 0),
                (2, (0, 64, 16, 64), 1)]
        case = _boxed("dense-past-2^31", ims, True, rows, BIG_S)
        big_idx = np.array([M - 1, M - 3, M - 2, M - 1, M + 5],
                           dtype=np.int64)
        assert (M - 3) * H * W * C > 2 ** 31
        _cache["big_dense"] = (case, big_idx)
    return _cache["big_dense"]
