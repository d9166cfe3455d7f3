"""crop_resize_kernel / crop_resize_ragged_kernel (csrc/data.hip) against the
fp64 reference and per-pixel band of tests/_crop_ref.py (pytest -m gpu).

Every launch goes through the C entry points of the library with an output
buffer this file owns (the Python wrappers allocate their own and take no
``out=``): NaN-prefilled for fp32 / bf16, 0xA5 for uint8, and 64 elements
longer than the output, so an element the kernel skips and a store past the
end are both visible. The public op is then asked for the same thing and must
return the same bits.

Tier 1 (tests/_crop_ref.py::tier1_cases) is fp32-exact: the allowance is 0,
the band is equality with floor(v) on every pixel, in all three modes, for
the dense and the ragged kernel, C in {1, 3, 4}: integer boxes at S - 1
dyadic; lanes that span up to 16 samples (S = 1, N = 37; S = 2 and 3 at
C = 1) with a partial last vector; a partial vector in the 2nd / 3rd / 5th
block (S = 17, C = 3, N = 5: 4335 elements, 15 / 7 / 3 left over in uint8 /
bf16 / fp32); origins below 0 and past the far border; all-zero images
between 255 guards; one > 2^31-byte source per kernel.

Tier 2 has generic scales (S - 1 prime, and the older tests' S = 16): every
pixel in the band, the undecided share capped as the self-test asserts on the
CPU for the same inputs. In addition the kernel must equal the project's CPU
path bit for bit in all three modes: data.hip compiles with contraction off,
no fast-math flag, a correctly rounded divide, so the two evaluate the same
fp32 expression with the same roundings, knife edges included. Measured on
the MI355X: 0 differing elements on every tier 2 input (COVERAGE.md). It is
the one check that sees a contracted or reordered lerp, which moves values
only on knife edges, inside the oracle band.
"""

import numpy as np
import pytest
import torch

import _crop_ref as CR
from test_crop_resize_oracle_selftest import _cpu_path, _same_bits

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(),
                                 reason="needs GPU")]

DT = {"u8": torch.uint8, "f32": torch.float32, "bf16": torch.bfloat16}
MODE_CODE = {"u8": 0, "f32": 1, "bf16": 2}
PAD = 64


def _bits(t):
    """Flat integer view: NaN prefill compares equal to itself."""
    t = t.contiguous().view(-1)
    return t if t.dtype == torch.uint8 else \
        t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)) \
        .cuda()


def _run(case, mode, source=None, idx=None):
    """Raw launch into a prefilled, padded buffer + the public op -> numpy
    output (bf16 as bits). ``source``: device tensors of a source other than
    the case's own ((src,) dense or (pool, offsets, hw) ragged), with its
    ``idx``."""
    from cilfw import _hip_ops as H
    from cilfw.ops import crop_resize, crop_resize_ragged
    if source is None:
        source = (_dev(np.stack(case.images)),) if case.dense else \
            (_dev(case.pool), _dev(case.offsets), _dev(case.hw))
        idx = case.idx
    idx = _dev(idx)
    params, flip = _dev(case.params), _dev(case.flip)
    mean, std = _dev(case.mean255), _dev(case.std255)
    N, S, C, total = case.N, case.S, case.C, case.total
    fill = CR.PREFILL_U8 if mode == "u8" else float("nan")
    buf = torch.full((total + PAD,), fill, dtype=DT[mode], device="cuda")
    prefill = _bits(buf).clone()
    assert buf.data_ptr() % 16 == 0
    stats = (None, None) if mode == "u8" else (mean, std)
    c_i, ptr = H.c_i, H._ptr
    if case.dense:
        src, = source
        M, Hs, Ws, _ = src.shape
        H._lib.cilfw_crop_resize(
            ptr(src), ptr(idx), ptr(params), ptr(flip), ptr(stats[0]),
            ptr(stats[1]), ptr(buf), c_i(M), c_i(N), c_i(Hs), c_i(Ws),
            c_i(C), c_i(S), c_i(MODE_CODE[mode]), H._stream())
        norm = () if mode == "u8" else (mean, std, DT[mode])
        pub = crop_resize(src, idx, params, flip, S, *norm)
    else:
        pool, offsets, hw = source
        H._lib.cilfw_crop_resize_ragged(
            ptr(pool), ptr(offsets), ptr(hw), ptr(idx), ptr(params),
            ptr(flip), ptr(stats[0]), ptr(stats[1]), ptr(buf),
            c_i(offsets.shape[0]), c_i(N), c_i(C), c_i(S),
            c_i(MODE_CODE[mode]), H._stream())
        norm = () if mode == "u8" else (mean, std, DT[mode])
        pub = crop_resize_ragged(pool, offsets, hw, C, idx, params, flip, S,
                                 *norm)
    torch.cuda.synchronize()
    assert torch.equal(_bits(buf)[total:], prefill[total:]), \
        f"{case.name} {mode}: a store past the end of the output"
    out = buf[:total].view(N, S, S, C)
    assert pub.shape == out.shape and pub.dtype == out.dtype
    assert torch.equal(_bits(pub), _bits(out)), \
        f"{case.name} {mode}: the public op differs from the raw launch"
    return CR.to_numpy(out)


def _judge_all_modes(case, source=None, idx=None, bit_equal_cpu=False):
    for mode in CR.MODES:
        out = _run(case, mode, source, idx)
        CR.check(case.ref, out, mode, case.name, case.mean255, case.std255,
                 cap=case.cap)
        cpu = _cpu_path(case, mode)
        ubits = {1: np.uint8, 2: np.uint16, 4: np.uint32}[out.itemsize]
        ndiff = int((out.view(ubits) != cpu.view(ubits)).sum())
        print(f"{case.name} {mode}: {ndiff} of {out.size} elements differ "
              f"from the CPU path")
        if bit_equal_cpu:
            assert ndiff == 0 and _same_bits(out, cpu), (case.name, mode)
    return out


@pytest.mark.parametrize("name", list(CR.tier1_cases()))
def test_tier1_exact(name):
    """Allowance 0: the band is equality with floor(v) (and with its
    correctly rounded normalisation) on every element. The CPU path is then
    equal too; that is asserted as well, it costs nothing here."""
    case = CR.tier1_cases()[name]
    assert case.ref.A.max() == 0.0 and case.cap == 0.0
    _judge_all_modes(case, bit_equal_cpu=True)
    if name.endswith("-zero"):
        assert int(_run(case, "u8").max()) == 0


def test_out_of_range_rows_hand_worked():
    """The docstring's asymmetry on one 2x2 image [[10, 30], [50, 110]],
    S = 1: below 0 the lerp extrapolates from cell 0 (t < 0) and is clamped
    to [0, 255]; past the far border it replicates."""
    img = [np.array([[[10], [30]], [[50], [110]]], np.uint8)]
    rows = [(0, 0, 10), (0, 0.25, 15), (0.5, 0.5, 50), (0, -0.25, 5),
            (0, -2, 0), (-0.25, 0, 0), (1, -0.5, 20), (-1.5, 1, 0),
            (0, 3, 30), (5, 0, 50), (7.5, 1.75, 110)]
    for dense in (True, False):
        case = CR.Case("hand", img, dense, [0] * len(rows),
                       [[oy, ox, 0.0, 0.0] for oy, ox, _ in rows],
                       [0] * len(rows), 1, 0.0)
        out = _run(case, "u8")
        assert out.reshape(-1).tolist() == [lv for _, _, lv in rows]
        _judge_all_modes(case, bit_equal_cpu=True)


@pytest.mark.parametrize("name", list(CR.tier2_cases()))
def test_tier2_band_and_bit_equal_to_the_cpu_path(name):
    case = CR.tier2_cases()[name]
    _judge_all_modes(case, bit_equal_cpu=True)


def test_fresh_device_sampled_rrc_rows():
    """Rows sampled now with a device generator (the loader's way), copied
    to the host: same judgement, share recorded (the capped inputs are the
    recorded rows of tests/golden/crop_rrc_rows.npz, which these equal as
    long as torch's device generator keeps its stream)."""
    from cilfw.data.device_augment import rrc_params, rrc_params_ragged
    gold = CR._golden()
    for S in (14, 24):
        for key, like in ((f"dense_37x23_S{S}", f"dense-rrc-37x23-S{S}"),
                          (f"ragged_S{S}", f"ragged-rrc-S{S}")):
            base = CR.tier2_cases()[like]
            g = torch.Generator(device="cuda")
            g.manual_seed(int(gold[key + "_seed"]))
            if base.dense:
                p, f = rrc_params(8, 37, 23, S, g, "cuda")
            else:
                hw = _dev(base.hw)[_dev(base.idx)]
                p, f = rrc_params_ragged(hw, S, g)
            same = np.array_equal(p.cpu().numpy(), base.params) \
                and np.array_equal(f.cpu().numpy(), base.flip)
            print(f"{key}: fresh rows equal the recorded ones: {same}")
            case = CR.Case(like + "-fresh", base.images, base.dense,
                           base.idx, p.cpu().numpy(), f.cpu().numpy(), S,
                           None)
            _judge_all_modes(case, bit_equal_cpu=True)


def _need_4gib():
    free, _ = torch.cuda.mem_get_info()
    if free < 4 * 2 ** 30:
        pytest.skip(f"{free / 2 ** 30:.1f} GiB of device memory free, the "
                    f"> 2^31-byte source needs 4 GiB")


def test_ragged_source_past_2_31_bytes():
    """pool + offsets[m] with offsets[m] > 2^31: three small images written
    past byte 2^31 of a 2^31 + 2^20-byte pool; the reference sees only the
    images."""
    _need_4gib()
    case, offs = CR.big_ragged()
    pool = torch.empty(CR.BIG_POOL_BYTES, dtype=torch.uint8, device="cuda")
    pool[:4096] = 0xEE
    for o, im in zip(offs.tolist(), case.images):
        pool[o - 1000:o + im.size + 1000] = 0xEE
        pool[o:o + im.size] = _dev(im.reshape(-1))
    _judge_all_modes(case, (pool, _dev(offs), _dev(case.hw)), case.idx,
                     bit_equal_cpu=True)
    del pool
    torch.cuda.empty_cache()


def test_dense_source_past_2_31_bytes():
    """src + m * img_elems with m * img_elems > 2^31: only the last three
    images of a (70000, 64, 128, 4) source are filled; idx selects them and
    one index >= M, which clamps to the last image."""
    _need_4gib()
    case, big_idx = CR.big_dense()
    src = torch.empty(CR.BIG_DENSE_SHAPE, dtype=torch.uint8, device="cuda")
    src[0] = 0xEE
    src[-4] = 0xEE
    src[-3:] = _dev(np.stack(case.images))
    _judge_all_modes(case, (src,), big_idx, bit_equal_cpu=True)
    del src
    torch.cuda.empty_cache()
