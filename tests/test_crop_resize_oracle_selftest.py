"""CPU self-test of tests/_crop_ref.py, the oracle of the crop_resize kernels:
the reference on hand-worked values, the input properties the GPU test relies
on (tier 1 exact, tier 2 undecided shares under their caps), the project's
CPU path and an fp32 model of the kernel accepted at every GPU input, the
model with one seeded fault each rejected by a named tier 1 input, and what
the two older GPU tests let through: their band accepts wrong bf16 rounding
and a bf16 level that is off by one, and their inputs cannot show a border
tap fault, a lane of three samples, or (at S = 16) stale per-sample state."""

import numpy as np
import pytest
import torch

import _crop_ref as CR
from cilfw.ops import crop_resize, crop_resize_ragged

DT = {"f32": torch.float32, "bf16": torch.bfloat16}


def _cpu_path(case, mode):
    """The project's CPU path on ``case`` (ops.crop_resize /
    crop_resize_ragged on CPU tensors) -> numpy (bf16 as bits)."""
    norm = () if mode == "u8" else (torch.from_numpy(case.mean255),
                                    torch.from_numpy(case.std255), DT[mode])
    params, flip = torch.from_numpy(case.params), torch.from_numpy(case.flip)
    if case.dense:
        idx = None if case.idx is None else torch.from_numpy(case.idx)
        out = crop_resize(torch.from_numpy(np.stack(case.images)), idx,
                          params, flip, case.S, *norm)
    else:
        out = crop_resize_ragged(
            torch.from_numpy(case.pool), torch.from_numpy(case.offsets),
            torch.from_numpy(case.hw), case.C, torch.from_numpy(case.idx),
            params, flip, case.S, *norm)
    return CR.to_numpy(out)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ------------------------------------------------------------- the reference

def test_reference_on_hand_worked_values():
    """One 2x2 image [[10, 30], [50, 110]], S = 1, rows written directly."""
    img = [np.array([[[10], [30]], [[50], [110]]], np.uint8)]

    def v(oy, ox):
        r = CR.reference(img, [0], [[oy, ox, 0.0, 0.0]], [0], 1)
        assert r.A.max() == 0.0
        return float(r.v[0, 0, 0, 0])

    assert v(0, 0) == 10 and v(0, 1) == 30 and v(1, 0) == 50
    assert v(0, 0.25) == 15 and v(0.5, 0) == 30
    assert v(0.5, 0.5) == 50          # top 20, bot 80
    # below 0: t < 0 extrapolates from cell 0, then the clamp
    assert v(0, -0.25) == 5           # 10 - 0.25 * 20
    assert v(0, -2) == 0              # 10 - 2 * 20 = -30 -> 0
    assert v(-0.25, 0) == 0           # 10 - 0.25 * 40
    assert v(1, -0.5) == 20           # 50 - 0.5 * 60
    assert v(-1.5, 1) == 0            # 30 - 1.5 * 80
    # past the far border: replicates
    assert v(0, 3) == 30 and v(5, 0) == 50 and v(7.5, 1.75) == 110
    # an extrapolation above 255 clamps too: [[250, 10]] at fx = -0.5 -> 370
    hi = [np.array([[[250], [10]]], np.uint8)]
    r = CR.reference(hi, [0], [[0.0, -0.5, 0.0, 0.0]], [0], 1)
    assert r.v[0, 0, 0, 0] == 255 and r.lo[0, 0, 0, 0] == 255


def test_allowance_is_zero_only_where_fp32_is_exact():
    img = CR._images([(21, 18)], 3, 1)
    exact = CR.reference(img, [0], [CR.box(2, 3, 9, 14, 17)], [1], 17)
    assert exact.A.max() == 0.0 and exact.undecided == 0.0
    generic = CR.reference(img, [0], [CR.box(2, 3, 9, 14, 16)], [1], 16)
    assert generic.A.max() > 0.0
    assert generic.A.max() < 5e-3     # far below a level
    # four equal taps: exact whatever the scale
    flat = [np.full((21, 18, 3), 77, np.uint8)]
    r = CR.reference(flat, [0], [CR.box(2, 3, 9, 14, 16)], [1], 16)
    assert r.A.max() == 0.0 and (r.v == 77).all()


def test_bf16_and_ulp_helpers():
    x = np.array([1.0, 1.00390625, 1.01171875, -2.5, 3.1415927], np.float32)
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy()
    assert np.array_equal(CR.rne_bf16(x), want.view(np.uint16))
    # 1 + 2^-8 is a tie: to even (down); 1 + 3 * 2^-8 is a tie: to even (up)
    assert CR.rne_bf16(x[1:2])[0] == 0x3F80 and CR.rne_bf16(x[2:3])[0] == 0x3F82
    q = np.array([1.0, 1.5, 1.9999, 2.0, -0.75, 0.0])
    assert np.array_equal(CR._ulp32(q), [2.0 ** -23, 2.0 ** -23, 2.0 ** -23,
                                         2.0 ** -22, 2.0 ** -24, 0.0])
    lo, hi = CR._f32_interval(np.array([1.0]))
    assert lo[0] == np.float32(1 - 2.0 ** -22) \
        and hi[0] == np.float32(1 + 2.0 ** -22)


# -------------------------------------------------- accepted at every input

@pytest.mark.parametrize("name", list(CR.tier1_cases()))
def test_tier1_is_exact_and_accepts_the_cpu_path_and_the_model(name):
    case = CR.tier1_cases()[name]
    assert case.ref.A.max() == 0.0 and case.ref.undecided == 0.0
    for mode in CR.MODES:
        model, cpu = case.model(mode), _cpu_path(case, mode)
        for what, out in (("model", model), ("cpu path", cpu)):
            why, share = CR.judge(case.ref, out, mode, case.mean255,
                                  case.std255)
            assert why is None and share == 0.0, (name, mode, what, why)
        assert _same_bits(model, cpu), (name, mode)
    if name.endswith("-zero"):
        assert case.ref.v.max() == 0.0
        assert int(case.model("u8").max()) == 0


@pytest.mark.parametrize("name", list(CR.tier2_cases()))
def test_tier2_caps_hold_and_accept_the_cpu_path_and_the_model(name):
    case = CR.tier2_cases()[name]
    ref = case.ref
    share = ref.undecided
    print(f"{name}: undecided {100 * share:.3f}%, max A {ref.A.max():.3g}")
    assert (ref.hi - ref.lo).max() <= 1
    # slopes <= 2 * 255, |df| <= 2 u * 64, seven roundings of <= 255: 5e-3
    assert 0.0 < ref.A.max() < 5e-3
    if case.cap is not None:
        assert share <= case.cap, (name, share)
    for mode in CR.MODES:
        model, cpu = case.model(mode), _cpu_path(case, mode)
        for what, out in (("model", model), ("cpu path", cpu)):
            why, _ = CR.judge(ref, out, mode, case.mean255, case.std255)
            assert why is None, (name, mode, what, why)
        # numpy fp32 and torch's CPU ops round alike: the model predicts the
        # CPU path bit for bit, knife edges included
        assert _same_bits(model, cpu), (name, mode)


def _big_model(which, mode, fault=None):
    """The model over a virtual > 2^31-byte source that holds the case's
    images at the offsets the GPU test uses (CR.Pool: no memory needed)."""
    if which == "ragged":
        case, offs = CR.big_ragged()
        data = np.full(int(offs[-1] - offs[0]) + case.images[-1].size, 0xEE,
                       np.uint8)
        for o, im in zip(offs, case.images):
            data[o - offs[0]:o - offs[0] + im.size] = im.reshape(-1)
        pool, idx = CR.Pool(data, base=int(offs[0])), case.idx
        hw = case.hw
    else:
        case, idx = CR.big_dense()
        M, H, W, C = CR.BIG_DENSE_SHAPE
        offs = np.arange(M, dtype=np.int64) * (H * W * C)
        pool = CR.Pool(np.stack(case.images), base=int(offs[M - 3]))
        hw = np.tile(np.array([[H, W]], np.int32), (M, 1))
    return case, CR.kernel_model(pool, offs, hw, case.C, idx, case.params,
                                 case.flip, case.S, mode, case.mean255,
                                 case.std255, fault)


@pytest.mark.parametrize("which", ["ragged", "dense"])
def test_past_2_31_inputs_are_exact_and_accepted(which):
    """The reference sees the small images only; the CPU path runs on the
    same images at compact offsets (the position in the pool is invisible to
    it by construction), the model at the real offsets."""
    case = (CR.big_ragged() if which == "ragged" else CR.big_dense())[0]
    assert case.ref.A.max() == 0.0 and case.ref.undecided == 0.0
    for mode in CR.MODES:
        _, model = _big_model(which, mode)
        for out in (model, _cpu_path(case, mode), case.model(mode)):
            why, _ = CR.judge(case.ref, out, mode, case.mean255, case.std255)
            assert why is None, (which, mode, why)


# ------------------------------------------------------------ seeded faults

# fault -> (tier 1 input, mode) that must reject it
CAUGHT_BY = {
    "mirror_S_minus_j": [("ragged-S5-C3", "u8"), ("dense-S33-C4", "f32")],
    "stale_flip": [("ragged-S5-C3", "u8"), ("dense-S33-C3", "bf16")],
    "stale_row_stride": [("ragged-S5-C3", "u8"), ("ragged-S3-C1", "f32")],
    "stale_clamp": [("ragged-S5-C3", "u8"), ("ragged-lane-S2-C1-N37", "u8")],
    "x1_unclamped": [("ragged-out-of-range-C3", "u8"),
                     ("dense-out-of-range-C4", "bf16")],
    "y1_clamp_H": [("ragged-out-of-range-C1", "u8"),
                   ("dense-out-of-range-C3", "f32")],
    "t_swapped": [("ragged-S5-C3", "u8"), ("dense-S33-C3", "bf16")],
    "tx_unflipped": [("ragged-S5-C3", "u8"), ("dense-S9-C1", "f32")],
    "t_before_clamp": [("ragged-out-of-range-C3", "u8"),
                       ("dense-out-of-range-C1", "f32")],
    "round_not_floor": [("ragged-S5-C3", "u8"), ("dense-S3-C4", "bf16")],
    "channel_not_reset": [("ragged-S5-C3", "u8"), ("dense-S17-C4", "u8")],
    "stats_next_channel": [("ragged-S5-C3", "f32"), ("dense-S2-C4", "bf16")],
    "bf16_truncation": [("ragged-S5-C3", "bf16"), ("dense-S33-C1", "bf16")],
    "no_partial_vector": [("ragged-block-boundary-S17-C3-N5", "u8"),
                          ("dense-block-boundary-S17-C3-N5", "f32"),
                          ("ragged-lane-S1-C3-N37", "bf16")],
    "two_samples_per_lane": [("ragged-lane-S1-C1-N37", "u8"),
                             ("dense-lane-S1-C3-N37", "u8"),
                             ("ragged-lane-S2-C1-N37", "u8"),
                             ("ragged-lane-S3-C1-N37", "u8"),
                             ("ragged-lane-S1-C1-N37", "bf16")],
    "offset_32bit": [("big:ragged", "u8"), ("big:dense", "bf16")],
    "idx_unclamped": [("ragged-S5-C3", "u8"), ("dense-S2-C1", "f32"),
                      ("big:dense", "u8")],
}


def test_every_listed_fault_has_a_catching_case():
    assert sorted(CAUGHT_BY) == sorted(CR.FAULTS)


@pytest.mark.parametrize("fault", CR.FAULTS)
def test_seeded_fault_is_rejected(fault):
    for name, mode in CAUGHT_BY[fault]:
        if name.startswith("big:"):
            case, out = _big_model(name[4:], mode, fault)
        else:
            case = CR.tier1_cases()[name]
            out = case.model(mode, fault)
        why, _ = CR.judge(case.ref, out, mode, case.mean255, case.std255)
        print(f"{fault} on {name} {mode}: {why}")
        assert why is not None, (fault, name, mode)


def test_faults_that_need_a_lane_of_three_samples_pass_two_sample_lanes():
    """Why the multi-sample-lane inputs exist: at S = 5, C = 3 (75 bytes a
    sample) no lane holds a third sample and the fault is invisible."""
    case = CR.tier1_cases()["ragged-S5-C3"]
    for mode in CR.MODES:
        assert _same_bits(case.model(mode, "two_samples_per_lane"),
                          case.model(mode))


# ----------------------------------------------- the band of the older tests

def _old_inputs():
    """Every kernel-vs-CPU-path input of test_crop_resize_gpu.py and
    test_crop_resize_ragged_gpu.py as Cases (S = 16 ones shared with tier 2)."""
    import test_crop_resize_gpu as D
    import test_crop_resize_ragged_gpu as R
    out = []
    for name, S in D.CASES:
        src, idx, boxes, flip = D._case(name, S)
        params = torch.tensor([D._box(*b, S) for b in boxes])
        out.append(CR.Case(f"old-dense-{name}-S{S}", list(src.numpy()), True,
                           None if idx is None else idx.numpy(),
                           params.numpy(), flip.numpy(), S, None))
    for C, S in R.CASES:
        imgs, _, _, _, idx, params, flip, _, _, _ = R._inputs_and_oracle(C, S)
        out.append(CR.Case(f"old-ragged-C{C}-S{S}", [i.numpy() for i in imgs],
                           False, idx.numpy(), params.numpy(), flip.numpy(),
                           S, None))
    return out


def _old_verdicts(fault):
    """Per older input and mode: None where the fault does not change one
    bit of the model's output, else (older band accepts, oracle rejects)."""
    out = {}
    for case in _old_inputs():
        want = _cpu_path(case, "u8")
        for mode in CR.MODES:
            bad = case.model(mode, fault)
            if _same_bits(bad, case.model(mode)):
                out[case.name, mode] = None
                continue
            got = CR.bf16_value(bad) if mode == "bf16" else bad
            old = CR.old_band_accepts(torch.from_numpy(got),
                                      torch.from_numpy(want), mode,
                                      case.mean255, case.std255)
            why, _ = CR.judge(case.ref, bad, mode, case.mean255, case.std255)
            out[case.name, mode] = (old, why is not None)
    return out


def test_the_older_band_accepts_wrong_bf16_rounding_and_a_level_off():
    """<= 1.6 levels after de-normalising is all the older tests ask of the
    bf16 output (the two loader tests ask nothing else): truncation instead
    of round-to-nearest passes on every one of their inputs, and so does a
    bf16 kernel that rounds the level instead of flooring it (one level off
    on half of the pixels). The oracle rejects both on the same inputs."""
    for fault in ("bf16_truncation", "round_not_floor"):
        v = _old_verdicts(fault)
        bf = [v[k] for k in v if k[1] == "bf16"]
        assert len(bf) == 11 and all(r == (True, True) for r in bf), fault
    # in uint8 and fp32 mode the older count (<= 2 % of pixels) does see a
    # level that is off everywhere
    v = _old_verdicts("round_not_floor")
    assert all(v[k] == (False, True) for k in v if k[1] != "bf16")


def test_the_older_inputs_cannot_show_border_tap_or_lane_faults():
    """Not the band but the inputs hide these: every older box is an integer
    box inside its image, so wherever a tap is clamped its weight t is
    exactly 0, and an unclamped x1, a y1 clamped to H, or t taken before the
    clamp change no bit of the output; no lane holds three samples; and at
    S = 16 a sample is a whole number of lanes in every mode, so stale
    per-sample state (flip, stride, clamp) and a lost partial vector cannot
    show either."""
    for fault in ("x1_unclamped", "y1_clamp_H", "t_before_clamp",
                  "two_samples_per_lane"):
        assert all(r is None for r in _old_verdicts(fault).values()), fault
    for fault in ("stale_flip", "stale_row_stride", "stale_clamp",
                  "no_partial_vector"):
        v = _old_verdicts(fault)
        assert all(v[k] is None for k in v if k[0].endswith("-S16")), fault
        # where a straddling lane exists the damage is large, and the older
        # band and the oracle both reject it
        seen = [r for r in v.values() if r is not None]
        assert seen and all(r == (False, True) for r in seen), fault
