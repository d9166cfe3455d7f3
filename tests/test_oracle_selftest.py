"""CPU self-test of the per-element comparator in ``tests/_oracle.py``.

"Wrong kernels" are built on the CPU from the fp64 reference, rounded to bf16
like a real kernel's output, each with one seeded fault. The comparator must
reject every one and accept the plain fp32 CPU oracle. No GPU involved, so
nothing has to be broken on a device to show the property.
"""

import pytest
import torch
import torch.nn.functional as F

import _oracle as O
import cilfw.ops.functional as CF
from test_ops_gpu import _cmp

# (N, H, W, C, K, k, stride, pad): M = 200 / 50 rows — ragged against any
# tile; C = 128 gives the 3x3x128 reduction the issue's arithmetic is about
GEOMS = [(2, 10, 10, 128, 32, 3, 1, 1),
         (2, 10, 10, 128, 32, 3, 2, 1)]


def _inputs(geom):
    N, H, W, C, K, k, st, pd = geom
    gen = torch.Generator().manual_seed(1234)
    x = O.signed_unit((N, H, W, C), gen)
    w = O.signed_unit((k, k, C, K), gen)
    return x, w


def _round(ref):
    return ref.to(torch.bfloat16)


def _faults(x, w, stride, pad):
    """name -> bf16 output of a kernel with exactly that fault."""
    out = {}
    # one (r,s) tap zeroed
    w1 = w.clone()
    w1[0, 2] = 0
    out["tap_zeroed"] = _round(O.conv_fwd_ref(x, w1, stride, pad)[0])
    # one channel dropped
    x2 = x.clone()
    x2[..., 5] = 0
    out["channel_dropped"] = _round(O.conv_fwd_ref(x2, w, stride, pad)[0])
    # padding row treated as the edge row (replicate instead of zero pad)
    xp = F.pad(x.permute(0, 3, 1, 2).float(), (pad,) * 4, mode="replicate")
    xp = xp.permute(0, 2, 3, 1).to(torch.bfloat16)
    out["pad_is_edge"] = _round(O.conv_fwd_ref(xp, w, stride, 0)[0])
    good = O.conv_fwd_ref(x, w, stride, pad)[0]
    K = good.shape[-1]
    # last M row left unwritten (output buffer was zero-filled)
    y4 = good.clone()
    y4.view(-1, K)[-1] = 0
    out["last_row_unwritten"] = _round(y4)
    # output transposed within one 16x16 block (MFMA C-layout mix-up)
    y5 = good.clone()
    blk = y5.view(-1, K)[16:32, 16:32]
    blk.copy_(blk.t().clone())
    out["block_transposed"] = _round(y5)
    return out


@pytest.mark.parametrize("geom", GEOMS, ids=["3x3s1", "3x3s2"])
def test_comparator_rejects_seeded_faults_accepts_oracle(geom):
    """All five seeded faults are rejected; the fp32 CPU oracle and the
    correctly rounded fp64 reference are accepted."""
    N, H, W, C, K, k, st, pd = geom
    x, w = _inputs(geom)
    ref, mag, n = O.conv_fwd_ref(x, w, st, pd)
    assert O.accepts(_round(ref), ref, mag, n, True)
    y_cpu = CF.conv2d(x, w.float(), st, pd)
    O.check(y_cpu, ref, mag, n, True, "fp32 CPU oracle")
    for name, y_bad in _faults(x, w, st, pd).items():
        r, _ = O.worst(y_bad, ref, mag, n, True)
        assert r > 1.0, f"{name}: fault accepted (err/bound {r:.3g})"


@pytest.mark.parametrize("geom", GEOMS, ids=["3x3s1", "3x3s2"])
def test_comparator_rejects_faulty_dx_and_dw(geom):
    """Same property for the backward outputs: a zeroed tap in dx (bf16) and
    in dW (fp32), and a dW row that was never written."""
    N, H, W, C, K, k, st, pd = geom
    x, w = _inputs(geom)
    gen = torch.Generator().manual_seed(99)
    Ho = (H + 2 * pd - k) // st + 1
    dy = O.signed_unit((N, Ho, Ho, K), gen)
    ref, mag, n = O.conv_dx_ref(dy, w, st, pd, H, W)
    assert O.accepts(_round(ref), ref, mag, n, True)
    w1 = w.clone()
    w1[1, 0] = 0
    bad = _round(O.conv_dx_ref(dy, w1, st, pd, H, W)[0])
    assert not O.accepts(bad, ref, mag, n, True)
    ref, mag, n = O.conv_dw_ref(dy, x, st, pd, k, k)
    assert O.accepts(ref.float(), ref, mag, n, False)
    bad = ref.float().clone()
    bad[2, 1] = 0
    assert not O.accepts(bad, ref, mag, n, False)
    bad = ref.float().clone()
    bad[0, 0, 0, 0] = float("nan")
    assert not O.accepts(bad, ref, mag, n, False)


def _cmp_accepts(got, ref, **kw):
    try:
        _cmp(got, ref, **kw)
    except AssertionError:
        return False
    return True


def test_whole_tensor_cmp_misses_dropped_products():
    """Why the per-element helper exists. ``_cmp`` allows
    ``0.02 + 0.02 * max|ref|`` on every element; with unit-magnitude inputs a
    3x3x128 output reaches |ref| ~ 80, so the allowance is ~1.6 — more than a
    whole product (0.25..1).

    Measured here with ``_cmp``'s forward tolerances (rtol = atol = 0.02):
    it ACCEPTS the first two seeded faults at the granularity a staging bug
    really has — tap (r,s) zeroed for one input channel, and one channel
    dropped at one tap, each a single missing product per output — while the
    per-element comparator rejects both. (Zeroing a whole (r,s) slice or a
    whole channel removes 128 resp. 9 products per output; those sums reach
    ~10 resp. ~5 and ``_cmp`` does reject them at this size — the full-slice
    variants are the ones in the five-fault test above, and the literal
    reading of "_cmp accepts the first two faults" does not hold for them.)
    """
    geom = GEOMS[0]
    N, H, W, C, K, k, st, pd = geom
    x, w = _inputs(geom)
    ref, mag, n = O.conv_fwd_ref(x, w, st, pd)
    good = _round(ref)
    assert _cmp_accepts(good, ref)

    w1 = w.clone()
    w1[0, 2, 7] = 0            # tap (0,2) zeroed, input channel 7 only
    tap = _round(O.conv_fwd_ref(x, w1, st, pd)[0])
    w2 = w.clone()
    w2[1, 1, 5] = 0            # channel 5 dropped at the centre tap
    chan = _round(O.conv_fwd_ref(x, w2, st, pd)[0])
    for name, bad in (("tap", tap), ("channel", chan)):
        assert _cmp_accepts(bad, ref), f"_cmp rejected the {name} fault"
        assert not O.accepts(bad, ref, mag, n, True), \
            f"per-element comparator accepted the {name} fault"



def test_shapes_select_their_routes():
    """The route predicates are pure host code, so the shape -> route table
    of test_conv_routes_gpu.py is also pinned without a GPU."""
    from cilfw import _hip_ops as H
    import test_conv_routes_gpu as T
    for (N, Hh, W, C, K, k, st, pd, route) in T.BN_PARTS_SHAPES:
        assert H.conv2d_fwd_route(N, Hh, W, C, K, k, k, st, pd) == (route, 1)
    assert H.conv2d_fwd_route(9, 30, 30, 512, 128, 1, 1, 1, 0) == \
        ("v2_bn128", 4)
    assert H.conv2d_bwd_data_route(32, 31, 31, 128, 32, 3, 3, 2)[0] == \
        "s2_fused"
    assert H.conv2d_bwd_data_route(13, 110, 110, 32, 24, 3, 3, 2)[0] == "v2"
    assert H.conv2d_bwd_data_route(128, 16, 16, 128, 128, 3, 3, 1)[0] == \
        "v1_bk64"
    assert H.conv2d_bwd_weight_route(4, 64, 128, 1, 1, 4, 4, True)[0] == \
        "v1_fast"
    assert H.conv2d_bwd_weight_route(4, 24, 64, 3, 3, 5, 5, False)[0] == "v2"
    assert H.conv2d_bwd_weight_route(4, 3, 16, 3, 3, 32, 32, False)[0] == \
        "v1_generic"
