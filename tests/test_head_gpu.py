"""Classifier-head GEMMs (csrc/gemm.hip), WA / CE / KD losses and top-k
(csrc/loss.hip) against the fp64 references of _head_ref (pytest -m gpu).
Shapes, inputs and allowances are those of _head_ref; every element is
compared, and every case prints its max err/bound."""

import pytest
import torch

import _head_ref as R
import cilfw.ops.functional as CF

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(),
                                 reason="needs GPU")]

DEV = "cuda:0"
T, LAM = R.T_KD, R.LAM


def _H():
    from cilfw import _hip_ops as H
    return H


# --------------------------------------------------------------------- linear

def _linear_run(x, w, b, dy):
    H = _H()
    xd, wd, dyd = x.to(DEV), w.to(DEV), dy.to(DEV)
    bd = b.to(DEV) if b is not None else None
    y = H.linear_fwd(xd, wd, bd)
    dx, dw, db = H.linear_bwd(dyd, xd, wd, b is not None)
    torch.cuda.synchronize()
    return y, dx, dw, db


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("shape,splits", R.LINEAR_SHAPES, ids=R.LINEAR_IDS)
def test_linear_kernels(shape, splits, bias):
    M, N, K = shape
    assert _H().linear_ksplits(M, N, K) == splits
    x, w, b, dy = R.linear_inputs(M, N, K)
    if not bias:
        b = None
    ref = R.linear_ref(x, w, b, dy, splits)
    y, dx, dw, db = _linear_run(x, w, b, dy)
    assert y.dtype == torch.bfloat16 and dx.dtype == torch.bfloat16
    assert dw.dtype == torch.float32
    tag = f"linear {shape} {'bias' if bias else 'nobias'}"
    R.linear_check(y, ref["y"], f"{tag} y (split {splits[0]})")
    R.linear_check(dx, ref["dx"], f"{tag} dx (split {splits[1]})")
    R.linear_check(dw, ref["dw"], f"{tag} dW (split {splits[2]})")
    if bias:
        assert db.dtype == torch.float32
        R.linear_check(db, ref["db"], f"{tag} db")
    else:
        assert db is None


def test_linear_autograd():
    """CF.linear: fp32 master weight and bias, grads fp32, same bounds."""
    (M, N, K), splits = R.LINEAR_SHAPES[2]
    x, w, b, dy = R.linear_inputs(M, N, K)
    ref = R.linear_ref(x, w, b, dy, splits)
    xg = x.to(DEV).requires_grad_(True)
    wg = w.float().to(DEV).requires_grad_(True)
    bg = b.to(DEV).requires_grad_(True)
    y = CF.linear(xg, wg, bg)
    y.backward(dy.to(DEV))
    assert wg.grad.dtype == torch.float32 and bg.grad.dtype == torch.float32
    R.linear_check(y, ref["y"], "CF.linear y")
    R.linear_check(xg.grad, ref["dx"], "CF.linear dx")
    R.linear_check(wg.grad, ref["dw"], "CF.linear dW")
    R.linear_check(bg.grad, ref["db"], "CF.linear db")


@pytest.mark.parametrize("which", [2, 3, 4],
                         ids=[R.LINEAR_IDS[i] for i in (2, 3, 4)])
def test_linear_split_rerun_bit_identical(which):
    (M, N, K), splits = R.LINEAR_SHAPES[which]
    assert max(splits) > 1
    x, w, b, dy = R.linear_inputs(M, N, K)
    a = _linear_run(x, w, b, dy)
    c = _linear_run(x, w, b, dy)
    for u, v in zip(a, c):
        assert torch.equal(u, v)


# --------------------------------------------------------------------- losses

def _wa_run(s, t, y, smooth, up):
    x = s.to(DEV).requires_grad_(True)
    td = t.to(DEV) if t is not None else None
    total, ce, kd = CF.wa_loss(x, td, y.to(DEV), smooth, T, LAM)
    (total * up).backward()
    torch.cuda.synchronize()
    return total.detach(), ce.detach(), kd.detach(), x.grad


@pytest.mark.parametrize("scale", R.SCALES)
@pytest.mark.parametrize("shape", R.WA_SHAPES, ids=R.WA_IDS)
def test_wa_loss(shape, scale):
    M, C, Ck = shape
    s, t, y = R.loss_inputs(M, C, Ck, scale, torch.bfloat16)
    forced = {c for c in (0, Ck - 1, Ck, C - 1) if 0 <= c < C}
    assert len(forced & set(y.tolist())) == min(M, len(forced))
    for smooth in (0.0, 0.1):
        for up in (1.0, 0.37):
            ref = R.loss_ref(s, t, y, smooth, T, LAM, up)
            total, ce, kd, g = _wa_run(s, t, y, smooth, up)
            assert g.dtype == torch.bfloat16
            R.loss_check(dict(total=total, ce=ce, kd=kd), g, ref,
                         f"wa_loss {shape} x{scale} s{smooth} up{up}")
    again = _wa_run(s, t, y, smooth, up)
    for u, v in zip((total, ce, kd, g), again):
        assert torch.equal(u, v)


@pytest.mark.parametrize("scale", R.SCALES)
@pytest.mark.parametrize("shape", R.CE_SHAPES, ids=str)
def test_cross_entropy(shape, scale):
    M, C = shape
    s, _, y = R.loss_inputs(M, C, C, scale, torch.float32)
    for smooth, up in ((0.0, 1.0), (0.1, 0.37), (0.1, 1.0)):
        ref = R.loss_ref(s, None, y, smooth, T, 0.0, up, bf16_grad=False)
        x = s.to(DEV).requires_grad_(True)
        loss = CF.cross_entropy(x, y.to(DEV), smooth)
        (loss * up).backward()
        assert x.grad.dtype == torch.float32
        R.loss_check(dict(total=loss.detach()), x.grad, ref,
                     f"ce {shape} x{scale} s{smooth} up{up}")


@pytest.mark.parametrize("scale", R.SCALES)
@pytest.mark.parametrize("shape", R.CE_SHAPES, ids=str)
def test_kd_loss(shape, scale):
    M, C = shape
    s, t, y = R.loss_inputs(M, C, C, scale, torch.float32)
    for up in (1.0, 0.37):
        ref = R.loss_ref(s, t, y, 0.0, T, 1.0, up, ce=False, bf16_grad=False)
        x = s.to(DEV).requires_grad_(True)
        loss = CF.kd_loss(x, t.to(DEV), T)
        (loss * up).backward()
        assert x.grad.dtype == torch.float32
        R.loss_check(dict(kd=loss.detach()), x.grad, ref,
                     f"kd {shape} x{scale} up{up}")


# ---------------------------------------------------------------------- top-k

@pytest.mark.parametrize("M,C,maxk", R.TOPK_CASES)
def test_topk_with_ties(M, C, maxk):
    lg, y = R.topk_case(M, C, maxk)
    # ties in half the rows, counts neither all 0 nor all M, and different
    # from those of higher-index-wins and of a 256-column read
    want = R.topk_case_is_telling(lg, y, maxk)
    lgd, yd = lg.to(DEV), y.to(DEV)
    got = _H().topk_correct(lgd, yd, maxk)
    assert got.dtype == torch.int64 and got.shape == (maxk,)
    assert got.cpu().tolist() == want.tolist()
    # the launcher zeroes the counts: a second call gives the same
    assert _H().topk_correct(lgd, yd, maxk).cpu().tolist() == want.tolist()
    ks = tuple(sorted({1, maxk}))
    acc = CF.accuracy(lgd, yd, topk=ks)
    assert acc == [want[k - 1].item() * 100.0 / M for k in ks]
    # bf16 logits, as the engine passes them
    got16 = _H().topk_correct(lgd.to(torch.bfloat16), yd, maxk)
    assert got16.cpu().tolist() == want.tolist()


def test_topk_constructed_rows():
    lg, y, counts = R.topk_constructed()
    got = _H().topk_correct(lg.to(DEV), y.to(DEV), 5)
    assert got.cpu().tolist() == counts.tolist()
    for i in range(4):        # and row by row
        one = _H().topk_correct(lg[i:i + 1].to(DEV), y[i:i + 1].to(DEV), 5)
        assert one.cpu().tolist() == R.topk_ref(lg[i:i + 1], y[i:i + 1],
                                                5).tolist()


def test_topk_refuses_maxk_out_of_range():
    lg = torch.zeros(2, 20, device=DEV)
    y = torch.zeros(2, dtype=torch.long, device=DEV)
    for maxk in (0, 9):
        with pytest.raises(ValueError, match="maxk"):
            _H().topk_correct(lg, y, maxk)
        with pytest.raises(ValueError, match="maxk"):
            CF.accuracy(lg, y, topk=(1, maxk) if maxk else (0,))
