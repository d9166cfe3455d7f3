"""BN / SGD entry points exactly as the engine-driven training step calls them
(flat-grad slot delivery, frozen-teacher BN, bf16 mirror + device lr), against
fp64 references (run on MI355X: pytest -m gpu)."""

import pytest
import torch

import _oracle as O

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(),
                                 reason="needs GPU")]

U = O.U_F32
NAN = float("nan")


def _H():
    from cilfw import _hip_ops
    return _hip_ops


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ------------------------------------------------- bn_bwd slot delivery

@pytest.mark.parametrize("C", [16, 64, 256])
@pytest.mark.parametrize("relu,want_dres", [(False, False), (True, False),
                                            (True, True)])
def test_bn_bwd_slot_delivery(C, relu, want_dres):
    """out_gamma/out_beta are views into a larger NaN-filled buffer (the
    flat-grad slots): values bit-equal to the returned-tensor variant and to
    the fp64 sums within fp32 summation error; neighbours untouched."""
    Hop = _H()
    gen = torch.Generator().manual_seed(100 + C)
    M = 8 * 6 * 6 + 5                       # two row blocks, second ragged
    x = torch.randn(M, 1, 1, C, generator=gen).bfloat16()
    dy = O.signed_unit((M, 1, 1, C), gen)
    gamma = torch.rand(C, generator=gen) + 0.5
    beta = torch.randn(C, generator=gen)
    xg, dyg = x.cuda(), dy.cuda()
    rm, rv = torch.zeros(C).cuda(), torch.ones(C).cuda()
    y, mean, invstd = Hop.bn_fwd(xg, gamma.cuda(), beta.cuda(), rm, rv, 0.1,
                                 1e-5, True, relu)
    a = Hop.bn_bwd(dyg, xg, gamma.cuda(), mean, invstd, y, relu, True,
                   want_dres=want_dres)
    a_dg, a_db = a[1].clone(), a[2].clone()

    buf = torch.full((3 * C + 11,), NAN, device="cuda")
    og, ob = buf[4:4 + C], buf[8 + C + 4:8 + 2 * C + 4]  # 16-byte aligned
    b = Hop.bn_bwd(dyg, xg, gamma.cuda(), mean, invstd, y, relu, True,
                   want_dres=want_dres, out_gamma=og, out_beta=ob)
    assert b[1].data_ptr() == og.data_ptr()
    assert b[2].data_ptr() == ob.data_ptr()
    assert torch.equal(_bits(og), _bits(a_dg)), "dgamma differs in the slot"
    assert torch.equal(_bits(ob), _bits(a_db)), "dbeta differs in the slot"
    assert torch.equal(a[0], b[0]), "dx differs under slot delivery"
    if want_dres:
        assert torch.equal(a[3], b[3])
    keep = torch.ones(buf.numel(), dtype=torch.bool)
    keep[4:4 + C] = False
    keep[8 + C + 4:8 + 2 * C + 4] = False
    assert torch.isnan(buf.cpu()[keep]).all(), "slot neighbours were written"

    # fp64 sums from the kernel's own (mean, invstd, y)
    g = dy.double().view(M, C)
    if relu:
        g = g * (y.double().cpu().view(M, C) > 0)
    xhat = (x.double().view(M, C) - mean.double().cpu()) \
        * invstd.double().cpu()
    for got, terms, name in ((og, g * xhat, "dgamma"), (ob, g, "dbeta")):
        ref = terms.sum(0)
        tol = (M + 4) * U * terms.abs().sum(0)
        r = ((got.double().cpu() - ref).abs() / tol.clamp_min(1e-300)).max()
        print(f"{name}: max err/tol = {r.item():.4f}")
        assert r <= 1.0, f"{name}: err/tol {r.item():.3g}"
    if want_dres:
        assert torch.equal(b[3].cpu().view(M, C).double(),
                           g.to(torch.bfloat16).double())


# ------------------------------------------------------------ frozen BN

@pytest.mark.parametrize("C", [16, 64])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("with_res", [False, True])
def test_frozen_bn_apply_only(C, relu, with_res):
    """Teacher BN after cast_compute_weights_: (mean, invstd) precomputed and
    attached to running_mean; one apply launch. Allowance: half a bf16 ulp of
    the result plus 4 fp32 ulps of the pre-rounding magnitude, i.e. of
    |x*sc| + |mean*sc| + |beta| (+ |res|) — the kernel folds BN to
    x*sc + (beta - mean*sc), so those are the terms its fp32 ops round."""
    Hop = _H()
    gen = torch.Generator().manual_seed(200 + C)
    M = 3 * 7 * 7                                   # odd row count
    x = torch.randn(3, 7, 7, C, generator=gen).bfloat16()
    res = torch.randn(3, 7, 7, C, generator=gen).bfloat16() if with_res \
        else None
    gamma = torch.rand(C, generator=gen) + 0.5
    beta = torch.randn(C, generator=gen)
    rm = (torch.randn(C, generator=gen) * 0.3).cuda()
    rv = (torch.rand(C, generator=gen) + 0.5).cuda()
    eps = 1e-5
    # exactly what CilModel.cast_compute_weights_ attaches
    mean = rm.float().clone()
    invstd = torch.rsqrt(rv.float() + eps)
    rm._cilfw_frozen = (mean.contiguous(), invstd.contiguous())
    rm0, rv0 = rm.clone(), rv.clone()
    y, m_out, i_out = Hop.bn_fwd(x.cuda(), gamma.cuda(), beta.cuda(), rm, rv,
                                 0.1, eps, False, relu,
                                 residual=None if res is None else res.cuda())
    assert m_out is rm._cilfw_frozen[0] and i_out is rm._cilfw_frozen[1]
    assert torch.equal(rm, rm0) and torch.equal(rv, rv0)

    x64 = x.double().view(M, C)
    sc = invstd.double().cpu() * gamma.double()
    mu = mean.double().cpu()
    ref = (x64 - mu) * sc + beta.double()
    mag = x64.abs() * sc.abs() + (mu * sc).abs() + beta.double().abs()
    if with_res:
        ref = ref + res.double().view(M, C)
        mag = mag + res.double().view(M, C).abs()
    if relu:
        ref = ref.clamp_min(0)
    tol = O.HALF_ULP_BF16 * ref.abs() + 4 * 2.0 ** -23 * mag
    err = (y.double().cpu().view(M, C) - ref).abs()
    r = (err / tol.clamp_min(1e-300)).max().item()
    print(f"frozen bn: max err/tol = {r:.4f}")
    assert torch.isfinite(y).all() and r <= 1.0, f"err/tol {r:.3g}"


# ----------------------------------------------------------- SGD mirror

@pytest.mark.parametrize("n", [1, 7, 8, 1023, 10007])
def test_sgd_step_mirror_device_lr(n):
    Hop = _H()
    gen = torch.Generator().manual_seed(300 + n)
    lr, mu, wd = 0.05, 0.9, 5e-4
    PAD = 4                                  # one float4 / one bf16x4 vector

    def padded(dtype):
        buf = torch.full((n + 2 * PAD,), 7.0, dtype=dtype)
        return buf

    p, g, m = (torch.randn(n, generator=gen) for _ in range(3))
    bufs = {}
    for name, src in (("p", p), ("g", g), ("m", m)):
        b = padded(torch.float32)
        b[PAD:PAD + n] = src
        bufs[name] = b.cuda()
    bufs["pb"] = padded(torch.bfloat16).cuda()
    view = {k: v[PAD:PAD + n] for k, v in bufs.items()}
    lr_dev = torch.full((1,), lr, dtype=torch.float32, device="cuda")
    Hop.sgd_step(view["p"], view["g"], view["m"], lr_dev, mu, wd,
                 p_bf16=view["pb"])
    torch.cuda.synchronize()

    lr64 = lr_dev.double().item()            # the fp32 value the kernel read
    mu64, wd64 = float(torch.tensor(mu).float()), float(torch.tensor(wd)
                                                        .float())
    p64, g64, m64 = p.double(), g.double(), m.double()
    m_new = mu64 * m64 + (g64 + wd64 * p64)
    p_new = p64 - lr64 * m_new
    tol_m = 4 * U * (mu64 * m64.abs() + g64.abs() + wd64 * p64.abs())
    tol_p = 4 * U * (p64.abs() + lr64 * (mu64 * m64.abs() + g64.abs()
                                         + wd64 * p64.abs()))
    for got, ref, tol, name in ((view["m"], m_new, tol_m, "m"),
                                (view["p"], p_new, tol_p, "p")):
        r = ((got.double().cpu() - ref).abs() / tol).max().item()
        print(f"sgd {name} n={n}: max err/tol = {r:.4f}")
        assert r <= 1.0, f"sgd {name}: err/tol {r:.3g}"
    assert torch.equal(view["pb"].cpu(), view["p"].cpu().to(torch.bfloat16)), \
        "bf16 mirror is not the rounding of the kernel's own fp32 p"
    assert torch.equal(view["g"].cpu(), g), "g was modified"
    for name, b in bufs.items():
        b = b.cpu().float()
        assert (b[:PAD] == 7).all() and (b[PAD + n:] == 7).all(), \
            f"{name}: padding was written"
