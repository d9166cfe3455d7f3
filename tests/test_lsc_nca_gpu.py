"""LSC / NCA HIP kernels (csrc/lsc.hip) against the fp64 oracle of _lsc_ref,
sigma / targets / upstream read on the device under graph replay, the wrapper
refusals, and a --gpu_data engine run with the PODNet flag set (pytest -m
gpu). Shapes, inputs and allowances are those of _lsc_ref; no element or row
is excluded."""

import contextlib
import io
import math
import re

import pytest
import torch

import _cos_ref as CR
import _lsc_ref as R
from cilfw import ops
from cilfw.config import parse_args
from cilfw.ops import lsc as L  # noqa: F401  (the feature under test)

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(),
                                 reason="needs GPU")]

DEV = "cuda:0"
BF = torch.bfloat16
UPS = [1.0, 0.37]
_CACHE = {}


def _nan(*shape, dtype=torch.float32):
    if dtype == torch.int32:
        return torch.full(shape, -12345, dtype=dtype, device=DEV)
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


# ------------------------------------------------------------------ lsc_reduce

def _lsc_fwd_bwd(xd, sd, K, gamma, gd):
    x = xd.clone().requires_grad_(True)
    s = sd.clone().requires_grad_(True)
    out = ops.lsc_reduce(x, s, K, gamma)
    out.backward(gd)
    return out.detach(), x.grad, s.grad


def _lsc_case(name, gamma):
    """The oracle and one device forward + backward per shape and gamma,
    computed once and shared (read-only) by the tests."""
    key = ("lsc", name, gamma)
    if key not in _CACHE:
        sims, sigma, K, g = R.make_lsc(name)
        xd, sd, gd = sims.to(DEV), sigma.to(DEV), g.to(DEV)
        c = dict(K=K, xd=xd, sd=sd, gd=gd,
                 ref=R.lsc_ref(sims, sigma, K, gamma, g),
                 out=_lsc_fwd_bwd(xd, sd, K, gamma, gd))
        torch.cuda.synchronize()
        _CACHE[key] = c
    return _CACHE[key]


def _lsc_check(c, what):
    ref = c["ref"]
    out, dx, ds = c["out"]
    M, C, K = ref["M"], ref["C"], ref["K"]
    assert out.dtype == BF and out.shape == (M, C)
    assert dx.dtype == BF and dx.shape == (M, C * K)
    assert ds.dtype == torch.float32 and ds.shape == (1,)
    rs = dict(logits=R.worst_logits(out, ref), dsims=R.worst_dsims(dx, ref),
              dsigma=R.worst_lsc_dsigma(ds, ref))
    print(f"{what}: err/allowance " + " ".join(
        f"{k} {v:.4f}" for k, v in rs.items()))
    assert all(v <= 1.0 for v in rs.values()), rs


@pytest.mark.parametrize("gamma", R.GAMMAS)
@pytest.mark.parametrize("name", R.LSC_IDS)
def test_lsc_against_the_oracle(name, gamma):
    c = _lsc_case(name, gamma)
    _lsc_check(c, f"lsc {name} gamma {gamma}")
    # the upstream is not ignored
    sims, sigma, K, g = R.make_lsc(name)
    assert R.worst_dsims(c["out"][1],
                         R.lsc_ref(sims, sigma, K, gamma, -g)) > 1.0
    if K > 1:  # nor is gamma
        other = R.GAMMAS[1 - R.GAMMAS.index(gamma)]
        assert R.worst_logits(c["out"][0],
                              R.lsc_ref(sims, sigma, K, other, g)) > 1.0


def test_lsc_gamma_zero():
    _lsc_check(_lsc_case("podnet", 0.0), "lsc podnet gamma 0")


def test_lsc_one_proxy_is_sigma_times_sims():
    sims, sigma, _, _ = R.make_lsc("odd")
    xd, sd = sims.to(DEV), sigma.to(DEV)
    want = (sigma * sims.float()).to(BF)
    for gamma in (0.0, 4.0):
        assert torch.equal(ops.lsc_reduce(xd, sd, 1, gamma).cpu(), want)


@pytest.mark.parametrize("name", R.LSC_IDS)
def test_lsc_out_buffers_and_repeat(name):
    """NaN-prefilled out= buffers: every element is written, bit-equal to
    the first run; two launches are bit-identical."""
    from cilfw import _hip_ops as H
    gamma = R.GAMMAS[1]
    c = _lsc_case(name, gamma)
    K, xd, sd, gd = c["K"], c["xd"], c["sd"], c["gd"]
    M, CK = xd.shape
    C = CK // K
    first = H.lsc_reduce_fwd(xd, sd, K, gamma)
    again = H.lsc_reduce_fwd(xd, sd, K, gamma, out=_nan(M, C, dtype=BF),
                             yhat=_nan(M, C))
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    assert torch.equal(first[0], c["out"][0])
    assert torch.isfinite(again[1]).all()
    assert R.worst_yhat(again[1], c["ref"]) <= 1.0
    b1 = H.lsc_reduce_bwd(xd, first[1], gd, sd, K, gamma)
    b2 = H.lsc_reduce_bwd(xd, again[1], gd, sd, K, gamma,
                          out=_nan(M, CK, dtype=BF), rows=_nan(M))
    assert all(torch.equal(a, b) for a, b in zip(b1, b2))
    assert torch.equal(b1[0], c["out"][1])
    assert torch.equal(H.cos_sum(b2[1]), c["out"][2])
    rerun = _lsc_fwd_bwd(xd, sd, K, gamma, gd)
    assert all(torch.equal(a, b) for a, b in zip(rerun, c["out"]))


# -------------------------------------------------------------------- nca_loss

def _nca_fwd_bwd(ld, td, sd, margin, scale=1.0):
    lg = ld.clone().requires_grad_(True)
    sg = sd.clone().requires_grad_(True)
    loss = ops.nca_loss(lg, td, sg, margin)
    (loss * scale).backward()
    return loss.detach(), lg.grad, sg.grad


def _nca_case(name, invalid=False):
    key = ("nca", name, invalid)
    if key not in _CACHE:
        logits, targets, sigma, margin = R.make_nca(name)
        if invalid:
            targets = R.with_invalid_targets(targets, logits.shape[1])
        ld, td, sd = logits.to(DEV), targets.to(DEV), sigma.to(DEV)
        c = dict(margin=margin, ld=ld, td=td, sd=sd, ref={}, out={})
        for up in UPS:
            u32 = float(torch.tensor(up, dtype=torch.float32))
            c["ref"][up] = R.nca_ref(logits, targets, sigma, margin, up=u32)
            c["out"][up] = _nca_fwd_bwd(ld, td, sd, margin, up)
        c["rows"] = ops.nca_rows(ld, td, sd, margin)
        torch.cuda.synchronize()
        _CACHE[key] = c
    return _CACHE[key]


def _nca_check(c, up, what):
    ref = c["ref"][up]
    loss, dl, ds = c["out"][up]
    h, active = c["rows"]
    M, C = ref["M"], ref["C"]
    assert dl.dtype == BF and dl.shape == (M, C) and ds.shape == (1,)
    assert ds.dtype == torch.float32 and loss.dtype == torch.float32
    assert h.dtype == torch.float32 and h.shape == (M,)
    rs = dict(loss=R.worst_loss(loss, ref), h=R.worst_h(h, ref),
              dlogits=R.worst_dlogits(dl, ref),
              dsigma=R.worst_nca_dsigma(ds, ref))
    print(f"{what} upstream {up}: err/allowance " + " ".join(
        f"{k} {v:.4f}" for k, v in rs.items()))
    assert all(v <= 1.0 for v in rs.values()), rs
    assert R.same_active(active, ref)
    # exactly 0 wherever the oracle is (the comparator asks it too)
    assert (dl.cpu()[ref["dlogits"] == 0] == 0).all()
    if up != 1.0 and ref["n_active"]:
        # the upstream is not ignored: the result fails the upstream-1 oracle
        ref1 = c["ref"][1.0]
        assert R.worst_dlogits(dl, ref1) > 1.0
        assert R.worst_nca_dsigma(ds, ref1) > 1.0


@pytest.mark.parametrize("up", UPS)
@pytest.mark.parametrize("name", R.NCA_IDS)
def test_nca_against_the_oracle(name, up):
    _nca_check(_nca_case(name), up, f"nca {name}")


@pytest.mark.parametrize("up", UPS)
def test_nca_invalid_targets_give_zero_rows(up):
    c = _nca_case("ragged", invalid=True)
    ref = c["ref"][up]
    assert not ref["valid"][0] and not ref["valid"][2]
    _nca_check(c, up, "nca ragged, rows 0 and 2 skipped")
    dl = c["out"][up][1]
    assert (dl[0] == 0).all() and (dl[2] == 0).all()
    h, active = c["rows"]
    assert h[0] == 0 and h[2] == 0 and active[0] == 0 and active[2] == 0


def test_nca_every_row_skipped():
    logits, targets, sigma, margin = R.make_nca("small")
    bad = torch.full_like(targets, -3).to(DEV)
    loss, dl, ds = _nca_fwd_bwd(logits.to(DEV), bad, sigma.to(DEV), margin)
    assert loss.item() == 0.0 and ds.item() == 0.0 and (dl == 0).all()


@pytest.mark.parametrize("sg", [0.0, -2.0])
def test_nonpositive_sigma_is_finite(sg):
    logits, targets, _, margin = R.make_nca("small")
    sigma = torch.tensor([sg])
    out = _nca_fwd_bwd(logits.to(DEV), targets.to(DEV), sigma.to(DEV),
                       margin, UPS[1])
    assert all(torch.isfinite(t.float()).all() for t in out)
    ref = R.nca_ref(logits, targets, sigma, margin,
                    up=float(torch.tensor(UPS[1])))
    assert R.worst_loss(out[0], ref) <= 1.0
    assert R.worst_dlogits(out[1], ref) <= 1.0
    assert R.worst_nca_dsigma(out[2], ref) <= 1.0
    sims, _, K, g = R.make_lsc("podnet")
    res = _lsc_fwd_bwd(sims.to(DEV), sigma.to(DEV), K, 1.0, g.to(DEV))
    assert all(torch.isfinite(t.float()).all() for t in res)
    lref = R.lsc_ref(sims, sigma, K, 1.0, g)
    assert R.worst_logits(res[0], lref) <= 1.0
    assert R.worst_dsims(res[1], lref) <= 1.0
    assert R.worst_lsc_dsigma(res[2], lref) <= 1.0


@pytest.mark.parametrize("name", R.NCA_IDS)
def test_nca_out_buffers_and_repeat(name):
    """NaN-prefilled out= buffers: every element is written, bit-equal to
    the first run; two launches are bit-identical."""
    from cilfw import _hip_ops as H
    c = _nca_case(name)
    ld, td, sd, margin = c["ld"], c["td"], c["sd"], c["margin"]
    M, C = ld.shape
    first = H.nca_fwd(ld, td, sd, margin)
    bufs = dict(h=_nan(M), lse=_nan(M), active=_nan(M, dtype=torch.int32),
                fin=_nan(3), nact=_nan(1, dtype=torch.int32))
    again = H.nca_fwd(ld, td, sd, margin, out=bufs)
    assert again[1] is bufs["h"] and again[4] is bufs["fin"]
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    assert all(torch.isfinite(again[i]).all() for i in (1, 3, 4))
    assert again[5].item() == c["ref"][1.0]["A"]
    assert torch.equal(again[1], c["rows"][0])
    assert torch.equal(again[2], c["rows"][1])
    assert torch.equal(first[0], c["out"][1.0][0])
    up = torch.full((1,), UPS[1], device=DEV)
    dl, ds = H.nca_bwd(ld, td, first[3], first[2], first[4], up)
    dl2, ds2 = H.nca_bwd(ld, td, again[3], again[2], again[4], up,
                         out=_nan(M, C, dtype=BF), dsig=_nan(1))
    assert torch.equal(dl, dl2) and torch.equal(ds, ds2)
    assert torch.equal(dl, c["out"][UPS[1]][1])
    assert torch.equal(ds, c["out"][UPS[1]][2])
    rerun = _nca_fwd_bwd(ld, td, sd, margin, UPS[1])
    assert all(torch.equal(a, b) for a, b in zip(rerun, c["out"][UPS[1]]))


# ------------------------------------------------------------- graph / wrappers

def _head_inputs():
    """Features of _cos_ref's "ragged40" head (70 rows, D = 40) against 67
    classes x 3 proxies, targets over the 67 classes."""
    x, _, _, _ = CR.make_head("ragged40")
    g = torch.Generator().manual_seed(13)
    w = torch.randn(67 * 3, 40, generator=g)
    targets = torch.randint(0, 67, (70,), generator=g)
    return x, w, targets, 3, 2.0, 0.6


def _chain_ratios(out, targets, sigma, K, gamma, margin):
    """(sims, logits, loss, dlogits, dsims, dsigma) of one replay against
    the oracles taken from the device's own intermediate tensors; dsigma is
    the total sigma.grad, the reduce's plus the loss's explicit term."""
    sims, logits, loss, dlogits, dsims, dsg = out
    lref = R.lsc_ref(sims, sigma, K, gamma, dlogits)
    nref = R.nca_ref(logits, targets, sigma, margin)
    return dict(logits=R.worst_logits(logits, lref),
                dsims=R.worst_dsims(dsims, lref),
                loss=R.worst_loss(loss, nref),
                dlogits=R.worst_dlogits(dlogits, nref),
                dsigma=R.worst_total_dsigma(dsg, lref, nref)), nref, lref


def test_device_reads_under_graph_replay():
    """cosine_linear -> lsc_reduce -> nca_loss forward + backward captured
    once; sigma AND the static targets changed in place between two replays:
    the second replay matches the new oracle and fails the old."""
    x, w, targets, K, gamma, margin = _head_inputs()
    sigma = torch.tensor([8.0])
    xd = x.to(DEV).requires_grad_(True)
    wd = w.to(DEV).requires_grad_(True)
    sd = sigma.to(DEV).requires_grad_(True)
    one = torch.ones(1, device=DEV)
    td = targets.to(DEV)

    def step():
        sims = ops.cosine_linear(xd, wd, one)
        logits = ops.lsc_reduce(sims, sd, K, gamma)
        loss = ops.nca_loss(logits, td, sd, margin)
        dlogits, dsims, dsg = torch.autograd.grad(loss, (logits, sims, sd))
        return sims, logits, loss, dlogits, dsims, dsg

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    graph.replay()
    torch.cuda.synchronize()
    rs, old, old_l = _chain_ratios(out, targets, sigma, K, gamma, margin)
    print("first replay: err/allowance " + " ".join(
        f"{k} {v:.4f}" for k, v in rs.items()))
    assert old["min_abs_h"] >= R.MIN_ABS_H and old["n_active"] >= 1
    assert all(v <= 1.0 for v in rs.values()), rs
    old_logits, old_loss = out[1].clone(), out[2].clone()
    old_dl, old_dsg = out[3].clone(), out[5].clone()

    sigma2 = torch.tensor([5.25])
    targets2 = (targets + 1 + torch.arange(70) % 5) % 67
    with torch.no_grad():
        sd.fill_(5.25)
        td.copy_(targets2)
    graph.replay()
    torch.cuda.synchronize()
    rs, new, _ = _chain_ratios(out, targets2, sigma2, K, gamma, margin)
    print(f"after sigma.fill_ and targets.copy_ (A {old['A']} -> "
          f"{new['A']}): err/allowance " + " ".join(
              f"{k} {v:.4f}" for k, v in rs.items()))
    assert new["min_abs_h"] >= R.MIN_ABS_H and new["n_active"] >= 1
    assert all(v <= 1.0 for v in rs.values()), rs
    # and fails the old: the first replay's results are not repeated
    lref_old = R.lsc_ref(out[0], sigma, K, gamma, out[3])
    assert R.worst_logits(out[1], lref_old) > 1.0
    assert R.worst_loss(out[2], old) > 1.0
    assert R.worst_dlogits(out[3], old) > 1.0
    assert R.worst_total_dsigma(out[5], old_l, old) > 1.0
    assert not torch.equal(out[1], old_logits)
    assert not torch.equal(out[2], old_loss)
    assert not torch.equal(out[3], old_dl)
    assert not torch.equal(out[5], old_dsg)


def test_wrapper_refusals():
    """Refused by the wrappers before any launch."""
    from cilfw import _hip_ops as H
    sims, sigma, K, g = R.make_lsc("podnet")
    xd, sd, gd = sims.to(DEV), sigma.to(DEV), g.to(DEV)
    M, C = g.shape
    for bad in (0, 17):
        with pytest.raises(AssertionError, match="nb_proxy must be"):
            ops.lsc_reduce(xd, sd, bad, 1.0)
        with pytest.raises(AssertionError, match="nb_proxy must be"):
            H.lsc_reduce_fwd(xd, sd, bad, 1.0)
    with pytest.raises(AssertionError, match="multiple of nb_proxy"):
        H.lsc_reduce_fwd(xd, sd, 7, 1.0)
    with pytest.raises(AssertionError, match="gamma must be"):
        H.lsc_reduce_fwd(xd, sd, K, -1.0)
    with pytest.raises(AssertionError, match="bf16"):
        ops.lsc_reduce(xd.float(), sd, K, 1.0)
    with pytest.raises(AssertionError, match="host tensor"):
        H.lsc_reduce_fwd(sims, sd, K, 1.0)
    with pytest.raises(AssertionError, match="DEVICE tensor"):
        H.lsc_reduce_fwd(xd, sigma, K, 1.0)
    with pytest.raises(AssertionError, match="fp32"):
        ops.lsc_reduce(xd, sd.double(), K, 1.0)
    with pytest.raises(AssertionError, match="out buffer"):
        H.lsc_reduce_fwd(xd, sd, K, 1.0,
                         out=torch.empty(M, C + 1, dtype=BF, device=DEV))
    with pytest.raises(AssertionError, match="out buffer"):
        H.lsc_reduce_fwd(xd, sd, K, 1.0, yhat=torch.empty(M, C, device="cpu"))
    _, yhat = H.lsc_reduce_fwd(xd, sd, K, 1.0)
    with pytest.raises(AssertionError, match="upstream"):
        H.lsc_reduce_bwd(xd, yhat, gd[:, :3].contiguous(), sd, K, 1.0)
    with pytest.raises(AssertionError, match="bf16"):
        H.lsc_reduce_bwd(xd, yhat, gd.float(), sd, K, 1.0)
    with pytest.raises(AssertionError, match="out buffer"):
        H.lsc_reduce_bwd(xd, yhat, gd, sd, K, 1.0,
                         out=torch.empty(M, C, dtype=BF, device=DEV))

    logits, targets, sigma, margin = R.make_nca("small")
    ld, td, sd = logits.to(DEV), targets.to(DEV), sigma.to(DEV)
    M, C = ld.shape
    with pytest.raises(AssertionError, match="C >= 2"):
        ops.nca_loss(ld[:, :1].contiguous(), td, sd, margin)
    with pytest.raises(AssertionError, match="C >= 2"):
        H.nca_fwd(ld[:, :1].contiguous(), td, sd, margin)
    with pytest.raises(AssertionError, match="margin must be"):
        H.nca_fwd(ld, td, sd, -1.0)
    with pytest.raises(AssertionError, match="bf16"):
        ops.nca_loss(ld.float(), td, sd, margin)
    with pytest.raises(AssertionError, match="targets"):
        H.nca_fwd(ld, td.int(), sd, margin)
    with pytest.raises(AssertionError, match="targets"):
        H.nca_fwd(ld, targets, sd, margin)
    with pytest.raises(AssertionError, match="host tensor"):
        H.nca_fwd(logits, td, sd, margin)
    with pytest.raises(AssertionError, match="DEVICE tensor"):
        H.nca_fwd(ld, td, sigma, margin)
    with pytest.raises(AssertionError, match="fp32"):
        ops.nca_loss(ld, td, sd.double(), margin)
    with pytest.raises(AssertionError, match="out buffer"):
        H.nca_fwd(ld, td, sd, margin,
                  out=dict(h=torch.empty(M + 1, device=DEV)))
    _, _, active, lse, fin, _ = H.nca_fwd(ld, td, sd, margin)
    with pytest.raises(AssertionError, match="out buffer"):
        H.nca_bwd(ld, td, lse, active, fin, torch.ones(1, device=DEV),
                  out=torch.empty(M, C, device=DEV))
    with pytest.raises(AssertionError, match="DEVICE tensor"):
        H.nca_bwd(ld, td, lse, active, fin, torch.ones(1))
    lib = H._lib
    assert lib.cilfw_lsc_supported(1, 1, 1) == 1
    assert lib.cilfw_lsc_supported(5, 10, 10) == 1
    assert lib.cilfw_lsc_supported(9, 5, 16) == 1
    assert lib.cilfw_lsc_supported(7, 1100, 2) == 1
    assert lib.cilfw_lsc_supported(0, 10, 10) == 0
    assert lib.cilfw_lsc_supported(5, 0, 10) == 0
    assert lib.cilfw_lsc_supported(5, 10, 0) == 0
    assert lib.cilfw_lsc_supported(5, 10, 17) == 0
    assert lib.cilfw_lsc_supported(5, 2 ** 28, 16) == 0
    assert lib.cilfw_nca_supported(1, 2) == 1
    assert lib.cilfw_nca_supported(7, 1100) == 1
    assert lib.cilfw_nca_supported(0, 10) == 0
    assert lib.cilfw_nca_supported(5, 1) == 0


# ---------------------------------------------------------------------- engine

def _engine_run():
    from cilfw.engine import run
    args = parse_args([
        "--data_set", "synthetic", "--backbone", "resnet20",
        "--synthetic_classes", "10", "--num_bases", "5", "--increment", "5",
        "--num_epochs", "1", "--batch_size", "32", "--workers", "0",
        "--synthetic_train_size", "640", "--memory_size", "40",
        "--eval_every_epoch", "0", "--input_size", "32", "--no_aug",
        "--lr", "0.05", "--seed", "3", "--dtype", "bf16", "--gpu_data",
        "--head", "cosine", "--nb_proxy", "3", "--cls_loss", "nca",
        "--lambda_kd", "0", "--lambda_pod", "3", "--lambda_flat", "1"])
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        accs = run(args)
    return accs, out.getvalue()


def test_engine_podnet_captures_and_repeats():
    """--gpu_data with the PODNet flag set: the run completes with the
    reduce and the NCA term inside the captured step graph, the nca meter is
    finite, no ce / kd meter appears, and a second identical run repeats the
    meters bit for bit."""
    accs, out = _engine_run()
    assert len(accs) == 2
    assert "capture failed" not in out
    lines = re.findall(r"^task \d+ epoch \d+: .*$", out, re.M)
    assert len(lines) == 2
    for line in lines:
        m = re.search(r"  nca: (\S+) \((\S+)\)", line)
        assert m, line
        assert all(math.isfinite(float(v)) and float(v) >= 0.0
                   for v in m.groups())
        assert "ce:" not in line and "kd:" not in line
    assert "  pod: " in lines[1] and "  flat: " in lines[1]
    accs2, out2 = _engine_run()
    assert accs2 == accs

    def meters(line):
        return re.sub(r"imgs/s \d+", "", line)
    lines2 = re.findall(r"^task \d+ epoch \d+: .*$", out2, re.M)
    assert [meters(v) for v in lines] == [meters(v) for v in lines2]
