"""Margin-ranking HIP kernels (csrc/mrank.hip) against the fp64 oracle of
_mr_ref, sigma / targets / upstream read on the device under graph replay,
the wrapper refusals, and a --gpu_data engine run with --head cosine
--lambda_flat 1 --lambda_mr 1 --imprint (pytest -m gpu). Shapes, inputs and
allowances are those of _mr_ref; no element, row or pair is excluded."""

import contextlib
import io
import math
import re

import pytest
import torch

import _cos_ref as CR
import _mr_ref as R
import _oracle
from cilfw import ops
from cilfw.config import parse_args

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


def _fwd_bwd(ld, td, sd, known, k, margin, scale=1.0):
    lg = ld.clone().requires_grad_(True)
    sg = sd.clone().requires_grad_(True)
    loss = ops.margin_rank_loss(lg, td, sg, known, k, margin)
    (loss * scale).backward()
    return loss.detach(), lg.grad, sg.grad


def _case(name):
    """The oracle and one device forward + backward per shape and upstream,
    computed once and shared (read-only) by the tests."""
    if name not in _CACHE:
        logits, targets, sigma, known, k, margin = R.make_case(name)
        ld, td, sd = logits.to(DEV), targets.to(DEV), sigma.to(DEV)
        c = dict(args=(known, k, margin), ld=ld, td=td, sd=sd, ref={},
                 out={})
        for up in UPS:
            u32 = float(torch.tensor(up, dtype=torch.float32))
            c["ref"][up] = R.mr_ref(logits, targets, sigma, known, k, margin,
                                    up=u32)
            c["out"][up] = _fwd_bwd(ld, td, sd, known, k, margin, up)
        c["sel"] = ops.margin_rank_select(ld, td, sd, known, k, margin)
        torch.cuda.synchronize()
        _CACHE[name] = c
    return _CACHE[name]


@pytest.mark.parametrize("up", UPS)
@pytest.mark.parametrize("name", R.SHAPE_IDS)
def test_against_the_oracle(name, up):
    c = _case(name)
    ref = c["ref"][up]
    loss, dl, ds = c["out"][up]
    M, C = ref["M"], ref["C"]
    assert dl.dtype == BF and dl.shape == (M, C) and ds.shape == (1,)
    assert ds.dtype == torch.float32 and loss.dtype == torch.float32
    rs = dict(loss=R.worst_loss(loss, ref), dlogits=R.worst_dlogits(dl, ref),
              dsigma=R.worst_dsigma(ds, ref))
    print(f"{name} upstream {up}: err/allowance " + " ".join(
        f"{k_} {v:.4f}" for k_, v in rs.items()))
    assert all(v <= 1.0 for v in rs.values()), rs
    assert R.same_sel(c["sel"], ref)
    # exactly 0 wherever the oracle is (the comparator asks it too)
    assert (dl.cpu()[ref["dlogits"] == 0] == 0).all()
    if up != 1.0 and ref["n_active"]:
        # the upstream is not ignored: the result fails the upstream-1 oracle
        ref1 = c["ref"][1.0]
        assert R.worst_dlogits(dl, ref1) > 1.0
        assert R.worst_dsigma(ds, ref1) > 1.0


@pytest.mark.parametrize("name", R.SHAPE_IDS)
def test_out_buffers_are_fully_overwritten(name):
    """NaN-prefilled out= buffers: every element is written, bit-equal to
    the first run."""
    from cilfw import _hip_ops as H
    c = _case(name)
    known, k, margin = c["args"]
    M, C = c["ld"].shape
    first = H.mrank_fwd(c["ld"], c["td"], c["sd"], known, k, margin)
    bufs = dict(sel=_nan(M, k, dtype=torch.int32), fin=_nan(3),
                nold=_nan(1, dtype=torch.int32), rho=_nan(M), dsum=_nan(M),
                old=_nan(M, dtype=torch.int32))
    again = H.mrank_fwd(c["ld"], c["td"], c["sd"], known, k, margin,
                        out=bufs)
    assert again[1] is bufs["sel"] and again[2] is bufs["fin"]
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    assert torch.isfinite(again[2]).all() and torch.isfinite(again[4]).all()
    assert again[3].item() == c["ref"][1.0]["N"]
    assert torch.equal(again[6].bool().cpu(), c["ref"][1.0]["old"])
    assert torch.equal(again[1], c["sel"])
    up = torch.full((1,), UPS[1], device=DEV)
    dl, ds = H.mrank_bwd(first[1], c["td"], first[2], up, C, known)
    dl2, ds2 = H.mrank_bwd(again[1], c["td"], again[2], up, C, known,
                           out=_nan(M, C, dtype=BF), dsig=_nan(1))
    assert torch.equal(dl, dl2) and torch.equal(ds, ds2)
    assert torch.equal(dl, c["out"][UPS[1]][1])
    assert torch.equal(ds, c["out"][UPS[1]][2])
    assert torch.equal(first[0], c["out"][1.0][0])


@pytest.mark.parametrize("name", R.SHAPE_IDS)
def test_two_launches_bit_identical(name):
    c = _case(name)
    known, k, margin = c["args"]
    again = _fwd_bwd(c["ld"], c["td"], c["sd"], known, k, margin, UPS[1])
    assert all(torch.equal(a, b) for a, b in zip(again, c["out"][UPS[1]]))
    assert torch.equal(
        ops.margin_rank_select(c["ld"], c["td"], c["sd"], known, k, margin),
        c["sel"])


def test_tie_goes_to_the_lower_index():
    logits, targets, sigma, known = R.tie_case(BF)
    ld, td, sd = logits.to(DEV), targets.to(DEV), sigma.to(DEV)
    sel1 = ops.margin_rank_select(ld, td, sd, known, 1, 0.5)
    assert sel1.tolist() == [[known + 1], [known + 7]]
    sel2 = ops.margin_rank_select(ld, td, sd, known, 2, 0.5)
    assert sel2.tolist() == [[known + 1, known + 65],
                             [known + 7, known + 3]]
    ref = R.mr_ref(logits, targets, sigma, known, 2, 0.5)
    loss, dl, ds = _fwd_bwd(ld, td, sd, known, 2, 0.5)
    assert R.worst_loss(loss, ref) <= 1.0 and R.worst_dlogits(dl, ref) <= 1.0
    assert R.worst_dsigma(ds, ref) <= 1.0


def test_no_old_row():
    logits, targets, sigma, known, k, margin = R.make_case("ragged")
    td = targets.clamp_min(known).to(DEV)
    loss, dl, ds = _fwd_bwd(logits.to(DEV), td, sigma.to(DEV), known, k,
                            margin)
    assert loss.item() == 0.0 and ds.item() == 0.0 and (dl == 0).all()
    sel = ops.margin_rank_select(logits.to(DEV), td, sigma.to(DEV), known, k,
                                 margin)
    assert (sel == -1).all()


@pytest.mark.parametrize("sg", [0.0, -2.0])
def test_nonpositive_sigma(sg):
    logits, targets, _, known, k, margin = R.make_case("lucir")
    sd = torch.tensor([sg], device=DEV)
    loss, dl, ds = _fwd_bwd(logits.to(DEV), targets.to(DEV), sd, known, k,
                            margin, UPS[1])
    for t in (loss, dl, ds):
        assert torch.isfinite(t.float()).all() and (t == 0).all()


def _head_inputs():
    """Features and weights of _cos_ref's "ragged40" head (70 x 67, D = 40)
    with targets over its 67 classes, 31 of them known."""
    x, w, sigma, _ = CR.make_head("ragged40")
    g = torch.Generator().manual_seed(11)
    targets = torch.randint(0, 67, (70,), generator=g)
    return x, w, sigma, targets, 31, 2, 0.5


def _total_dsigma_ratio(got, cos_ref, mr_ref):
    """|total sigma.grad - (the two oracles' sum)| over the sum of the two
    allowances."""
    n = cos_ref["C"] + CR.MAX_SPLIT + 2.0 * cos_ref["D"] + cos_ref["M"] + 16
    b = _oracle.bound(cos_ref["dsigma"], cos_ref["dsigma_mag"], n, False,
                      extra=CR.E2 * cos_ref["dsigma_mag"]) \
        + R.bound_dsigma(mr_ref)
    err = (got.detach().double().cpu().reshape(1)
           - (cos_ref["dsigma"] + mr_ref["dsigma"])).abs()
    return (err / b).item()


def test_sigma_gradients_cancel_end_to_end():
    """cosine_linear -> margin_rank_loss on the device: the total sigma.grad
    (the head's plus the loss's explicit term, about 0) is within the sum of
    _cos_ref's dsigma allowance and this module's."""
    x, w, sigma, targets, known, k, margin = _head_inputs()
    xd = x.to(DEV).requires_grad_(True)
    wd = w.to(DEV).requires_grad_(True)
    sd = sigma.to(DEV).requires_grad_(True)
    logits = ops.cosine_linear(xd, wd, sd)
    logits.retain_grad()
    loss = ops.margin_rank_loss(logits, targets.to(DEV), sd, known, k, margin)
    loss.backward()
    mref = R.mr_ref(logits.detach(), targets, sigma, known, k, margin)
    assert mref["min_abs_v"] >= R.MIN_ABS_V and mref["n_active"] >= 1
    assert R.worst_loss(loss.detach(), mref) <= 1.0
    assert R.worst_dlogits(logits.grad, mref) <= 1.0
    cref = CR.head_ref(x, w, sigma, logits.grad)
    r = _total_dsigma_ratio(sd.grad, cref, mref)
    print(f"total sigma.grad {sd.grad.item():.3e} (head "
          f"{cref['dsigma'].item():.3e}, loss {mref['dsigma'].item():.3e}): "
          f"err/allowance {r:.4f}")
    assert r <= 1.0
    # the explicit term is not dropped: without it the head's part stands
    assert abs(cref["dsigma"].item()) > 100 * abs(sd.grad.item())


def test_device_reads_under_graph_replay():
    """cosine_linear -> margin_rank_loss forward + backward captured once;
    sigma AND the static targets changed in place between two replays (N
    changes): the second replay matches the new oracle and fails the old."""
    x, w, sigma, targets, known, k, margin = _head_inputs()
    xd = x.to(DEV).requires_grad_(True)
    wd = w.to(DEV).requires_grad_(True)
    sd = sigma.to(DEV).requires_grad_(True)
    td = targets.to(DEV)

    def step():
        logits = ops.cosine_linear(xd, wd, sd)
        loss = ops.margin_rank_loss(logits, td, sd, known, k, margin)
        return (logits, loss) + torch.autograd.grad(loss, (logits, sd))

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
    old = R.mr_ref(out[0], targets, sigma, known, k, margin)
    assert old["min_abs_v"] >= R.MIN_ABS_V and old["n_active"] >= 1
    assert R.worst_loss(out[1], old) <= 1.0
    assert R.worst_dlogits(out[2], old) <= 1.0
    assert _total_dsigma_ratio(
        out[3], CR.head_ref(x, w, sigma, out[2]), old) <= 1.0

    sigma2 = torch.tensor([1.25])
    targets2 = targets.clone()
    targets2[:20] = torch.arange(20) % known        # old rows
    targets2[20:30] = known + torch.arange(10) % 5  # new rows
    with torch.no_grad():
        sd.fill_(1.25)
        td.copy_(targets2)
    graph.replay()
    torch.cuda.synchronize()
    new = R.mr_ref(out[0], targets2, sigma2, known, k, margin)
    assert new["N"] != old["N"]
    assert new["min_abs_v"] >= R.MIN_ABS_V and new["n_active"] >= 1
    rs = dict(loss=R.worst_loss(out[1], new),
              dlogits=R.worst_dlogits(out[2], new),
              dsigma=_total_dsigma_ratio(
                  out[3], CR.head_ref(x, w, sigma2, out[2]), new))
    print(f"after sigma.fill_ and targets.copy_ (N {old['N']} -> "
          f"{new['N']}): err/allowance " + " ".join(
              f"{k_} {v:.4f}" for k_, v in rs.items()))
    assert all(v <= 1.0 for v in rs.values()), rs
    assert R.worst_loss(out[1], old) > 1.0
    assert R.worst_dlogits(out[2], old) > 1.0


def test_wrapper_refusals():
    """Refused by the wrappers before any launch."""
    from cilfw import _hip_ops as H
    logits, targets, sigma, known, k, margin = R.make_case("lucir")
    ld, td, sd = logits.to(DEV), targets.to(DEV), sigma.to(DEV)
    C = ld.shape[1]
    for bad in (0, C):
        with pytest.raises(AssertionError, match="known must be"):
            ops.margin_rank_loss(ld, td, sd, bad, k, margin)
        with pytest.raises(AssertionError, match="known must be"):
            H.mrank_fwd(ld, td, sd, bad, k, margin)
    for bad in (0, 6, 9):
        with pytest.raises(AssertionError, match="k must be"):
            ops.margin_rank_loss(ld, td, sd, known, bad, margin)
        with pytest.raises(AssertionError, match="k must be"):
            H.mrank_fwd(ld, td, sd, known, bad, margin)
    with pytest.raises(AssertionError, match="margin must be"):
        H.mrank_fwd(ld, td, sd, known, k, -1.0)
    with pytest.raises(AssertionError, match="bf16"):
        ops.margin_rank_loss(ld.float(), td, sd, known, k, margin)
    with pytest.raises(AssertionError, match="targets"):
        H.mrank_fwd(ld, td.int(), sd, known, k, margin)
    with pytest.raises(AssertionError, match="DEVICE tensor"):
        H.mrank_fwd(ld, td, sigma, known, k, margin)
    with pytest.raises(AssertionError, match="fp32"):
        ops.margin_rank_loss(ld, td, sd.double(), known, k, margin)
    with pytest.raises(AssertionError, match="out buffer"):
        H.mrank_fwd(ld, td, sd, known, k, margin,
                    out=dict(sel=torch.empty(5, 3, dtype=torch.int32,
                                             device=DEV)))
    sel, fin = H.mrank_fwd(ld, td, sd, known, k, margin)[1:3]
    with pytest.raises(AssertionError, match="out buffer"):
        H.mrank_bwd(sel, td, fin, torch.ones(1, device=DEV), C, known,
                    out=torch.empty(5, C, device=DEV))
    with pytest.raises(AssertionError, match="DEVICE tensor"):
        H.mrank_bwd(sel, td, fin, torch.ones(1), C, known)
    lib = H._lib
    assert lib.cilfw_mrank_supported(5, 10, 5, 2) == 1
    assert lib.cilfw_mrank_supported(1, 2, 1, 1) == 1
    assert lib.cilfw_mrank_supported(7, 1100, 100, 8) == 1
    assert lib.cilfw_mrank_supported(0, 10, 5, 2) == 0
    assert lib.cilfw_mrank_supported(5, 1, 1, 1) == 0
    assert lib.cilfw_mrank_supported(5, 10, 0, 2) == 0
    assert lib.cilfw_mrank_supported(5, 10, 10, 1) == 0
    assert lib.cilfw_mrank_supported(5, 10, 5, 0) == 0
    assert lib.cilfw_mrank_supported(5, 10, 5, 6) == 0
    assert lib.cilfw_mrank_supported(5, 100, 5, 9) == 0


def _engine_run():
    from cilfw.engine import run
    args = parse_args([
        "--data_set", "synthetic", "--backbone", "resnet20",
        "--synthetic_classes", "10", "--num_bases", "5", "--increment", "5",
        "--num_epochs", "1", "--batch_size", "32", "--workers", "0",
        "--synthetic_train_size", "640", "--memory_size", "40",
        "--eval_every_epoch", "0", "--input_size", "32", "--no_aug",
        "--lr", "0.05", "--seed", "3", "--dtype", "bf16", "--gpu_data",
        "--head", "cosine", "--lambda_flat", "1", "--lambda_mr", "1",
        "--imprint"])
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        accs = run(args)
    return accs, out.getvalue()


def test_engine_lucir_captures_and_repeats():
    """--gpu_data --head cosine --lambda_flat 1 --lambda_mr 1 --imprint: the
    run completes with the margin term inside the captured step graph, the
    mr meter is finite on task 1 only, the imprint line appears on task 1
    only, and a second identical run repeats it bit for bit."""
    accs, out = _engine_run()
    assert len(accs) == 2
    assert "capture failed" not in out
    t0 = re.findall(r"^task 0 epoch \d+: .*$", out, re.M)
    t1 = re.findall(r"^task 1 epoch \d+: .*$", out, re.M)
    assert len(t0) == 1 and len(t1) == 1 and "mr:" not in t0[0]
    m = re.search(r"  mr: (\S+) \((\S+)\)", t1[0])
    assert m, t1[0]
    assert all(math.isfinite(float(v)) and float(v) >= 0.0
               for v in m.groups())
    assert "  flat: " in t1[0]
    imp = re.findall(r"^imprint: .*$", out, re.M)
    assert len(imp) == 1 and "task 1: 5 new head rows" in imp[0]
    accs2, out2 = _engine_run()
    assert accs2 == accs
    assert re.findall(r"^imprint: .*$", out2, re.M) == imp

    def meters(line):
        return re.sub(r"imgs/s \d+", "", line)
    for task in (0, 1):
        a = re.findall(rf"^task {task} epoch \d+: .*$", out, re.M)
        b = re.findall(rf"^task {task} epoch \d+: .*$", out2, re.M)
        assert [meters(v) for v in a] == [meters(v) for v in b]
