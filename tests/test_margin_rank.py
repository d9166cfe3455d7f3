"""LUCIR's margin-ranking loss on the CPU: the torch path of ops/margin.py
against the fp64 oracle of _mr_ref (whose fixtures are checked here too), the
tie rule, the degenerate cases, sigma-invariance through cosine_linear, the
argument refusals, the CLI flags and the engine wiring with --imprint."""

import contextlib
import io
import math
import re

import pytest
import torch

import _mr_ref as R
from cilfw import ops
from cilfw.config import parse_args
from cilfw.engine import run
from cilfw.models import CilModel


def _fwd_bwd(logits, targets, sigma, known, k, margin, scale=1.0):
    lg = logits.clone().requires_grad_(True)
    sg = sigma.clone().requires_grad_(True)
    loss = ops.margin_rank_loss(lg, targets, sg, known, k, margin)
    (loss * scale).backward()
    sel = ops.margin_rank_select(lg.detach(), targets, sg.detach(), known, k,
                                 margin)
    return loss.detach(), lg.grad, sg.grad, sel


# --------------------------------------------------------------- the fixtures

@pytest.mark.parametrize("name", R.SHAPE_IDS)
def test_fixture_conditions(name):
    """Asserted here so that a failure cannot hide: every non-degenerate
    shape has an active and an inactive pair, old and new rows, and every
    pair of every old row has |v_j| >= 1e-4 in the oracle."""
    logits, targets, sigma, known, k, margin = R.make_case(name)
    assert logits.dtype == torch.bfloat16
    assert tuple(logits.shape) == R.SHAPES[name][:2]
    ref = R.mr_ref(logits, targets, sigma, known, k, margin)
    print(f"{name}: N {ref['N']} active {ref['n_active']} inactive "
          f"{ref['n_inactive']} partial rows {ref['n_partial']} min|v| "
          f"{ref['min_abs_v']:.3e}")
    assert ref["min_abs_v"] >= R.MIN_ABS_V
    assert ref["N"] >= 1
    if name != "degenerate":
        assert ref["n_active"] >= 1 and ref["n_inactive"] >= 1
        assert 1 <= ref["N"] < ref["M"]  # targets mix old and new rows


# ------------------------------------------------------- torch path vs oracle

@pytest.mark.parametrize("name", R.SHAPE_IDS)
def test_cpu_fp32_within_allowances(name):
    logits, targets, sigma, known, k, margin = R.make_case(name)
    ref = R.mr_ref(logits, targets, sigma, known, k, margin)
    loss, dl, ds, sel = _fwd_bwd(logits.float(), targets, sigma, known, k,
                                 margin)
    assert dl.dtype == torch.float32 and ds.shape == (1,)
    rs = dict(loss=R.worst_loss(loss, ref), dlogits=R.worst_dlogits(dl, ref),
              dsigma=R.worst_dsigma(ds, ref))
    print(f"{name}: err/allowance " + " ".join(
        f"{k_} {v:.4f}" for k_, v in rs.items()))
    assert all(v <= 1.0 for v in rs.values()), rs
    assert R.same_sel(sel, ref)
    # upstream 0.37 is honoured and fails the upstream-1 oracle
    up = float(torch.tensor(0.37, dtype=torch.float32))
    _, dl37, ds37, _ = _fwd_bwd(logits.float(), targets, sigma, known, k,
                                margin, scale=0.37)
    ref37 = R.mr_ref(logits, targets, sigma, known, k, margin, up=up)
    assert R.worst_dlogits(dl37, ref37) <= 1.0
    assert R.worst_dsigma(ds37, ref37) <= 1.0
    if ref["n_active"]:
        assert R.worst_dlogits(dl37, ref) > 1.0
        assert R.worst_dsigma(ds37, ref) > 1.0


@pytest.mark.parametrize("name", R.SHAPE_IDS)
def test_cpu_fp64_to_1e12(name):
    logits, targets, sigma, known, k, margin = R.make_case(name)
    ref = R.mr_ref(logits, targets, sigma, known, k, margin)
    # fp64 input: sigma margin is an fp64 product, the oracle's an fp32 one;
    # margin 0.5 makes both exact
    assert margin == 0.5
    loss, dl, ds, sel = _fwd_bwd(logits.double(), targets, sigma.double(),
                                 known, k, margin)
    assert loss.dtype == torch.float64 and dl.dtype == torch.float64
    assert ds.dtype == torch.float64
    assert abs(loss.item() - ref["loss"].item()) <= 1e-12
    assert (dl - ref["dlogits"]).abs().max().item() <= 1e-12
    assert abs(ds.item() - ref["dsigma"].item()) <= 1e-12
    assert R.same_sel(sel, ref)


def test_gradcheck():
    logits, targets, sigma, known, k, margin = R.make_case("lucir")
    lg = logits.double().requires_grad_(True)
    sg = sigma.double().requires_grad_(True)
    assert torch.autograd.gradcheck(
        lambda a, b: ops.margin_rank_loss(a, targets, b, known, k, margin),
        (lg, sg))


# ------------------------------------------------------------- special cases

def test_tie_goes_to_the_lower_index():
    logits, targets, sigma, known = R.tie_case()
    sel1 = ops.margin_rank_select(logits, targets, sigma, known, 1, 0.5)
    assert sel1.tolist() == [[known + 1], [known + 7]]
    sel2 = ops.margin_rank_select(logits, targets, sigma, known, 2, 0.5)
    assert sel2.tolist() == [[known + 1, known + 65],
                             [known + 7, known + 3]]
    ref = R.mr_ref(logits, targets, sigma, known, 2, 0.5)
    assert R.same_sel(sel2, ref)


def test_no_old_row():
    logits, targets, sigma, known, k, margin = R.make_case("lucir")
    targets = targets.clamp_min(known)
    loss, dl, ds, sel = _fwd_bwd(logits.float(), targets, sigma, known, k,
                                 margin)
    assert loss.item() == 0.0 and (dl == 0).all() and ds.item() == 0.0
    assert (sel == -1).all()


@pytest.mark.parametrize("sg", [0.0, -2.0])
def test_nonpositive_sigma(sg):
    logits, targets, _, known, k, margin = R.make_case("lucir")
    sigma = torch.tensor([sg], dtype=torch.float32)
    loss, dl, ds, _ = _fwd_bwd(logits.float(), targets, sigma, known, k,
                               margin)
    for t in (loss, dl, ds):
        assert torch.isfinite(t).all() and (t == 0).all()


def test_sigma_invariance_through_the_head():
    """The loss is a function of the cosines alone: through cosine_linear ->
    margin_rank_loss the loss does not depend on sigma and the two paths to
    sigma cancel."""
    g = torch.Generator().manual_seed(5)
    x = torch.randn(12, 16, generator=g, dtype=torch.float64).abs() + 0.1
    w = torch.randn(9, 16, generator=g, dtype=torch.float64)
    targets = torch.arange(12) % 9
    losses = []
    for sg in (1.0, 3.7):
        sigma = torch.tensor([sg], dtype=torch.float64, requires_grad=True)
        logits = ops.cosine_linear(x, w, sigma)
        loss = ops.margin_rank_loss(logits, targets, sigma, 5, 2, 0.5)
        loss.backward()
        assert loss.item() > 0
        assert abs(sigma.grad.item()) <= 1e-12
        losses.append(loss.item())
    assert abs(losses[0] - losses[1]) <= 1e-12


def test_argument_refusals():
    logits, targets, sigma, known, k, margin = R.make_case("lucir")
    lg = logits.float()
    C = lg.shape[1]
    for bad in (0, C, -1):
        with pytest.raises(AssertionError, match="known must be"):
            ops.margin_rank_loss(lg, targets, sigma, bad, k, margin)
    for bad in (0, 6, 9):  # C - known = 5
        with pytest.raises(AssertionError, match="k must be"):
            ops.margin_rank_loss(lg, targets, sigma, known, bad, margin)
    with pytest.raises(AssertionError, match="margin must be"):
        ops.margin_rank_loss(lg, targets, sigma, known, k, -0.1)
    with pytest.raises(AssertionError, match="targets"):
        ops.margin_rank_loss(lg, targets[:3], sigma, known, k, margin)
    with pytest.raises(AssertionError, match="fp32 or fp64"):
        ops.margin_rank_loss(logits, targets, sigma, known, k, margin)
    wide = torch.zeros(2, 30)
    with pytest.raises(AssertionError, match="k must be"):
        ops.margin_rank_loss(wide, targets[:2], sigma, 10, 9, margin)


# ------------------------------------------------------------ flags / engine

def test_cli_flags(capsys):
    a = parse_args([])
    assert a.lambda_mr == 0.0 and a.mr_k == 2 and a.mr_margin == 0.5
    assert a.imprint is False
    a = parse_args(["--head", "cosine", "--lambda_mr", "1", "--mr_k", "3",
                    "--mr_margin", "0.25", "--imprint"])
    assert a.lambda_mr == 1.0 and a.mr_k == 3 and a.mr_margin == 0.25
    assert a.imprint is True
    with pytest.raises(SystemExit):
        parse_args(["--lambda_mr", "1"])
    err = capsys.readouterr().err
    assert "--lambda_mr" in err and "--head cosine" in err
    with pytest.raises(SystemExit):
        parse_args(["--imprint"])
    err = capsys.readouterr().err
    assert "--imprint" in err and "--head cosine" in err
    with pytest.raises(SystemExit):
        parse_args(["--head", "cosine", "--lambda_mr", "1", "--mr_k", "9"])
    from cilfw.config import get_args_parser
    text = re.sub(r"\s+", " ", get_args_parser().format_help())
    for flag in ("--lambda_mr", "--mr_k", "--mr_margin", "--imprint"):
        assert flag in text
    assert "per-rank" in text


def test_start_up_errors_in_run():
    """A Namespace that did not come through parse_args is refused by the
    engine before anything is built. The run is a tiny CPU one, so that an
    engine without the check cannot train for long before the test fails."""
    from cilfw.config import check_args
    for extra, flag in ((dict(lambda_mr=1.0), "--lambda_mr"),
                        (dict(imprint=True), "--imprint")):
        args = parse_args([
            "--data_set", "synthetic", "--backbone", "resnet20",
            "--synthetic_classes", "4", "--num_bases", "2", "--increment",
            "2", "--num_epochs", "1", "--batch_size", "8", "--workers", "0",
            "--synthetic_train_size", "16", "--memory_size", "4",
            "--eval_every_epoch", "0", "--input_size", "16", "--no_aug",
            "--max_tasks", "1", "--dtype", "fp32", "--device", "cpu"])
        for k_, v in extra.items():
            setattr(args, k_, v)
        with pytest.raises(ValueError, match=flag + ".*--head cosine"):
            check_args(args)
        with pytest.raises(ValueError, match=flag + ".*--head cosine"):
            run(args)


def _run(extra):
    args = parse_args([
        "--data_set", "synthetic", "--backbone", "resnet20",
        "--synthetic_classes", "10", "--num_bases", "5", "--increment", "5",
        "--num_epochs", "1", "--batch_size", "32", "--workers", "0",
        "--synthetic_train_size", "320", "--memory_size", "20",
        "--eval_every_epoch", "0", "--input_size", "16", "--no_aug",
        "--lr", "0.05", "--seed", "3", "--dtype", "fp32", "--device", "cpu",
        "--head", "cosine", "--lambda_flat", "1", "--lambda_mr", "1",
        "--imprint"] + list(extra))
    seen = []
    orig = CilModel.imprint_new_head

    def spy(self, protos):
        out = orig(self, protos)
        w_old = torch.cat([h.weight for h in self.fc.heads[:-1]], 0)
        seen.append(dict(
            protos=tuple(protos.shape),
            proto_norms=protos.norm(dim=1).detach().clone(),
            new_norms=self.fc.heads[-1].weight.norm(dim=1).detach().clone(),
            old_mean=w_old.norm(dim=1).mean().item(), ret=out))
        return out

    CilModel.imprint_new_head = spy
    out = io.StringIO()
    try:
        with contextlib.redirect_stdout(out):
            accs = run(args)
    finally:
        CilModel.imprint_new_head = orig
    return accs, out.getvalue(), seen


def _epoch_lines(out, task):
    return re.findall(rf"^task {task} epoch \d+: .*$", out, re.M)


def _trajectory(line):
    return re.sub(r"imgs/s \d+", "imgs/s -", line)


@pytest.fixture(scope="module")
def lucir_run(tmp_path_factory):
    d = tmp_path_factory.mktemp("lucir")
    accs, out, seen = _run(["--output_dir", str(d)])
    return d, accs, out, seen


def test_engine_margin_rank_and_imprint(lucir_run):
    d, accs, out, seen = lucir_run
    assert len(accs) == 2
    t0, t1 = _epoch_lines(out, 0), _epoch_lines(out, 1)
    assert len(t0) == 1 and len(t1) == 1 and "mr:" not in t0[0]
    m = re.search(r"  mr: (\S+) \((\S+)\)", t1[0])
    assert m, t1[0]
    assert all(math.isfinite(float(v)) and float(v) >= 0.0
               for v in m.groups())
    assert "  flat: " in t1[0]
    # the imprint line: task 1 only, before that task's first epoch
    lines = re.findall(r"^imprint: .*$", out, re.M)
    assert len(lines) == 1 and "task 1" in lines[0] \
        and "5 new head rows" in lines[0]
    assert out.index(lines[0]) < out.index(t1[0])
    assert out.index(lines[0]) > out.index(t0[0])
    # through the spy: 5 unit prototypes in, rows of the mean old norm out
    assert len(seen) == 1
    s = seen[0]
    assert s["protos"][0] == 5 and s["ret"][0] == 5
    assert torch.allclose(s["proto_norms"], torch.ones(5), atol=1e-5)
    assert torch.allclose(s["new_norms"], torch.full((5,), s["old_mean"]),
                          rtol=1e-5)
    assert abs(s["ret"][1] - s["old_mean"]) <= 1e-5 * s["old_mean"]
    assert f"{s['old_mean']:.4f}" in lines[0]


def test_resume_repeats_task_1(lucir_run):
    d, accs, out, _ = lucir_run
    accs_r, out_r, seen_r = _run(["--output_dir", str(d / "again"),
                                  "--resume", str(d / "task_0.pth")])
    assert accs_r == accs and len(seen_r) == 1
    assert _trajectory(_epoch_lines(out_r, 1)[0]) \
        == _trajectory(_epoch_lines(out, 1)[0])
    assert re.findall(r"^imprint: .*$", out_r, re.M) \
        == re.findall(r"^imprint: .*$", out, re.M)
