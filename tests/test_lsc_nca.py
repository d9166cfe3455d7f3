"""PODNet's multi-proxy LSC head and NCA loss on the CPU: the fixtures of
_lsc_ref, the project's fp32 path against the fp64 oracle, gradcheck in fp64,
the head, the flags, the checkpoint key and CPU engine runs. The HIP kernels
are covered by test_lsc_nca_gpu.py."""

import contextlib
import io
import math
import os
import re

import pytest
import torch

import _lsc_ref as R
from cilfw import ops
from cilfw.config import parse_args, check_args
from cilfw.engine import run
from cilfw.models import CilModel
from cilfw.models.cil_model import CosineClassifier
from cilfw.ops import lsc as L

UPS = [1.0, 0.37]


# -------------------------------------------------------------------- fixtures

@pytest.mark.parametrize("name", R.NCA_IDS)
def test_nca_fixture_conditions(name):
    logits, targets, sigma, margin = R.make_nca(name)
    M, C = R.NCA_SHAPES[name]
    assert logits.shape == (M, C) and logits.dtype == torch.bfloat16
    assert sigma.item() == 8.0 and margin == 0.6
    ref = R.nca_ref(logits, targets, sigma, margin)
    assert ref["valid"].all()
    assert ref["min_abs_h"] >= R.MIN_ABS_H
    # the fp32 evaluation of h cannot flip a row
    assert ref["h_allow"].max().item() < 0.5 * R.MIN_ABS_H
    if M > 1:
        assert ref["n_active"] >= 1 and ref["n_inactive"] >= 1
    print(f"{name}: active {ref['n_active']} inactive {ref['n_inactive']} "
          f"min |h| {ref['min_abs_h']:.4f}")


def test_nca_seeds_are_the_first_that_qualify():
    for name in R.NCA_IDS:
        M, _ = R.NCA_SHAPES[name]
        for seed in range(R.NCA_SEEDS[name] + 1):
            ref = R.nca_ref(*R.make_nca(name, seed))
            ok = ref["min_abs_h"] >= R.MIN_ABS_H and (
                M == 1 or (ref["n_active"] >= 1 and ref["n_inactive"] >= 1))
            assert ok == (seed == R.NCA_SEEDS[name])


@pytest.mark.parametrize("name", R.LSC_IDS)
def test_lsc_fixture_conditions(name):
    sims, sigma, K, g = R.make_lsc(name)
    M, C, K_ = R.LSC_SHAPES[name]
    assert sims.shape == (M, C * K) and K == K_ and g.shape == (M, C)
    assert sims.dtype == torch.bfloat16 and sims.float().abs().max() <= 1
    assert g.float().abs().min() >= 0.5
    if K > 1:
        # spread proxies: the weights of a class are far from uniform
        a = R.lsc_ref(sims, sigma, K, 1.0, g)["a"]
        assert (a.amax(dim=2) / a.amin(dim=2)).max() > 3.0


# ------------------------------------------------- fp32 CPU path vs the oracle

def _lsc_cpu(sims, sigma, K, gamma, g, dtype=torch.float32):
    x = sims.to(dtype).requires_grad_(True)
    s = sigma.clone().requires_grad_(True)
    out = ops.lsc_reduce(x, s, K, gamma)
    out.backward(g.to(dtype))
    return out.detach(), x.grad, s.grad


@pytest.mark.parametrize("gamma", R.GAMMAS)
@pytest.mark.parametrize("name", R.LSC_IDS)
def test_lsc_cpu_against_the_oracle(name, gamma):
    sims, sigma, K, g = R.make_lsc(name)
    ref = R.lsc_ref(sims, sigma, K, gamma, g)
    out, dx, ds = _lsc_cpu(sims, sigma, K, gamma, g)
    assert out.dtype == torch.float32 and out.shape == (ref["M"], ref["C"])
    assert dx.shape == sims.shape and ds.shape == (1,)
    rs = dict(logits=R.worst_logits(out, ref), dsims=R.worst_dsims(dx, ref),
              dsigma=R.worst_lsc_dsigma(ds, ref))
    print(f"{name} gamma {gamma}: err/allowance " + " ".join(
        f"{k} {v:.4f}" for k, v in rs.items()))
    assert all(v <= 1.0 for v in rs.values()), rs
    # the upstream is not ignored
    ref2 = R.lsc_ref(sims, sigma, K, gamma, -g)
    assert R.worst_dsims(dx, ref2) > 1.0


def test_lsc_gamma_zero_is_the_plain_mean():
    sims, sigma, K, g = R.make_lsc("podnet")
    ref = R.lsc_ref(sims, sigma, K, 0.0, g)
    M, C = ref["M"], ref["C"]
    mean = sims.double().reshape(M, C, K).mean(dim=2)
    assert torch.allclose(ref["yhat"], mean, rtol=0, atol=1e-15)
    out, dx, ds = _lsc_cpu(sims, sigma, K, 0.0, g)
    assert R.worst_logits(out, ref) <= 1.0 and R.worst_dsims(dx, ref) <= 1.0
    assert R.worst_lsc_dsigma(ds, ref) <= 1.0
    # and differs from gamma 1
    assert R.worst_logits(out, R.lsc_ref(sims, sigma, K, 1.0, g)) > 1.0


def test_one_proxy_is_sigma_times_sims():
    sims, sigma, _, _ = R.make_lsc("odd")
    x = sims.float()
    for gamma in (0.0, 1.0, 4.0):
        assert torch.equal(ops.lsc_reduce(x, sigma, 1, gamma), sigma * x)
    x64 = sims.double().requires_grad_(True)
    s64 = sigma.double().requires_grad_(True)
    out = ops.lsc_reduce(x64, s64, 1, 4.0)
    out.backward(torch.ones_like(out))
    assert torch.equal(x64.grad, torch.full_like(x64, s64.item()))
    assert torch.allclose(s64.grad, x64.detach().sum().reshape(1))


@pytest.mark.parametrize("up", UPS)
@pytest.mark.parametrize("name", R.NCA_IDS)
def test_nca_cpu_against_the_oracle(name, up):
    logits, targets, sigma, margin = R.make_nca(name)
    u32 = float(torch.tensor(up, dtype=torch.float32))
    ref = R.nca_ref(logits, targets, sigma, margin, up=u32)
    lg = logits.float().requires_grad_(True)
    sg = sigma.clone().requires_grad_(True)
    loss = ops.nca_loss(lg, targets, sg, margin)
    (loss * up).backward()
    h, active = ops.nca_rows(logits.float(), targets, sigma, margin)
    assert loss.dim() == 0 and h.dtype == torch.float32
    rs = dict(loss=R.worst_loss(loss.detach(), ref), h=R.worst_h(h, ref),
              dlogits=R.worst_dlogits(lg.grad, ref),
              dsigma=R.worst_nca_dsigma(sg.grad, ref))
    print(f"{name} upstream {up}: err/allowance " + " ".join(
        f"{k} {v:.4f}" for k, v in rs.items()))
    assert all(v <= 1.0 for v in rs.values()), rs
    assert R.same_active(active, ref)
    assert (lg.grad[ref["dlogits"] == 0] == 0).all()
    if up != 1.0:
        ref1 = R.nca_ref(logits, targets, sigma, margin, up=1.0)
        assert R.worst_dlogits(lg.grad, ref1) > 1.0
        assert R.worst_nca_dsigma(sg.grad, ref1) > 1.0


def test_nca_excludes_the_positive_from_the_denominator():
    """C = 2: the denominator is the single negative, so h = l_neg - l_y +
    sigma margin exactly (the published code's stray exp(0) would add
    log(1 + exp(-l_neg)))."""
    logits = torch.tensor([[1.5, -0.25]], dtype=torch.float64)
    sigma = torch.tensor([2.0], dtype=torch.float64)
    h, active = ops.nca_rows(logits, torch.tensor([0]), sigma, 0.5)
    assert abs(h.item() - (-0.25 - (1.5 - 1.0))) < 1e-6 and active.item() == 0
    assert ops.nca_loss(logits, torch.tensor([0]), sigma, 0.5).item() == 0
    loss = ops.nca_loss(logits, torch.tensor([1]), sigma, 0.5)
    assert abs(loss.item() - (1.5 - (-0.25 - 1.0))) < 1e-15


def test_nca_invalid_targets_give_zero_rows():
    logits, targets, sigma, margin = R.make_nca("ragged")
    M, C = logits.shape
    t = R.with_invalid_targets(targets, C)
    ref = R.nca_ref(logits, t, sigma, margin)
    assert not ref["valid"][0] and not ref["valid"][2]
    lg = logits.float().requires_grad_(True)
    sg = sigma.clone().requires_grad_(True)
    loss = ops.nca_loss(lg, t, sg, margin)
    loss.backward()
    h, active = ops.nca_rows(logits.float(), t, sigma, margin)
    assert (lg.grad[0] == 0).all() and (lg.grad[2] == 0).all()
    assert h[0] == 0 and h[2] == 0 and active[0] == 0 and active[2] == 0
    assert R.worst_loss(loss.detach(), ref) <= 1.0
    assert R.worst_dlogits(lg.grad, ref) <= 1.0
    assert R.worst_nca_dsigma(sg.grad, ref) <= 1.0
    assert R.same_active(active, ref)
    # M stays the divisor: the loss is not that of the M - 2 valid rows alone
    keep = ref["valid"]
    sub = R.nca_ref(logits[keep], t[keep], sigma, margin)
    assert abs(ref["loss"].item() * M - sub["loss"].item() * (M - 2)) < 1e-9
    # every row skipped
    bad = torch.full_like(targets, C)
    lg2 = logits.float().requires_grad_(True)
    sg2 = sigma.clone().requires_grad_(True)
    loss2 = ops.nca_loss(lg2, bad, sg2, margin)
    loss2.backward()
    assert loss2.item() == 0 and (lg2.grad == 0).all() and sg2.grad.item() == 0


@pytest.mark.parametrize("sg", [0.0, -2.0])
def test_nonpositive_sigma_is_finite(sg):
    logits, targets, _, margin = R.make_nca("small")
    sigma = torch.tensor([sg], requires_grad=True)
    lg = logits.float().requires_grad_(True)
    loss = ops.nca_loss(lg, targets, sigma, margin)
    (loss * 0.37).backward()
    for t in (loss, lg.grad, sigma.grad):
        assert torch.isfinite(t).all()
    ref = R.nca_ref(logits, targets, sigma.detach(), margin,
                    up=float(torch.tensor(0.37)))
    assert R.worst_loss(loss.detach(), ref) <= 1.0
    assert R.worst_dlogits(lg.grad, ref) <= 1.0
    sims, _, K, g = R.make_lsc("podnet")
    x = sims.float().requires_grad_(True)
    s2 = torch.tensor([sg], requires_grad=True)
    out = ops.lsc_reduce(x, s2, K, 1.0)
    out.backward(g.float())
    ref = R.lsc_ref(sims, s2.detach(), K, 1.0, g)
    assert torch.isfinite(out).all() and torch.isfinite(x.grad).all()
    assert R.worst_logits(out.detach(), ref) <= 1.0
    assert R.worst_dsims(x.grad, ref) <= 1.0
    assert R.worst_lsc_dsigma(s2.grad, ref) <= 1.0


def test_gradcheck_fp64():
    sims, sigma, K, _ = R.make_lsc("podnet")
    x = sims.double().requires_grad_(True)
    s = sigma.double().requires_grad_(True)
    for gamma in (0.0, 1.0, 4.0):
        assert torch.autograd.gradcheck(
            lambda a, b: ops.lsc_reduce(a, b, K, gamma), (x, s))
    out = ops.lsc_reduce(x, s, K, 1.0)
    assert out.dtype == torch.float64
    logits, targets, sigma, margin = R.make_nca("small")
    lg = logits.double().requires_grad_(True)
    s = sigma.double().requires_grad_(True)
    assert torch.autograd.gradcheck(
        lambda a, b: ops.nca_loss(a, targets, b, margin), (lg, s))
    t = R.with_invalid_targets(targets, logits.shape[1])
    assert torch.autograd.gradcheck(
        lambda a, b: ops.nca_loss(a, t, b, margin), (lg, s))
    assert ops.nca_loss(lg, targets, s, margin).dtype == torch.float64


def test_argument_refusals():
    sims, sigma, K, _ = R.make_lsc("podnet")
    x = sims.float()
    for bad in (0, 17, -1):
        with pytest.raises(AssertionError, match="nb_proxy must be"):
            ops.lsc_reduce(x, sigma, bad, 1.0)
    with pytest.raises(AssertionError, match="multiple of nb_proxy"):
        ops.lsc_reduce(x, sigma, 7, 1.0)
    with pytest.raises(AssertionError, match="gamma must be"):
        ops.lsc_reduce(x, sigma, K, -0.5)
    with pytest.raises(AssertionError, match="fp32 or fp64"):
        ops.lsc_reduce(sims, sigma, K, 1.0)
    with pytest.raises(AssertionError, match="sigma"):
        ops.lsc_reduce(x, torch.ones(2), K, 1.0)
    logits, targets, sigma, margin = R.make_nca("small")
    lg = logits.float()
    with pytest.raises(AssertionError, match="C >= 2"):
        ops.nca_loss(lg[:, :1].contiguous(), targets, sigma, margin)
    with pytest.raises(AssertionError, match="margin must be"):
        ops.nca_loss(lg, targets, sigma, -0.1)
    with pytest.raises(AssertionError, match="targets"):
        ops.nca_loss(lg, targets[:3], sigma, margin)
    with pytest.raises(AssertionError, match="targets"):
        ops.nca_loss(lg, targets.int(), sigma, margin)
    with pytest.raises(AssertionError, match="fp32 or fp64"):
        ops.nca_loss(logits, targets, sigma, margin)


# ------------------------------------------------------------------------ head

def test_single_proxy_head_is_unchanged():
    """nb_proxy = 1: the same parameters from the same RNG stream, no new
    buffer or state-dict key, and the forward torch.equal to the single
    cosine_linear call."""
    torch.manual_seed(5)
    a = CosineClassifier(24, 6, 2.5)
    a.adaption(4)
    torch.manual_seed(5)
    b = CosineClassifier(24, 6, 2.5, nb_proxy=1)
    b.adaption(4)
    assert list(a.state_dict()) == ["sigma", "heads.0.weight",
                                    "heads.1.weight"]
    assert list(b.state_dict()) == list(a.state_dict())
    assert not list(b.buffers())
    for k, v in a.state_dict().items():
        assert torch.equal(v, b.state_dict()[k])
    x = torch.randn(7, 24)
    w = torch.cat([h.weight for h in b.heads], 0)
    assert torch.equal(b(x), ops.cosine_linear(x, w, b.sigma))
    assert torch.equal(b(x), a(x))


def test_multi_proxy_head():
    torch.manual_seed(5)
    fc = CosineClassifier(24, 6, 2.5, nb_proxy=3, proxy_gamma=4.0)
    fc.adaption(4)
    assert [tuple(h.weight.shape) for h in fc.heads] == [(18, 24), (12, 24)]
    assert [h.out_features for h in fc.heads] == [6, 4]
    assert fc.nb_classes == 10
    assert "unit_scale" not in fc.state_dict()
    assert not fc.unit_scale.requires_grad
    x = torch.randn(7, 24, requires_grad=True)
    out = fc(x)
    assert out.shape == (7, 10)
    w = torch.cat([h.weight for h in fc.heads], 0)
    sims = ops.cosine_linear(x, w, torch.ones(1))
    assert sims.abs().max() <= 1 + 1e-6
    assert torch.equal(out, ops.lsc_reduce(sims, fc.sigma, 3, 4.0))
    out.sum().backward()
    assert fc.sigma.grad is not None and x.grad is not None
    assert all(h.weight.grad.abs().sum() > 0 for h in fc.heads)
    with pytest.raises(ValueError, match="nb_proxy"):
        CosineClassifier(24, 6, 1.0, nb_proxy=17)
    with pytest.raises(ValueError, match="cosine head"):
        CilModel("resnet20", 32, head="linear", nb_proxy=3)


def test_frozen_teacher_applies_the_same_reduce():
    torch.manual_seed(1)
    model = CilModel("resnet20", 16, head="cosine", cos_scale_init=3.0,
                     nb_proxy=3, proxy_gamma=2.0)
    model.prev_model_adaption(4)
    model.eval()
    x = torch.randn(5, 16, 16, 3)
    with torch.no_grad():
        ref = model(x)[0]
    teacher = model.copy()
    teacher.freeze(["all"])
    teacher.cast_compute_weights_(torch.float32)
    assert len(teacher.fc._frozen_cat) == 3
    out = teacher(x)[0]
    assert out.shape == (5, 4) and not out.requires_grad
    assert torch.allclose(out, ref, rtol=1e-5, atol=1e-6)


def test_imprint_refused_with_proxies():
    model = CilModel("resnet20", 16, head="cosine", nb_proxy=2)
    model.prev_model_adaption(3)
    model.prev_model_adaption(2)
    with pytest.raises(RuntimeError, match="nb_proxy > 1"):
        model.imprint_new_head(torch.zeros(2, model.feature_dim))


# ----------------------------------------------------------------------- flags

def _refused(argv, capsys, *words):
    with pytest.raises(SystemExit):
        parse_args(argv)
    err = capsys.readouterr().err
    assert all(w in err for w in words), err


def test_cli_flags(capsys):
    a = parse_args([])
    assert a.nb_proxy == 1 and a.proxy_gamma == 1.0 and a.cls_loss == "ce"
    assert a.nca_margin == 0.6
    a = parse_args(["--head", "cosine", "--nb_proxy", "10", "--proxy_gamma",
                    "2", "--cls_loss", "nca", "--nca_margin", "0.4",
                    "--lambda_kd", "0", "--lambda_pod", "3", "--lambda_flat",
                    "1"])
    assert a.nb_proxy == 10 and a.proxy_gamma == 2.0 and a.cls_loss == "nca"
    assert a.nca_margin == 0.4
    _refused(["--nb_proxy", "3"], capsys, "--nb_proxy", "--head cosine")
    _refused(["--proxy_gamma", "2"], capsys, "--proxy_gamma",
             "--head cosine")
    _refused(["--head", "cosine", "--nb_proxy", "0"], capsys, "--nb_proxy")
    _refused(["--head", "cosine", "--nb_proxy", "17"], capsys, "--nb_proxy")
    _refused(["--head", "cosine", "--proxy_gamma", "-1"], capsys,
             "--proxy_gamma")
    _refused(["--cls_loss", "nca", "--lambda_kd", "0"], capsys, "--cls_loss",
             "--head cosine")
    _refused(["--head", "cosine", "--cls_loss", "nca"], capsys, "--cls_loss",
             "--lambda_kd")
    _refused(["--head", "cosine", "--cls_loss", "nca", "--lambda_kd", "0",
              "--dynamic_lambda_kd"], capsys, "--cls_loss",
             "--dynamic_lambda_kd")
    _refused(["--head", "cosine", "--cls_loss", "nca", "--lambda_kd", "0",
              "--smooth", "0.1"], capsys, "--cls_loss", "--smooth")
    _refused(["--head", "cosine", "--cls_loss", "nca", "--lambda_kd", "0",
              "--nca_margin", "-0.1"], capsys, "--nca_margin")
    _refused(["--head", "cosine", "--imprint", "--nb_proxy", "2"], capsys,
             "--imprint", "--nb_proxy")
    from cilfw.config import get_args_parser
    text = re.sub(r"\s+", " ", get_args_parser().format_help())
    for flag in ("--nb_proxy", "--proxy_gamma", "--cls_loss", "--nca_margin"):
        assert flag in text


BASE = ["--data_set", "synthetic", "--backbone", "resnet20",
        "--synthetic_classes", "10", "--num_bases", "5", "--increment", "5",
        "--num_epochs", "1", "--batch_size", "32", "--workers", "0",
        "--synthetic_train_size", "320", "--memory_size", "20",
        "--eval_every_epoch", "0", "--input_size", "16", "--no_aug",
        "--lr", "0.05", "--seed", "3", "--dtype", "fp32", "--device", "cpu"]
PODNET = ["--head", "cosine", "--nb_proxy", "3", "--cls_loss", "nca",
          "--lambda_kd", "0", "--lambda_flat", "1"]


def test_start_up_errors_in_run():
    """A Namespace that did not come through parse_args is refused by the
    engine before anything is built."""
    for extra, words in ((dict(cls_loss="nca", lambda_kd=0.0),
                          "--cls_loss nca.*--head cosine"),
                         (dict(nb_proxy=3), "--nb_proxy.*--head cosine")):
        args = parse_args(BASE + ["--max_tasks", "1"])
        for k, v in extra.items():
            setattr(args, k, v)
        with pytest.raises(ValueError, match=words):
            check_args(args)
        with pytest.raises(ValueError, match=words):
            run(args)


# ---------------------------------------------------------------------- engine

def _run(extra):
    args = parse_args(BASE + list(extra))
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        accs = run(args)
    return accs, out.getvalue()


def _epoch_lines(out, task=None):
    pat = r"^task \d+ epoch \d+: .*$" if task is None \
        else rf"^task {task} epoch \d+: .*$"
    return [re.sub(r"imgs/s \d+", "", v) for v in re.findall(pat, out, re.M)]


@pytest.fixture(scope="module")
def podnet_run(tmp_path_factory):
    d = tmp_path_factory.mktemp("lsc_ckpt")
    return (str(d),) + _run(PODNET + ["--output_dir", str(d)])


def test_engine_podnet_flag_set(podnet_run):
    _, accs, out = podnet_run
    assert len(accs) == 2
    lines = _epoch_lines(out)
    assert len(lines) == 2
    for line in lines:
        m = re.search(r"  nca: (\S+) \((\S+)\)", "  " + line.split(": ", 1)[1])
        assert m, line
        assert all(math.isfinite(float(v)) and float(v) >= 0.0
                   for v in m.groups())
        assert "ce:" not in line and "kd:" not in line
        assert "loss:" in line and "acc1:" in line
    assert "flat:" in lines[1] and "flat:" not in lines[0]


def test_engine_podnet_run_repeats(podnet_run):
    _, accs, out = podnet_run
    accs2, out2 = _run(PODNET)
    assert accs2 == accs
    assert _epoch_lines(out2) == _epoch_lines(out)


def test_checkpoint_round_trip_and_mismatch(podnet_run):
    d, accs, _ = podnet_run
    path = os.path.join(d, "task_0.pth")
    state = torch.load(path, map_location="cpu", weights_only=False)
    assert state["nb_proxy"] == 3 and state["head_kind"] == "cosine"
    assert state["head_widths"] == [5]
    assert tuple(state["model"]["fc.heads.0.weight"].shape)[0] == 15
    assert not any("unit_scale" in k for k in state["model"])
    # resuming after task 0 repeats task 1 of the uninterrupted run
    accs2, out2 = _run(PODNET + ["--resume", path])
    assert len(accs2) == 2 and accs2[0] == accs[0]
    assert "resumed from" in out2
    with pytest.raises(ValueError, match="--nb_proxy 3.*--nb_proxy 1"):
        _run(["--head", "cosine", "--resume", path])
    with pytest.raises(ValueError, match="--nb_proxy 3.*--nb_proxy 2"):
        _run(["--head", "cosine", "--nb_proxy", "2", "--resume", path])


def test_checkpoint_without_the_key_means_one_proxy(tmp_path):
    _run(["--head", "cosine", "--max_tasks", "1", "--output_dir",
          str(tmp_path)])
    path = os.path.join(str(tmp_path), "task_0.pth")
    state = torch.load(path, map_location="cpu", weights_only=False)
    assert "nb_proxy" not in state
    with pytest.raises(ValueError, match="--nb_proxy 1.*--nb_proxy 3"):
        _run(["--head", "cosine", "--nb_proxy", "3", "--resume", path])


def test_default_flags_launch_nothing_new(monkeypatch):
    """Every new flag at its default: neither new op is called, the epoch
    lines carry the meters of before (lr, ce, kd, loss, acc1 in that order,
    no nca) and equal, on this same code, those of a run that spells the
    defaults out. The lines are not pinned to values recorded from the
    parent commit; that the default path computes what it computed is shown
    by the existing suite passing unchanged."""
    calls = []
    for fn in ("lsc_reduce", "nca_loss"):
        orig = getattr(L, fn)
        monkeypatch.setattr(L, fn, lambda *a, _o=orig, _n=fn, **k: (
            calls.append(_n), _o(*a, **k))[1])
        monkeypatch.setattr(ops, fn, getattr(L, fn))
    accs, out = _run(["--head", "cosine"])
    accs2, out2 = _run(["--head", "cosine", "--nb_proxy", "1",
                        "--proxy_gamma", "1.0", "--cls_loss", "ce",
                        "--nca_margin", "0.6"])
    assert calls == []
    assert accs == accs2 and _epoch_lines(out) == _epoch_lines(out2)
    for line in _epoch_lines(out):
        names = re.findall(r"(\w+): ", line.split(": ", 1)[1])
        assert names == ["lr", "ce", "kd", "loss", "acc1"], line
    # and the spy does see the ops when they run
    _run(PODNET + ["--max_tasks", "1"])
    assert "lsc_reduce" in calls and "nca_loss" in calls
