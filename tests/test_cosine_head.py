"""Cosine head and embedding distillation on the CPU: the torch path of
ops/cosine.py against torch.autograd.gradcheck and the fp64 oracle of
_cos_ref, the comparator self-test, CosineClassifier / CilModel, the CLI
flags, the engine wiring and the checkpoint's head kind."""

import contextlib
import io
import math
import re

import pytest
import torch

import _cos_ref as R
from cilfw import ops
from cilfw.cil.checkpoint import load_task_checkpoint
from cilfw.config import parse_args
from cilfw.engine import run
from cilfw.models import CilModel, CosineClassifier

BF = torch.bfloat16


# ------------------------------------------------------------------ fp64 checks

def test_gradcheck_cosine_linear():
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(5, 16, generator=g, dtype=torch.float64).abs() + 0.1
         ).requires_grad_(True)
    w = torch.randn(3, 16, generator=g, dtype=torch.float64,
                    requires_grad=True)
    s = torch.tensor([2.5], dtype=torch.float64, requires_grad=True)
    assert ops.cosine_linear(x, w, s).dtype == torch.float64
    assert torch.autograd.gradcheck(ops.cosine_linear, (x, w, s))


def test_gradcheck_flat_loss():
    g = torch.Generator().manual_seed(2)
    s = (torch.randn(5, 16, generator=g, dtype=torch.float64).abs() + 0.1
         ).requires_grad_(True)
    t = (torch.randn(5, 16, generator=g, dtype=torch.float64).abs() + 0.1
         ).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a: ops.flat_loss(a, t), (s,))
    ops.flat_loss(s, t).backward()
    assert t.grad is None  # the teacher gets no gradient


def _head_cpu(x, w, sigma, g):
    x = x.clone().requires_grad_(True)
    w = w.clone().requires_grad_(True)
    sigma = sigma.clone().requires_grad_(True)
    logits = ops.cosine_linear(x, w, sigma)
    logits.backward(g)
    return logits.detach(), x.grad, w.grad, sigma.grad


@pytest.mark.parametrize("name", R.SHAPE_IDS)
def test_cpu_head_within_allowances(name):
    x, w, sigma, dy = R.make_head(name)
    ref = R.head_ref(x, w, sigma, dy)
    logits, dx, dw, ds = _head_cpu(x, w, sigma, dy)
    assert logits.dtype == BF and dx.dtype == BF
    assert dw.dtype == torch.float32 and ds.shape == (1,)
    rs = dict(logits=R.worst_logits(logits, ref), dx=R.worst_dx(dx, ref),
              dw=R.worst_dw(dw, ref), dsigma=R.worst_dsigma(ds, ref))
    print(f"{name}: err/allowance " + " ".join(
        f"{k} {v:.4f}" for k, v in rs.items()))
    assert all(v <= 1.0 for v in rs.values()), rs


def _flat_cpu(s, t, scale=1.0):
    s = s.clone().requires_grad_(True)
    loss = ops.flat_loss(s, t)
    (loss * scale).backward()
    return loss.detach(), s.grad


@pytest.mark.parametrize("name", R.SHAPE_IDS)
def test_cpu_flat_within_allowances(name):
    s, t = R.make_feats(name)
    ref = R.flat_ref(s, t)
    loss, ds = _flat_cpu(s, t)
    assert ds.dtype == BF and ds.shape == s.shape
    rs = dict(l=R.worst_flat_rows(ops.flat_dist(s, t), ref),
              loss=R.worst_flat_loss(loss, ref),
              ds=R.worst_flat_grad(ds, ref))
    print(f"{name}: err/allowance " + " ".join(
        f"{k} {v:.4f}" for k, v in rs.items()))
    assert all(v <= 1.0 for v in rs.values()), rs
    up = float(torch.tensor(0.37, dtype=torch.float32))
    _, ds37 = _flat_cpu(s, t, scale=0.37)
    assert R.worst_flat_grad(ds37, ref, scale=up) <= 1.0
    assert R.worst_flat_grad(ds37, ref, scale=1.0) > 1.0


@pytest.mark.parametrize("dtype", [BF, torch.float32, torch.float64])
def test_zero_rows_and_equal_features_cpu(dtype):
    """A zero feature row and a zero weight row: logits and gradients exactly
    0 and finite. Bitwise-equal student and teacher: loss 0, gradient 0."""
    x, w, sigma, dy = R.make_head("cifar64")
    x, dy = x.to(dtype), dy.to(dtype)
    if dtype == torch.float64:
        w, sigma = w.double(), sigma.double()
    x[2] = 0
    w[1] = 0
    logits, dx, dw, _ = _head_cpu(x, w, sigma, dy)
    assert (logits[2] == 0).all() and (logits[:, 1] == 0).all()
    assert (dx[2] == 0).all() and (dw[1] == 0).all()
    assert all(torch.isfinite(t.double()).all() for t in (logits, dx, dw))
    for zero_row in (False, True):
        s = R.make_feats("cifar64")[0].to(dtype)
        if zero_row:
            s[3] = 0
        loss, ds = _flat_cpu(s, s.clone())
        assert loss.item() == 0.0
        assert torch.isfinite(ds.double()).all() and (ds == 0).all()
        assert (ops.flat_dist(s, s.clone()) == 0).all()


def test_flat_shape_mismatch_refused():
    s, t = R.make_feats("cifar64")
    with pytest.raises(AssertionError, match="student features"):
        ops.flat_loss(s, t[:, :32])
    with pytest.raises(AssertionError, match="student features"):
        ops.flat_dist(s[:3], t)


# --------------------------------------------------------- comparator self-test

def _bf(t):
    return t.to(BF)


def test_comparators_accept_the_rounded_oracle():
    x, w, sigma, dy = R.make_head("sweep520")
    ref = R.head_ref(x, w, sigma, dy)
    assert R.worst_logits(_bf(ref["logits"]), ref) <= 1.0
    assert R.worst_dx(_bf(ref["dx"]), ref) <= 1.0
    assert R.worst_dw(ref["dw"].float(), ref) <= 1.0
    assert R.worst_dsigma(ref["dsigma"].float(), ref) <= 1.0
    assert R.worst_rinv(ref["rw"].float(), ref["rw"], ref["D"]) <= 1.0
    s, t = R.make_feats("sweep520")
    fr = R.flat_ref(s, t)
    assert R.worst_flat_rows(fr["l"].float(), fr) <= 1.0
    assert R.worst_flat_loss(fr["loss"].float(), fr) <= 1.0
    assert R.worst_flat_grad(_bf(fr["ds"]), fr) <= 1.0


def test_comparators_reject_seeded_faults():
    """"Wrong kernels" built from the fp64 oracle, one seeded fault each,
    rounded like a real kernel's output; each must be rejected by more than
    10 times its bound."""
    x, w, sigma, dy = R.make_head("sweep520")
    ref = R.head_ref(x, w, sigma, dy)
    M, C, D, sg = ref["M"], ref["C"], ref["D"], ref["sigma"]
    assert D == 520 and sg != 1.0

    # 1: sigma dropped from dx
    r = R.worst_dx(_bf(ref["dx"] / sg), ref)
    print(f"fault 1 (sigma dropped from dx): {r:.1f}")
    assert r > 10.0

    # 2: the projection term x^ (x^ . G) dropped. With signed weights and
    # upstream the term is small against mag (G is a sum of C terms of random
    # sign) and the fault is rejected by about 2 times the bound; the 10
    # times are asked of data without that cancellation, |w| and |dy|.
    x64 = x.double()
    G = dy.double() @ ref["wn"]
    r = R.worst_dx(_bf(sg * ref["rx"].reshape(M, 1) * G), ref)
    assert r > 1.0
    refp = R.head_ref(x, w.abs(), sigma, dy.abs())
    Gp = dy.abs().double() @ refp["wn"]
    rp = R.worst_dx(_bf(sg * refp["rx"].reshape(M, 1) * Gp), refp)
    print(f"fault 2 (projection dropped): {r:.1f}, unsigned data {rp:.1f}")
    assert rp > 10.0

    # 3: weight norm taken from the bf16-rounded weights of a badly scaled
    # row: every entry sits just below a bf16 rounding midpoint, so all of
    # them round down and the norm is off by almost half a bf16 ulp
    wb = w.clone()
    sign = torch.where(wb[0] < 0, -1.0, 1.0)
    wb[0] = sign * (1.0 + 2.0 ** -8 - 2.0 ** -14)
    refb = R.head_ref(x, wb, sigma, dy)
    r_fault = R.rinv64(wb.to(BF).double()).reshape(C)
    r = R.worst_rinv(r_fault.float(), refb["rw"], D)
    print(f"fault 3 (norm of bf16-rounded weights): {r:.1f}")
    assert r > 10.0

    # 4: 1/M dropped from the flat loss
    s, t = R.make_feats("sweep520")
    fr = R.flat_ref(s, t)
    r = R.worst_flat_loss((fr["loss"] * M).float(), fr)
    print(f"fault 4 (1/M dropped): {r:.1f}")
    assert M > 1 and r > 10.0

    # 5: a 512-element sweep truncated at D = 520: the last 8 elements enter
    # no sum
    r_tr = R.rinv64(x64[:, :512]).reshape(M)
    ra = R.worst_rinv(r_tr.float(), ref["rx"], D)
    s64, t64 = s.double(), t.double()
    u = s64 * R.rinv64(s64) - t64 * R.rinv64(t64)
    rb = R.worst_flat_rows((0.5 * (u[:, :512] ** 2).sum(dim=1)).float(), fr)
    xs_tr = ref["xs"].clone()
    for fill in (0.0, float("nan")):
        xs_tr[:, 512:] = fill
        assert R.worst_unit(_bf(xs_tr), ref["xs"], D) > 10.0
    print(f"fault 5 (truncated sweep): rinv {ra:.1f} l {rb:.1f}")
    assert ra > 10.0 and rb > 10.0

    # 6: zero-row gradient G / eps in place of 0
    xz = x.clone()
    xz[1] = 0
    refz = R.head_ref(xz, w, sigma, dy)
    assert (refz["dx"][1] == 0).all() and (refz["dx_mag"][1] == 0).all()
    bad = refz["dx"].clone()
    bad[1] = sg * G[1] / 1e-12
    r = R.worst_dx(_bf(bad), refz)
    print(f"fault 6 (G / eps on a zero row): {r}")
    assert r > 10.0
    assert R.worst_dx(_bf(refz["dx"]), refz) <= 1.0


# ------------------------------------------------------------------------ model

def _cos_model(nb=(4, 3), scale=2.0):
    torch.manual_seed(0)
    model = CilModel("resnet20", 16, head="cosine", cos_scale_init=scale)
    for n in nb:
        model.prev_model_adaption(n)
    return model.eval()


def test_cosine_classifier_grows_in_head_order():
    model = _cos_model()
    fc = model.fc
    assert isinstance(fc, CosineClassifier)
    assert len(fc) == 2 and fc.nb_classes == 7
    assert [h.out_features for h in fc.heads] == [4, 3]
    assert fc[1].weight.shape == (3, model.feature_dim)
    assert not any("bias" in n for n, _ in fc.named_parameters())
    assert fc.sigma.shape == (1,) and fc.sigma.item() == 2.0
    assert fc.sigma.requires_grad
    f = torch.randn(6, model.feature_dim).abs()
    with torch.no_grad():
        logits = fc(f)
        for i, lo in ((0, 0), (1, 4)):
            want = 2.0 * torch.nn.functional.normalize(f, dim=1) \
                @ torch.nn.functional.normalize(fc[i].weight, dim=1).t()
            got = logits[:, lo:lo + fc[i].out_features]
            assert torch.allclose(got, want, atol=1e-6)
    assert logits.abs().max() <= 2.0 + 1e-6


def test_logits_invariant_under_row_rescaling():
    model = _cos_model()
    f = torch.randn(6, model.feature_dim).abs()
    with torch.no_grad():
        before = model.fc(f)
        model.fc[0].weight.mul_(7.0)
        model.fc[1].weight[1].mul_(0.01)
        after = model.fc(f)
    assert torch.allclose(before, after, atol=1e-6)


def test_no_weight_align_on_a_cosine_head(capsys):
    model = _cos_model()
    w = [h.weight.detach().clone() for h in model.fc.heads]
    model.after_model_adaption(3)
    assert "skipped" in capsys.readouterr().out
    assert all(torch.equal(a, h.weight) for a, h in zip(w, model.fc.heads))
    with pytest.raises(RuntimeError, match="cosine"):
        model.weight_align(3)
    with pytest.raises(ValueError, match="foo"):
        CilModel("resnet20", 16, head="foo")


def test_cast_compute_weights_keeps_the_logits():
    model = _cos_model(scale=3.0)
    x = torch.randn(4, 16, 16, 3)
    with torch.no_grad():
        before, feats = model(x)
    teacher = model.copy()
    teacher.freeze(["all"])
    teacher.cast_compute_weights_(BF)
    wn, sg = teacher.fc._frozen_cat
    assert wn.dtype == BF and wn.shape == (7, model.feature_dim)
    assert sg.item() == 3.0
    assert teacher.fc[0].weight.dtype == torch.float32  # masters untouched
    with torch.no_grad():
        after = teacher.fc(feats)
    # the one new rounding is that of the unit rows to bf16: 2^-8 relative on
    # every product, against sigma sum_k |x^_k w^_k| <= sigma
    assert (after - before).abs().max().item() <= 3.0 * 2.0 ** -8
    assert not torch.equal(after, before)


def test_sigma_gets_a_flat_slot():
    """A 1-element parameter needs no special case in the engine / FlatSGD:
    it owns one element of the flat buffers and is stepped like the rest."""
    from cilfw.distributed import DataParallelEngine
    from cilfw.optim import FlatSGD
    model = _cos_model(nb=(5,), scale=1.0).train()
    engine = DataParallelEngine(model)
    opt = FlatSGD(engine, lr=0.1)
    sigma = model.fc.sigma
    i = [j for j, p in enumerate(engine.params) if p is sigma]
    assert len(i) == 1
    off = engine._offsets[i[0]]
    assert sigma.data_ptr() == engine.flat_params[off:off + 1].data_ptr()
    assert sigma.grad.data_ptr() == engine.flat_grads[off:off + 1].data_ptr()
    opt.zero_grad()
    logits, _ = model(torch.randn(8, 16, 16, 3))
    ops.cross_entropy(logits.float(), torch.arange(8) % 5).backward()
    engine.finalize()
    assert engine.flat_grads[off].item() != 0.0
    opt.step()
    assert sigma.item() != 1.0 and sigma.item() == engine.flat_params[off]


# ---------------------------------------------------------- engine / checkpoint

def test_cli_flags():
    a = parse_args([])
    assert a.head == "linear" and a.lambda_flat == 0.0
    assert a.cos_scale_init == 1.0
    a = parse_args(["--head", "cosine", "--cos_scale_init", "4",
                    "--lambda_flat", "2.5"])
    assert a.head == "cosine" and a.cos_scale_init == 4.0
    assert a.lambda_flat == 2.5
    with pytest.raises(SystemExit):
        parse_args(["--head", "foo"])


def _run(extra):
    args = parse_args([
        "--data_set", "synthetic", "--backbone", "resnet20",
        "--synthetic_classes", "10", "--num_bases", "5", "--increment", "5",
        "--num_epochs", "1", "--batch_size", "32", "--workers", "0",
        "--synthetic_train_size", "320", "--memory_size", "20",
        "--eval_every_epoch", "0", "--input_size", "16", "--no_aug",
        "--lr", "0.05", "--seed", "3", "--dtype", "fp32", "--device", "cpu",
    ] + list(extra))
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        accs = run(args)
    return accs, out.getvalue()


def _trajectory(out):
    """stdout without the one figure that is a wall-clock time."""
    return re.sub(r"imgs/s \d+", "imgs/s -", out)


def test_default_flags_take_todays_path():
    accs, out = _run([])
    accs2, out2 = _run(["--lambda_flat", "0", "--head", "linear"])
    assert accs == accs2
    assert _trajectory(out) == _trajectory(out2)
    assert "flat" not in out and "cosine" not in out
    assert "gamma:" in out  # weight aligning ran


@pytest.fixture(scope="module")
def cosine_run(tmp_path_factory):
    d = tmp_path_factory.mktemp("cos")
    accs, out = _run(["--head", "cosine", "--lambda_flat", "1", "--nme_eval",
                      "--output_dir", str(d)])
    return d, accs, out


def _epoch_lines(out, task):
    return re.findall(rf"^task {task} epoch \d+: .*$", out, re.M)


def test_engine_cosine_flat_nme(cosine_run):
    d, accs, out = cosine_run
    assert len(accs) == 2
    t0, t1 = _epoch_lines(out, 0), _epoch_lines(out, 1)
    assert len(t0) == 1 and len(t1) == 1 and "flat:" not in t0[0]
    m = re.search(r"  flat: (\S+) \((\S+)\)", t1[0])
    assert m, t1[0]
    assert all(math.isfinite(float(v)) and 0.0 <= float(v) <= 2.0
               for v in m.groups())
    assert "weight aligning skipped" in out and "gamma:" not in out
    assert len(re.findall(r"@NME1 = ", out)) == 2
    state = torch.load(d / "task_1.pth", map_location="cpu",
                       weights_only=False)
    assert state["head_kind"] == "cosine"
    assert "fc.sigma" in state["model"]
    assert state["model"]["fc.sigma"].item() != 1.0  # sigma was trained
    assert not any(k.endswith("bias") and k.startswith("fc.")
                   for k in state["model"])


def test_resume_repeats_task_1(cosine_run):
    d, accs, out = cosine_run
    accs_r, out_r = _run(["--head", "cosine", "--lambda_flat", "1",
                          "--nme_eval", "--output_dir", str(d / "again"),
                          "--resume", str(d / "task_0.pth")])
    assert accs_r == accs
    assert _trajectory(_epoch_lines(out_r, 1)[0]) \
        == _trajectory(_epoch_lines(out, 1)[0])


def test_resume_with_another_head_is_refused(cosine_run):
    d, _, _ = cosine_run
    with pytest.raises(ValueError, match="cosine.*linear"):
        _run(["--resume", str(d / "task_0.pth")])


def test_checkpoint_without_head_kind_loads_as_linear(tmp_path):
    _run(["--max_tasks", "1", "--output_dir", str(tmp_path)])
    path = tmp_path / "task_0.pth"
    state = torch.load(path, map_location="cpu", weights_only=False)
    assert "head_kind" not in state
    model = CilModel("resnet20", 16)
    load_task_checkpoint(str(path), model, None, parse_args([]),
                         restore_rng=False)
    assert model.head_kind == "linear" and model.fc.nb_classes == 5
    with pytest.raises(ValueError, match="linear.*cosine"):
        load_task_checkpoint(str(path), CilModel("resnet20", 16,
                                                 head="cosine"),
                             None, parse_args([]), restore_rng=False)
