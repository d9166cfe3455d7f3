"""NME evaluation on the CPU: ops.nme_prototypes / ops.nme_topk (torch path)
against the fp64 oracle of tests/_nme_ref.py, the CIL layer on a tiny model,
the CLI flag, and the engine wiring (a run with --nme_eval trains exactly
like one without, prints the NME lines, keeps and checkpoints nme1s)."""

import contextlib
import io
import re

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

import _nme_ref as R
from cilfw import ops
from cilfw.cil import RehearsalMemory
from cilfw.cil.nme import build_prototypes, evaluate_nme
from cilfw.config import parse_args
from cilfw.data.scenario import TaskSet
from cilfw.data.transforms import EvalTransform
from cilfw.engine import run
from cilfw.models import CilModel


@pytest.mark.parametrize("shape_id", [1, 2, 3])
def test_ops_match_oracle(shape_id):
    N, C, D, q = R.SHAPES[shape_id]
    inp = R.make_inputs(shape_id)
    protos = ops.nme_prototypes(inp["ex"].reshape(C * q, D),
                                R.seg_offsets(C, q))
    assert protos.shape == (C, D) and protos.dtype == torch.float32
    R.check_protos(protos, inp["ex"], f"cpu protos shape {shape_id}")
    maxk = min(5, C)
    idx, score, counts = ops.nme_topk(inp["x"], protos, maxk, inp["targets"])
    assert idx.dtype == torch.int32
    R.check_topk(idx, score, counts, inp["x"], protos, inp["targets"], maxk,
                 f"cpu topk shape {shape_id}")
    assert 0 < counts[0].item() < N  # every third target is wrong
    idx2, score2, none = ops.nme_topk(inp["x"], protos, maxk)
    assert none is None and torch.equal(idx, idx2) \
        and torch.equal(score, score2)


def test_ragged_segments():
    """Classes with different exemplar counts: each prototype only sees its
    own segment."""
    _, C, D, q = R.SHAPES[1]
    ex = R.make_inputs(1)["ex"]
    keep = [q, 1, 3, q - 1, 2]
    feats = torch.cat([ex[c, :k] for c, k in enumerate(keep)])
    off = np.concatenate([[0], np.cumsum(keep)])
    protos = ops.nme_prototypes(feats, torch.from_numpy(off))
    for c, k in enumerate(keep):
        R.check_protos(protos[c:c + 1], ex[c:c + 1, :k], f"ragged class {c}")


def test_tie_goes_to_lower_index():
    N, C, D, q = R.SHAPES[1]
    inp = R.make_inputs(1)
    protos = ops.nme_prototypes(inp["ex"].reshape(C * q, D),
                                R.seg_offsets(C, q))
    protos[1] = protos[3]  # bitwise copy
    ref = R.scores_ref(inp["x"], protos)[0]
    near = (ref.argmax(dim=1) == 1) | (ref.argmax(dim=1) == 3)
    assert near.any()
    targets = torch.full((N,), 3, dtype=torch.int64)
    idx, score, counts = ops.nme_topk(inp["x"], protos, C, targets)
    idx = idx.long()
    assert (idx[near, 0] == 1).all() and (idx[near, 1] == 3).all()
    assert torch.equal(score[near, 0], score[near, 1])
    pos1 = (idx == 1).int().argmax(dim=1)
    pos3 = (idx == 3).int().argmax(dim=1)
    assert (pos3 == pos1 + 1).all()  # everywhere, not only at the top
    assert counts[0].item() == 0 and counts[C - 1].item() == N


def test_zero_row_and_errors():
    _, C, D, q = R.SHAPES[1]
    inp = R.make_inputs(1)
    feats = inp["ex"].reshape(C * q, D)
    protos = ops.nme_prototypes(feats, R.seg_offsets(C, q))
    x = inp["x"].clone()
    x[4] = 0
    idx, score, _ = ops.nme_topk(x, protos, C)
    assert idx[4].tolist() == list(range(C)) and (score[4] == 0).all()
    off = R.seg_offsets(C, q)
    off[2] = off[1]  # class 1 holds nothing
    with pytest.raises(ValueError, match="no exemplar"):
        ops.nme_prototypes(feats, off)
    with pytest.raises(AssertionError, match="D % 4 == 0"):
        ops.nme_topk(torch.ones(3, 6), torch.ones(2, 6), 1)
    with pytest.raises(AssertionError, match="maxk"):
        ops.nme_topk(x, protos, C + 1)


def test_cli_flag():
    assert parse_args([]).nme_eval is False
    assert parse_args(["--nme_eval"]).nme_eval is True


# ------------------------------------------------------------------ CIL layer

def _tiny_setup():
    args = parse_args(["--data_set", "synthetic", "--backbone", "resnet20",
                       "--input_size", "16", "--batch_size", "8",
                       "--workers", "0", "--dtype", "fp32", "--device",
                       "cpu", "--memory_size", "12"])
    torch.manual_seed(5)
    model = CilModel("resnet20", 16)
    model.prev_model_adaption(3)
    model.prev_model_adaption(1)
    rng = np.random.default_rng(5)
    memory = RehearsalMemory(12)
    base = rng.integers(0, 256, (4, 1, 1, 3))
    for c, k in enumerate([3, 2, 3, 1]):
        noise = rng.integers(-40, 41, (k, 16, 16, 3))
        memory._x[c] = np.clip(base[c] + noise, 0, 255).astype(np.uint8)
        memory._y[c] = np.full(k, c, dtype=np.int64)
        memory._t[c] = np.zeros(k, dtype=np.int64)
    vy = np.arange(22) % 4
    vx = np.clip(base[vy] + rng.integers(-40, 41, (22, 16, 16, 3)), 0,
                 255).astype(np.uint8)
    return args, model, memory, vx, vy


@torch.no_grad()
def _features(model, args, x):
    """fp32 features in the loaders' batches of args.batch_size (a conv's
    rounding may depend on the batch it runs in)."""
    tf = EvalTransform(args, "synthetic")
    model.eval()
    t = torch.stack([tf(im) for im in x])
    f = torch.cat([model.extract_vector(t[i:i + args.batch_size]).float()
                   for i in range(0, len(t), args.batch_size)])
    model.train()
    return f


def test_cil_layer_matches_fp64_recomputation(capsys):
    args, model, memory, vx, vy = _tiny_setup()
    state = torch.get_rng_state()
    protos = build_prototypes(model, memory, "cpu", args)
    assert protos.shape == (4, model.feature_dim)
    # test-side: the same images through the same transform, then fp64
    mx, my, _ = memory.get()
    f = _features(model, args, mx)
    for c in range(4):
        R.check_protos(protos[c:c + 1], f[my == c][None], f"class {c}")

    loader = DataLoader(TaskSet(vx, vy, np.zeros(22),
                                EvalTransform(args, "synthetic")),
                        batch_size=8, shuffle=False)
    nme1, nme5 = evaluate_nme(model, protos, loader, "cpu", args)
    assert torch.equal(torch.get_rng_state(), state), "consumed torch RNG"
    assert model.training
    assert f"* NME Acc@1 {nme1:.3f} Acc@5 {nme5:.3f}" in capsys.readouterr().out
    assert nme5 == 100.0  # maxk = min(5, C) = C = 4
    # fp64 scores of the same fp32 features: a row counts for certain when
    # its target leads by more than both allowances, and cannot count when it
    # trails by more
    ref, mag, D = R.scores_ref(_features(model, args, vx), protos)
    allow = R.score_allowance(mag, D)
    t = torch.from_numpy(vy)[:, None]
    lead = ref.gather(1, t) - allow.gather(1, t)
    trail = ref.gather(1, t) + allow.gather(1, t)
    other_hi = (ref + allow).scatter(1, t, -1e9).max(dim=1, keepdim=True).values
    other_lo = (ref - allow).scatter(1, t, -1e9).max(dim=1, keepdim=True).values
    sure, possible = (lead > other_hi).sum().item(), \
        (trail >= other_lo).sum().item()
    assert sure <= round(nme1 * 22 / 100) <= possible


def test_missing_exemplars_name_memory_size():
    args, model, memory, _, _ = _tiny_setup()
    del memory._x[2], memory._y[2], memory._t[2]
    with pytest.raises(ValueError, match="--memory_size"):
        build_prototypes(model, memory, "cpu", args)


# --------------------------------------------------------------------- engine

def _engine_args(extra=()):
    return parse_args([
        "--data_set", "synthetic", "--backbone", "resnet20",
        "--synthetic_classes", "10", "--num_bases", "5", "--increment", "5",
        "--num_epochs", "1", "--batch_size", "32", "--workers", "0",
        "--synthetic_train_size", "320", "--memory_size", "20",
        "--eval_every_epoch", "0", "--input_size", "16", "--no_aug",
        "--lr", "0.05", "--seed", "3",
    ] + list(extra))


def _run(extra):
    args = _engine_args(extra)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        accs = run(args)
    return args, accs, out.getvalue()


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d_nme = tmp_path_factory.mktemp("nme")
    d_plain = tmp_path_factory.mktemp("plain")
    return dict(
        nme=_run(["--nme_eval", "--output_dir", str(d_nme)]) + (d_nme,),
        plain=_run(["--output_dir", str(d_plain)]) + (d_plain,))


def test_engine_flag_leaves_training_unchanged(runs):
    _, accs_nme, _, _ = runs["nme"]
    args_plain, accs_plain, out_plain, _ = runs["plain"]
    assert accs_nme == accs_plain and len(accs_plain) == 2
    assert "NME" not in out_plain and args_plain.nme1s == []


def test_engine_prints_and_keeps_nme(runs):
    args, _, out, _ = runs["nme"]
    assert len(re.findall(r"^\* NME Acc@1 \d+\.\d{3} Acc@5 \d+\.\d{3}$", out,
                          re.M)) == 2
    per_task = re.findall(r"^task id = (\d)  @NME1 = (\d+\.\d{5}), "
                          r"nme1s = \[(.*)\]$", out, re.M)
    assert [p[0] for p in per_task] == ["0", "1"]
    assert len(re.findall(r"^average incremental NME accuracy = \d+\.\d{5}$",
                          out, re.M)) == 1
    assert len(args.nme1s) == 2
    assert all(0.0 <= v <= 100.0 for v in args.nme1s)
    assert float(per_task[1][1]) == pytest.approx(args.nme1s[1], abs=1e-5)


def test_engine_resume_preserves_nme1s(runs):
    args, accs, _, d_nme = runs["nme"]
    r_args, r_accs, _ = _run(["--nme_eval", "--resume",
                              str(d_nme / "task_0.pth")])
    # the resumed run redoes task 1 only; task 0's figures come from the file
    assert len(r_accs) == 2 and r_accs[0] == accs[0]
    assert len(r_args.nme1s) == 2 and r_args.nme1s[0] == args.nme1s[0]
    assert 0.0 <= r_args.nme1s[1] <= 100.0


def test_engine_resume_from_checkpoint_without_key(runs):
    _, accs, _, d_plain = runs["plain"]
    ckpt = torch.load(d_plain / "task_0.pth", map_location="cpu",
                      weights_only=False)
    assert "nme1s" not in ckpt
    r_args, r_accs, out = _run(["--nme_eval", "--resume",
                                str(d_plain / "task_0.pth")])
    assert len(r_accs) == 2 and r_accs[0] == accs[0]
    assert len(r_args.nme1s) == 1  # the history starts empty, task 1 adds one
    assert "task id = 1  @NME1 = " in out
