"""The fused NME kernels (csrc/nme.hip) on the GPU against the fp64 oracle of
tests/_nme_ref.py, on all five shapes, plus the exact-tie and zero-row cases
and one --gpu_data engine run (pytest -m gpu). Inputs, allowances and the
verified properties are those of _nme_ref; no row is excluded anywhere."""

import contextlib
import io

import pytest
import torch

import _nme_ref as R
from cilfw import ops
from cilfw.config import parse_args

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(),
                                 reason="needs GPU")]

DEV = "cuda:0"
_cache = {}


def _case(shape_id):
    """Inputs (host) and device prototypes of a shape, built once."""
    if shape_id not in _cache:
        N, C, D, q = R.SHAPES[shape_id]
        inp = R.make_inputs(shape_id)
        feats = inp["ex"].reshape(C * q, D).to(DEV)
        protos = ops.nme_prototypes(feats, R.seg_offsets(C, q))
        _cache[shape_id] = (inp, feats, protos)
    return _cache[shape_id]


@pytest.mark.parametrize("shape_id", sorted(R.SHAPES))
def test_prototypes(shape_id):
    N, C, D, q = R.SHAPES[shape_id]
    inp, feats, protos = _case(shape_id)
    assert protos.shape == (C, D) and protos.dtype == torch.float32 \
        and protos.is_cuda
    R.check_protos(protos, inp["ex"], f"protos shape {shape_id}")
    again = ops.nme_prototypes(feats, R.seg_offsets(C, q))
    assert torch.equal(protos, again), "prototypes differ between launches"


@pytest.mark.parametrize("shape_id", sorted(R.SHAPES))
def test_topk(shape_id):
    N, C, D, q = R.SHAPES[shape_id]
    inp, _, protos = _case(shape_id)
    x, targets = inp["x"].to(DEV), inp["targets"].to(DEV)
    maxk = min(5, C)
    idx, score, counts = ops.nme_topk(x, protos, maxk, targets)
    assert idx.dtype == torch.int32 and idx.is_cuda
    R.check_topk(idx, score, counts, inp["x"], protos, inp["targets"], maxk,
                 f"topk shape {shape_id}")
    if N >= 3 and C > 1:
        assert 0 < counts[0].item() < N  # every third target is wrong
    idx2, score2, counts2 = ops.nme_topk(x, protos, maxk, targets)
    assert torch.equal(idx, idx2) and torch.equal(score, score2) \
        and torch.equal(counts, counts2), "top-k differs between launches"
    idx3, score3, none = ops.nme_topk(x, protos, maxk)
    assert none is None and torch.equal(idx, idx3) \
        and torch.equal(score, score3)


def test_exact_tie_goes_to_lower_index():
    N, C, D, q = R.SHAPES[1]
    inp, _, protos = _case(1)
    protos = protos.clone()
    protos[1] = protos[3]  # bitwise copy
    ref = R.scores_ref(inp["x"], protos.cpu())[0]
    near = (ref.argmax(dim=1) == 1) | (ref.argmax(dim=1) == 3)
    assert near.any()
    targets = inp["y"].clone()
    targets[near] = 3
    idx, score, counts = ops.nme_topk(inp["x"].to(DEV), protos, C,
                                      targets.to(DEV))
    R.check_topk(idx, score, counts, inp["x"], protos, targets, C, "tie")
    idx, score = idx.cpu().long(), score.cpu()
    assert (idx[near, 0] == 1).all() and (idx[near, 1] == 3).all()
    assert torch.equal(score[near, 0], score[near, 1])
    pos1 = (idx == 1).int().argmax(dim=1)
    pos3 = (idx == 3).int().argmax(dim=1)
    assert (pos3 == pos1 + 1).all()  # on every row, wherever the pair ranks


def test_zero_feature_row():
    N, C, D, q = R.SHAPES[1]
    inp, _, protos = _case(1)
    x = inp["x"].clone()
    x[4] = 0
    x[36] = 0  # the last row of the ragged tile too
    idx, score, _ = ops.nme_topk(x.to(DEV), protos, C)
    for r in (4, 36):
        assert idx[r].tolist() == list(range(C))
        assert (score[r] == 0).all()


def test_wrapper_refuses_unsupported_widths():
    with pytest.raises(AssertionError, match="D % 4 == 0"):
        ops.nme_topk(torch.ones(3, 6, device=DEV),
                     torch.ones(2, 6, device=DEV), 1)
    with pytest.raises(AssertionError, match="D % 4 == 0"):
        ops.nme_prototypes(torch.ones(3, 4100, device=DEV), [0, 3])
    with pytest.raises(ValueError, match="no exemplar"):
        ops.nme_prototypes(torch.ones(3, 8, device=DEV), [0, 3, 3])


def test_engine_gpu_data_prototypes_via_mirror(monkeypatch):
    """--gpu_data run: prototypes built from the resident DeviceReplayMirror
    are bitwise those built from the host memory (mirror=None), which proves
    the exemplar ordering of the two agrees; the NME lines are printed."""
    import cilfw.cil.nme as nme
    from cilfw.engine import run
    orig = nme.build_prototypes
    same = []

    def spy(model, memory, device, args, mirror=None):
        assert mirror is not None, "engine did not pass the resident mirror"
        p = orig(model, memory, device, args, mirror=mirror)
        host = orig(model, memory, device, args, mirror=None)
        same.append(torch.equal(p, host))
        return p

    monkeypatch.setattr(nme, "build_prototypes", spy)
    args = parse_args([
        "--data_set", "synthetic", "--backbone", "resnet20",
        "--synthetic_classes", "10", "--num_bases", "5", "--increment", "5",
        "--num_epochs", "1", "--batch_size", "32", "--workers", "0",
        "--synthetic_train_size", "640", "--memory_size", "40",
        "--eval_every_epoch", "0", "--input_size", "32", "--no_aug",
        "--lr", "0.05", "--seed", "3", "--dtype", "bf16", "--gpu_data",
        "--nme_eval"])
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        accs = run(args)
    out = out.getvalue()
    assert len(accs) == 2 and same == [True, True]
    assert out.count("* NME Acc@1 ") == 2
    assert "task id = 0  @NME1 = " in out and "task id = 1  @NME1 = " in out
    assert "average incremental NME accuracy = " in out
    assert len(args.nme1s) == 2
    assert all(0.0 <= v <= 100.0 for v in args.nme1s)
