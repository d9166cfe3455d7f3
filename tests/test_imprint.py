"""Class-mean imprinting of the new cosine head (CilModel.imprint_new_head,
engine.imprint_new_classes) on the CPU."""

import numpy as np
import pytest
import torch

from cilfw import ops
from cilfw.models import CilModel


def _model(head="cosine", nb=(4, 3)):
    torch.manual_seed(0)
    model = CilModel("resnet20", 16, head=head)
    for n in nb:
        model.prev_model_adaption(n)
    return model


def test_imprint_matches_a_direct_fp64_computation():
    model = _model()
    D = model.feature_dim
    g = torch.Generator().manual_seed(4)
    feats = torch.randn(11, D, generator=g).abs() + 0.05
    seg_off = [0, 5, 7, 11]  # three new classes
    protos = ops.nme_prototypes(feats, seg_off)
    old = [h.weight.detach().clone() for h in model.fc.heads[:-1]]
    n, norm_old = model.imprint_new_head(protos)

    f64 = feats.double()
    fh = f64 / f64.norm(dim=1, keepdim=True)
    want_norm = torch.cat(old).double().norm(dim=1).mean()
    want = []
    for a, b in zip(seg_off[:-1], seg_off[1:]):
        m = fh[a:b].mean(dim=0)
        want.append(m / m.norm() * want_norm)
    want = torch.stack(want)
    got = model.fc.heads[-1].weight.detach().double()
    assert n == 3 and abs(norm_old - want_norm.item()) <= 1e-5
    assert (got - want).abs().max().item() <= 1e-5 * want_norm.item()
    assert torch.allclose(got.norm(dim=1), want_norm.expand(3), rtol=1e-5)
    # the old heads are left alone
    assert all(torch.equal(a, h.weight)
               for a, h in zip(old, model.fc.heads[:-1]))
    assert model.fc.heads[-1].weight.requires_grad


def test_imprint_refusals():
    model = _model()
    D = model.feature_dim
    with pytest.raises(ValueError, match="prototypes for a new head"):
        model.imprint_new_head(torch.ones(4, D))
    with pytest.raises(ValueError, match="prototypes for a new head"):
        model.imprint_new_head(torch.ones(3, D + 4))
    linear = _model(head="linear")
    with pytest.raises(RuntimeError, match="cosine head"):
        linear.imprint_new_head(torch.ones(3, D))
    first = _model(nb=(4,))
    with pytest.raises(RuntimeError, match="old head"):
        first.imprint_new_head(torch.ones(4, D))


class _Set:
    def __init__(self, x, y):
        self.x, self.y = x, y
        self.t = np.zeros(len(y), np.int64)


def _args(known):
    from cilfw.config import parse_args
    args = parse_args(["--head", "cosine", "--imprint", "--device", "cpu",
                       "--dtype", "fp32", "--input_size", "16",
                       "--batch_size", "8", "--workers", "0", "--no_aug"])
    args.known_classes, args.task_id = known, 1
    return args


def test_engine_pass_skips_exemplars_and_sorts_by_label(capsys):
    """Rows of old classes (host replay exemplars) are left out; the rest is
    grouped by label whatever its order in the task set."""
    from cilfw.engine import imprint_new_classes, extract_task_features
    model = _model()
    rng = np.random.RandomState(0)
    y = np.array([5, 4, 1, 6, 4, 0, 5, 6, 6, 4, 2])
    x = rng.randint(0, 255, (len(y), 16, 16, 3)).astype(np.uint8)
    ds, args = _Set(x, y), _args(4)
    state = torch.get_rng_state()
    imprint_new_classes(model, ds, "cpu", args)
    assert torch.equal(torch.get_rng_state(), state)  # no random numbers
    assert "imprint: task 1: 3 new head rows" in capsys.readouterr().out
    feats = extract_task_features(model, ds, "cpu", args)
    want = ops.nme_prototypes(
        torch.cat([feats[y == c] for c in (4, 5, 6)]), [0, 3, 5, 8])
    norm_old = model.fc.heads[0].weight.norm(dim=1).mean()
    assert torch.allclose(model.fc.heads[-1].weight, want * norm_old,
                          rtol=1e-5, atol=1e-7)


def test_empty_new_class_surfaces_the_nme_error():
    from cilfw.engine import imprint_new_classes
    model = _model()
    y = np.array([4, 4, 6, 1])  # class 5 has no sample
    x = np.zeros((len(y), 16, 16, 3), np.uint8)
    with pytest.raises(ValueError, match="hold no exemplar"):
        imprint_new_classes(model, _Set(x, y), "cpu", _args(4))
