"""K-means proxy initialisation on the CPU: CilModel.init_new_proxies,
the --proxy_init / --kmeans_iters flags, engine.init_new_proxies_kmeans and
engine runs with --proxy_init kmeans (the kernel's oracle is
test_kmeans_oracle_selftest.py / test_kmeans_gpu.py)."""

import contextlib
import io
import os
import re

import numpy as np
import pytest
import torch

import cilfw.engine as E
from cilfw import ops
from cilfw.config import check_args, get_args_parser, parse_args
from cilfw.engine import run
from cilfw.models import CilModel


def _model(head="cosine", nb=(4, 3), nb_proxy=3):
    torch.manual_seed(0)
    model = CilModel("resnet20", 16, head=head, nb_proxy=nb_proxy)
    for n in nb:
        model.prev_model_adaption(n)
    return model


def test_init_matches_a_direct_fp64_computation():
    model = _model()
    D = model.feature_dim
    g = torch.Generator().manual_seed(4)
    proxies = torch.randn(9, D, generator=g)
    proxies = proxies / proxies.norm(dim=1, keepdim=True)
    old = [h.weight.detach().clone() for h in model.fc.heads[:-1]]
    n, norm_old = model.init_new_proxies(proxies)
    want_norm = torch.cat(old).double().norm(dim=1).mean()
    got = model.fc.heads[-1].weight.detach().double()
    assert n == 9 and abs(norm_old - want_norm.item()) <= 1e-5
    assert (got - proxies.double() * want_norm).abs().max().item() \
        <= 1e-5 * want_norm.item()
    assert torch.allclose(got.norm(dim=1), want_norm.expand(9), rtol=1e-5)
    assert all(torch.equal(a, h.weight)
               for a, h in zip(old, model.fc.heads[:-1]))
    assert model.fc.heads[-1].weight.requires_grad


def test_init_refusals():
    model = _model()
    D = model.feature_dim
    with pytest.raises(ValueError, match="proxies for a new head"):
        model.init_new_proxies(torch.ones(3, D))       # classes, not rows
    with pytest.raises(ValueError, match="proxies for a new head"):
        model.init_new_proxies(torch.ones(9, D + 4))
    linear = _model(head="linear", nb_proxy=1)
    with pytest.raises(RuntimeError, match="cosine head"):
        linear.init_new_proxies(torch.ones(3, D))
    first = _model(nb=(4,))
    with pytest.raises(RuntimeError, match="old head"):
        first.init_new_proxies(torch.ones(12, D))
    single = _model(nb_proxy=1)
    with pytest.raises(RuntimeError, match="imprint_new_head"):
        single.init_new_proxies(torch.ones(3, D))
    # and imprinting still refuses the multi-proxy head
    with pytest.raises(RuntimeError, match="nb_proxy > 1"):
        model.imprint_new_head(torch.ones(9, D))


def test_cli_flags_and_refusals(capsys):
    a = parse_args([])
    assert a.proxy_init == "random" and a.kmeans_iters == 100
    a = parse_args(["--head", "cosine", "--nb_proxy", "10", "--proxy_init",
                    "kmeans", "--kmeans_iters", "7"])
    assert a.proxy_init == "kmeans" and a.kmeans_iters == 7
    for argv, words in (
            (["--proxy_init", "kmeans"], "--head cosine"),
            (["--head", "cosine", "--proxy_init", "kmeans"], "--nb_proxy > 1"),
            (["--head", "cosine", "--nb_proxy", "3", "--proxy_init", "kmeans",
              "--kmeans_iters", "0"], "--kmeans_iters"),
            (["--head", "cosine", "--nb_proxy", "3", "--imprint"],
             "--imprint")):
        args = get_args_parser().parse_args(argv)
        with pytest.raises(ValueError, match=words):
            check_args(args)
    with pytest.raises(SystemExit):
        parse_args(["--proxy_init", "kmeans++"])
    capsys.readouterr()
    text = re.sub(r"\s+", " ", get_args_parser().format_help())
    assert "--proxy_init" in text and "--kmeans_iters" in text


class _Set:
    def __init__(self, x, y):
        self.x, self.y = x, y
        self.t = np.zeros(len(y), np.int64)


def _args(known, extra=()):
    args = parse_args(["--head", "cosine", "--nb_proxy", "3", "--proxy_init",
                       "kmeans", "--device", "cpu", "--dtype", "fp32",
                       "--input_size", "16", "--batch_size", "8",
                       "--workers", "0", "--no_aug", *extra])
    args.known_classes, args.task_id = known, 1
    return args


def test_engine_pass_sets_every_row_to_a_centre_of_its_class(capsys):
    model = _model()
    rng = np.random.RandomState(0)
    y = np.array([5, 4, 1, 6, 4, 0, 5, 6, 6, 4, 2, 5, 6, 4, 5, 4, 6, 5])
    x = rng.randint(0, 255, (len(y), 16, 16, 3)).astype(np.uint8)
    ds, args = _Set(x, y), _args(4)
    old = [h.weight.detach().clone() for h in model.fc.heads[:-1]]
    state = torch.get_rng_state()
    E.init_new_proxies_kmeans(model, ds, "cpu", args)
    assert torch.equal(torch.get_rng_state(), state)  # no random numbers
    out = capsys.readouterr().out
    m = re.search(r"^proxy init: task 1: 9 new head rows set to k-means "
                  r"centres, mean old norm (\S+), iterations (\d+)\.\.(\d+)$",
                  out, re.M)
    assert m, out
    assert all(torch.equal(a, h.weight)
               for a, h in zip(old, model.fc.heads[:-1]))
    norm_old = torch.cat(old).norm(dim=1).mean()
    assert abs(float(m.group(1)) - norm_old.item()) <= 1e-4
    new = model.fc.heads[-1].weight.detach()
    assert torch.allclose(new.norm(dim=1), norm_old.expand(9), rtol=1e-5)
    feats = E.extract_task_features(model, ds, "cpu", args)
    for j, c in enumerate((4, 5, 6)):
        fc = feats[y == c]
        want, _, iters = ops.kmeans_proxies(fc, [0, fc.shape[0]], 3)
        assert int(m.group(2)) <= iters.item() <= int(m.group(3))
        assert torch.allclose(new[3 * j:3 * j + 3], want * norm_old,
                              rtol=1e-5, atol=1e-7), f"class {c}"


def test_too_small_class_surfaces_the_op_error():
    model = _model()
    y = np.array([4, 4, 4, 5, 5, 5, 6, 6, 1])  # class 6: two rows, K = 3
    x = np.zeros((len(y), 16, 16, 3), np.uint8)
    with pytest.raises(ValueError, match=r"segment\(s\) \[2\] hold fewer"):
        E.init_new_proxies_kmeans(model, _Set(x, y), "cpu", _args(4))


BASE = ["--data_set", "synthetic", "--backbone", "resnet20",
        "--synthetic_classes", "10", "--num_bases", "5", "--increment", "5",
        "--num_epochs", "1", "--batch_size", "32", "--workers", "0",
        "--synthetic_train_size", "320", "--memory_size", "20",
        "--eval_every_epoch", "0", "--input_size", "16", "--no_aug",
        "--lr", "0.05", "--seed", "3", "--dtype", "fp32", "--device", "cpu"]
PODNET = ["--head", "cosine", "--nb_proxy", "3", "--cls_loss", "nca",
          "--lambda_kd", "0", "--lambda_flat", "1"]
KMEANS = PODNET + ["--proxy_init", "kmeans"]


def _run(extra):
    args = parse_args(BASE + list(extra))
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        accs = run(args)
    return accs, out.getvalue()


def _lines(out):
    keep = re.findall(r"^(?:task \d+ epoch \d+|proxy init): .*$", out, re.M)
    return [re.sub(r"imgs/s \d+", "", v) for v in keep]


@pytest.fixture(scope="module")
def kmeans_run(tmp_path_factory):
    d = tmp_path_factory.mktemp("kmeans_ckpt")
    return (str(d),) + _run(KMEANS + ["--output_dir", str(d)])


def test_engine_run_with_kmeans_init(kmeans_run):
    _, accs, out = kmeans_run
    assert len(accs) == 2
    lines = _lines(out)
    assert len(lines) == 3 and lines[1].startswith(
        "proxy init: task 1: 15 new head rows set to k-means centres")
    # the initialisation is in effect: task 1 differs from the random start
    accs_r, out_r = _run(PODNET)
    rand = _lines(out_r)
    assert len(rand) == 2 and rand[0] == lines[0] and rand[1] != lines[2]


def test_engine_run_repeats_and_resumes(kmeans_run):
    d, accs, out = kmeans_run
    accs2, out2 = _run(KMEANS)
    assert accs2 == accs and _lines(out2) == _lines(out)
    accs3, out3 = _run(KMEANS + ["--resume", os.path.join(d, "task_0.pth")])
    assert "resumed from" in out3
    assert len(accs3) == 2 and accs3 == accs
    assert _lines(out3) == _lines(out)[1:]


def test_default_flags_launch_nothing_new(monkeypatch):
    """Without --proxy_init kmeans neither the op nor the extra feature pass
    runs, and the run equals, on this same code, one that spells the default
    out; that the default path computes what it computed before is shown by
    the existing suite passing unchanged."""
    calls = []
    orig_op, orig_pass = ops.kmeans_proxies, E.init_new_proxies_kmeans
    monkeypatch.setattr(ops, "kmeans_proxies", lambda *a, **k: (
        calls.append("op"), orig_op(*a, **k))[1])
    monkeypatch.setattr(E, "init_new_proxies_kmeans", lambda *a, **k: (
        calls.append("pass"), orig_pass(*a, **k))[1])
    accs, out = _run(PODNET)
    accs2, out2 = _run(PODNET + ["--proxy_init", "random", "--kmeans_iters",
                                 "100"])
    assert calls == []
    assert accs == accs2 and _lines(out) == _lines(out2)
    assert "proxy init" not in out
    # and the spies do see the pass when it runs
    _run(KMEANS)
    assert calls == ["pass", "op"]
