"""The k-means oracle judged on the CPU (tests/_kmeans_ref.py): every input
of test_kmeans_gpu.py has a decisive fp64 reference (gap / allowance >= 10 at
every seeding step and every assignment of every pass), the project's CPU
path is accepted at every shape, and each seeded fault of the fp32 kernel
model is rejected on an input built to show it."""

import numpy as np
import pytest
import torch

import _kmeans_ref as R
from cilfw import ops


@pytest.mark.parametrize("name", list(R.CASES))
def test_reference_is_decisive_by_a_factor_ten(name):
    f, sizes, K, max_iter, refs = R.case(name)
    for c, r in enumerate(refs):
        print(f"{name} class {c} (n = {sizes[c]}): min seeding gap / "
              f"allowance = {r['seed_ratio'].min():.4g}, min assignment gap "
              f"/ allowance = {r['assign_ratio']:.4g}, iters = {r['iters']}")
        assert r["seed_ratio"].min() >= 10.0
        assert r["assign_ratio"] >= 10.0
        assert 1 <= r["iters"] <= max_iter


@pytest.mark.parametrize("name", list(R.CASES))
def test_cpu_path_and_model_are_accepted(name):
    f, sizes, K, max_iter, refs = R.case(name)
    out = ops.kmeans_proxies(f, R.seg_offsets(sizes), K, max_iter)
    R.check(refs, sizes, K, out, f"cpu path {name}")
    assert (out[0].double().norm(dim=1) - 1).abs().max().item() <= 1e-6
    R.check(refs, sizes, K, R.model(f, sizes, K, max_iter),
            f"fp32 model {name}")


def test_case_properties():
    """What the inputs were built for is really in them."""
    dup = R.case("48x16x4_dup")
    f, r = dup[0], dup[4][0]
    groups = {}
    for i in range(f.shape[0]):
        groups.setdefault(f[i].numpy().tobytes(), []).append(i)
    copies = sorted(g for g in groups.values() if len(g) == 3)
    assert len(copies) == 2
    # the original of each group is the lowest index and is a seed
    assert sorted(g[0] for g in copies) == sorted([r["seeds"][0],
                                                   r["seeds"][2]])
    emp = R.case("3x4x3_dup_empty")[4][0]
    assert emp["emptied"] and emp["seeds"] == [0, 2, 0] \
        and emp["assign"].tolist() == [0, 0, 1] and emp["iters"] == 2
    assert [r["iters"] for r in R.case("5x4x5")[4]] == [1]
    assert [r["iters"] for r in R.case("iter1")[4]] == [1, 1, 1, 1]
    full = [r["iters"] for r in R.case("batch_D64_K7")[4]]
    assert max(full) >= 3
    assert [r["iters"] for r in R.case("iter2")[4]] == [min(i, 2)
                                                        for i in full]


# fault -> (case that shows it, keyword arguments of R.model)
FAULTS = {
    "ties_to_the_higher_row": ("3x4x3_dup_empty", dict(tie_high_row=True)),
    "ties_to_the_higher_centre": ("3x4x3_dup_empty",
                                  dict(tie_high_centre=True)),
    "seeding_from_row_0": ("batch_D64_K10", dict(seed_row0=True)),
    "emptied_centre_reset_to_zero": ("3x4x3_dup_empty",
                                     dict(empty_zero=True)),
    "first_256_columns_only": ("D300_K6", dict(cols=256)),
    "first_4_rows_only": ("batch_D64_K7", dict(rows=4)),
    "global_assign": ("batch_D64_K10", dict(global_assign=True)),
    "neighbouring_segment": ("D300_K6", dict(seg_shift=40)),
    "unnormalised_output": ("64x1000x16", dict(unnormalised=True)),
    "one_iteration_too_few": ("batch_D64_K7", dict(one_short=True)),
}


@pytest.mark.parametrize("fault", list(FAULTS))
def test_seeded_fault_is_rejected(fault):
    name, kw = FAULTS[fault]
    f, sizes, K, max_iter, refs = R.case(name)
    assert R.verdict(refs, sizes, K, *R.model(f, sizes, K, max_iter))[0] \
        is None
    why, _ = R.verdict(refs, sizes, K, *R.model(f, sizes, K, max_iter, **kw))
    print(f"{fault} on {name}: {why}")
    assert why is not None


def test_verdict_rejects_wrong_shapes_and_dtypes():
    f, sizes, K, max_iter, refs = R.case("5x4x5")
    p, a, i = R.model(f, sizes, K, max_iter)
    assert R.verdict(refs, sizes, K, p[:-1], a, i)[0] is not None
    assert R.verdict(refs, sizes, K, p, a.long(), i)[0] is not None
    assert R.verdict(refs, sizes, K, p, a, i.long())[0] is not None
    q = p.clone()
    q[0, 0] = float("nan")
    assert R.verdict(refs, sizes, K, q, a, i)[0] is not None


def test_refusals():
    f = R.blobs(24, 8, 3, 77)
    off = [0, 10, 24]
    with pytest.raises(ValueError, match=r"segment\(s\) \[0\] hold fewer"):
        ops.kmeans_proxies(f, off, 11)
    with pytest.raises(ValueError, match=r"segment\(s\) \[0, 1\] hold fewer"):
        ops.kmeans_proxies(f, off, 16)
    for bad in (float("nan"), float("inf"), -float("inf")):
        g = f.clone()
        g[13, 5] = bad
        with pytest.raises(ValueError, match="finite"):
            ops.kmeans_proxies(g, off, 3)
    with pytest.raises(ValueError, match="unsupported shape"):
        ops.kmeans_proxies(f[:, :6], off, 3)                 # D % 4
    with pytest.raises(ValueError, match="unsupported shape"):
        ops.kmeans_proxies(torch.ones(32, 1004), [0, 32], 16)  # K D > 16000
    with pytest.raises(ValueError, match="unsupported shape"):
        ops.kmeans_proxies(torch.ones(8, 4100), [0, 8], 2)   # D > 4096
    with pytest.raises(ValueError, match="nb_proxy must be"):
        ops.kmeans_proxies(f, off, 17)
    with pytest.raises(ValueError, match="nb_proxy must be"):
        ops.kmeans_proxies(f, off, 0)
    with pytest.raises(ValueError, match="max_iter"):
        ops.kmeans_proxies(f, off, 3, max_iter=0)
    with pytest.raises(AssertionError, match="seg_off"):
        ops.kmeans_proxies(f, [0, 10, 23], 3)
    # the limit itself is accepted
    p, a, i = ops.kmeans_proxies(torch.rand(16, 1000) + 0.1, [0, 16], 16)
    assert p.shape == (16, 1000) and i.tolist() == [1]
