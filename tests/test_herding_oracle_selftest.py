"""CPU self-test of the herding oracle in ``tests/_herd_ref.py``.

The comparator must accept the project's CPU path (``cil.memory.
herding_select``, fp32 torch) and an fp32 numpy model of the kernel at every
input of test_herding_gpu.py, show that every input on which the GPU test
demands the reference's exact order has ``gap / allowance >= 10``, and reject
nine seeded faults simulated on the CPU. The input refusals that need no GPU
are checked here too. No GPU involved.
"""

import numpy as np
import pytest
import torch

import _herd_ref as R
from cilfw import _herding_checks as HC
from cilfw.cil import RehearsalMemory, herding_select

SINGLE = list(R.SINGLE_CASES)
BATCH = list(R.BATCH_CASES)


def _rejected(f, order, m, what, distance_fault=True):
    """The comparator rejects ``order``; a fault that changes a distance
    must show at its worst step by more than 10 allowances."""
    n = f.shape[0]
    why, worst = R.verdict(f, order, m)
    assert why is not None, f"{what}: accepted (worst {worst:.3g})"
    if R.structure_error(order, n, m) is None and distance_fault:
        r = R.step_ratios(f, order)
        k = int(np.argmax(r))
        assert r[k] > 10.0, f"{what}: step {k} only {r[k]:.3g} allowances"
        print(f"{what}: first rejected at step {int(np.argmax(r > 1.0))}, "
              f"worst step {k} by {r[k]:.4g} allowances")
    else:
        print(f"{what}: rejected ({why})")
    return why


# ----------------------------------------------------- accepted, and decisive

@pytest.mark.parametrize("name", SINGLE)
def test_cpu_path_and_kernel_model_accepted(name):
    f, m, exact, ref = R.single_case(name)
    got = herding_select(f, m).tolist()
    R.check(f, got, m, f"{name} cpu path", exact=exact, ref=ref)
    R.check(f, R.kernel_model(f, m), m, f"{name} fp32 model", exact=exact,
            ref=ref)
    assert R.verdict(f, ref["order"], m, exact=exact, ref=ref)[0] is None


@pytest.mark.parametrize("name", SINGLE)
def test_exact_order_inputs_are_decisive(name):
    f, m, exact, ref = R.single_case(name)
    ratio = float(ref["ratio"].min())
    print(f"{name}: min gap / allowance = {ratio:.4g}, smallest literal gap "
          f"{ref['gap'].min():.3g}")
    assert exact, "every single-launch input demands the exact order"
    assert ratio >= 10.0


@pytest.mark.parametrize("name", BATCH)
def test_batch_inputs_accepted_and_decisive(name):
    feats, quota, refs = R.batch_case(name)
    for c, (f, ref) in enumerate(zip(feats, refs)):
        m = min(quota, f.shape[0])
        ratio = float(ref["ratio"].min())
        print(f"{name} class {c} (n = {f.shape[0]}): min gap / allowance = "
              f"{ratio:.4g}")
        assert ratio >= 10.0
        R.check(f, herding_select(f, quota).tolist(), m,
                f"{name} class {c} cpu path", exact=True, ref=ref)
    for c, o in enumerate(R.batch_model(feats, quota)):
        R.check(feats[c], o, len(refs[c]["order"]),
                f"{name} class {c} fp32 model", exact=True, ref=refs[c])


def test_inputs_reach_the_edges_they_are_meant_for():
    """Asserted on the reference, as the GPU test relies on it."""
    f, m, _, ref = R.single_case("257x64x20")
    assert ref["order"][0] == 256           # winner in the second trip
    _, _, _, ref = R.single_case("600x8x30")
    assert any(256 <= i < 512 for i in ref["order"])
    assert any(i >= 512 for i in ref["order"])
    for name, groups in R.DUP_GROUPS.items():
        f, m, _, ref = R.single_case(name)
        for grp in groups:
            assert all(torch.equal(f[grp[0]], f[i]) for i in grp)
            picked = [i for i in ref["order"] if i in grp]
            assert picked == grp, (name, grp, picked)   # all, ascending
    feats, quota, refs = R.batch_case("D64")
    assert [len(r["order"]) for r in refs] == [1, 7, 20, 20, 20]
    assert any(i >= 512 for i in refs[4]["order"])
    # a global index would leave its class (D64: offset 521 + pick >= 600)
    for name in BATCH:
        feats, quota, refs = R.batch_case(name)
        offs = np.cumsum([0] + [f.shape[0] for f in feats])
        assert any(max(r["order"]) + offs[c] >= feats[c].shape[0]
                   for c, r in enumerate(refs) if c > 0), name
    assert (14900 + 64) * 4 == 59_856 <= HC.LDS_BYTES


# -------------------------------------------------------------- seeded faults

@pytest.mark.parametrize("name", list(R.DUP_GROUPS))
def test_fault_higher_index_wins_tie(name):
    f, m, _, _ = R.single_case(name)
    bad = R.kernel_model(f, m, tie_high=True)
    assert R.structure_error(bad, f.shape[0], m) is None
    assert R.step_ratios(f, bad).max() <= 1.0    # the distances cannot tell
    why = _rejected(f, bad, m, f"{name} tie to the higher index",
                    distance_fault=False)
    assert "identical rows" in why


def test_fault_higher_index_wins_tie_batched():
    feats, quota, refs = R.batch_case("D16_dup")
    for c, o in enumerate(R.batch_model(feats, quota, tie_high=True)):
        why = R.verdict(feats[c], o, quota)[0]
        assert why is not None and "identical rows" in why, (c, why)


@pytest.mark.parametrize("name", ["257x64x20", "64x16x12_dup",
                                  "320x16x12_dup"])
def test_fault_selected_flag_ignored(name):
    f, m, _, _ = R.single_case(name)
    bad = R.kernel_model(f, m, honour_selected=False)
    assert len(set(bad)) < m, "the input does not make this fault repeat"
    why = _rejected(f, bad, m, f"{name} selected flag ignored")
    assert "repeated" in why


@pytest.mark.parametrize("name", ["257x64x20", "600x8x30", "300x300x6",
                                  "130x2048x4", "14900x64x3",
                                  "200x64x50_randn", "64x16x12_dup"])
@pytest.mark.parametrize("fault", ["sum_not_updated", "plain_sort", "no_inv"])
def test_fault_in_the_running_mean(name, fault):
    f, m, _, _ = R.single_case(name)
    kw = dict(sum_not_updated=dict(update_sum=False),
              plain_sort=dict(update_sum=False, use_inv=False),
              no_inv=dict(use_inv=False))[fault]
    _rejected(f, R.kernel_model(f, m, **kw), m, f"{name} {fault}")


@pytest.mark.parametrize("name", ["257x64x20", "600x8x30", "14900x64x3",
                                  "320x16x12_dup"])
def test_fault_first_256_candidates_only(name):
    f, m, _, _ = R.single_case(name)
    bad = R.kernel_model(f, m, scan=256)
    assert all(i < 256 for i in bad)
    _rejected(f, bad, m, f"{name} candidates < 256 only")


@pytest.mark.parametrize("name", ["300x300x6", "130x2048x4"])
def test_fault_sum_sel_first_256_coordinates_only(name):
    f, m, _, _ = R.single_case(name)
    _rejected(f, R.kernel_model(f, m, sum_cols=256), m,
              f"{name} sum_sel over 256 coordinates only")


@pytest.mark.parametrize("name", BATCH)
@pytest.mark.parametrize("fault", ["neighbour_mean", "row_shift",
                                   "global_index"])
def test_fault_in_the_batched_launch(name, fault):
    feats, quota, refs = R.batch_case(name)
    kw = dict(neighbour_mean=dict(mean_shift=1), row_shift=dict(row_shift=1),
              global_index=dict(global_idx=True))[fault]
    orders = R.batch_model(feats, quota, **kw)
    rejected = []
    for c, (f, o) in enumerate(zip(feats, orders)):
        m = min(quota, f.shape[0])
        why, worst = R.verdict(f, o, m, exact=True, ref=refs[c])
        if why is None:
            continue
        rejected.append(c)
        if R.structure_error(o, f.shape[0], m) is None:
            # a distance fault: more than 10 allowances at its worst step
            r = R.step_ratios(f, o)
            if (r > 1.0).any():
                assert r.max() > 10.0, (name, fault, c, r.max())
        print(f"{name} {fault} class {c}: {why}")
    if fault == "global_index":
        # class 0 has offset 0 and cannot show it; a later class must leave
        # its range
        assert any("outside" in R.verdict(feats[c], orders[c],
                                          min(quota, feats[c].shape[0]))[0]
                   for c in rejected)
    else:
        # every class with more candidates than picks shows it (a class that
        # is taken whole returns the same set in whatever order its distances
        # give; n = 1 has one possible answer)
        need = [c for c, f in enumerate(feats) if f.shape[0] > 1]
        assert set(need) <= set(rejected), (need, rejected)


# ---------------------------------------- what the older objective check sees

def _objective_check_accepts(f, got, want):
    """test_ops_gpu.py::test_herding_gpu_matches_cpu's assertions, applied
    to two orders on the CPU."""
    mu = f.mean(0)

    def objective(order):
        sel = f[order]
        means = sel.cumsum(0) / torch.arange(1, len(order) + 1).unsqueeze(1)
        return (means - mu).norm(dim=1)

    og, ow = objective(got), objective(want)
    return bool(torch.allclose(og, ow, rtol=1e-3, atol=1e-4)) \
        and got[0] == want[0]


def test_what_the_objective_check_accepts():
    """On that test's own input (seed 18, (200, 64), m = 50) its prefix
    objective at rtol 1e-3 cannot see: the tie-break (no ties in randn), the
    candidate and ``sum_sel`` strides (n, D < 256), and a late pick swapped
    for one within 1e-3 - each of which the new comparator, on the inputs
    above, rejects. The faults that move the running mean are caught by
    both."""
    torch.manual_seed(18)
    f = torch.randn(200, 64)
    m = 50
    want = herding_select(f, m).tolist()
    faults = {
        "tie_high": dict(tie_high=True),
        "selected_ignored": dict(honour_selected=False),
        "sum_not_updated": dict(update_sum=False),
        "no_inv": dict(use_inv=False),
        "scan_256": dict(scan=256),
        "sum_cols_256": dict(sum_cols=256),
    }
    accepted = {k for k, kw in faults.items()
                if _objective_check_accepts(f, R.kernel_model(f, m, **kw),
                                            want)}
    print("objective check accepts:", sorted(accepted))
    assert accepted == {"tie_high", "scan_256", "sum_cols_256"}
    # a wrong pick at rank >= 2: cut the run after step k and hand the step to
    # another candidate whose prefix objective is within the check's 1e-3.
    # The check accepts it; the comparator, whose allowance is what fp32 can
    # really confuse, does not.
    st = R._Stepper(f)
    found = []
    for k in range(m):
        d, tol = st.dist_tol()
        d[st.sel] = np.inf
        a = int(np.argmin(d))
        near = np.flatnonzero(
            (np.sqrt(d) - np.sqrt(d[a]) <= 0.9 * (1e-4 + 1e-3 * np.sqrt(d[a])))
            & (d - d[a] > 1.5 * (tol + tol[a])))
        for j in near:
            swapped = want[:k] + [int(j)]
            assert _objective_check_accepts(f, swapped, want[:k + 1]) \
                == (k > 0)        # step 0 is guarded by the first-pick check
            assert R.verdict(f, swapped, k + 1)[0] is not None
            found.append((k, int(j)))
        st.take(want[k])
    print("wrong picks the objective check accepts (step, index):", found)
    assert any(k >= 2 for k, _ in found)


# ------------------------------------------------------- RehearsalMemory, CPU

def test_memory_with_cpu_features_matches_reference():
    tasks = R.memory_tasks()
    stores, selections, gmin = R.ref_memory(tasks)
    print(f"memory scenario: min gap / allowance = {gmin:.4g}")
    assert gmin >= 10.0
    mem = RehearsalMemory(memory_size=R.MEMORY_SIZE)
    for x, y, t, feats in tasks:
        mem.add(x, y, t, feats)
    assert mem.last_quota == 6 and len(mem) == 6 + 6 + 5 + 6
    R.check_memory(mem, selections, stores, "cpu features")


# ------------------------------------------------------------------- refusals

def _feat(n=6, D=4):
    return R.relu_bf16(n, D, 77) + 0.25


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf"),
                                 2.0 ** 49, -2.0 ** 49])
def test_cpu_path_refuses_bad_features(bad):
    f = _feat()
    f[4, 2] = bad
    with pytest.raises(ValueError, match="finite"):
        herding_select(f, 3)
    with pytest.raises(ValueError, match="finite"):
        herding_select(f.double(), 3)
    x = np.zeros((6, 2, 2, 3), dtype=np.uint8)
    mem = RehearsalMemory(memory_size=4)
    with pytest.raises(ValueError, match="finite"):
        mem.add(x, np.zeros(6, dtype=np.int64), np.zeros(6, dtype=np.int64),
                f)
    assert mem.nb_classes == 0


def test_cpu_path_refuses_fp64_overflowing_fp32():
    f = _feat().double()
    f[0, 0] = 1e300                  # inf once cast to fp32
    with pytest.raises(ValueError, match="finite"):
        herding_select(f, 2)


def test_value_check_names_the_class_position():
    fs = [_feat(), _feat(5), _feat(7)]
    fs[2][3, 1] = float("nan")
    with pytest.raises(ValueError, match="list position 2"):
        HC.check_values_batch(torch.cat(fs), [6, 5, 7], "batch")
    HC.check_values_batch(torch.cat(fs[:2]), [6, 5], "batch")
    HC.check_values("single", fs[0], fs[1])
    with pytest.raises(ValueError, match="finite"):
        HC.check_values("single", fs[0], fs[2])
    HC.check_values("empty", torch.empty(0, 4))


def test_raw_wrapper_argument_checks():
    f = _feat()
    mu = f.mean(0)
    assert HC.check_select_args(f, mu, 6) == (6, 4, 6)
    assert HC.check_select_args(f, mu, 0) == (6, 4, 0)
    for m in (7, -1):
        with pytest.raises(ValueError, match="m <= n"):
            HC.check_select_args(f, mu, m)
    with pytest.raises(ValueError, match="fp32"):
        HC.check_select_args(f.double(), mu.double(), 3)
    with pytest.raises(ValueError, match="fp32"):
        HC.check_select_args(f.bfloat16(), mu, 3)
    with pytest.raises(ValueError, match="contiguous"):
        HC.check_select_args(f.t().contiguous().t(), mu, 3)
    with pytest.raises(ValueError, match="contiguous"):
        HC.check_select_args(_feat(6, 8)[:, ::2], mu, 3)
    with pytest.raises(ValueError, match="2-d"):
        HC.check_select_args(f.reshape(-1), mu, 3)
    with pytest.raises(ValueError, match="shape"):
        HC.check_select_args(f, mu[:3], 3)
    with pytest.raises(ValueError, match="shape"):
        HC.check_select_args(f, mu.unsqueeze(0), 3)
    with pytest.raises(ValueError, match="mu must be"):
        HC.check_select_args(f, mu.double(), 3)


def test_batch_wrapper_argument_checks():
    fs = [_feat(), _feat(5), _feat(7)]
    assert HC.check_batch_args(fs, [3, 9, 2]) == ([6, 5, 7], 4, fs[0].device)
    with pytest.raises(ValueError, match="2 quotas for 3"):
        HC.check_batch_args(fs, [3, 3])
    with pytest.raises(ValueError, match="list position 1.*width"):
        HC.check_batch_args([fs[0], _feat(5, 3), fs[2]], [3, 3, 3])
    with pytest.raises(ValueError, match="list position 2.*2-d"):
        HC.check_batch_args([fs[0], fs[1], fs[2].reshape(-1)], [3, 3, 3])
    with pytest.raises(ValueError, match="list position 1.*negative"):
        HC.check_batch_args(fs, [3, -1, 3])
    with pytest.raises(ValueError, match="list position 0.*floating"):
        HC.check_batch_args([fs[0].long(), fs[1]], [3, 3])
    with pytest.raises(ValueError, match="empty"):
        HC.check_batch_args([], [])
    meta = _feat(5).to("meta")
    with pytest.raises(ValueError, match="list position 1.*on meta"):
        HC.check_batch_args([fs[0], meta], [3, 3])


def test_scale_2_pow_48_is_accepted_and_exact():
    """Valid input at exactly the bound: max|f| = 2^48."""
    f = R.relu_bf16(12, 5, 4812).clamp(max=2.0)
    f[7, 3] = 2.0
    f = f * 2.0 ** 47
    assert f.abs().max().item() == HC.HERDING_MAX_ABS
    m = 6
    ref = R.ref_order(f, m)
    ratio = float(ref["ratio"].min())
    print(f"2^48 scale: min gap / allowance = {ratio:.4g}")
    assert ratio >= 10.0
    R.check(f, herding_select(f, m).tolist(), m, "2^48 scale cpu path",
            exact=True, ref=ref)
    R.check(f, R.kernel_model(f, m), m, "2^48 scale fp32 model", exact=True,
            ref=ref)
    f[0, 0] = 2.0 ** 48 * (1 + 2.0 ** -23)      # one ulp above the bound
    with pytest.raises(ValueError, match="finite"):
        herding_select(f, m)
