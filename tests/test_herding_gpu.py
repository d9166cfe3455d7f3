"""``herding_kernel`` / ``herding_batch_kernel`` (csrc/loss.hip) against the
fp64 greedy reference of ``tests/_herd_ref.py`` (run on MI355X: pytest -m gpu).

A returned order is judged step by step, conditioned on its own prefix, under
the allowance derived in ``_herd_ref``; identical rows obey the exact tie
rule; and every input here has a decisive reference (gap / allowance >= 10,
asserted on the CPU in test_herding_oracle_selftest.py), so the order must
equal the reference exactly. Each test prints the largest
``(d(pick) - min) / allowance`` and the smallest reference
``gap / allowance``.
"""

import numpy as np
import pytest
import torch

import _herd_ref as R
from cilfw.cil import RehearsalMemory, herding_select

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(),
                                 reason="needs GPU")]

DEV = "cuda"


def _H():
    from cilfw.ops._backend import ext
    return ext()


def _single(f, m):
    """The raw single launch on device copies -> list."""
    fd = f.to(DEV).contiguous()
    return _H().herding_select(fd, fd.mean(0).contiguous(), m).cpu().tolist()


# --------------------------------------------------------------- single launch

@pytest.mark.parametrize("name", list(R.SINGLE_CASES))
def test_single_launch_vs_fp64(name):
    f, m, exact, ref = R.single_case(name)
    n, D = f.shape
    assert (n + D) * 4 <= 60_000
    got = herding_select(f.to(DEV), m)
    assert got.dtype == torch.int64 and got.device.type == "cuda"
    got = got.cpu().tolist()
    R.check(f, got, m, f"herding_select {name}", exact=exact, ref=ref)
    # the raw wrapper, and a rerun of it: bit-identical
    raw = _single(f, m)
    assert raw == got, "raw wrapper differs from cil.memory.herding_select"
    assert _single(f, m) == raw, "rerun differs"


def test_single_launch_m_zero_and_prefix_property():
    f, m, _, ref = R.single_case("600x8x30")
    assert _single(f, 0) == []
    assert _single(f, 7) == ref["order"][:7]
    # m above n is clamped by the caller in cil/memory.py
    f5, _, _, ref5 = R.single_case("5x3x5_all")
    assert herding_select(f5.to(DEV), 9).cpu().tolist() == ref5["order"]


# -------------------------------------------------------------- batched launch

@pytest.mark.parametrize("name", list(R.BATCH_CASES))
def test_batched_launch_vs_fp64_and_single(name):
    feats, quota, refs = R.batch_case(name)
    fd = [f.to(DEV) for f in feats]
    outs = _H().herding_select_batch(fd, [quota] * len(fd))
    assert len(outs) == len(feats)
    got = [o.cpu().tolist() for o in outs]
    for c, (f, o, ref) in enumerate(zip(feats, got, refs)):
        n = f.shape[0]
        m = min(quota, n)
        assert outs[c].dtype == torch.int64 and len(o) == m     # m clipped
        assert all(0 <= i < n for i in o), \
            f"class {c}: index outside the class (global index?): {o}"
        R.check(f, o, m, f"herding_select_batch {name} class {c} (n = {n})",
                exact=True, ref=ref)
        assert o == _single(f, m), f"class {c}: batched != single launch"
    again = _H().herding_select_batch(fd, [quota] * len(fd))
    assert [o.cpu().tolist() for o in again] == got, "rerun differs"


def test_batched_launch_per_class_quotas():
    """m_list entries may differ; each class is clipped on its own."""
    feats, _, refs = R.batch_case("D64")
    quotas = [3, 2, 0, 20, 5]
    outs = _H().herding_select_batch([f.to(DEV) for f in feats], quotas)
    for f, q, o, ref in zip(feats, quotas, outs, refs):
        m = min(q, f.shape[0])
        assert o.cpu().tolist() == ref["order"][:m]


# ------------------------------------------- RehearsalMemory, device features

def test_rehearsal_memory_with_device_features(monkeypatch):
    """Task A: one new class (single launch). Task B: three new classes of
    unequal size, one below the quota (batched launch), then every class
    shrinks to the new quota. Contents and ``last_selection`` equal the
    memory built from ``ref_order`` and a RehearsalMemory fed CPU features."""
    H = _H()
    calls = {"single": 0, "batch": 0}
    single, batch = H.herding_select, H.herding_select_batch

    def spy_single(*a, **k):
        calls["single"] += 1
        return single(*a, **k)

    def spy_batch(*a, **k):
        calls["batch"] += 1
        return batch(*a, **k)

    monkeypatch.setattr(H, "herding_select", spy_single)
    monkeypatch.setattr(H, "herding_select_batch", spy_batch)
    tasks = R.memory_tasks()
    stores, selections, gmin = R.ref_memory(tasks)
    print(f"memory scenario: min reference gap / allowance = {gmin:.4g}")
    dev = RehearsalMemory(memory_size=R.MEMORY_SIZE)
    cpu = RehearsalMemory(memory_size=R.MEMORY_SIZE)
    for step, (x, y, t, feats) in enumerate(tasks):
        dev.add(x, y, t, feats.to(DEV))
        cpu.add(x, y, t, feats)
        assert calls == [dict(single=1, batch=0),
                         dict(single=1, batch=1)][step]
        assert sorted(dev.last_selection) == sorted(selections[step])
        for c, keep in selections[step].items():
            assert np.array_equal(dev.last_selection[c], keep), \
                f"task {step} class {c}: {dev.last_selection[c].tolist()} " \
                f"vs {keep.tolist()}"
    assert dev.last_quota == 6 and len(dev) == 6 + 6 + 5 + 6
    R.check_memory(dev, selections, stores, "device features")
    R.check_memory(cpu, selections, stores, "cpu features")
    for a, b in zip(dev.get(), cpu.get()):
        assert np.array_equal(a, b)


# ------------------------------------------------------------------- refusals

class _CountingLib:
    """Stands in for ``_hip_ops._lib``: every entry point counts its calls
    and does nothing."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*a):
            self.calls.append(name)
            return 0
        return fn


def test_refusals_launch_nothing(monkeypatch):
    H = _H()
    lib = _CountingLib()
    monkeypatch.setattr(H, "_lib", lib)
    f = (R.relu_bf16(12, 8, 99) + 0.25).to(DEV)
    mu = f.mean(0)
    others = [(R.relu_bf16(n, 8, 100 + n) + 0.25).to(DEV) for n in (5, 9)]

    for bad in (float("nan"), float("inf"), -float("inf"), 2.0 ** 49):
        g = f.clone()
        g[7, 3] = bad
        with pytest.raises(ValueError, match="finite"):
            H.herding_select(g, mu, 4)
        with pytest.raises(ValueError, match="finite"):
            herding_select(g, 4)
        with pytest.raises(ValueError, match="list position 1"):
            H.herding_select_batch([others[0], g, others[1]], [4, 4, 4])
        mem = RehearsalMemory(memory_size=8)
        x = np.zeros((12, 2, 2, 3), dtype=np.uint8)
        zeros = np.zeros(12, dtype=np.int64)
        with pytest.raises(ValueError, match="finite"):
            mem.add(x, zeros, zeros, g)                       # single path
        with pytest.raises(ValueError, match="list position"):
            mem.add(x, np.arange(12) % 2, zeros, g)           # batched path
        assert mem.nb_classes == 0
    with pytest.raises(ValueError, match="finite"):
        H.herding_select(f, torch.full_like(mu, float("nan")), 4)
    for m in (13, -1):
        with pytest.raises(ValueError, match="m <= n"):
            H.herding_select(f, mu, m)
    with pytest.raises(ValueError, match="fp32"):
        H.herding_select(f.double(), mu.double(), 4)
    with pytest.raises(ValueError, match="fp32"):
        H.herding_select(f.bfloat16(), mu, 4)
    with pytest.raises(ValueError, match="contiguous"):
        H.herding_select(f.t().contiguous().t(), mu, 4)
    with pytest.raises(ValueError, match="shape"):
        H.herding_select(f, mu[:7], 4)
    with pytest.raises(ValueError, match="on the GPU"):
        H.herding_select(f.cpu(), mu.cpu(), 4)
    with pytest.raises(ValueError, match="list position 1.*width"):
        H.herding_select_batch([f, f[:, :7]], [4, 4])
    with pytest.raises(ValueError, match="list position 1.*on cpu"):
        H.herding_select_batch([f, others[0].cpu()], [4, 4])
    with pytest.raises(ValueError, match="1 quotas for 2"):
        H.herding_select_batch([f, others[0]], [4])
    with pytest.raises(AssertionError, match="n\\+D <= 15000"):
        big = torch.zeros(14_937, 64, device=DEV)
        H.herding_select(big, big[0], 3)
    with pytest.raises(AssertionError, match="LDS limit"):
        H.herding_select_batch([f, torch.zeros(14_993, 8, device=DEV)],
                               [4, 4])
    assert lib.calls == [], f"launched: {lib.calls}"
    # and the stand-in does count: valid input reaches the entry point
    H.herding_select(f, mu, 4)
    H.herding_select_batch([f, others[0]], [4, 4])
    assert lib.calls == ["cilfw_herding_select",
                         "cilfw_herding_select_batch"]
