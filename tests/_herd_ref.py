"""fp64 reference, step-wise comparator and test inputs for the herding
kernels ``herding_kernel`` / ``herding_batch_kernel`` of csrc/loss.hip
(tests/test_herding_gpu.py, tests/test_herding_oracle_selftest.py).

The kernels return a ranked list of indices, not floats: at step k they take

    argmin_i d_k(i),  d_k(i) = sum_d t_d^2,
    t_d = (S_d + f_i[d]) / (k + 1) - mu_d,   S = sum of the rows picked so far,

over the rows not picked yet, the lowest index on exact ties. Two correct
implementations may differ where two candidates are closer than fp32 can
tell, and from then on their prefixes differ, so an order is judged step by
step CONDITIONED ON ITS OWN PREFIX:

* every entry lies in [0, n), no entry repeats, the length is m;
* at step k, with S the fp64 sum of ``f[order[:k]]`` and d_k in fp64 (mu the
  fp64 mean),  d_k(order[k]) <= min_i d_k(i) + tol_k(order[k]) + tol_k(argmin).
  A kernel that evaluates every d_k(i) within tol_k(i) and takes its own
  minimum satisfies this; one that takes a candidate further away does not.

Allowance tol_k(i)
------------------
Counted from the kernel's fp32 arithmetic; nothing is fitted to its output.
``u = 2^-24`` is the unit roundoff, ``g(j) = j u / (1 - j u)`` bounds j
successive roundings (and a sum of j + 1 terms in any order, against the sum
of the magnitudes). Per coordinate d the kernel forms

    t^ = fl(fl(fl(s^ + f) * inv^) - mu^)

* ``s^`` is the running fp32 sum of the k picked rows (``sum_sel``, one add
  per pick, the first onto zero): at most k roundings, each relative to the
  partial sums, which ``A_d = sum_{j<k} |f_pick_j[d]|`` bounds.
* ``s^ + f`` rounds once more; ``inv^ = fl(1 / (k + 1))`` carries one
  rounding and the product another. Together
  ``|b^ - (S + f)/(k + 1)| <= g(k + 3) * B_d / (k + 1)``, ``B_d = A_d + |f_d|``.
  (The torch CPU path divides instead: one rounding fewer.)
* ``mu^`` is the fp32 mean the caller computed on the device, an n-term
  reduction in some tree plus one division, against the fp64 mean the
  reference uses: ``|mu^ - mu| <= g(n) * mean_i |f_i[d]|``.
* the subtraction rounds once, relative to its own result.

      e_d = (g(k + 3) B_d / (k + 1) + g(n) mean|f[d]|) (1 + u) + u |t_d|

* ``t^2`` moves by at most ``(2 |t_d| + e_d) e_d``; the D products each round
  once and are added one after the other (D - 1 adds):
  ``g(D + 1) * sum_d (|t_d| + e_d)^2``.
* a product below the smallest normal fp32 number may be flushed:
  ``D * 2^-126``. (Irrelevant except for all-zero data.)

      tol_k(i) = sum_d (2 |t_d| + e_d) e_d + g(D + 1) sum_d (|t_d| + e_d)^2
                 + D 2^-126

A fused multiply-add (``a * inv - mu``, ``t * t + d2``) only removes
roundings, so the compiler's contraction stays inside the count.

Exact tie rule
--------------
Bitwise identical rows give bitwise identical d2 in the kernel (same
operations on the same numbers), and the reduction prefers the lower index on
equality. So for identical rows i < j: if both are picked, i comes first; if
one is picked, it is i. Equivalently: of every group of identical rows the
picked ones are the lowest indices, in ascending order. No allowance.

Exact order where the reference is decisive
-------------------------------------------
``ref_order`` reports per step the literal gap between the best and the
second-best distance, and ``gap / allowance``:

    min over candidates i whose row differs from the winner a's row of
        (d_k(i) - d_k(a)) / ((tol_k(i) + tol_k(a)) / 2)

If that exceeds 2, every such i has ``d(i) - tol(i) > d(a) + tol(a)``: no
kernel within the allowance can prefer i, and among rows identical to a the
tie rule picks the same index as the reference. By induction over the steps
(same prefix, same S) the whole order is forced. The pairwise form is the
tight version of "gap > twice the allowance": a far candidate has a larger
tol but also a far larger distance. Rows identical to the winner are left
out of the gap because the tie rule, not the distance, decides among them.
The self-test demands a factor 10 instead of 2 for every input on which the
GPU test asks for equality.

Inputs
------
Post-ReLU, GAP-like data unless noted: ``relu(randn)`` rounded to the bf16
grid and held in fp32 - non-negative, exact zeros, natural duplicate values.
The seeds were chosen on the CPU, from the reference alone, so that every
input is decisive (gap / allowance >= 10; plain seeds often are not: seed 18
of the (200, 64, 50) randn case has 0.32).

Record
------
Nothing was calibrated. On the MI355X every order of test_herding_gpu.py
equals the fp64 reference, so ``(d(pick) - min) / allowance`` is 0 at every
shape; the smallest gap / allowance per input (a property of the input, from
the CPU) is 16.2 (257, 64, 20), 17.5 (600, 8, 30), 67.6 (300, 300, 6), 111
(130, 2048, 4), 18.4 (14900, 64, 3), 15.3 (200, 64, 50), 275 / 24.9 (the
duplicate-row inputs), 16.8 at the least in the batched calls, 13.1 in the
memory scenario. COVERAGE.md holds the table.
"""

import numpy as np
import torch

U = 2.0 ** -24
F32_MIN_NORMAL = 2.0 ** -126


def g(j):
    return j * U / (1.0 - j * U)


def _f64(f):
    if torch.is_tensor(f):
        f = f.detach().cpu().double().numpy()
    return np.asarray(f, dtype=np.float64)


class _Stepper:
    """fp64 state of one greedy run over ``f`` (n, D)."""

    def __init__(self, f):
        self.f = _f64(f)
        self.n, self.D = self.f.shape
        self.mu = self.f.mean(axis=0) if self.n else np.zeros(self.D)
        self.absmean = np.abs(self.f).mean(axis=0) if self.n \
            else np.zeros(self.D)
        self.S = np.zeros(self.D)
        self.A = np.zeros(self.D)
        self.sel = np.zeros(self.n, dtype=bool)
        self.k = 0

    def dist_tol(self):
        """-> d_k (n,), tol_k (n,), both fp64, for every row."""
        k, n, D = self.k, self.n, self.D
        t = (self.S[None, :] + self.f) / (k + 1) - self.mu[None, :]
        at = np.abs(t)
        B = self.A[None, :] + np.abs(self.f)
        e = (g(k + 3) * B / (k + 1) + g(n) * self.absmean[None, :]) \
            * (1 + U) + U * at
        d = (t * t).sum(axis=1)
        tol = ((2 * at + e) * e).sum(axis=1) \
            + g(D + 1) * ((at + e) ** 2).sum(axis=1) + D * F32_MIN_NORMAL
        return d, tol

    def take(self, i):
        self.S += self.f[i]
        self.A += np.abs(self.f[i])
        self.sel[i] = True
        self.k += 1


def ref_order(f, m):
    """The literal iCaRL loop in fp64, lowest index on exact ties ->
    dict(order: list, gap: (m,) best-to-second distance, ratio: (m,)
    gap / allowance as the module docstring defines it; inf when no other
    candidate is left)."""
    st = _Stepper(f)
    assert 0 <= m <= st.n
    order, gaps, ratios = [], [], []
    for _ in range(m):
        d, tol = st.dist_tol()
        dm = np.where(st.sel, np.inf, d)
        a = int(np.argmin(dm))          # first minimum: lowest index
        rest = dm.copy()
        rest[a] = np.inf
        gaps.append(float(rest.min() - dm[a]))
        other = ~st.sel & ~(st.f == st.f[a]).all(axis=1)
        if other.any():
            r = (d[other] - d[a]) / ((tol[other] + tol[a]) / 2)
            ratios.append(float(r.min()))
        else:
            ratios.append(float("inf"))
        order.append(a)
        st.take(a)
    return dict(order=order, gap=np.array(gaps), ratio=np.array(ratios))


def structure_error(order, n, m):
    """None, or what is wrong with the shape / range / distinctness."""
    o = [int(v) for v in order]
    if len(o) != m:
        return f"{len(o)} entries, expected {m}"
    bad = [v for v in o if not 0 <= v < n]
    if bad:
        return f"entries outside [0, {n}): {bad[:5]}"
    if len(set(o)) != len(o):
        seen, rep = set(), []
        for v in o:
            if v in seen:
                rep.append(v)
            seen.add(v)
        return f"repeated picks: {rep[:5]}"
    return None


def step_ratios(f, order):
    """(d_k(pick) - min_i d_k(i)) / (tol_k(pick) + tol_k(argmin)) for every
    step of a structurally valid ``order`` -> (m,) fp64. <= 1 is accepted."""
    st = _Stepper(f)
    out = []
    for p in (int(v) for v in order):
        d, tol = st.dist_tol()
        dm = np.where(st.sel, np.inf, d)
        a = int(np.argmin(dm))
        out.append((d[p] - dm[a]) / (tol[p] + tol[a]))
        st.take(p)
    return np.array(out)


def tie_error(f, order):
    """None, or the first violation of the exact tie rule."""
    fa = np.ascontiguousarray(_f64(f))
    groups = {}
    for i in range(fa.shape[0]):
        groups.setdefault(fa[i].tobytes(), []).append(i)
    pos = {int(v): k for k, v in enumerate(order)}
    for members in groups.values():
        if len(members) < 2:
            continue
        picked = [i for i in members if i in pos]
        if picked != members[:len(picked)]:
            return f"identical rows {members}: picked {picked}, not the " \
                   f"lowest indices"
        steps = [pos[i] for i in picked]
        if steps != sorted(steps):
            return f"identical rows {picked} picked at steps {steps}: a " \
                   f"higher index came first"
    return None


def verdict(f, order, m, exact=False, ref=None):
    """-> (reason or None, worst err/allowance). Never raises on a wrong
    order; ``exact`` asserts its own precondition (a decisive reference)."""
    n = _f64(f).shape[0]
    order = [int(v) for v in order]
    why = structure_error(order, n, m)
    if why:
        return why, float("inf")
    r = step_ratios(f, order)
    worst = float(r.max()) if len(r) else 0.0
    if worst > 1.0:
        k = int(np.argmax(r > 1.0))
        return f"step {k}: pick {order[k]} is {r[k]:.3g} allowances above " \
               f"the minimum", worst
    why = tie_error(f, order)
    if why:
        return why, worst
    if exact:
        ref = ref or ref_order(f, m)
        assert m == 0 or ref["ratio"].min() > 2.0, \
            "exact order asked of an input whose reference is not decisive"
        if order != ref["order"]:
            k = next(i for i, (a, b) in enumerate(zip(order, ref["order"]))
                     if a != b)
            return f"order differs from the decisive reference at step {k}: " \
                   f"{order[k]} vs {ref['order'][k]}", worst
    return None, worst


def check(f, order, m, what, exact=False, ref=None):
    """Assert ``order`` is an acceptable herding of ``f``; prints the
    diagnostics first -> worst err/allowance."""
    ref = ref or ref_order(f, m)
    why, worst = verdict(f, order, m, exact=exact, ref=ref)
    gmin = float(ref["ratio"].min()) if m else float("inf")
    print(f"{what}: max (d(pick) - min) / allowance = {worst:.4g}, "
          f"min reference gap / allowance = {gmin:.4g}"
          f"{' (exact order demanded)' if exact else ''}")
    assert why is None, f"{what}: {why}"
    return worst


# ------------------------------------------------------------------- inputs

def relu_bf16(n, D, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.relu(torch.randn(n, D, generator=gen)) \
        .to(torch.bfloat16).float()


def _bf16(v):
    return v.to(torch.bfloat16).float()


def _case_second_trip_winner():
    """(257, 64, 20): the only candidate of the second trip of the candidate
    loop, row 256, sits at the mean of the others and must be picked first."""
    f = relu_bf16(257, 64, 2)
    f[256] = _bf16(f[:256].mean(0))
    return f


def _case_duplicates(n, seed):
    """Rows 3, 40, 41 are copies of one vector near the mean; with n = 320
    rows 10, 266 and 300 are copies of another (266: the same thread's second
    trip; 300: another thread's)."""
    f = relu_bf16(n, 16, seed)
    gen = torch.Generator().manual_seed(seed + 1)
    mu = f.mean(0)
    f[[3, 40, 41]] = _bf16(mu + 0.02 * torch.randn(16, generator=gen))
    if n > 300:
        f[[10, 266, 300]] = _bf16(mu + 0.02 * torch.randn(16, generator=gen))
    return f


def _case_randn():
    gen = torch.Generator().manual_seed(RANDN_SEED)
    return torch.randn(200, 64, generator=gen)


RANDN_SEED = 132

# name -> (builder, m, exact order demanded). The exact flags are earned in
# test_herding_oracle_selftest.py: min gap / allowance >= 10 on the CPU.
SINGLE_CASES = {
    "1x1x1": (lambda: relu_bf16(1, 1, 111), 1, True),
    "5x3x5_all": (lambda: relu_bf16(5, 3, 535), 5, True),
    "257x64x20": (_case_second_trip_winner, 20, True),
    "600x8x30": (lambda: relu_bf16(600, 8, 38), 30, True),
    "300x300x6": (lambda: relu_bf16(300, 300, 1), 6, True),
    "130x2048x4": (lambda: relu_bf16(130, 2048, 2), 4, True),
    "14900x64x3": (lambda: relu_bf16(14900, 64, 29), 3, True),
    "200x64x50_randn": (_case_randn, 50, True),
    "64x16x12_dup": (lambda: _case_duplicates(64, 641612), 12, True),
    "320x16x12_dup": (lambda: _case_duplicates(320, 3201612), 12, True),
}
DUP_GROUPS = {"64x16x12_dup": [[3, 40, 41]],
              "320x16x12_dup": [[3, 40, 41], [10, 266, 300]]}

_cache = {}


def single_case(name):
    """-> (f (n, D) fp32 CPU tensor, m, exact, ref_order dict); built once,
    shared between the tests, never modified."""
    if name not in _cache:
        build, m, exact = SINGLE_CASES[name]
        f = build()
        _cache[name] = (f, m, exact, ref_order(f, m))
    return _cache[name]


# name -> (class sizes, D, quota, per-class seeds); D16_dup holds the two
# duplicate-row inputs above, so the batched kernel's own tie-break is judged
BATCH_CASES = {
    "D64": ([1, 7, 256, 257, 600], 64, 20, [101, 107, 364, 359, 4]),
    "D300": ([40, 300], 300, 6, [140, 1]),
    "D16_dup": ([64, 320], 16, 12, None),
}


def batch_case(name):
    """-> (list of per-class (n_c, D) fp32 CPU tensors, quota, list of
    per-class ref_order dicts at m_c = min(quota, n_c))."""
    key = "batch:" + name
    if key not in _cache:
        sizes, D, quota, seeds = BATCH_CASES[name]
        if name == "D16_dup":
            feats = [single_case(k)[0] for k in DUP_GROUPS]
            assert [f.shape[0] for f in feats] == sizes
        else:
            feats = [relu_bf16(n, D, s) for n, s in zip(sizes, seeds)]
        refs = [ref_order(f, min(quota, f.shape[0])) for f in feats]
        _cache[key] = (feats, quota, refs)
    return _cache[key]


# -------------------------------------------------- RehearsalMemory scenario

MEMORY_SIZE = 24
MEMORY_D = 16


def memory_tasks():
    """Two tasks for ``RehearsalMemory.add`` -> [(x, y, t, feats), ...].
    Task A brings class 0 alone (40 samples: the single launch, quota 24).
    Task B brings classes 1, 2, 3 with 30, 5 and 270 samples (the batched
    launch; quota 24 // 4 = 6, so class 2 is smaller than the quota and class
    0 shrinks from 24 to 6) plus 9 replayed samples of class 0, which add()
    must ignore; rows are shuffled so that class-local and global indices
    differ."""
    if "memory" not in _cache:
        rng = np.random.default_rng(2024)
        tasks = []
        for tid, sizes in enumerate([{0: 40}, {1: 30, 2: 5, 3: 270, 0: 9}]):
            y = np.concatenate([np.full(n, c) for c, n in sizes.items()])
            y = y[rng.permutation(len(y))]
            x = rng.integers(0, 255, size=(len(y), 4, 4, 3), dtype=np.uint8)
            t = np.full_like(y, tid)
            feats = relu_bf16(len(y), MEMORY_D, 5000 + tid)
            tasks.append((x, y, t, feats))
        _cache["memory"] = tasks
    return _cache["memory"]


def ref_memory(tasks, memory_size=MEMORY_SIZE):
    """What RehearsalMemory must hold after the tasks, rebuilt from
    ``ref_order`` -> (stores: class -> (x, y, t), selections: per task
    class -> global indices, min gap / allowance over every class)."""
    if "ref_memory" in _cache:
        return _cache["ref_memory"]
    stores, selections, gmin = {}, [], float("inf")
    for x, y, t, feats in tasks:
        new = [int(c) for c in np.unique(y) if int(c) not in stores]
        quota = memory_size // (len(stores) + len(new))
        sel = {}
        for c in new:
            idx = np.where(y == c)[0]
            r = ref_order(feats[idx], min(quota, len(idx)))
            gmin = min(gmin, float(r["ratio"].min()))
            keep = idx[np.array(r["order"], dtype=np.int64)]
            sel[c] = keep
            stores[c] = (x[keep], y[keep], t[keep])
        for c in stores:
            stores[c] = tuple(a[:quota] for a in stores[c])
        selections.append(sel)
    _cache["ref_memory"] = (stores, selections, gmin)
    return _cache["ref_memory"]


def check_memory(mem, tasks_selections, stores, what):
    """``mem`` (after the last task) holds exactly ``stores``; its
    ``last_selection`` equals the last task's reference selection."""
    assert sorted(mem._x) == sorted(stores), f"{what}: classes"
    for c, (x, y, t) in stores.items():
        assert np.array_equal(mem._x[c], x), f"{what}: x of class {c}"
        assert np.array_equal(mem._y[c], y), f"{what}: y of class {c}"
        assert np.array_equal(mem._t[c], t), f"{what}: t of class {c}"
    last = tasks_selections[-1]
    assert sorted(mem.last_selection) == sorted(last), f"{what}: selection"
    for c, keep in last.items():
        assert np.array_equal(mem.last_selection[c], keep), \
            f"{what}: last_selection of class {c}: " \
            f"{mem.last_selection[c].tolist()} vs {keep.tolist()}"
    gx, gy, gt = mem.get()
    cs = sorted(stores)
    assert np.array_equal(gx, np.concatenate([stores[c][0] for c in cs]))
    assert np.array_equal(gy, np.concatenate([stores[c][1] for c in cs]))
    assert np.array_equal(gt, np.concatenate([stores[c][2] for c in cs]))


# ------------------------------------------ fp32 model of the kernel + faults

def kernel_model(f, m, mu=None, *, tie_high=False, honour_selected=True,
                 update_sum=True, use_inv=True, scan=None, sum_cols=None):
    """The kernel's loop in numpy fp32 (vectorised, so the D-sum order is
    numpy's, within the allowance). The keyword arguments seed one fault
    each: ties to the higher index; the selected flag ignored; ``sum_sel``
    never updated; ``1/(k+1)`` omitted; only the first ``scan`` candidates
    visited; ``sum_sel`` updated for the first ``sum_cols`` coordinates only.
    A step with no candidate left returns -1 from there on."""
    f32 = np.ascontiguousarray(
        f.detach().cpu().numpy() if torch.is_tensor(f) else f,
        dtype=np.float32)
    n, D = f32.shape
    if mu is None:
        mu = f32.mean(axis=0, dtype=np.float32)
    mu = np.asarray(mu, dtype=np.float32)
    s = np.zeros(D, dtype=np.float32)
    sel = np.zeros(n, dtype=bool)
    order = []
    for k in range(m):
        inv = np.float32(1) / np.float32(k + 1) if use_inv else np.float32(1)
        t = (s[None, :] + f32) * inv - mu[None, :]
        d2 = (t * t).sum(axis=1, dtype=np.float32)
        if honour_selected:
            d2[sel] = np.inf
        if scan is not None:
            d2[scan:] = np.inf
        best = d2.min() if n else np.inf
        if not np.isfinite(best):
            order.append(-1)
            continue
        cands = np.flatnonzero(d2 == best)
        i = int(cands[-1] if tie_high else cands[0])
        order.append(i)
        sel[i] = True
        if update_sum:
            c = D if sum_cols is None else sum_cols
            s[:c] += f32[i, :c]
    return order


def batch_model(feats, quota, *, mean_shift=0, row_shift=0,
                global_idx=False, tie_high=False):
    """The batched launch modelled class by class with ``kernel_model`` ->
    list of orders. Faults: class c uses the mean of class c + mean_shift
    (cyclic); reads its rows from its offset + row_shift (zeros past the
    end); writes global instead of class-local indices; ties to the higher
    index."""
    f32 = [f.detach().cpu().numpy().astype(np.float32) for f in feats]
    D = f32[0].shape[1]
    fall = np.concatenate(f32 + [np.zeros((abs(row_shift) + 1, D),
                                          dtype=np.float32)])
    offs = np.concatenate([[0], np.cumsum([a.shape[0] for a in f32])])
    out = []
    for c, a in enumerate(f32):
        n = a.shape[0]
        rows = fall[offs[c] + row_shift: offs[c] + row_shift + n]
        mu = f32[(c + mean_shift) % len(f32)].mean(axis=0, dtype=np.float32)
        o = kernel_model(rows, min(quota, n), mu, tie_high=tie_high)
        out.append([i + int(offs[c]) for i in o] if global_idx else o)
    return out
