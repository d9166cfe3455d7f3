"""fp64 reference, comparator, test inputs and a fault-seeding fp32 model for
``ops.kmeans_proxies`` (cilfw/ops/kmeans.py, csrc/kmeans.hip), shared by
test_kmeans_oracle_selftest.py and test_kmeans_gpu.py.

Definition: the docstring of cilfw/ops/kmeans.py. ``ref_class`` is that text in
fp64, with the distance as the literal ``sum_d (x^_d - c_d)^2``.

The op returns discrete choices (seed rows, assignments, an iteration count)
and floats that depend on them. Float noise may flip a choice, so equality is
only demanded where the reference is decisive, and that is asserted.

Allowance (nothing is fitted to an output)
------------------------------------------
``u = 2^-24``, ``g(j) = j u / (1 - j u)`` bounds a summation tree of depth j
(j successive roundings on any path) against the sum of the magnitudes.

* a D-term sum of products in the kernel (``km_dot4``): every lane chains
  ``4 ceil(D / 256)`` fmas, one rounding each, and the xor butterfly adds six
  more levels: depth ``J = 4 ceil(D / 256) + 6`` (10 at D = 64, 22 at
  D = 1000), not D. The CPU path sums in torch's order; the self-test holds
  it to the same allowance instead of assuming anything about that order.
* unit row: ``x^ = fl(x * fl(1 / fl(sqrt(ss))))``, ss such a sum (g(J)
  relative, halved by the root), three more roundings: every element within
  ``ex |x^_d|``, ``ex = g(J + 4)`` (counted generously).
* centre: a seed is a copy of a unit row: ``dc_d = ex |c_d|``. A mean of m
  members is an m-term sum plus one division of operands that carry ex:
  ``dc_d = (g(m + 1) + ex) mean_members |x^_d|`` (the mean that seeds centre 0:
  m = n). A centre without members keeps its previous value and its dc. This
  presumes the same members as the reference: by induction over the passes,
  true while every choice so far was decisive.
* distance of row i to centre k, evaluated as ``c2 - 2 dot + xx`` with three
  D-term sums and two more roundings, against the fp64 distance of the exact
  operands:
      tol(i, k) = g(J + 3) (sum c^2 + 2 sum |x c| + sum x^2)
                  + sum_d (2 |t_d| + e_d) e_d,
  ``t = x^ - c``, ``e_d = ex |x^_d| + dc_d`` (the operands' own errors).
  Clamping a negative result to 0 only moves it towards the true value.

Decisive reference
------------------
* a seeding step picks row a by its value v(a) (distance to the mean, or the
  smallest distance to the chosen centres) against every other row i:
  ``|v(i) - v(a)| / ((T(i) + T(a)) / 2)``, T(i) the largest tol(i, k) over the
  centres involved. Rows bitwise identical to row a are left out: the kernel
  evaluates identical rows identically and the index rule decides. So are
  copies of a centre already chosen: a seed centre is a bit copy of its row,
  their distance to it is exactly 0 and cannot win a step unless every row
  left is such a copy, where again the index rule decides.
* an assignment of row i: ``(d(i, second) - d(i, best)) / ((tol(i, second) +
  tol(i, best)) / 2)``; centres bitwise identical to the best one are left
  out (index rule).
Above 2 no implementation within the allowance can choose differently. The
self-test demands 10 for every input; then ``assign`` and ``iters`` must equal
the reference exactly and the passes of both runs see the same members.

Proxy bound
-----------
``p = c / |c|`` with c within dc of the fp64 centre c*:
    |p_d - p*_d| <= (dc_d + |p*_d| |dc|_2) / |c*| + g(J + 4) |p*_d| + 2^-126.

Inputs
------
``blobs``: K random non-negative directions plus noise, rectified (post-ReLU
like). The seeds below were searched on the CPU, from the reference alone.

Record (MI355X, test_kmeans_gpu.py): assign and iters equal the reference at
every shape; COVERAGE.md tabulates err / bound and gap / allowance.
"""

import numpy as np
import torch

U = 2.0 ** -24
EPS = 1e-12
TINY = 2.0 ** -126


def g(j):
    return j * U / (1.0 - j * U)


def depth(D):
    """Depth of the kernel's D-term sums (module docstring)."""
    return 4 * -(-D // 256) + 6


def _f64(f):
    if torch.is_tensor(f):
        f = f.detach().cpu().double().numpy()
    return np.asarray(f, dtype=np.float64)


def _unit(x):
    return x / np.maximum(np.sqrt((x * x).sum(axis=1, keepdims=True)), EPS)


def _dist_tol(X, cen, dc, ex):
    """X (n, D), cen (K, D), dc (K, D) -> d (n, K), tol (n, K) in fp64."""
    D = X.shape[1]
    t = X[:, None, :] - cen[None]
    d = (t * t).sum(axis=2)
    S = (cen * cen).sum(axis=1)[None] + 2 * np.abs(X) @ np.abs(cen).T \
        + (X * X).sum(axis=1)[:, None]
    e = ex * np.abs(X)[:, None, :] + dc[None]
    tol = g(depth(D) + 3) * S + ((2 * np.abs(t) + e) * e).sum(axis=2) + 3 * TINY
    return d, tol


def _same_rows(A, v):
    return (A == v[None]).all(axis=1)


def ref_class(f, K, max_iter):
    """One class in fp64 -> dict(centres (K, D), dc (K, D), proxies (K, D),
    bound (K, D), assign (n,), iters, seeds, seed_ratio (K,), assign_ratio
    (smallest over all passes), emptied (bool: some centre lost all its
    members in some pass))."""
    X = _unit(_f64(f))
    n, D = X.shape
    assert n >= K >= 1
    ex = g(depth(D) + 4)
    absX = np.abs(X)
    seed_ratio = []

    def pick(v, T, largest):
        a = int(np.argmax(v)) if largest else int(np.argmin(v))  # first
        other = ~_same_rows(X, X[a])
        for sd in seeds:  # copies of a chosen centre: distance exactly 0
            other &= ~_same_rows(X, X[sd])
        r = np.abs(v[other] - v[a]) / ((T[other] + T[a]) / 2)
        seed_ratio.append(float(r.min()) if other.any() else float("inf"))
        return a

    seeds = []
    mean = X.mean(axis=0)
    dcm = (g(n + 1) + ex) * absX.mean(axis=0)
    d, tol = _dist_tol(X, mean[None], dcm[None], ex)
    row = pick(d[:, 0], tol[:, 0], False)
    cen = np.zeros((K, D))
    dc = np.zeros((K, D))
    assign = np.full(n, -1, dtype=np.int64)
    dmin = Tmax = None
    for j in range(K):
        cen[j], dc[j] = X[row], ex * absX[row]
        assign[row] = j
        seeds.append(row)
        if j + 1 < K:
            d, tol = _dist_tol(X, cen[j:j + 1], dc[j:j + 1], ex)
            dmin = d[:, 0] if dmin is None else np.minimum(dmin, d[:, 0])
            Tmax = tol[:, 0] if Tmax is None else np.maximum(Tmax, tol[:, 0])
            row = pick(dmin, Tmax, True)
    it, assign_ratio, emptied = 0, float("inf"), False
    while it < max_iter:
        it += 1
        d, tol = _dist_tol(X, cen, dc, ex)
        new = d.argmin(axis=1)                          # first minimum
        if K > 1:
            rows = np.arange(n)
            same = (cen[None] == cen[new][:, None, :]).all(axis=2)  # (n, K)
            r = (d - d[rows, new][:, None]) \
                / ((tol + tol[rows, new][:, None]) / 2)
            r = np.where(same, np.inf, r)
            assign_ratio = min(assign_ratio, float(r.min()))
        changed = bool((new != assign).any())
        assign = new
        for k in range(K):
            mem = assign == k
            m = int(mem.sum())
            if m == 0:
                emptied = True
                continue
            cen[k] = X[mem].sum(axis=0) / m
            dc[k] = (g(m + 1) + ex) * absX[mem].mean(axis=0)
        if not changed:
            break
    nc = np.maximum(np.sqrt((cen * cen).sum(axis=1, keepdims=True)), EPS)
    prox = cen / nc
    bound = (dc + np.abs(prox) * np.sqrt((dc * dc).sum(axis=1,
                                                       keepdims=True))) / nc \
        + g(depth(D) + 4) * np.abs(prox) + TINY
    return dict(centres=cen, dc=dc, proxies=prox, bound=bound, assign=assign,
                iters=it, seeds=seeds, seed_ratio=np.array(seed_ratio),
                assign_ratio=assign_ratio, emptied=emptied)


def ref_batch(feats, sizes, K, max_iter):
    """-> list of ``ref_class`` dicts, one per class segment."""
    out, o = [], 0
    for n in sizes:
        out.append(ref_class(feats[o:o + n], K, max_iter))
        o += n
    return out


def min_ratio(refs):
    """Smallest gap / allowance over every seeding step and assignment."""
    return min(min(float(r["seed_ratio"].min()), r["assign_ratio"])
               for r in refs)


def verdict(refs, sizes, K, proxies, assign, iters):
    """-> (reason or None, worst proxy err / bound). Never raises on a wrong
    result."""
    C, n = len(sizes), sum(sizes)
    D = refs[0]["proxies"].shape[1]
    if tuple(proxies.shape) != (C * K, D) or proxies.dtype != torch.float32:
        return f"proxies {tuple(proxies.shape)} {proxies.dtype}", float("inf")
    if tuple(assign.shape) != (n,) or assign.dtype != torch.int32:
        return f"assign {tuple(assign.shape)} {assign.dtype}", float("inf")
    if tuple(iters.shape) != (C,) or iters.dtype != torch.int32:
        return f"iters {tuple(iters.shape)} {iters.dtype}", float("inf")
    p = proxies.detach().cpu().double().numpy()
    a = assign.detach().cpu().numpy().astype(np.int64)
    it = iters.detach().cpu().numpy().astype(np.int64)
    if not np.isfinite(p).all():
        return "non-finite proxies", float("inf")
    worst, o = 0.0, 0
    for c, (r, q) in enumerate(zip(refs, sizes)):
        ac = a[o:o + q]
        o += q
        if ac.min() < 0 or ac.max() >= K:
            return f"class {c}: assign outside [0, {K}): " \
                   f"{ac.min()}..{ac.max()}", float("inf")
        if it[c] != r["iters"]:
            return f"class {c}: iters {it[c]} vs {r['iters']}", float("inf")
        if not np.array_equal(ac, r["assign"]):
            i = int(np.argmax(ac != r["assign"]))
            return f"class {c}: assign[{i}] = {ac[i]} vs " \
                   f"{r['assign'][i]}", float("inf")
        ratio = np.abs(p[c * K:(c + 1) * K] - r["proxies"]) / r["bound"]
        worst = max(worst, float(ratio.max()))
    if worst > 1.0:
        return f"proxy err / bound = {worst:.4g}", worst
    return None, worst


def check(refs, sizes, K, out, what):
    """Assert ``out = (proxies, assign, iters)`` equals the decisive
    reference; prints the figures first -> worst proxy err / bound."""
    gmin = min_ratio(refs)
    assert gmin > 2.0, \
        f"{what}: equality asked of an input whose reference is not decisive"
    why, worst = verdict(refs, sizes, K, *out)
    print(f"{what}: max proxy err / bound = {worst:.4g}, min reference gap / "
          f"allowance = {gmin:.4g}, iters = "
          f"{[r['iters'] for r in refs]}")
    assert why is None, f"{what}: {why}"
    return worst


# ------------------------------------------------------------------- inputs

def blobs(n, D, K, seed, noise=0.15):
    """n rows around K random non-negative directions, rectified."""
    gen = torch.Generator().manual_seed(seed)
    dirs = torch.relu(torch.randn(K, D, generator=gen))
    which = torch.randint(0, K, (n,), generator=gen)
    x = torch.relu(dirs[which] + noise * torch.randn(n, D, generator=gen))
    return x + 0.01  # no all-zero row


def _case_dup():
    """([48]; 16; 4): rows 30 and 44 are copies of row 5, rows 20 and 41 of
    row 9; the seeds are chosen so that a duplicated row is a maximin winner
    (the lower index must be taken) and the copies follow their original."""
    f = blobs(48, 16, 4, DUP_SEED)
    r = ref_class(f, 4, 100)
    f = f.clone()
    a, b = r["seeds"][0], r["seeds"][2]
    others = [i for i in range(47, 0, -1) if i not in r["seeds"]]
    f[others[0]] = f[a]
    f[others[5]] = f[a]
    f[others[1]] = f[b]
    f[others[9]] = f[b]
    return f


def _case_dup_empty():
    """([3]; 4; 3): rows A, A, B. Two distinct rows for three centres: the
    seeds are rows 0, 2, 0 (the maximin tie at distance 0 goes to the lowest
    row), the centres A, B, A; the identical centres tie in every assignment
    (the lower wins), so centre 2 loses its seed row in the first pass and
    must keep its value. Two copies, not three: (A + A) / 2 is exact in every
    format, so centre 0 stays a bit copy of A."""
    ab = blobs(2, 4, 2, DUP_EMPTY_SEED, noise=0.5)
    return ab[[0, 0, 1]].clone()


DUP_SEED = 3
DUP_EMPTY_SEED = 5

# name -> (class sizes, D, K, max_iter, builder of the (n_total, D) rows)
CASES = {
    "1x4x1": ([1], 4, 1, 100, lambda: blobs(1, 4, 1, 11)),
    "5x4x5": ([5], 4, 5, 100, lambda: blobs(5, 4, 5, 12, noise=0.5)),
    "batch_D64_K10": ([10, 40, 257, 600], 64, 10, 100, lambda: torch.cat(
        [blobs(n, 64, 10, s) for n, s in zip([10, 40, 257, 600],
                                              BATCH_SEEDS)])),
    "D300_K6": ([40, 300], 300, 6, 100, lambda: torch.cat(
        [blobs(n, 300, 6, s) for n, s in zip([40, 300], D300_SEEDS)])),
    "64x1000x16": ([64], 1000, 16, 100,
                   lambda: blobs(64, 1000, 16, KD_SEED)),
    "48x16x4_dup": ([48], 16, 4, 100, _case_dup),
    "3x4x3_dup_empty": ([3], 4, 3, 100, _case_dup_empty),
    "batch_D64_K7": ([7, 40, 257, 600], 64, 7, 100, lambda: torch.cat(
        [blobs(n, 64, 10, s) for n, s in zip([7, 40, 257, 600],
                                              BATCH7_SEEDS)])),
    "iter1": ([7, 40, 257, 600], 64, 7, 1, None),    # rows of batch_D64_K7
    "iter2": ([7, 40, 257, 600], 64, 7, 2, None),
}
# The issue lists ([7, 40, 257, 600]; 64; 10), which its own rule n >= K
# refuses (7 < 10; test_kmeans_gpu.py asserts the refusal). Both halves are
# kept: K = 10 with the smallest class raised to 10 rows, and the listed
# sizes at K = 7 (ten planted directions for seven centres: 3 to 5 passes).
BATCH_SEEDS = [7, 3, 6, 1]
BATCH7_SEEDS = [3, 3, 6, 1]
D300_SEEDS = [0, 0]
KD_SEED = 0

_cache = {}


def case(name):
    """-> (feats (n, D) fp32 CPU tensor, sizes, K, max_iter, refs); built
    once, shared between the tests, never modified."""
    if name not in _cache:
        sizes, D, K, max_iter, build = CASES[name]
        f = case("batch_D64_K7")[0] if build is None else build()
        assert tuple(f.shape) == (sum(sizes), D)
        _cache[name] = (f, sizes, K, max_iter,
                        ref_batch(f, sizes, K, max_iter))
    return _cache[name]


def seg_offsets(sizes):
    return [0] + np.cumsum(sizes).tolist()


# ------------------------------------------ fp32 model of the kernel + faults

def _first(v, largest=False, high=False):
    m = v.max() if largest else v.min()
    c = np.flatnonzero(v == m)
    return int(c[-1] if high else c[0])


def model(feats, sizes, K, max_iter, *, tie_high_row=False,
          tie_high_centre=False, seed_row0=False, empty_zero=False, cols=None,
          rows=None, global_assign=False, seg_shift=0, unnormalised=False,
          one_short=False):
    """The kernel's algorithm in numpy fp32 (vectorised sums: numpy's order,
    within the allowance) -> (proxies, assign, iters) tensors. Each keyword
    seeds one fault: seeding ties to the higher row; assignment ties to the
    higher centre; centre 0 seeded from row 0; an emptied centre reset to
    zero; only the first ``cols`` columns of the means updated; only the
    first ``rows`` rows visited by the assignment (the rest go to centre 0);
    assign made global (class c adds c K); class c reads its rows from its
    offset + seg_shift rows (cyclic); output left un-normalised; one
    iteration fewer than needed."""
    f32 = np.ascontiguousarray(
        feats.detach().cpu().numpy() if torch.is_tensor(feats) else feats,
        dtype=np.float32)
    off = seg_offsets(sizes)
    one = np.float32(1)
    xh_all = f32 * (one / np.maximum(
        np.sqrt((f32 * f32).sum(axis=1, dtype=np.float32, keepdims=True)),
        np.float32(EPS)))
    P, A, I = [], [], []

    def dist(X, xx, cen):
        c2 = (cen * cen).sum(axis=1, dtype=np.float32)
        dots = (X[:, None, :] * cen[None]).sum(axis=2, dtype=np.float32)
        return np.maximum(c2[None] - np.float32(2) * dots + xx[:, None],
                          np.float32(0))

    def run(X, limit):
        n, D = X.shape
        xx = (X * X).sum(axis=1, dtype=np.float32)
        mean = X.sum(axis=0, dtype=np.float32) / np.float32(n)
        row = 0 if seed_row0 else _first(dist(X, xx, mean[None])[:, 0],
                                         high=tie_high_row)
        cen = np.zeros((K, D), dtype=np.float32)
        assign = np.full(n, -1, dtype=np.int64)
        dmin = None
        for j in range(K):
            cen[j] = X[row]
            assign[row] = j
            if j + 1 < K:
                d = dist(X, xx, cen[j:j + 1])[:, 0]
                dmin = d if dmin is None else np.minimum(dmin, d)
                row = _first(dmin, largest=True, high=tie_high_row)
        it = 0
        while it < limit:
            it += 1
            d = dist(X, xx, cen)
            new = np.array([_first(d[i], high=tie_high_centre)
                            for i in range(n)])
            if rows is not None:
                new[rows:] = 0
            changed = bool((new != assign).any())
            assign = new
            for k in range(K):
                mem = assign == k
                m = int(mem.sum())
                cc = D if cols is None else min(cols, D)
                if m == 0:
                    if empty_zero:
                        cen[k] = 0
                    continue
                cen[k, :cc] = X[mem][:, :cc].sum(axis=0, dtype=np.float32) \
                    / np.float32(m)
            if not changed:
                break
        return cen, assign, it

    n_all = f32.shape[0]
    for c, q in enumerate(sizes):
        idx = (np.arange(off[c], off[c] + q) + seg_shift) % n_all
        X = xh_all[idx]
        cen, assign, it = run(X, max_iter)
        if one_short and it > 1:
            cen, assign, it = run(X, it - 1)
        if not unnormalised:
            cen = cen * (one / np.maximum(np.sqrt(
                (cen * cen).sum(axis=1, dtype=np.float32, keepdims=True)),
                np.float32(EPS)))
        P.append(cen)
        A.append(assign + (c * K if global_assign else 0))
        I.append(it)
    return (torch.from_numpy(np.concatenate(P).astype(np.float32)),
            torch.from_numpy(np.concatenate(A).astype(np.int32)),
            torch.tensor(I, dtype=torch.int32))
