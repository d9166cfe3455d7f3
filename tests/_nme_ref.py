"""fp64 oracle, seeded inputs and allowances for the NME ops
(cilfw/ops/nme.py, csrc/nme.hip), shared by test_nme.py and test_nme_gpu.py.

Definition, with ``x^ = x / max(|x|_2, 1e-12)``: prototype
``p_c = m / max(|m|_2, 1e-12)``, ``m = mean_i f^_i``; score
``s(x, c) = x^ . p_c``; top-k descending, ties to the lower class index.

Allowances (u = 2^-24, fp32 unit roundoff):

* score:      ``|err| <= 2 u D sum_d |x^_d||p_d| + 8 u`` — the project's
  summation term (``_oracle.C_SUM = 2``) plus the rounding of the two
  normalisations and the final scale on a quantity <= 1;
* prototype:  ``|err| <= 2 u (D + q) (mag + |ref|)``,
  ``mag[c, d] = mean_i |f^_i[d]| / |m|``.

Inputs come from one CPU ``torch.Generator``; every generator call yields one
tensor and the tensors are drawn in the order of ``make_inputs``.
"""

import torch

import _oracle

EPS = 1e-12
SCORE_EXTRA = 8 * _oracle.U_F32

# (N, C, D, q)
SHAPES = {
    1: (37, 5, 64, 7),       # maxk = C, ragged row tile
    2: (37, 3, 68, 4),       # maxk = 3, D not a multiple of 64
    3: (130, 100, 512, 20),  # several row tiles
    4: (9, 1000, 2048, 2),   # many class tiles, deep D
    5: (1, 1, 4, 1),         # minimal
}


def make_inputs(shape_id, seed=0):
    """-> dict(ex (C, q, D), x (N, D), y (N,), targets (N,)) fp32 / int64."""
    N, C, D, q = SHAPES[shape_id]
    g = torch.Generator().manual_seed(1000 * shape_id + seed)
    centre = torch.relu(torch.randn(C, D, generator=g))
    ex = torch.relu(centre[:, None, :]
                    + 0.5 * torch.randn(C, q, D, generator=g))
    y = torch.randint(0, C, (N,), generator=g)
    x = torch.relu(centre[y] + 0.5 * torch.randn(N, D, generator=g))
    targets = y.clone()
    third = torch.arange(N) % 3 == 2  # every third row: a wrong target
    targets[third] = (y[third] + 1) % C
    return dict(ex=ex, x=x, y=y, targets=targets)


def seg_offsets(C, q):
    return [i * q for i in range(C + 1)]


def _unit(t):
    return t / t.norm(dim=-1, keepdim=True).clamp_min(EPS)


def protos_ref(ex):
    """ex (C, q, D) -> (ref, mag, n) in fp64 for _oracle.worst / bound with
    bf16_out=False: allowance 2 u n mag, mag already holding (mag + |ref|)."""
    C, q, D = ex.shape
    fh = _unit(ex.double())
    m = fh.mean(dim=1)
    nm = m.norm(dim=1, keepdim=True).clamp_min(EPS)
    ref = m / nm
    mag = fh.abs().mean(dim=1) / nm
    return ref, mag + ref.abs(), float(D + q)


def scores_ref(x, protos):
    """fp64 scores of fp32 rows x (N, D) against the fp32 prototypes AS GIVEN
    (C, D) -> (ref (N, C), mag (N, C), n = D); allowance
    2 u D mag + SCORE_EXTRA."""
    xh = _unit(x.double())
    p = protos.double()
    return xh @ p.T, xh.abs() @ p.abs().T, float(x.shape[1])


def score_allowance(mag, D):
    return _oracle.bound(mag, mag, D, False, extra=SCORE_EXTRA)


def check_protos(got, ex, what):
    ref, mag, n = protos_ref(ex)
    _oracle.check(got, ref, mag, n, False, what)
    norms = got.detach().double().cpu().norm(dim=1)
    # a correctly rounded unit vector: |p|^2 off by at most ~(D + 2) u
    tol = 2 * _oracle.U_F32 * (ex.shape[2] + 2)
    assert (norms - 1).abs().max().item() <= tol, \
        f"{what}: prototype norms off 1 by {(norms - 1).abs().max().item()}"


def check_topk(idx, score, counts, x, protos, targets, maxk, what):
    """Every property of a correct (idx, score, counts) against the fp64
    scores, with no row excluded."""
    idx = idx.detach().cpu().long()
    score = score.detach().cpu()
    N, C = x.shape[0], protos.shape[0]
    assert idx.shape == (N, maxk) and score.shape == (N, maxk)
    assert score.dtype == torch.float32
    ref, mag, D = scores_ref(x.cpu(), protos.cpu())
    allow = score_allowance(mag, D)
    # indices distinct and in range
    assert idx.min().item() >= 0 and idx.max().item() < C, f"{what}: range"
    srt = idx.sort(dim=1).values
    assert (srt[:, 1:] != srt[:, :-1]).all(), f"{what}: repeated class"
    # each returned score within allowance of the fp64 score of its index
    r_ref, r_allow = ref.gather(1, idx), allow.gather(1, idx)
    ratio = ((score.double() - r_ref).abs() / r_allow).max().item()
    print(f"{what}: max score err/allowance = {ratio:.4f}")
    assert ratio <= 1.0, f"{what}: score err/allowance {ratio}"
    # non-increasing; equal scores in ascending class order
    assert (score[:, 1:] <= score[:, :-1]).all(), f"{what}: order"
    eq = score[:, 1:] == score[:, :-1]
    assert (idx[:, 1:][eq] > idx[:, :-1][eq]).all(), f"{what}: tie order"
    # no class left out that fp64 puts clearly above the k-th returned one
    left = torch.ones(N, C, dtype=torch.bool)
    left.scatter_(1, idx, False)
    kth, kth_allow = score[:, -1:].double(), r_allow[:, -1:]
    over = (ref - kth) - (allow + kth_allow)
    assert not (left & (over > 0)).any(), f"{what}: a nearer class is missing"
    # top-1 equals fp64's (margins of make_inputs dwarf the allowance)
    assert (idx[:, 0] == ref.argmax(dim=1)).all(), f"{what}: top-1"
    # counts: recomputed on the host from the returned idx, exactly
    if targets is not None:
        hit = (idx == targets.cpu()[:, None]).cumsum(dim=1) > 0
        want = hit.sum(dim=0)
        assert counts.dtype == torch.int64
        assert torch.equal(counts.cpu(), want), \
            f"{what}: counts {counts.tolist()} vs {want.tolist()}"
    else:
        assert counts is None
