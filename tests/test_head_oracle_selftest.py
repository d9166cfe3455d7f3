"""CPU self-test of the head / loss oracle in ``tests/_head_ref.py``.

"Wrong kernels" are built on the CPU from the fp64 reference, rounded like
the kernel's output, each with one seeded fault; the comparator must reject
every one and accept the project's fp32 CPU path at the shapes of
test_head_gpu.py. The split factors those shapes rely on are pinned from the
launcher's own function. No GPU involved.
"""

import pytest
import torch

import _head_ref as R
import cilfw.ops.functional as CF
from test_ops_gpu import _cmp

T, LAM = R.T_KD, R.LAM


# --------------------------------------------------------------------- losses

def _softmax64(v):
    return torch.softmax(v, 1)


def _grad_formula(s, t, y, smooth, T, lam, up, ce=True, kd_cols=None,
                  kd_T=None, mean_over=None):
    """Closed-form fp64 dlogits; the keyword arguments seed the faults."""
    s64 = s.double()
    M, C = s64.shape
    g = torch.zeros_like(s64)
    if ce:
        g += _softmax64(s64) - smooth / C
        g.scatter_add_(1, y.view(-1, 1),
                       torch.full((M, 1), -(1 - smooth), dtype=g.dtype))
    if t is not None:
        Ck = t.shape[1] if kd_cols is None else kd_cols
        ps = _softmax64(s64[:, :Ck] / T)
        pt = _softmax64(t.double()[:, :Ck] / T)
        g[:, :Ck] += lam * (T if kd_T is None else kd_T) * (ps - pt)
    return g * (up / (M if mean_over is None else mean_over))


def _loss_faults(s, t, y, smooth, up, ce, scale):
    """name -> fp64 dlogits of a kernel with exactly that fault (only the
    faults that exist for this family / shape)."""
    M, C = s.shape
    Ck = 0 if t is None else t.shape[1]
    lam = LAM if ce else 1.0
    args = (s, t, y, smooth, T, lam, up)
    out = {}
    if C == 1:          # the gradient is identically zero: nothing to seed
        return out
    if ce and smooth > 0:
        out["smoothing_dropped"] = _grad_formula(s, t, y, 0.0, T, lam, up, ce)
    if Ck > 1:          # one KD column: ps = pt = 1, the term vanishes
        out["T_applied_once"] = _grad_formula(*args, ce, kd_T=1.0)
        if scale <= 8:
            out["kd_over_Ck-1"] = _grad_formula(*args, ce, kd_cols=Ck - 1)
    if ce and C > 1:
        out["target_off_by_one"] = _grad_formula(s, t, (y + 1) % C, smooth, T,
                                                 lam, up, ce)
    if C > 256:
        g = _grad_formula(*args, ce)
        g[:, 256:] = 0
        out["cols_ge_256_unwritten"] = g
    if M != 64:
        out["mean_over_64"] = _grad_formula(*args, ce, mean_over=64)
    if up != 1.0:
        out["upstream_ignored"] = _grad_formula(s, t, y, smooth, T, lam, 1.0,
                                                ce)
    return out


@pytest.mark.parametrize("scale", R.SCALES)
@pytest.mark.parametrize("shape", R.WA_SHAPES, ids=R.WA_IDS)
def test_wa_loss_cpu_path_accepted_faults_rejected(shape, scale):
    M, C, Ck = shape
    s, t, y = R.loss_inputs(M, C, Ck, scale, torch.bfloat16)
    for smooth in (0.0, 0.1):
        for up in (1.0, 0.37):
            ref = R.loss_ref(s, t, y, smooth, T, LAM, up)
            good = _grad_formula(s, t, y, smooth, T, LAM, up)
            assert (good - ref["grad"]).abs().max() <= 1e-12
            x = s.clone().requires_grad_(True)
            total, ce, kd = CF.wa_loss(x, t, y, smooth, T, LAM)
            (total * up).backward()
            assert x.grad.dtype == torch.bfloat16
            R.loss_check(dict(total=total, ce=ce, kd=kd), x.grad, ref,
                         f"cpu wa_loss {shape} x{scale} s{smooth} up{up}")
            assert R.grad_worst(good.to(torch.bfloat16), ref) <= 1.0
            for name, bad in _loss_faults(s, t, y, smooth, up, True,
                                          scale).items():
                r = R.grad_worst(bad.to(torch.bfloat16), ref)
                # measured smallest: 14.1 (mean over 64 at (1, 2, 1))
                assert r > 10.0, f"{name}: fault accepted or too close " \
                    f"to rest a test on (err/bound {r:.3g})"


def test_wa_loss_every_fault_is_seeded_somewhere():
    """The per-shape filter above must not silently drop a fault family."""
    s, t, y = R.loss_inputs(37, 300, 257, 1, torch.bfloat16)
    names = set(_loss_faults(s, t, y, 0.1, 0.37, True, 1))
    assert names == {"smoothing_dropped", "T_applied_once", "kd_over_Ck-1",
                     "target_off_by_one", "cols_ge_256_unwritten",
                     "mean_over_64", "upstream_ignored"}


def test_wa_loss_scalar_rejects_dropped_smoothing():
    """The total loss without the smoothing term is rejected (``_cmp`` with
    test_wa_loss_gpu's tolerances accepts it)."""
    s, t, y = R.loss_inputs(37, 300, 257, 1, torch.bfloat16)
    ref = R.loss_ref(s, t, y, 0.1, T, LAM)
    bad = R.loss_ref(s, t, y, 0.0, T, LAM)
    for k in ("total", "ce"):
        r = R.scalar_worst(torch.tensor(bad[k]).float(), ref, k)
        assert r > 10.0, f"{k} without smoothing accepted ({r:.3g})"


@pytest.mark.parametrize("scale", R.SCALES)
@pytest.mark.parametrize("shape", R.CE_SHAPES, ids=str)
def test_ce_kd_cpu_path_accepted_faults_rejected(shape, scale):
    M, C = shape
    s, t, y = R.loss_inputs(M, C, C, scale, torch.float32)
    for smooth, up in ((0.0, 1.0), (0.1, 0.37)):
        ref = R.loss_ref(s, None, y, smooth, T, 0.0, up, bf16_grad=False)
        x = s.clone().requires_grad_(True)
        loss = CF.cross_entropy(x, y, smooth)
        (loss * up).backward()
        R.loss_check(dict(total=loss), x.grad, ref,
                     f"cpu ce {shape} x{scale} s{smooth} up{up}")
        for name, bad in _loss_faults(s, None, y, smooth, up, True,
                                      scale).items():
            r = R.grad_worst(bad.float(), ref)
            assert r > 10.0, f"ce {name}: fault accepted ({r:.3g})"
    for up in (1.0, 0.37):
        ref = R.loss_ref(s, t, y, 0.0, T, 1.0, up, ce=False, bf16_grad=False)
        x = s.clone().requires_grad_(True)
        loss = CF.kd_loss(x, t, T)
        (loss * up).backward()
        R.loss_check(dict(total=loss, kd=loss), x.grad, ref,
                     f"cpu kd {shape} x{scale} up{up}")
        for name, bad in _loss_faults(s, t, y, 0.0, up, False,
                                      scale).items():
            r = R.grad_worst(bad.float(), ref)
            assert r > 10.0, f"kd {name}: fault accepted ({r:.3g})"


def _cmp_accepts(got, ref, **kw):
    try:
        _cmp(got, ref, **kw)
    except AssertionError:
        return False
    return True


def test_whole_tensor_cmp_accepts_zero_gradient():
    """Why the per-element allowance exists. With test_wa_loss_gpu's own data
    and tolerances (rtol 2e-2, atol 2e-3) ``_cmp`` allows 0.022 on every
    element of a gradient whose largest element is ~0.014: it ACCEPTS an
    all-zero gradient, one without the KD term and one without label
    smoothing. The per-element comparator rejects all three."""
    torch.manual_seed(40)
    M, C, Ck = 64, 110, 90
    s = torch.randn(M, C).to(torch.bfloat16)
    t = torch.randn(M, Ck).to(torch.bfloat16)
    y = torch.randint(0, C, (M,))
    x = s.clone().requires_grad_(True)
    CF.wa_loss(x, t, y, 0.1, 2.0, 0.5)[0].backward()
    good = x.grad
    assert good.float().abs().max() < 0.022
    ref = R.loss_ref(s, t, y, 0.1, 2.0, 0.5)
    assert R.grad_worst(good, ref) <= 1.0
    bads = {"zero": torch.zeros_like(good),
            "no_kd": _grad_formula(s, None, y, 0.1, 2.0, 0.5, 1.0),
            "no_smoothing": _grad_formula(s, t, y, 0.0, 2.0, 0.5, 1.0)}
    for name, bad in bads.items():
        bad = bad.to(torch.bfloat16)
        assert _cmp_accepts(bad, good, rtol=2e-2, atol=2e-3), \
            f"_cmp rejected the {name} gradient"
        assert R.grad_worst(bad, ref) > 1.0, \
            f"per-element comparator accepted the {name} gradient"


# --------------------------------------------------------------------- linear

def test_split_factors_pinned():
    """cilfw_linear_ksplit is pure host code: the (fwd, dx, dW) split factor
    of every shape of test_head_gpu.py is pinned without a GPU. A failure
    here after a retune needs a new smallest shape, not a relaxed assertion."""
    from cilfw import _hip_ops as H
    for (M, N, K), splits in R.LINEAR_SHAPES:
        assert H.linear_ksplits(M, N, K) == splits, (M, N, K)
    # the facts the issue was written from
    assert H.linear_ksplits(128, 100, 512) == (4, 1, 1)
    assert H.linear_ksplits(37, 13, 64) == (1, 1, 1)
    assert H.linear_ksplits(128, 1000, 2048)[:2] == (8, 4)


def test_topk_refuses_maxk_out_of_range():
    """Raised before any launch (CPU tensors never reach a kernel)."""
    from cilfw import _hip_ops as H
    lg, y = torch.zeros(2, 20), torch.zeros(2, dtype=torch.long)
    for maxk in (0, 9, -1):
        with pytest.raises(ValueError, match="maxk"):
            H.topk_correct(lg, y, maxk)


@pytest.mark.parametrize("shape,splits", R.LINEAR_SHAPES, ids=R.LINEAR_IDS)
def test_linear_cpu_path_accepted(shape, splits):
    M, N, K = shape
    x, w, b, dy = R.linear_inputs(M, N, K)
    for bias in (b, None):
        ref = R.linear_ref(x, w, bias, dy, splits)
        xg = x.clone().requires_grad_(True)
        wg = w.float().requires_grad_(True)
        bg = bias.clone().requires_grad_(True) if bias is not None else None
        yv = CF.linear(xg, wg, bg)
        yv.backward(dy)
        R.linear_check(yv, ref["y"], f"cpu linear {shape} y")
        R.linear_check(xg.grad, ref["dx"], f"cpu linear {shape} dx")
        R.linear_check(wg.grad, ref["dw"], f"cpu linear {shape} dw")
        if bias is not None:
            R.linear_check(bg.grad, ref["db"], f"cpu linear {shape} db")
        # the correctly rounded fp64 reference itself
        assert R.linear_worst(ref["y"][0].to(torch.bfloat16), ref["y"]) <= 1
        assert R.linear_worst(ref["dw"][0].float(), ref["dw"]) <= 1


def _bf(t):
    return t.to(torch.bfloat16)


def _steps_of_slab(K, ks, slab):
    """[k0, k1) that gemm_kernel's slice ``slab`` of ``ks`` covers."""
    nk = -(-K // 32)
    steps = -(-nk // ks)
    return min(slab * steps * 32, K), min((slab + 1) * steps * 32, K)


def test_linear_faults_rejected():
    """Six seeded faults of the forward GEMM, and the slab / row faults for
    dx (bf16) and dW (fp32)."""
    # -- (70, 67, 40): two blocks each way, ragged K tail
    (M, N, K), splits = R.LINEAR_SHAPES[0]
    x, w, b, dy = R.linear_inputs(M, N, K)
    ref = R.linear_ref(x, w, b, dy, splits)
    y = ref["y"][0]
    bad = {}
    x1 = x.clone()
    x1[:, 0:32] = 0
    bad["k_step_dropped"] = _bf(R.linear_ref(x1, w, b, dy, splits)["y"][0])
    x2 = x.clone()
    x2[:, 32:] = 0
    bad["k_tail_dropped"] = _bf(R.linear_ref(x2, w, b, dy, splits)["y"][0])
    y3 = y.clone()
    blk = y3[16:32, 16:32]
    blk.copy_(blk.t().clone())
    bad["block_transposed"] = _bf(y3)
    y4 = y.clone()
    y4[-1] = 0
    bad["last_row_unwritten"] = _bf(y4)
    for name, got in bad.items():
        r = R.linear_worst(got, ref["y"])
        assert r > 1.0, f"{name}: fault accepted (err/bound {r:.3g})"

    # -- (37, 13, 520): forward split 4, ragged last slice
    (M, N, K), splits = R.LINEAR_SHAPES[2]
    x, w, b, dy = R.linear_inputs(M, N, K)
    ref = R.linear_ref(x, w, b, dy, splits)
    bad = {}
    for slab in (1, 3):
        k0, k1 = _steps_of_slab(K, splits[0], slab)
        assert k0 < k1 <= K
        xs = x.clone()
        xs[:, k0:k1] = 0
        bad[f"slab{slab}_left_out"] = _bf(
            R.linear_ref(xs, w, b, dy, splits)["y"][0])
    assert _steps_of_slab(K, splits[0], 3) == (480, 520)
    xt = x.clone()
    xt[:, 512:] = 0
    bad["k_tail_dropped"] = _bf(R.linear_ref(xt, w, b, dy, splits)["y"][0])
    bad["bias_in_every_slab"] = _bf(ref["y"][0]
                                    + (splits[0] - 1) * b.double())
    for name, got in bad.items():
        r = R.linear_worst(got, ref["y"])
        assert r > 1.0, f"{name}: fault accepted (err/bound {r:.3g})"

    # -- dx split (37, 300, 72): slab 1 = classes [160, 300)
    (M, N, K), splits = R.LINEAR_SHAPES[3]
    x, w, b, dy = R.linear_inputs(M, N, K)
    ref = R.linear_ref(x, w, b, dy, splits)
    k0, k1 = _steps_of_slab(N, splits[1], 1)
    dys = dy.clone()
    dys[:, k0:k1] = 0
    got = _bf(R.linear_ref(x, w, b, dys, splits)["dx"][0])
    assert R.linear_worst(got, ref["dx"]) > 1.0
    got = ref["dx"][0].clone()
    got[-1] = 0
    assert R.linear_worst(_bf(got), ref["dx"]) > 1.0

    # -- dW split (300, 13, 72): slab 1 = rows [160, 300)
    (M, N, K), splits = R.LINEAR_SHAPES[4]
    x, w, b, dy = R.linear_inputs(M, N, K)
    ref = R.linear_ref(x, w, b, dy, splits)
    k0, k1 = _steps_of_slab(M, splits[2], 1)
    xs = x.clone()
    xs[k0:k1] = 0
    got = R.linear_ref(xs, w, b, dy, splits)["dw"][0].float()
    assert R.linear_worst(got, ref["dw"]) > 1.0
    got = ref["dw"][0].float().clone()
    got[-1] = 0
    assert R.linear_worst(got, ref["dw"]) > 1.0
    got = ref["db"][0].float().clone()
    got[-1] -= dy[-1, -1].float()           # db misses the last batch row
    assert R.linear_worst(got, ref["db"]) > 1.0


# ---------------------------------------------------------------------- top-k

def test_topk_reference():
    """The exact reference agrees with torch.topk where there are no ties,
    and with the constructed rows where there are."""
    g = torch.Generator().manual_seed(5)
    lg = torch.randn(64, 50, generator=g, dtype=torch.float64)
    y = torch.randint(0, 50, (64,), generator=g)
    want = [int(lg.topk(k, 1).indices.eq(y.view(-1, 1)).any(1).sum())
            for k in range(1, 6)]
    assert R.topk_ref(lg, y, 5).tolist() == want
    lg, y, counts = R.topk_constructed()
    assert R.topk_ref(lg, y, 5).tolist() == counts.tolist()


@pytest.mark.parametrize("M,C,maxk", R.TOPK_CASES)
def test_topk_cases_tell_wrong_kernels_apart(M, C, maxk):
    """The data of test_head_gpu.py's top-k cases: the expected counts are
    non-trivial, a kernel whose ties go to the higher index or that reads
    only the first 256 columns would give other counts (asserted inside),
    and so would one that never finds the target or stops one pass early."""
    lg, y = R.topk_case(M, C, maxk)
    assert torch.equal(lg, lg.to(torch.bfloat16).float())
    want = R.topk_case_is_telling(lg, y, maxk)
    assert want.tolist() == sorted(want.tolist())       # cumulative in k
    if M > maxk + 1:
        # targets sit at ranks 0..maxk (handing one to a column >= 256 can
        # move it by one within its tie group): hits at k = 1, more hits at
        # larger k, and rows that still miss at k = maxk
        assert 0 < want[0] < want[-1] < M
        assert len(set(want.tolist())) >= min(maxk, 3)
    if C > 256:
        assert (y >= 256).any() and (y < 256).any()
