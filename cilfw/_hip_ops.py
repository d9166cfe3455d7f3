"""ctypes bridge to the in-tree HIP kernel library (cilfw/_hip_lib.so).

Raises ImportError at import time when the library isn't built — ``ops._backend``
then refuses to run GPU compute (no silent ATen fallback).

Every function allocates outputs with torch (same allocator/stream semantics as
the rest of the program) and launches the hand-written gfx950 kernels on the
CURRENT torch HIP stream, so ordering with surrounding torch ops is implicit and
hipGraph capture of a training step captures these launches too.
"""

import ctypes
import os

import torch

from . import _herding_checks as _hc

_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                         "_hip_lib.so")
if not os.path.exists(_LIB_PATH):
    raise ImportError(f"cilfw HIP library not built: {_LIB_PATH}")
_lib = ctypes.CDLL(_LIB_PATH)

_DEBUG = os.environ.get("CILFW_SYNC_DEBUG") == "1"

c_vp = ctypes.c_void_p
c_i = ctypes.c_int
c_l = ctypes.c_long
c_f = ctypes.c_float

_lib.cilfw_sync.restype = c_i
_lib.cilfw_error_string.restype = ctypes.c_char_p
_lib.cilfw_error_string.argtypes = [c_i]

# Explicit prototypes: ctypes cannot catch arity/type mismatches on its own and
# a wrong call corrupts device memory (see gap_bwd incident, round 1).
_PROTOS = {
    "cilfw_conv2d_fwd": [c_vp] * 4 + [c_i] * 12 + [c_vp, c_vp],
    "cilfw_conv2d_bwd_data": [c_vp] * 4 + [c_i] * 12 + [c_vp] * 5 + [c_i, c_vp],
    "cilfw_conv2d_bwd_weight": [c_vp] * 4 + [c_i] * 13 + [c_vp],
    "cilfw_fill_mtable": [c_vp] + [c_i] * 4 + [c_vp],
    "cilfw_im2col_smallc": [c_vp] * 3 + [c_i] * 11 + [c_vp],
    "cilfw_bn_apply_only": [c_vp] * 7 + [c_l, c_i, c_i, c_vp],
    "cilfw_bn_fwd": [c_vp] * 11 + [c_i, c_l, c_i, c_f, c_f, c_i, c_i, c_vp],
    "cilfw_bn_bwd": [c_vp] * 11 + [c_vp, c_i] + [c_l, c_i, c_i, c_i, c_vp],
    "cilfw_add_relu_fwd": [c_vp] * 3 + [c_l, c_vp],
    "cilfw_add_relu_bwd": [c_vp] * 3 + [c_l, c_vp],
    "cilfw_add_relu_tap_fwd": [c_vp] * 4 + [c_l, c_vp],
    "cilfw_add_relu_tap_bwd": [c_vp] * 4 + [c_l, c_vp],
    "cilfw_downsample_a_fwd": [c_vp] * 2 + [c_i] * 4 + [c_vp],
    "cilfw_downsample_a_bwd": [c_vp] * 2 + [c_i] * 4 + [c_vp],
    "cilfw_gap_fwd": [c_vp] * 2 + [c_i] * 3 + [c_vp],
    "cilfw_gap_bwd": [c_vp] * 2 + [c_i] * 3 + [c_vp],
    "cilfw_stride_gather": [c_vp] * 2 + [c_i] * 7 + [c_vp],
    "cilfw_stride_scatter": [c_vp] * 2 + [c_i] * 7 + [c_vp],
    "cilfw_maxpool_fwd": [c_vp] * 3 + [c_i] * 9 + [c_vp],
    "cilfw_maxpool_bwd": [c_vp] * 3 + [c_i] * 9 + [c_vp],
    "cilfw_linear_fwd": [c_vp] * 5 + [c_i] * 4 + [c_vp],
    "cilfw_linear_dx": [c_vp] * 4 + [c_i] * 4 + [c_vp],
    "cilfw_linear_dw": [c_vp] * 5 + [c_i] * 4 + [c_vp],
    "cilfw_ce_fwd": [c_vp] * 5 + [c_i, c_i, c_f, c_vp],
    "cilfw_ce_bwd": [c_vp] * 4 + [c_i, c_i, c_f, c_vp],
    "cilfw_kd_fwd": [c_vp] * 6 + [c_i, c_i, c_f, c_vp],
    "cilfw_kd_bwd": [c_vp] * 4 + [c_i, c_i, c_f, c_vp],
    "cilfw_wa_loss_fwd": [c_vp] * 8 + [c_i] * 3 + [c_f] * 3 + [c_vp],
    "cilfw_wa_loss_bwd": [c_vp] * 6 + [c_i] * 3 + [c_f] * 3 + [c_vp],
    "cilfw_sgd_step": [c_vp] * 4 + [c_l, c_vp, c_f, c_f, c_vp],
    "cilfw_topk_correct": [c_vp] * 3 + [c_i] * 3 + [c_vp],
    "cilfw_herding_select": [c_vp] * 3 + [c_i] * 3 + [c_vp],
    "cilfw_herding_select_batch": [c_vp] * 6 + [c_i] * 3 + [c_vp],
    "cilfw_crop_resize": [c_vp] * 7 + [c_i] * 7 + [c_vp],
    "cilfw_crop_resize_ragged": [c_vp] * 9 + [c_i] * 5 + [c_vp],
    "cilfw_nme_prototypes": [c_vp] * 3 + [c_i] * 2 + [c_vp],
    "cilfw_nme_topk": [c_vp] * 6 + [c_i] * 4 + [c_vp],
    "cilfw_pod_pool": [c_vp] * 2 + [c_i] * 4 + [c_vp],
    "cilfw_pod_dist": [c_vp] * 5 + [c_i] * 2 + [c_vp],
    "cilfw_pod_bwd": [c_vp] * 4 + [c_i] * 4 + [c_vp],
    "cilfw_rownorm_fwd": [c_vp] * 4 + [c_i] * 3 + [c_vp],
    "cilfw_rownorm_bwd": [c_vp] * 6 + [c_i] * 3 + [c_vp],
    "cilfw_cos_sum": [c_vp] * 2 + [c_i, c_f, c_vp],
    "cilfw_flat_dist": [c_vp] * 5 + [c_i] * 2 + [c_vp],
    "cilfw_flat_bwd": [c_vp] * 3 + [c_i] * 2 + [c_vp],
    "cilfw_mrank_fwd": [c_vp] * 9 + [c_i] * 4 + [c_f, c_vp],
    "cilfw_mrank_bwd": [c_vp] * 6 + [c_i] * 4 + [c_vp],
    "cilfw_lsc_reduce_fwd": [c_vp] * 4 + [c_i] * 3 + [c_f, c_vp],
    "cilfw_lsc_reduce_bwd": [c_vp] * 6 + [c_i] * 3 + [c_f, c_vp],
    "cilfw_nca_fwd": [c_vp] * 8 + [c_i] * 2 + [c_f, c_vp],
    "cilfw_nca_bwd": [c_vp] * 8 + [c_i] * 2 + [c_vp],
    "cilfw_kmeans_proxies": [c_vp] * 8 + [c_i] * 5 + [c_vp],
}
for _name, _args in _PROTOS.items():
    _fn = getattr(_lib, _name)
    _fn.argtypes = _args
    _fn.restype = None

_lib.cilfw_conv2d_bwd_data.restype = c_i  # 1 = BN partials were emitted
for _name in ("cilfw_pod_pool", "cilfw_pod_dist", "cilfw_pod_bwd",
              "cilfw_rownorm_fwd", "cilfw_rownorm_bwd", "cilfw_cos_sum",
              "cilfw_flat_dist", "cilfw_flat_bwd", "cilfw_mrank_fwd",
              "cilfw_mrank_bwd", "cilfw_lsc_reduce_fwd",
              "cilfw_lsc_reduce_bwd", "cilfw_nca_fwd", "cilfw_nca_bwd",
              "cilfw_kmeans_proxies"):
    getattr(_lib, _name).restype = c_i  # 1 = shape refused, nothing launched

for _name, _n in [("cilfw_linear_ksplit", 3),
                  ("cilfw_conv2d_fwd_ksplit", 7),
                  ("cilfw_conv2d_bwd_data_ksplit", 7),
                  ("cilfw_conv2d_bwd_data_can_fuse_bn", 8),
                  ("cilfw_conv2d_bwd_data_bn_gy", 3),
                  ("cilfw_conv2d_fwd_bn_gy", 3),
                  ("cilfw_bnbwd_fuse_enabled", 0),
                  ("cilfw_conv2d_bwd_weight_nslices", 7),
                  ("cilfw_conv2d_fwd_route", 8),
                  ("cilfw_conv2d_bwd_data_route", 9),
                  ("cilfw_conv2d_bwd_weight_route", 8),
                  ("cilfw_pod_supported", 4),
                  ("cilfw_pod_pool_groups", 2),
                  ("cilfw_cosine_supported", 3),
                  ("cilfw_mrank_supported", 4),
                  ("cilfw_lsc_supported", 3),
                  ("cilfw_nca_supported", 2),
                  ("cilfw_kmeans_supported", 3)]:
    _fn = getattr(_lib, _name)
    _fn.argtypes = [c_i] * _n
    _fn.restype = c_i
_lib.cilfw_bn_sums_gy.argtypes = [c_l]
_lib.cilfw_bn_sums_gy.restype = c_i

# route codes of csrc/conv.hip (enum order); the launchers branch on the same
# C functions these queries call
_FWD_ROUTES = ("v1_bk32", "v1_bk64", "v2_bn64", "v2_bn128")
_BWD_DATA_ROUTES = ("s2_fused", "v2", "v1_bk32", "v1_bk64")
_BWD_WEIGHT_ROUTES = ("v2", "v1_fast", "v1_generic")


def _stream():
    return c_vp(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return c_vp(0 if t is None else t.data_ptr())


def _check(name):
    if _DEBUG:
        e = _lib.cilfw_sync()
        if e != 0:
            raise RuntimeError(
                f"HIP error after {name}: "
                f"{_lib.cilfw_error_string(e).decode()}")


def _bf16(t, name):
    assert t.dtype == torch.bfloat16, \
        f"{name}: GPU compute path is bf16 (got {t.dtype}); run with " \
        f"--dtype bf16 or set CILFW_FORCE_TORCH=1 for debugging"
    assert t.is_contiguous(), f"{name}: needs contiguous tensor"
    return t


# ------------------------------------------------------------------------ conv

def _out_hw(H, W_, R, S, stride, pad):
    return ((H + 2 * pad - R) // stride + 1,
            (W_ + 2 * pad - S) // stride + 1)


def _crs_pad(C, R, S):
    """C*R*S rounded up to the 16-element k-chunks of the fast GEMM path:
    row length of the padded stem im2col."""
    return (C * R * S + 15) // 16 * 16


def _slab_ws(nslabs, numel, device, always=False):
    """fp32 split-K workspace [nslabs][numel]; None when a single slice
    stores its result directly (bwd-weight ``always`` goes through slabs)."""
    if nslabs > 1 or always:
        return torch.empty(nslabs * numel, dtype=torch.float32, device=device)
    return None


def _stem_as_1x1(x, R, S, stride, pad, Ho, Wo):
    """Padded im2col for tiny-C stems: x as the (M, 1, 1, CRSpad) bf16 input
    of a 1x1 conv (pad columns zero)."""
    N, H, W_, C = x.shape
    M, CRSpad = N * Ho * Wo, _crs_pad(C, R, S)
    mt = _mtable(N, Ho, Wo, stride, x.device)
    col = torch.zeros(M, 1, 1, CRSpad, dtype=torch.bfloat16, device=x.device)
    _lib.cilfw_im2col_smallc(_ptr(x), _ptr(mt), _ptr(col), c_i(N), c_i(H),
                             c_i(W_), c_i(C), c_i(R), c_i(S), c_i(stride),
                             c_i(pad), c_i(Ho), c_i(Wo), c_i(CRSpad),
                             _stream())
    _check("im2col_smallc")
    return col


def conv2d_fwd_route(N, H, W_, C, K, R, S, stride, pad):
    """(route name, ksplit) conv2d_fwd takes for this geometry outside graph
    capture: v1_bk32 | v1_bk64 | v2_bn64 | v2_bn128."""
    Ho, Wo = _out_hw(H, W_, R, S, stride, pad)
    ks = _lib.cilfw_conv2d_fwd_ksplit(N, C, K, R, S, Ho, Wo)
    return _FWD_ROUTES[_lib.cilfw_conv2d_fwd_route(N, C, K, R, S, Ho, Wo,
                                                   ks)], ks


def conv2d_bwd_data_route(N, H, W_, C, K, R, S, stride):
    """(route name, ksplit) conv2d_bwd_data takes for dx of shape (N,H,W_,C):
    s2_fused | v2 | v1_bk32 | v1_bk64. A strided 1x1 is solved on its
    subsampled stride-1 grid, exactly as conv2d_bwd_data does."""
    if R == 1 and S == 1 and stride > 1:
        H, W_, stride = (H - 1) // stride + 1, (W_ - 1) // stride + 1, 1
    ks = _lib.cilfw_conv2d_bwd_data_ksplit(N, H, W_, C, K, R, S)
    return _BWD_DATA_ROUTES[_lib.cilfw_conv2d_bwd_data_route(
        N, H, W_, C, K, R, S, stride, ks)], ks


def bnbwd_fuse_enabled():
    """CILFW_BNBWD_FUSE, as csrc/conv.hip (the knob's one reader) sees it."""
    return bool(_lib.cilfw_bnbwd_fuse_enabled())


def _stem_im2col_dw(C, K, R, S):
    """7x7 stems (ImageNet): the per-element gather path measured 542 us on
    the 224^2 stem dW; padded-im2col + flat fast-path GEMM is far cheaper
    there (3x3 CIFAR stems measured better on the direct gather)."""
    use_im2col = (os.environ.get("CILFW_STEM_IM2COL") == "1"
                  or (R * S >= 25
                      and os.environ.get("CILFW_STEM_IM2COL") != "0"))
    return C < 16 and R * S > 1 and K % 16 == 0 and use_im2col


def conv2d_bwd_weight_route(N, C, K, R, S, Ho, Wo, accum=False):
    """(route name, nslices) conv2d_bwd_weight takes: v2 | v1_fast |
    v1_generic. Tiny-C stems on the im2col route run the flat GEMM over the
    padded (M, CRSpad) columns, which never accumulates in-kernel."""
    if _stem_im2col_dw(C, K, R, S):
        N, C, R, S, Ho, Wo = N * Ho * Wo, _crs_pad(C, R, S), 1, 1, 1, 1
        accum = False
    ns = _lib.cilfw_conv2d_bwd_weight_nslices(N, C, K, R, S, Ho, Wo)
    return _BWD_WEIGHT_ROUTES[_lib.cilfw_conv2d_bwd_weight_route(
        N, C, K, R, S, Ho, Wo, 1 if accum else 0)], ns


def conv2d_fwd(x, w, stride, pad, want_bn_parts=False):
    """want_bn_parts: also produce per-M-block per-channel (sum, sumsq)
    partials of y in the conv epilogue — a following training-mode BN skips
    its own bn_sums pass (and a full re-read of y). Returns (y, parts|None):
    parts is (gy, 2, K) fp32, None when the shape routed off the v2 kernel or used split-K."""
    _bf16(x, "conv2d_fwd.x")
    _bf16(w, "conv2d_fwd.w")
    N, H, W_, C = x.shape
    R, S, Cw, K = w.shape
    assert Cw == C
    assert K % 8 == 0, "conv kernels vector-stage over output channels (K%8==0)"
    Ho, Wo = _out_hw(H, W_, R, S, stride, pad)
    if C < 16 and R * S > 1 and K % 16 == 0 \
            and os.environ.get("CILFW_STEM_IM2COL") == "1":
        # measured: the generic gather already fills the chip at stem sizes —
        # this alternate path is kept for experiments (CILFW_STEM_IM2COL=1):
        # a 1x1 conv over the padded im2col columns
        col = _stem_as_1x1(x, R, S, stride, pad, Ho, Wo)
        wpad = torch.zeros(1, 1, col.shape[-1], K, dtype=torch.bfloat16,
                           device=x.device)
        wpad[0, 0, :C * R * S] = w.reshape(C * R * S, K)
        y, _ = conv2d_fwd(col, wpad, 1, 0)
        return y.view(N, Ho, Wo, K), None
    y = torch.empty(N, Ho, Wo, K, dtype=torch.bfloat16, device=x.device)
    ks = _lib.cilfw_conv2d_fwd_ksplit(N, C, K, R, S, Ho, Wo)
    ws = _slab_ws(ks, y.numel(), x.device)
    parts = None
    # the BN-statistics epilogue lives in the v2 kernels' ksplit==1 stores
    if want_bn_parts and ks == 1 \
            and _FWD_ROUTES[_lib.cilfw_conv2d_fwd_route(
                N, C, K, R, S, Ho, Wo, ks)].startswith("v2_") \
            and os.environ.get("CILFW_CONV_BN_FUSE", "1") != "0":
        parts = torch.empty(_lib.cilfw_conv2d_fwd_bn_gy(N, Ho, Wo), 2, K,
                            dtype=torch.float32, device=x.device)
    _lib.cilfw_conv2d_fwd(_ptr(x), _ptr(w), _ptr(y), _ptr(ws), c_i(N),
                          c_i(H), c_i(W_), c_i(C), c_i(K), c_i(R), c_i(S),
                          c_i(stride), c_i(pad), c_i(Ho), c_i(Wo), c_i(ks),
                          _ptr(parts), _stream())
    _check("conv2d_fwd")
    return y, parts


def conv2d_bwd_data(dy, w, stride, pad, H, W_, bn_meta=None):
    """bn_meta = (bn_y, bn_x, bn_mean, bn_invstd, bn_relu): this conv's input
    is a training BN(+ReLU) output with a single consumer — the kernel
    epilogue then also emits that BN's backward (dgamma, dbeta) partials so
    the BN can skip its sums pass. Returns (dx, parts-or-None) when bn_meta
    is given, plain dx otherwise."""
    _bf16(dy, "conv2d_bwd_data.dy")
    N, Ho, Wo, K = dy.shape
    R, S, C, Kw = w.shape
    assert Kw == K
    if R == 1 and S == 1 and stride > 1:
        # strided 1x1 projection: 3/4 of positions are structurally zero —
        # solve on the subsampled (stride-1) grid, then scatter
        dxs = conv2d_bwd_data(dy, w, 1, 0, Ho, Wo)
        dx = torch.empty(N, H, W_, C, dtype=torch.bfloat16, device=dy.device)
        _lib.cilfw_stride_scatter(_ptr(dxs), _ptr(dx), c_i(N), c_i(H),
                                  c_i(W_), c_i(C), c_i(stride), c_i(Ho),
                                  c_i(Wo), _stream())
        _check("stride_scatter")
        # keep the return shape contract: callers that passed bn_meta unpack
        # a (dx, parts) pair (no fusion on the strided-1x1 scatter path)
        return (dx, None) if bn_meta is not None else dx
    dx = torch.empty(N, H, W_, C, dtype=torch.bfloat16, device=dy.device)
    ks = _lib.cilfw_conv2d_bwd_data_ksplit(N, H, W_, C, K, R, S)
    ws = _slab_ws(ks, dx.numel(), dy.device)
    parts = None
    bn_y = bn_x = bn_mean = bn_invstd = None  # null pointers: nothing fused
    bn_relu = False
    if (bn_meta is not None
            and _lib.cilfw_conv2d_bwd_data_can_fuse_bn(
                N, H, W_, C, K, R, S, stride)):
        bn_y, bn_x, bn_mean, bn_invstd, bn_relu = bn_meta
        parts = torch.empty(_lib.cilfw_conv2d_bwd_data_bn_gy(N, H, W_), 2, C,
                            dtype=torch.float32, device=dy.device)
    fused = _lib.cilfw_conv2d_bwd_data(
        _ptr(dy), _ptr(w), _ptr(dx), _ptr(ws), c_i(N), c_i(H), c_i(W_),
        c_i(C), c_i(K), c_i(R), c_i(S), c_i(stride), c_i(pad), c_i(Ho),
        c_i(Wo), c_i(ks), _ptr(bn_y), _ptr(bn_x), _ptr(bn_mean),
        _ptr(bn_invstd), _ptr(parts), c_i(1 if bn_relu else 0), _stream())
    if not fused:
        parts = None
    _check("conv2d_bwd_data")
    if bn_meta is not None:
        return dx, parts
    return dx


_mtable_cache = {}


def _mtable(N, Ho, Wo, stride, device):
    """Packed im2col pixel table mt[m] = n<<20 | ho*stride<<10 | wo*stride,
    built once per conv geometry and cached for the process lifetime."""
    key = (N, Ho, Wo, stride, device)
    mt = _mtable_cache.get(key)
    if mt is None:
        assert N < 4096 and Ho * stride < 1024 and Wo * stride < 1024, \
            "mtable packing limits exceeded"
        M = N * Ho * Wo
        mt = torch.empty(M, dtype=torch.int32, device=device)
        _lib.cilfw_fill_mtable(_ptr(mt), c_i(M), c_i(Ho * Wo), c_i(Wo),
                               c_i(stride), _stream())
        _mtable_cache[key] = mt
    return mt


def conv2d_bwd_weight(dy, x, stride, pad, R, S, out=None, accum=False):
    """dW (R,S,C,K) fp32. With ``out`` the reduce writes straight into the
    given buffer (the DataParallelEngine's flat-grad slot — no AccumulateGrad
    add); ``accum=True`` adds instead of overwriting (grad accumulation)."""
    _bf16(dy, "conv2d_bwd_weight.dy")
    _bf16(x, "conv2d_bwd_weight.x")
    N, H, W_, C = x.shape
    _, Ho, Wo, K = dy.shape
    if _stem_im2col_dw(C, K, R, S):
        # dW of the 1x1 conv over the padded im2col columns; pad rows dropped
        col = _stem_as_1x1(x, R, S, stride, pad, Ho, Wo)
        dwp = conv2d_bwd_weight(dy.view(-1, 1, 1, K), col, 1, 0, 1, 1)
        dw = dwp.view(-1, K)[:C * R * S].reshape(R, S, C, K)
        if out is None:
            return dw
        (out.add_(dw) if accum else out.copy_(dw))
        return out
    if R == 1 and S == 1 and stride > 1:
        xg = torch.empty(N, Ho, Wo, C, dtype=torch.bfloat16, device=x.device)
        _lib.cilfw_stride_gather(_ptr(x), _ptr(xg), c_i(N), c_i(H), c_i(W_),
                                 c_i(C), c_i(stride), c_i(Ho), c_i(Wo),
                                 _stream())
        _check("stride_gather")
        return conv2d_bwd_weight(dy, xg, 1, 0, R, S, out=out, accum=accum)
    if out is None:
        dw = torch.empty(R, S, C, K, dtype=torch.float32, device=dy.device)
        accum = False
    else:
        assert out.is_contiguous() and out.dtype == torch.float32 \
            and out.shape == (R, S, C, K)
        dw = out
    ns = _lib.cilfw_conv2d_bwd_weight_nslices(N, C, K, R, S, Ho, Wo)
    ws = _slab_ws(ns, dw.numel(), dy.device, always=True)
    _lib.cilfw_conv2d_bwd_weight(_ptr(dy), _ptr(x), _ptr(dw),
                                 _ptr(ws), c_i(N), c_i(H), c_i(W_), c_i(C),
                                 c_i(K), c_i(R), c_i(S), c_i(stride),
                                 c_i(pad), c_i(Ho), c_i(Wo), c_i(ns),
                                 c_i(1 if accum else 0), _stream())
    _check("conv2d_bwd_weight")
    return dw


# -------------------------------------------------------------------------- bn

def bn_fwd(x, gamma, beta, running_mean, running_var, momentum, eps, training,
           relu, residual=None, ext_parts=None):
    """ext_parts: (gy, 2, C) per-M-block (sum, sumsq) partials produced by the
    conv that made x (conv2d_fwd want_bn_parts) — skips the bn_sums pass."""
    _bf16(x, "bn_fwd.x")
    if residual is not None:
        _bf16(residual, "bn_fwd.residual")
        # the apply kernel indexes the residual by x's extent
        assert residual.shape == x.shape, \
            f"bn_fwd: residual {tuple(residual.shape)} vs x {tuple(x.shape)}"
    frozen = (None if training
              else getattr(running_mean, "_cilfw_frozen", None))
    if frozen is not None:
        mean, invstd = frozen
        C = x.shape[-1]
        assert C % 8 == 0, "bn kernels vectorize over channels (C%8==0)"
        M = x.numel() // C
        y = torch.empty_like(x)
        gf = gamma.float().contiguous()
        bf = beta.float().contiguous()
        _lib.cilfw_bn_apply_only(_ptr(x), _ptr(y), _ptr(residual), _ptr(gf),
                                 _ptr(bf), _ptr(mean), _ptr(invstd),
                                 c_l(M * C), c_i(C),
                                 c_i(1 if relu else 0), _stream())
        _check("bn_apply_only")
        return y, mean, invstd
    C = x.shape[-1]
    assert C % 8 == 0, "bn kernels vectorize over channels (C%8==0)"
    M = x.numel() // C
    y = torch.empty_like(x)
    mean = torch.empty(C, dtype=torch.float32, device=x.device)
    invstd = torch.empty(C, dtype=torch.float32, device=x.device)
    gy = _lib.cilfw_bn_sums_gy(M)
    scratch = torch.empty((gy + 1) * 2 * C, dtype=torch.float32,
                          device=x.device)
    gf = gamma.float().contiguous()
    bf = beta.float().contiguous()
    if not training:
        ext_parts = None
    ext_gy = 0 if ext_parts is None else ext_parts.shape[0]
    _lib.cilfw_bn_fwd(_ptr(x), _ptr(y), _ptr(residual), _ptr(gf), _ptr(bf),
                      _ptr(running_mean), _ptr(running_var), _ptr(mean),
                      _ptr(invstd), _ptr(scratch), _ptr(ext_parts),
                      c_i(ext_gy), c_l(M), c_i(C),
                      c_f(momentum), c_f(eps), c_i(1 if training else 0),
                      c_i(1 if relu else 0), _stream())
    _check("bn_fwd")
    return y, mean, invstd


def bn_bwd(dy, x, gamma, mean, invstd, y, relu, training, want_dres=False,
           out_gamma=None, out_beta=None, ext_parts=None):
    """With out_gamma/out_beta the reduced per-channel grads are written
    straight into the given fp32 buffers (flat-grad slot delivery) and the
    returned dgamma/dbeta are those buffers. ext_parts: [gy][2][C]
    (dgamma, dbeta) partials already emitted by the producing conv's
    bwd-data epilogue — the sums pass over (dy, x, y) is skipped."""
    _bf16(dy, "bn_bwd.dy")
    C = x.shape[-1]
    assert C % 8 == 0, "bn kernels vectorize over channels (C%8==0)"
    assert dy.shape == x.shape and y.shape == x.shape, \
        f"bn_bwd: dy {tuple(dy.shape)} / y {tuple(y.shape)} vs x " \
        f"{tuple(x.shape)}"
    M = x.numel() // C
    dx = torch.empty_like(x)
    dres = torch.empty_like(x) if want_dres else None
    if ext_parts is not None:
        ext_gy = ext_parts.shape[0]
        dgb = torch.empty(2 * C, dtype=torch.float32, device=x.device)
        base = 0
    else:
        ext_gy = 0
        gy = _lib.cilfw_bn_sums_gy(M)
        dgb = torch.empty((gy + 1) * 2 * C, dtype=torch.float32,
                          device=x.device)
        base = gy * 2 * C
    gf = gamma.float().contiguous()
    _lib.cilfw_bn_bwd(_ptr(dy), _ptr(x), _ptr(y), _ptr(dx), _ptr(dres),
                      _ptr(gf), _ptr(mean), _ptr(invstd), _ptr(dgb),
                      _ptr(out_gamma), _ptr(out_beta),
                      _ptr(ext_parts), c_i(ext_gy),
                      c_l(M), c_i(C), c_i(1 if relu else 0),
                      c_i(1 if training else 0), _stream())
    _check("bn_bwd")
    dgamma = out_gamma if out_gamma is not None else dgb[base:base + C]
    dbeta = out_beta if out_beta is not None else dgb[base + C:base + 2 * C]
    return dx, dgamma, dbeta, dres


# ------------------------------------------------------------------ elementwise

def add_relu_fwd(a, b):
    _bf16(a, "add_relu.a")
    _bf16(b, "add_relu.b")
    assert a.shape == b.shape, \
        f"add_relu: a {tuple(a.shape)} vs b {tuple(b.shape)}"
    y = torch.empty_like(a)
    _lib.cilfw_add_relu_fwd(_ptr(a), _ptr(b), _ptr(y), c_l(a.numel()),
                            _stream())
    _check("add_relu_fwd")
    return y


def add_relu_bwd(dy, y):
    _bf16(dy, "add_relu_bwd.dy")
    assert dy.shape == y.shape, \
        f"add_relu_bwd: dy {tuple(dy.shape)} vs y {tuple(y.shape)}"
    da = torch.empty_like(dy)
    _lib.cilfw_add_relu_bwd(_ptr(dy), _ptr(y), _ptr(da), c_l(dy.numel()),
                            _stream())
    _check("add_relu_bwd")
    return da


def _tap_buf(t, ref, name):
    """bf16 buffer of ``ref``'s shape the tap kernels read or write with
    16-byte vectors."""
    _bf16(t, name)
    assert t.shape == ref.shape and t.device == ref.device, \
        f"{name}: {tuple(t.shape)} on {t.device} vs {tuple(ref.shape)} on " \
        f"{ref.device}"
    assert t.data_ptr() % 16 == 0, f"{name}: needs a 16-byte aligned tensor"
    return t


def add_relu_tap_fwd(a, b, out=None):
    """-> (y, z): z = bf16(a + b), y = relu(z), bit-identical to
    ``add_relu_fwd(a, b)``. ``out = (y, z)`` may be supplied (every element
    of both is written)."""
    _tap_buf(a, a, "add_relu_tap.a")
    _tap_buf(b, a, "add_relu_tap.b")
    y, z = out if out is not None else (torch.empty_like(a),
                                        torch.empty_like(a))
    _tap_buf(y, a, "add_relu_tap.y")
    _tap_buf(z, a, "add_relu_tap.z")
    assert y.data_ptr() != z.data_ptr() or a.numel() == 0
    _lib.cilfw_add_relu_tap_fwd(_ptr(a), _ptr(b), _ptr(y), _ptr(z),
                                c_l(a.numel()), _stream())
    _check("add_relu_tap_fwd")
    return y, z


def add_relu_tap_bwd(dy, dz, z, out=None):
    """g = bf16(dz + (z > 0 ? dy : 0)), the gradient of both inputs of
    ``add_relu_tap_fwd``. ``dz=None`` is exactly ``add_relu_bwd(dy, y)``,
    ``dy=None`` a copy of ``dz`` (one of the two must be given). ``out`` may
    be supplied (every element is written)."""
    assert dy is not None or dz is not None, \
        "add_relu_tap_bwd: needs dy or dz"
    _tap_buf(z, z, "add_relu_tap_bwd.z")
    if dy is not None:
        _tap_buf(dy, z, "add_relu_tap_bwd.dy")
    if dz is not None:
        _tap_buf(dz, z, "add_relu_tap_bwd.dz")
    if out is None:
        out = torch.empty_like(z)
    _tap_buf(out, z, "add_relu_tap_bwd.out")
    _lib.cilfw_add_relu_tap_bwd(_ptr(dy), _ptr(dz), _ptr(z), _ptr(out),
                                c_l(z.numel()), _stream())
    _check("add_relu_tap_bwd")
    return out


def downsample_a_fwd(x):
    _bf16(x, "downsample_a.x")
    N, H, W_, C = x.shape
    # AvgPool2d(1, 2) extent: the last row/column of an odd H/W is kept
    y = torch.empty(N, (H + 1) // 2, (W_ + 1) // 2, 2 * C, dtype=x.dtype,
                    device=x.device)
    _lib.cilfw_downsample_a_fwd(_ptr(x), _ptr(y), c_i(N), c_i(H), c_i(W_),
                                c_i(C), _stream())
    _check("downsample_a_fwd")
    return y


def downsample_a_bwd(dy, H, W_):
    _bf16(dy, "downsample_a_bwd.dy")
    N = dy.shape[0]
    C = dy.shape[3] // 2
    assert dy.shape == (N, (H + 1) // 2, (W_ + 1) // 2, 2 * C), \
        f"downsample_a_bwd: dy {tuple(dy.shape)} for input {H}x{W_}"
    dx = torch.empty(N, H, W_, C, dtype=dy.dtype, device=dy.device)
    _lib.cilfw_downsample_a_bwd(_ptr(dy), _ptr(dx), c_i(N), c_i(H), c_i(W_),
                                c_i(C), _stream())
    _check("downsample_a_bwd")
    return dx


def gap_fwd(x):
    _bf16(x, "gap.x")
    N, H, W_, C = x.shape
    y = torch.empty(N, C, dtype=x.dtype, device=x.device)
    _lib.cilfw_gap_fwd(_ptr(x), _ptr(y), c_i(N), c_i(H * W_), c_i(C),
                       _stream())
    _check("gap_fwd")
    return y


def gap_bwd(dy, H, W_):
    _bf16(dy, "gap_bwd.dy")
    assert dy.dim() == 2, f"gap_bwd: dy {tuple(dy.shape)} is not (N, C)"
    N, C = dy.shape
    dx = torch.empty(N, H, W_, C, dtype=dy.dtype, device=dy.device)
    _lib.cilfw_gap_bwd(_ptr(dy), _ptr(dx), c_i(N), c_i(H * W_), c_i(C),
                       _stream())
    _check("gap_bwd")
    return dx


def maxpool_fwd(x, kernel, stride, pad):
    _bf16(x, "maxpool.x")
    N, H, W_, C = x.shape
    Ho = (H + 2 * pad - kernel) // stride + 1
    Wo = (W_ + 2 * pad - kernel) // stride + 1
    y = torch.empty(N, Ho, Wo, C, dtype=x.dtype, device=x.device)
    idx = torch.empty(N, Ho, Wo, C, dtype=torch.int32, device=x.device)
    _lib.cilfw_maxpool_fwd(_ptr(x), _ptr(y), _ptr(idx), c_i(N), c_i(H),
                           c_i(W_), c_i(C), c_i(kernel), c_i(stride),
                           c_i(pad), c_i(Ho), c_i(Wo), _stream())
    _check("maxpool_fwd")
    return y, idx


def maxpool_bwd(dy, idx, H, W_, kernel, stride, pad):
    _bf16(dy, "maxpool_bwd.dy")
    N, Ho, Wo, C = dy.shape
    assert (Ho, Wo) == _out_hw(H, W_, kernel, kernel, stride, pad) \
        and idx.shape == dy.shape and idx.dtype == torch.int32 \
        and idx.is_contiguous(), \
        f"maxpool_bwd: dy {tuple(dy.shape)} / idx {tuple(idx.shape)} for " \
        f"input {H}x{W_}"
    dx = torch.empty(N, H, W_, C, dtype=dy.dtype, device=dy.device)
    _lib.cilfw_maxpool_bwd(_ptr(dy), _ptr(idx), _ptr(dx), c_i(N), c_i(H),
                           c_i(W_), c_i(C), c_i(kernel), c_i(stride),
                           c_i(pad), c_i(Ho), c_i(Wo), _stream())
    _check("maxpool_bwd")
    return dx


# ---------------------------------------------------------------------- linear

def linear_ksplits(M, N, K):
    """(fwd, dx, dW) split-K factors linear_fwd / linear_bwd launch with for
    x (M, K), w (N, K): cilfw_linear_ksplit(rows, cols, reduce length)."""
    return (_lib.cilfw_linear_ksplit(M, N, K),
            _lib.cilfw_linear_ksplit(M, K, N),
            _lib.cilfw_linear_ksplit(N, K, M))


def linear_fwd(x, w, bias):
    _bf16(x, "linear.x")
    _bf16(w, "linear.w")
    M, K = x.shape
    N, _ = w.shape
    y = torch.empty(M, N, dtype=torch.bfloat16, device=x.device)
    bf = bias.float().contiguous() if bias is not None else None
    ks = _lib.cilfw_linear_ksplit(M, N, K)
    ws = (torch.empty(ks * M * N, dtype=torch.float32, device=x.device)
          if ks > 1 else None)
    _lib.cilfw_linear_fwd(_ptr(x), _ptr(w), _ptr(bf), _ptr(y), _ptr(ws),
                          c_i(M), c_i(N), c_i(K), c_i(ks), _stream())
    _check("linear_fwd")
    return y


def linear_bwd(dy, x, w, has_bias):
    _bf16(dy, "linear_bwd.dy")
    M, K = x.shape
    N, _ = w.shape
    dx = torch.empty(M, K, dtype=torch.bfloat16, device=x.device)
    dw = torch.empty(N, K, dtype=torch.float32, device=x.device)
    db = torch.empty(N, dtype=torch.float32, device=x.device) if has_bias \
        else None
    ks_dx = _lib.cilfw_linear_ksplit(M, K, N)
    ws_dx = (torch.empty(ks_dx * M * K, dtype=torch.float32, device=x.device)
             if ks_dx > 1 else None)
    _lib.cilfw_linear_dx(_ptr(dy), _ptr(w), _ptr(dx), _ptr(ws_dx), c_i(M),
                         c_i(N), c_i(K), c_i(ks_dx), _stream())
    ks_dw = _lib.cilfw_linear_ksplit(N, K, M)
    ws_dw = (torch.empty(ks_dw * N * K, dtype=torch.float32, device=x.device)
             if ks_dw > 1 else None)
    _lib.cilfw_linear_dw(_ptr(dy), _ptr(x), _ptr(dw), _ptr(db), _ptr(ws_dw),
                         c_i(M), c_i(N), c_i(K), c_i(ks_dw), _stream())
    _check("linear_bwd")
    return dx, dw, db


# ---------------------------------------------------------------------- losses

def ce_fwd(logits, targets, smooth):
    logits = logits.float().contiguous()
    M, C = logits.shape
    probs = torch.empty_like(logits)
    loss = torch.empty((), dtype=torch.float32, device=logits.device)
    rowloss = torch.empty(M, dtype=torch.float32, device=logits.device)
    _lib.cilfw_ce_fwd(_ptr(logits), _ptr(targets.contiguous()), _ptr(probs),
                      _ptr(loss), _ptr(rowloss), c_i(M), c_i(C), c_f(smooth),
                      _stream())
    _check("ce_fwd")
    return loss, probs


def ce_bwd(probs, targets, smooth, dloss):
    M, C = probs.shape
    dlogits = torch.empty_like(probs)
    dl = dloss.float().reshape(1).contiguous()
    _lib.cilfw_ce_bwd(_ptr(probs), _ptr(targets.contiguous()), _ptr(dl),
                      _ptr(dlogits), c_i(M), c_i(C), c_f(smooth), _stream())
    _check("ce_bwd")
    return dlogits


def kd_fwd(s_logits, t_logits, T):
    s = s_logits.float().contiguous()
    t = t_logits.float().contiguous()
    M, C = s.shape
    ps = torch.empty_like(s)
    pt = torch.empty_like(s)
    loss = torch.empty((), dtype=torch.float32, device=s.device)
    rowloss = torch.empty(M, dtype=torch.float32, device=s.device)
    _lib.cilfw_kd_fwd(_ptr(s), _ptr(t), _ptr(ps), _ptr(pt), _ptr(loss),
                      _ptr(rowloss), c_i(M), c_i(C), c_f(T), _stream())
    _check("kd_fwd")
    return loss, ps, pt


def kd_bwd(ps, pt, T, dloss):
    M, C = ps.shape
    ds = torch.empty_like(ps)
    dl = dloss.float().reshape(1).contiguous()
    _lib.cilfw_kd_bwd(_ptr(ps), _ptr(pt), _ptr(dl), _ptr(ds), c_i(M), c_i(C),
                      c_f(T), _stream())
    _check("kd_bwd")
    return ds


def wa_loss_fwd(s_logits, t_logits, targets, smooth, T, lam):
    """Fused CE(+smoothing) + lambda*KD over bf16 logits. t_logits may be
    None (plain CE). Returns (loss_total, loss_ce, loss_kd, probs, ps, pt)."""
    _bf16(s_logits, "wa_loss.s")
    M, C = s_logits.shape
    Ck = 0
    if t_logits is not None:
        _bf16(t_logits, "wa_loss.t")
        Ck = t_logits.shape[1]
    dev = s_logits.device
    probs = torch.empty(M, C, dtype=torch.float32, device=dev)
    ps = torch.empty(M, max(Ck, 1), dtype=torch.float32, device=dev)
    pt = torch.empty(M, max(Ck, 1), dtype=torch.float32, device=dev)
    rl2 = torch.empty(2 * M, dtype=torch.float32, device=dev)
    out3 = torch.empty(3, dtype=torch.float32, device=dev)
    _lib.cilfw_wa_loss_fwd(_ptr(s_logits), _ptr(t_logits),
                           _ptr(targets.contiguous()), _ptr(probs), _ptr(ps),
                           _ptr(pt), _ptr(rl2), _ptr(out3), c_i(M), c_i(C),
                           c_i(Ck), c_f(smooth), c_f(T), c_f(lam), _stream())
    _check("wa_loss_fwd")
    return out3[2], out3[0], out3[1], probs, ps, pt


def wa_loss_bwd(probs, ps, pt, targets, dtotal, smooth, T, lam, Ck):
    M, C = probs.shape
    dlogits = torch.empty(M, C, dtype=torch.bfloat16, device=probs.device)
    dl = dtotal.float().reshape(1).contiguous()
    _lib.cilfw_wa_loss_bwd(_ptr(probs), _ptr(ps), _ptr(pt),
                           _ptr(targets.contiguous()), _ptr(dl),
                           _ptr(dlogits), c_i(M), c_i(C), c_i(Ck),
                           c_f(smooth), c_f(T), c_f(lam), _stream())
    _check("wa_loss_bwd")
    return dlogits


# ------------------------------------------------------------- optimizer / misc

def sgd_step(p, g, m, lr_dev, momentum, wd, p_bf16=None):
    """lr_dev: 1-elem fp32 DEVICE tensor (graph-replayable lr input);
    a plain float is boxed into one for convenience."""
    if not torch.is_tensor(lr_dev):
        lr_dev = torch.full((1,), float(lr_dev), dtype=torch.float32,
                            device=p.device)
    _lib.cilfw_sgd_step(_ptr(p), _ptr(g), _ptr(m), _ptr(p_bf16),
                        c_l(p.numel()), _ptr(lr_dev), c_f(momentum), c_f(wd),
                        _stream())
    _check("sgd_step")


def topk_correct(logits, targets, maxk):
    maxk = int(maxk)
    if not 1 <= maxk <= 8:
        # topk_kernel keeps the winners of earlier passes in excluded[8]
        raise ValueError(f"topk_correct: maxk must be in 1..8 (got {maxk})")
    lf = logits.float().contiguous()
    M, C = lf.shape
    counts = torch.empty(maxk, dtype=torch.int64, device=lf.device)
    _lib.cilfw_topk_correct(_ptr(lf), _ptr(targets.contiguous()),
                            _ptr(counts), c_i(M), c_i(C), c_i(maxk),
                            _stream())
    _check("topk_correct")
    return counts


_CROP_RESIZE_MODES = {torch.uint8: 0, torch.float32: 1, torch.bfloat16: 2}


def _crop_args(name, dev, M, C, S, idx, params, flip, mean255, std255, dtype,
               move_stats):
    """Validation shared by crop_resize / crop_resize_ragged -> (N, idx,
    params, flip, mean255, std255, out). idx None samples all M sources.
    move_stats: mean255/std255 are moved to ``dev``; otherwise they must
    already live there."""
    if idx is not None:
        assert idx.dtype == torch.int64 and idx.dim() == 1 \
            and idx.device == dev
        idx = idx.contiguous()
        N = idx.shape[0]
    else:
        N = M
    assert params.shape == (N, 4) and params.dtype == torch.float32 \
        and params.device == dev
    assert flip.shape == (N,) and flip.dtype == torch.uint8 \
        and flip.device == dev
    params = params.contiguous()
    flip = flip.contiguous()
    if mean255 is None:
        assert std255 is None
        dtype = torch.uint8
    else:
        assert dtype in (torch.float32, torch.bfloat16), \
            f"{name}: normalized output is fp32 or bf16 (got {dtype})"
        if move_stats:
            mean255, std255 = mean255.to(dev), std255.to(dev)
        assert mean255.device == dev and std255.device == dev
        mean255 = mean255.to(torch.float32).reshape(-1).contiguous()
        std255 = std255.to(torch.float32).reshape(-1).contiguous()
        assert mean255.numel() == C and std255.numel() == C
    out = torch.empty(N, S, S, C, dtype=dtype, device=dev)
    assert out.data_ptr() % 16 == 0  # the kernel stores 16-byte vectors
    return N, idx, params, flip, mean255, std255, out


def crop_resize(src, idx, params, flip, out_size, mean255, std255, dtype):
    """Fused gather -> affine bilinear resample -> flip -> quantize ->
    normalize (csrc/data.hip). src uint8 (M,Hs,Ws,C); idx int64 (N,) or None;
    params fp32 (N,4) = (oy, ox, sy, sx); flip uint8 (N,). mean255/std255
    None -> uint8 levels, else normalized ``dtype`` (fp32 / bf16)."""
    assert src.dtype == torch.uint8 and src.dim() == 4 and src.is_contiguous()
    M, Hs, Ws, C = src.shape
    S = int(out_size)
    assert 1 <= C <= 4 and M >= 1 and Hs >= 1 and Ws >= 1 and S >= 1
    assert S * S * C < 2 ** 31 and Hs * Ws * C < 2 ** 31
    N, idx, params, flip, mean255, std255, out = _crop_args(
        "crop_resize", src.device, M, C, S, idx, params, flip, mean255,
        std255, dtype, move_stats=True)
    _lib.cilfw_crop_resize(_ptr(src), _ptr(idx), _ptr(params), _ptr(flip),
                           _ptr(mean255), _ptr(std255), _ptr(out), c_i(M),
                           c_i(N), c_i(Hs), c_i(Ws), c_i(C), c_i(S),
                           c_i(_CROP_RESIZE_MODES[out.dtype]), _stream())
    _check("crop_resize")
    return out


def crop_resize_ragged(pool, offsets, hw, channels, idx, params, flip,
                       out_size, mean255, std255, dtype):
    """crop_resize over a ragged source (csrc/data.hip): pool uint8 flat
    bytes; offsets int64 (M,) byte offset of image m; hw int32 (M,2) = (H, W);
    image m is H*W*C contiguous HWC bytes. idx int64 (N,); the rest as
    crop_resize. The tables live on the device, so offsets[m] + H*W*C <=
    pool.numel() and H*W*C < 2**31 are the store's construction-time checks
    (RaggedImageStore), not per-call ones: checking here would sync."""
    assert pool.dtype == torch.uint8 and pool.dim() == 1 \
        and pool.is_contiguous()
    dev = pool.device
    C, S = int(channels), int(out_size)
    assert offsets.dtype == torch.int64 and offsets.dim() == 1 \
        and offsets.device == dev and offsets.is_contiguous()
    M = offsets.shape[0]
    assert hw.dtype == torch.int32 and hw.shape == (M, 2) \
        and hw.device == dev and hw.is_contiguous()
    assert 1 <= C <= 4 and M >= 1 and S >= 1
    assert S * S * C < 2 ** 31
    assert idx is not None
    N, idx, params, flip, mean255, std255, out = _crop_args(
        "crop_resize_ragged", dev, M, C, S, idx, params, flip, mean255,
        std255, dtype, move_stats=False)
    _lib.cilfw_crop_resize_ragged(
        _ptr(pool), _ptr(offsets), _ptr(hw), _ptr(idx), _ptr(params),
        _ptr(flip), _ptr(mean255), _ptr(std255), _ptr(out), c_i(M), c_i(N),
        c_i(C), c_i(S), c_i(_CROP_RESIZE_MODES[out.dtype]), _stream())
    _check("crop_resize_ragged")
    return out


def herding_select(f, mu, m):
    """Greedy herding of one class: f (n, D) fp32 contiguous GPU features, mu
    (D,) their mean, 0 <= m <= n -> (m,) int64 ranked indices. Bad arguments
    and non-finite / oversized values raise ValueError before any launch
    (``_herding_checks``: with them no candidate would win a step and the
    kernel would index out of bounds)."""
    n, D, m = _hc.check_select_args(f, mu, m)
    if not f.is_cuda:
        raise ValueError("herding_select: features must be on the GPU")
    assert (n + D) * 4 <= _hc.LDS_BYTES, \
        "herding_select kernel supports n+D <= 15000 (per-class sample sets)"
    # one reduction + one sync per call; herding runs once per task
    _hc.check_values("herding_select", f, mu)
    order = torch.empty(m, dtype=torch.int64, device=f.device)
    _lib.cilfw_herding_select(_ptr(f), _ptr(mu), _ptr(order), c_i(n), c_i(D),
                              c_i(m), _stream())
    _check("herding_select")
    return order


def herding_select_batch(feats_list, m_list):
    """All classes' greedy herding in ONE launch (block per class).
    feats_list: list of (n_c, D) fp32 GPU tensors; returns list of int64
    ranked-index tensors (local indices, length m_c = min(m, n_c)). A list
    whose entries disagree in D or device, a quota list of another length and
    non-finite / oversized values raise ValueError before any launch; the
    message names the position of the offending class."""
    ns, D, device = _hc.check_batch_args(feats_list, m_list)
    if device.type != "cuda":
        raise ValueError("herding_select_batch: features must be on the GPU")
    assert all((n + D) * 4 <= _hc.LDS_BYTES for n in ns), "herding LDS limit"
    fall = torch.cat([f.float().contiguous() for f in feats_list])
    # one reduction + one sync per call; herding runs once per task
    _hc.check_values_batch(fall, ns, "herding_select_batch")
    mus = torch.stack([f.float().mean(0) for f in feats_list]).contiguous()
    foff = torch.tensor([0] + list(torch.tensor(ns).cumsum(0)),
                        dtype=torch.int32, device=device)
    ms = [min(m, n) for m, n in zip(m_list, ns)]
    ooff = torch.tensor([0] + list(torch.tensor(ms).cumsum(0)),
                        dtype=torch.int32, device=device)
    mvec = torch.tensor(ms, dtype=torch.int32, device=device)
    order = torch.empty(sum(ms), dtype=torch.int64, device=device)
    _lib.cilfw_herding_select_batch(_ptr(fall), _ptr(foff), _ptr(mus),
                                    _ptr(ooff), _ptr(mvec), _ptr(order),
                                    c_i(len(ns)), c_i(D), c_i(max(ns)),
                                    _stream())
    _check("herding_select_batch")
    outs, o = [], 0
    for m in ms:
        outs.append(order[o:o + m])
        o += m
    return outs


# ------------------------------------------------------------------------- nme

def _nme_f32(t, name, D=None):
    assert t.dtype == torch.float32 and t.dim() == 2 and t.is_contiguous(), \
        f"{name}: needs a contiguous 2-d fp32 tensor"
    assert t.shape[1] % 4 == 0 and 4 <= t.shape[1] <= 4096, \
        f"{name}: nme kernels support feature widths D % 4 == 0, " \
        f"4 <= D <= 4096 (got D = {t.shape[1]})"
    assert D is None or t.shape[1] == D, \
        f"{name}: feature width {t.shape[1]} != {D}"
    assert t.data_ptr() % 16 == 0  # the kernels load 16-byte vectors
    return t


def nme_prototypes(feats, seg_off):
    """Unit-norm class prototypes (csrc/nme.hip). feats fp32 (n, D), rows
    grouped by class; seg_off int32 (C+1,) device tensor of row offsets (the
    caller has checked 0 = seg_off[0] < ... < seg_off[C] = n on the host:
    checking here would sync). -> (C, D) fp32."""
    _nme_f32(feats, "nme_prototypes.feats")
    assert seg_off.dtype == torch.int32 and seg_off.dim() == 1 \
        and seg_off.is_contiguous() and seg_off.device == feats.device \
        and seg_off.numel() >= 2
    C, D = seg_off.numel() - 1, feats.shape[1]
    protos = torch.empty(C, D, dtype=torch.float32, device=feats.device)
    _lib.cilfw_nme_prototypes(_ptr(feats), _ptr(seg_off), _ptr(protos),
                              c_i(C), c_i(D), _stream())
    _check("nme_prototypes")
    return protos


def nme_topk(feats, protos, maxk, targets=None):
    """Fused normalize -> score -> running top-k (csrc/nme.hip): the (N, C)
    score matrix is never materialized. -> (idx int32 (N, maxk), score fp32
    (N, maxk), counts int64 (maxk,) | None); counts[k-1] = rows whose target
    is within the top-k."""
    _nme_f32(feats, "nme_topk.feats")
    N, D = feats.shape
    _nme_f32(protos, "nme_topk.protos", D)
    C = protos.shape[0]
    maxk = int(maxk)
    assert protos.device == feats.device
    assert 1 <= maxk <= min(8, C), \
        f"nme_topk: maxk must be in 1..min(8, C) (got maxk={maxk}, C={C})"
    assert N * maxk < 2 ** 31 and N < 2 ** 31 - 64
    dev = feats.device
    idx = torch.empty(N, maxk, dtype=torch.int32, device=dev)
    score = torch.empty(N, maxk, dtype=torch.float32, device=dev)
    counts = None
    if targets is not None:
        assert targets.dtype == torch.int64 and targets.shape == (N,) \
            and targets.device == dev
        targets = targets.contiguous()
        counts = torch.empty(maxk, dtype=torch.int64, device=dev)
    _lib.cilfw_nme_topk(_ptr(feats), _ptr(protos), _ptr(targets), _ptr(idx),
                        _ptr(score), _ptr(counts), c_i(N), c_i(C), c_i(D),
                        c_i(maxk), _stream())
    _check("nme_topk")
    return idx, score, counts


# ---------------------------------------------------------------------- kmeans

KMEANS_MAX_ABS = 2.0 ** 48


def kmeans_proxies(feats, seg_off, K, max_iter, out=None):
    """K-means proxies of every class in ONE launch (csrc/kmeans.hip: maximin
    seeding and Lloyd iterations, block per class). feats fp32 (n, D)
    contiguous GPU rows grouped by class; seg_off int32 (C+1,) device tensor of
    row offsets. -> (proxies fp32 (C*K, D) unit rows, class-major; assign
    int32 (n,) class-local centre of every row; iters int32 (C,)). ``out``:
    that triple supplied by the caller (every element is written).

    Bad arguments, a shape ``cilfw_kmeans_supported`` refuses, a class with
    fewer than K rows and non-finite / oversized values raise ValueError
    before any launch: a NaN distance wins no ``<`` (the defect found in
    herding), and with max|f| <= 2^48 no row norm overflows (D <= 4096:
    |f|^2 <= 2^108). Two host syncs per call (offsets, values); the op runs
    once per task."""
    what = "kmeans_proxies"
    if not (torch.is_tensor(feats) and feats.dim() == 2):
        raise ValueError(f"{what}: features must be a 2-d tensor (n, D)")
    if feats.dtype != torch.float32:
        raise ValueError(f"{what}: features must be fp32 (got {feats.dtype})")
    if not feats.is_contiguous():
        raise ValueError(f"{what}: features must be contiguous")
    if not feats.is_cuda:
        raise ValueError(f"{what}: features must be on the GPU")
    if not (torch.is_tensor(seg_off) and seg_off.dtype == torch.int32
            and seg_off.dim() == 1 and seg_off.numel() >= 2
            and seg_off.is_contiguous() and seg_off.device == feats.device):
        raise ValueError(
            f"{what}: seg_off must be a contiguous int32 (C+1,) tensor on the "
            f"device of the features")
    n, D = feats.shape
    K, max_iter = int(K), int(max_iter)
    if max_iter < 1:
        raise ValueError(f"{what}: max_iter must be >= 1 (got {max_iter})")
    off = seg_off.cpu().tolist()
    if off[0] != 0 or off[-1] != n or any(b < a for a, b in
                                           zip(off[:-1], off[1:])):
        raise ValueError(
            f"{what}: seg_off must run from 0 to n = {n} without decreasing "
            f"(got {off})")
    sizes = [b - a for a, b in zip(off[:-1], off[1:])]
    small = [c for c, q in enumerate(sizes) if q < K]
    if small and 1 <= K <= 16:
        raise ValueError(
            f"{what}: class segment(s) {small} hold fewer than K = {K} rows")
    if _lib.cilfw_kmeans_supported(c_i(min(sizes)), c_i(D), c_i(K)) != 1:
        raise ValueError(
            f"{what}: cilfw_kmeans_supported refuses (n_min, D, K) = "
            f"({min(sizes)}, {D}, {K}): needs D % 4 == 0, 4 <= D <= 4096, "
            f"1 <= K <= 16, K * D <= 16000 (the centres live in LDS) and "
            f"n >= K")
    if n * D >= 2 ** 40:
        raise ValueError(f"{what}: {n} x {D} features are too many")
    a = feats.detach().abs().amax().item()
    if not (a <= KMEANS_MAX_ABS):  # written so that NaN fails
        raise ValueError(
            f"{what}: features must be finite with max|f| <= 2^48 (got "
            f"max|f| = {a}); a diverged run cannot be clustered")
    assert feats.data_ptr() % 16 == 0  # the kernel loads 16-byte vectors
    C, dev = len(sizes), feats.device
    xh = torch.empty(n, D, dtype=torch.float32, device=dev)
    xx = torch.empty(n, dtype=torch.float32, device=dev)
    dmin = torch.empty(n, dtype=torch.float32, device=dev)
    if out is None:
        out = (torch.empty(C * K, D, dtype=torch.float32, device=dev),
               torch.empty(n, dtype=torch.int32, device=dev),
               torch.empty(C, dtype=torch.int32, device=dev))
    proxies, assign, iters = out
    for t, shape, dt in ((proxies, (C * K, D), torch.float32),
                         (assign, (n,), torch.int32),
                         (iters, (C,), torch.int32)):
        if not (tuple(t.shape) == shape and t.dtype == dt
                and t.is_contiguous() and t.device == dev):
            raise ValueError(
                f"{what}: out must hold contiguous proxies ({C * K}, {D}) "
                f"fp32, assign ({n},) int32 and iters ({C},) int32 on the "
                f"device of the features")
    rc = _lib.cilfw_kmeans_proxies(_ptr(feats), _ptr(seg_off), _ptr(xh),
                                   _ptr(xx), _ptr(dmin), _ptr(proxies),
                                   _ptr(assign), _ptr(iters), c_i(C),
                                   c_i(min(sizes)), c_i(D), c_i(K),
                                   c_i(max_iter), _stream())
    if rc != 0:
        raise RuntimeError(f"{what}: launcher refused the shape")
    _check(what)
    return proxies, assign, iters


# ------------------------------------------------------------------------- pod

def _pod_map(t, name):
    """bf16 NHWC map the POD kernels accept; the launchers in csrc/pod.hip
    apply the same shape rule (cilfw_pod_supported) on the host."""
    assert t.dim() == 4, f"{name}: needs an (N, H, W, C) map"
    _bf16(t, name)
    N, H, W_, C = t.shape
    assert C % 8 == 0, \
        f"{name}: POD kernels need C % 8 == 0 (got C = {C})"
    assert 1 <= H <= 256 and 1 <= W_ <= 256, \
        f"{name}: POD kernels support 1 <= H, W <= 256 (got {H} x {W_})"
    assert N >= 1 and _lib.cilfw_pod_supported(N, H, W_, C) == 1
    assert t.data_ptr() % 16 == 0  # the kernels load 16-byte vectors
    return N, H, W_, C


def pod_pool_groups(W_, C):
    """Channel groups (of 8) one pod_pool block covers — for docs/benches."""
    return _lib.cilfw_pod_pool_groups(c_i(W_), c_i(C))


def pod_pool(a, out=None):
    """(N, H, W, C) bf16 -> (N, H+W, C) fp32: row sums of squares r[h, c]
    first, then column sums q[w, c] (csrc/pod.hip). ``out`` may be supplied
    (every element is written)."""
    N, H, W_, C = _pod_map(a, "pod_pool")
    if out is None:
        out = torch.empty(N, H + W_, C, dtype=torch.float32, device=a.device)
    assert out.shape == (N, H + W_, C) and out.dtype == torch.float32 \
        and out.is_contiguous() and out.device == a.device
    rc = _lib.cilfw_pod_pool(_ptr(a), _ptr(out), c_i(N), c_i(H), c_i(W_),
                             c_i(C), _stream())
    assert rc == 0, "pod_pool: launcher refused the shape"
    _check("pod_pool")
    return out


def pod_dist(vs, vt):
    """Pooled student / teacher vectors (N, H+W, C) fp32 -> (loss 0-d fp32,
    dist (N,) fp32, g_v (N, H+W, C) fp32 for upstream 1)."""
    assert vs.shape == vt.shape and vs.dim() == 3
    for t in (vs, vt):
        assert t.dtype == torch.float32 and t.is_contiguous() \
            and t.device == vs.device and t.data_ptr() % 16 == 0
    N, L = vs.shape[0], vs.shape[1] * vs.shape[2]
    assert L < 2 ** 31
    gv = torch.empty_like(vs)
    dist = torch.empty(N, dtype=torch.float32, device=vs.device)
    loss = torch.empty(1, dtype=torch.float32, device=vs.device)
    rc = _lib.cilfw_pod_dist(_ptr(vs), _ptr(vt), _ptr(gv), _ptr(dist),
                             _ptr(loss), c_i(N), c_i(L), _stream())
    assert rc == 0, "pod_dist: launcher refused the shape"
    _check("pod_dist")
    return loss[0], dist, gv


def pod_bwd(a, gv, up, out=None):
    """da = 2 a (g_v.r[h] + g_v.q[w]) * up, bf16 like ``a``. ``up``: 1-element
    fp32 DEVICE tensor (read by the kernel: no host sync, graph-safe)."""
    N, H, W_, C = _pod_map(a, "pod_bwd")
    assert gv.shape == (N, H + W_, C) and gv.dtype == torch.float32 \
        and gv.is_contiguous() and gv.device == a.device \
        and gv.data_ptr() % 16 == 0
    assert up.dtype == torch.float32 and up.numel() == 1 \
        and up.device == a.device
    if out is None:
        out = torch.empty_like(a)
    assert out.shape == a.shape and out.dtype == torch.bfloat16 \
        and out.is_contiguous() and out.device == a.device \
        and out.data_ptr() % 16 == 0
    rc = _lib.cilfw_pod_bwd(_ptr(a), _ptr(gv), _ptr(up), _ptr(out), c_i(N),
                            c_i(H), c_i(W_), c_i(C), _stream())
    assert rc == 0, "pod_bwd: launcher refused the shape"
    _check("pod_bwd")
    return out


# ---------------------------------------------------------- cosine head / flat

def _cos_rows(t, name, dtypes=(torch.bfloat16,)):
    """(rows, D) matrix the row-normalisation kernels accept; the launchers
    in csrc/cosine.hip apply the same rule (cilfw_cosine_supported)."""
    assert t.dim() == 2, f"{name}: needs a (rows, D) matrix"
    if dtypes == (torch.bfloat16,):
        _bf16(t, name)
    else:
        assert t.dtype in dtypes, \
            f"{name}: rows are bf16 or fp32 (got {t.dtype})"
        assert t.is_contiguous(), f"{name}: needs contiguous tensor"
    rows, D = t.shape
    f32 = t.dtype == torch.float32
    assert 1 <= D <= 2048, \
        f"{name}: cosine kernels need 1 <= D <= 2048 (got D = {D})"
    if f32:
        assert D % 4 == 0, \
            f"{name}: fp32 rows need D % 4 == 0 (got D = {D})"
    else:
        assert D % 8 == 0, \
            f"{name}: bf16 rows need D % 8 == 0 (got D = {D})"
    assert rows >= 1, f"{name}: needs rows >= 1"
    assert _lib.cilfw_cosine_supported(rows, D, 1 if f32 else 0) == 1
    assert t.data_ptr() % 16 == 0  # the kernels load 16-byte vectors
    return rows, D, f32


def _dev_scalar(s, ref, name):
    if s is None:
        return None
    assert s.dtype == torch.float32 and s.numel() == 1 \
        and s.device == ref.device, \
        f"{name}: the scalar is a 1-element fp32 DEVICE tensor"
    return s


def rownorm_fwd(x, scale=None, out=None, rinv=None):
    """x (rows, D) bf16 or fp32 -> (y bf16 (rows, D) = scale * x r(x), rinv
    fp32 (rows,)), r(x) = 1/|x| or 0 for a zero row (csrc/cosine.hip).
    ``scale``: 1-element fp32 DEVICE tensor read by the kernel (graph-safe) or
    None for 1. ``out`` / ``rinv`` may be supplied (every element is
    written)."""
    rows, D, f32 = _cos_rows(x, "rownorm_fwd",
                             (torch.bfloat16, torch.float32))
    scale = _dev_scalar(scale, x, "rownorm_fwd")
    if out is None:
        out = torch.empty(rows, D, dtype=torch.bfloat16, device=x.device)
    if rinv is None:
        rinv = torch.empty(rows, dtype=torch.float32, device=x.device)
    assert out.shape == (rows, D) and out.dtype == torch.bfloat16 \
        and out.is_contiguous() and out.device == x.device \
        and out.data_ptr() % 16 == 0
    assert rinv.shape == (rows,) and rinv.dtype == torch.float32 \
        and rinv.is_contiguous() and rinv.device == x.device
    rc = _lib.cilfw_rownorm_fwd(_ptr(x), _ptr(scale), _ptr(out), _ptr(rinv),
                                c_i(rows), c_i(D), c_i(1 if f32 else 0),
                                _stream())
    assert rc == 0, "rownorm_fwd: launcher refused the shape"
    _check("rownorm_fwd")
    return out, rinv


def rownorm_bwd(x, rinv, g, scale=None, want_dsig=False, out=None):
    """dx = (scale r) (g - x^ (x^ . g)), x^ = x r, in the dtype of x; g has
    that dtype too (bf16 features, fp32 class weights). -> (dx, dsig fp32
    (rows,) = x^ . g | None)."""
    rows, D, f32 = _cos_rows(x, "rownorm_bwd",
                             (torch.bfloat16, torch.float32))
    assert g.shape == x.shape and g.dtype == x.dtype and g.is_contiguous() \
        and g.device == x.device and g.data_ptr() % 16 == 0, \
        "rownorm_bwd: the gradient has the shape and dtype of the rows"
    assert rinv.shape == (rows,) and rinv.dtype == torch.float32 \
        and rinv.is_contiguous() and rinv.device == x.device
    scale = _dev_scalar(scale, x, "rownorm_bwd")
    if out is None:
        out = torch.empty_like(x)
    assert out.shape == x.shape and out.dtype == x.dtype \
        and out.is_contiguous() and out.device == x.device \
        and out.data_ptr() % 16 == 0
    dsig = (torch.empty(rows, dtype=torch.float32, device=x.device)
            if want_dsig else None)
    rc = _lib.cilfw_rownorm_bwd(_ptr(x), _ptr(rinv), _ptr(g), _ptr(scale),
                                _ptr(out), _ptr(dsig), c_i(rows), c_i(D),
                                c_i(1 if f32 else 0), _stream())
    assert rc == 0, "rownorm_bwd: launcher refused the shape"
    _check("rownorm_bwd")
    return out, dsig


def cos_sum(v, scale=1.0):
    """scale * sum(v) of a 1-d fp32 tensor in a fixed order -> (1,) fp32."""
    assert v.dim() == 1 and v.dtype == torch.float32 and v.is_contiguous() \
        and 1 <= v.numel() < 2 ** 31
    out = torch.empty(1, dtype=torch.float32, device=v.device)
    rc = _lib.cilfw_cos_sum(_ptr(v), _ptr(out), c_i(v.numel()), c_f(scale),
                            _stream())
    assert rc == 0, "cos_sum: launcher refused the shape"
    _check("cos_sum")
    return out


def flat_dist(s, t, out=None, rows_out=None):
    """Student / teacher features (M, D) bf16 -> (loss 0-d fp32 = mean l, l
    (M,) fp32 = |s^ - t^|^2 / 2, gs (M, D) fp32: d loss / d s for upstream
    1)."""
    M, D, _ = _cos_rows(s, "flat_dist.student")
    assert t.shape == s.shape, \
        f"flat_dist: student features {tuple(s.shape)} vs teacher " \
        f"{tuple(t.shape)}"
    _cos_rows(t, "flat_dist.teacher")
    assert t.device == s.device
    gs = out if out is not None else torch.empty(
        M, D, dtype=torch.float32, device=s.device)
    l = rows_out if rows_out is not None else torch.empty(
        M, dtype=torch.float32, device=s.device)
    assert gs.shape == (M, D) and gs.dtype == torch.float32 \
        and gs.is_contiguous() and gs.data_ptr() % 16 == 0
    assert l.shape == (M,) and l.dtype == torch.float32 and l.is_contiguous()
    loss = torch.empty(1, dtype=torch.float32, device=s.device)
    rc = _lib.cilfw_flat_dist(_ptr(s), _ptr(t), _ptr(gs), _ptr(l),
                              _ptr(loss), c_i(M), c_i(D), _stream())
    assert rc == 0, "flat_dist: launcher refused the shape"
    _check("flat_dist")
    return loss[0], l, gs


def flat_bwd(gs, up, out=None):
    """ds bf16 (M, D) = up * gs. ``up``: 1-element fp32 DEVICE tensor (read
    by the kernel: no host sync, graph-safe)."""
    M, D, _ = _cos_rows(gs, "flat_bwd", (torch.float32,))
    assert D % 8 == 0, f"flat_bwd: bf16 rows need D % 8 == 0 (got D = {D})"
    up = _dev_scalar(up, gs, "flat_bwd")
    assert up is not None
    if out is None:
        out = torch.empty(M, D, dtype=torch.bfloat16, device=gs.device)
    assert out.shape == (M, D) and out.dtype == torch.bfloat16 \
        and out.is_contiguous() and out.device == gs.device \
        and out.data_ptr() % 16 == 0
    rc = _lib.cilfw_flat_bwd(_ptr(gs), _ptr(up), _ptr(out), c_i(M), c_i(D),
                             _stream())
    assert rc == 0, "flat_bwd: launcher refused the shape"
    _check("flat_bwd")
    return out


# -------------------------------------------------------------- margin ranking

def _mrank_args(M, C, known, k, name):
    """The shape rule of csrc/mrank.hip (cilfw_mrank_supported)."""
    known, k = int(known), int(k)
    assert M >= 1 and C >= 2, \
        f"{name}: needs M >= 1 rows and C >= 2 classes (got {M} x {C})"
    assert 1 <= known < C, \
        f"{name}: known must be in 1..C-1 (got known={known}, C={C})"
    assert 1 <= k <= min(8, C - known), \
        f"{name}: k must be in 1..min(8, C - known) (got k={k}, " \
        f"C - known = {C - known})"
    assert M * max(C, k) < 2 ** 62 and M < 2 ** 31 - 64 and C < 2 ** 31 - 64
    assert _lib.cilfw_mrank_supported(M, C, known, k) == 1
    return known, k


def _mrank_buf(t, shape, dtype, ref, name):
    if t is None:
        return torch.empty(shape, dtype=dtype, device=ref.device)
    assert tuple(t.shape) == tuple(shape) and t.dtype == dtype \
        and t.is_contiguous() and t.device == ref.device, \
        f"{name}: out buffer must be a contiguous {dtype} tensor of shape " \
        f"{tuple(shape)} on the device of the logits"
    return t


def mrank_fwd(logits, targets, sigma, known, k, margin, out=None):
    """LUCIR's margin-ranking loss, forward (csrc/mrank.hip). logits (M, C)
    bf16, targets (M,) int64, sigma: 1-element fp32 DEVICE tensor read by the
    kernels (graph-safe). -> (loss 0-d fp32, sel int32 (M, k), fin fp32 (3,) =
    [loss, q, dsigma for upstream 1], nold int32 (1,), rho fp32 (M,), dsum
    fp32 (M,), old int32 (M,)). ``out``: a dict of buffers under those names
    (every element of each is written)."""
    assert logits.dim() == 2, "mrank_fwd: logits are (M, C)"
    _bf16(logits, "mrank_fwd.logits")
    M, C = logits.shape
    known, k = _mrank_args(M, C, known, k, "mrank_fwd")
    margin = float(margin)
    assert margin >= 0.0, f"mrank_fwd: margin must be >= 0 (got {margin})"
    assert targets.dtype == torch.int64 and targets.shape == (M,) \
        and targets.is_contiguous() and targets.device == logits.device, \
        "mrank_fwd: targets are a contiguous int64 (M,) tensor on the " \
        "device of the logits"
    sigma = _dev_scalar(sigma, logits, "mrank_fwd")
    assert sigma is not None
    out = out or {}
    f32, i32 = torch.float32, torch.int32
    sel = _mrank_buf(out.get("sel"), (M, k), i32, logits, "mrank_fwd.sel")
    fin = _mrank_buf(out.get("fin"), (3,), f32, logits, "mrank_fwd.fin")
    nold = _mrank_buf(out.get("nold"), (1,), i32, logits, "mrank_fwd.nold")
    rho = _mrank_buf(out.get("rho"), (M,), f32, logits, "mrank_fwd.rho")
    dsum = _mrank_buf(out.get("dsum"), (M,), f32, logits, "mrank_fwd.dsum")
    old = _mrank_buf(out.get("old"), (M,), i32, logits, "mrank_fwd.old")
    rc = _lib.cilfw_mrank_fwd(_ptr(logits), _ptr(targets), _ptr(sigma),
                              _ptr(rho), _ptr(dsum), _ptr(old), _ptr(sel),
                              _ptr(fin), _ptr(nold), c_i(M), c_i(C),
                              c_i(known), c_i(k), c_f(margin), _stream())
    assert rc == 0, "mrank_fwd: launcher refused the arguments"
    _check("mrank_fwd")
    return fin[0], sel, fin, nold, rho, dsum, old


def mrank_bwd(sel, targets, fin, up, C, known, out=None, dsig=None):
    """-> (dlogits bf16 (M, C), dsigma fp32 (1,)) from what mrank_fwd left:
    +up q at the selected classes, -up q A at the target, 0 elsewhere (the
    whole row is written). ``up``: 1-element fp32 DEVICE tensor (read by the
    kernel: no host sync, graph-safe)."""
    assert sel.dim() == 2 and sel.dtype == torch.int32 \
        and sel.is_contiguous(), "mrank_bwd: sel is int32 (M, k)"
    M, k = sel.shape
    C = int(C)
    known, k = _mrank_args(M, C, known, k, "mrank_bwd")
    assert targets.dtype == torch.int64 and targets.shape == (M,) \
        and targets.is_contiguous() and targets.device == sel.device
    assert fin.shape == (3,) and fin.dtype == torch.float32 \
        and fin.is_contiguous() and fin.device == sel.device
    up = _dev_scalar(up, sel, "mrank_bwd")
    assert up is not None
    out = _mrank_buf(out, (M, C), torch.bfloat16, sel, "mrank_bwd.out")
    dsig = _mrank_buf(dsig, (1,), torch.float32, sel, "mrank_bwd.dsig")
    rc = _lib.cilfw_mrank_bwd(_ptr(sel), _ptr(targets), _ptr(fin), _ptr(up),
                              _ptr(out), _ptr(dsig), c_i(M), c_i(C),
                              c_i(known), c_i(k), _stream())
    assert rc == 0, "mrank_bwd: launcher refused the arguments"
    _check("mrank_bwd")
    return out, dsig


# ------------------------------------------------------------------- LSC / NCA

def _lsc_args(sims, nb_proxy, gamma, name):
    """The shape rule of csrc/lsc.hip (cilfw_lsc_supported). -> M, C, K,
    gamma."""
    assert sims.dim() == 2, f"{name}: sims are (M, C * nb_proxy)"
    assert sims.is_cuda, f"{name}: the kernels take GPU tensors (got a " \
        f"host tensor)"
    _bf16(sims, f"{name}.sims")
    K, gamma = int(nb_proxy), float(gamma)
    assert 1 <= K <= 16, f"{name}: nb_proxy must be in 1..16 (got {K})"
    M, CK = sims.shape
    assert M >= 1 and CK >= 1 and CK % K == 0, \
        f"{name}: sims (M, C * nb_proxy) need M >= 1 and a column count " \
        f"that is a multiple of nb_proxy = {K} (got {M} x {CK})"
    assert gamma >= 0.0, f"{name}: gamma must be >= 0 (got {gamma})"
    C = CK // K
    assert M * CK < 2 ** 62 and M < 2 ** 31 - 64 and CK < 2 ** 31 - 64, \
        f"{name}: sims too large for the kernels' int indices (got " \
        f"{M} x {CK}; M and C * nb_proxy must stay below 2^31 - 64)"
    assert _lib.cilfw_lsc_supported(M, C, K) == 1, \
        f"{name}: cilfw_lsc_supported refuses (M, C, nb_proxy) = " \
        f"({M}, {C}, {K})"
    return M, C, K, gamma


def _row_buf(t, shape, dtype, ref, name):
    if t is None:
        return torch.empty(shape, dtype=dtype, device=ref.device)
    assert tuple(t.shape) == tuple(shape) and t.dtype == dtype \
        and t.is_contiguous() and t.device == ref.device, \
        f"{name}: out buffer must be a contiguous {dtype} tensor of shape " \
        f"{tuple(shape)} on the device of the input"
    return t


def lsc_reduce_fwd(sims, sigma, nb_proxy, gamma=1.0, out=None, yhat=None):
    """PODNet's local similarity classifier, forward (csrc/lsc.hip). sims
    (M, C * nb_proxy) bf16 cosines, class-major; sigma: 1-element fp32 DEVICE
    tensor read by the kernel (graph-safe). -> (logits bf16 (M, C) = sigma
    yhat, yhat fp32 (M, C)), yhat the softmax(gamma s)-weighted mean of each
    class's cosines. ``out`` / ``yhat`` may be supplied (every element is
    written)."""
    M, C, K, gamma = _lsc_args(sims, nb_proxy, gamma, "lsc_reduce_fwd")
    sigma = _dev_scalar(sigma, sims, "lsc_reduce_fwd")
    assert sigma is not None, "lsc_reduce_fwd: sigma is required"
    out = _row_buf(out, (M, C), torch.bfloat16, sims, "lsc_reduce_fwd.out")
    yhat = _row_buf(yhat, (M, C), torch.float32, sims, "lsc_reduce_fwd.yhat")
    rc = _lib.cilfw_lsc_reduce_fwd(_ptr(sims), _ptr(sigma), _ptr(out),
                                   _ptr(yhat), c_i(M), c_i(C), c_i(K),
                                   c_f(gamma), _stream())
    assert rc == 0, "lsc_reduce_fwd: launcher refused the arguments"
    _check("lsc_reduce_fwd")
    return out, yhat


def lsc_reduce_bwd(sims, yhat, g, sigma, nb_proxy, gamma=1.0, out=None,
                   rows=None):
    """-> (dsims bf16 (M, C * nb_proxy), rows fp32 (M,) = sum_c g_c yhat_c;
    ``cos_sum(rows)`` is dsigma) from the sims, the yhat lsc_reduce_fwd left
    and the upstream g bf16 (M, C). The softmax weights are recomputed."""
    M, C, K, gamma = _lsc_args(sims, nb_proxy, gamma, "lsc_reduce_bwd")
    assert yhat.shape == (M, C) and yhat.dtype == torch.float32 \
        and yhat.is_contiguous() and yhat.device == sims.device, \
        "lsc_reduce_bwd: yhat is the fp32 (M, C) tensor of lsc_reduce_fwd"
    assert g.shape == (M, C) and g.device == sims.device, \
        f"lsc_reduce_bwd: the upstream is (M, C) = ({M}, {C}) on the " \
        f"device of the sims (got {tuple(g.shape)})"
    _bf16(g, "lsc_reduce_bwd.g")
    sigma = _dev_scalar(sigma, sims, "lsc_reduce_bwd")
    assert sigma is not None, "lsc_reduce_bwd: sigma is required"
    out = _row_buf(out, (M, C * K), torch.bfloat16, sims,
                   "lsc_reduce_bwd.out")
    rows = _row_buf(rows, (M,), torch.float32, sims, "lsc_reduce_bwd.rows")
    rc = _lib.cilfw_lsc_reduce_bwd(_ptr(sims), _ptr(yhat), _ptr(g),
                                   _ptr(sigma), _ptr(out), _ptr(rows),
                                   c_i(M), c_i(C), c_i(K), c_f(gamma),
                                   _stream())
    assert rc == 0, "lsc_reduce_bwd: launcher refused the arguments"
    _check("lsc_reduce_bwd")
    return out, rows


def _nca_args(logits, targets, name):
    """The shape rule of csrc/lsc.hip (cilfw_nca_supported). -> M, C."""
    assert logits.dim() == 2, f"{name}: logits are (M, C)"
    assert logits.is_cuda, f"{name}: the kernels take GPU tensors (got a " \
        f"host tensor)"
    _bf16(logits, f"{name}.logits")
    M, C = logits.shape
    assert M >= 1 and C >= 2, \
        f"{name}: needs M >= 1 rows and C >= 2 classes (got {M} x {C})"
    assert targets.dtype == torch.int64 and targets.shape == (M,) \
        and targets.is_contiguous() and targets.device == logits.device, \
        f"{name}: targets are a contiguous int64 (M,) tensor on the " \
        f"device of the logits"
    assert M * C < 2 ** 62 and M < 2 ** 31 - 64 and C < 2 ** 31 - 64, \
        f"{name}: logits too large for the kernels' int indices (got " \
        f"{M} x {C}; M and C must stay below 2^31 - 64)"
    assert _lib.cilfw_nca_supported(M, C) == 1, \
        f"{name}: cilfw_nca_supported refuses (M, C) = ({M}, {C})"
    return M, C


def nca_fwd(logits, targets, sigma, margin, out=None):
    """PODNet's NCA loss, forward (csrc/lsc.hip). logits (M, C) bf16, targets
    (M,) int64, sigma: 1-element fp32 DEVICE tensor read by the kernels
    (graph-safe). -> (loss 0-d fp32, h fp32 (M,), active int32 (M,), lse fp32
    (M,), fin fp32 (3,) = [loss, 1/M, dsigma for upstream 1], nact int32
    (1,)). ``out``: a dict of buffers under the names h, active, lse, fin,
    nact (every element of each is written)."""
    M, C = _nca_args(logits, targets, "nca_fwd")
    margin = float(margin)
    assert margin >= 0.0, f"nca_fwd: margin must be >= 0 (got {margin})"
    sigma = _dev_scalar(sigma, logits, "nca_fwd")
    assert sigma is not None, "nca_fwd: sigma is required"
    out = out or {}
    f32, i32 = torch.float32, torch.int32
    h = _row_buf(out.get("h"), (M,), f32, logits, "nca_fwd.h")
    lse = _row_buf(out.get("lse"), (M,), f32, logits, "nca_fwd.lse")
    active = _row_buf(out.get("active"), (M,), i32, logits, "nca_fwd.active")
    fin = _row_buf(out.get("fin"), (3,), f32, logits, "nca_fwd.fin")
    nact = _row_buf(out.get("nact"), (1,), i32, logits, "nca_fwd.nact")
    rc = _lib.cilfw_nca_fwd(_ptr(logits), _ptr(targets), _ptr(sigma), _ptr(h),
                            _ptr(lse), _ptr(active), _ptr(fin), _ptr(nact),
                            c_i(M), c_i(C), c_f(margin), _stream())
    assert rc == 0, "nca_fwd: launcher refused the arguments"
    _check("nca_fwd")
    return fin[0], h, active, lse, fin, nact


def nca_bwd(logits, targets, lse, active, fin, up, out=None, dsig=None):
    """-> (dlogits bf16 (M, C), dsigma fp32 (1,)) from what nca_fwd left: the
    softmax over the negatives times up/M and -up/M at the target for an
    active row, 0 for every other row (the whole row is written). ``up``:
    1-element fp32 DEVICE tensor (read by the kernel: no host sync,
    graph-safe)."""
    M, C = _nca_args(logits, targets, "nca_bwd")
    f32 = torch.float32
    assert lse.shape == (M,) and lse.dtype == f32 and lse.is_contiguous() \
        and lse.device == logits.device, \
        "nca_bwd: lse is the contiguous fp32 (M,) tensor of nca_fwd on the " \
        "device of the logits"
    assert active.shape == (M,) and active.dtype == torch.int32 \
        and active.is_contiguous() and active.device == logits.device, \
        "nca_bwd: active is the contiguous int32 (M,) tensor of nca_fwd on " \
        "the device of the logits"
    assert fin.shape == (3,) and fin.dtype == f32 and fin.is_contiguous() \
        and fin.device == logits.device, \
        "nca_bwd: fin is the contiguous fp32 (3,) tensor of nca_fwd on the " \
        "device of the logits"
    up = _dev_scalar(up, logits, "nca_bwd")
    assert up is not None, "nca_bwd: the upstream scalar is required"
    out = _row_buf(out, (M, C), torch.bfloat16, logits, "nca_bwd.out")
    dsig = _row_buf(dsig, (1,), f32, logits, "nca_bwd.dsig")
    rc = _lib.cilfw_nca_bwd(_ptr(logits), _ptr(targets), _ptr(lse),
                            _ptr(active), _ptr(fin), _ptr(up), _ptr(out),
                            _ptr(dsig), c_i(M), c_i(C), _stream())
    assert rc == 0, "nca_bwd: launcher refused the arguments"
    _check("nca_bwd")
    return out, dsig
