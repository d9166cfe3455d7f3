"""Which kernel every conv geometry routes to, as JSON (no GPU needed).

The route / split-K / slice / BN-fusion queries of csrc/conv.hip launch
nothing, so this runs wherever cilfw/_hip_lib.so is built. The knobs are
per-process statics on the C side: ``table()`` therefore answers each
environment of ENVS from a fresh child process. tests/golden/conv_routes.json
is the stored ``table()``; tests/test_conv_route_table.py requires equality.

    python tools/conv_route_table.py          # {env: [row, ...]} for ENVS
    python tools/conv_route_table.py --rows   # rows of this process's env
"""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENVS = ("", "CILFW_CONV_V2=0", "CILFW_CONV_V2_BWD_MINM=1",
        "CILFW_CONV_V2_BN128=0", "CILFW_CONV_V2_BN128_MIN3X3=0",
        "CILFW_CONV_BK64_MIN=0", "CILFW_CONV_BK64_MAXBLOCKS=100000",
        "CILFW_CONV_KSPLIT_TARGET=1", "CILFW_CONV_DW_TARGET=256",
        "CILFW_NO_S2_FUSED=1", "CILFW_BNBWD_FUSE=1", "CILFW_STEM_IM2COL=1")


def _resnet(batch, hw, layers, bottleneck):
    """(N, H, W, C, K, k, stride, pad) of every conv of models/resnet.py."""
    small = hw <= 64
    g = [(batch, hw, hw, 3, 64) + ((3, 1, 1) if small else (7, 2, 3))]
    if not small:
        hw = (hw // 2 - 1) // 2 + 1  # 7x7/s2 stem, then 3x3/s2 max-pool
    cin = 64
    for i, n in enumerate(layers):
        width = 64 << i
        cout = width * (4 if bottleneck else 1)
        for b in range(n):
            st = 2 if (b == 0 and i > 0) else 1
            ho = hw // st
            if bottleneck:
                g += [(batch, hw, hw, cin, width, 1, 1, 0),
                      (batch, hw, hw, width, width, 3, st, 1),
                      (batch, ho, ho, width, cout, 1, 1, 0)]
            else:
                g += [(batch, hw, hw, cin, width, 3, st, 1),
                      (batch, ho, ho, width, width, 3, 1, 1)]
            if st != 1 or cin != cout:
                g.append((batch, hw, hw, cin, cout, 1, st, 0))
            cin, hw = cout, ho
    return g


# geometry lists of tests/test_conv_routes_gpu.py (that test module checks
# they stay a subset of GEOMS)
FUZZ = [(3, 7, 7, 16, 16, 3, 1, 1), (5, 9, 9, 32, 48, 3, 2, 1),
        (2, 11, 11, 64, 24, 1, 1, 0), (7, 5, 5, 24, 64, 3, 1, 1),
        (1, 17, 17, 16, 40, 5, 2, 2), (4, 6, 6, 128, 72, 3, 1, 1),
        (2, 14, 14, 40, 16, 7, 2, 3), (4, 16, 16, 64, 128, 3, 2, 1)]
BN_PARTS = [(3, 7, 7, 16, 24, 3, 1, 1), (5, 9, 9, 24, 72, 3, 2, 1),
            (2, 11, 11, 64, 136, 1, 1, 0), (17, 31, 31, 64, 256, 1, 1, 0),
            (64, 32, 32, 64, 64, 3, 1, 1)]
PARAMETRISED = [
    (9, 30, 30, 512, 128, 1, 1, 0),                          # fwd bn128
    (32, 31, 31, 128, 32, 3, 2, 1), (32, 32, 32, 128, 16, 3, 2, 1),
    (22, 31, 31, 136, 16, 3, 2, 1), (32, 31, 31, 128, 16, 5, 2, 2),
    (3, 224, 224, 16, 16, 3, 1, 1), (13, 108, 108, 24, 40, 3, 1, 1),
    (13, 110, 110, 32, 24, 3, 2, 1), (13, 108, 108, 64, 64, 1, 1, 0),
    (4, 8, 8, 64, 128, 1, 2, 0), (2, 32, 32, 3, 64, 7, 2, 3),  # dW delivery
    (3, 7, 7, 16, 16, 3, 1, 1), (7, 5, 5, 24, 64, 3, 1, 1),  # BN epilogue
]


def _unique(seq):
    return list(dict.fromkeys(seq))


GEOMS = _unique(_resnet(128, 32, [2, 2, 2, 2], False)
                + _resnet(32, 224, [3, 4, 6, 3], True)
                + FUZZ + BN_PARTS + PARAMETRISED)
# (M, N, K) of the classifier heads: x (M, K) @ w (N, K)^T
LINEAR = [(128, 100, 512), (32, 1000, 2048), (128, 10, 64), (7, 13, 40)]


def _fwd_bn_gy(H, N, Ho, Wo):
    return H._lib.cilfw_conv2d_fwd_bn_gy(N, Ho, Wo)


def rows():
    """One row per geometry under THIS process's environment."""
    sys.path.insert(0, HERE)
    from cilfw import _hip_ops as H
    out = []
    for N, Hh, W, C, K, k, st, pd in GEOMS:
        Ho, Wo = (Hh + 2 * pd - k) // st + 1, (W + 2 * pd - k) // st + 1
        out.append({
            "geom": [N, Hh, W, C, K, k, st, pd],
            "fwd": list(H.conv2d_fwd_route(N, Hh, W, C, K, k, k, st, pd)),
            "bwd_data": list(H.conv2d_bwd_data_route(N, Hh, W, C, K, k, k,
                                                     st)),
            "bwd_weight": list(H.conv2d_bwd_weight_route(N, C, K, k, k, Ho,
                                                         Wo, False)),
            "bwd_weight_accum": list(H.conv2d_bwd_weight_route(
                N, C, K, k, k, Ho, Wo, True)),
            "can_fuse_bn": H._lib.cilfw_conv2d_bwd_data_can_fuse_bn(
                N, Hh, W, C, K, k, k, st),
            "fwd_bn_gy": _fwd_bn_gy(H, N, Ho, Wo),
            "bwd_data_bn_gy": H._lib.cilfw_conv2d_bwd_data_bn_gy(N, Hh, W),
        })
    out.append({"linear": [[list(s), list(H.linear_ksplits(*s))]
                           for s in LINEAR]})
    return out


def table(argv=None):
    """{environment setting: rows()} over ENVS, one child process each."""
    argv = argv or [sys.executable, os.path.abspath(__file__), "--rows"]
    knobs = {e.split("=")[0] for e in ENVS if e}
    base = {k: v for k, v in os.environ.items() if k not in knobs}
    procs = [subprocess.Popen(argv, stdout=subprocess.PIPE, text=True,
                              env=dict(base, **dict([e.split("=")] if e
                                                    else [])))
             for e in ENVS]  # all at once: each child is mostly import time
    out = {}
    for e, p in zip(ENVS, procs):
        stdout, _ = p.communicate()
        assert p.returncode == 0, f"route query child failed under {e!r}"
        out[e or "default"] = json.loads(stdout)
    return out


def dumps(t):
    """One row per line: a readable diff when a route changes."""
    body = ",\n".join(
        json.dumps(e) + ": [\n" + ",\n".join(
            "  " + json.dumps(r) for r in rs) + "\n]" for e, rs in t.items())
    return "{\n" + body + "\n}\n"


if __name__ == "__main__":
    if "--rows" in sys.argv:
        print(json.dumps(rows()))
    else:
        sys.stdout.write(dumps(table()))
