"""Conv routing is pinned: tools/conv_route_table.py regenerates, on the CPU,
the route / split-K / slice / BN-fusion answer of every geometry under every
knob setting, and it must equal tests/golden/conv_routes.json exactly. A
deliberate retune regenerates the golden file in the same change."""

import json
import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
import conv_route_table as T  # noqa: E402

pytestmark = pytest.mark.skipif(
    not os.path.exists(os.path.join(REPO, "cilfw", "_hip_lib.so")),
    reason="cilfw/_hip_lib.so not built")


def test_geometry_list_covers_the_gpu_route_tests():
    import test_conv_routes_gpu as G
    geoms = set(T.GEOMS)
    assert set(G.FUZZ) <= geoms and set(G.DW_GEOMS) <= geoms
    assert {s[:8] for s in G.BN_PARTS_SHAPES} <= geoms
    assert {(N, h, w, C, K, 3, 1, 1)
            for N, h, w, C, K, _, _ in G.BNP_SHAPES} <= geoms


def test_routes_match_golden_table():
    with open(os.path.join(REPO, "tests", "golden", "conv_routes.json")) as f:
        golden = json.load(f)
    got = T.table()
    assert list(got) == list(golden)
    for env in golden:
        for g, w in zip(got[env], golden[env]):
            assert g == w, (env, g, w)
        assert len(got[env]) == len(golden[env])
