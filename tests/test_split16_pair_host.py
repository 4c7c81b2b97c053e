"""The pair plan of the three-product split route (conv_split16.hip / conv_split16_c.hip: the tap-paired 16x16x32 body, variant 9) on
the host: queries only, and the lane map of the body's fragment reads.

The plan grants 3x3x3 filters with Cin % 16 == 0 whose 256-voxel tiling gives at least 256 (tile, 64-channel block) units and at least
2^25 voxel x Cin x Cout products, and -- where a workgroup has a single tile -- eight chunks; ``diqt_set_conv_f9h_mode(2)`` lifts the floors.  Everything the other two plans answer is unchanged
(test_split16_host.py, test_split16_fill_host.py)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_split16_fill_host import K, TINY  # noqa: E402

# the launches of a C2 sampler step that run variant 6 today
# (64 -> 128 @ 8 x 16^3, the fifth, was sent back by measurement: one tile of four chunks per workgroup does not pay for the prologue)
C2 = [(8, 32, 32, 32, 64, 64), (8, 32, 32, 32, 128, 64), (8, 16, 16, 16, 128, 128), (8, 16, 16, 16, 192, 128)]


@pytest.fixture(scope="module")
def lib():
    from diffusioniqt_amd import _lib
    _lib.load()
    assert _lib.query("diqt_set_conv_f9h_mode", -1) == 1
    return _lib


def test_pair_plan_grants_the_c2_launches_of_variant_6(lib):
    for geo in C2:
        assert lib.query("diqt_conv3d_fwd_split16_pair_supported", *geo, *K) == 1, geo
        assert lib.query("diqt_conv3d_fwd_gn_split16_pair_supported", *geo, *K, 1) == 1, geo
        assert lib.query("diqt_conv3d_fwd_split16_fill_variant", *geo, *K) == 6, geo
        rows = lib.query("diqt_conv3d_fwd_split16_pair_stats_blocks", *geo, *K)
        assert rows == lib.query("diqt_conv3d_fwd_split16_stats_blocks", *geo, *K) > 0, geo


def test_pair_plan_refuses(lib):
    sup = lambda *geo: lib.query("diqt_conv3d_fwd_split16_pair_supported", *geo, *K)
    for geo in TINY:
        assert sup(*geo) == 0, geo
        assert lib.query("diqt_conv3d_fwd_split16_pair_stats_blocks", *geo, *K) == 0, geo
    assert sup(8, 16, 16, 16, 64, 64) == 0            # 128 units: the fill plan's 128-voxel tiles
    assert sup(8, 8, 8, 8, 128, 128) == 0             # 32 units
    assert sup(8, 16, 16, 16, 64, 128) == 0           # one tile of four chunks per workgroup: sent back (slower than variant 6 when measured)
    assert sup(6, 16, 32, 32, 16, 128) == 1 and sup(5, 16, 32, 32, 16, 128) == 1      # walks of several tiles stay, whatever their chunks
    assert sup(8, 32, 32, 32, 24, 64) == 0            # Cin % 16
    assert lib.query("diqt_conv3d_fwd_split16_pair_supported", 8, 32, 32, 32, 64, 64, 1, 3, 3, 0, 1, 1, 0, 0, 0) == 0     # 3x3x3 only
    assert lib.query("diqt_conv3d_fwd_gn_split16_pair_supported", 8, 32, 32, 32, 64, 64, *K, 99) == 0                     # unknown activation


def test_mode_2_lifts_the_floors_and_nothing_else_changes(lib):
    geo = (1, 8, 8, 16, 16, 64)
    q = lambda name: lib.query(f"diqt_conv3d_fwd_split16_pair_{name}", *geo, *K)
    before = [lib.query(f"diqt_conv3d_fwd_split16{s}", 8, 32, 32, 32, 64, 64, *K) for s in ("_variant", "_fill_variant", "_stats_blocks")]
    assert q("supported") == 0 and before == [6, 6, 256]
    prev = lib.query("diqt_set_conv_f9h_mode", 2)
    try:
        assert q("supported") == 1 and q("stats_blocks") == lib.query("diqt_conv3d_fwd_split16_stats_blocks", *geo, *K) == 4 * 2      # 2 x 1 x 2 tiles, two voxel halves each
        assert lib.query("diqt_conv3d_fwd_split16_fill_variant", 8, 32, 32, 32, 64, 64, *K) == 6
    finally:
        lib.query("diqt_set_conv_f9h_mode", prev)
    assert q("supported") == 0
    assert [lib.query(f"diqt_conv3d_fwd_split16{s}", 8, 32, 32, 32, 64, 64, *K) for s in ("_variant", "_fill_variant", "_stats_blocks")] == before
    assert lib.query("diqt_set_conv_split16_fill_tile", 9) in (0,) and lib.query("diqt_set_conv_split16_fill_tile", -1) == 0      # domain {6, 7, 8}


def test_ops_plan_order(lib, monkeypatch):
    from diffusioniqt_amd import ops
    asked = []
    answers = {}

    def query(name, *args):
        asked.append(name)
        return answers.get(name, 0)
    monkeypatch.setattr(ops._lib, "query", query)
    geo = (8, 32, 32, 32, 64, 64, *K)
    P, F, S = ("diqt_conv3d_fwd_gn_split16_pair_supported", "diqt_conv3d_fwd_gn_split16_fill_supported", "diqt_conv3d_fwd_gn_split16_supported")
    answers.update({P: 1, F: 1, S: 1})
    assert ops._split16_plan(geo, 0, "pair") == "_pair" and asked == [P]
    asked.clear(); answers[P] = 0
    assert ops._split16_plan(geo, 0, "pair") == "_fill" and asked == [P, F]
    asked.clear(); answers[F] = 0
    assert ops._split16_plan(geo, 0, "pair") == "" and asked == [P, F, S]
    asked.clear(); answers[S] = 0
    assert ops._split16_plan(geo, 0, "pair") is None and asked == [P, F, S]
    # "fill" and True: what they answered before, the pair plan is not asked
    answers.update({P: 1, F: 1, S: 1}); asked.clear()
    assert ops._split16_plan(geo, 0, "fill") == "_fill" and asked == [F]
    asked.clear()
    assert ops._split16_plan(geo, 0, True) == "" and asked == [S]
    asked.clear(); answers[F] = 0
    assert ops._split16_plan(geo, 0, "fill") == "" and asked == [F, S]
    asked.clear()
    assert ops._split16_plan(geo, 0, False) is None and asked == []
    monkeypatch.setattr(ops, "SPLIT16", False)
    assert ops._split16_plan(geo, 0, "pair") is None and asked == []


def test_pair_lane_map_is_conflict_free(lib):
    """The host query counts, from the kernel header's own address function, the worst number of distinct addresses on one 16-byte LDS
    slot among the lanes a ds_read_b128 serves together: 14 pair steps, heads and tails, eight column blocks, both voxel halves."""
    assert lib.query("diqt_conv_split16_pair_lds_conflicts") == 1
