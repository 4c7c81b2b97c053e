"""The fill plan of the three-product split route (conv_split16.hip / conv_split16_b.hip) on the host: queries only.

The plan tries the 256-, 128- and 64-voxel tiles (conv_f9h_kernel variants 6, 7, 8) in that order, a smaller one only when the larger
gives fewer than 256 (tile, 64-channel block) units; it grants at 128 units or more and B Do Ho Wo Cin Cout >= 2^25.  The plan behind
``diqt_conv3d_fwd_split16*`` answers what it answered before (the geometries of test_split16_host.py)."""
import pytest

K = (3, 3, 3, 1, 1, 1, 0, 0, 0)
# the parity suite's tiny U-Nets and the ragged cases of the Winograd suite (test_split16_host.py): all below 1.9e7 products
TINY = [(1, 8, 8, 8, 16, 16), (2, 8, 8, 8, 16, 32), (1, 16, 16, 16, 16, 16), (2, 16, 16, 16, 32, 32), (1, 4, 4, 4, 32, 32),
        (2, 13, 11, 16, 48, 64), (2, 8, 16, 16, 64, 72), (2, 8, 8, 8, 8, 8), (1, 16, 16, 16, 24, 24)]


@pytest.fixture(scope="module")
def lib():
    from diffusioniqt_amd import _lib
    _lib.load()
    assert _lib.query("diqt_set_conv_f9h_mode", -1) == 1 and _lib.query("diqt_set_conv_split16_fill_tile", -1) == 0
    return _lib


def test_old_queries_answer_as_before(lib):
    q = lambda *geo: lib.query("diqt_conv3d_fwd_split16_supported", *geo, *K)
    for geo in TINY:
        assert q(*geo) == 0, geo
        assert lib.query("diqt_conv3d_fwd_split16_variant", *geo, *K) == -1 and lib.query("diqt_conv3d_fwd_split16_stats_blocks", *geo, *K) == 0
    assert q(8, 32, 32, 32, 64, 64) == 1 and q(8, 16, 16, 16, 128, 128) == 1 and q(8, 16, 16, 16, 64, 64) == 1
    assert q(8, 8, 8, 8, 256, 256) == 0 and q(8, 8, 8, 8, 128, 128) == 0
    assert q(8, 32, 32, 32, 24, 64) == 0 and q(8, 32, 32, 32, 64, 60) == 0
    assert lib.query("diqt_conv3d_fwd_split16_supported", 8, 32, 32, 32, 64, 64, 1, 3, 3, 0, 1, 1, 0, 0, 0) == 0
    assert lib.query("diqt_conv3d_fwd_gn_split16_supported", 8, 32, 32, 32, 64, 64, *K, 99) == 0
    assert lib.query("diqt_conv3d_fwd_split16_stats_blocks", 8, 32, 32, 32, 64, 64, *K) == 128 * 2
    for geo in [(8, 32, 32, 32, 64, 64), (8, 16, 16, 16, 128, 128), (8, 16, 16, 16, 64, 64)]:
        assert lib.query("diqt_conv3d_fwd_split16_variant", *geo, *K) == 6, geo
    assert lib.query("diqt_conv3d_fwd_split16_stats_blocks", 8, 16, 16, 16, 64, 64, *K) == 16 * 2
    assert lib.query("diqt_conv3d_fwd_split16_variant", 8, 8, 8, 8, 128, 128, *K) == -1


def test_fill_plan_refuses_tiny_networks(lib):
    for geo in TINY:
        assert geo[0] * geo[1] * geo[2] * geo[3] * geo[4] * geo[5] < 1.9e7
        assert lib.query("diqt_conv3d_fwd_split16_fill_supported", *geo, *K) == 0, geo
        assert lib.query("diqt_conv3d_fwd_split16_fill_variant", *geo, *K) == -1, geo
        assert lib.query("diqt_conv3d_fwd_split16_fill_stats_blocks", *geo, *K) == 0, geo
        assert lib.query("diqt_conv3d_fwd_gn_split16_fill_supported", *geo, *K, 1) == 0, geo


def test_fill_plan_tiles(lib):
    sup = lambda *geo: lib.query("diqt_conv3d_fwd_split16_fill_supported", *geo, *K)
    var = lambda *geo: lib.query("diqt_conv3d_fwd_split16_fill_variant", *geo, *K)
    rows = lambda *geo: lib.query("diqt_conv3d_fwd_split16_fill_stats_blocks", *geo, *K)
    # C2, 64 -> 64 @ 8 x 16^3: 128 units of 256 voxels -> 256 units of 128 voxels; 32 tiles x 2 voxel halves per entry
    assert sup(8, 16, 16, 16, 64, 64) == 1 and var(8, 16, 16, 16, 64, 64) == 7 and rows(8, 16, 16, 16, 64, 64) == 64
    # C2, 128 -> 128 @ 8 x 8^3: 32 units of 256 voxels, 64 of 128, 128 of 64
    assert sup(8, 8, 8, 8, 128, 128) == 1 and var(8, 8, 8, 8, 128, 128) == 8 and rows(8, 8, 8, 8, 128, 128) == 16
    # launches that fill 256 workgroups with 256-voxel tiles keep them
    assert var(8, 32, 32, 32, 64, 64) == 6 and rows(8, 32, 32, 32, 64, 64) == 256
    assert var(8, 16, 16, 16, 128, 128) == 6 and rows(8, 16, 16, 16, 128, 128) == 32
    # the floors: 64 units of 64-voxel tiles (three ways); 128 units but 8.4e6 products
    assert sup(1, 16, 16, 16, 64, 64) == 0 and sup(1, 8, 8, 8, 512, 512) == 0 and sup(8, 8, 8, 8, 64, 64) == 0
    assert sup(2, 16, 16, 16, 32, 32) == 0 and sup(2, 16, 16, 16, 64, 64) == 1
    # 64-voxel tiles on fewer than 256 workgroups: up to Cin = 128 (measured: 256 -> 128 @ 8 x 8^3 is slower than the Winograd launch)
    assert sup(8, 8, 8, 8, 256, 128) == 0 and sup(8, 8, 8, 8, 256, 256) == 1 and var(8, 8, 8, 8, 256, 256) == 8
    # the domain of the route
    assert sup(8, 32, 32, 32, 24, 64) == 0 and sup(8, 32, 32, 32, 64, 60) == 0                                           # Cin % 16, Cout % 8
    assert lib.query("diqt_conv3d_fwd_split16_fill_supported", 8, 32, 32, 32, 64, 64, 1, 3, 3, 0, 1, 1, 0, 0, 0) == 0   # 3x3x3 only
    assert lib.query("diqt_conv3d_fwd_gn_split16_fill_supported", 8, 16, 16, 16, 64, 64, *K, 99) == 0                   # unknown activation
    assert lib.query("diqt_conv3d_fwd_gn_split16_fill_supported", 8, 16, 16, 16, 64, 64, *K, 1) == 1


def test_mode_2_lifts_the_floors_and_the_pinned_tile_needs_it(lib):
    geo = (1, 8, 8, 16, 16, 64)
    q = lambda name: lib.query(f"diqt_conv3d_fwd_split16_fill_{name}", *geo, *K)
    assert q("supported") == 0
    assert lib.query("diqt_set_conv_split16_fill_tile", 7) == 0
    try:
        assert q("supported") == 0, "a pinned tile without mode 2 changes nothing"
        assert lib.query("diqt_conv3d_fwd_split16_fill_variant", 8, 32, 32, 32, 64, 64, *K) == 6
        prev = lib.query("diqt_set_conv_f9h_mode", 2)
        try:
            assert q("supported") == 1 and q("variant") == 7 and q("stats_blocks") == 4 * 2 * 2
            assert lib.query("diqt_set_conv_split16_fill_tile", 8) == 7
            assert q("variant") == 8 and q("stats_blocks") == 8 * 2 * 2
            assert lib.query("diqt_set_conv_split16_fill_tile", 0) == 8
            assert q("variant") == 8, "unpinned: 4 units of 256 voxels, 8 of 128, 16 of 64 -- the smallest tile"
            assert lib.query("diqt_conv3d_fwd_split16_variant", *geo, *K) == 6
        finally:
            lib.query("diqt_set_conv_f9h_mode", prev)
    finally:
        lib.query("diqt_set_conv_split16_fill_tile", 0)
    assert q("supported") == 0
