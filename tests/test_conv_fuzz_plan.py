"""What tests/test_gpu_conv_fuzz.py will run, proven without a GPU: the plan of tests/conv_fuzz_plan.py is reproducible, stays inside the
caps where the float64 reference is affordable and the suite's tolerances are known to hold, and -- by the library's own shape queries --
reaches every kernel of the conv3d dispatch, with cases on both sides of each planner threshold.  These are conditions, not measurements:
a planner whose threshold moves turns a threshold test red until the constructed shape is moved with it.  ``pytest -s`` prints the table
target -> number of planned cases.  (That the queries tell the truth is the GPU worker's part: it compares the launches it sees with them.)
"""
import os

import pytest

from tests import conv_fuzz_plan as plan

K333, K133, K311, K111 = plan.K333, plan.K133, plan.K311, plan.K111


@pytest.fixture(scope="module")
def planned():
    """[(seed, case, route)] of the default family; the routes are those of the default configuration"""
    assert not [k for k in os.environ if k in ("DIQT_CONV_F9", "DIQT_CONV_F9W")], "the coverage proof is for the default configuration"
    return [(seed, c, plan.route(c)) for seed in plan.DEFAULT_SEEDS for c in plan.cases("default", seed)]


def cdiv(a, b):
    return -(-a // b)


def ntiles(case, tile):
    """tiles of extent ``tile`` over the whole batch of a case's output"""
    n = case[0]
    for o, t in zip(plan.out_extent(case), tile):
        n *= cdiv(o, t)
    return n


def taps(c):
    return c[6][0] * c[6][1] * c[6][2]


def causal(c):
    return c[8][0] < 0


W3_TILE = {K333: (2, 4, 8), K133: (1, 8, 8), K311: (8, 2, 4)}      # conv_wgrad3_kernel's 64-voxel tiles (conv_wgrad.hip)


def wgrad3_several_tiles(c):
    """more than 256 tiles: a grid has at most 256 split-K ranges, so some workgroup walks several (the in-loop prefetch of the next tile)"""
    return (plan.voxels(c) // 64 if c[6] == K111 else ntiles(c, W3_TILE[c[6]])) > 256


def targets():
    """{name: predicate(case, route)}"""
    t = {}
    fw = lambda r: r["fwd"]
    bw = lambda r: r["bwd_data"] or {"kid": None, "variant": -1, "split": False, "kernel": ""}
    wg = lambda r: r["wgrad"] or {"kid": None, "kind": ""}
    t["fwd id0 conv_fwd_kernel"] = lambda c, r: fw(r)["kid"] == 0 and not fw(r)["split"]
    t["fwd id0 split-K"] = lambda c, r: fw(r)["kid"] == 0 and fw(r)["split"]
    t["fwd id1 conv_fwd_smallcin_kernel"] = lambda c, r: fw(r)["kid"] == 1
    t["fwd id2 conv1x1_fwd_kernel"] = lambda c, r: fw(r)["kid"] == 2
    t["fwd id3 conv_fwd8_kernel"] = lambda c, r: fw(r)["kid"] == 3
    t["fwd id4 conv_fwd9_kernel"] = lambda c, r: fw(r)["kid"] == 4
    for v in range(8):
        t["fwd conv_fwd9 variant %d un-split" % v] = lambda c, r, v=v: fw(r)["kid"] == 4 and fw(r)["variant"] == v and not fw(r)["split"]
    t["fwd conv_fwd9 split-K 3x3x3 direct"] = lambda c, r: fw(r)["kid"] == 4 and fw(r)["split"] and fw(r)["variant"] in (0, 1)
    t["fwd conv_fwd9 split-K 1x3x3"] = lambda c, r: fw(r)["kid"] == 4 and fw(r)["split"] and fw(r)["variant"] in (2, 3, 4)
    t["fwd conv_fwd9 split-K 3x1x1"] = lambda c, r: fw(r)["kid"] == 4 and fw(r)["split"] and fw(r)["variant"] in (5, 6)
    t["fwd conv_fwd9 split-K Winograd"] = lambda c, r: fw(r)["kid"] == 4 and fw(r)["split"] and fw(r)["variant"] == 7
    t["fwd statistics from the epilogue"] = lambda c, r: plan.want_stats(c) and fw(r)["stats_blocks"] > 0
    t["fwd conv_fwd9 split-K refused for statistics"] = lambda c, r: fw(r).get("stats_fallback", False)
    for k, co in ((K111, 1), (K133, 1), (K333, 1), (K311, 1), (K111, 2), (K133, 2)):
        t["fwd conv_smallcout_kernel %dx%dx%d Cout %d" % (*k, co)] = lambda c, r, k=k, co=co: fw(r)["kernel"] == "smallcout" and c[6] == k and c[5] == co
    for i in range(5):
        t["bwd-data id%d" % i] = lambda c, r, i=i: bw(r)["kid"] == i
    t["bwd-data id0 split-K"] = lambda c, r: bw(r)["kid"] == 0 and bw(r)["split"]
    t["bwd-data id4 split-K"] = lambda c, r: bw(r)["kid"] == 4 and bw(r)["split"]
    t["bwd-data causal"] = lambda c, r: r["bwd_data"] is not None and causal(c)
    t["bwd-data causal on conv_fwd9"] = lambda c, r: bw(r)["kid"] == 4 and causal(c)
    for k in (K333, K133, K311, K111):
        t["wgrad id3 conv_wgrad3_kernel %dx%dx%d" % k] = lambda c, r, k=k: wg(r)["kid"] == 3 and c[6] == k
    t["wgrad id3 3x1x1 causal"] = lambda c, r: wg(r)["kid"] == 3 and c[6] == K311 and causal(c)
    t["wgrad id3 several tiles per workgroup"] = lambda c, r: wg(r)["kid"] == 3 and wgrad3_several_tiles(c)
    t["wgrad id2 conv_bwd_weight2_kernel <= 3 taps"] = lambda c, r: wg(r)["kid"] == 2 and taps(c) <= 3
    t["wgrad id2 4..12 taps"] = lambda c, r: wg(r)["kid"] == 2 and 4 <= taps(c) <= 12
    t["wgrad id2 > 12 taps"] = lambda c, r: wg(r)["kid"] == 2 and taps(c) > 12
    t["wgrad id1 conv_bwd_weight_kernel"] = lambda c, r: wg(r)["kid"] == 1
    t["wgrad id0 column sum (Cout 1, 1x1x1)"] = lambda c, r: wg(r)["kind"] == "colsum"
    t["wgrad id0 im2col + GEMM (Cin <= 4)"] = lambda c, r: wg(r)["kind"] == "im2col"
    t["wgrad id0 split-K GEMM (1x1x1)"] = lambda c, r: wg(r)["kind"] == "pw"
    t["wgrad Cin <= 4 below 4096 voxels"] = lambda c, r: r["wgrad"] is not None and c[4] <= 4 and taps(c) > 1 and plan.voxels(c) < 4096
    for g in ("xw", "x", "w"):
        t["gradients required: " + g] = lambda c, r, g=g: c[10] == g
    t["residual"] = lambda c, r: c[9]
    return t


def test_every_dispatch_target_is_planned_three_times(planned):
    table = {name: sum(1 for _, c, r in planned if pred(c, r)) for name, pred in targets().items()}
    print()
    for name, n in table.items():
        print(f"{n:4d}  {name}")
    print(f"{len(planned):4d}  cases in all")
    short = {name: n for name, n in table.items() if n < 3}
    assert not short, f"targets planned fewer than 3 times: {short}"
    # the Winograd tile has no backward-data form (pack mode 1 carries no panels)
    assert not [c for _, c, r in planned if r["bwd_data"] is not None and r["bwd_data"]["variant"] == 7]


def test_cases_on_both_sides_of_each_planner_threshold(planned):
    """The constructed cases: the count the planner compares is recomputed here from the tile sizes in csrc/, and the route has to be the
    one that side of the threshold gives."""
    for seed in plan.DEFAULT_SEEDS:
        import random
        fixed = plan.fixed_cases(random.Random(seed))
        cases = plan.cases("default", seed)
        assert cases[:len(fixed)] == list(fixed.values()), "a seed's plan starts with its constructed cases"
        R = {lab: plan.route(c) for lab, c in fixed.items()}
        nwg9 = lambda c, cout: ntiles(c, (4, 8, 8)) * cdiv(cout, 64)
        # f9_try: fewer than 241 workgroups, or less than 0.94 of whole rounds of 256, is not conv_fwd9_kernel's (4x8x8 tiles here)
        for n, on in ((240, False), (241, True), (256, True), (258, False), (272, False)):
            c = fixed["f9_try %d" % n]
            assert nwg9(c, c[5]) == n and c[4] == 16                      # one 16-channel chunk: no split-K to fall back on
            assert (R["f9_try %d" % n]["fwd"]["kid"] == 4) == on, (n, R["f9_try %d" % n])
            assert not R["f9_try %d" % n]["fwd"]["split"]
        # ... its split-K form: 256 / workgroups shares; 2 x 120 = 240 is refused, 2 x 121 taken (backward-data: Cin is the output)
        for n, on in ((120, False), (121, True)):
            c, r = fixed["f9_try split %dx2" % n], R["f9_try split %dx2" % n]["bwd_data"]
            assert nwg9(c, c[4]) == n and c[5] == 32
            assert (r["kid"] == 4 and r["split"]) == on and (on or r["kid"] == 0), (n, r)
        # fwd8_plan: 256 workgroups of 256 voxels
        for n, on in ((255, False), (256, True)):
            c = fixed["fwd8 %d" % n]
            assert nwg9(c, c[5]) == n and c[4] % 16 != 0 and c[4] % 4 == 0
            assert (R["fwd8 %d" % n]["fwd"]["kid"] == 3) == on, (n, R["fwd8 %d" % n])
        # fwd_ksplit: `nwg >= 384` is its written threshold, but 512 / nwg shares make 256 | 257 the one that decides
        for n, split in ((256, True), (257, False), (383, False), (384, False)):
            c, r = fixed["fwd_ksplit %d" % n], R["fwd_ksplit %d" % n]["fwd"]
            assert ntiles(c, (1, 8, 16)) == n and cdiv(c[4], 32) == 2 and r["kid"] == 0
            assert r["split"] == split, (n, r)
        # wgrad3_plan: Cin >= 16
        for cin, on in ((12, False), (16, True), (20, True)):
            c = fixed["wgrad3_plan Cin %d" % cin]
            assert c[4] == cin and c[5] % 4 == 0 and (R["wgrad3_plan Cin %d" % cin]["wgrad"]["kid"] == 3) == on
        # pw_plan / sc_plan: >= 4096 voxels; pw_plan: more than 64 channels on the larger side
        for V, on in ((4032, False), (4096, True), (4160, True)):
            for what, kind in (("pw_plan", "pw"), ("sc_plan", "im2col")):
                c = fixed["%s V %d" % (what, V)]
                assert plan.voxels(c) == V and (R["%s V %d" % (what, V)]["wgrad"]["kind"] == kind) == on
        c = fixed["pw_plan M 64"]
        assert max(c[4], c[5]) == 64 and plan.voxels(c) >= 4096 and R["pw_plan M 64"]["wgrad"]["kind"] != "pw"
        c = fixed["pw_plan M 68, dY first"]
        assert max(c[4], c[5]) == 68 and c[5] > c[4] and R["pw_plan M 68, dY first"]["wgrad"]["kind"] == "pw"
        assert R["f9 split refused for statistics"]["fwd"].get("stats_fallback")


def test_reference_budget_and_tolerance_validity():
    """float64 F.conv3d + autograd on 16 threads took 0.1-0.65 s per 1e9 multiply-adds when the caps were set; the GPU test's docstring
    holds what a seed really takes."""
    for family, seeds in (("default", plan.DEFAULT_SEEDS), ("f9small", plan.F9SMALL_SEEDS)):
        for seed in seeds:
            cases = plan.cases(family, seed)
            for c in cases:
                B, D, H, W, Cin, Cout, k, pad, epad, res, grads = c
                assert min(plan.out_extent(c)) >= 1 and min(B, Cin, Cout) >= 1
                assert plan.macs(c) <= plan.MAX_MACS_CASE, c
                assert plan.voxels(c) <= plan.MAX_VOXELS, c                      # the longest weight-gradient reduction held to 5e-5
                assert max(Cin, Cout) * taps(c) <= plan.MAX_RED, c               # the longest forward reduction held to 2e-5
                assert all(p in (0, kk // 2) for p, kk in zip(pad[1:], k[1:])) and grads in ("xw", "x", "w")
                assert (pad[0], epad) in ((0, (0, 0, 0)), (k[0] // 2, (0, 0, 0)), (k[0] - 1, (1 - k[0], 0, 0))), c      # symmetric or causal
                assert k != (1, 15, 15) or Cin <= 4
            assert sum(plan.macs(c) for c in cases) <= plan.MAX_MACS_SEED, (family, seed)
    assert (plan.MAX_VOXELS, plan.MAX_RED, plan.MAX_MACS_CASE, plan.MAX_MACS_SEED) == (65536, 10368, 8e9, 1.5e11)


def test_plan_is_reproducible():
    for seed in plan.DEFAULT_SEEDS:
        assert plan.cases("default", seed) == plan.cases("default", seed)
    assert plan.cases("default", 11) != plan.cases("default", 12)
    # the shapes tests/test_gpu_conv_fuzz.py has always run through conv_fwd9_kernel (36 draws, those with an empty output dropped)
    a, b = plan.cases("f9small", 1), plan.cases("f9small", 2)
    assert (len(a), len(b)) == (33, 28)
    assert a[0] == (3, 3, 9, 4, 64, 64, (3, 3, 3), (1, 1, 1), (0, 0, 0), False, "xw")
    assert a[-1] == (1, 8, 6, 4, 64, 64, (1, 3, 3), (0, 1, 1), (0, 0, 0), False, "xw")
    assert b[0] == (1, 3, 12, 6, 48, 40, (3, 3, 3), (0, 0, 0), (0, 0, 0), False, "xw")
    assert b[-1] == (2, 3, 3, 2, 32, 40, (3, 3, 3), (1, 1, 1), (0, 0, 0), True, "xw")
    assert a == plan.cases("f9small", 1)


def test_the_router_follows_the_library_on_known_shapes():
    """Shapes whose kernels tests/test_gpu_kernels.py names, so that a router that drifts from ops.conv3d is caught here too."""
    r = plan.route((8, 32, 32, 32, 64, 64, K333, (1, 1, 1), (0, 0, 0), True, "xw"))
    assert (r["fwd"]["kid"], r["fwd"]["variant"], r["fwd"]["split"]) == (4, 7, False) and r["fwd"]["stats_blocks"] > 0
    assert (r["bwd_data"]["kid"], r["bwd_data"]["variant"]) == (4, 0) and r["wgrad"]["kind"] == "v3"
    r = plan.route((8, 8, 8, 8, 256, 256, K333, (1, 1, 1), (0, 0, 0), False, "w"))
    assert r["fwd"]["kid"] == 4 and r["fwd"]["split"] and r["fwd"]["stats_blocks"] == 0 and r["bwd_data"] is None
    r = plan.route((8, 32, 8, 8, 256, 256, K311, (2, 0, 0), (-2, 0, 0), False, "x"))
    assert r["fwd"]["kid"] == 4 and r["bwd_data"]["kid"] == 4 and r["wgrad"] is None
    r = plan.route((1, 16, 16, 16, 64, 1, K111, (0, 0, 0), (0, 0, 0), False, "xw"))
    assert r["fwd"]["kernel"] == "smallcout" and r["wgrad"]["kind"] == "colsum"
    r = plan.route((2, 16, 16, 16, 2, 24, K333, (1, 1, 1), (0, 0, 0), False, "xw"))
    assert r["fwd"]["kid"] == 1 and r["wgrad"]["kind"] == "im2col"
    assert plan.wgrad_tags(r["wgrad"])["conv3d_bwd_weight(im2col)"] == 1
