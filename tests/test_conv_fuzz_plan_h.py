"""What tests/test_gpu_conv_fuzz_h.py will run, proven without a GPU: the plan of tests/conv_fuzz_plan_h.py is reproducible, stays inside
its caps, and -- by the library's own shape queries -- reaches every kernel of the 16-bit conv dispatch, with cases on both sides of each
threshold.  ``mirror_hid`` restates convh_route (conv_half.hip: half_geom's tile choice, the prefetch / persistent / four-wave / GEMM /
conv_f9h rules) from the constants in csrc/, and has to agree with diqt_conv3d_fwd_h_kernel_id on EVERY planned case: a planner whose
threshold moves turns this red until the restatement moves with it.  ``pytest -s`` prints the table target -> number of planned cases.
(That the queries tell the truth is the GPU worker's part: it compares the launches it sees with them.)

conv_f9h_kernel's variant 0 (H9_333_512, 8x8x8 tiles at one workgroup per CU) is a target no shape can reach: f9h_plan tries variant 1
(4x8x8 tiles, two workgroups per CU) first and replaces it only by a strictly shorter estimate, and variant 1 never has more than twice
variant 0's tiles for twice the workgroup slots at half the tile length, so variant 0's estimate is never shorter
(test_conv_f9h_variant_0_is_never_planned sweeps that).  It stays in the table; the day the planner can choose it, the sweep fails and
the plan owes it three cases.
"""
import os
import random

import pytest

from diffusioniqt_amd import _lib
from tests import conv_fuzz_plan_h as plan

K333, K133, K311, K111 = plan.K333, plan.K133, plan.K311, plan.K111
cdiv = plan.cdiv

# ---- constants of csrc/conv_half.hip ----
HCK, HROWB, HNT, HMT, HTG, HHREG = 32, 80, 64, 256, 9, 10
CAND = plan.HALF_TILES


def lds_bytes(HV, TG, NS=1, wbufs=2):
    return NS * HV * HROWB + wbufs * TG * HNT * HROWB + max(HMT + HV, 2 * HMT) * 4


def half_geom(B, D, H, W, Cin, Cout, k, pad, epad):
    """half_geom restated: None, or the tile it picks with what the launcher derives from it"""
    T = k[0] * k[1] * k[2]
    if Cin % 4 or (Cin < 8 and T > 1):
        return None
    if k == K111 and pad == (0, 0, 0) and epad == (0, 0, 0):
        B, D, H, W = 1, 1, 1, B * D * H * W
    out = [n + 2 * p + e - kk + 1 for n, p, e, kk in zip((D, H, W), pad, epad, k)]
    if min(out) <= 0:
        return None
    TG = min(T, HTG)
    best = None
    for t in CAND:
        HV = (t[0] + k[0] - 1) * (t[1] + k[1] - 1) * (t[2] + k[2] - 1)
        if lds_bytes(HV, TG) > 160 * 1024:
            continue
        tiles = cdiv(out[0], t[0]) * cdiv(out[1], t[1]) * cdiv(out[2], t[2])
        cost = tiles * (HV + 256.0 * T)
        if best is None or cost < best[0]:
            best = (cost, t, HV, tiles)
    if best is None:
        return None
    return {"tile": best[1], "HV": best[2], "units": B * best[3] * cdiv(Cout, HNT), "TG": TG, "groups": cdiv(T, TG), "chunks": cdiv(Cin, HCK),
            "rows": B * D * H * W, "same_extent": out == [D, H, W], "T": T}


def f9h_takes(c, mode):
    if not mode or c.k not in (K333, K133) or c.Cin % 32 or c.Cout % 8 or c.Cout < 8 or max(c.pad) > 16 or min(plan.out_extent(c)) <= 0:
        return False
    return plan.f9h_variant(c, mode) >= 0


def mirror_hid(c, xh, yh, res, stats, f9mode, wgs):
    """convh_route restated"""
    if xh and not (yh and res) and f9h_takes(c, f9mode):
        return 8
    g = half_geom(c.B, c.D, c.H, c.W, c.Cin, c.Cout, c.k, c.pad, c.epad)
    if g is None:
        return 0
    kd, kh, kw = c.k
    if (not yh and not stats and kh == 1 and kw == 1 and c.pad[1] == 0 and c.pad[2] == 0 and g["same_extent"] and c.Cin % HCK == 0
            and c.Cin >= 64 and g["rows"] >= 2048 and c.Cout >= 32):                                                  # pwh_takes
        if kd == 1 and not xh and c.pad[0] == 0:
            return 6
        if kd > 1 and xh and kd <= 4 and c.pad[0] < kd:
            return 7
    HV = g["HV"]
    if not (g["groups"] == 1 and HV * 8 <= 512 * HHREG and g["units"] >= 2 * wgs):                                   # convh_persistent_takes
        return 0 if (xh or yh or stats) else (1 if HV * 8 <= 512 * HHREG else 2)
    if (xh or yh) and not (c.Cin % 8 == 0 and c.Cout % 8 == 0 and (not yh or not res)):
        return 0
    if stats and (g["T"] == 1 or not xh):
        return 0
    ns2 = g["T"] == 1 and g["chunks"] >= 2 and xh
    NS, TG = (2, 2) if ns2 else (1, g["TG"])
    four = lds_bytes(HV, TG, NS, 1) <= 80 * 1024 - 1024 and ((g["T"] > 1 and xh and HV * 4 <= 256 * 6) or
                                                             (g["T"] == 1 and not xh and NS == 1 and HV * 8 <= 256 * 8))   # convh_four_waves
    return 5 if four else 4 if ns2 else 3


@pytest.fixture(scope="module")
def planned():
    assert not [k for k in os.environ if k.startswith("DIQT_CONV")], "the coverage proof is for the default configuration"
    assert (_lib.query("diqt_set_conv_f9h_mode", -1), _lib.query("diqt_set_convh_workgroups", 0)) == (1, 256)
    o = [(seed, c, plan.route_ops16(c)) for seed in plan.OPS16_SEEDS for c in plan.cases("ops16", seed)]
    i = [(seed, c, plan.route_io16(c)) for seed in plan.IO16_SEEDS for c in plan.cases("io16", seed)]
    assert (_lib.query("diqt_set_conv_f9h_mode", -1), _lib.query("diqt_set_convh_workgroups", 0)) == (1, 256), "the routers restore the switches"
    return {"ops16": o, "io16": i}


# x_half, y_half, statistics, residual: what diqt_conv3d_fwd_h_io accepts on some shape.  A 16-bit y takes no residual (conv_f9h_kernel
# is skipped for it, the persistent kernel refuses it, the others take no 16-bit y); statistics are built for a 16-bit x only.
ACCEPTED = [(xh, yh, st, rs) for xh in (0, 1) for yh in (0, 1) for st in (0, 1) for rs in (0, 1) if not (yh and rs) and not (st and not xh)]


def targets():
    """{name: (family, predicate(case, route))}"""
    t = {}
    halves = lambda r: [p for p in (r["fwd"], r["bwd_data"]) if p is not None and p["half"]]
    for hid in (1, 2, 3, 6):
        t["ops16 forward on id %d %s" % (hid, plan.HID_NAMES[hid])] = ("ops16", lambda c, r, h=hid: r["fwd"].get("hid") == h)
    for hid in range(1, 9):
        t["io16 id %d %s" % (hid, plan.HID_NAMES[hid])] = ("io16", lambda c, r, h=hid: c.op == "fwd" and r["hid"] == h)
    for v in range(1, 6):
        t["io16 conv_f9h_kernel variant %d" % v] = ("io16", lambda c, r, v=v: c.op == "fwd" and r["variant"] == v)
    for m in (1, 2):
        t["io16 conv_f9h_kernel in mode %d" % m] = ("io16", lambda c, r, m=m: c.op == "fwd" and r["hid"] == 8 and c.f9mode == m)
    for w in (1, 2, 3, 5, 256):
        t["io16 persistent kernel with %d workgroups" % w] = ("io16", lambda c, r, w=w: c.op == "fwd" and r["hid"] in (3, 4, 5) and c.wgs == w)
    for p in ("fp16", "bf16", "fp16s"):
        t["ops16 " + p] = ("ops16", lambda c, r, p=p: c.prec == p)
        t["ops16 %s forward on a 16-bit kernel" % p] = ("ops16", lambda c, r, p=p: c.prec == p and r["fwd"]["half"])
    for bf in (0, 1):
        t["io16 forward %s" % ("bf16" if bf else "fp16")] = ("io16", lambda c, r, bf=bf: c.op == "fwd" and r["ok"] and c.bf16 == bf)
    for xh, yh, st, rs in ACCEPTED:
        t["io16 x_half %d y_half %d statistics %d residual %d" % (xh, yh, st, rs)] = \
            ("io16", lambda c, r, k=(xh, yh, st, rs): c.op == "fwd" and r["ok"] and (c.xh, c.yh, int(c.stats), int(c.res)) == k)
    for st_kernel, ids in (("conv_f9h_kernel", (8,)), ("conv_fwd_hp_kernel, 8 waves", (3,)), ("conv_fwd_hp_kernel, 4 waves", (5,))):
        t["io16 statistics from " + st_kernel] = ("io16", lambda c, r, ids=ids: c.op == "fwd" and c.stats and r["hid"] in ids)
    for T in (25, 27, 49):
        t["ops16 %d taps on a 16-bit kernel" % T] = ("ops16", lambda c, r, T=T: plan.taps(c) == T and bool(halves(r)))
    # (no tile of a 5x5x5 filter fits half_geom's LDS budget: 125 taps always fall back)
    t["ops16 125 taps (fp32: beyond the 16-bit kernel's LDS)"] = ("ops16", lambda c, r: plan.taps(c) == 125 and not r["fwd"]["half"])
    t["ops16 mode-1 packing on a 16-bit kernel"] = ("ops16", lambda c, r: r["bwd_data"] is not None and r["bwd_data"]["half"])
    for hid in (1, 2, 3, 6):
        t["ops16 mode-1 packing on id %d" % hid] = ("ops16", lambda c, r, h=hid: r["bwd_data"] is not None and r["bwd_data"].get("hid") == h)
    t["ops16 mode-1 packing, causal"] = ("ops16", lambda c, r: r["bwd_data"] is not None and r["bwd_data"]["half"] and c.epad[0] < 0)
    t["ops16 mode-1 packing with fp16 under the scaler"] = ("ops16", lambda c, r: c.prec == "fp16s" and r["bwd_data"] is not None and r["bwd_data"]["half"])
    t["ops16 fp16 without a scaler: fp32 backward"] = ("ops16", lambda c, r: c.prec == "fp16" and r["fwd"]["half"] and "x" in c.grads and not r["bwd_data"]["half"])
    t["ops16 16-bit forward, fp32 backward-data (geometry)"] = \
        ("ops16", lambda c, r: c.prec != "fp16" and r["fwd"]["half"] and r["bwd_data"] is not None and not r["bwd_data"]["half"])
    t["ops16 fp32 forward, 16-bit backward-data"] = ("ops16", lambda c, r: r["fwd"]["kernel"] != "smallcout" and not r["fwd"]["half"] and r["bwd_data"] is not None and r["bwd_data"]["half"])
    for fam in ("ops16", "io16"):
        wg = (lambda c, r: r["wgrad"] if r["wgrad"] is not None and r["wgrad"]["half"] else None) if fam == "ops16" else \
             (lambda c, r: r if c.op == "wgrad" and r["ok"] else None)
        for k in (K333, K133, K311):
            t["%s conv_wgrad_h_kernel %dx%dx%d ksplit 1" % (fam, *k)] = (fam, lambda c, r, k=k, wg=wg: c.k == k and wg(c, r) is not None and wg(c, r)["ksplit"] == 1)
            t["%s conv_wgrad_h_kernel %dx%dx%d ksplit > 1" % (fam, *k)] = (fam, lambda c, r, k=k, wg=wg: c.k == k and wg(c, r) is not None and wg(c, r)["ksplit"] > 1)
        t["%s conv_wgrad_h_kernel several tiles per slice" % fam] = (fam, lambda c, r, wg=wg: wg(c, r) is not None and plan.wgradh_tiles(c) > wg(c, r)["ksplit"])
        t["%s conv_wgrad_h_kernel 3x1x1 causal" % fam] = (fam, lambda c, r, wg=wg: wg(c, r) is not None and c.epad[0] < 0)
    for xh, yh in ((0, 0), (1, 0), (1, 1)):
        t["io16 weight gradient flags x16 %d dY16 %d" % (xh, yh)] = ("io16", lambda c, r, k=(xh, yh): c.op == "wgrad" and r["ok"] and (c.xh, c.yh) == k)
    t["io16 weight gradient refused: dY16 without x16"] = ("io16", lambda c, r: c.op == "wgrad" and not r["ok"] and (c.xh, c.yh) == (0, 1))
    t["io16 weight gradient refused: shape"] = ("io16", lambda c, r: c.op == "wgrad" and not r["ok"] and r["nbytes"] == 0)
    t["ops16 weight gradient on an fp32 kernel after a 16-bit forward"] = ("ops16", lambda c, r: r["fwd"]["half"] and r["wgrad"] is not None and not r["wgrad"]["half"])
    t["ops16 forward falls back to fp32: Cin % 4"] = ("ops16", lambda c, r: not r["fwd"]["half"] and c.Cin % 4 != 0 and c.Cout > 2)
    t["ops16 forward falls back to fp32: Cin < 8 with taps"] = ("ops16", lambda c, r: not r["fwd"]["half"] and c.Cin == 4 and plan.taps(c) > 1 and c.Cout > 2)
    t["ops16 conv_smallcout_kernel (Cout <= 2)"] = ("ops16", lambda c, r: r["fwd"]["kernel"] == "smallcout")
    t["ops16 bias None"] = ("ops16", lambda c, r: not c.bias)
    t["ops16 bias None, weight gradient on conv_wgrad_h_kernel"] = ("ops16", lambda c, r: not c.bias and r["wgrad"] is not None and r["wgrad"]["half"])
    t["ops16 residual on a 16-bit forward"] = ("ops16", lambda c, r: c.res and r["fwd"]["half"])
    for g in ("xw", "x", "w"):
        t["ops16 gradients required: " + g] = ("ops16", lambda c, r, g=g: c.grads == g)
    t["ops16 unpadded"] = ("ops16", lambda c, r: c.pad == (0, 0, 0) and plan.taps(c) > 1 and r["fwd"]["half"])
    t["ops16 an extent of 1"] = ("ops16", lambda c, r: min(c.D, c.H, c.W) == 1 and r["fwd"]["half"])
    t["io16 refusal (forward)"] = ("io16", lambda c, r: c.op == "fwd" and not r["ok"])
    t["io16 refusal: 16-bit y with a residual"] = ("io16", lambda c, r: c.op == "fwd" and not r["ok"] and c.yh and c.res)
    t["io16 refusal: statistics with fp32 x"] = ("io16", lambda c, r: c.op == "fwd" and not r["ok"] and c.stats and not c.xh)
    t["io16 refusal: 16-bit tensors off the persistent kernel"] = ("io16", lambda c, r: c.op == "fwd" and not r["ok"] and r["io16"] == 0 and not c.stats and not c.res)
    return t


def test_every_16_bit_dispatch_target_is_planned_three_times(planned):
    table = {name: sum(1 for _, c, r in planned[fam] if pred(c, r)) for name, (fam, pred) in targets().items()}
    table["io16 conv_f9h_kernel variant 0 (unreachable: see the module docstring)"] = sum(1 for _, c, r in planned["io16"] if c.op == "fwd" and r["variant"] == 0)
    print()
    for name, n in table.items():
        print(f"{n:4d}  {name}")
    print(f"{len(planned['ops16']):4d}  ops16 cases, {len(planned['io16'])} io16 cases")
    short = {name: n for name, n in table.items() if n < 3 and "variant 0" not in name}
    assert not short, f"targets planned fewer than 3 times: {short}"
    nref = sum(1 for _, c, r in planned["io16"] if not r["ok"])
    assert 0.25 <= nref / len(planned["io16"]) <= 0.4, "about a third of the io16 cases are refusals: %d of %d" % (nref, len(planned["io16"]))
    # a combination outside ACCEPTED is refused on every shape
    assert not [c for _, c, r in planned["io16"] if c.op == "fwd" and r["ok"] and (c.xh, c.yh, int(c.stats), int(c.res)) not in ACCEPTED]
    assert [c for _, c, r in planned["io16"] if c.op == "fwd" and (c.xh, c.yh, int(c.stats), int(c.res)) not in ACCEPTED]


def test_conv_f9h_variant_0_is_never_planned():
    rnd = random.Random(5)
    for _ in range(20000):
        c = plan.i16(rnd.randint(1, 64), (rnd.randint(1, 70), rnd.randint(1, 70), rnd.randint(1, 70)), 32, 8 * rnd.randint(1, 80), K333,
                     pad=rnd.choice([(1, 1, 1), (0, 0, 0)]), f9mode=2)
        if min(plan.out_extent(c)) >= 1:
            assert plan.f9h_variant(c, 2) == 1, c
    # ... and the library agrees with the restatement where it can be asked: conv_f9h_kernel writes two statistics rows per tile
    for sp in ((8, 8, 8), (64, 64, 64), (9, 17, 33), (40, 8, 8)):
        c = plan.i16(2, sp, 32, 64, K333, f9mode=2)
        with plan.switches(2, 256):
            nblk = _lib.query("diqt_conv3d_fwd_h_stats_blocks", *plan.geo_of(c), 1, 0)
        t = plan.f9h_tiles_per_entry(c, 1)
        assert nblk == 2 * t[0] * t[1] * t[2], (sp, nblk)


def test_the_restated_dispatch_agrees_with_the_library_on_every_planned_case(planned):
    """Both sides of each threshold: mirror_hid recomputes halo voxels, units, rows and LDS bytes from the constants of csrc/."""
    n = 0
    for _, c, r in planned["io16"]:
        if c.op != "fwd":
            continue
        assert mirror_hid(c, c.xh, c.yh, c.res, c.stats, c.f9mode, c.wgs) == r["hid"], (c, r)
        if r["hid"] == 8:                                       # the variant restated in the plan against the library's tile count
            with plan.switches(c.f9mode, c.wgs):
                nblk = _lib.query("diqt_conv3d_fwd_h_stats_blocks", *plan.geo_of(c), 1, c.yh)
            t = plan.f9h_tiles_per_entry(c, r["variant"])
            assert nblk == 2 * t[0] * t[1] * t[2], (c, r, nblk)
        # io16_supported against the launch's own decision, both ways: without residual and statistics it promises the persistent kernel
        # or conv_f9h_kernel, except where the temporal GEMM takes 16-bit rows ahead of a persistent launch (fp32 y only)
        if (c.xh or c.yh) and not c.res and not c.stats:
            assert (r["io16"] == 1) == (r["hid"] in (3, 4, 5, 8)) or (r["hid"] == 7 and not c.yh), (c, r)
        if c.stats:
            assert (r["stats_blocks"] > 0) == (r["hid"] != 0) or (c.yh and c.res), (c, r)      # (the query knows of no residual)
            assert r["hid"] in (0, 3, 5, 8)
        n += 1
    for _, c, r in planned["ops16"]:
        for p, geo_c, res in ((r["fwd"], c, c.res), (r["bwd_data"], bwd_case(c), False)):
            if p is not None and p["half"]:
                assert mirror_hid(geo_c, 0, 0, res, False, 1, 256) == p["hid"], (c, p)
                n += 1
            elif p is not None and p["kernel"] != "smallcout":
                assert half_geom(geo_c.B, geo_c.D, geo_c.H, geo_c.W, geo_c.Cin, geo_c.Cout, geo_c.k, geo_c.pad, geo_c.epad) is None or \
                    (p is r["bwd_data"] and plan.LP_BACKWARD[c.prec] is None) or (p is r["bwd_data"] and r["fwd"]["kernel"] == "smallcout"), (c, p)
    assert n > 400


def bwd_case(c):
    """the forward-type geometry of a case's backward-data pass"""
    Do, Ho, Wo = plan.out_extent(c)
    return c._replace(D=Do, H=Ho, W=Wo, Cin=c.Cout, Cout=c.Cin, pad=tuple(kk - 1 - p for kk, p in zip(c.k, c.pad)), epad=tuple(-e for e in c.epad))


def test_constructed_cases_fall_on_the_intended_side():
    for seed in plan.OPS16_SEEDS:
        f = plan.fixed_ops16(random.Random(seed))
        assert plan.cases("ops16", seed)[:len(f)] == list(f.values()), "a seed's plan starts with its constructed cases"
        R = {lab: plan.route_ops16(c) for lab, c in f.items()}
        G = {lab: half_geom(c.B, c.D, c.H, c.W, c.Cin, c.Cout, c.k, c.pad, c.epad) for lab, c in f.items()}
        # prefetch: 640 halo voxels
        assert G["prefetch 600 halo voxels"]["HV"] == 600 and R["prefetch 600 halo voxels"]["fwd"]["hid"] == 1
        assert G["prefetch 720 halo voxels"]["HV"] == 720 and R["prefetch 720 halo voxels"]["fwd"]["hid"] == 2
        # persistent: units against twice the 256 workgroups
        assert G["persistent 510 units"]["units"] == 510 and R["persistent 510 units"]["fwd"]["hid"] == 1
        assert G["persistent 513 units"]["units"] == 513 and R["persistent 513 units"]["fwd"]["hid"] == 3
        r = R["persistent backward-data, 513 units"]
        assert r["fwd"]["hid"] == 1 and r["bwd_data"]["hid"] == 3 and f["persistent backward-data, 513 units"].Cin == 136
        assert G["persistent 3x1x1 causal"]["units"] >= 512 and R["persistent 3x1x1 causal"]["fwd"]["hid"] == 3
        # pwh_takes
        for lab, rows, hid in (("pwh rows 2047", 2047, 1), ("pwh rows 2048", 2048, 6), ("pwh Cin 32", 2048, 1), ("pwh Cin 64 Cout 24", 2048, 1),
                               ("pwh Cin 64 Cout 32", 2048, 6), ("pwh Cin 64 Cout 64", 2112, 6), ("pwh Cin 96 Cout 72, ragged rows", 2907, 6)):
            assert G[lab]["rows"] == rows and R[lab]["fwd"]["hid"] == hid, (lab, G[lab], R[lab])
        assert (f["pwh Cin 32"].Cin, f["pwh Cin 64 Cout 24"].Cout, f["pwh Cin 64 Cout 32"].Cout) == (32, 24, 32)
        # wgradh_plan
        assert not R["wgradh Cin 40"]["wgrad"]["half"] and not R["wgradh Cout 28"]["wgrad"]["half"] and R["wgradh Cout 32"]["wgrad"]["half"]
        for k in (K333, K133, K311):
            a, b = "wgradh %dx%dx%d ksplit 1" % k, "wgradh %dx%dx%d ksplit > 1" % k
            assert plan.wgradh_tiles(f[a]) == 1 and R[a]["wgrad"]["ksplit"] == 1
            blocks = cdiv(f[b].Cout, 64) * (f[b].Cin // 32)
            assert R[b]["wgrad"]["ksplit"] == min(256 // blocks, plan.wgradh_tiles(f[b])) > 1, (b, R[b])
        c = f["wgradh several tiles per slice"]
        blocks = cdiv(c.Cout, 64) * (c.Cin // 32)
        assert plan.wgradh_tiles(c) > 256 // blocks and R["wgradh several tiles per slice"]["wgrad"]["ksplit"] <= 256 // blocks
        assert R["wgradh fp16 without a scaler stays fp32"]["wgrad"]["half"] is False and f["wgradh fp16 without a scaler stays fp32"].prec == "fp16"
        # fallbacks
        assert not R["fallback Cin 6"]["fwd"]["half"] and not R["fallback Cin 4, 3x3x3"]["fwd"]["half"] and R["Cin 4, 1x1x1 is taken"]["fwd"]["half"]
        assert R["Cout 2 smallcout"]["fwd"]["kernel"] == R["Cout 1 smallcout"]["fwd"]["kernel"] == "smallcout"
        assert not R["Cout 2 smallcout"]["bwd_data"]["half"], "an fp32 forward on conv_smallcout_kernel keeps the backward in fp32"
        assert not R["fwd fp32, dX 16-bit"]["fwd"]["half"] and R["fwd fp32, dX 16-bit"]["bwd_data"]["half"]
        assert [G[lab]["groups"] for lab in ("25 taps", "49 taps", "27 taps, ragged chunk")] == [3, 6, 3] and G["125 taps"] is None
    for seed in plan.IO16_SEEDS:
        f = plan.fixed_io16(random.Random(seed))
        assert plan.cases("io16", seed)[:len(f)] == list(f.values())
        R = {lab: plan.route_io16(c) for lab, c in f.items()}
        G = {lab: half_geom(c.B, c.D, c.H, c.W, c.Cin, c.Cout, c.k, c.pad, c.epad) for lab, c in f.items()}
        hid = lambda lab: R[lab]["hid"]
        assert G["natural persistent, 512 units"]["units"] == 512 and hid("natural persistent, 512 units") == 4 and f["natural persistent, 512 units"].wgs == 256
        assert G["natural, 504 units: refused"]["units"] == 504 and hid("natural, 504 units: refused") == 0
        for lab, units, want in (("persistent wgs 3, 5 units: refused", 5, 0), ("persistent wgs 3, 6 units", 6, 5),
                                 ("persistent wgs 5, 9 units: refused", 9, 0), ("persistent wgs 5, 10 units", 10, 3)):
            assert G[lab]["units"] == units and hid(lab) == want, (lab, G[lab], R[lab])
        # four waves: halo 384 voxels, LDS 79 KiB
        assert G["four waves, halo 324"]["HV"] == 324 and hid("four waves, halo 324") == 5
        assert G["four waves, 3x1x1 causal"]["HV"] <= 384 and hid("four waves, 3x1x1 causal") == 5
        assert hid("four waves, fp32 pointwise rows") == 5 and hid("eight waves, fp32 3x1x1") == 3
        # (the 79 KiB rule cannot decide on its own: a one-group launch of 384 halo voxels needs 384 x 80 + 9 x 64 x 80 + 2560 = 79360 bytes)
        assert G["eight waves, halo 396"]["HV"] == 396 and hid("eight waves, halo 396") == 3 and lds_bytes(384, 9, 1, 1) == 79360 <= 79 * 1024
        # NS = 2 with an odd chunk count
        assert [G[lab]["chunks"] for lab in ("NS 2, Cin 96", "NS 2, Cin 160", "NS 2, Cin 40 (ragged second chunk)")] == [3, 5, 2]
        assert hid("NS 2, Cin 96") == hid("NS 2, Cin 160") == hid("NS 2, Cin 40 (ragged second chunk)") == 4
        # GEMM
        assert G["gemm temporal rows 2048"]["rows"] == 2048 and hid("gemm temporal rows 2048") == 7
        assert G["gemm temporal rows 2040: one-unit kernel refuses 16-bit x"]["rows"] == 2040 and hid("gemm temporal rows 2040: one-unit kernel refuses 16-bit x") == 0
        assert hid("gemm temporal Cin 96 Cout 160") == 7 and hid("gemm temporal, fp32 rows stay on the one-unit kernel") == 1 and hid("gemm pointwise via io") == 6
        # f9h_plan
        assert hid("f9h Cin 48: not taken") == 0 and hid("f9h Cout 12: not taken") == 0 and hid("f9h mode 0") == 0
        assert hid("f9h mode 1, 1x4x8x8 32->8") == 8 and hid("f9h mode 2, mostly padding") == 8
        assert hid("f9h mode 1, 1536 tiles of one voxel") == 8 and plan.voxels(f["f9h mode 1, 1536 tiles of one voxel"]) == 1536
        assert hid("f9h mode 1, mostly padding: refused") == 0 and plan.f9h_variant(f["f9h mode 1, mostly padding: refused"], 1) == -1
        assert hid("f9h 16-bit y with a residual: refused") == 0
        for v in range(1, 6):
            assert (hid("f9h v%d" % v), R["f9h v%d" % v]["variant"]) == (8, v), (v, R["f9h v%d" % v])
        for lab in f:
            if lab.endswith(": refused"):
                assert not R[lab]["ok"], lab
            elif f[lab].op == "wgrad":
                assert R[lab]["ok"], lab
        for k in (K333, K133, K311):
            assert R["wgrad %dx%dx%d x16 dY16 ksplit 1" % k]["ksplit"] == 1 and R["wgrad %dx%dx%d x16 dY16 ksplit > 1" % k]["ksplit"] > 1
        c = f["wgrad several tiles per slice"]
        assert plan.wgradh_tiles(c) > R["wgrad several tiles per slice"]["ksplit"]


def test_caps_and_budgets():
    """float64 F.conv3d + autograd on 16 threads takes 0.12-0.14 s per 1e9 multiply-adds (tests/test_gpu_conv_fuzz.py): 5e10 are about 7 s."""
    assert (plan.MAX_VOXELS, plan.MAX_RED, plan.MAX_MACS_SEED, plan.MAX_STATS_WORK) == (65536, 10368, 5e10, 2.4e7)
    for family, seeds in (("ops16", plan.OPS16_SEEDS), ("io16", plan.IO16_SEEDS)):
        for seed in seeds:
            cases = plan.cases(family, seed)
            for c in cases:
                assert min(plan.out_extent(c)) >= 1 and min(c.B, c.Cin, c.Cout) >= 1
                assert plan.voxels(c) <= plan.MAX_VOXELS and plan.macs(c) <= plan.MAX_MACS_CASE, c
                assert max(c.Cin, c.Cout) * plan.taps(c) <= plan.MAX_RED, c          # |y| <= 6 * 10368 + 4 < 65504, |dX| <= 4 * 10368
                assert (c.pad[0], c.epad) in ((0, (0, 0, 0)), (c.k[0] // 2, (0, 0, 0)), (c.k[0] - 1, (1 - c.k[0], 0, 0))), c
                if family == "io16":
                    assert c.f9mode in (0, 1, 2) and c.wgs in (1, 2, 3, 5, 256) and c.op in ("fwd", "wgrad")
                    Do, Ho, Wo = plan.out_extent(c)
                    assert not c.stats or c.Cin * plan.taps(c) * Do * Ho * Wo <= plan.MAX_STATS_WORK, c
                else:
                    assert c.prec in ("fp16", "bf16", "fp16s") and c.grads in ("xw", "x", "w")
            assert sum(plan.ref_macs(c) for c in cases) <= plan.MAX_MACS_SEED, (family, seed)


def test_plan_is_reproducible():
    for family, seeds in (("ops16", plan.OPS16_SEEDS), ("io16", plan.IO16_SEEDS)):
        assert plan.cases(family, seeds[0]) == plan.cases(family, seeds[0])
        assert plan.cases(family, seeds[0]) != plan.cases(family, seeds[1])


def test_the_router_follows_the_library_on_known_shapes():
    """Shapes whose kernels tests/test_gpu_lowprec.py and tests/test_gpu_conv_f9h.py name."""
    # test_pointwise_conv_with_many_output_channels_as_a_gemm: conv_pw_h_kernel behind diqt_conv3d_fwd_h
    r = plan.route_ops16(plan.o16(1, (1, 1, 4096), 256, 512, K111, prec="bf16"))
    assert r["fwd"]["hid"] == 6 and r["bwd_data"]["hid"] == 6 and not r["wgrad"]["half"]
    # test_conv_half_is_bit_exact_on_integer_data: the one-unit kernel by default, the persistent walk with 1 and 3 workgroups
    c = plan.i16(2, (8, 8, 8), 32, 64, K333, xh=0, yh=0, res=True, f9mode=1, wgs=256)
    assert plan.route_io16(c)["hid"] == 1
    c = plan.i16(2, (6, 12, 12), 64, 32, K133, xh=0, yh=0, res=True, f9mode=1, wgs=3)
    assert plan.route_io16(c)["hid"] == 3
    # test_temporal_conv_as_a_gemm_over_shifted_rows
    assert plan.route_io16(plan.i16(2, (5, 16, 16), 64, 64, K311, causal=True, xh=1, yh=0))["hid"] == 7
    # test_weight_gradient_on_the_16_bit_mfma; test_bf16_training_backward_data_on_the_bf16_kernel
    r = plan.route_ops16(plan.o16(8, (32, 32, 32), 64, 64, K333, prec="bf16"))
    assert r["wgrad"]["half"] and r["bwd_data"]["half"] and r["fwd"]["hid"] == 1      # three tap groups: never the persistent walk
    r = plan.route_ops16(plan.o16(1, (9, 6, 7), 40, 24, K311, causal=True, prec="bf16"))
    assert r["bwd_data"]["half"] and not r["wgrad"]["half"]
    # test_backward_under_autocast_uses_fp32_gradients / test_fp16_training_with_the_loss_scaler
    assert not plan.route_ops16(plan.o16(2, (8, 8, 8), 32, 64, K333, prec="fp16"))["bwd_data"]["half"]
    assert plan.route_ops16(plan.o16(2, (8, 8, 8), 32, 64, K333, prec="fp16s"))["bwd_data"]["half"]
    # test_conv_f9h_equals_the_persistent_16_bit_kernel_bit_for_bit_on_random_data: mode 2 | mode 0 with 3 workgroups
    assert plan.route_io16(plan.i16(2, (6, 24, 40), 96, 72, K133, xh=1, yh=1, f9mode=2, wgs=3))["hid"] == 8
    assert plan.route_io16(plan.i16(2, (6, 24, 40), 96, 72, K133, xh=1, yh=1, f9mode=0, wgs=3))["hid"] in (3, 5)
    # test_conv_f9h_random_data_within_one_ulp_of_the_operand_type: the default mode takes the C2 U-Net's dominant conv
    assert plan.route_io16(plan.i16(8, (32, 32, 32), 64, 64, K333, xh=1, yh=0))["hid"] == 8
