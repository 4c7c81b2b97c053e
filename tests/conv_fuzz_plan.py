"""Case generator and router of the conv3d dispatch fuzz (tests/conv_fuzz_worker.py runs the cases on the GPU, tests/test_conv_fuzz_plan.py
proves on the CPU which kernels they reach).  Needs no GPU: ``route`` asks only the library's shape queries.

A case is ``(B, D, H, W, Cin, Cout, k, pad, epad, residual, grads)``; ``grads`` is "xw" (x, weight and bias require grad), "x" or "w":
the three ways through ``_Conv3dFn.backward``.  Families:

* ``f9small``: small random shapes for conv_fwd9_kernel, run under DIQT_CONV_F9=2 (its tile-count rules off).
* ``default``: run with no DIQT_* variable set.  Every seed holds the ``fixed_cases`` (shapes constructed so that a planner's count falls
  on or next to its threshold, and shapes for the routes a random draw rarely meets) followed by random draws over the filters, channel
  counts and extents of the models.

Caps (see tests/test_conv_fuzz_plan.py): at most 65536 output voxels and Cin*T, Cout*T <= 10368 per case (where the suite's 2e-5 / 5e-5
bounds are known to hold), at most 8e9 multiply-adds per case and 1.5e11 per seed (the float64 reference).
"""
import random

from diffusioniqt_amd import _lib, ops

MAX_VOXELS = 65536
MAX_RED = 10368
MAX_MACS_CASE = 8e9
MAX_MACS_SEED = 1.5e11
DEFAULT_SEEDS = (11, 12, 13)      # the seeds tests/test_gpu_conv_fuzz.py runs the default family with
F9SMALL_SEEDS = (1, 2)

# ---- launch tags (check_launch names in csrc/) the worker counts; FOREIGN ones belong to launches this fuzz must never see ----
FWD_TAGS = ("conv3d_fwd", "conv3d_fwd(small Cin)", "conv3d_fwd(split-K)", "conv3d_fwd(split-K reduce)", "conv3d_fwd(v9)",
            "conv3d_fwd(v9 split-K reduce)", "conv3d_fwd(8 waves)", "conv3d_fwd(1x1x1)", "conv3d_fwd(1x1x1, K = 64)", "conv3d_fwd_smallcout")
WG_TAGS = ("conv3d_bwd_weight", "conv3d_bwd_weight(v2)", "conv3d_bwd_weight(v3)", "conv3d_bwd_weight(im2col)",
           "conv3d_bwd_weight(small Cin reduce)", "conv3d_bwd_weight(1x1x1 reduce)", "conv_reduce_dw", "conv_reduce_dw3", "colsum_stage1",
           "colsum_stage2", "weighted_colsum")
FOREIGN_TAGS = ("conv3d_fwd_gn(split-K reduce)", "conv3d_fwd_h(gemm)", "conv3d_fwd_h(persistent)", "conv3d_fwd_h", "conv3d_fwd_h(v9h)",
                "conv3d_bwd_weight_h", "conv_reduce_dw3(h)")


def out_extent(case):
    B, D, H, W, Cin, Cout, k, pad, epad, res, grads = case
    return tuple(n + 2 * p + e - kk + 1 for n, p, e, kk in zip((D, H, W), pad, epad, k))


def voxels(case):
    Do, Ho, Wo = out_extent(case)
    return case[0] * Do * Ho * Wo


def macs(case):
    k = case[6]
    return voxels(case) * case[4] * case[5] * k[0] * k[1] * k[2]


def want_stats(case):
    """The worker asks for the epilogue's column sums except where that would keep the call off conv_smallcout_kernel (ops.conv3d takes
    it only without them, as the models' final convs do)."""
    return case[5] > 2


def _geo(case):
    B, D, H, W, Cin, Cout, k, pad, epad, res, grads = case
    return (B, D, H, W, Cin, Cout, *k, *pad, *epad)


def _fwd_route(geo, npk, has_stats=False):
    """The launch of _conv_fwd_raw's diqt_conv3d_fwd_pk call with a packed buffer of npk floats, the workspace the query asks for and
    (has_stats) a wish for statistics: the library's own decision, diqt_conv3d_fwd_route."""
    kid, ksplit, variant, rows = (_lib.query("diqt_conv3d_fwd_route", *geo, npk, 1, int(has_stats), 0, 0, field) for field in range(4))
    return {"kernel": "id%d" % kid, "kid": kid, "variant": variant, "split": ksplit > 1, "stats_blocks": rows}


def route(case):
    """The kernels ops.conv3d / _Conv3dFn dispatch a case to: {"fwd": ..., "bwd_data": ... or None, "wgrad": ... or None}."""
    B, D, H, W, Cin, Cout, k, pad, epad, res, grads = case
    geo = _geo(case)
    q = _lib.query
    assert q("diqt_conv3d_lds_bytes", D, H, W, *k, *pad, *epad) <= 160 * 1024, "conv3d_direct is out of scope"
    if Cout <= 2 and not want_stats(case) and q("diqt_conv3d_fwd_smallcout_supported", *geo):
        fwd = {"kernel": "smallcout", "kid": None, "variant": -1, "split": False, "stats_blocks": 0}
    else:
        npk = sum(ops._packed_len((Cout, Cin, *k), 0))                           # direct pack + Winograd panels
        fwd, plain = _fwd_route(geo, npk, want_stats(case)), _fwd_route(geo, npk)
        if plain["kid"] == 4 and plain["split"] and fwd["kid"] == 0 and not fwd["split"]:
            # the launch without statistics is conv_fwd9_kernel in its split-K form; granted statistics, it runs un-split conv_fwd_kernel
            fwd["stats_fallback"] = True
    bwd = wg = None
    Do, Ho, Wo = out_extent(case)
    if "x" in grads:
        bgeo = (B, Do, Ho, Wo, Cout, Cin, *k, *(kk - 1 - p for kk, p in zip(k, pad)), *(-e for e in epad))
        bwd = _fwd_route(bgeo, ops._packed_len((Cout, Cin, *k), 1)[0])            # direct pack only: never the Winograd tile
    if "w" in grads:
        wg = wgrad_route(case)
    return {"fwd": fwd, "bwd_data": bwd, "wgrad": wg}


def wgrad_route(case):
    """The path diqt_conv3d_bwd_weight (fp32) takes for a case (aligned tensors, as torch allocates them): the library's own decision,
    diqt_conv3d_bwd_weight_route."""
    kid, path = (_lib.query("diqt_conv3d_bwd_weight_route", *_geo(case), 1, 1, field) for field in (0, 1))
    assert path >= 0, (case, "the launch refuses")
    return {"kid": kid, "kind": ("colsum", "im2col", "pw", "v3", "v2", "v1")[path]}


def fwd_tags(r):
    """Launch tags a forward-type pass planned as ``r`` shows in the census.  id 2 is conv1x1_fwd_kernel or its K = 64 sibling: no query
    tells them apart, either tag is accepted (returned as a tuple of alternatives)."""
    if r["kernel"] == "smallcout":
        return ({"conv3d_fwd_smallcout": 1},)
    kid = r["kid"]
    if kid == 1:
        return ({"conv3d_fwd(small Cin)": 1},)
    if kid == 4:
        return ({"conv3d_fwd(v9)": 1, "conv3d_fwd(v9 split-K reduce)": 1},) if r["split"] else ({"conv3d_fwd(v9)": 1},)
    if kid == 3:
        return ({"conv3d_fwd(8 waves)": 1},)
    if kid == 2:
        return ({"conv3d_fwd(1x1x1)": 1}, {"conv3d_fwd(1x1x1, K = 64)": 1})
    assert kid == 0, r
    return ({"conv3d_fwd(split-K)": 1, "conv3d_fwd(split-K reduce)": 1},) if r["split"] else ({"conv3d_fwd": 1},)


def wgrad_tags(w):
    """Launch tags of the weight + bias gradient (the bias gradient rides on the v2 / v3 kernels, else it is the two-stage column sum)."""
    cs = {"colsum_stage1": 1, "colsum_stage2": 1}
    return {"v3": {"conv3d_bwd_weight(v3)": 1, "conv_reduce_dw3": 1},
            "v2": {"conv3d_bwd_weight(v2)": 1, "conv_reduce_dw": 1},
            "v1": {"conv3d_bwd_weight": 1, "conv_reduce_dw": 1, **cs},
            "im2col": {"conv3d_bwd_weight(im2col)": 1, "conv3d_bwd_weight(small Cin reduce)": 1, **cs},
            "pw": {"conv3d_bwd_weight(1x1x1 reduce)": 1, **cs},
            "colsum": {"weighted_colsum": 1, **cs}}[w["kind"]]


def describe(r):
    """One word per pass, for the worker's lines and the coverage table."""
    def f(p):
        if p is None:
            return "-"
        if p["kernel"] == "smallcout":
            return "smallcout"
        s = p["kernel"] + ("v%d" % p["variant"] if p["kid"] == 4 else "")
        return s + ("+splitK" if p["split"] else "")
    return "fwd=%s bwd=%s wg=%s" % (f(r["fwd"]), f(r["bwd_data"]), r["wgrad"]["kind"] if r["wgrad"] else "-")


# ---------------------------------------------------------------------------------------------------------------------------------
def _f9small(seed):
    rnd = random.Random(seed)
    out = []
    for _ in range(36):
        k = rnd.choice([(3, 3, 3), (1, 3, 3), (3, 1, 1)])
        B = rnd.randint(1, 3)
        D, H, W = (rnd.randint(1, 19) for _ in range(3))
        Cin = 16 * rnd.randint(1, 5)
        Cout = rnd.choice([8, 16, 40, 64, 72, 130])
        causal = k == (3, 1, 1) and rnd.random() < 0.5
        if causal:
            pads, epad = (2, 0, 0), (-2, 0, 0)
        else:
            p = rnd.choice([0, 1])
            pads, epad = tuple(p * (kk // 2) for kk in k), (0, 0, 0)
        Do, Ho, Wo = (n + 2 * p + e - kk + 1 for n, p, e, kk in zip((D, H, W), pads, epad, k))
        if min(Do, Ho, Wo) < 1:
            continue
        use_res = rnd.random() < 0.5
        out.append((B, D, H, W, Cin, Cout, k, pads, epad, use_res, "xw"))
    return out


def _same(k):
    return tuple(kk // 2 for kk in k)


def _case(B, sp, Cin, Cout, k, pad=None, causal=False, res=False, grads="xw"):
    pad = _same(k) if pad is None else pad
    epad = (0, 0, 0)
    if causal:
        pad, epad = (k[0] - 1, pad[1], pad[2]), (-(k[0] - 1), 0, 0)
    return (B, *sp, Cin, Cout, tuple(k), tuple(pad), epad, res, grads)


K333, K133, K311, K111 = (3, 3, 3), (1, 3, 3), (3, 1, 1), (1, 1, 1)


def fixed_cases(rnd):
    """{label: case}: the constructed shapes of a seed.  The free choices (which multiple of 16, which Cout inside a 64-channel block
    count, residual, which gradients) are drawn from ``rnd``; what puts the case on its target is fixed.  The labels name the target
    tests/test_conv_fuzz_plan.py holds the case to."""
    res = lambda: rnd.random() < 0.5
    gr = lambda: rnd.choice(["xw", "xw", "x", "w"])
    c16 = lambda: 16 * rnd.randint(1, 3)
    co2 = lambda: rnd.choice([68, 72, 96, 128])          # two 64-channel blocks
    f = {}
    # ---- conv_fwd9_kernel, un-split: 241..256 workgroups = tiles x 64-channel blocks (f9_try), inside the 65536-voxel cap ----
    f["f9 v7 unsplit, 244 workgroups"] = _case(61, (8, 8, 16), c16(), rnd.choice([16, 40, 64]), K333, res=res(), grads=gr())
    f["f9 v0 unsplit (odd width: no Winograd), 244"] = _case(61, (8, 8, 15), 16, co2(), K333, res=res(), grads=gr())
    f["f9 v1 unsplit, 244"] = _case(61, (4, 8, 15), c16(), co2(), K333, res=res(), grads=gr())
    f["f9 v2 unsplit, 244"] = _case(2, (61, 16, 32), 16, co2(), K133, res=res(), grads=gr())
    f["f9 v3 unsplit, 244"] = _case(2, (122, 16, 16), 16, co2(), K133, res=res(), grads=gr())
    f["f9 v4 unsplit, 248"] = _case(4, (122, 8, 8), c16(), co2(), K133, res=res(), grads=gr())
    f["f9 v5 unsplit, 244"] = _case(61, (16, 8, 8), 16, co2(), K311, res=res(), grads=gr())
    f["f9 v6 unsplit, 244"] = _case(122, (4, 8, 8), c16(), co2(), K311, causal=rnd.random() < 0.5, res=res(), grads=gr())
    # backward-data on conv_fwd9_kernel: Cin takes Cout's place (two 64-channel blocks of input channels)
    f["bwd-data f9 v0 unsplit"] = _case(61, (8, 8, 16), 80, 16, K333, res=res(), grads="x")
    f["bwd-data f9 v6 unsplit, causal"] = _case(122, (4, 8, 8), 96, 16, K311, causal=True, res=res(), grads="x")
    # f9_try's thresholds: 240 | 241 ... 256 | 258, 272 (257 is prime: 257 tiles of 256 voxels do not fit 65536 voxels at 0.9 useful)
    f["f9_try 240"] = _case(120, (4, 8, 8), 16, co2(), K333, res=res(), grads="xw")
    f["f9_try 241"] = _case(241, (4, 8, 8), 16, 16, K333, res=res(), grads="xw")
    f["f9_try 256"] = _case(128, (4, 8, 8), 16, co2(), K333, res=res(), grads="xw")
    f["f9_try 258"] = _case(129, (4, 8, 8), 16, co2(), K333, res=res(), grads="xw")
    f["f9_try 272"] = _case(136, (4, 8, 8), 16, co2(), K333, res=res(), grads="xw")
    # split-K: 120 workgroups x 2 shares = 240 (refused) | 121 x 2 = 242, in the backward-data pass (32 -> 16 there; a forward launch
    # that is granted statistics does not split)
    f["f9_try split 120x2"] = _case(120, (4, 8, 8), 16, 32, K311, res=res(), grads="xw")
    f["f9_try split 121x2"] = _case(121, (4, 8, 8), 16, 32, K311, res=res(), grads="xw")
    f["f9 split refused for statistics"] = _case(121, (4, 8, 8), 32, 16, K311, res=res(), grads="w")
    f["f9 split 333 (Winograd)"] = _case(2, (16, 16, 16), 64, co2(), K333, res=res(), grads=gr())
    f["f9 split 333 (direct: odd width)"] = _case(2, (16, 16, 15), 64, co2(), K333, res=res(), grads=gr())
    f["f9 split 133"] = _case(2, (16, 16, 16), 64, co2(), K133, res=res(), grads=gr())
    f["f9 split 311"] = _case(2, (16, 16, 16), 64, co2(), K311, causal=rnd.random() < 0.5, res=res(), grads=gr())
    # ---- conv_fwd8_kernel: >= 12 taps, Cin % 4 == 0 but not % 16: 255 | 256 workgroups of 256 voxels ----
    f["fwd8 255"] = _case(5, (4, 8, 136), 20, 136, K333, res=res(), grads="xw")
    f["fwd8 256"] = _case(2, (16, 32, 32), 20, co2(), K333, res=res(), grads="xw")
    f["fwd8 256, 1x5x5"] = _case(4, (16, 32, 32), 8, 24, (1, 5, 5), res=res(), grads="w")
    f["bwd-data fwd8"] = _case(2, (16, 32, 32), 72, 20, K333, res=res(), grads="x")
    # ---- conv_fwd_kernel's split-K (fwd_ksplit): 383 | 384 workgroups of 128 voxels, two 32-channel chunks ----
    # (its share count is 512 / workgroups, so the 384 in its first line never decides: the launch splits up to 256 workgroups)
    for n in (256, 257, 383, 384):
        f["fwd_ksplit %d" % n] = _case(n, (1, 8, 16), 40, 8, K133, res=res(), grads="xw")
    # ---- conv1x1_fwd_kernel (id 2): one 32-channel chunk, or more than 256 workgroups ----
    f["fwd id2, one chunk"] = _case(2, (8, 9, 12), rnd.choice([8, 24, 32]), rnd.choice([40, 72]), K111, res=res(), grads=gr())
    f["fwd id2, two chunks"] = _case(5, (16, 16, 32), 64, 136, K111, res=res(), grads="w")
    f["bwd-data id2"] = _case(3, (7, 9, 12), 72, rnd.choice([8, 24, 32]), K111, res=res(), grads="x")
    # ---- weight gradient ----
    for cin in (12, 16, 20):
        f["wgrad3_plan Cin %d" % cin] = _case(2, (8, 10, 12), cin, 24, K333, res=res(), grads="w")
    f["wgrad3 333, several tiles per workgroup"] = _case(1, (16, 32, 36), 32, 32, K333, res=res(), grads="w")
    f["wgrad3 311 causal, several tiles"] = _case(2, (40, 16, 18), 32, 48, K311, causal=True, res=res(), grads="xw")
    f["wgrad3 111"] = _case(2, (8, 8, 12), 48, 136, K111, res=res(), grads="xw")
    f["wgrad v2, 3 taps"] = _case(2, (9, 6, 7), 33, 7, K311, causal=rnd.random() < 0.5, res=res(), grads="xw")
    f["wgrad v2, 9 taps"] = _case(2, (5, 12, 11), rnd.choice([8, 12, 18]), 40, K133, res=res(), grads="xw")
    f["wgrad v2, 27 taps"] = _case(1, (7, 9, 10), 20, 22, K333, res=res(), grads="xw")
    f["wgrad v2, 49 taps"] = _case(2, (6, 8, 8), 8, 40, (1, 7, 7), res=res(), grads="xw")
    f["wgrad v1 (5x5x5)"] = _case(1, (6, 12, 12), 20, 24, (5, 5, 5), res=res(), grads="xw")
    for V, sp in ((4032, (7, 18, 16)), (4096, (8, 16, 16)), (4160, (5, 26, 16))):
        f["pw_plan V %d" % V] = _case(2, sp, 62, 68, K111, res=res(), grads="xw")
        f["sc_plan V %d" % V] = _case(2, sp, rnd.randint(1, 4), 20, K333, res=res(), grads="xw")
    f["pw_plan M 64"] = _case(2, (8, 16, 16), 62, 64, K111, res=res(), grads="xw")
    f["pw_plan M 68, dY first"] = _case(2, (8, 16, 16), 30, 68, K111, res=res(), grads="w")
    f["colsum Cout 1"] = _case(rnd.randint(1, 3), (9, 10, 11), rnd.choice([8, 30, 64]), 1, K111, res=res(), grads="xw")
    # ---- conv_smallcout_kernel ----
    for k, co in ((K111, 1), (K133, 1), (K333, 1), (K311, 1), (K111, 2), (K133, 2)):
        f["smallcout %dx%dx%d Cout %d" % (*k, co)] = _case(rnd.randint(1, 2), (rnd.randint(4, 10), rnd.randint(7, 18), rnd.randint(7, 18)),
                                                          rnd.choice([16, 24, 33, 64]), co, k, causal=k == K311 and rnd.random() < 0.5,
                                                          res=res(), grads=gr())
    # ---- the 1x15x15 cross-embed of Family B (Cin <= 4) ----
    f["1x15x15"] = _case(1, (3, 16, 16), rnd.randint(1, 4), 16, (1, 15, 15), res=res(), grads="xw")
    return f


_FILTERS = [K333, K333, K133, K133, K311, K311, K111, K111, (1, 7, 7), (1, 5, 5), (5, 5, 5)]


def _random_case(rnd):
    k = rnd.choice(_FILTERS)
    T = k[0] * k[1] * k[2]
    kind = rnd.choice(["m16", "m16", "m4", "odd", "tiny", "co12"])
    Cin = {"m16": 16 * rnd.randint(1, 6), "m4": rnd.choice([4, 8, 12, 20, 24, 36, 40, 72]), "odd": rnd.choice([5, 7, 17, 33, 50]),
           "tiny": rnd.randint(1, 4), "co12": rnd.choice([16, 20, 32, 64])}[kind]
    Cout = rnd.choice([1, 2]) if kind == "co12" else rnd.choice([4, 7, 8, 16, 20, 24, 40, 64, 72, 130, 136])
    if T > 27:
        Cin, Cout = min(Cin, 24), min(Cout, 24)
    B = rnd.randint(1, 3)
    D, H, W = rnd.randint(1, 12), rnd.randint(1, 20), rnd.randint(1, 20)
    causal = k == K311 and rnd.random() < 0.5
    pad = _same(k) if (causal or rnd.random() < 0.7) else (0, 0, 0)
    return _case(B, (D, H, W), Cin, Cout, k, pad=pad, causal=causal, res=rnd.random() < 0.5, grads=rnd.choice(["xw", "xw", "x", "w"]))


def _random_big_case(rnd):
    """20000..65536 output voxels on the filters and channel counts conv_fwd9_kernel / conv_fwd8_kernel take: launches of 80..500
    workgroups, where the tile-count rules of f9_try, fwd8_plan and fwd_ksplit decide"""
    k = rnd.choice([K333, K133, K311])
    Cin = rnd.choice([16, 32, 48, 64, 20, 40])
    Cout = rnd.choice([16, 32, 64, 72, 96, 128, 136])
    B = rnd.randint(1, 64)
    D, H, W = rnd.choice([1, 2, 4, 6, 8, 12, 16]), rnd.choice([8, 12, 15, 16, 24, 32]), rnd.choice([8, 12, 15, 16, 24, 32])
    causal = k == K311 and rnd.random() < 0.5
    return _case(B, (D, H, W), Cin, Cout, k, causal=causal, res=rnd.random() < 0.5, grads=rnd.choice(["xw", "xw", "x", "w"]))


def _default(seed, n_random=60, n_big=12):
    rnd = random.Random(seed)
    out = list(fixed_cases(rnd).values())
    while n_big > 0:
        c = _random_big_case(rnd)
        if min(out_extent(c)) < 1 or not 20000 <= voxels(c) <= MAX_VOXELS or macs(c) > MAX_MACS_CASE / 2:
            continue
        out.append(c)
        n_big -= 1
    while n_random > 0:
        c = _random_case(rnd)
        if min(out_extent(c)) < 1 or voxels(c) > MAX_VOXELS or macs(c) > MAX_MACS_CASE:
            continue
        out.append(c)
        n_random -= 1
    return out


def cases(family, seed):
    return {"f9small": _f9small, "default": _default}[family](seed)
