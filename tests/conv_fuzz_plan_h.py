"""Case generator and router of the 16-bit conv dispatch fuzz, the sibling of tests/conv_fuzz_plan.py (tests/conv_fuzz_worker_h.py runs the
cases on the GPU, tests/test_conv_fuzz_plan_h.py proves on the CPU which kernels they reach).  Needs no GPU: the routers ask only the
library's shape queries.

Families:

* ``ops16``: ``ops.conv3d`` with autograd under ``ops.low_precision``.  A case is the tuple of the fp32 fuzz plus ``prec`` ("fp16", "bf16",
  or "fp16s": fp16 with ``ops.FP16_BACKWARD = True``, as under the trainer's loss scaler) and ``bias`` (present or None).
  ``route_ops16`` restates ``_Conv3dFn``: forward = conv_smallcout, else the 16-bit kernel where diqt_conv3d_fwd_h_supported, else fp32;
  dX on the 16-bit kernel (mode-1 packing) iff ``_lp_backward`` gives a type and the transformed geometry is supported; dW on
  conv3d_bwd_weight_h iff its workspace query is positive.
* ``io16``: ``diqt_conv3d_fwd_h_io`` called directly (op "fwd") with 16-bit x / y, residual, statistics and the test switches
  diqt_set_conv_f9h_mode / diqt_set_convh_workgroups, and ``diqt_conv3d_bwd_weight_h`` (op "wgrad": ``xh`` / ``yh`` are its flag bits 2 / 4,
  16-bit x / dY).  About a third of its cases are refusals: diqt_conv3d_fwd_h_kernel_id answers 0 (the weight-gradient plan refuses): the
  call must return an error and leave the output untouched.

All data are small integers (x in [-3, 3], w in [-2, 2], bias in [-4, 4], dY in [-2, 2], residual in [-5, 5]): exact in fp16 and bf16,
every partial sum exact in fp32, so the worker compares with ``torch.equal``.  Caps: those of the fp32 fuzz (65536 output voxels, Cin*T and
Cout*T <= 10368, so |y| <= 6 * 10368 + 4 = 62212 < 65504 = fp16's largest, and every sum < 2^24); at most 5e10 multiply-adds of float64
reference per seed.  Statistics cases draw x, w, bias from {-1, 0, 1} and keep Cin*T x voxels per batch entry <= 2.4e7, so that the sum
of y^2 over a batch entry stays below 2^24 (the worker checks that bound on the reference itself).
"""
import collections
import contextlib
import random

from diffusioniqt_amd import _lib, ops
from tests import conv_fuzz_plan as base

MAX_VOXELS, MAX_RED = base.MAX_VOXELS, base.MAX_RED
MAX_MACS_CASE = 6e9
MAX_MACS_SEED = 5e10
MAX_STATS_WORK = 2.4e7            # Cin * T * output voxels per batch entry of a statistics case
OPS16_SEEDS = (21, 22, 23)        # the seeds tests/test_gpu_conv_fuzz_h.py runs
IO16_SEEDS = (31, 32, 33)

Ops16 = collections.namedtuple("Ops16", "B D H W Cin Cout k pad epad res grads prec bias")
Io16 = collections.namedtuple("Io16", "B D H W Cin Cout k pad epad res op xh yh stats bf16 f9mode wgs")

K333, K133, K311, K111 = base.K333, base.K133, base.K311, base.K111
K155, K177, K555 = (1, 5, 5), (1, 7, 7), (5, 5, 5)
LP = {"fp16": 0, "bf16": 1, "fp16s": 0}
LP_BACKWARD = {"fp16": None, "bf16": 1, "fp16s": 0}      # ops._lp_backward: bf16 follows the forward, fp16 only under a loss scaler

# diqt_conv3d_fwd_h_kernel_id
HID_NAMES = {0: "unsupported", 1: "conv_fwd_h_kernel, prefetch", 2: "conv_fwd_h_kernel, no prefetch", 3: "conv_fwd_hp_kernel, 8 waves",
             4: "conv_fwd_hp_kernel, 8 waves, two-chunk pointwise", 5: "conv_fwd_hp_kernel, 4 waves", 6: "conv_pw_h_kernel, pointwise",
             7: "conv_pw_h_kernel, temporal", 8: "conv_f9h_kernel"}
HID_TAG = {1: "conv3d_fwd_h", 2: "conv3d_fwd_h", 3: "conv3d_fwd_h(persistent)", 4: "conv3d_fwd_h(persistent)", 5: "conv3d_fwd_h(persistent)",
           6: "conv3d_fwd_h(gemm)", 7: "conv3d_fwd_h(gemm)", 8: "conv3d_fwd_h(v9h)"}
H_FWD_TAGS = ("conv3d_fwd_h", "conv3d_fwd_h(persistent)", "conv3d_fwd_h(gemm)", "conv3d_fwd_h(v9h)")
H_WG_TAGS = ("conv3d_bwd_weight_h", "conv_reduce_dw3(h)")
# conv_f9h_kernel's tilings (conv_f9h_kernel.h: H9_333_512, H9_333_256, H9_133_A .. D): variant -> (tile, workgroups per CU)
F9H_CFG = {0: ((8, 8, 8), 1), 1: ((4, 8, 8), 2), 2: ((1, 16, 32), 1), 3: ((2, 16, 16), 1), 4: ((4, 8, 8), 1), 5: ((1, 8, 32), 2)}
# half_geom's candidate tiles (conv_half.hip), all of 256 voxels
HALF_TILES = [(4, 8, 8), (8, 8, 4), (8, 4, 8), (2, 8, 16), (2, 16, 8), (1, 16, 16), (16, 4, 4), (4, 4, 16), (4, 16, 4), (16, 16, 1), (16, 1, 16),
              (32, 4, 2), (64, 2, 2), (256, 1, 1), (1, 1, 256), (1, 256, 1), (1, 8, 32), (1, 32, 8), (8, 32, 1), (32, 8, 1), (1, 4, 64), (1, 2, 128),
              (128, 2, 1), (128, 1, 2)]
WH_TILE = (2, 4, 16)              # conv_wgrad_h_kernel's 128-voxel tile (conv_wgrad_h.hip: WTD, WTH, WTW)


def cdiv(a, b):
    return -(-a // b)


def geo_of(c):
    return (c.B, c.D, c.H, c.W, c.Cin, c.Cout, *c.k, *c.pad, *c.epad)


def out_extent(c):
    return tuple(n + 2 * p + e - kk + 1 for n, p, e, kk in zip((c.D, c.H, c.W), c.pad, c.epad, c.k))


def taps(c):
    return c.k[0] * c.k[1] * c.k[2]


def voxels(c):
    Do, Ho, Wo = out_extent(c)
    return c.B * Do * Ho * Wo


def macs(c):
    return voxels(c) * c.Cin * c.Cout * taps(c)


def ref_macs(c):
    """multiply-adds of the float64 reference: the conv, and one more conv-sized pass per gradient"""
    if isinstance(c, Io16):
        return macs(c)
    return macs(c) * (1 + ("x" in c.grads) + ("w" in c.grads))


@contextlib.contextmanager
def switches(f9mode, wgs):
    """The two test switches, set through diqt_set_* (which also empties _lib.query's memo) and restored on the way out."""
    p9, pw = _lib.query("diqt_set_conv_f9h_mode", f9mode), _lib.query("diqt_set_convh_workgroups", wgs)
    try:
        yield
    finally:
        _lib.query("diqt_set_conv_f9h_mode", p9)
        _lib.query("diqt_set_convh_workgroups", pw)


def f9h_variant(c, mode):
    """f9h_plan's choice (conv_f9h.hip) restated: the candidate with the shortest estimated duration, ties to the earlier one; -1 when the
    "mostly padding" rule of mode 1 leaves the launch to the other kernels.  Only meaningful where the kernel id says conv_f9h_kernel."""
    Do, Ho, Wo = out_extent(c)
    nNt = cdiv(c.Cout, 64)
    order = [1, 0] if c.k == K333 else ([5] if c.Cin <= 64 else []) + [2, 3, 5, 4]
    best, bv = None, -1
    for v in order:
        (td, th, tw), occ = F9H_CFG[v]
        nwg = c.B * cdiv(Do, td) * cdiv(Ho, th) * cdiv(Wo, tw) * nNt
        slots = 256 * occ
        gr = nwg if nwg <= slots else slots - slots % nNt
        est = cdiv(nwg, gr) * td * th * tw * occ * (1.0 / occ if nwg <= 256 else 1.0)
        if best is None or est < best:
            best, bv = est, v
    useful = float(c.B * Do * Ho * Wo * nNt)
    if mode != 2 and best * 256.0 > 6.0 * max(useful, 256.0 * 256.0):
        return -1
    return bv


def stats_rows_bound(c):
    """No launch writes more statistics rows per batch entry: 8 per tile, over every tile shape of the 16-bit kernels."""
    Do, Ho, Wo = out_extent(c)
    return 8 * max(cdiv(Do, t[0]) * cdiv(Ho, t[1]) * cdiv(Wo, t[2]) for t in HALF_TILES + [cfg[0] for cfg in F9H_CFG.values()])


def f9h_tiles_per_entry(c, v):
    return [cdiv(o, t) for o, t in zip(out_extent(c), F9H_CFG[v][0])]


# ---------------------------------------------------------------------------------------------------------------------------------
# routers
# ---------------------------------------------------------------------------------------------------------------------------------
def _h(hid, variant=-1):
    return {"kernel": "h%d" % hid, "hid": hid, "variant": variant, "half": True}


def route_ops16(c):
    """The kernels ops.conv3d / _Conv3dFn dispatch a case to under ops.low_precision(prec), with the default switches:
    {"fwd", "bwd_data", "wgrad"}; a pass on a 16-bit kernel carries "half": True."""
    q = _lib.query
    geo = geo_of(c)
    wshape = (c.Cout, c.Cin, *c.k)
    assert q("diqt_conv3d_lds_bytes", c.D, c.H, c.W, *c.k, *c.pad, *c.epad) <= 160 * 1024, "conv3d_direct is out of scope"
    lp = LP[c.prec]
    if c.Cout <= 2 and q("diqt_conv3d_fwd_smallcout_supported", *geo):
        fwd = {"kernel": "smallcout", "kid": None, "variant": -1, "split": False, "half": False}
        lp = None                                     # _Conv3dFn.forward: an exact fp32 forward, and the backward follows it
    elif q("diqt_conv3d_fwd_h_supported", *geo):
        fwd = _h(q("diqt_conv3d_fwd_h_kernel_id", *geo, 0, 0, int(c.res), 0))
        assert fwd["hid"] in (1, 2, 3, 6), (c, fwd)  # fp32 tensors at both ends: the one-unit kernel, the 8-wave walk, or the pointwise GEMM
    else:
        fwd = dict(base._fwd_route(geo, sum(ops._packed_len(wshape, 0))), half=False)
    lpb = LP_BACKWARD[c.prec] if lp is not None else None
    bwd = wg = None
    Do, Ho, Wo = out_extent(c)
    if "x" in c.grads:
        bgeo = (c.B, Do, Ho, Wo, c.Cout, c.Cin, *c.k, *(kk - 1 - p for kk, p in zip(c.k, c.pad)), *(-e for e in c.epad))
        if lpb is not None and q("diqt_conv3d_fwd_h_supported", *bgeo):
            bwd = _h(q("diqt_conv3d_fwd_h_kernel_id", *bgeo, 0, 0, 0, 0))
        else:
            bwd = dict(base._fwd_route(bgeo, ops._packed_len(wshape, 1)[0]), half=False)
    if "w" in c.grads:
        nh = q("diqt_conv3d_bwd_weight_h_workspace_bytes", *geo) if lpb is not None else 0
        wg = {"kind": "h", "kid": None, "ksplit": wgradh_ksplit(c, nh), "half": True} if nh else dict(base.wgrad_route(tuple(c[:11])), half=False)
    return {"fwd": fwd, "bwd_data": bwd, "wgrad": wg}


def wgradh_ksplit(c, nbytes):
    """split-K slices of conv_wgrad_h_kernel, from its workspace: ksplit x (Cout Cin T + CoutPad) floats"""
    per = (c.Cout * c.Cin * taps(c) + cdiv(c.Cout, 64) * 64) * 4
    assert nbytes % per == 0, (c, nbytes)
    return nbytes // per


def wgradh_tiles(c):
    Do, Ho, Wo = out_extent(c)
    return c.B * cdiv(Do, WH_TILE[0]) * cdiv(Ho, WH_TILE[1]) * cdiv(Wo, WH_TILE[2])


def route_io16(c):
    """{"ok": the call is taken, "hid", "variant", "stats_blocks"} (op "fwd") or {"ok", "ksplit"} (op "wgrad"), under the case's switches."""
    q = _lib.query
    geo = geo_of(c)
    with switches(c.f9mode, c.wgs):
        if c.op == "wgrad":
            nh = q("diqt_conv3d_bwd_weight_h_workspace_bytes", *geo)
            # (with 16-bit tensors the plan asks more than the workspace query: a 16-bit dY needs Cout % 8 == 0 and a 16-bit x)
            ok = q("diqt_conv3d_bwd_weight_h_supported", *geo, (2 if c.xh else 0) | (4 if c.yh else 0)) == 1
            assert not ok or nh > 0, c
            return {"ok": bool(ok), "ksplit": wgradh_ksplit(c, nh) if nh else 0, "nbytes": nh}
        hid = q("diqt_conv3d_fwd_h_kernel_id", *geo, int(c.xh), int(c.yh), int(c.res), int(c.stats))
        nblk = q("diqt_conv3d_fwd_h_stats_blocks", *geo, int(c.xh), int(c.yh)) if c.stats else 0
        return {"ok": hid != 0, "hid": hid, "variant": f9h_variant(c, c.f9mode) if hid == 8 else -1, "stats_blocks": nblk,
                "io16": q("diqt_conv3d_fwd_h_io16_supported", *geo, int(c.xh), int(c.yh))}


def fwd_tags(r):
    """alternatives of {tag: count} for a forward-type pass (see conv_fuzz_plan.fwd_tags)"""
    if r.get("half"):
        return ({HID_TAG[r["hid"]]: 1},)
    return base.fwd_tags(r)


def wgrad_tags(w, bias):
    if w.get("half"):
        return {t: 1 for t in H_WG_TAGS}
    tags = base.wgrad_tags(w)
    if not bias:                  # the two-stage column sum is the bias gradient of the kernels that do not carry it
        tags = {t: n for t, n in tags.items() if not t.startswith("colsum_stage")}
    return tags


def describe_ops16(r):
    def f(p):
        if p is None:
            return "-"
        if p.get("half"):
            return "h%d" % p["hid"]
        return "smallcout" if p["kernel"] == "smallcout" else p["kernel"] + ("+splitK" if p["split"] else "")
    w = r["wgrad"]
    return "fwd=%s bwd=%s wg=%s" % (f(r["fwd"]), f(r["bwd_data"]), "-" if w is None else "h/ks%d" % w["ksplit"] if w.get("half") else w["kind"])


# ---------------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------------
def _same(k):
    return tuple(kk // 2 for kk in k)


def _pads(k, pad=None, causal=False):
    pad = _same(k) if pad is None else tuple(pad)
    if causal:
        return (k[0] - 1, pad[1], pad[2]), (-(k[0] - 1), 0, 0)
    return pad, (0, 0, 0)


def o16(B, sp, Cin, Cout, k, pad=None, causal=False, res=False, grads="xw", prec="bf16", bias=True):
    pad, epad = _pads(k, pad, causal)
    return Ops16(B, *sp, Cin, Cout, tuple(k), pad, epad, res, grads, prec, bias)


def i16(B, sp, Cin, Cout, k, pad=None, causal=False, res=False, op="fwd", xh=1, yh=0, stats=False, bf16=0, f9mode=1, wgs=256):
    pad, epad = _pads(k, pad, causal)
    return Io16(B, *sp, Cin, Cout, tuple(k), pad, epad, res, op, int(xh), int(yh), stats, int(bf16), f9mode, wgs)


def fixed_ops16(rnd):
    """{label: case}: constructed ops16 cases (default switches).  tests/test_conv_fuzz_plan_h.py recomputes each threshold's count."""
    pr = lambda: rnd.choice(["fp16", "bf16", "fp16s"])
    prb = lambda: rnd.choice(["bf16", "fp16s"])
    res = lambda: rnd.random() < 0.5
    bias = lambda: rnd.random() < 0.75
    f = {}
    # prefetch of the one-unit kernel: HV * 8 <= 512 * HHREG, 640 halo voxels.  3x3x3 on 4x8x8 tiles: 600; on a 2x8x16 tile: 720
    f["prefetch 600 halo voxels"] = o16(1, (4, 8, 8), 16, 24, K333, res=res(), prec=pr(), bias=bias())
    f["prefetch 720 halo voxels"] = o16(1, (2, 8, 16), 16, 24, K333, res=res(), prec=pr(), bias=bias())
    # convh_persistent_takes: units >= 2 x 256 workgroups.  (1,3,3), 1x16x16 tiles, three 64-channel blocks: 170 x 3 = 510 | 171 x 3 = 513
    f["persistent 510 units"] = o16(1, (170, 16, 16), 8, 130, K133, res=res(), grads="x", prec=pr(), bias=bias())
    f["persistent 513 units"] = o16(1, (171, 16, 16), 8, 130, K133, res=res(), grads="x", prec=pr(), bias=bias())
    f["persistent backward-data, 513 units"] = o16(1, (171, 16, 16), 136, 8, K133, res=res(), grads="x", prec=prb(), bias=bias())
    f["persistent 3x1x1 causal"] = o16(3, (16, 32, 32), 8, 136, K311, causal=True, res=res(), grads="w", prec=pr(), bias=bias())
    # pwh_takes: rows 2047 | 2048, Cin 32 | 64, Cout 24 | 32 | 64 | 72
    f["pwh rows 2047"] = o16(1, (1, 23, 89), 64, 72, K111, res=res(), prec=pr(), bias=bias())
    f["pwh rows 2048"] = o16(1, (2, 32, 32), 64, 72, K111, res=res(), prec=pr(), bias=bias())
    f["pwh Cin 32"] = o16(1, (2, 32, 32), 32, 64, K111, res=res(), prec=pr(), bias=bias())
    f["pwh Cin 64 Cout 24"] = o16(1, (2, 32, 32), 64, 24, K111, res=res(), prec=pr(), bias=bias())
    f["pwh Cin 64 Cout 32"] = o16(1, (2, 32, 32), 64, 32, K111, res=res(), prec=pr(), bias=bias())
    f["pwh Cin 64 Cout 64"] = o16(1, (2, 32, 33), 64, 64, K111, res=res(), prec=pr(), bias=bias())
    f["pwh Cin 96 Cout 72, ragged rows"] = o16(3, (3, 17, 19), 96, 72, K111, res=res(), prec=pr(), bias=bias())
    # wgradh_plan: Cin 0 | 32 (mod 32), Cout 28 | 32, ksplit 1 and > 1, more tiles than 256 / blocks
    f["wgradh Cin 40"] = o16(1, (4, 8, 16), 40, 32, K333, res=res(), grads="w", prec=prb(), bias=bias())
    f["wgradh Cout 28"] = o16(1, (4, 8, 16), 32, 28, K333, res=res(), grads="w", prec=prb(), bias=bias())
    f["wgradh Cout 32"] = o16(1, (4, 8, 16), 32, 32, K333, res=res(), grads="xw", prec=prb(), bias=bias())
    for k in (K333, K133, K311):
        cz = k == K311 and rnd.random() < 0.5
        f["wgradh %dx%dx%d ksplit 1" % k] = o16(1, (2, 4, 16), 32, rnd.choice([32, 36, 72]), k, causal=cz, res=res(), grads="w", prec=prb(), bias=bias())
        f["wgradh %dx%dx%d ksplit > 1" % k] = o16(2, (5, 9, 18), 64, rnd.choice([32, 40, 72]), k, causal=cz, res=res(), grads=rnd.choice(["w", "xw"]),
                                                  prec=prb(), bias=bias())
    f["wgradh several tiles per slice"] = o16(2, (8, 16, 32), 96, 136, K133, res=res(), grads="w", prec=prb(), bias=bias())
    f["wgradh fp16 without a scaler stays fp32"] = o16(1, (4, 8, 16), 32, 32, K333, res=res(), grads="xw", prec="fp16", bias=bias())
    # fallback to fp32: Cin % 4, Cin < 8 with taps, Cout <= 2
    f["fallback Cin 6"] = o16(2, (5, 9, 11), 6, 24, K111, res=res(), prec=pr(), bias=bias())
    f["fallback Cin 4, 3x3x3"] = o16(1, (5, 9, 11), 4, 24, K333, res=res(), prec=pr(), bias=bias())
    f["Cin 4, 1x1x1 is taken"] = o16(2, (5, 9, 11), 4, 24, K111, res=res(), prec=pr(), bias=bias())
    f["Cout 2 smallcout"] = o16(1, (6, 9, 11), 32, 2, K133, res=res(), prec=pr(), bias=bias())
    f["Cout 1 smallcout"] = o16(1, (6, 9, 11), 64, 1, K111, res=res(), prec=pr(), bias=bias())
    # forward falls back (Cin % 4) but the backward-data pass, whose input channels are Cout, runs on the 16-bit kernel
    f["fwd fp32, dX 16-bit"] = o16(2, (4, 9, 10), 6, 24, K133, res=res(), grads="x", prec=prb(), bias=bias())
    # more than one tap group
    f["25 taps"] = o16(1, (2, 9, 9), 16, 24, K155, res=res(), prec=pr(), bias=bias())
    f["49 taps"] = o16(1, (2, 9, 10), 12, 24, K177, res=res(), prec=pr(), bias=bias())
    f["125 taps"] = o16(1, (6, 7, 9), 8, 8, K555, res=res(), prec=pr(), bias=bias())
    f["27 taps, ragged chunk"] = o16(1, (9, 10, 11), 36, 72, K333, res=res(), prec=pr(), bias=bias())
    return f


_OPS_FILTERS = [K333, K333, K133, K133, K311, K311, K111, K111, K155, K177, K555]
_COUTS = [1, 2, 8, 24, 32, 40, 64, 72, 130, 136]


def _draw_geometry(rnd, cins, couts):
    k = rnd.choice(_OPS_FILTERS)
    T = k[0] * k[1] * k[2]
    Cin, Cout = rnd.choice(cins), rnd.choice(couts)
    while Cin * T > MAX_RED:
        Cin = rnd.choice(cins)
    while Cout * T > MAX_RED:
        Cout = rnd.choice(couts)
    B = rnd.randint(1, 3)
    sp = (rnd.randint(1, 20), rnd.randint(1, 20), rnd.randint(1, 20))
    causal = k == K311 and rnd.random() < 0.5
    pad = _same(k) if (causal or rnd.random() < 0.7) else (0, 0, 0)
    return B, sp, Cin, Cout, k, pad, causal


def _fits(c, budget):
    return min(out_extent(c)) >= 1 and voxels(c) <= MAX_VOXELS and macs(c) <= MAX_MACS_CASE and ref_macs(c) <= budget


def _ops16(seed, n_random=70, n_wgrad=14):
    rnd = random.Random(seed)
    out = list(fixed_ops16(rnd).values())
    budget = MAX_MACS_SEED - sum(ref_macs(c) for c in out)
    cins = [4, 8, 12, 16, 20, 24, 32, 36, 40, 64, 72, 96, 128, 160, 6, 17, 2]
    while n_random > 0:
        B, sp, Cin, Cout, k, pad, causal = _draw_geometry(rnd, cins, _COUTS)
        c = o16(B, sp, Cin, Cout, k, pad=pad, causal=causal, res=rnd.random() < 0.5, grads=rnd.choice(["xw", "xw", "x", "w"]),
                prec=rnd.choice(["fp16", "bf16", "fp16s"]), bias=rnd.random() < 0.75)
        if not _fits(c, budget / (n_random + n_wgrad)):
            continue
        out.append(c)
        budget -= ref_macs(c)
        n_random -= 1
    while n_wgrad > 0:            # conv_wgrad_h_kernel: rare among the draws above (Cin % 32 == 0, Cout >= 32, three filters, a 16-bit backward)
        k = rnd.choice([K333, K133, K311])
        causal = k == K311 and rnd.random() < 0.5
        c = o16(rnd.randint(1, 3), (rnd.randint(1, 20), rnd.randint(1, 20), rnd.randint(1, 20)), rnd.choice([32, 64, 96, 160]),
                rnd.choice([32, 36, 40, 64, 72, 130, 136]), k, pad=_same(k) if (causal or rnd.random() < 0.7) else (0, 0, 0), causal=causal,
                res=rnd.random() < 0.5, grads=rnd.choice(["xw", "w"]), prec=rnd.choice(["bf16", "fp16s"]), bias=rnd.random() < 0.75)
        if c.Cin * taps(c) > MAX_RED or c.Cout * taps(c) > MAX_RED or not _fits(c, budget / n_wgrad):
            continue
        out.append(c)
        budget -= ref_macs(c)
        n_wgrad -= 1
    return out


def fixed_io16(rnd):
    """{label: case}: constructed io16 cases."""
    bf = lambda: rnd.randint(0, 1)
    f = {}
    # a natural persistent launch (no switch): 16-bit rows of a pointwise conv, 64 tiles x 8 channel blocks = 512 units; two chunks per step
    f["natural persistent, 512 units"] = i16(1, (16, 32, 32), 64, 512, K111, xh=1, yh=rnd.randint(0, 1), bf16=bf())
    f["natural, 504 units: refused"] = i16(1, (63, 16, 16), 64, 512, K111, xh=1, yh=1, bf16=bf())
    # convh_persistent_takes against twice the workgroup count: 3 workgroups, 5 | 6 units (1x16x16 tiles of a (1,3,3) conv, one channel block)
    f["persistent wgs 3, 5 units: refused"] = i16(1, (5, 16, 16), 32, 64, K133, xh=1, yh=1, f9mode=0, wgs=3, bf16=bf())
    f["persistent wgs 3, 6 units"] = i16(1, (6, 16, 16), 32, 64, K133, xh=1, yh=1, f9mode=0, wgs=3, bf16=bf())
    f["persistent wgs 5, 9 units: refused"] = i16(1, (9, 16, 16), 32, 40, K133, xh=0, yh=1, f9mode=0, wgs=5, bf16=bf())
    f["persistent wgs 5, 10 units"] = i16(1, (10, 16, 16), 32, 40, K133, xh=0, yh=1, f9mode=0, wgs=5, bf16=bf())
    # convh_four_waves: 16-bit x, one tap group, halo <= 384 voxels and LDS <= 79 KiB.  (1,3,3) on 1x16x16: 324; (3,1,1) on 16x4x4: 288 ...
    f["four waves, halo 324"] = i16(2, (3, 16, 16), 64, 72, K133, xh=1, yh=0, stats=True, f9mode=0, wgs=2, bf16=bf())
    f["eight waves, halo 400 (1x5x5 has three groups: one-unit, refused)"] = i16(2, (3, 16, 16), 64, 72, K155, xh=1, yh=0, f9mode=0, wgs=2, bf16=bf())
    f["eight waves, halo 396"] = i16(2, (6, 4, 64), 64, 72, K133, xh=1, yh=rnd.randint(0, 1), stats=True, f9mode=0, wgs=2, bf16=bf())
    f["four waves, 3x1x1 causal"] = i16(1, (20, 9, 9), 40, 24, K311, causal=True, xh=1, yh=1, stats=True, f9mode=0, wgs=1, bf16=bf())
    f["four waves, fp32 pointwise rows"] = i16(2, (4, 9, 10), 32, 72, K111, xh=0, yh=1, f9mode=0, wgs=1, bf16=bf())
    f["eight waves, fp32 3x1x1"] = i16(2, (9, 9, 10), 32, 72, K311, xh=0, yh=1, f9mode=0, wgs=2, bf16=bf())
    # pointwise NS = 2 with an odd chunk count
    f["NS 2, Cin 96"] = i16(2, (4, 9, 10), 96, 72, K111, xh=1, yh=rnd.randint(0, 1), res=False, f9mode=0, wgs=3, bf16=bf())
    f["NS 2, Cin 160"] = i16(1, (5, 9, 10), 160, 40, K111, xh=1, yh=0, res=True, f9mode=0, wgs=1, bf16=bf())
    f["NS 2, Cin 40 (ragged second chunk)"] = i16(1, (5, 9, 10), 40, 24, K111, xh=1, yh=1, f9mode=0, wgs=1, bf16=bf())
    # GEMM: temporal with 16-bit rows (rows 2047 | 2048), pointwise with fp32 rows through the io entry point
    f["gemm temporal rows 2048"] = i16(1, (8, 16, 16), 64, 64, K311, causal=True, xh=1, yh=0, res=rnd.random() < 0.5, bf16=bf())
    f["gemm temporal rows 2040: one-unit kernel refuses 16-bit x"] = i16(1, (8, 15, 17), 64, 64, K311, causal=True, xh=1, yh=0, bf16=bf())
    f["gemm temporal Cin 96 Cout 160"] = i16(1, (8, 16, 20), 96, 160, K311, xh=1, yh=0, res=True, bf16=bf())
    f["gemm temporal, fp32 rows stay on the one-unit kernel"] = i16(1, (8, 16, 16), 64, 64, K311, xh=0, yh=0, bf16=bf())
    f["gemm pointwise via io"] = i16(1, (3, 32, 32), 64, 40, K111, xh=0, yh=0, res=True, bf16=bf())
    # f9h_plan: Cin % 32, Cout % 8, and the "mostly padding" rule of mode 1
    f["f9h Cin 48: not taken"] = i16(1, (4, 8, 8), 48, 8, K333, xh=1, yh=0, f9mode=2, wgs=1, bf16=bf())
    f["f9h Cout 12: not taken"] = i16(1, (4, 8, 8), 32, 12, K333, xh=1, yh=0, f9mode=2, wgs=1, bf16=bf())
    f["f9h mode 1, 1x4x8x8 32->8"] = i16(1, (4, 8, 8), 32, 8, K333, xh=1, yh=1, stats=True, f9mode=1, bf16=bf())
    # "mostly padding": estimate x 256 > 6 x max(useful voxels, 65536).  One output voxel per 256-voxel tile: 1536 tiles are three rounds of
    # 512 workgroup slots (3 x 512 x 256 = 6 x 65536: taken), 1537 are four (refused in mode 1, taken in mode 2)
    f["f9h mode 1, 1536 tiles of one voxel"] = i16(1536, (3, 3, 3), 32, 8, K333, pad=(0, 0, 0), xh=1, yh=1, f9mode=1, bf16=bf())
    f["f9h mode 1, mostly padding: refused"] = i16(1537, (3, 3, 3), 32, 8, K333, pad=(0, 0, 0), xh=1, yh=1, f9mode=1, bf16=bf())
    f["f9h mode 2, mostly padding"] = i16(1537, (3, 3, 3), 32, 8, K333, pad=(0, 0, 0), xh=1, yh=1, stats=True, f9mode=2, bf16=bf())
    f["f9h mode 0"] = i16(1, (4, 8, 8), 32, 8, K333, xh=1, yh=1, f9mode=0, bf16=bf())
    f["f9h 16-bit y with a residual: refused"] = i16(1, (4, 8, 8), 32, 8, K333, res=True, xh=1, yh=1, f9mode=2, bf16=bf())
    # every conv_f9h_kernel variant the planner can choose (see test_conv_fuzz_plan_h.py on variant 0)
    f["f9h v1"] = i16(2, (9, 10, 11), 96, 72, K333, res=True, xh=1, yh=0, stats=True, f9mode=2, bf16=bf())
    # (1,3,3): 256-voxel tiles at two workgroups per CU (v5) win every launch of at most 256 workgroups; the others need launches of
    # several rounds -- four 64-channel blocks -- where their tile wastes less: see f9h_variant
    f["f9h v2"] = i16(2, (50, 9, 25), 96, 256, K133, xh=1, yh=1, f9mode=2, bf16=bf())
    f["f9h v3"] = i16(2, (100, 9, 9), 32, 256, K133, xh=1, yh=0, res=True, stats=True, f9mode=2, bf16=bf())
    f["f9h v4"] = i16(3, (20, 20, 8), 64, 72, K133, xh=1, yh=1, stats=True, f9mode=2, bf16=bf())
    f["f9h v5"] = i16(2, (3, 8, 32), 64, 64, K133, xh=1, yh=0, stats=True, f9mode=2, bf16=bf())
    # refusals the entry point documents
    f["statistics with fp32 x: refused"] = i16(2, (3, 16, 16), 64, 72, K133, xh=0, yh=0, stats=True, f9mode=0, wgs=2, bf16=bf())
    f["statistics of a 1x1x1 conv: refused"] = i16(2, (4, 9, 10), 64, 72, K111, xh=1, yh=0, stats=True, f9mode=0, wgs=2, bf16=bf())
    f["16-bit y with a residual: refused"] = i16(2, (3, 16, 16), 64, 72, K133, res=True, xh=1, yh=1, f9mode=0, wgs=2, bf16=bf())
    # found by this fuzz: diqt_conv3d_fwd_h_stats_blocks promised 24 rows for a launch the entry point refuses (Cout % 8 != 0)
    f["statistics, Cout 12: refused"] = i16(2, (7, 10, 13), 16, 12, K311, xh=1, yh=0, stats=True, f9mode=2, wgs=3, bf16=bf())
    f["16-bit x, Cin 36: refused"] = i16(2, (3, 16, 16), 36, 72, K133, xh=1, yh=0, f9mode=0, wgs=2, bf16=bf())
    # the weight gradient with 16-bit tensors
    for k in (K333, K133, K311):
        cz = k == K311
        f["wgrad %dx%dx%d x16 dY16 ksplit 1" % k] = i16(1, (2, 4, 16), 32, 40, k, causal=cz, op="wgrad", xh=1, yh=1, bf16=bf())
        f["wgrad %dx%dx%d x16 dY16 ksplit > 1" % k] = i16(2, (5, 9, 18), 64, 72, k, causal=cz, op="wgrad", xh=1, yh=1, bf16=bf())
        f["wgrad %dx%dx%d x16 dY32" % k] = i16(1, (6, 9, 18), 96, 36, k, causal=cz, op="wgrad", xh=1, yh=0, bf16=bf())
        f["wgrad %dx%dx%d x32 dY32" % k] = i16(2, (3, 9, 20), 32, 136, k, causal=cz, op="wgrad", xh=0, yh=0, bf16=bf())
    f["wgrad several tiles per slice"] = i16(2, (8, 16, 32), 96, 136, K133, op="wgrad", xh=1, yh=1, bf16=bf())
    f["wgrad dY16 without x16: refused"] = i16(1, (4, 8, 16), 32, 32, K333, op="wgrad", xh=0, yh=1, bf16=bf())
    f["wgrad dY16, Cout 36: refused"] = i16(1, (4, 8, 16), 32, 36, K333, op="wgrad", xh=1, yh=1, bf16=bf())
    f["wgrad Cin 40: refused"] = i16(1, (4, 8, 16), 40, 32, K333, op="wgrad", xh=1, yh=1, bf16=bf())
    f["wgrad Cout 28: refused"] = i16(1, (4, 8, 16), 32, 28, K333, op="wgrad", xh=1, yh=0, bf16=bf())
    f["wgrad 1x1x1: refused"] = i16(1, (4, 8, 16), 32, 32, K111, op="wgrad", xh=1, yh=1, bf16=bf())
    return f


def _stats_ok(c):
    Do, Ho, Wo = out_extent(c)
    return c.Cin * taps(c) * Do * Ho * Wo <= MAX_STATS_WORK


def _io16(seed, n_ok=56, n_refused=16):
    rnd = random.Random(seed)
    out = list(fixed_io16(rnd).values())
    budget = MAX_MACS_SEED - sum(ref_macs(c) for c in out)
    cins = [8, 16, 24, 32, 32, 40, 64, 64, 72, 96, 128, 160, 12, 20, 36]
    couts = [8, 24, 32, 40, 64, 72, 130, 136, 12, 2]
    while n_ok + n_refused > 0:
        B, sp, Cin, Cout, k, pad, causal = _draw_geometry(rnd, cins, couts)
        xh, yh = rnd.choice([(1, 0), (1, 1), (1, 1), (0, 1), (0, 0)])
        c = i16(B, sp, Cin, Cout, k, pad=pad, causal=causal, res=rnd.random() < (0.5 if not yh else 0.1), xh=xh, yh=yh,
                stats=rnd.random() < (0.4 if xh else 0.05), bf16=rnd.randint(0, 1), f9mode=rnd.choice([0, 1, 2, 2]),
                wgs=rnd.choice([1, 2, 3, 5, 256]))
        if rnd.random() < 0.15:   # the weight gradient on the same draw
            c = c._replace(op="wgrad", res=False, stats=False, f9mode=1, wgs=256)
        if not _fits(c, budget / (n_ok + n_refused)) or (c.stats and not _stats_ok(c)):
            continue
        ok = route_io16(c)["ok"]
        if (ok and n_ok == 0) or (not ok and n_refused == 0):
            continue
        out.append(c)
        budget -= ref_macs(c)
        if ok:
            n_ok -= 1
        else:
            n_refused -= 1
    return out


def cases(family, seed):
    return {"ops16": _ops16, "io16": _io16}[family](seed)
