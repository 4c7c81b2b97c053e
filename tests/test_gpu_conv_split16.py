"""The three-product split route of the fp32 3x3x3 sampler convs (conv_split16.hip: ``ops.conv3d(split16=True)``,
``ops.gn_conv3d(split16=True)``) against a float64 host convolution.  Inputs come from tests/f9w_worker.py's helpers (its reference
too where the case is GroupNorm + Mish without conditioning; the SiLU / scale-shift references below follow it line by line).

The geometries are small ones the route's ``_supported`` query grants in its default mode -- at least 128 (4 x 8 x 8-voxel tile,
64-channel block) units -- AND whose default route is the Winograd tile (conv_fwd9_kernel variant 7), found with the queries on the CPU:
  walk2    4 x (16, 32, 32), 16 -> 128: 256 tiles x 2 channel blocks = 512 units on a grid of 256 = two tiles per workgroup; ONE chunk
  co128    2 x (16, 16, 32), 32 -> 128: 64 tiles x 2 channel blocks = the 128-unit threshold; two chunks
  co40     1 x (32, 32, 32), 32 -> 40: 128 tiles, Cout padded to 64
  ragged   2 x (30, 32, 32), 16 -> 64: the last D tile of each entry holds two planes
Per case: taken, the kernel tag and tile variant that ran, max error relative to max |ref| at or below that of the default route (the
same call with ``split16=False``, measured here on the same inputs) and below the 2e-5 the Winograd tile is held to, column sums and
sums of squares within 1e-4, two runs bit-identical.

Measured on an MI355X (max error / max |ref|: split route, default route, the default launch):
  walk2_plain        1.69e-7   3.90e-7   Winograd tile
  walk2_gn_mish_ss   3.56e-7   7.22e-7   Winograd tile, GN-apply
  co128_gn_silu      2.13e-7   3.52e-7   Winograd tile, split-K
  co128_plain_nores  2.82e-7   4.45e-7   Winograd tile, split-K
  co40_gn_mish       2.87e-7   3.64e-7   Winograd tile, GN, split-K
  co40_gn_silu_ss    2.68e-7   4.94e-7   Winograd tile, split-K
  ragged_plain       1.90e-7   3.98e-7   Winograd tile
  ragged_gn_mish     2.75e-7   6.23e-7   Winograd tile, GN-apply
  x_1e-3             4.15e-8   4.22e-8   Winograd tile, split-K
  x_300              2.66e-7   4.53e-7   Winograd tile, split-K
  w_1e-4             5.50e-8   5.98e-8   Winograd tile, split-K
(With ONE accumulator set for the head x head products the two-chunk cases read 4.7-6.2e-7 and four of them were above the Winograd
tile's split-K form: the error left is the fp32 accumulation of that chain, which the kernel therefore keeps in two halves.)"""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import f9w_worker as worker  # noqa: E402

# f9w_worker case tuples (name, B, (D, H, W), Cin, Cout, pad, residual, GroupNorm-apply) + (activation, scale/shift, statistics, what)
#   what: None | ("xscale", s) | ("wstd", s) | "planted"
CASES = {
    "walk2_plain": (("s16_walk2", 4, (16, 32, 32), 16, 128, 1, True, False), None, False, True, None),
    "walk2_gn_mish_ss": (("s16_walk2g", 4, (16, 32, 32), 16, 128, 1, False, True), "mish", True, True, None),
    "co128_gn_silu": (("s16_co128", 2, (16, 16, 32), 32, 128, 1, True, True), "silu", False, False, None),
    "co128_plain_nores": (("s16_co128p", 2, (16, 16, 32), 32, 128, 1, False, False), None, False, False, None),
    "co40_gn_mish": (("s16_co40", 1, (32, 32, 32), 32, 40, 1, True, True), "mish", False, True, None),
    "co40_gn_silu_ss": (("s16_co40s", 1, (32, 32, 32), 32, 40, 1, False, True), "silu", True, False, None),
    "ragged_plain": (("s16_ragged", 2, (30, 32, 32), 16, 64, 1, True, False), None, False, True, None),
    "ragged_gn_mish": (("s16_raggedg", 2, (30, 32, 32), 16, 64, 1, False, True), "mish", True, True, None),
    "x_1e-3": (("s16_xs", 2, (16, 16, 32), 32, 128, 1, False, False), None, False, False, ("xscale", 1e-3)),
    "x_300": (("s16_xl", 2, (16, 16, 32), 32, 128, 1, False, False), None, False, False, ("xscale", 300.0)),
    "w_1e-4": (("s16_ws", 2, (16, 16, 32), 32, 128, 1, False, False), None, False, False, ("wstd", 1e-4)),
}
DEV = "cuda"
TAG = "conv3d_fwd_split16(v9h)"


def make(name):
    case, act, use_ss, stats, what = CASES[name]
    x, w, b, r, gamma, beta = worker.inputs(case)
    B, Cin = case[1], case[3]
    if what and what[0] == "xscale":
        x = F.mish(x) * what[1]
    if what and what[0] == "wstd":
        w = w * (what[1] * (27 * Cin) ** 0.5)
    ss = torch.randn(B, 2 * Cin, generator=torch.Generator().manual_seed(len(name))) * 0.3 if use_ss else None
    return case, act, ss, stats, (x, w, b, r, gamma, beta)


def reference(case, act, ss, t):
    x, w, b, r, gamma, beta = t
    B, Cin, pad, res, gna = case[1], case[3], case[5], case[6], case[7]
    idx = [0, B - 1] if B > 1 else [0]
    if not gna or (act == "mish" and ss is None):
        return idx, worker.reference(case, x, w, b, r, gamma, beta, idx)
    h = F.group_norm(x[idx].double(), 8, gamma.double(), beta.double(), eps=1e-5)
    if ss is not None:
        s = ss[idx].double()
        h = h * (s[:, :Cin, None, None, None] + 1.0) + s[:, Cin:, None, None, None]
    h = F.mish(h) if act == "mish" else F.silu(h)
    ref = F.conv3d(h, w.double(), b.double(), padding=pad)
    return idx, (ref + r[idx].double() if res else ref)


def launch(case, act, ss, stats, dev_t, split16):
    from diffusioniqt_amd import ops
    x, w, b, r, gamma, beta = dev_t
    pads = (case[5],) * 3
    with torch.no_grad():
        if case[7]:
            a = ops.ACT_MISH if act == "mish" else ops.ACT_SILU
            y = ops.gn_conv3d(x, gamma, beta, ss, 8, a, 1e-5, w, b, pads, r, want_stats=stats, split16=split16)
            if y is None and not split16:         # SiLU: no GroupNorm-apply build of the Winograd tile -- the two-kernel default route
                y = ops.conv3d(ops.groupnorm_act(x, gamma, beta, ss, 8, a), w, b, pads, residual=r, want_stats=stats)
            return y
        return ops.conv3d(x, w, b, pads, residual=r, want_stats=stats, split16=split16)


def errors(y, idx, ref):
    got = y.cpu().permute(0, 4, 1, 2, 3).double()[idx]
    err = (got - ref).abs().max().item() / max(ref.abs().max().item(), 1e-30)
    serr = qerr = None
    st = getattr(y, "_diqt_stats", None)
    if st is not None:
        s = st.partials.double().sum(1).cpu()[idx]
        rs, rq = ref.sum(dim=(2, 3, 4)), (ref * ref).sum(dim=(2, 3, 4))
        serr = (s[:, 0] - rs).abs().max().item() / max(rs.abs().max().item(), 1e-30)
        qerr = (s[:, 1] - rq).abs().max().item() / max(rq.abs().max().item(), 1e-30)
    return err, serr, qerr


_RUNS = {}


def evaluate(name):
    if name in _RUNS:
        return _RUNS[name]
    try:
        return _evaluate(name)
    except RuntimeError as e:            # a HIP error: nothing more is started on the device in this session
        pytest.exit(f"{name}: {e}", returncode=3)


def _evaluate(name):
    from diffusioniqt_amd import _lib, ops
    _lib.load()
    case, act, ss, stats, t = make(name)
    B, sp, Cin, Cout, pad = case[1], case[2], case[3], case[4], case[5]
    geo = (B, *sp, Cin, Cout, 3, 3, 3, pad, pad, pad, 0, 0, 0)
    cl = lambda v: None if v is None else v.permute(0, 2, 3, 4, 1).contiguous().to(DEV)
    x, w, b, r, gamma, beta = t
    dev_t = (cl(x), w.to(DEV), b.to(DEV), cl(r), gamma.to(DEV), beta.to(DEV))
    ssd = ss.to(DEV) if ss is not None else None
    out = {"supported": _lib.query("diqt_conv3d_fwd_split16_supported", *geo)}
    assert ops.SPLIT16
    _lib.query("diqt_get_last_conv_f9h_variant")
    y = launch(case, act, ssd, stats, dev_t, True)
    torch.cuda.synchronize()
    out["tag"], out["variant"] = _lib.last_launch(), _lib.query("diqt_get_last_conv_f9h_variant")
    y2 = launch(case, act, ssd, stats, dev_t, True)
    _lib.query("diqt_get_last_conv_fwd9_variant")
    y0 = launch(case, act, ssd, stats, dev_t, False)
    torch.cuda.synchronize()
    out["tag_default"], out["variant_default"] = _lib.last_launch(), _lib.query("diqt_get_last_conv_fwd9_variant")
    idx, ref = reference(case, act, ss, t)
    out["err"], out["stats"], out["sumsq"] = errors(y, idx, ref)
    out["err_default"] = errors(y0, idx, ref)[0]
    out["same"] = torch.equal(y, y2) and (not stats or torch.equal(y._diqt_stats.partials, y2._diqt_stats.partials))
    out["nblk"] = y._diqt_stats.nblk if stats else None
    out["nblk_query"] = _lib.query("diqt_conv3d_fwd_split16_stats_blocks", *geo)
    _RUNS[name] = out
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_split16_against_float64(name):
    v = evaluate(name)
    print(f"{name}: {v}")
    stats = CASES[name][3]
    assert v["supported"] == 1, "the route's planner refuses this geometry"
    assert v["tag"] == TAG and v["variant"] == 6, f"ran {v['tag']} variant {v['variant']}"
    assert v["tag_default"] != TAG and v["variant_default"] == 7, "split16=False did not run the Winograd tile"
    assert v["err"] <= v["err_default"], f"max error {v['err']:.3e} above the default route's {v['err_default']:.3e}"
    assert v["err"] < 2e-5
    if stats:
        assert v["nblk"] == v["nblk_query"] > 0
        assert v["stats"] <= 1e-4 and v["sumsq"] <= 1e-4, f"column sums {v['stats']:.3e} / sums of squares {v['sumsq']:.3e}"
    assert v["same"], "two runs differ"


@pytest.mark.gpu
def test_split16_planted_activation_beyond_fp16_stays_finite():
    """An activation of 1e5 behind GroupNorm (a conditioning shift of 1e5 on one channel): the head is clamped to 65504, the output
    is finite (its accuracy in that channel's reach is not claimed)."""
    from diffusioniqt_amd import _lib, ops
    _lib.load()
    case, act, ss, stats, t = make("co40_gn_silu_ss")
    x, w, b, r, gamma, beta = t
    ss = ss.clone()
    ss[0, case[3] + 3] = 1e5
    cl = lambda v: None if v is None else v.permute(0, 2, 3, 4, 1).contiguous().to(DEV)
    y = launch(case, "mish", ss.to(DEV), True, (cl(x), w.to(DEV), b.to(DEV), cl(r), gamma.to(DEV), beta.to(DEV)), True)
    torch.cuda.synchronize()
    assert _lib.last_launch() == TAG
    assert torch.isfinite(y).all() and torch.isfinite(y._diqt_stats.partials).all()
    assert y.abs().max().item() > 1e3          # the planted value reached the output


@pytest.mark.gpu
def test_split16_switch_and_refused_weight():
    """``ops.SPLIT16 = False`` and a weight beyond the fp16 range both leave the launch on the default route, with its bits."""
    from diffusioniqt_amd import _lib, ops
    _lib.load()
    case, act, ss, stats, t = make("co128_plain_nores")
    x, w, b, r, gamma, beta = t
    xd = x.permute(0, 2, 3, 4, 1).contiguous().to(DEV)
    wd, bd = w.to(DEV), b.to(DEV)
    with torch.no_grad():
        y_def = ops.conv3d(xd, wd, bd, 1)
        ops.SPLIT16 = False
        try:
            y_off = ops.conv3d(xd, wd, bd, 1, split16=True)
            torch.cuda.synchronize()
            assert _lib.last_launch() != TAG and torch.equal(y_off, y_def)
        finally:
            ops.SPLIT16 = True
        wbig = wd.clone()
        wbig[5, 7, 1, 1, 1] = 7e4
        y_big = ops.conv3d(xd, wbig, bd, 1, split16=True)
        torch.cuda.synchronize()
        assert _lib.last_launch() != TAG and ops._packed_split16(wbig) is None
        assert torch.equal(y_big, ops.conv3d(xd, wbig, bd, 1))
        y_on = ops.conv3d(xd, wd, bd, 1, split16=True)
        torch.cuda.synchronize()
        assert _lib.last_launch() == TAG and not torch.equal(y_on, y_def)
