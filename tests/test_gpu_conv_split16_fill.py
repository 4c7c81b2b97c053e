"""The fill tiles of the three-product split route (conv_split16_b.hip: conv_f9h_kernel variants 7 = 2 x 8 x 8 voxels and 8 = 1 x 8 x 8
voxels, ``ops.conv3d(split16="fill")`` / ``ops.gn_conv3d(split16="fill")``) against the 256-voxel tile (variant 6, ``split16=True``), a
float64 host convolution and the default route.  Small shapes under ``diqt_set_conv_f9h_mode(2)`` (no unit or work floor), every case
with both tiles pinned through ``diqt_set_conv_split16_fill_tile``.  Inputs and the GroupNorm + Mish reference come from
tests/f9w_worker.py as in test_gpu_conv_split16.py (whose scale / shift reference this one calls).

  one_chunk   1 x (8, 8, 16), 16 -> 64   residual + statistics   one chunk: the peeled first-chunk path only
  plain       1 x (8, 8, 16), 16 -> 64   neither                 the instantiation without residual and statistics
  co40        1 x (8, 8, 16), 32 -> 40   statistics, GN + Mish + scale / shift   two chunks, Cout padded to 64
  ragged      2 x (5, 12, 16), 48 -> 64  residual, GN + Mish + scale / shift     D ragged for the 128-voxel tile, H ragged for both
  walk        2 x (16, 16, 32), 16 -> 128  statistics            512 units of 64-voxel tiles on 256 workgroups: the persistent walk

A smaller tile changes which workgroup computes a voxel, not how: y must EQUAL variant 6's bit for bit.  The statistics rows are sums
over other voxel sets (their count is the fill query's), held to 1e-4 of float64 like the other producers'.  The error bounds are
test_gpu_conv_split16.py's: at or below the default route's on the same inputs, and below 2e-5.

Measured on an MI355X (both tiles the same, y being equal): max error / max |ref| 1.2e-7 / 1.9e-7 / 3.8e-7 / 4.0e-7 / 1.9e-7 in the order
above against 4.9e-7 / 8.7e-7 / 9.1e-7 / 8.0e-7 / 8.1e-7 on the default route; column sums and sums of squares within 8.3e-8."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import f9w_worker as worker  # noqa: E402
import test_gpu_conv_split16 as base  # noqa: E402

# f9w_worker case tuples (name, B, (D, H, W), Cin, Cout, pad, residual, GroupNorm-apply) + (scale/shift, statistics)
CASES = {
    "one_chunk": (("s16f_one", 1, (8, 8, 16), 16, 64, 1, True, False), False, True),
    "plain": (("s16f_plain", 1, (8, 8, 16), 16, 64, 1, False, False), False, False),
    "co40": (("s16f_co40", 1, (8, 8, 16), 32, 40, 1, False, True), True, True),
    "ragged": (("s16f_ragged", 2, (5, 12, 16), 48, 64, 1, True, True), True, False),
    "walk": (("s16f_walk", 2, (16, 16, 32), 16, 128, 1, False, False), False, True),
}
DEV = "cuda"
TAG = base.TAG
_RUNS = {}


def evaluate(name):
    if name in _RUNS:
        return _RUNS[name]
    try:
        _RUNS[name] = _evaluate(name)
    except RuntimeError as e:            # a HIP error: nothing more is started on the device in this session
        pytest.exit(f"{name}: {e}", returncode=3)
    return _RUNS[name]


def _evaluate(name):
    from diffusioniqt_amd import _lib, ops
    _lib.load()
    case, use_ss, stats = CASES[name]
    B, sp, Cin, Cout, pad = case[1], case[2], case[3], case[4], case[5]
    geo = (B, *sp, Cin, Cout, 3, 3, 3, pad, pad, pad, 0, 0, 0)
    t = worker.inputs(case)
    x, w, b, r, gamma, beta = t
    ss = torch.randn(B, 2 * Cin, generator=torch.Generator().manual_seed(len(name))) * 0.3 if use_ss else None
    cl = lambda v: None if v is None else v.permute(0, 2, 3, 4, 1).contiguous().to(DEV)
    dev_t = (cl(x), w.to(DEV), b.to(DEV), cl(r), gamma.to(DEV), beta.to(DEV))
    ssd = ss.to(DEV) if ss is not None else None
    idx, ref = base.reference(case, "mish", ss, t)
    run = lambda s16: base.launch(case, "mish", ssd, stats, dev_t, s16)
    assert ops.SPLIT16
    out = {}
    prev = _lib.query("diqt_set_conv_f9h_mode", 2)
    try:
        y0 = run(False)
        torch.cuda.synchronize()
        out["tag_default"] = _lib.last_launch()
        out["err_default"] = base.errors(y0, idx, ref)[0]
        _lib.query("diqt_get_last_conv_f9h_variant")
        y6 = run(True)
        torch.cuda.synchronize()
        out["tag6"], out["variant6"] = _lib.last_launch(), _lib.query("diqt_get_last_conv_f9h_variant")
        for v in (7, 8):
            _lib.query("diqt_set_conv_split16_fill_tile", v)
            y = run("fill")
            torch.cuda.synchronize()
            o = {"tag": _lib.last_launch(), "variant": _lib.query("diqt_get_last_conv_f9h_variant")}
            y2 = run("fill")
            o["equal6"] = torch.equal(y, y6)
            o["same"] = torch.equal(y, y2) and (not stats or torch.equal(y._diqt_stats.partials, y2._diqt_stats.partials))
            o["err"], o["stats"], o["sumsq"] = base.errors(y, idx, ref)
            if stats:
                o["nblk"], o["rows"] = y._diqt_stats.nblk, y._diqt_stats.partials.shape[1]
                o["nblk_query"] = _lib.query("diqt_conv3d_fwd_split16_fill_stats_blocks", *geo)
            out[v] = o
    finally:
        _lib.query("diqt_set_conv_split16_fill_tile", 0)
        _lib.query("diqt_set_conv_f9h_mode", prev)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [7, 8])
@pytest.mark.parametrize("name", list(CASES))
def test_fill_tile_equals_the_256_voxel_tile(name, variant):
    r = evaluate(name)
    v = r[variant]
    print(f"{name} variant {variant}: {v}  default {r['tag_default']} {r['err_default']:.3e}")
    stats = CASES[name][2]
    assert r["tag6"] == TAG and r["variant6"] == 6, f"split16=True ran {r['tag6']} variant {r['variant6']}"
    assert r["tag_default"] != TAG
    assert v["tag"] == TAG and v["variant"] == variant, f"ran {v['tag']} variant {v['variant']}"
    assert v["equal6"], "y differs from the 256-voxel tile's"
    if stats:
        assert v["nblk"] == v["rows"] == v["nblk_query"] > 0
        assert v["stats"] <= 1e-4 and v["sumsq"] <= 1e-4, f"column sums {v['stats']:.3e} / sums of squares {v['sumsq']:.3e}"
    assert v["err"] <= r["err_default"], f"max error {v['err']:.3e} above the default route's {r['err_default']:.3e}"
    assert v["err"] < 2e-5
    assert v["same"], "two runs differ"


@pytest.mark.gpu
def test_fill_request_honours_the_switch():
    """``ops.SPLIT16 = False`` switches ``split16="fill"`` off too, with the default route's bits; ``ops._split16_plan`` names the plan
    a request gets."""
    from diffusioniqt_amd import _lib, ops
    _lib.load()
    case = CASES["plain"][0]
    x, w, b, r, gamma, beta = worker.inputs(case)
    xd, wd, bd = x.permute(0, 2, 3, 4, 1).contiguous().to(DEV), w.to(DEV), b.to(DEV)
    geo = (case[1], *case[2], case[3], case[4], 3, 3, 3, 1, 1, 1, 0, 0, 0)
    prev = _lib.query("diqt_set_conv_f9h_mode", 2)
    try:
        with torch.no_grad():
            y_def = ops.conv3d(xd, wd, bd, 1)
            y_fill = ops.conv3d(xd, wd, bd, 1, split16="fill")
            torch.cuda.synchronize()
            assert _lib.last_launch() == TAG and _lib.query("diqt_get_last_conv_f9h_variant") == 8
            ops.SPLIT16 = False
            try:
                assert ops._split16_plan(geo, 0, "fill") is None
                y_off = ops.conv3d(xd, wd, bd, 1, split16="fill")
                torch.cuda.synchronize()
                assert _lib.last_launch() != TAG and torch.equal(y_off, y_def)
            finally:
                ops.SPLIT16 = True
            assert ops._split16_plan(geo, 0, "fill") == "_fill" and ops._split16_plan(geo, 0, True) == "" and ops._split16_plan(geo, 0, False) is None
            assert not torch.equal(y_fill, y_def)
    finally:
        _lib.query("diqt_set_conv_f9h_mode", prev)
    assert ops._split16_plan(geo, 0, "fill") is None          # default mode: the tiny shape is refused by both plans
