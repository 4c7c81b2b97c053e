"""The tap-paired build of the three-product split route (conv_split16_c.hip, conv_f9p_kernel.h: variant 9 on
v_mfma_f32_16x16x32_f16; ``ops.conv3d`` / ``ops.gn_conv3d(split16="pair")``) against a float64 host convolution, the default route and
variant 6.  Inputs, the reference, ``errors`` and ``launch`` are test_gpu_conv_split16.py's.  The small cases run under
``diqt_set_conv_f9h_mode(2)`` (no unit or work floor); the walk cases are granted in the default mode.

  one_chunk  1 x (8, 8, 16), 16 -> 64, residual + statistics        the peeled first chunk alone
  plain      the same, neither residual nor statistics
  co40       1 x (8, 8, 16), 32 -> 40, statistics, GN + Mish + ss   two chunks, padded Cout
  ragged     2 x (5, 12, 16), 48 -> 64, residual, GN + Mish + ss    three chunks, ragged D and H
  walk3      6 x (16, 32, 32), 16 -> 128, statistics                three tiles per workgroup, the weight ring wraps across tiles
  uneven     5 x (16, 32, 32), 16 -> 128, residual                  workgroups with three and with two tiles

Per case: the split kernel's launch tag and variant 9; max error / max |ref| at or below the default route's on the same inputs and
below 2e-5 (the bounds of test_gpu_conv_split16.py); column sums and sums of squares within 1e-4 of float64; two runs bit-identical.
``ops.SPLIT16 = False`` gives the default route's bits back.  A NaN planted one voxel outside an output's stencil leaves it finite.

Measured on an MI355X (max error / max |ref|: variant 9, variant 6 on the same inputs, the default route):
  one_chunk  1.93e-7   1.28e-7   4.58e-7
  plain      2.90e-7   1.89e-7   6.83e-7
  co40       6.31e-7   3.38e-7   1.69e-6
  ragged     5.00e-7   2.86e-7   7.45e-7   (default: split-K)
  walk3      3.38e-7   2.18e-7   5.55e-7   (default: Winograd tile)
  uneven     2.33e-7   1.58e-7   6.36e-7
(One head x head chain per block where variant 6 keeps two halves: 1.5-1.9 x its error.)"""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import f9w_worker as worker  # noqa: E402
import test_gpu_conv_split16 as base  # noqa: E402

# f9w_worker case tuples (name, B, (D, H, W), Cin, Cout, pad, residual, GroupNorm-apply) + (scale/shift, statistics, needs mode 2)
CASES = {
    "one_chunk": (("s16p_one", 1, (8, 8, 16), 16, 64, 1, True, False), False, True, True),
    "plain": (("s16p_plain", 1, (8, 8, 16), 16, 64, 1, False, False), False, False, True),
    "co40": (("s16p_co40", 1, (8, 8, 16), 32, 40, 1, False, True), True, True, True),
    "ragged": (("s16p_ragged", 2, (5, 12, 16), 48, 64, 1, True, True), True, False, True),
    "walk3": (("s16p_walk3", 6, (16, 32, 32), 16, 128, 1, False, False), False, True, False),
    "uneven": (("s16p_uneven", 5, (16, 32, 32), 16, 128, 1, True, False), False, False, False),
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


def _device_inputs(name):
    case, use_ss, stats, lifted = CASES[name]
    B, Cin = case[1], case[3]
    t = worker.inputs(case)
    x, w, b, r, gamma, beta = t
    ss = torch.randn(B, 2 * Cin, generator=torch.Generator().manual_seed(len(name))) * 0.3 if use_ss else None
    cl = lambda v: None if v is None else v.permute(0, 2, 3, 4, 1).contiguous().to(DEV)
    dev_t = (cl(x), w.to(DEV), b.to(DEV), cl(r), gamma.to(DEV), beta.to(DEV))
    return case, ss, stats, lifted, t, dev_t


def _evaluate(name):
    from diffusioniqt_amd import _lib, ops
    _lib.load()
    case, ss, stats, lifted, t, dev_t = _device_inputs(name)
    B, sp, Cin, Cout, pad = case[1], case[2], case[3], case[4], case[5]
    geo = (B, *sp, Cin, Cout, 3, 3, 3, pad, pad, pad, 0, 0, 0)
    ssd = ss.to(DEV) if ss is not None else None
    idx, ref = base.reference(case, "mish", ss, t)
    run = lambda s16: base.launch(case, "mish", ssd, stats, dev_t, s16)
    assert ops.SPLIT16
    out = {"granted_default_mode": _lib.query("diqt_conv3d_fwd_split16_pair_supported", *geo)}
    prev = _lib.query("diqt_set_conv_f9h_mode", 2) if lifted else None
    try:
        y0 = run(False)
        torch.cuda.synchronize()
        out["tag_default"] = _lib.last_launch()
        out["err_default"] = base.errors(y0, idx, ref)[0]
        _lib.query("diqt_get_last_conv_f9h_variant")
        y6 = run(True)
        torch.cuda.synchronize()
        out["variant6"] = _lib.query("diqt_get_last_conv_f9h_variant")
        out["err6"] = base.errors(y6, idx, ref)[0]
        y = run("pair")
        torch.cuda.synchronize()
        out["tag"], out["variant"] = _lib.last_launch(), _lib.query("diqt_get_last_conv_f9h_variant")
        y2 = run("pair")
        out["same"] = torch.equal(y, y2) and (not stats or torch.equal(y._diqt_stats.partials, y2._diqt_stats.partials))
        out["err"], out["stats"], out["sumsq"] = base.errors(y, idx, ref)
        if stats:
            out["nblk"] = y._diqt_stats.nblk
            out["nblk_query"] = _lib.query("diqt_conv3d_fwd_split16_pair_stats_blocks", *geo)
            out["nblk6"] = y6._diqt_stats.nblk
        ops.SPLIT16 = False
        try:
            y_off = run("pair")
            torch.cuda.synchronize()
            # None: the request was dropped and there is no one-launch default route for this shape (the caller then runs
            # groupnorm_act + conv3d, which is how y0 was made); otherwise the default route's launch and its bits
            out["off_declined"] = y_off is None
            out["tag_off"] = _lib.last_launch()
            out["off_equals_default"] = y_off is not None and torch.equal(y_off, y0)
        finally:
            ops.SPLIT16 = True
    finally:
        if lifted:
            _lib.query("diqt_set_conv_f9h_mode", prev)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_pair_against_float64(name):
    v = evaluate(name)
    print(f"{name}: {v}")
    stats, lifted = CASES[name][2], CASES[name][3]
    assert v["granted_default_mode"] == (0 if lifted else 1)
    assert v["tag"] == TAG and v["variant"] == 9, f"ran {v['tag']} variant {v['variant']}"
    assert v["variant6"] == 6
    assert v["err"] <= v["err_default"], f"max error {v['err']:.3e} above the default route's {v['err_default']:.3e}"
    assert v["err"] < 2e-5
    if stats:
        assert v["nblk"] == v["nblk_query"] == v["nblk6"] > 0
        assert v["stats"] <= 1e-4 and v["sumsq"] <= 1e-4, f"column sums {v['stats']:.3e} / sums of squares {v['sumsq']:.3e}"
    assert v["same"], "two runs differ"
    assert v["off_declined"] or (v["tag_off"] != TAG and v["off_equals_default"]), "ops.SPLIT16 = False did not give the default route back"


@pytest.mark.gpu
def test_pair_nan_outside_the_stencil_does_not_leak():
    """The half-empty fourteenth pair step: its upper-K lanes have zero weights and must re-read tap 26's row.  An unclamped read would
    take "tap 27" = halo row (kz, ky, kx) = (3, 0, 0), that is input voxel (d + 2, h - 1, w - 1) of output (d, h, w), and 0 x NaN is NaN.
    So x = NaN at input voxel (3, 4, 8) of the plain case: output (1, 5, 9) is the one such a read would poison, and (3, 4, 8) is outside
    its 3 x 3 x 3 neighbourhood (d = 0..2).  Every output whose neighbourhood holds the voxel is NaN, every other one is finite."""
    from diffusioniqt_amd import _lib, ops
    _lib.load()
    case, ss, stats, lifted, t, dev_t = _device_inputs("plain")
    x = dev_t[0].clone()
    x[0, 3, 4, 8, :] = float("nan")
    prev = _lib.query("diqt_set_conv_f9h_mode", 2)
    try:
        _lib.query("diqt_get_last_conv_f9h_variant")
        y = base.launch(case, "mish", None, False, (x,) + dev_t[1:], "pair")
        torch.cuda.synchronize()
        assert _lib.last_launch() == TAG and _lib.query("diqt_get_last_conv_f9h_variant") == 9
    finally:
        _lib.query("diqt_set_conv_f9h_mode", prev)
    inside = torch.zeros(y.shape[:4], dtype=torch.bool, device=y.device)
    inside[0, 2:5, 3:6, 7:10] = True
    assert torch.isfinite(y[0, 1, 5, 9]).all(), "the fourteenth step read a row from outside the stencil"
    assert torch.isnan(y[0, 2, 4, 8]).all() and torch.isnan(y[inside]).all(), "the planted value did not reach its own outputs"
    assert torch.isfinite(y[~inside]).all()
