"""Winograd F(2,3) tile of conv_fwd9_kernel (variant 7, the fp32 3x3x3 forward convs): routing, float64 accuracy held to the direct
tiles' on the same inputs (tests/f9w_worker.py, once with DIQT_CONV_F9W=1 and once with =0), epilogue statistics, determinism and
placement, and the Winograd weight panels of diqt_conv_pack_weight modes 2 / 3."""
import json
import math
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import f9w_worker  # noqa: E402

DEV = "cuda"
C2_SHAPES = [(8, 32, 64, 64), (8, 32, 128, 64), (8, 16, 128, 128), (8, 16, 192, 128), (8, 16, 64, 64), (8, 8, 128, 128)]


@pytest.fixture(scope="module")
def lib():
    from diffusioniqt_amd import _lib
    _lib.load()
    return _lib


@pytest.fixture(scope="module")
def worker_runs():
    runs = {"1": {}, "0": {}}
    for group in ("main", "ragged"):
        for f9w in ("1", "0"):
            env = dict(os.environ, DIQT_CONV_F9W=f9w)
            if group == "ragged":
                env["DIQT_CONV_F9"] = "2"
            r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "f9w_worker.py"), group], env=env, capture_output=True,
                               text=True, timeout=900)
            assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("F9W_RESULT ")]
            assert line, r.stdout[-3000:]
            runs[f9w].update(json.loads(line[-1][len("F9W_RESULT "):]))
    return runs


@pytest.mark.gpu
@pytest.mark.parametrize("B,S,Cin,Cout", C2_SHAPES)
def test_c2_shapes_take_the_winograd_variant(lib, B, S, Cin, Cout):
    geo = (B, S, S, S, Cin, Cout, 3, 3, 3, 1, 1, 1, 0, 0, 0)
    n, nw = lib.query("diqt_conv_packed_elems", Cout, Cin, 3, 3, 3), lib.query("diqt_conv_packed_wino_elems", Cout, Cin, 3, 3, 3)
    assert lib.query("diqt_conv3d_fwd_kernel_id", *geo) == 4
    assert lib.query("diqt_conv3d_fwd9_variant", *geo, n + nw) == 7
    assert lib.query("diqt_conv3d_fwd9_variant", *geo, n) in (0, 1), "a direct pack alone keeps the direct tiles"


@pytest.mark.gpu
def test_odd_output_width_and_other_filters_stay_direct(lib):
    big = 1 << 24                                                     # any length: the panels exist only for 3x3x3 filters
    assert lib.query("diqt_conv3d_fwd9_variant", 8, 32, 32, 31, 64, 64, 3, 3, 3, 1, 1, 1, 0, 0, 0, big) != 7
    assert lib.query("diqt_conv3d_fwd9_variant", 8, 32, 32, 32, 64, 64, 1, 3, 3, 0, 1, 1, 0, 0, 0, big) != 7
    assert lib.query("diqt_conv3d_fwd9_variant", 8, 32, 32, 32, 64, 64, 3, 1, 1, 1, 0, 0, 0, 0, 0, big) != 7


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c[0] for c in f9w_worker.CASES])
def test_winograd_against_float64_and_the_direct_tiles(worker_runs, name):
    w, d = worker_runs["1"][name], worker_runs["0"][name]
    assert w["kid"] == 4 and w["variant"] == 7, f"the launch ran variant {w['variant']}"
    assert d["variant"] in (0, 1), "DIQT_CONV_F9W=0 must force the direct tiles"
    if name in f9w_worker.SPLIT:
        assert w["ws"] > 0 and d["ws"] > 0, "a split-K case must be a split-K launch"
    assert w["err"] <= 2e-5, f"{name}: Winograd max error {w['err']:.3e} vs float64"
    assert w["err"] <= 4 * d["err"], f"{name}: Winograd error {w['err']:.3e} > 4x the direct tiles' {d['err']:.3e}"
    if w["stats"] is not None:
        assert w["stats"] <= 1e-4 and w["sumsq"] <= 1e-4, f"{name}: column sums {w['stats']:.3e} / sums of squares {w['sumsq']:.3e}"


def _conv(case, x, w, b, r):
    from diffusioniqt_amd import ops
    pad = case[5]
    cl = lambda t: t.permute(0, 2, 3, 4, 1).contiguous().to(DEV)
    with torch.no_grad():
        return ops.conv3d(cl(x), w.to(DEV), b.to(DEV), (pad,) * 3, residual=cl(r) if r is not None else None)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["c2_16_128", "c2_16_64", "c2_32_64"])
def test_winograd_determinism_and_placement(lib, name):
    case = [c for c in f9w_worker.CASES if c[0] == name][0]
    B, sp, Cin, Cout, pad = case[1], case[2], case[3], case[4], case[5]
    x, w, b, r, _, _ = f9w_worker.inputs(case)
    lib.query("diqt_get_last_conv_fwd9_variant")
    y = _conv(case, x, w, b, r)
    torch.cuda.synchronize()
    assert lib.query("diqt_get_last_conv_fwd9_variant") == 7
    assert torch.equal(_conv(case, x, w, b, r), y), "two runs must give identical bits"
    rolled = _conv(case, torch.roll(x, 1, 0), w, b, torch.roll(r, 1, 0) if r is not None else None)
    assert torch.equal(rolled, torch.roll(y, 1, 0)), "a batch-rotated input must give the batch-rotated output"
    rolled = _conv(case, x, torch.roll(w, 32, 0), torch.roll(b, 32, 0), torch.roll(r, 32, 1) if r is not None else None)
    assert torch.equal(rolled, torch.roll(y, 32, 4)), "an output-channel-rotated filter must give the channel-rotated output"


@pytest.mark.gpu
def test_direct_pack_through_the_plain_entry_points_stays_direct_and_correct(lib):
    """A caller of the C ABI that packs with mode 0 into diqt_conv_packed_elems floats and calls diqt_conv3d_fwd on a C2 shape gets
    the direct tiles (never a read of panels behind its buffer); diqt_conv3d_fwd_pk refuses a buffer shorter than the direct pack."""
    from diffusioniqt_amd import ops
    import torch.nn.functional as F
    B, S, Cin, Cout = 8, 32, 64, 64
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B, Cin, S, S, S, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, 3, generator=g) / math.sqrt(Cin * 27)
    b = torch.randn(Cout, generator=g) * 0.1
    n = lib.query("diqt_conv_packed_elems", Cout, Cin, 3, 3, 3)
    packed = torch.empty(n, dtype=torch.float32, device=DEV)
    s = ops._stream()
    lib.call("diqt_conv_pack_weight", w.to(DEV), packed, Cout, Cin, 3, 3, 3, 0, s)
    xd, bd = x.permute(0, 2, 3, 4, 1).contiguous().to(DEV), b.to(DEV)
    y = torch.empty(B, S, S, S, Cout, device=DEV)
    geo = (B, S, S, S, Cin, Cout, 3, 3, 3, 1, 1, 1, 0, 0, 0)
    lib.query("diqt_get_last_conv_fwd9_variant")
    lib.call("diqt_conv3d_fwd", xd, packed, bd, None, y, *geo, s)
    torch.cuda.synchronize()
    assert lib.query("diqt_get_last_conv_fwd9_variant") in (0, 1)
    y2 = torch.empty_like(y)
    lib.call("diqt_conv3d_fwd_pk", xd, packed, n, bd, None, y2, None, None, 0, *geo, s)
    torch.cuda.synchronize()
    assert lib.query("diqt_get_last_conv_fwd9_variant") in (0, 1)
    assert torch.equal(y, y2), "the _pk entry with the direct pack's length is the plain entry"
    with pytest.raises(RuntimeError):
        lib.call("diqt_conv3d_fwd_pk", xd, packed, n - 1, bd, None, y2, None, None, 0, *geo, s)
    ref = F.conv3d(x[[0, B - 1]].double(), w.double(), b.double(), padding=1)
    got = y.cpu().permute(0, 4, 1, 2, 3).double()[[0, B - 1]]
    assert (got - ref).abs().max().item() / ref.abs().max().item() <= 2e-5


@pytest.mark.gpu
def test_backward_data_keeps_the_direct_tiles(lib):
    """Only forward packs carry the Winograd panels: the backward-data launch of a 3x3x3 conv (mode-1 pack) runs a direct tile."""
    from diffusioniqt_amd import ops
    g = torch.Generator().manual_seed(5)
    x = torch.randn(8, 16, 16, 16, 64, generator=g).to(DEV).requires_grad_(True)
    w = (torch.randn(64, 64, 3, 3, 3, generator=g) / math.sqrt(64 * 27)).to(DEV)
    y = ops.conv3d(x, w, None, (1, 1, 1))
    lib.query("diqt_get_last_conv_fwd9_variant")
    y.backward(torch.ones_like(y))
    torch.cuda.synchronize()
    assert lib.query("diqt_get_last_conv_fwd9_variant") in (0, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [2, 3])
def test_winograd_weight_panels_against_a_float64_transform(lib, mode):
    Cout, Cin = 80, 48                 # both multiples of 16 (mode 3 packs the (Cin, Cout)-swapped filter), Cout not of 64
    g = torch.Generator().manual_seed(mode)
    w = torch.randn(Cout, Cin, 3, 3, 3, generator=g)
    eff = (Cout, Cin) if mode == 2 else (Cin, Cout)
    n = lib.query("diqt_conv_packed_elems", *eff, 3, 3, 3)
    nw = lib.query("diqt_conv_packed_wino_elems", *eff, 3, 3, 3)
    assert nw == n // 27 * 36
    wd = w.to(DEV)
    packed = torch.zeros(n + nw, dtype=torch.float32, device=DEV)
    direct = torch.zeros(n, dtype=torch.float32, device=DEV)
    lib.call("diqt_conv_pack_weight", wd, packed, Cout, Cin, 3, 3, 3, mode, 0)
    lib.call("diqt_conv_pack_weight", wd, direct, Cout, Cin, 3, 3, 3, mode - 2, 0)
    torch.cuda.synchronize()
    assert torch.equal(packed[:n], direct), "modes 2 / 3 start with the direct pack of mode 0 / 1"
    # effective filter [out][in][kd][kh][kw] (mode 3: in / out swapped, taps flipped), F(2,3) transform along kw in float64
    ge = w.double() if mode == 2 else w.double().flip(2, 3, 4).transpose(0, 1)
    g0, g1, g2 = ge[..., 0], ge[..., 1], ge[..., 2]
    U = torch.stack([g0, (g0 + g1 + g2) / 2, (g0 - g1 + g2) / 2, g2], -1)          # [out][in][kd][kh][j]
    outE, inE = eff
    coPad, nCh = (outE + 63) // 64 * 64, (inE + 31) // 32
    ref = torch.zeros(nCh, 36, coPad, 32, dtype=torch.float64)
    Ur = U.reshape(outE, inE, 36)                                                    # tap = (kd * 3 + kh) * 4 + j
    for c in range(nCh):
        k = min(32, inE - 32 * c)
        ref[c, :, :outE, :k] = Ur[:, 32 * c:32 * c + k, :].permute(2, 0, 1)
    got = packed[n:].cpu().double().reshape(nCh, 36, coPad, 32)
    err = (got - ref).abs().max().item() / ref.abs().max().item()
    assert err < 1e-6, f"Winograd panels vs float64 transform: {err:.3e}"
