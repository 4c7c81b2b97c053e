"""The three-product split that carries the fp32 3x3x3 sampler convs on the fp16 matrix pipe (conv_split16.hip), on the host:

    xh = fp16(x)   xl = fp16((x - xh) 2^11)      wh = fp16(w)   wl = fp16((w - wh) 2^11)
    x w ~= xh wh + 2^-11 (xh wl + xl wh)          (tail x tail dropped)

emulated with fp16 rounding of heads and scaled tails and float64 products and sums, so the figures hold the split error alone.  Its
relative L2 error against a float64 convolution must stay below that of torch's fp32 conv3d on the same inputs (the reference the
sampler's results are held to); measured: 7-11e-8 against 2.5-2.6e-7.  This pins the scheme: tail scale 2^11, tail x tail dropped.
Also here: the route's ``_supported`` query refuses the tiny-network shapes of the parity / Winograd suites and grants the C2 levels."""
import math

import pytest
import torch
import torch.nn.functional as F


def split(t):
    head = t.to(torch.float16)
    tail = ((t - head.float()) * 2048.0).to(torch.float16)
    return head.double(), tail.double()


def split_conv(x, w):
    xh, xl = split(x)
    wh, wl = split(w)
    return F.conv3d(xh, wh, padding=1) + (F.conv3d(xh, wl, padding=1) + F.conv3d(xl, wh, padding=1)) / 2048.0


def rel_l2(a, ref):
    return ((a.double() - ref).norm() / ref.norm()).item()


# (Cin, Cout, size, input scale, weight std or None = 1 / sqrt(27 Cin))
CASES = [(64, 32, 16, 1.0, None), (256, 32, 8, 1.0, None), (64, 32, 16, 1e-3, None), (64, 32, 16, 300.0, None), (64, 32, 16, 1.0, 1e-4),
         (256, 32, 8, 1e-3, None), (256, 32, 8, 300.0, None), (256, 32, 8, 1.0, 1e-4)]


@pytest.mark.parametrize("Cin,Cout,S,xs,wstd", CASES)
def test_split_error_is_below_fp32_conv(Cin, Cout, S, xs, wstd):
    g = torch.Generator().manual_seed(Cin + S)
    act = F.mish if Cin == 64 else F.silu
    x = act(torch.randn(1, Cin, S, S, S, generator=g)) * xs
    w = torch.randn(Cout, Cin, 3, 3, 3, generator=g) * (wstd if wstd is not None else 1.0 / math.sqrt(27 * Cin))
    ref = F.conv3d(x.double(), w.double(), padding=1)
    e_split = rel_l2(split_conv(x, w), ref)
    e_fp32 = rel_l2(F.conv3d(x, w, padding=1), ref)
    print(f"split {e_split:.3e}  fp32 conv3d {e_fp32:.3e}")
    assert e_split < e_fp32


def test_supported_refuses_tiny_networks_and_grants_c2_levels():
    from diffusioniqt_amd import _lib
    _lib.load()
    q = lambda *geo: _lib.query("diqt_conv3d_fwd_split16_supported", *geo, 3, 3, 3, 1, 1, 1, 0, 0, 0)
    # the parity suite's tiny U-Nets (dim 8-16, 8^3-16^3 volumes, batch 1-2) and the ragged cases of the Winograd suite
    for geo in [(1, 8, 8, 8, 16, 16), (2, 8, 8, 8, 16, 32), (1, 16, 16, 16, 16, 16), (2, 16, 16, 16, 32, 32), (1, 4, 4, 4, 32, 32),
                (2, 13, 11, 16, 48, 64), (2, 8, 16, 16, 64, 72), (2, 8, 8, 8, 8, 8), (1, 16, 16, 16, 24, 24)]:
        assert q(*geo) == 0, geo
    # C2 sampler step, batch 8: the 32^3 and 16^3 levels are granted, the 8^3 level (64 units) stays on the Winograd tile's split-K
    assert q(8, 32, 32, 32, 64, 64) == 1 and q(8, 16, 16, 16, 128, 128) == 1 and q(8, 16, 16, 16, 64, 64) == 1
    assert q(8, 8, 8, 8, 256, 256) == 0 and q(8, 8, 8, 8, 128, 128) == 0
    assert q(8, 32, 32, 32, 24, 64) == 0 and q(8, 32, 32, 32, 64, 60) == 0          # Cin % 16, Cout % 8
    assert _lib.query("diqt_conv3d_fwd_split16_supported", 8, 32, 32, 32, 64, 64, 1, 3, 3, 0, 1, 1, 0, 0, 0) == 0      # 3x3x3 only
    assert _lib.query("diqt_conv3d_fwd_gn_split16_supported", 8, 32, 32, 32, 64, 64, 3, 3, 3, 1, 1, 1, 0, 0, 0, 99) == 0
    assert _lib.query("diqt_conv_packed_split16_elems", 64, 64, 3, 3, 3) == 4 * 27 * 64 * 32
    assert _lib.query("diqt_conv3d_fwd_split16_stats_blocks", 8, 32, 32, 32, 64, 64, 3, 3, 3, 1, 1, 1, 0, 0, 0) == 128 * 2
    assert _lib.query("diqt_conv3d_fwd_split16_variant", 8, 32, 32, 32, 64, 64, 3, 3, 3, 1, 1, 1, 0, 0, 0) == 6
