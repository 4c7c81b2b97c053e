#!/usr/bin/env python3
"""Micro-benchmark of the MFMA conv kernels on the dominant C2 shape (B=8, 32^3, 64->64, 3x3x3) — for
rocprofv3 --pmc passes and A/B timing.  Usage: python tools/conv_bench.py [fwd|bwdw|both|gn|s16|s16f|s16p|fwdh] [iters] [B S Cin Cout]"""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from diffusioniqt_amd import ops, _lib

mode = sys.argv[1] if len(sys.argv) > 1 else "both"
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 20
B, S, Cin, Cout = (int(v) for v in sys.argv[3:7]) if len(sys.argv) > 6 else (8, 32, 64, 64)
_lib.load()
dev = "cuda"
SP = tuple(int(v) for v in os.environ["SHAPE"].split(",")) if "SHAPE" in os.environ else (S, S, S)    # non-cubic volumes (Family B: frames x H x W)
x = torch.randn(B, *SP, Cin, device=dev)
KS = tuple(int(v) for v in os.environ.get("KSHAPE", "3,3,3").split(","))      # filter extents (padding = k // 2)
PADS = tuple(k // 2 for k in KS)
w = (torch.randn(Cout, Cin, *KS, device=dev) * 0.02).requires_grad_()
bias = torch.zeros(Cout, device=dev, requires_grad=True)
dy = torch.randn(B, *SP, Cout, device=dev)
flops = 2.0 * B * SP[0] * SP[1] * SP[2] * Cin * Cout * KS[0] * KS[1] * KS[2]


def timeit(fn, n):
    for _ in range(max(3, int(os.environ.get("WARM", "300")))):     # DVFS: clocks need ~100 ms of load to settle
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / n


if mode in ("fwd", "both"):
    with torch.no_grad():
        ms = timeit(lambda: ops.conv3d(x, w, bias, PADS), iters)
    print(f"conv fwd  B={B} {SP} k={KS} {Cin}->{Cout}: {ms*1e3:.1f} us  {flops/ms/1e9:.1f} TFLOP/s")
if mode == "gn":                # Block on the sampling path: GroupNorm-apply inside the conv staging vs groupnorm_act + conv3d
    gamma, beta = torch.randn(Cin, device=dev), torch.randn(Cin, device=dev)
    ss = torch.randn(B, 2 * Cin, device=dev) * 0.3
    act = ops.ACT_SILU if KS[0] == 1 else ops.ACT_MISH
    with torch.no_grad():
        assert ops.gn_conv3d(x, gamma, beta, ss, 8, act, 1e-5, w, bias, PADS) is not None, "shape not taken"
        ms_f = timeit(lambda: ops.gn_conv3d(x, gamma, beta, ss, 8, act, 1e-5, w, bias, PADS), iters)
        ms_c = timeit(lambda: ops.conv3d(x, w, bias, PADS), iters)
        ms_u = timeit(lambda: ops.conv3d(ops.groupnorm_act(x, gamma, beta, ss, 8, act), w, bias, PADS), iters)
    print(f"GN+act+conv B={B} {SP} k={KS} {Cin}->{Cout}: fused {ms_f*1e3:.1f} us (incl. statistics pass + coefficient launch), "
          f"two-kernel path {ms_u*1e3:.1f} us, conv alone {ms_c*1e3:.1f} us = {flops/ms_c/1e9:.1f} TFLOP/s")
if mode == "s16":               # Block on the sampling path: the three-product split (pre-pass + conv_f9h_kernel) vs the Winograd GroupNorm-apply launch
    gamma, beta = torch.randn(Cin, device=dev), torch.randn(Cin, device=dev)
    ss = torch.randn(B, 2 * Cin, device=dev) * 0.3
    gn = lambda s16: ops.gn_conv3d(x, gamma, beta, ss, 8, ops.ACT_MISH, 1e-5, w, bias, PADS, want_stats=True, split16=s16)
    with torch.no_grad():
        assert gn(True) is not None and "split16" in _lib.last_launch(), "shape not granted to the split route"
        assert gn(False) is not None and "split16" not in _lib.last_launch(), "no default GroupNorm-apply route for this shape"
        ms_s, ms_w = timeit(lambda: gn(True), iters), timeit(lambda: gn(False), iters)
        ms_s2, ms_w2 = timeit(lambda: gn(True), iters), timeit(lambda: gn(False), iters)
    print(f"GN+act+conv B={B} {SP} {Cin}->{Cout}: split16 {ms_s*1e3:.1f} / {ms_s2*1e3:.1f} us, Winograd {ms_w*1e3:.1f} / {ms_w2*1e3:.1f} us "
          f"(both incl. statistics / coefficient launch; two alternating rounds)")
if mode == "s16f":              # the split route's fill plan (128- / 64-voxel tiles) vs what split16=True runs on the shape (its 256-voxel tiles or, refused, the Winograd launch)
    gamma, beta = torch.randn(Cin, device=dev), torch.randn(Cin, device=dev)
    ss = torch.randn(B, 2 * Cin, device=dev) * 0.3
    gn = lambda s16: ops.gn_conv3d(x, gamma, beta, ss, 8, ops.ACT_MISH, 1e-5, w, bias, PADS, want_stats=True, split16=s16)
    rounds = int(os.environ.get("ROUNDS", "3"))
    with torch.no_grad():
        assert gn("fill") is not None and "split16" in _lib.last_launch(), "shape not granted to the fill plan"
        var = _lib.query("diqt_get_last_conv_f9h_variant")
        fused = gn(True) is not None      # (None: no one-launch route today -- the Block then runs groupnorm_act + conv3d)

        def old():
            if fused:
                return gn(True)
            return ops.conv3d(ops.groupnorm_act(x, gamma, beta, ss, 8, ops.ACT_MISH), w, bias, PADS, want_stats=True)
        old()
        today = _lib.last_launch()
        res = [(timeit(lambda: gn("fill"), iters), timeit(old, iters)) for _ in range(rounds)]
    print(f"GN+act+conv B={B} {SP} {Cin}->{Cout}: fill (variant {var}) " + " / ".join(f"{a*1e3:.1f}" for a, _ in res) + f" us, today ({today}) "
          + " / ".join(f"{b*1e3:.1f}" for _, b in res) + f" us (both incl. statistics / coefficient launch; {rounds} alternating rounds)")
if mode == "s16p":              # the split route's pair plan (variant 9: tap-paired 16x16x32 body) vs what "fill" runs on the shape today (variant 6 where the pair plan grants)
    gamma, beta = torch.randn(Cin, device=dev), torch.randn(Cin, device=dev)
    ss = torch.randn(B, 2 * Cin, device=dev) * 0.3
    gn = lambda s16: ops.gn_conv3d(x, gamma, beta, ss, 8, ops.ACT_MISH, 1e-5, w, bias, PADS, want_stats=True, split16=s16)
    rounds = int(os.environ.get("ROUNDS", "3"))
    with torch.no_grad():
        _lib.query("diqt_get_last_conv_f9h_variant")
        assert gn("pair") is not None and "split16" in _lib.last_launch(), "shape not granted to the split route"
        var = _lib.query("diqt_get_last_conv_f9h_variant")
        assert var == 9, f"shape not granted to the pair plan (variant {var})"
        assert gn("fill") is not None
        var_old = _lib.query("diqt_get_last_conv_f9h_variant")
        res = [(timeit(lambda: gn("pair"), iters), timeit(lambda: gn("fill"), iters)) for _ in range(rounds)]
    print(f"GN+act+conv B={B} {SP} {Cin}->{Cout}: pair (variant {var}) " + " / ".join(f"{a*1e3:.1f}" for a, _ in res) + f" us, today (variant {var_old}) "
          + " / ".join(f"{b*1e3:.1f}" for _, b in res) + f" us (both incl. pre-pass, statistics / coefficient launch; {rounds} alternating rounds)")
if mode in ("fwdh",):          # fp16 / bf16 operand kernel (LP=fp16|bf16)
    with torch.no_grad(), ops.low_precision(os.environ.get("LP", "fp16")):
        ms = timeit(lambda: ops.conv3d(x, w, bias, PADS), iters)
    print(f"conv fwd {os.environ.get('LP', 'fp16')}  B={B} {S}^3 {Cin}->{Cout}: {ms*1e3:.1f} us  {flops/ms/1e9:.1f} TFLOP/s")
if mode in ("bwdw", "both"):
    xr = x.clone()
    y = ops.conv3d(xr, w, bias, PADS)

    def bw():
        w.grad = None
        bias.grad = None
        y.backward(dy, retain_graph=True, inputs=[w, bias])
    ms = timeit(bw, iters)
    print(f"conv bwd-weight(+bias): {ms*1e3:.1f} us  {flops/ms/1e9:.1f} TFLOP/s")
