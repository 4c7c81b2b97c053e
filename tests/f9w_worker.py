"""Worker of tests/test_gpu_conv_f9w.py: the 3x3x3 cases of the Winograd F(2,3) tile of conv_fwd9_kernel through ops.conv3d /
ops.gn_conv3d, with their max errors against float64 on the host, printed as one JSON line.  The test runs it with DIQT_CONV_F9W=1
and =0 (the direct tiles), so that the Winograd error can be held to a multiple of the direct one on the same inputs.
argv[1] = group: "main" runs the production routing (split-K where the planner splits), "ragged" runs under DIQT_CONV_F9=2 (set by
the test), which lets the ragged shapes reach conv_fwd9_kernel.  Per case it reports the variant the launch actually ran
(diqt_get_last_conv_fwd9_variant) and the split-K workspace the planner asked for."""
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

# (name, B, (D, H, W), Cin, Cout, pad, residual, GroupNorm-apply)
MAIN = [
    ("c2_32_64", 8, (32, 32, 32), 64, 64, 1, True, False),       # 32^3 level: persistent walk of two 256-voxel tiles per workgroup
    ("c2_16_128", 8, (16, 16, 16), 128, 128, 1, False, False),   # 16^3 level, one round
    ("c2_16_64", 8, (16, 16, 16), 64, 64, 1, True, False),       # 16^3 level 64 -> 64: split-K
    ("c2_8_128", 8, (8, 8, 8), 128, 128, 1, False, False),       # 8^3 level: split-K
    ("gna_32", 2, (32, 32, 32), 64, 64, 1, False, True),         # GroupNorm + Mish fused into the halo
    ("gna_16", 8, (16, 16, 16), 128, 128, 1, True, True),
    ("gna_8", 8, (8, 8, 8), 128, 128, 1, False, True),           # ... split-K
]
RAGGED = [
    ("ragged_dh", 2, (13, 11, 16), 48, 64, 1, True, False),      # ragged D and H tiles, 3 chunks of 16 channels
    ("cout_72", 2, (8, 16, 16), 64, 72, 1, False, False),        # Cout not a multiple of 64
    ("unpadded", 2, (10, 10, 18), 32, 64, 0, False, False),      # no zero padding: Wo = 16
]
SPLIT = ("c2_16_64", "c2_8_128", "gna_8")                          # split-K launches: no statistics (they come with the reduce)
CASES = MAIN + RAGGED
REF_B = 2           # float64 reference on the first and the last batch entry (the full conv in float64 takes the CPU minutes)


def inputs(case):
    name, B, sp, Cin, Cout, pad, res, gna = case
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    x = torch.randn(B, Cin, *sp, generator=g) * (1.7 if gna else 1.0) + (0.4 if gna else 0.0)
    if gna:
        x[:, :, :, :2] += 25.0                                  # activations beyond Mish's x > 20 branch
    w = torch.randn(Cout, Cin, 3, 3, 3, generator=g) / math.sqrt(Cin * 27)
    b = torch.randn(Cout, generator=g) * 0.1
    Do, Ho, Wo = (n + 2 * pad - 2 for n in sp)
    r = torch.randn(B, Cout, Do, Ho, Wo, generator=g) if res else None
    gamma, beta = torch.randn(Cin, generator=g), torch.randn(Cin, generator=g) * 0.3
    return x, w, b, r, gamma, beta


def reference(case, x, w, b, r, gamma, beta, idx):
    name, B, sp, Cin, Cout, pad, res, gna = case
    h = x[idx].double()
    if gna:
        h = F.mish(F.group_norm(h, 8, gamma.double(), beta.double(), eps=1e-5))
    ref = F.conv3d(h, w.double(), b.double(), padding=pad)
    return ref + r[idx].double() if res else ref


def run(case, dev="cuda"):
    from diffusioniqt_amd import ops
    name, B, sp, Cin, Cout, pad, res, gna = case
    want_stats = name not in SPLIT
    x, w, b, r, gamma, beta = inputs(case)
    cl = lambda t: t.permute(0, 2, 3, 4, 1).contiguous().to(dev)
    pads = (pad, pad, pad)
    with torch.no_grad():
        if gna:
            y = ops.gn_conv3d(cl(x), gamma.to(dev), beta.to(dev), None, 8, ops.ACT_MISH, 1e-5, w.to(dev), b.to(dev), pads,
                              cl(r) if res else None, want_stats=want_stats)
            assert y is not None, f"{name}: not taken by the GroupNorm-apply instantiation"
        else:
            y = ops.conv3d(cl(x), w.to(dev), b.to(dev), pads, residual=cl(r) if res else None, want_stats=want_stats)
    return y, (x, w, b, r, gamma, beta)


def main():
    from diffusioniqt_amd import _lib, ops
    _lib.load()
    out = {}
    for case in (RAGGED if sys.argv[1:] == ["ragged"] else MAIN):
        name, B, sp, Cin, Cout, pad, res, gna = case
        _lib.query("diqt_get_last_conv_fwd9_variant")                   # clears it
        y, (x, w, b, r, gamma, beta) = run(case)
        torch.cuda.synchronize()
        ran = _lib.query("diqt_get_last_conv_fwd9_variant")
        idx = [0, B - 1] if B > 1 else [0]
        ref = reference(case, x, w, b, r, gamma, beta, idx)
        got = y.cpu().permute(0, 4, 1, 2, 3).double()[idx]
        scale = max(ref.abs().max().item(), 1e-6)
        err = (got - ref).abs().max().item() / scale
        # epilogue statistics of the final y: per-(batch, channel) sums and sums of squares over its tiles
        serr = qerr = None
        st = getattr(y, "_diqt_stats", None)
        if st is not None:
            s = st.partials.double().sum(1).cpu()[idx]                      # [len(idx), 2, Cout]
            rs, rq = ref.sum(dim=(2, 3, 4)), (ref * ref).sum(dim=(2, 3, 4))
            serr = (s[:, 0] - rs).abs().max().item() / max(rs.abs().max().item(), 1e-6)
            qerr = (s[:, 1] - rq).abs().max().item() / max(rq.abs().max().item(), 1e-6)
        kd = (B, *sp, Cin, Cout, 3, 3, 3, pad, pad, pad, 0, 0, 0)
        npk = sum(ops._packed_len(w.shape, 0))
        out[name] = {"err": err, "stats": serr, "sumsq": qerr, "kid": _lib.query("diqt_conv3d_fwd_kernel_id", *kd), "variant": ran,
                     "ws": _lib.query("diqt_conv3d_fwd_workspace_bytes_pk", *kd, npk)}
    print("F9W_RESULT " + json.dumps(out))


if __name__ == "__main__":
    main()
