"""TEST INFRASTRUCTURE: the bit fixture of the three-product split route (conv_split16.hip).  A change to conv_f9h_kernel that
leaves the arithmetic alone -- the same products, the chunk -> tap -> k-half order, the three accumulator sets, the bias behind the K
sum, the statistics rows in their layout and order -- leaves every y and every statistics row bit-identical; this records them.

Run on an MI355X on a checkout of the commit whose bits are the reference:   python tools/make_golden_split16_bits.py
Writes tests/golden/split16_bits.json: per case the SHA-256 of y and of the statistics partials (raw little-endian fp32 bytes in
memory order), with the commit named inside.  tests/test_gpu_conv_split16_bits.py imports CASES / run_case / digests from here.

Only ``ops.conv3d(..., split16=True)`` and ``ops.gn_conv3d(..., split16=True)`` are called, on inputs of tests/f9w_worker.py's seeded
helpers.  The cases (all granted in the default mode; (4, 8, 8)-voxel tiles, 64-channel blocks, a grid of 256 workgroups):
  walk3        6 x (16, 32, 32), 16 -> 128: 768 units = three tiles per workgroup, one chunk; residual {off, on} x statistics {off, on}
  uneven       5 x (16, 32, 32), 16 -> 128: 640 units = workgroups with three and with two tiles
  chunks2      4 x (16, 32, 32), 32 -> 128: two tiles x two chunks; GroupNorm + Mish with scale / shift, statistics
  chunks3      2 x (16, 16, 32), 48 -> 128: one tile per workgroup, three chunks, no residual
  co40_ragged  2 x (30, 32, 32), 16 -> 40: Cout padded to 64, last D tile of two planes; residual + statistics"""
import hashlib
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import f9w_worker as worker  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "split16_bits.json")
TAG = "conv3d_fwd_split16(v9h)"

# name -> (f9w_worker case tuple (seed name, B, (D, H, W), Cin, Cout, pad, residual generated, GroupNorm-apply), residual used,
#          statistics, scale / shift)
_W3 = ("s16b_walk3", 6, (16, 32, 32), 16, 128, 1, True, False)
CASES = {
    "walk3": (_W3, False, False, False),
    "walk3_stats": (_W3, False, True, False),
    "walk3_res": (_W3, True, False, False),
    "walk3_res_stats": (_W3, True, True, False),
    "uneven": (("s16b_uneven", 5, (16, 32, 32), 16, 128, 1, True, False), True, True, False),
    "chunks2": (("s16b_chunks2", 4, (16, 32, 32), 32, 128, 1, False, True), False, True, True),
    "chunks3": (("s16b_chunks3", 2, (16, 16, 32), 48, 128, 1, False, False), False, True, False),
    "co40_ragged": (("s16b_co40r", 2, (30, 32, 32), 16, 40, 1, True, False), True, True, False),
}


def geometry(name):
    case = CASES[name][0]
    return (case[1], *case[2], case[3], case[4], 3, 3, 3, case[5], case[5], case[5], 0, 0, 0)


def host_inputs(name):
    case, use_res, stats, use_ss = CASES[name]
    x, w, b, r, gamma, beta = worker.inputs(case)
    ss = torch.randn(case[1], 2 * case[3], generator=torch.Generator().manual_seed(len(name))) * 0.3 if use_ss else None
    return x, w, b, (r if use_res else None), gamma, beta, ss


def run_case(name, host=None, dev="cuda"):
    """Two launches of the case: [(y, statistics partials or None)] * 2, after a synchronize."""
    from diffusioniqt_amd import _lib, ops
    case, use_res, stats, use_ss = CASES[name]
    x, w, b, r, gamma, beta, ss = host if host is not None else host_inputs(name)
    cl = lambda t: None if t is None else t.permute(0, 2, 3, 4, 1).contiguous().to(dev)
    xd, wd, bd, rd = cl(x), w.to(dev), b.to(dev), cl(r)
    pads = (case[5],) * 3
    out = []
    with torch.no_grad():
        for _ in range(2):
            if case[7]:
                y = ops.gn_conv3d(xd, gamma.to(dev), beta.to(dev), ss.to(dev) if ss is not None else None, 8, ops.ACT_MISH, 1e-5, wd, bd,
                                  pads, rd, want_stats=stats, split16=True)
            else:
                y = ops.conv3d(xd, wd, bd, pads, residual=rd, want_stats=stats, split16=True)
            torch.cuda.synchronize()
            assert y is not None and _lib.last_launch() == TAG, f"{name}: ran {_lib.last_launch()}"
            out.append((y, y._diqt_stats.partials if stats else None))
    return out


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def digests(y, partials):
    return {"y": sha(y), "stats": sha(partials) if partials is not None else None}


if __name__ == "__main__":
    from diffusioniqt_amd import _lib
    _lib.load()
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    out = {"commit": (sys.argv[1] if len(sys.argv) > 1 else commit) or "unknown",
           "what": "SHA-256 of y and of the statistics partials (fp32 bytes in memory order) per case of tools/make_golden_split16_bits.py",
           "cases": {}}
    for name in CASES:
        assert _lib.query("diqt_conv3d_fwd_split16_supported", *geometry(name)) == 1, f"{name}: not granted"
        (y, st), (y2, st2) = run_case(name)
        assert torch.equal(y, y2) and (st is None or torch.equal(st, st2)), f"{name}: two runs differ"
        out["cases"][name] = digests(y, st)
        print(name, out["cases"][name])
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", GOLDEN)
