"""Worker of tests/test_gpu_conv_f9w_sched.py: cases of the Winograd F(2,3) tile of conv_fwd9_kernel (variant 7) that tests/f9w_worker.py
does not reach -- a workgroup walking two tiles (weight ring and halo prefetch across the tile boundary, the epilogue between them),
one-chunk tiles (every chunk end is a wrap), one-chunk split-K slabs with a residual, and ragged D, H and W tiles with statistics.
Per case it reports the variant that ran, the max error against a float64 host convolution, the errors of the epilogue statistics,
and the SHA-256 of the output bytes and of the statistics bytes.

  python tests/f9w_sched_worker.py main|ragged            prints one JSON line ("F9WS_RESULT {...}")
  python tests/f9w_sched_worker.py main|ragged --record   also writes the digests into tests/golden/f9w_sched_digests.json

"ragged" has to run under DIQT_CONV_F9=2 (the planner reads it once per process), which lets ragged shapes reach conv_fwd9_kernel.
The golden digests pin the kernel's results bit for bit: they are recorded with --record on a build of the commit whose results
are to be kept, and compared on every later build."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch

import f9w_worker  # noqa: E402  (inputs and the float64 reference: same tuple layout)

GOLDEN = os.path.join(ROOT, "tests", "golden", "f9w_sched_digests.json")

# (name, B, (D, H, W), Cin, Cout, pad, residual, GroupNorm-apply), statistics wanted
MAIN = [
    (("gna_walk", 8, (16, 16, 32), 32, 128, 1, True, True), True),          # 512 units on 256 workgroups, 2 chunks
    (("walk_plain", 8, (16, 16, 32), 32, 128, 1, True, False), True),       # the same through the plain build
    (("gna_one_chunk", 8, (16, 16, 32), 16, 64, 1, False, True), True),     # one chunk per tile
    (("gna_split_res", 2, (16, 16, 16), 128, 64, 1, True, True), False),    # split-K: 8 slabs of one chunk each
]
RAGGED = [
    (("gna_ragged_res", 2, (6, 12, 20), 32, 64, 1, True, True), True),      # ragged D, H and W tiles: the masked epilogue
]
GROUPS = {"main": MAIN, "ragged": RAGGED}


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def evaluate(case, want_stats, dev="cuda"):
    from diffusioniqt_amd import _lib, ops
    name, B, sp, Cin, Cout, pad, res, gna = case
    x, w, b, r, gamma, beta = f9w_worker.inputs(case)
    cl = lambda t: t.permute(0, 2, 3, 4, 1).contiguous().to(dev)
    pads = (pad, pad, pad)
    _lib.query("diqt_get_last_conv_fwd9_variant")                       # clears it
    with torch.no_grad():
        if gna:
            y = ops.gn_conv3d(cl(x), gamma.to(dev), beta.to(dev), None, 8, ops.ACT_MISH, 1e-5, w.to(dev), b.to(dev), pads,
                              cl(r) if res else None, want_stats=want_stats)
        else:
            y = ops.conv3d(cl(x), w.to(dev), b.to(dev), pads, residual=cl(r) if res else None, want_stats=want_stats)
    torch.cuda.synchronize()
    ran = _lib.query("diqt_get_last_conv_fwd9_variant")
    out = {"variant": ran, "taken": y is not None, "err": None, "stats": None, "sumsq": None, "y_sha": None, "stats_sha": None}
    if y is None:
        return out
    idx = [0, B - 1]
    ref = f9w_worker.reference(case, x, w, b, r, gamma, beta, idx)
    got = y.cpu().permute(0, 4, 1, 2, 3).double()[idx]
    out["err"] = (got - ref).abs().max().item() / max(ref.abs().max().item(), 1e-6)
    out["y_sha"] = sha(y)
    st = getattr(y, "_diqt_stats", None)
    if st is not None:
        s = st.partials.double().sum(1).cpu()[idx]                        # [len(idx), 2, Cout]
        rs, rq = ref.sum(dim=(2, 3, 4)), (ref * ref).sum(dim=(2, 3, 4))
        out["stats"] = (s[:, 0] - rs).abs().max().item() / max(rs.abs().max().item(), 1e-6)
        out["sumsq"] = (s[:, 1] - rq).abs().max().item() / max(rq.abs().max().item(), 1e-6)
        out["stats_sha"] = sha(st.partials)
    return out


def main():
    from diffusioniqt_amd import _lib
    _lib.load()
    group = sys.argv[1]
    out = {case[0]: evaluate(case, want) for case, want in GROUPS[group]}
    print("F9WS_RESULT " + json.dumps(out))
    if "--record" in sys.argv[2:]:
        gold = json.load(open(GOLDEN)) if os.path.exists(GOLDEN) else {}
        for name, v in out.items():
            assert v["variant"] == 7 and v["taken"], f"{name}: not a variant-7 launch, nothing to record"
            gold[name] = {"y_sha256": v["y_sha"], "stats_sha256": v["stats_sha"]}
        os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
        with open(GOLDEN, "w") as f:
            json.dump(gold, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
