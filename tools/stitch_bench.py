"""The stitch phase of whole-volume inference alone, on one MI355X: gather, a free sampler (``x * 0.5 + 0.25``), stitching, background
reset -- ``VolumeInference`` with ``blend=None`` (crop-and-overwrite: one scatter launch per window once the stride is below half
a patch), ``blend='gaussian'`` (every window kept in HBM, one gather-side blend launch) and ``'gaussian'`` with 4 samples and the
deviation map.  Synthetic ellipsoid head as in tools/volume_bench.py.  The configurations alternate inside every round, so they see
the same machine state; medians and ranges over the rounds are reported, and the blend kernel is also timed on its own (device
events) against the bytes it has to move.
    python tools/stitch_bench.py [--size 256] [--patch 32] [--strides 32,16,8] [--rounds 9] [--batch 64] [--json PATH]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from diffusioniqt_amd import _lib, ops
from diffusioniqt_amd.inference import VolumeInference, blend_taps, sliding_window_origins

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=256)
ap.add_argument("--patch", type=int, default=32)
ap.add_argument("--strides", default="32,16,8")
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--json", default=None)
args = ap.parse_args()
_lib.load()
if not torch.cuda.is_available():
    raise SystemExit("stitch_bench: needs an MI355X (a CPU run measures nothing)")
dev = torch.device("cuda:0")
N, P = args.size, args.patch
strides = [int(s) for s in args.strides.split(",")]
MODES = (("blend=None", dict()), ("gaussian", dict(blend='gaussian')), ("gaussian x4 + std", dict(blend='gaussian', samples=4)))

ax = torch.linspace(-1, 1, N, device=dev)
zz, yy, xx = torch.meshgrid(ax, ax, ax, indexing="ij")
head = ((zz / 0.8) ** 2 + (yy / 0.7) ** 2 + (xx / 0.6) ** 2) < 1
vol = torch.where(head, 600 + 300 * torch.sin(9 * xx) * torch.cos(7 * yy) + 200 * zz, torch.zeros_like(xx)).float()
del zz, yy, xx, head
MEAN, STD = 271.64814106698583, 377.117173547721
sample_fn = lambda x: x * 0.5 + 0.25


def configs(stride):
    return {'Data': {'norm': 'z-score', 'mean': MEAN, 'std': STD},
            'Train': {'batch_sample': False, 'patch_size_sub': P, 'batch_sample_factor': 3},
            'Eval': {'overlap': stride, 'batch_size': args.batch}}


def run(stride, kw):
    inf = VolumeInference(configs(stride), sample_fn, **kw)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = inf(vol, return_std=True) if kw.get('samples', 1) > 1 else inf(vol)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


# warm-up of every configuration; the launches of the stitching kernels are counted on the way
info = {}
for stride in strides:
    for name, kw in MODES:
        with _lib.census() as c:
            _, out = run(stride, kw)
        info[(stride, name)] = dict(scatter_launches=c.count("patch_scatter"), blend_launches=c.count("volume_blend"))
        assert all(torch.isfinite(o).all() for o in (out if isinstance(out, tuple) else (out,)))
        del out
times = {k: [] for k in info}
for _ in range(args.rounds):
    for stride in strides:
        for name, kw in MODES:
            dt, out = run(stride, kw)
            del out
            times[(stride, name)].append(dt)

result = {"size": N, "patch": P, "batch": args.batch, "rounds": args.rounds, "device": torch.cuda.get_device_name(0), "stitch": [], "kernel": []}
print(f"stitch phase, {N}^3 volume, {P}^3 windows, batch {args.batch}, {args.rounds} alternating rounds (median [min .. max], ms)")
for stride in strides:
    org = sliding_window_origins((N, N, N), P, stride)
    for name, _ in MODES:
        t = sorted(times[(stride, name)])
        row = dict(stride=stride, mode=name, candidates=int(org.shape[0]), median_ms=statistics.median(t) * 1e3, min_ms=t[0] * 1e3,
                   max_ms=t[-1] * 1e3, **info[(stride, name)])
        result["stitch"].append(row)
        print(f"  stride {stride:2d}  {name:18s} {row['median_ms']:9.2f} [{row['min_ms']:9.2f} .. {row['max_ms']:9.2f}]   "
              f"{row['candidates']} candidates, {row['scatter_launches']} scatter / {row['blend_launches']} blend launches")

# the blend kernel alone: all candidate windows kept, S = 1 and S = 4 (with the deviation map), device events
print("volume_blend kernel alone (every candidate kept; bytes = patches read once + volume read + maps written)")
for stride in strides:
    G = len(range(0, N - P + 1, stride))
    n = G ** 3
    slot = torch.arange(n, dtype=torch.int32, device=dev).view(G, G, G)
    taps = torch.from_numpy(blend_taps(P, 'gaussian')).to(dev)
    for S in (1, 4):
        patches = torch.empty((S, n, P, P, P), dtype=torch.float32, device=dev).uniform_(-1, 1)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(12)]
        for i in range(11):                                   # the first launch is the warm-up
            ev[i].record()
            ops.volume_blend(patches, slot, taps, vol, MEAN, STD, -0.72, -0.72, stride, S > 1)
        ev[11].record()
        torch.cuda.synchronize()
        t = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(1, 11))
        nbytes = 4 * (patches.numel() + vol.numel() * (2 + (S > 1)))
        row = dict(stride=stride, samples=S, windows=n, median_ms=statistics.median(t), min_ms=t[0], max_ms=t[-1], bytes=nbytes,
                   tb_per_s=nbytes / statistics.median(t) / 1e9)
        result["kernel"].append(row)
        print(f"  stride {stride:2d}  S={S}  {n:6d} windows  {row['median_ms']:8.3f} [{t[0]:8.3f} .. {t[-1]:8.3f}] ms   "
              f"{nbytes / 1e9:7.3f} GB  {row['tb_per_s']:.2f} TB/s")
        del patches
print(json.dumps(result))
if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(result, f, indent=1)
