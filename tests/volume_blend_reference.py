"""Float64 specification of the blend modes of ``diffusioniqt_amd.inference.VolumeInference`` in plain numpy: candidate origins,
the 5 % rule, the taps (cast to fp32, then widened), per-sample numerator / denominator accumulation over the covering windows,
mean and unbiased deviation over the samples, the fill value of uncovered voxels and the background reset.  The sampler is
evaluated in fp32 on fp32 patches, as on the device; everything after it is float64.  Not a test module: the host and GPU tests
of the blend import it, with the shared inputs and the derived tolerance.
"""
import math

import numpy as np


def origins_of(shape, P, stride):
    """data.py:157-160: candidate origins in candidate order, and the lattice shape (G0, G1, G2)."""
    rng = [range(0, s - P + 1, stride) for s in shape]
    org = np.array([[i, j, k] for i in rng[0] for j in rng[1] for k in rng[2]], dtype=np.int64).reshape(-1, 3)
    return org, tuple(len(r) for r in rng)


def taps_of(P, kind, sigma_scale=0.125):
    """The 1-D window as the device holds it (fp32), widened to float64."""
    if kind == 'constant':
        t = np.ones(P, dtype=np.float32)
    elif kind == 'gaussian':
        i = np.arange(P, dtype=np.float64)
        t = np.exp(-(i - (P - 1) / 2.0) ** 2 / (2.0 * (sigma_scale * P) ** 2))
        t = (t / t.max()).astype(np.float32)
    else:
        raise ValueError(kind)
    return t.astype(np.float64)


def split_block(x, A):
    """utils_mine.py:25-42 on one [1,1,P,P,P] block: sub-volume n = b2 + f b3 + f^2 b4 (the first spatial axis runs fastest)."""
    f = x.shape[2] // A
    return np.stack([x[0, :, b2 * A:(b2 + 1) * A, b3 * A:(b3 + 1) * A, b4 * A:(b4 + 1) * A]
                     for b4 in range(f) for b3 in range(f) for b2 in range(f)])


def merge_block(sub, P):
    """utils_mine.py:44-67, the inverse of ``split_block``."""
    A = sub.shape[2]
    f = P // A
    out = np.empty((1, sub.shape[1], P, P, P), dtype=sub.dtype)
    for n in range(sub.shape[0]):
        b2, b3, b4 = n % f, (n // f) % f, n // (f * f)
        out[0, :, b2 * A:(b2 + 1) * A, b3 * A:(b3 + 1) * A, b4 * A:(b4 + 1) * A] = sub[n]
    return out


def blend_accumulate(patches, slot, taps, stride, shape, vol=None, mean=0.0, std=1.0, min_val=0.0, fill=0.0):
    """What ``diqt_volume_blend`` computes, in float64.  patches [S,N,P,P,P]; slot [G0,G1,G2] (< 0: not kept); taps [P]; ``vol`` the RAW
    fp32 volume or None.  Returns (mean, std, covered, background): float64 maps (std is zeros for S == 1) and two boolean masks."""
    patches = np.asarray(patches, dtype=np.float64)
    taps = np.asarray(taps, dtype=np.float64)
    S, N, P = patches.shape[:3]
    w3 = (taps[:, None, None] * taps[None, :, None]) * taps[None, None, :]
    num = np.zeros((S,) + tuple(shape), dtype=np.float64)
    den = np.zeros(shape, dtype=np.float64)
    G0, G1, G2 = slot.shape
    for g0 in range(G0):                                      # candidate order
        for g1 in range(G1):
            for g2 in range(G2):
                n = int(slot[g0, g1, g2])
                if n < 0:
                    continue
                i, j, k = g0 * stride, g1 * stride, g2 * stride
                num[:, i:i + P, j:j + P, k:k + P] += w3 * patches[:, n]
                den[i:i + P, j:j + P, k:k + P] += w3
    covered = den > 0
    b = np.where(covered, num / np.where(covered, den, 1.0), 0.0)
    out_mean = np.where(covered, b.mean(axis=0), np.float64(fill))
    out_std = np.where(covered, b.std(axis=0, ddof=1), 0.0) if S > 1 else np.zeros(shape, dtype=np.float64)
    background = np.zeros(shape, dtype=bool)
    if vol is not None:
        v32 = np.asarray(vol, dtype=np.float32)
        background = ((v32 - np.float32(mean)) / np.float32(std)) == np.float32(min_val)      # background_reset_kernel's expression
        out_mean = np.where(background, np.float64(np.float32(min_val)), out_mean)
        out_std = np.where(background, 0.0, out_std)
    return out_mean, out_std, covered, background


def reference(vol, cfg, sampler, samples=1, blend='gaussian', sigma_scale=0.125, nonzero_ratio=0.05):
    """The blend modes of ``VolumeInference(cfg, sampler, nonzero_ratio, blend, sigma_scale, samples)(vol, return_std=samples > 1)``.
    ``sampler`` takes and returns fp32 numpy arrays [B,1,A,A,A].  Returns a dict: mean, std (float64 [D,H,W]), covered, background
    (bool), max_abs_y (largest |sampler output|), kept, candidates, windows_per_voxel (the n of the tolerance)."""
    vol = np.asarray(vol, dtype=np.float32)
    tr = cfg['Train']
    sub, block = int(tr['patch_size_sub']), bool(tr.get('batch_sample', False))
    factor = int(tr.get('batch_sample_factor', 3))
    P = sub * factor if block else sub
    stride = int(cfg['Eval']['overlap'])
    batch = 1 if block else int(cfg['Eval'].get('batch_size', 27))
    mean32, std32 = np.float32(cfg['Data']['mean']), np.float32(cfg['Data']['std'])
    org, lattice = origins_of(vol.shape, P, stride)
    nz = np.array([np.count_nonzero(vol[i:i + P, j:j + P, k:k + P]) for i, j, k in org], dtype=np.float64)
    keep = nz / float(P ** 3) >= nonzero_ratio                                            # data.py:187-191
    kept = org[keep]
    N = kept.shape[0]
    slot = np.full(org.shape[0], -1, dtype=np.int64)
    slot[keep] = np.arange(N)
    patches = np.empty((samples, N, P, P, P), dtype=np.float32)
    for lo in range(0, N, batch):
        x = np.stack([((vol[i:i + P, j:j + P, k:k + P] - mean32) / std32)[None] for i, j, k in kept[lo:lo + batch]]).astype(np.float32)
        n = x.shape[0]
        if block:
            x = split_block(x, sub)
        for s in range(samples):
            y = np.asarray(sampler(x), dtype=np.float32)
            if block:
                y = merge_block(y, P)
            patches[s, lo:lo + n] = y.reshape(n, P, P, P)
    fill = (np.float32(0.) - mean32) / std32
    min_val = (vol.min() - mean32) / std32
    m, sd, covered, background = blend_accumulate(patches, slot.reshape(lattice), taps_of(P, blend, sigma_scale), stride, vol.shape, vol,
                                                  mean32, std32, min_val, fill)
    return dict(mean=m, std=sd, covered=covered, background=background, max_abs_y=float(np.abs(patches).max()) if N else 0.0,
                kept=N, candidates=org.shape[0], windows_per_voxel=math.ceil(P / stride) ** 3, fill=fill, min_val=min_val,
                patches=patches, slot=slot.reshape(lattice))


def tolerance(windows_per_voxel, max_abs_y):
    """A blended voxel is the ratio of two fp32 sums of at most n non-negative-weight terms: the standard summation bound gives
    |b - b64| <= (n + 3) 2^-23 max|y|.  The deviation map is allowed twice that (std is 1-Lipschitz in the sample vector up to
    sqrt(S / (S - 1)), plus Welford's own rounding, at S = 3)."""
    return (windows_per_voxel + 3) * 2.0 ** -23 * max_abs_y


# ---- the shared inputs ----------------------------------------------------------------------------------------------------------
def shared_volume():
    rng = np.random.default_rng(1)
    vol = rng.integers(1, 1000, (40, 36, 44)).astype(np.float32)
    vol[:, :, :20] = 0
    vol[:6] = 0
    return vol


def shared_cfg(stride, batch_size=7, P=16):
    return {'Data': {'mean': 300.0, 'std': 200.0, 'norm': 'z-score'},
            'Train': {'batch_sample': False, 'boundary': False, 'patch_size_sub': P, 'batch_sample_factor': 3},
            'Eval': {'batch_size': batch_size, 'overlap': stride}}


def block_volume():
    return np.random.default_rng(2).integers(1, 1000, (56, 56, 56)).astype(np.float32)


def block_cfg():
    return {'Data': {'mean': 300.0, 'std': 200.0, 'norm': 'z-score'},
            'Train': {'batch_sample': True, 'boundary': False, 'patch_size_sub': 8, 'batch_sample_factor': 3},
            'Eval': {'batch_size': 27, 'overlap': 16}}


def _rows(x):
    if isinstance(x, np.ndarray):
        return np.arange(x.shape[0], dtype=np.float32).reshape(-1, 1, 1, 1, 1)
    import torch
    return torch.arange(x.shape[0], device=x.device, dtype=x.dtype).view(-1, 1, 1, 1, 1)


def make_sampler(samples):
    """y = x 0.5 + 0.125 (r % 7) + 0.25 s x with r the row in the batch and s = (call counter) % samples, the sample the call draws:
    differs per window of a batch and per sample, so order and sample index are both visible in the result.  Works on fp32 numpy
    arrays and torch tensors alike, with the same roundings (every product is exact, each sum rounds once)."""
    calls = {'n': 0}

    def sampler(x):
        s = calls['n'] % samples
        calls['n'] += 1
        return x * 0.5 + 0.125 * (_rows(x) % 7) + (0.25 * s) * x
    return sampler


def make_window_sampler(samples):
    """As ``make_sampler`` with r the window's CANDIDATE index among the kept windows (a closure counter of the windows seen so far)
    instead of its batch row: the result may not depend on how the windows were batched."""
    state = {'calls': 0, 'seen': 0}

    def sampler(x):
        s = state['calls'] % samples
        r = _rows(x) + state['seen']
        state['calls'] += 1
        if s == samples - 1:
            state['seen'] += x.shape[0]
        return x * 0.5 + 0.125 * (r % 7) + (0.25 * s) * x
    return sampler
