"""Float64 restatement of torchmetrics 0.9.0 ``multiscale_structural_similarity_index_measure`` on 5-D input with the defaults
the reference's ``MSSIM`` uses (metrics.py:32-34): Gaussian window (sigma 1.5, 11 taps, generated in fp32 as torchmetrics does),
``k1=0.01, k2=0.03``, ``normalize=None``, ``data_range=None``.  torchmetrics is not available, so this text is the specification
the device kernels are tested against ("parity unpinned" for the third-party part, like ``oracle.iqt_data_oracle.ssim``):

per scale, on the current pair: range = max(p.max - p.min, t.max - t.min) over the whole tensor; the five moments filtered with
the separable Gaussian over the windows that lie fully inside the volume (what survives reflect-pad + crop); ``ssim`` and ``cs``
are the means of the two maps over all volumes and windows; then ``avg_pool3d(2)``.  Result: ``prod_s term_s ** beta_s`` with
``term_s = cs_s`` below the last scale and ``ssim`` at it — no clamp, a negative term gives NaN.

Also holds the formula-generated test volumes of tests/test_gpu_msssim.py (nothing is read from outside the tree).
"""
import numpy as np
import torch
import torch.nn.functional as F

BETAS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def gaussian_taps(sigma=1.5, dtype=torch.float64):
    k = int(3.5 * sigma + 0.5) * 2 + 1
    dist = torch.arange(start=(1 - k) / 2, end=(1 + k) / 2, step=1, dtype=torch.float32)
    g = torch.exp(-torch.pow(dist / sigma, 2) / 2)
    return (g / g.sum()).to(dtype)


def _filter_valid(x, g):
    """x: [N,1,D,H,W]; separable 'valid' convolution along D, H, W."""
    K = g.numel()
    x = F.conv3d(x, g.view(1, 1, K, 1, 1))
    x = F.conv3d(x, g.view(1, 1, 1, K, 1))
    return F.conv3d(x, g.view(1, 1, 1, 1, K))


def scale_terms(p, t, g, k1=0.01, k2=0.03, data_range=None):
    """p, t: [N,1,D,H,W] of one scale -> (ssim, cs, range) as Python floats."""
    rng = torch.maximum(p.max() - p.min(), t.max() - t.min()) if data_range is None else torch.as_tensor(data_range, dtype=p.dtype)
    c1, c2 = (k1 * rng) ** 2, (k2 * rng) ** 2
    mp, mt, mpp, mtt, mpt_ = (_filter_valid(v, g) for v in (p, t, p * p, t * t, p * t))
    mp2, mt2, mpt = mp * mp, mt * mt, mp * mt
    sp, st, spt = mpp - mp2, mtt - mt2, mpt_ - mpt
    upper, lower = 2 * spt + c2, sp + st + c2
    ssim = ((2 * mpt + c1) * upper) / ((mp2 + mt2 + c1) * lower)
    cs = upper / lower
    return float(ssim.mean()), float(cs.mean()), float(rng)


def msssim(pred, target, betas=BETAS, k1=0.01, k2=0.03, dtype=torch.float64, data_range=None):
    """pred, target: [B,C,D,H,W] (tensor or array).  Returns (ms_ssim, rows) with rows[s] = (ssim_s, cs_s, range_s)."""
    p = torch.as_tensor(pred).to(dtype)
    t = torch.as_tensor(target).to(dtype)
    assert p.ndim == 5 and p.shape == t.shape
    p, t = p.reshape(-1, 1, *p.shape[2:]), t.reshape(-1, 1, *t.shape[2:])
    g = gaussian_taps(dtype=dtype)
    rows = []
    for s in range(len(betas)):
        rows.append(scale_terms(p, t, g, k1, k2, data_range))
        if s + 1 < len(betas):
            p, t = F.avg_pool3d(p, 2), F.avg_pool3d(t, 2)
    terms = [r[1] for r in rows[:-1]] + [rows[-1][0]]
    with np.errstate(invalid='ignore'):
        value = float(np.prod([np.float64(x) ** np.float64(b) for x, b in zip(terms, betas)]))
    return value, rows


def terms_of(rows):
    """The factors of the product: cs below the last scale, ssim at it."""
    return [r[1] for r in rows[:-1]] + [rows[-1][0]]


def product_tolerance(value, rows, betas=BETAS, per_term=1e-5, own=2e-7):
    """First-order propagation of a per-term absolute tolerance through prod term ** beta, plus the fp32 result's own rounding."""
    return value * sum(b * per_term / x for b, x in zip(betas, terms_of(rows))) + own


# ---- formula-generated volumes ------------------------------------------------------------------------------------------------
def _grid(shape):
    D, H, W = shape
    return np.meshgrid(np.arange(D, dtype=np.int64), np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing='ij')


def hash_noise(shape, seed):
    """(h mod 1000) / 999 with the integer hash of oracle/iqt_infer_oracle.synthetic_volume (restated: three lines)."""
    i, j, k = _grid(shape)
    h = (i * 73856093) ^ (j * 19349663) ^ (k * 83492791) ^ (seed * 2654435761)
    h = (h ^ (h >> 13)) * 1274126177
    h = h ^ (h >> 16)
    return (h % 1000) / 999.0


def ball_and_structure(shape):
    D, H, W = shape
    i, j, k = _grid(shape)
    ball = ((i - D / 2) / D) ** 2 + ((j - 0.45 * H) / H) ** 2 + ((k - 0.55 * W) / W) ** 2 < 0.16
    s = (np.sin(.21 * i) * np.cos(.13 * j) + np.sin(.34 * k + .05 * i) + .5 * np.cos(.55 * (j + k))
         + 2 * np.sin(.023 * i) * np.sin(.031 * j) * np.sin(.027 * k))
    return ball, s


def target_volume(shape, seed=0):
    ball, s = ball_and_structure(shape)
    return np.where(ball, 600 + 150 * s + 40 * hash_noise(shape, seed), 0.0)


def noise_pred(shape, seed0=0, seed1=1):
    ball, s = ball_and_structure(shape)
    return np.where(ball, 1.1 * (600 + 150 * s) + 30 + 200 * (hash_noise(shape, seed1) - 0.5) + 40 * hash_noise(shape, seed0), 0.0)


def bias_texture_pred(shape):
    ball, s = ball_and_structure(shape)
    i, j, k = _grid(shape)
    base = 600 + 150 * s + 40 * hash_noise(shape, 0)
    pred = (base * (1 + 0.5 * np.sin(0.05 * i) * np.cos(0.04 * k)) + 120 * np.sin(0.09 * i + 0.07 * j) * np.cos(0.11 * k)
            + 100 * (hash_noise(shape, 1) - 0.5))
    return np.where(ball, pred, 0.0)


def blur_pred(shape):
    """5^3 box blur of the target (edge windows average the voxels they hold).  Not re-masked with the ball: the blur of a volume
    that is 0 outside the ball already is ~0 there, and this form gives the terms quoted in tests/test_gpu_msssim.py."""
    t =torch.as_tensor(target_volume(shape))[None, None]
    return F.avg_pool3d(t, 5, stride=1, padding=2, count_include_pad=False)[0, 0].numpy()


def minmax(x):
    return (x - x.min()) / (x.max() - x.min())
