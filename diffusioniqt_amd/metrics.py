"""Validation and evaluation metrics on the device (reference metrics.py:6-35).

``valid_step`` (trainer.py) min-max normalises both tensors and calls torchmetrics 0.9.0 (requirements.txt:201), which is not
vendored: ``peak_signal_noise_ratio(data_range=1.0)`` and ``StructuralSimilarityIndexMeasure(kernel_size=3, data_range=1.0)`` on
5-D tensors — i.e. the 3-D SSIM with torchmetrics' default GAUSSIAN window (sigma 1.5 -> 11 taps per axis; ``kernel_size`` only
sizes the uniform window and is ignored for the Gaussian one), reflect padding and a crop of the padded border.  Here the
normalisation, the five filtered moments, the SSIM map and its mean are two kernel launches on volumes that never leave HBM
(``diqt_minmax`` + ``diqt_ssim3d`` / ``diqt_psnr``, csrc/datapath.hip).  The evaluation script scores every reconstructed volume
with ``MSSIM`` (test_all.py:56-62 -> ``MultiScaleStructuralSimilarityIndexMeasure()``): ``diqt_msssim3d``, the same tile kernel
once per scale.  Parity: torchmetrics is absent from the reference tree and from this image, so these follow its published 0.9.0
algorithm (SSIM / PSNR restated in oracle/iqt_data_oracle.py, MS-SSIM in tests/msssim_reference.py) — "parity unpinned" for the
third-party part, pinned for the reference's own normalisation and call pattern.
"""
import numpy as np
import torch

from . import ops


def count_parameters(model):
    return sum(p.numel() for p in model.parameters() if p.requires_grad)


def _dev(t):
    t = t.detach()
    if not t.is_cuda:
        if not torch.cuda.is_available():
            raise RuntimeError("diffusioniqt_amd.metrics runs on the MI355X only (no CPU fallback); use oracle/ for CPU checks")
        t = t.cuda()
    return t.float().contiguous()


def _stats(p, t):
    return torch.cat((ops.minmax(p), ops.minmax(t)))


def gaussian_taps(sigma=1.5):
    """torchmetrics 0.9.0 ``_gaussian``: size int(3.5 sigma + 0.5) * 2 + 1, fp32 arithmetic (host; 11 numbers)."""
    k = int(3.5 * sigma + 0.5) * 2 + 1
    dist = torch.arange(start=(1 - k) / 2, end=(1 + k) / 2, step=1, dtype=torch.float32)
    g = torch.exp(-torch.pow(dist / sigma, 2) / 2)
    return np.ascontiguousarray((g / g.sum()).numpy())


def psnr_impl(pred, target):
    """metrics.py:9-15 (unused by the trainer): 20 log10(max(pred, target) / sqrt(mse))."""
    p, t = _dev(pred), _dev(target)
    mse = ops.psnr(p, t)[0]
    if mse == 0:
        return float('inf')
    peak = torch.maximum(ops.minmax(p)[1], ops.minmax(t)[1])
    return (20 * torch.log10(peak / torch.sqrt(mse))).to(pred.device)


def PSNR(pred, target):
    p, t = _dev(pred), _dev(target)
    return ops.psnr(p, t, _stats(p, t), 1.0)[1].to(pred.device)


def SSIM(pred, target, kernel_size=3, data_range=None):
    p, t = _dev(pred), _dev(target)
    if p.ndim != 5:
        raise NotImplementedError("SSIM: the reference's hot path only scores 5-D [B,C,D,H,W] volumes")
    p, t = p.reshape(-1, *p.shape[2:]), t.reshape(-1, *t.shape[2:])
    taps = gaussian_taps(1.5)
    if min(p.shape[1:]) < taps.shape[0]:
        # torchmetrics crops (K-1)/2 from every face of the SSIM map: nothing is left, and the mean of nothing is NaN
        return torch.full((), float('nan'), device=pred.device)
    if data_range is None:
        out = ops.ssim3d(p, t, taps, _stats(p, t), 1.0)
    else:
        out = ops.ssim3d(p, t, taps, None, float(data_range))
    return out[0].to(pred.device)


MSSIM_BETAS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def MSSIM(pred, target):
    """metrics.py:32-34, called on every volume by test_all.py:61: torchmetrics 0.9.0
    ``MultiScaleStructuralSimilarityIndexMeasure()`` with its defaults (Gaussian window, sigma 1.5, 11 taps, k1 0.01, k2 0.03,
    the five betas above, ``normalize=None``, ``data_range=None``) on a 5-D ``[B,C,D,H,W]`` pair.  Per scale: the SSIM and the
    contrast-sensitivity maps over the windows fully inside the volume, averaged over all volumes and windows, then a 2x2x2
    average pool; the result is ``prod_s term_s ** beta_s`` with ``term_s = cs_s`` below the last scale and ``ssim_4`` at it.
    The data range ``max(p.max - p.min, t.max - t.min)`` is refreshed per scale (``data_range=None`` reaches every per-scale
    ``_ssim_compute``, which resolves it on the pooled tensors); there is no ReLU or clamp, so a negative term gives NaN as
    ``torch.pow`` does; the batch is reduced before the powers.  Unlike ``SSIM`` / ``PSNR`` the inputs are NOT min-max normalised
    here — the script normalises before it calls (test_all.py:59-60).  Parity unpinned for the third-party part (no torchmetrics
    in the reference tree or this image): tests/msssim_reference.py restates the published algorithm.

    Size rule: torchmetrics raises ``ValueError`` when ``size // 16 <= 10`` on the last two axes; here all three of D, H, W are
    held to it (the last scale needs 11 voxels on every axis for one window to survive).  CPU or device tensors in, 0-d tensor on
    the input's device out.  One enqueue on the current stream: no host synchronisation between the scales."""
    if pred.ndim != 5 or target.ndim != 5:
        raise ValueError(f"MSSIM: expected 5-D [B,C,D,H,W] tensors, got {tuple(pred.shape)} and {tuple(target.shape)}")
    if pred.shape != target.shape:
        raise ValueError(f"MSSIM: shapes differ: {tuple(pred.shape)} and {tuple(target.shape)}")
    scales = len(MSSIM_BETAS)
    if any(s // 2 ** (scales - 1) <= 10 for s in pred.shape[2:]):
        raise ValueError(f"MSSIM: with {scales} scales and an 11-tap window every one of D, H, W must satisfy size // "
                         f"{2 ** (scales - 1)} > 10; got {tuple(pred.shape[2:])}")
    p, t = _dev(pred), _dev(target)
    p, t = p.reshape(-1, *p.shape[2:]), t.reshape(-1, *t.shape[2:])
    out = ops.msssim3d(p, t, gaussian_taps(1.5), np.asarray(MSSIM_BETAS, dtype=np.float32))
    return out[0].to(pred.device)
