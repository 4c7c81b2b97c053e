"""Float64 specification of the lockstep joint sampling of ``diffusioniqt_amd.inference.VolumeInference(joint=True)`` in plain numpy:
one noisy state for the whole volume, per step the kept windows' x0 predictions fused per voxel with the blend weights
(``volume_blend_reference.blend_accumulate`` on the clamped predictions), the sampler step with the volume-anchored normals
(``anchored_noise_reference``), and the finish (final clamp, fill, background, mean / deviation over the samples).  Candidate origins,
the 5 % rule, the taps and the low-res windows (fp32, then widened) are the blend specification's; everything else is float64.  Not a
test module: the host and GPU tests of the joint mode import it, with the shared inputs and the derived bounds.
"""
import math

import numpy as np

from tests import anchored_noise_reference as A
from tests import volume_blend_reference as R

STEPS = 4
MIN_BOUND = -0.75
SEED = 11
_NORMALS = {}


def normals(shape, seed, draw, sample):
    """Float64 normals [D,H,W] of channel 0 of the anchored field (cached, read only)."""
    key = (tuple(shape), seed, draw, sample)
    if key not in _NORMALS:
        _NORMALS[key] = A.normals(A.field(shape, 1, seed, draw, sample))[0]
        _NORMALS[key].setflags(write=False)
    return _NORMALS[key]


def clamp_of(lo, hi, mode):
    """``ddpm_step_kernel``'s clamp: mode 0 is max(y, lo), mode 1 is clip(y, lo, hi)."""
    return (lambda v: np.maximum(v, lo)) if mode == 0 else (lambda v: np.clip(v, lo, hi))


def tables(scheduler, steps, eta, objective):
    """The chain's host numbers as the device holds them (fp32, widened): coefs [T,3] = (kx, k0, kn), x0c [T,2] = the (a, b) of
    x0 = a x + b pred as the ancestral branch forms them, log_snr [T]."""
    import torch
    from diffusioniqt_amd.imagen_pytorch3D import log_snr_to_alpha_sigma
    pairs = list(scheduler.get_sampling_timesteps(1, device='cpu', steps=steps))
    coefs = torch.stack([torch.stack(scheduler.ddim_coefficients(t, tn, eta)) for t, tn in pairs]).numpy()[:, :, 0]
    conds = torch.stack([scheduler.log_snr(t) for t, _ in pairs])
    al, sg = log_snr_to_alpha_sigma(conds)
    x0c = torch.stack((1. / al.clamp(min=1e-8), -sg / al.clamp(min=1e-8)) if objective == 'noise' else (al, -sg), dim=1).numpy()[:, :, 0]
    return coefs.astype(np.float64), x0c.astype(np.float64), conds.numpy()[:, 0].astype(np.float64)


def layout(vol, cfg, nonzero_ratio=0.05):
    """Windows of a volume under a config: P, stride, block mode, kept origins, the slot lattice, windows per voxel."""
    vol = np.asarray(vol, dtype=np.float32)
    tr = cfg['Train']
    sub, block = int(tr['patch_size_sub']), bool(tr.get('batch_sample', False))
    factor = int(tr.get('batch_sample_factor', 3))
    P = sub * factor if block else sub
    stride = int(cfg['Eval']['overlap'])
    org, lattice = R.origins_of(vol.shape, P, stride)
    nz = np.array([np.count_nonzero(vol[i:i + P, j:j + P, k:k + P]) for i, j, k in org], dtype=np.float64)
    keep = nz / float(P ** 3) >= nonzero_ratio                                            # data.py:187-191
    slot = np.full(org.shape[0], -1, dtype=np.int64)
    slot[keep] = np.arange(int(keep.sum()))
    return dict(P=P, sub=sub, block=block, stride=stride, kept=org[keep], slot=slot.reshape(lattice),
                windows_per_voxel=math.ceil(P / stride) ** 3)


def joint_step(y, slot, taps, stride, x_t, kx, k0, kn, clamp, n):
    """What ``diqt_volume_joint_step`` computes, in float64: (x_next, x0_out, covered).  y [N,P,P,P]; n the normals [D,H,W]."""
    x0, _, covered, _ = R.blend_accumulate(clamp(np.asarray(y, dtype=np.float64))[None], slot, taps, stride, x_t.shape)
    x0 = np.where(covered, x0, 0.0)
    step = kx * x_t + k0 * x0
    if kn != 0:
        step = step + kn * n
    return np.where(covered, step, x_t), x0, covered


def dynamic_threshold_rows(pred, q, floor):
    """Per batch row: s = max(quantile(|x0|, q), floor), clip(x0, -s, s) / s -- the fp32 rank arithmetic of torch.quantile, as
    ``anchored_noise_reference.ddim_reference_loop`` has it."""
    B = pred.shape[0]
    flat = np.sort(np.abs(pred).reshape(B, -1), axis=1)
    rank = np.float32(q) * np.float32(flat.shape[1] - 1)
    k = int(np.floor(rank))
    w = np.float64(np.float32(rank - np.float32(k)))
    s = flat[:, k] + w * (flat[:, min(k + 1, flat.shape[1] - 1)] - flat[:, k])
    s = np.maximum(s, floor).reshape((B,) + (1,) * (pred.ndim - 1))
    return np.clip(pred, -s, s) / s


def joint_chain(vol, cfg, net, tabs, objective, clamp, blend, seed=SEED, sample=0, dyn=None, self_cond=False):
    """One sample's joint chain in float64, before the finish.  ``net(x, lowres, log_snr_rows, self_cond)`` is the network in float64 on
    [B,1,A,A,A] rows; ``tabs`` = ``tables(...)``; ``clamp`` = (lo, hi, mode) of the step (ignored under ``dyn`` = (q, floor), where
    every row is thresholded by its own quantile instead).  Returns the final state [D,H,W] and the layout."""
    vol = np.asarray(vol, dtype=np.float32)
    L = layout(vol, cfg)
    P, stride, kept, slot = L['P'], L['stride'], L['kept'], L['slot']
    mean32, std32 = np.float32(cfg['Data']['mean']), np.float32(cfg['Data']['std'])
    low = ((vol - mean32) / std32).astype(np.float64)                                    # fp32 normalisation, widened
    taps = R.taps_of(P, blend)
    coefs, x0c, log_snr = tabs
    c = clamp_of(-np.inf, np.inf, 1) if dyn is not None else clamp_of(*clamp)
    cut = lambda a, o: a[o[0]:o[0] + P, o[1]:o[1] + P, o[2]:o[2] + P][None, None]
    rows = (lambda w: R.split_block(w, L['sub'])) if L['block'] else (lambda w: w)
    x = normals(vol.shape, seed, 0, sample).copy()
    x0_vol = None
    y = np.empty((kept.shape[0], P, P, P), dtype=np.float64)
    for i in range(coefs.shape[0]):
        for r, o in enumerate(kept):
            xw, lw = rows(cut(x, o)), rows(cut(low, o))
            sc = rows(cut(x0_vol, o)) if self_cond and x0_vol is not None else None
            pred = net(xw, lw, np.full(xw.shape[0], log_snr[i]), sc)
            if objective != 'x_start':
                pred = x0c[i, 0] * xw + x0c[i, 1] * pred
            if dyn is not None:
                pred = dynamic_threshold_rows(pred, *dyn)
            y[r] = (R.merge_block(pred, P) if L['block'] else pred).reshape(P, P, P)
        kn = coefs[i, 2]
        n = normals(vol.shape, seed, i + 1, sample) if kn != 0 else None
        x, x0_vol, _ = joint_step(y, slot, taps, stride, x, coefs[i, 0], coefs[i, 1], kn, c, n)
    return x, L


def joint_reference(vol, cfg, net, tabs, objective, clamp, blend, seed=SEED, samples=1, dyn=None, self_cond=False):
    """``VolumeInference(cfg, denoiser, blend=blend, noise='anchored', joint=True, samples=samples, seed=seed)(vol, return_std=samples > 1)``
    in float64.  ``clamp`` = (lo, hi, mode) is the static clamp of the data normalisation: the step's clamp unless ``dyn``, and the final
    clamp always.  Returns a dict: mean, std, covered, background, fill, min_val, windows_per_voxel, scale (largest |value| compared)."""
    vol = np.asarray(vol, dtype=np.float32)
    mean32, std32 = np.float32(cfg['Data']['mean']), np.float32(cfg['Data']['std'])
    fill, min_val = (np.float32(0.) - mean32) / std32, (vol.min() - mean32) / std32
    finals = []
    for s in range(samples):
        x, L = joint_chain(vol, cfg, net, tabs, objective, clamp, blend, seed, s, dyn, self_cond)
        finals.append(clamp_of(*clamp)(x))
    covered = R.blend_accumulate(np.zeros((1, L['kept'].shape[0], L['P'], L['P'], L['P'])), L['slot'], np.ones(L['P']), L['stride'],
                                 vol.shape)[2]
    background = ((vol - mean32) / std32) == np.float32(min_val)                          # background_reset_kernel's expression
    r = np.stack([np.where(background, np.float64(min_val), np.where(covered, f, np.float64(fill))) for f in finals])
    std = r.std(axis=0, ddof=1) if samples > 1 else np.zeros(vol.shape)
    return dict(mean=r.mean(axis=0), std=std, covered=covered, background=background, fill=fill, min_val=min_val,
                windows_per_voxel=L['windows_per_voxel'], scale=float(np.abs(r).max()), kept=L['kept'].shape[0],
                candidates=L['slot'].size)


def chain_bound(windows_per_voxel, scale, steps=STEPS):
    """Per step the sampler's 8 fp32 operations (tests/test_gpu_ddim.py) plus the blend's n + 3 summation terms
    (``volume_blend_reference.tolerance``), each 2^-23 of the largest magnitude compared."""
    return steps * (8 + windows_per_voxel + 3) * 2.0 ** -23 * scale


# ---- the stand-in networks ------------------------------------------------------------------------------------------------------------
def stub64(x, lowres, log_snr, self_cond=None):
    return A.stub_net64(x, lowres, log_snr)


def self_cond_stub64(x, lowres, log_snr, self_cond=None):
    """``stub_net64`` + 0.125 self_cond (zeros on the first step)."""
    out = A.stub_net64(x, lowres, log_snr)
    return out if self_cond is None else out + 0.125 * np.asarray(self_cond, dtype=np.float64)


def make_self_cond_unet():
    """``self_cond_stub64`` as the module ``Imagen`` samples from."""
    import torch

    class SelfCondStubUnet(torch.nn.Module):
        lowres_cond = True
        self_cond = True

        def cast_model_parameters(self, **kwargs):
            return self

        def forward_with_cond_scale(self, x, time_steps, log_snr, *, lowres_cond_img=None, self_cond=None, **kwargs):
            out = 0.5 * (x / (1.0 + x.abs())) + 0.25 * lowres_cond_img + 0.015625 * log_snr.view(-1, 1, 1, 1, 1)
            return out if self_cond is None else out + 0.125 * self_cond

    return SelfCondStubUnet()
