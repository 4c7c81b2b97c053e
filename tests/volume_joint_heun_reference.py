"""Float64 specification of the EDM branch of ``diffusioniqt_amd.inference.VolumeInference(joint=True)`` in plain numpy: the stochastic
Heun sampler of ``ElucidatedImagen.one_unet_sample`` (churn, predictor, corrector; two evaluations per step) on ONE noisy state of the
whole volume, the kept windows' predictions fused per voxel with the blend weights after each evaluation.  Layout, blend, normals and
dynamic thresholding are ``volume_blend_reference`` / ``volume_joint_reference``'s; the network is the elementwise stub below inside the
EDM preconditioning (c_in, c_skip, c_out, c_noise -- the fp32 numbers the device holds, widened).  Not a test module: the host and GPU
tests of the EDM volume path import it, with the shared inputs and the derived bound.

Draw numbering of the anchored field (``AnchoredNoise.source`` handed to ``ElucidatedImagen.sample``): draw 0 is the low-res augmentation
noise (channel 0 at the window's voxels), draw 1 the initial image, draw 2 + i the eps of step i.

``chain_bound`` -- no constant is chosen, every term is a rounding count.  u = 2^-24; eps_n = 5e-6 is the distance of a device normal
from the float64 transform of the same bits (derived in tests/test_gpu_anchored_noise.py::test_normals_match_the_float64_transform); M
is the largest |state| of the float64 chain, 6 bounds |n|, the fused predictions are clamped to |y| <= 1.  An update sum_j k_j v_j of
t terms costs at most u t sum_j |k_j| max|v_j| (t products, t - 1 sums, one rounding each, fewer where the device fuses).
  * denoiser at sigma, D = clamp(c_skip x + c_out F(c_in x, lowres', c_noise, self_cond)), F the stub with |F'| <= 1/2 in x and 1/8 in
    self_cond: Lipschitz constant L = c_skip + c_out c_in / 2 in the state and c_out / 8 in the self-conditioning volume; the clamp is
    1-Lipschitz; dynamic thresholding clip(x, -s, s) / s with s = max(quantile, 1) moves by at most 2 e under a perturbation e of every
    element (|clip(x', s') - clip(x, s)| <= e and |1/s' - 1/s| <= e / (s s')), so L doubles there;
  * its local fp32 error: the product c_in x (u c_in M, through F and c_out: c_out c_in M u / 2), the stub's own operations (1 + |x|, the
    quotient, three sums: at most 8 roundings of values <= Fmax = 1/2 + max|lowres'| / 4 + |c_noise| / 64 + 1/8), the two-term update
    c_skip x + c_out F, and the noised low-res window alpha l + sigma n (three roundings and sigma eps_n) through F's 1/4 and c_out;
    thresholding doubles it and adds 4 u (the interpolated quantile, the clip and the division on values <= 1);
  * a fused prediction adds the blend's (n + 3) 2^-23 max|y| (``volume_blend_reference.tolerance``) with max|y| = 1;
  * initial image and churn: (sigma0 + kc_0) eps_n + u (sigma0 6 + 2 (sigma0 6 + kc_0 6));
  * predictor xn = a xh + b x0:  e_n = |a| e_h + |b| e_0 + 2 u (|a| M + |b|), with e_0 = L e_h + (c_out / 8) e_sc + local;
  * corrector x = a xh + b x0 + c xn + d x0b:  e_x = |a| e_h + |b| e_0 + |c| e_n + |d| e_0b + 4 u ((|a| + |c|) M + |b| + |d|), with
    e_0b = L' e_n + (c_out' / 8) e_0 + local';  next churn: e_h' = e_x + kc eps_n + 2 u (M + 6 kc).
Unrolled, this recursion is the sum over the steps of the local errors, each multiplied by the gains (|a| + |b| L, |c| + |d| L', ...) of
the steps after it; the bound is its value at the end of the chain (the final clamp is 1-Lipschitz).
"""
import math

import numpy as np

from tests import volume_blend_reference as R
from tests import volume_joint_reference as J

SEED = J.SEED
EPS_N = 5e-6
U = 2.0 ** -24
# a mild schedule: successive sigmas within a factor ~1.7, so |r2| = |sigma_next - sigma_hat| / (2 sigma_next) stays below 1 and the
# product of the steps' gains, which multiplies every local error in ``chain_bound``, stays small beside the signal also under dynamic
# thresholding with the default churn (sigma_max 2 / sigma_min 0.2 put that case's bound at 1.3e-3 of the peak-to-peak, above the 1e-3
# tests/test_volume_joint_heun_host.py asks for)
HP = dict(num_sample_steps=4, sigma_min=0.3, sigma_max=1.5, sigma_data=0.5, rho=7, S_tmin=0.05, S_tmax=50, S_noise=1.003)
CHURN = {'churn-off': 0, 'churn-on': 80}                      # S_churn: none, and the default (gamma = sqrt(2) - 1 on every step here)
PERCENTILE = 0.95
LOWRES_LEVEL = 0.2


# ---- the stand-in network ---------------------------------------------------------------------------------------------------------------
def stub64(x, lowres, c_noise, self_cond=None):
    """F(x, noised low-res, c_noise, self_cond) = x / (2 (1 + |x|)) + lowres / 4 + c_noise / 64 (+ self_cond / 8) per batch row, in the
    dtype of ``x``: elementwise, the scalings are powers of two."""
    dt = x.dtype
    cn = np.asarray(c_noise, dtype=dt).reshape((x.shape[0],) + (1,) * (x.ndim - 1))
    out = dt.type(0.5) * (x / (dt.type(1.0) + np.abs(x))) + dt.type(0.25) * lowres + dt.type(0.015625) * cn
    return out if self_cond is None else out + dt.type(0.125) * self_cond


def make_stub_unet(self_cond=False):
    """``stub64`` as a module ``ElucidatedImagen`` accepts: a ``Unet`` subclass whose ``__init__`` runs only ``nn.Module.__init__``."""
    import torch
    from diffusioniqt_amd.imagen_pytorch3D import Unet

    class EDMStubUnet(Unet):
        lowres_cond = True

        def __init__(self, self_cond):
            torch.nn.Module.__init__(self)
            self.self_cond = self_cond
            self.dummy_parameter = torch.nn.Parameter(torch.tensor([0.]))

        def cast_model_parameters(self, **kwargs):
            return self

        def forward_with_cond_scale(self, x, c_noise, *, lowres_cond_img=None, self_cond=None, **kwargs):
            out = 0.5 * (x / (1.0 + x.abs())) + 0.25 * lowres_cond_img + 0.015625 * c_noise.view(-1, 1, 1, 1, 1)
            return out if self_cond is None else out + 0.125 * self_cond

    return EDMStubUnet(bool(self_cond))


def make_elucidated(churn, dynamic, self_cond=False, size=16, unet=None, **hp):
    """``ElucidatedImagen`` (NullUnet, stub or ``unet``) with the test schedule, on the CPU; no image normalisation (the volume is
    z-scored already)."""
    from diffusioniqt_amd.elucidated_imagen import ElucidatedImagen
    from diffusioniqt_amd.imagen_pytorch3D import NullUnet
    kw = {**HP, 'S_churn': CHURN[churn], **hp}
    return ElucidatedImagen(unets=(NullUnet(), unet if unet is not None else make_stub_unet(self_cond)), image_sizes=(size, size), channels=1,
                            condition_on_text=False, auto_normalize_img=False, cond_drop_prob=0.0, dynamic_thresholding=dynamic,
                            dynamic_thresholding_percentile=PERCENTILE, lowres_sample_noise_level=LOWRES_LEVEL, **kw)


# ---- host tables, computed here independently of the product --------------------------------------------------------------------------
def tables(hp, churn_S):
    """The chain's host numbers as the device holds them (fp32 where the product rounds to fp32, widened): a dict with sched [T,3] =
    (sigma, sigma_next, gamma), sigma0, coefs [T,7] = (kc, 1 + r, -r, 1 + r/2, -r/2, r2, -r2), per step and stage the preconditioning
    scalars pre[T][2] = (sigma_eval, c_in, c_skip, c_out, c_noise), and the low-res q_sample pair (alpha, sigma)."""
    import torch
    from diffusioniqt_amd.imagen_pytorch3D import GaussianDiffusionContinuousTimes, log_snr_to_alpha_sigma
    N, inv_rho = hp['num_sample_steps'], 1 / hp['rho']
    steps = torch.arange(N, dtype=torch.float32)                                        # elucidated_imagen.py:365-379
    sigmas = (hp['sigma_max'] ** inv_rho + steps / (N - 1) * (hp['sigma_min'] ** inv_rho - hp['sigma_max'] ** inv_rho)) ** hp['rho']
    sigmas = torch.cat((sigmas, torch.zeros(1)))
    gammas = torch.where((sigmas >= hp['S_tmin']) & (sigmas <= hp['S_tmax']), min(churn_S / N, math.sqrt(2) - 1), 0.)   # :418-422
    sched = [(float(s), float(sn), float(g)) for s, sn, g in zip(sigmas[:-1], sigmas[1:], gammas[:-1])]
    sd = hp['sigma_data']
    coefs, pre = [], []
    for sigma, sigma_next, gamma in sched:
        sigma_hat = sigma + gamma * sigma
        r = (sigma_next - sigma_hat) / sigma_hat
        r2 = 0.5 * (sigma_next - sigma_hat) / sigma_next if sigma_next != 0 else 0.0
        coefs.append([hp['S_noise'] * math.sqrt(max(sigma_hat ** 2 - sigma ** 2, 0.0)), 1.0 + r, -r, 1.0 + 0.5 * r, -0.5 * r, r2, -r2])
        row = []
        for s_eval in (sigma_hat, sigma_next):
            sig = torch.full((1,), float(s_eval))                                        # fp32, as preconditioned_network_forward has it
            row.append((float(s_eval), float(1 * (sig ** 2 + sd ** 2) ** -0.5), float((sd ** 2) / (sig ** 2 + sd ** 2)),
                        float(sig * sd * (sd ** 2 + sig ** 2) ** -0.5), float(torch.log(sig.clamp(min=1e-20)) * 0.25)))
        pre.append(row)
    log_snr = GaussianDiffusionContinuousTimes(noise_schedule='linear').log_snr(torch.full((1,), float(LOWRES_LEVEL)))
    alpha, sigma_lr = (float(v) for v in log_snr_to_alpha_sigma(log_snr))
    return dict(sched=np.array(sched, dtype=np.float64), sigma0=float(sigmas[0]), pre=pre, lowres=(alpha, sigma_lr),
                coefs=np.array(coefs, dtype=np.float64).astype(np.float32).astype(np.float64))


# ---- the chain ----------------------------------------------------------------------------------------------------------------------------
def fuse(y, slot, taps, stride, shape, dtype=np.float64):
    """The fused prediction of one evaluation: (x0 [D,H,W] with 0 where uncovered, covered).  float64: ``blend_accumulate``; another
    dtype: the same walk with every product and sum in that dtype (the fp32 emulation)."""
    if dtype == np.float64:
        x0, _, covered, _ = R.blend_accumulate(y[None], slot, taps, stride, shape)
        return np.where(covered, x0, 0.0), covered
    P = y.shape[1]
    t = np.asarray(taps, dtype=dtype)
    w3 = (t[:, None, None] * t[None, :, None]) * t[None, None, :]
    num, den = np.zeros(shape, dtype=dtype), np.zeros(shape, dtype=dtype)
    for g in np.ndindex(*slot.shape):
        n = int(slot[g])
        if n >= 0:
            sl = tuple(slice(a * stride, a * stride + P) for a in g)
            num[sl] += w3 * y[n]
            den[sl] += w3
    covered = den > 0
    return np.where(covered, num / np.where(covered, den, dtype(1)), dtype(0)), covered


def heun_phase1(x0, covered, xh, a, b):
    """Phase 1 of ``diqt_volume_joint_heun`` after the walk: (xn, x0)."""
    return np.where(covered, a * xh + b * x0, xh), x0


def heun_phase2(x0b, covered, xh, xn, x0, coefs, kc, n):
    """Phase 2 after the walk: (xh, x0) with x = (a xh + b x0 + c xn) + d x0b and xh = x + kc n on covered voxels."""
    a, b, c, d = coefs
    x = (a * xh + b * x0 + c * xn) + d * x0b
    if kc != 0:
        x = x + kc * n
    return np.where(covered, x, xh), x0b


def joint_chain(vol, cfg, tabs, blend, dynamic, seed=SEED, sample=0, self_cond=False, dtype=np.float64, net=stub64):
    """One sample's joint Heun chain, before the finish, in ``dtype`` (float64: the specification; float32: the emulation of the device
    arithmetic on the same inputs).  Returns the final state [D,H,W], the layout and the largest |state| met on covered voxels."""
    dt = np.dtype(dtype).type
    vol = np.asarray(vol, dtype=np.float32)
    L = J.layout(vol, cfg)
    P, sub, stride, kept, slot = L['P'], L['sub'], L['stride'], L['kept'], L['slot']
    mean32, std32 = np.float32(cfg['Data']['mean']), np.float32(cfg['Data']['std'])
    shape = vol.shape
    alpha, sigma_lr = (dt(v) for v in tabs['lowres'])
    normal = lambda k: J.normals(shape, seed, k, sample).astype(dtype)
    low = alpha * ((vol - mean32) / std32).astype(dtype) + sigma_lr * normal(0)         # elementwise, so noised once for the volume
    taps = R.taps_of(P, blend)
    coefs, pre = tabs['coefs'], tabs['pre']
    T = coefs.shape[0]
    cut = lambda a, o: a[o[0]:o[0] + P, o[1]:o[1] + P, o[2]:o[2] + P][None, None]
    rows = (lambda w: R.split_block(w, sub)) if L['block'] else (lambda w: w)
    y = np.empty((kept.shape[0], P, P, P), dtype=dtype)
    state_max = 0.0

    def evaluate(state, i, stage, sc_vol):
        _, cin, cskip, cout, cnoise = (dt(v) for v in pre[i][stage])
        for r, o in enumerate(kept):
            xw, lw = rows(cut(state, o)), rows(cut(low, o))
            sc = rows(cut(sc_vol, o)) if self_cond and sc_vol is not None else None
            pred = cskip * xw + cout * net(cin * xw, lw, np.full(xw.shape[0], cnoise), sc)
            pred = J.dynamic_threshold_rows(pred, PERCENTILE, 1.0).astype(dtype) if dynamic else np.clip(pred, dt(-1), dt(1))
            y[r] = (R.merge_block(pred, P) if L['block'] else pred).reshape(P, P, P)
        return fuse(y, slot, taps, stride, shape, dtype)

    xh = dt(tabs['sigma0']) * normal(1)
    if coefs[0, 0] != 0:
        xh = xh + dt(coefs[0, 0]) * normal(2)
    x0 = None
    for i in range(T):
        kc, a1, b1, a2, b2, c2, d2 = (dt(v) for v in coefs[i])
        x0, covered = evaluate(xh, i, 0, x0)
        xn, x0 = heun_phase1(x0, covered, xh, a1, b1)
        state_max = max(state_max, float(np.abs(xh[covered]).max()), float(np.abs(xn[covered]).max()))
        if tabs['sched'][i, 1] == 0:
            return xn, L, state_max
        x0b, covered = evaluate(xn, i, 1, x0)
        kc_next = dt(coefs[i + 1, 0]) if i + 1 < T else dt(0)
        xh, x0 = heun_phase2(x0b, covered, xh, xn, x0, (a2, b2, c2, d2), kc_next, normal(3 + i) if kc_next != 0 else None)
    return xh, L, state_max


def joint_reference(vol, cfg, tabs, blend, dynamic, seed=SEED, samples=1, self_cond=False, dtype=np.float64):
    """``VolumeInference(cfg, elu.window_denoiser(), blend=blend, noise='anchored', joint=True, samples=samples, seed=seed)(vol,
    return_std=samples > 1)``: the chains, clamp(-1, 1), fill, background, mean / deviation over the samples.  Returns a dict like
    ``volume_joint_reference.joint_reference``'s, plus ``state_max``, ``lowres_max`` and the ``bound`` of the case."""
    vol = np.asarray(vol, dtype=np.float32)
    mean32, std32 = np.float32(cfg['Data']['mean']), np.float32(cfg['Data']['std'])
    fill, min_val = (np.float32(0.) - mean32) / std32, (vol.min() - mean32) / std32
    finals, state_max = [], 0.0
    for s in range(samples):
        x, L, m = joint_chain(vol, cfg, tabs, blend, dynamic, seed, s, self_cond, dtype)
        finals.append(np.clip(x.astype(np.float64), -1.0, 1.0))
        state_max = max(state_max, m)
    covered = R.blend_accumulate(np.zeros((1, L['kept'].shape[0], L['P'], L['P'], L['P'])), L['slot'], np.ones(L['P']), L['stride'],
                                 vol.shape)[2]
    background = ((vol - mean32) / std32) == np.float32(min_val)                          # background_reset_kernel's expression
    r = np.stack([np.where(background, np.float64(min_val), np.where(covered, f, np.float64(fill))) for f in finals])
    std = r.std(axis=0, ddof=1) if samples > 1 else np.zeros(vol.shape)
    lowres_max = tabs['lowres'][0] * float(np.abs((vol - mean32) / std32).max()) + 6 * tabs['lowres'][1]
    return dict(mean=r.mean(axis=0), std=std, covered=covered, background=background, fill=fill, min_val=min_val,
                windows_per_voxel=L['windows_per_voxel'], kept=L['kept'].shape[0], candidates=L['slot'].size, state_max=state_max,
                lowres_max=lowres_max,
                bound=chain_bound(tabs, L['windows_per_voxel'], state_max, lowres_max, dynamic, self_cond))


def chain_bound(tabs, windows_per_voxel, state_max, lowres_max, dynamic=False, self_cond=False):
    """The recursion of the module docstring, evaluated at the end of the chain."""
    M, coefs, pre = state_max, tabs['coefs'], tabs['pre']
    alpha, sigma_lr = tabs['lowres']
    blend = R.tolerance(windows_per_voxel, 1.0)
    k = 2.0 if dynamic else 1.0

    def denoiser(i, stage):
        """(Lipschitz constant in the state, in the self-conditioning volume, local error) of one fused evaluation."""
        _, cin, cskip, cout, cnoise = pre[i][stage]
        fmax = 0.5 + 0.25 * lowres_max + abs(cnoise) / 64 + 0.125
        local = U * (0.5 * cout * cin * M + 8 * cout * fmax + 2 * (cskip * M + cout * fmax)) \
            + 0.25 * cout * (3 * U * lowres_max + sigma_lr * EPS_N)
        local = k * local + (4 * U if dynamic else 0.0)
        return k * (cskip + 0.5 * cout * cin), (k * cout / 8 if self_cond else 0.0), local + blend

    kc0, s0 = abs(coefs[0, 0]), tabs['sigma0']
    e_h = (s0 + kc0) * EPS_N + U * (6 * s0 + 2 * (6 * s0 + 6 * kc0))
    e_sc = 0.0                                                                            # the error of the volume self-conditioning reads
    for i in range(coefs.shape[0]):
        _, a1, b1, a2, b2, c2, d2 = np.abs(coefs[i])
        L0, S0, local0 = denoiser(i, 0)
        e_0 = L0 * e_h + S0 * e_sc + local0
        e_n = a1 * e_h + b1 * e_0 + 2 * U * (a1 * M + b1)
        if tabs['sched'][i, 1] == 0:
            return e_n
        L1, S1, local1 = denoiser(i, 1)
        e_0b = L1 * e_n + S1 * e_0 + local1
        kc = abs(coefs[i + 1, 0]) if i + 1 < coefs.shape[0] else 0.0
        e_h = a2 * e_h + b2 * e_0 + c2 * e_n + d2 * e_0b + 4 * U * ((a2 + c2) * M + b2 + d2) + kc * EPS_N + 2 * U * (M + 6 * kc)
        e_sc = e_0b
    return e_h
