"""Float64 specification of ``ElucidatedImagen(sampler='dpmpp2m')`` in plain numpy: DPM-Solver++ 2M in sigma space, ODE (eta = 0) and
midpoint SDE (eta > 0) -- the coefficient table written from its formulas, the per-window loop of ``one_unet_sample``, one joint step
(``diqt_volume_joint_multistep_sde``) and the joint chain of ``VolumeInference(joint=True)``, the analytic Gaussian problem on which the
solver's order and the SDE's variance are measured, and a rounding bound.  Layout, blend, normals, the stub network, the EDM
preconditioning and dynamic thresholding are ``volume_joint_heun_reference``'s.  Not a test module: the host and GPU tests import it.

Draw numbering of the anchored field, as the Heun path numbers it: draw 0 the low-res augmentation noise, draw 1 the initial image,
draw 2 + i the normal of step i (used only where kn != 0).

``chain_bound`` -- built as ``volume_joint_heun_reference.chain_bound`` is; no constant is chosen.  u = 2^-24, eps_n = 5e-6 (a device
normal against the float64 transform of the same bits), M the largest |state| of the float64 chain, |n| <= 6, |D| <= 1.
  * denoiser at sigma_i: ``volume_joint_heun_reference``'s Lipschitz constants (L = c_skip + c_out c_in / 2 in the state, c_out / 8 in
    the self-conditioning volume; both doubled under dynamic thresholding) and its local fp32 error, plus the blend's (n + 3) 2^-23;
  * initial image sigma0 n: sigma0 eps_n + u 6 sigma0 (one product);
  * the update x' = kx x + k0 D + kp D_prev + kn n is allowed 12 fp32 operations per step -- the 10 of ``Imagen``'s multistep step
    (tests/dpmpp2m_reference.chain_bound) plus the noise product and its sum; the update itself rounds 7 times -- each on a value of at
    most S = |kx| M + |k0| + |kp| + 6 |kn|:
        e_x' = |kx| e_x + |k0| e_D + |kp| e_Dprev + |kn| eps_n + 12 u S,   e_D = L e_x + (c_out / 8) e_Dprev + local.
Unrolled, this is the sum over the steps of the local errors, each multiplied by the gains of the steps after it; the bound is its
value at the end of the chain (the final clamp is 1-Lipschitz).
"""
import math

import numpy as np

from tests import volume_blend_reference as R
from tests import volume_joint_heun_reference as HN
from tests import volume_joint_reference as J

SEED = HN.SEED
HP = HN.HP                                  # K = 4, sigma from 1.5 to 0.3
ETAS = {'ode': 0.0, 'sde': 1.0}
OPS_PER_STEP = 12
U, EPS_N = HN.U, HN.EPS_N


# ---- the table --------------------------------------------------------------------------------------------------------------------------
def schedule(hp, steps=None):
    """The fp32 Karras schedule of ``sample_schedule`` (elucidated_imagen.py:365-379) with the closing 0, widened: float64 [T + 1]."""
    import torch
    N, inv_rho = int(steps or hp['num_sample_steps']), 1 / hp['rho']
    t = torch.arange(N, dtype=torch.float32)
    sigmas = (hp['sigma_max'] ** inv_rho + t / (N - 1) * (hp['sigma_min'] ** inv_rho - hp['sigma_max'] ** inv_rho)) ** hp['rho']
    return np.concatenate((sigmas.numpy().astype(np.float64), [0.0]))


def table64(sigmas, eta=0.0, S_noise=1.0):
    """Rows (kx, k0, kp, kn) of x_next = kx x + k0 D_i + kp D_{i-1} + kn n in float64 [T,4], and c [T] (k0 + kp = c).  Per step
    h = log(sigma / sigma'), c = -expm1(-h - eta h), kx = (sigma' / sigma) exp(-eta h), r = h_{i-1} / h_i, k0 = c (1 + 1/(2r)),
    kp = -c / (2r), kn = S_noise sigma' sqrt(-expm1(-2 eta h)).  Row 0: (kx, c, 0, kn).  The row with sigma' = 0: (0, 1, 0, 0)."""
    s = np.asarray(sigmas, dtype=np.float64)
    T = s.shape[0] - 1
    out, cs = np.zeros((T, 4)), np.zeros(T)
    h_prev = None
    for i in range(T):
        if s[i + 1] == 0:
            out[i], cs[i], h_prev = (0.0, 1.0, 0.0, 0.0), 1.0, None
            continue
        h = np.log(s[i] / s[i + 1])
        c = -np.expm1(-h - eta * h)
        k0, kp = c, 0.0
        if h_prev is not None:
            r = h_prev / h
            k0, kp = c * (1 + 1 / (2 * r)), -c / (2 * r)
        out[i] = (s[i + 1] / s[i] * np.exp(-eta * h), k0, kp, S_noise * s[i + 1] * np.sqrt(-np.expm1(-2 * eta * h)))
        cs[i], h_prev = c, h
    return out, cs


def tables(hp, eta, steps=None, coefs=None):
    """The chain's host numbers as the device holds them, widened: sigmas [T + 1], sigma0, coefs [T,4] (``coefs``: the product's fp32
    table; None: ``table64`` rounded to fp32), per step the preconditioning scalars pre[T] = (sigma, c_in, c_skip, c_out, c_noise) in
    fp32 as ``preconditioned_network_forward`` forms them, and the low-res q_sample pair."""
    import torch
    from diffusioniqt_amd.imagen_pytorch3D import GaussianDiffusionContinuousTimes, log_snr_to_alpha_sigma
    sigmas = schedule(hp, steps)
    if coefs is None:
        coefs = table64(sigmas, eta, hp['S_noise'])[0].astype(np.float32)
    sd = hp['sigma_data']
    pre = []
    for s in sigmas[:-1]:
        sig = torch.full((1,), float(s))
        pre.append((float(s), float(1 * (sig ** 2 + sd ** 2) ** -0.5), float((sd ** 2) / (sig ** 2 + sd ** 2)),
                    float(sig * sd * (sd ** 2 + sig ** 2) ** -0.5), float(torch.log(sig.clamp(min=1e-20)) * 0.25)))
    log_snr = GaussianDiffusionContinuousTimes(noise_schedule='linear').log_snr(torch.full((1,), float(HN.LOWRES_LEVEL)))
    alpha, sigma_lr = (float(v) for v in log_snr_to_alpha_sigma(log_snr))
    return dict(sigmas=sigmas, sigma0=float(sigmas[0]), pre=pre, lowres=(alpha, sigma_lr), eta=float(eta),
                coefs=np.asarray(coefs, dtype=np.float32).astype(np.float64))


# ---- the per-window loop ----------------------------------------------------------------------------------------------------------------
def threshold(pred, dynamic, dtype=np.float64):
    dt = np.dtype(dtype).type
    return J.dynamic_threshold_rows(pred, HN.PERCENTILE, 1.0).astype(dtype) if dynamic else np.clip(pred, dt(-1), dt(1))


def update(x, d0, dprev, row, n):
    """x_next = kx x + k0 D + kp D_prev (+ kn n when kn != 0), in the dtype of ``x``."""
    kx, k0, kp, kn = row
    out = kx * x + k0 * d0
    if dprev is not None:
        out = out + kp * dprev
    return out + kn * n if kn != 0 else out


def window_loop(net, init, lowres, tabs, dynamic, step_noise, self_cond=False):
    """``one_unet_sample(sampler='dpmpp2m')`` on one window batch in float64: ``net(x_in, lowres, c_noise [B], self_cond)`` is the raw
    network on the NOISED low-res windows ``lowres``; ``init`` the initial normals; ``step_noise[i]`` the normals of step i (read only
    where kn != 0).  Returns (clip(x, -1, 1), largest |state|)."""
    x = tabs['sigma0'] * np.asarray(init, dtype=np.float64)
    prev, state_max = None, float(np.abs(x).max())
    for i, row in enumerate(tabs['coefs']):
        _, cin, cskip, cout, cnoise = tabs['pre'][i]
        d0 = threshold(cskip * x + cout * net(cin * x, lowres, np.full(x.shape[0], cnoise), prev if self_cond else None), dynamic)
        x = update(x, d0, prev, row, np.asarray(step_noise[i], dtype=np.float64) if row[3] != 0 else None)
        prev = d0
        state_max = max(state_max, float(np.abs(x).max()))
    return np.clip(x, -1.0, 1.0), state_max


# ---- the joint step and chain -----------------------------------------------------------------------------------------------------------
def joint_step(y, slot, taps, stride, x_t, x0_prev, row, clamp, n):
    """What ``diqt_volume_joint_multistep_sde`` computes on a state, in float64: (x_next, x0_out, covered)."""
    x0, _, covered, _ = R.blend_accumulate(clamp(np.asarray(y, dtype=np.float64))[None], slot, taps, stride, x_t.shape)
    x0 = np.where(covered, x0, 0.0)
    return np.where(covered, update(x_t, x0, x0_prev, row, n), x_t), x0, covered


def joint_chain(vol, cfg, tabs, blend, dynamic, seed=SEED, sample=0, self_cond=False, dtype=np.float64, net=HN.stub64):
    """One sample's joint chain, before the finish, in ``dtype`` (float64: the specification; float32: the emulation of the device
    arithmetic).  Returns the final state [D,H,W], the layout and the largest |state| met on covered voxels."""
    dt = np.dtype(dtype).type
    vol = np.asarray(vol, dtype=np.float32)
    L = J.layout(vol, cfg)
    P, sub, stride, kept, slot = L['P'], L['sub'], L['stride'], L['kept'], L['slot']
    mean32, std32 = np.float32(cfg['Data']['mean']), np.float32(cfg['Data']['std'])
    shape = vol.shape
    alpha, sigma_lr = (dt(v) for v in tabs['lowres'])
    normal = lambda k: J.normals(shape, seed, k, sample).astype(dtype)
    low = alpha * ((vol - mean32) / std32).astype(dtype) + sigma_lr * normal(0)
    taps = R.taps_of(P, blend)
    cut = lambda a, o: a[o[0]:o[0] + P, o[1]:o[1] + P, o[2]:o[2] + P][None, None]
    rows = (lambda w: R.split_block(w, sub)) if L['block'] else (lambda w: w)
    y = np.empty((kept.shape[0], P, P, P), dtype=dtype)
    x = dt(tabs['sigma0']) * normal(1)
    x0_vol, covered, state_max = None, None, 0.0
    for i, row in enumerate(tabs['coefs']):
        _, cin, cskip, cout, cnoise = (dt(v) for v in tabs['pre'][i])
        for r, o in enumerate(kept):
            xw, lw = rows(cut(x, o)), rows(cut(low, o))
            sc = rows(cut(x0_vol, o)) if self_cond and x0_vol is not None else None
            pred = threshold(cskip * xw + cout * net(cin * xw, lw, np.full(xw.shape[0], cnoise), sc), dynamic, dtype)
            y[r] = (R.merge_block(pred, P) if L['block'] else pred).reshape(P, P, P)
        x0, covered = HN.fuse(y, slot, taps, stride, shape, dtype)
        state_max = max(state_max, float(np.abs(x[covered]).max()))
        row = tuple(dt(v) for v in row)
        x = np.where(covered, update(x, x0, x0_vol, row, normal(2 + i) if row[3] != 0 else None), x)
        x0_vol = x0
    return x, L, max(state_max, float(np.abs(x[covered]).max()))


def joint_reference(vol, cfg, tabs, blend, dynamic, seed=SEED, samples=1, self_cond=False, dtype=np.float64):
    """``VolumeInference(cfg, elu.window_denoiser(sampler='dpmpp2m', ...), blend=blend, noise='anchored', joint=True, samples=samples,
    seed=seed)(vol, return_std=samples > 1)``: the chains, clamp(-1, 1), fill, background, mean / deviation over the samples, and the
    ``bound`` of the case -- the dict of ``volume_joint_heun_reference.joint_reference``."""
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
    background = ((vol - mean32) / std32) == np.float32(min_val)
    r = np.stack([np.where(background, np.float64(min_val), np.where(covered, f, np.float64(fill))) for f in finals])
    std = r.std(axis=0, ddof=1) if samples > 1 else np.zeros(vol.shape)
    lowres_max = tabs['lowres'][0] * float(np.abs((vol - mean32) / std32).max()) + 6 * tabs['lowres'][1]
    return dict(mean=r.mean(axis=0), std=std, covered=covered, background=background, fill=fill, min_val=min_val,
                windows_per_voxel=L['windows_per_voxel'], kept=L['kept'].shape[0], candidates=L['slot'].size, state_max=state_max,
                lowres_max=lowres_max, bound=chain_bound(tabs, L['windows_per_voxel'], state_max, lowres_max, dynamic, self_cond))


def chain_bound(tabs, windows_per_voxel, state_max, lowres_max, dynamic=False, self_cond=False):
    """The recursion of the module docstring, evaluated at the end of the chain.  ``windows_per_voxel`` 1 and no blend term: pass 0 for a
    per-window loop (nothing is fused there)."""
    M, coefs = state_max, np.abs(tabs['coefs'])
    _, sigma_lr = tabs['lowres']
    blend = R.tolerance(windows_per_voxel, 1.0) if windows_per_voxel else 0.0
    k = 2.0 if dynamic else 1.0
    e_x = tabs['sigma0'] * EPS_N + U * 6 * tabs['sigma0']
    e_prev = 0.0
    for i in range(coefs.shape[0]):
        _, cin, cskip, cout, cnoise = tabs['pre'][i]
        fmax = 0.5 + 0.25 * lowres_max + abs(cnoise) / 64 + 0.125
        local = U * (0.5 * cout * cin * M + 8 * cout * fmax + 2 * (cskip * M + cout * fmax)) \
            + 0.25 * cout * (3 * U * lowres_max + sigma_lr * EPS_N)
        local = k * local + (4 * U if dynamic else 0.0) + blend
        e_d = k * (cskip + 0.5 * cout * cin) * e_x + (k * cout / 8 if self_cond else 0.0) * e_prev + local
        kx, k0, kp, kn = coefs[i]
        e_x = kx * e_x + k0 * e_d + kp * e_prev + kn * EPS_N + OPS_PER_STEP * U * (kx * M + k0 + kp + 6 * kn)
        e_prev = e_d
    return e_x


# ---- the analytic problem -----------------------------------------------------------------------------------------------------------------
DATA_STD = 0.5
KARRAS = dict(sigma_min=0.002, sigma_max=80, rho=7)


def karras64(K, sigma_min=0.002, sigma_max=80.0, rho=7.0):
    """The Karras schedule in float64 with the closing 0: [K + 1]."""
    t = np.arange(K, dtype=np.float64) / (K - 1)
    return np.concatenate(((sigma_max ** (1 / rho) + t * (sigma_min ** (1 / rho) - sigma_max ** (1 / rho))) ** rho, [0.0]))


def gaussian_denoiser(sigma):
    """Data x0 ~ N(0, s^2), s = 0.5: x_sigma ~ N(0, s^2 + sigma^2) and the exact denoiser is linear, D(x, sigma) = g(sigma) x with
    g = s^2 / (s^2 + sigma^2)."""
    return DATA_STD ** 2 / (DATA_STD ** 2 + sigma ** 2)


def gaussian_problem_error(table, sigmas):
    """The probability-flow ODE of that problem has the solution x_sigma = x_0 sqrt(s^2 + sigma^2) / sqrt(s^2 + sigma0^2).  Runs the
    chain of ``table`` [T,4] (kn ignored: the ODE) from one standard deviation out, x = sqrt(s^2 + sigma0^2), with the exact denoiser
    and returns |x - s| at sigma = 0."""
    x, prev = math.sqrt(DATA_STD ** 2 + sigmas[0] ** 2), 0.0
    for i, (kx, k0, kp, _) in enumerate(np.asarray(table, dtype=np.float64)):
        d0 = gaussian_denoiser(sigmas[i]) * x
        x, prev = kx * x + k0 * d0 + kp * prev, d0
    return abs(x - DATA_STD)


def heun_problem_error(sigmas):
    """Deterministic Heun (the EDM sampler with S_churn = 0) on the same problem from the same start: |x - s| at sigma = 0."""
    x = math.sqrt(DATA_STD ** 2 + sigmas[0] ** 2)
    for s, sn in zip(sigmas[:-1], sigmas[1:]):
        d = (x - gaussian_denoiser(s) * x) / s
        xn = x + (sn - s) * d
        if sn != 0:
            d2 = (xn - gaussian_denoiser(sn) * xn) / sn
            xn = x + 0.5 * (sn - s) * (d + d2)
        x = xn
    return abs(x - DATA_STD)


def gaussian_problem_std(table, sigmas):
    """The SDE chain on the same problem, exactly: x_next = (kx + k0 g_i) x + kp d_prev + kn n and d = g_i x are linear in (x, d_prev)
    and the normals are independent, so the covariance C of (x, d_prev) obeys C' = A C A^T + kn^2 e e^T with A = [[kx + k0 g, kp],
    [g, 0]] and e = (1, 0); x starts as N(0, s^2 + sigma0^2) with d_prev = 0.  Returns the standard deviation of x at sigma = 0."""
    C = np.array([[DATA_STD ** 2 + sigmas[0] ** 2, 0.0], [0.0, 0.0]])
    for i, (kx, k0, kp, kn) in enumerate(np.asarray(table, dtype=np.float64)):
        g = gaussian_denoiser(sigmas[i])
        A = np.array([[kx + k0 * g, kp], [g, 0.0]])
        C = A @ C @ A.T
        C[0, 0] += kn ** 2
    return math.sqrt(C[0, 0])
