"""Float64 specification of the second-order multistep sampler ``sampler='dpmpp2m'`` (DPM-Solver++ 2M with a first-order first and
last step) in plain numpy: the coefficient table written from its formulas, the per-window sampling loop
(``anchored_noise_reference.ddim_reference_loop`` plus the history term), one joint step and the joint chain of
``VolumeInference(joint=True)`` (``volume_joint_reference`` with kp x0_prev in place of kn n), and the analytic Gaussian problem on which
the solver's order is measured.  Not a test module: the host and GPU tests of the sampler import it.
"""
import numpy as np

from tests import anchored_noise_reference as A
from tests import volume_blend_reference as R
from tests import volume_joint_reference as J

STEPS = 4                      # of the joint chains: two second-order steps between the two first-order ones


# ---- the table ------------------------------------------------------------------------------------------------------------------------
def chain_log_snr(scheduler, steps):
    """The fp32 log-SNR values of the chain linspace(1, 0, steps + 1) as the network is conditioned on them: (at t_i, at t_i') [T]."""
    pairs = list(scheduler.get_sampling_timesteps(1, device='cpu', steps=steps))
    return (np.array([scheduler.log_snr(t)[0].item() for t, _ in pairs], dtype=np.float32),
            np.array([scheduler.log_snr(tn)[0].item() for _, tn in pairs], dtype=np.float32))


def table64(log_snr, log_snr_next):
    """Rows (kx, k0, kp) of x_next = kx x + k0 x0_i + kp x0_{i-1} in float64 [T,3] from the (fp32) log-SNR values of the chain's pairs.
    lambda = log_snr / 2, h_i = lambda(t_i') - lambda(t_i), r = h_{i-1} / h_i; (kx, k0') = the deterministic DDIM pair.  Rows 0 and
    T - 1: (kx, k0', 0).  Rows between: (kx, k0' (1 + 1/(2r)), -k0'/(2r))."""
    ls, lsn = np.asarray(log_snr, dtype=np.float64), np.asarray(log_snr_next, dtype=np.float64)
    T = ls.shape[0]
    kx, k01, _ = A.ddim_coefficients64(ls, lsn, np.zeros(T), 0.0)
    h = lsn / 2 - ls / 2
    out = np.stack((kx, k01, np.zeros(T)), axis=1)
    for i in range(1, T - 1):
        r = h[i - 1] / h[i]
        out[i, 1] = k01[i] * (1 + 1 / (2 * r))
        out[i, 2] = -k01[i] / (2 * r)
    return out, k01


def amplification(table, k01):
    """c = max_i (|k0| + |kp|) / |k0'|: how much larger the two x0 products of a second-order step are than the one of DDIM."""
    return float(((np.abs(table[:, 1]) + np.abs(table[:, 2])) / np.abs(k01)).max())


# ---- the per-window loop --------------------------------------------------------------------------------------------------------------
def reference_loop(net, init, coefs, x0_coefs, log_snr, objective, lo, hi=None, dyn_q=None, dyn_floor=None):
    """``anchored_noise_reference.ddim_reference_loop`` with the history term: ``coefs`` [T,3,B] rows are (kx, k0, kp) and
    x = kx x + k0 x0_i + kp x0_{i-1}, x0_{-1} = 0, where the history holds the thresholded / clamped x0.  Same returns."""
    x = np.asarray(init, dtype=np.float64)
    B = x.shape[0]
    col = lambda v: np.asarray(v, dtype=np.float64).reshape((B,) + (1,) * (x.ndim - 1))
    clamp = (lambda v: np.maximum(v, lo)) if hi is None else (lambda v: np.clip(v, lo, hi))
    noisy, x0s = [], []
    x0 = prev = np.zeros_like(x)
    for i in range(coefs.shape[0]):
        pred = net(x, np.asarray(log_snr[i], dtype=np.float64))
        if objective != 'x_start':
            pred = col(x0_coefs[i, 0]) * x + col(x0_coefs[i, 1]) * pred
        x0 = J.dynamic_threshold_rows(pred, dyn_q, dyn_floor) if dyn_q is not None else clamp(pred)
        kx, k0, kp = (col(coefs[i, j]) for j in range(3))
        x = kx * x + k0 * x0 + kp * prev
        prev = x0
        noisy.append(x)
        x0s.append(x0)
    noisy.append(x)
    x0s.append(x0)
    return clamp(x), noisy, x0s


# ---- the joint chain ------------------------------------------------------------------------------------------------------------------
def joint_multistep(y, slot, taps, stride, x_t, x0_prev, kx, k0, kp, clamp):
    """What ``diqt_volume_joint_multistep`` computes, in float64: (x_next, x0_out, covered).  ``x0_prev`` None stands for zeros."""
    x0, _, covered, _ = R.blend_accumulate(clamp(np.asarray(y, dtype=np.float64))[None], slot, taps, stride, x_t.shape)
    x0 = np.where(covered, x0, 0.0)
    step = kx * x_t + k0 * x0
    if x0_prev is not None:
        step = step + kp * x0_prev
    return np.where(covered, step, x_t), x0, covered


def tables(scheduler, steps, objective):
    """``volume_joint_reference.tables`` for the multistep chain: the product's fp32 table, widened (coefs [T,3] = (kx, k0, kp))."""
    _, x0c, conds = J.tables(scheduler, steps, 0.0, objective)
    pairs = list(scheduler.get_sampling_timesteps(1, device='cpu', steps=steps))
    coefs = scheduler.dpmpp2m_coefficients(pairs).numpy()[:, :, 0].astype(np.float64)
    return coefs, x0c, conds


def joint_chain(vol, cfg, net, tabs, objective, clamp, blend, seed=J.SEED, sample=0, dyn=None, self_cond=False):
    """``volume_joint_reference.joint_chain`` with ``joint_multistep``: only draw 0 of the field is used."""
    vol = np.asarray(vol, dtype=np.float32)
    L = J.layout(vol, cfg)
    P, stride, kept, slot = L['P'], L['stride'], L['kept'], L['slot']
    mean32, std32 = np.float32(cfg['Data']['mean']), np.float32(cfg['Data']['std'])
    low = ((vol - mean32) / std32).astype(np.float64)
    taps = R.taps_of(P, blend)
    coefs, x0c, log_snr = tabs
    c = J.clamp_of(-np.inf, np.inf, 1) if dyn is not None else J.clamp_of(*clamp)
    cut = lambda a, o: a[o[0]:o[0] + P, o[1]:o[1] + P, o[2]:o[2] + P][None, None]
    rows = (lambda w: R.split_block(w, L['sub'])) if L['block'] else (lambda w: w)
    x = J.normals(vol.shape, seed, 0, sample).copy()
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
                pred = J.dynamic_threshold_rows(pred, *dyn)
            y[r] = (R.merge_block(pred, P) if L['block'] else pred).reshape(P, P, P)
        x, x0_vol, _ = joint_multistep(y, slot, taps, stride, x, x0_vol, coefs[i, 0], coefs[i, 1], coefs[i, 2], c)
    return x, L


def joint_reference(vol, cfg, net, tabs, objective, clamp, blend, seed=J.SEED, samples=1, dyn=None, self_cond=False):
    """``volume_joint_reference.joint_reference`` on ``joint_chain`` above: the same finish and the same dict."""
    vol = np.asarray(vol, dtype=np.float32)
    mean32, std32 = np.float32(cfg['Data']['mean']), np.float32(cfg['Data']['std'])
    fill, min_val = (np.float32(0.) - mean32) / std32, (vol.min() - mean32) / std32
    finals = []
    for s in range(samples):
        x, L = joint_chain(vol, cfg, net, tabs, objective, clamp, blend, seed, s, dyn, self_cond)
        finals.append(J.clamp_of(*clamp)(x))
    covered = R.blend_accumulate(np.zeros((1, L['kept'].shape[0], L['P'], L['P'], L['P'])), L['slot'], np.ones(L['P']), L['stride'],
                                 vol.shape)[2]
    background = ((vol - mean32) / std32) == np.float32(min_val)
    r = np.stack([np.where(background, np.float64(min_val), np.where(covered, f, np.float64(fill))) for f in finals])
    std = r.std(axis=0, ddof=1) if samples > 1 else np.zeros(vol.shape)
    return dict(mean=r.mean(axis=0), std=std, covered=covered, background=background, fill=fill, min_val=min_val,
                windows_per_voxel=L['windows_per_voxel'], scale=float(np.abs(r).max()), kept=L['kept'].shape[0],
                candidates=L['slot'].size)


def chain_bound(windows_per_voxel, scale, c, steps=STEPS):
    """``volume_joint_reference.chain_bound`` with 10 c in place of the sampler's 8: the DDIM step's 8 fp32 operations plus one product
    and one sum, on x0 products up to c times larger (``amplification``)."""
    return steps * (10 * c + windows_per_voxel + 3) * 2.0 ** -23 * scale


# ---- the analytic problem -------------------------------------------------------------------------------------------------------------
DATA_STD = 0.5


def gaussian_problem_error(table, log_snr, log_snr_next):
    """Data x0 ~ N(0, s^2), s = 0.5: x_t ~ N(0, alpha^2 s^2 + sigma^2), the exact predictor is linear, E[x0 | x_t] =
    alpha s^2 / (alpha^2 s^2 + sigma^2) x_t, and the probability-flow ODE has the solution x_t = x_1 std(t) / std(1).  Runs the chain of
    ``table`` [T,3] = (kx, k0, kp) from x_1 = std(1) (one standard deviation out) with that predictor and returns |x - std(t')| at the end
    of the chain, t' = 0."""
    ls, lsn = np.asarray(log_snr, dtype=np.float64), np.asarray(log_snr_next, dtype=np.float64)
    var = lambda l: (lambda a, s: a ** 2 * DATA_STD ** 2 + s ** 2)(*A.alpha_sigma64(l))
    x, prev = np.sqrt(var(ls[0])), 0.0
    for i in range(table.shape[0]):
        alpha, _ = A.alpha_sigma64(ls[i])
        x0 = alpha * DATA_STD ** 2 / var(ls[i]) * x
        x, prev = table[i, 0] * x + table[i, 1] * x0 + table[i, 2] * prev, x0
    return float(abs(x - np.sqrt(var(lsn[-1]))))
