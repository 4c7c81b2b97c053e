"""Specification of noise-aware data consistency (``consistency_noise=`` of the samplers and of ``VolumeInference``; DDNM+, Wang, Yu,
Zhang, ICLR 2023, section 3.3) in plain numpy, on top of tests/volume_joint_dc_reference.py and
tests/volume_joint_profile_reference.py.  Not a test module: tests/test_volume_noise_host.py and tests/test_gpu_volume_noise.py import
it.

The schedule.  A step is x_next = kx x + k0 x0' + kp x0'_prev + kn eps, x0' = x0 + w_i A+(y - A x0).  The measurement is
y = A x + n_y, n_y ~ N(0, sigma_y^2); the cells are disjoint with one profile, so A A^T = s^2 I, s = |u|_2 (1 / sqrt(n) for the plain
mean) and A+ n_y has the deviation sigma_y / s in the range of A.  x0' carries w_i A+ n_y and the history term w_{i-1} A+ n_y of the
SAME n_y, so the measurement noise enters x_next with the deviation |a_i| sigma_y / s, a_i = k0 w_i + kp w_{i-1}.  DDNM+ keeps the
step's variance in the range of A at kn^2: (a_i sigma_y / s)^2 + (rho_i kn)^2 = kn^2.  ``schedule64`` restates the rule in float64,
independently of ``ops.consistency_noise_schedule``: w_{-1} = 0; kn == 0: w_i = 0; else b = kn s / sigma_y,
w_i = min(w, max(0, (b - kp w_{i-1}) / k0)), a_i = k0 w_i + kp w_{i-1}, rho_i = sqrt(max(0, 1 - (a_i / b)^2)), shrink_i = 1 - rho_i.

The shaping.  eps' = eps - shrink g (u . eps) on a cell whose voxels are all covered: Phi = I - shrink g u^T has u^T Phi = rho u^T
(u . g = 1), so u . eps' = rho (u . eps) and the null space of A is untouched.  In the project's arithmetic it IS the projection of
the normals onto a zero measurement with weight = shrink, so the fp32 restatements are calls of the existing ones --
``volume_joint_dc_reference.project32`` / ``volume_joint_profile_reference.project_profile32`` -- whose fma emulation is checked
against exact rationals in tests/test_volume_profile_host.py.  Nothing is restated here but the order of the calls.

The normals.  The float64 chains take the anchored field of tests/anchored_noise_reference.py (``volume_joint_reference.normals``).
The bit-exact step tests hand the step's fp32 normals in: the device evaluates Box-Muller in fp32, which that float64 module
specifies to 5e-6 only, so the GPU test takes them from ``ops.volume_joint_init`` and asserts that distance.

Rounding count of one shaping: the projection's own count with weight = shrink and S = max |eps| (``shaping_roundings``); it enters
the update multiplied by kn.  ``vp_bound`` / ``edm_bound`` are the uniform and profile chain bounds plus that, nothing tuned.
"""
import math

import numpy as np

from tests import edm_dpmpp2m_reference as E
from tests import volume_blend_reference as R
from tests import volume_joint_dc_reference as DC
from tests import volume_joint_heun_reference as HN
from tests import volume_joint_profile_reference as PR
from tests import volume_joint_reference as J
from tests.volume_joint_dc_reference import _cells, clamp32, fma32, fuse32, replicate     # noqa: F401  (the tests take them from here)

PROFILE_222 = ((1, 2), (1, 1), (3, 0))                      # the profile of the schedule tests: one gap voxel pair along x


# ---- the schedule, float64 ------------------------------------------------------------------------------------------------------------------
def cell_norm64(cell, table=None):
    """s = |u|_2: 1 / sqrt(n), or sqrt(sum u^2) over the table's fp32 weights, widened and summed in sequence."""
    n = cell[0] * cell[1] * cell[2]
    if table is None:
        return 1.0 / math.sqrt(n)
    sq = 0.0
    for v in np.asarray(table[0], dtype=np.float32):
        sq += float(v) * float(v)
    return math.sqrt(sq)


def schedule64(rows, s, sigma_y, w):
    """float64 [T, 2] = (w_i, shrink_i) of rows (kx, k0, kp, kn) (module docstring)."""
    out, w_prev = np.zeros((len(rows), 2)), 0.0
    for i, (kx, k0, kp, kn) in enumerate(np.asarray(rows, dtype=np.float64).tolist()):
        if kn == 0.0:
            w_prev = 0.0
            continue
        assert k0 > 0.0
        b = kn * s / sigma_y
        w_i = min(w, max(0.0, (b - kp * w_prev) / k0))
        a = k0 * w_i + kp * w_prev
        out[i] = w_i, 1.0 - math.sqrt(max(0.0, 1.0 - (a / b) ** 2))
        w_prev = w_i
    return out


def dispatch(sched):
    """The schedule as the chains dispatch on it: rounded to fp32, widened."""
    return np.asarray(sched, dtype=np.float64).astype(np.float32).astype(np.float64)


def rows4(coefs):
    """[T, 3] rows (kx, k0, kn) of a first-order table as (kx, k0, 0, kn); [T, 4] rows as they are."""
    c = np.asarray(coefs, dtype=np.float64)
    return c if c.shape[1] == 4 else np.stack((c[:, 0], c[:, 1], np.zeros(len(c)), c[:, 2]), axis=1)


# ---- fp32 -----------------------------------------------------------------------------------------------------------------------------------
def shape_noise32(eps, cell, table, shrink, covered=None):
    """eps' in float32: the existing projection of ``eps`` onto a zero measurement with weight ``shrink``; ``covered``: only cells
    whose voxels are all covered are shaped."""
    eps = np.asarray(eps, dtype=np.float32)
    zero = np.zeros(eps.shape, dtype=np.float32)
    if table is None:
        return DC.project32(eps, zero, cell, shrink, covered)
    return PR.project_profile32(eps, zero, cell, table, shrink, covered)


def project32(a, meas_up, cell, table, w, covered=None):
    return DC.project32(a, meas_up, cell, w, covered) if table is None else PR.project_profile32(a, meas_up, cell, table, w, covered)


def project_noise32(x0, meas_up, eps, cell, table, w, shrink, clamp):
    """What ``diqt_cell_project_noise`` computes, bit for bit: (x0', eps'); ``clamp`` = (lo, hi, mode) or None."""
    a = clamp32(*(clamp or (0., 0., None)))(np.asarray(x0, dtype=np.float32))
    return project32(a, meas_up, cell, table, w), shape_noise32(eps, cell, table, shrink)


def joint_step_noise32(y, slot, taps, stride, x_t, x0_prev, meas_up, cell, table, w, shrink, form, kx, k0, kp, kn, clamp, n, fused=None):
    """What ``diqt_volume_joint_consistent_noise_step`` computes, bit for bit: (x_next, x0_out, covered) -- the consistent step of the
    two modules above with the step's float32 normals ``n`` shaped on the cells whose voxels are all covered.  Forms 0 and 2, kn != 0."""
    assert form in (0, 2) and kn != 0
    x0, covered = fused if fused is not None else fuse32(y, slot, taps, stride, np.asarray(x_t).shape, clamp)
    shaped = shape_noise32(n, cell, table, shrink, covered)
    if table is None:
        return DC.joint_step32(y, slot, taps, stride, x_t, x0_prev, meas_up, cell, w, form, kx, k0, kp, kn, clamp, shaped,
                               fused=(x0, covered))
    return PR.joint_step_profile32(y, slot, taps, stride, x_t, x0_prev, meas_up, cell, table, w, form, kx, k0, kp, kn, clamp, shaped,
                                   fused=(x0, covered))


# ---- float64 --------------------------------------------------------------------------------------------------------------------------------
def project64(x0, covered, meas_up, cell, table, w):
    if table is None:
        return DC.project64(x0, covered, meas_up, cell, w)
    return PR.project_profile64(x0, covered, meas_up, cell, w, table)


def shape_noise64(eps, covered, cell, table, shrink):
    return project64(np.asarray(eps, dtype=np.float64), covered, np.zeros(np.shape(eps)), cell, table, shrink)[0]


def roundings(cell, table, w, scale):
    """One projection's count: (n + 3) 2^-24 S, or ((n + 4) G + 1) 2^-24 S with a profile."""
    return DC.projection_roundings(cell, scale) if table is None else PR.profile_roundings(cell, table, w, scale)


def shaping_roundings(cell, table, shrink, eps_max):
    """The same count taken with weight = shrink and S = max |eps|."""
    return roundings(cell, table, shrink, eps_max)


def vp_chain(vol, cfg, coefs, log_snr, clamp, blend, meas_up, cell, table, sched, seed=J.SEED, sample=0, net=J.stub64):
    """``volume_joint_dc_reference.vp_chain`` for a first-order table with the per-step dispatch: ``sched`` [T, 2] the fp32-rounded
    (w_i, shrink_i); w_i = 0: the plain step; else the projection with w_i and, where shrink_i > 0, the shaped normals.  Returns
    (state, layout, largest |x0| / |x0'|, largest |eps|)."""
    vol = np.asarray(vol, dtype=np.float32)
    L = J.layout(vol, cfg)
    P, stride, kept, slot = L['P'], L['stride'], L['kept'], L['slot']
    mean32, std32 = np.float32(cfg['Data']['mean']), np.float32(cfg['Data']['std'])
    low = ((vol - mean32) / std32).astype(np.float64)
    taps, c = R.taps_of(P, blend), J.clamp_of(*clamp)
    cut = lambda a, o: a[o[0]:o[0] + P, o[1]:o[1] + P, o[2]:o[2] + P][None, None]
    x = J.normals(vol.shape, seed, 0, sample).copy()
    x0_max, eps_max = 0.0, 0.0
    y = np.empty((kept.shape[0], P, P, P), dtype=np.float64)
    for i in range(coefs.shape[0]):
        for r, o in enumerate(kept):
            y[r] = net(cut(x, o), cut(low, o), np.full(1, log_snr[i]), None).reshape(P, P, P)
        x0, _, covered, _ = R.blend_accumulate(c(y)[None], slot, taps, stride, vol.shape)
        x0_max = max(x0_max, float(np.abs(x0[covered]).max()))
        x0 = np.where(covered, x0, 0.0)
        w_i, sh_i = sched[i]
        if w_i > 0:
            x0 = project64(x0, covered, meas_up, cell, table, w_i)[0]
        x0_max = max(x0_max, float(np.abs(x0).max()))
        kx, k0, kn = coefs[i]
        step = kx * x + k0 * x0
        if kn != 0:
            n = J.normals(vol.shape, seed, i + 1, sample)
            eps_max = max(eps_max, float(np.abs(n).max()))
            if w_i > 0 and sh_i > 0:
                n = shape_noise64(n, covered, cell, table, sh_i)
            step = step + kn * n
        x = np.where(covered, step, x)
    return x, L, x0_max, eps_max


def edm_chain(vol, cfg, tabs, blend, dynamic, meas_up, cell, table, sched, seed=E.SEED, sample=0, net=HN.stub64):
    """``volume_joint_dc_reference.edm_chain`` with the per-step dispatch of ``vp_chain``.  Returns (state, layout, largest |state|,
    largest |x0| / |x0'|, largest |eps|)."""
    vol = np.asarray(vol, dtype=np.float32)
    L = J.layout(vol, cfg)
    P, stride, kept, slot = L['P'], L['stride'], L['kept'], L['slot']
    assert not L['block']
    mean32, std32 = np.float32(cfg['Data']['mean']), np.float32(cfg['Data']['std'])
    alpha, sigma_lr = tabs['lowres']
    normal = lambda k: J.normals(vol.shape, seed, k, sample)
    low = alpha * ((vol - mean32) / std32).astype(np.float64) + sigma_lr * normal(0)
    taps = R.taps_of(P, blend)
    cut = lambda a, o: a[o[0]:o[0] + P, o[1]:o[1] + P, o[2]:o[2] + P][None, None]
    y = np.empty((kept.shape[0], P, P, P), dtype=np.float64)
    x = tabs['sigma0'] * normal(1)
    x0_vol, covered, state_max, x0_max, eps_max = None, None, 0.0, 0.0, 0.0
    for i, row in enumerate(tabs['coefs']):
        _, cin, cskip, cout, cnoise = tabs['pre'][i]
        for r, o in enumerate(kept):
            xw, lw = cut(x, o), cut(low, o)
            y[r] = E.threshold(cskip * xw + cout * net(cin * xw, lw, np.full(1, cnoise), None), dynamic).reshape(P, P, P)
        x0, covered = HN.fuse(y, slot, taps, stride, vol.shape)
        x0_max = max(x0_max, float(np.abs(x0[covered]).max()))
        x0 = np.where(covered, x0, 0.0)
        w_i, sh_i = sched[i]
        if w_i > 0:
            x0 = project64(x0, covered, meas_up, cell, table, w_i)[0]
        x0_max = max(x0_max, float(np.abs(x0).max()))
        state_max = max(state_max, float(np.abs(x[covered]).max()))
        n = None
        if row[3] != 0:
            n = normal(2 + i)
            eps_max = max(eps_max, float(np.abs(n).max()))
            if w_i > 0 and sh_i > 0:
                n = shape_noise64(n, covered, cell, table, sh_i)
        x = np.where(covered, E.update(x, x0, x0_vol, tuple(row), n), x)
        x0_vol = x0
    return x, L, max(state_max, float(np.abs(x[covered]).max())), x0_max, eps_max


def extra_per_step(cell, table, sched, kn, x0_scale, eps_max):
    """What one step adds to its family's bound: the projection's count for x0 (weight w_i) plus kn times the count taken with
    weight = shrink_i and S = max |eps| -- the largest over the steps."""
    return max((roundings(cell, table, w_i, x0_scale) if w_i > 0 else 0.0) +
               (abs(k) * shaping_roundings(cell, table, sh_i, eps_max) if w_i > 0 and sh_i > 0 else 0.0)
               for (w_i, sh_i), k in zip(sched, kn))


def vp_bound(windows_per_voxel, scale, cell, table, sched, kn, x0_scale, eps_max, steps=J.STEPS):
    return J.chain_bound(windows_per_voxel, scale) + steps * extra_per_step(cell, table, sched, kn, x0_scale, eps_max)


def edm_bound(tabs, L, cell, table, sched, kn, state_max, lowres_max, dynamic, x0_scale, eps_max):
    """``edm_dpmpp2m_reference.chain_bound`` with the extra count in the local term of every step, as further terms of 2^-23."""
    terms = extra_per_step(cell, table, sched, kn, x0_scale, eps_max) / 2.0 ** -23
    return E.chain_bound(tabs, L['windows_per_voxel'] + math.ceil(terms), state_max, lowres_max, dynamic, False)
