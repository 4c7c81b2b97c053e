"""Specification of noise-aware data consistency for a tile operator (``consistency_row_noise=`` of the samplers and of
``VolumeInference``; DDNM+, Wang, Yu, Zhang, ICLR 2023, section 3.3, with one weight per singular direction) in plain numpy, on top
of tests/volume_joint_tile_reference.py and tests/volume_joint_noise_reference.py.  Not a test module:
tests/test_volume_tile_noise_host.py and tests/test_gpu_volume_tile_noise.py import it.  Nothing here calls ``ops``.

The model.  y = A x + n_y with independent rows, n_y[r] ~ N(0, sigma_r^2).  Whitening is unit-free: omega_r = sigma_min / sigma_r in
(0, 1], A_w = diag(omega) A = U S V^T (numpy's SVD; zero at or below 1e-10 s_max).  The effective pseudo-inverse is
A_p = A_w+ diag(omega) [n, m] and t = A_p y, so Cov(t) = A_p diag(sigma^2) A_p^T = sigma_min^2 V S^-2 V^T: along the right singular
vector v_j the noise of t has the deviation sigma_min / s_j.  Direction j therefore takes the scalar recursion of
``volume_joint_noise_reference.schedule64`` with s = s_j and sigma_y = sigma_min (``whiten`` / ``schedule64``), the history term, the
cap and the zero on rows with kn = 0 included; null-space directions have lambda = shrink = 0.

The tables (``tables64``).  M_i = V diag(lambda_i) V^T and G_i = V diag(shrink_i) V^T in float64, symmetrised (X + X^T) / 2, rounded
once to fp32 -- the rounded tables DEFINE the step, so the float64 side takes them widened.  lambda is continuous in s, so M does not
depend on the basis the SVD picks inside a repeated singular value.  G does, a little: on an uncapped step a = b exactly and
shrink = 1 - sqrt(1 - (a / b)^2) sits at the branch point of the root, where one ulp of s moves it by 1.5e-8 -- two SVDs of one
operator give G tables about 1e-8 apart, which is why the host test compares G given one decomposition.  ``kinds`` is the dispatch on the fp32
values of the schedule: every lambda 0 'plain'; every shrink 0 and all lambda equal w 'tile' (the constant-weight projection with
P); else 'noise'.

The arithmetic (include/diqt.h, above ``diqt_tile_project_noise``) on one tile, a the clamped or fused values, q the voxel:
    d[r] = t[r] - a[r];  s = 0;  s = fma(M[r][q], d[r], s) for r = 0 .. n - 1;  a'[q] = a[q] + s;
    g = 0;  g = fma(G[r][q], eps[r], g) for r = 0 .. n - 1;  eps'[q] = eps[q] - g.
``project_noise32`` restates it in float32 with ``volume_joint_tile_reference.apply32`` (whose fma is checked against exact
rationals; the host test checks THIS order against exact rationals again), ``joint_step_tile_noise32`` puts it between the fuse and
the three updates, ``project_noise64`` is the float64 side.

The rounding counts, to first order in u = 2^-24.  G_M = max_q sum_r |M[r][q]| and G_G likewise, on the fp32 tables
(``gain_of``); S = the largest of |a|, |t| and |a'| in the tile, E = the largest |eps|.
  Projection (``projection_roundings``):
  * d = t - a is rounded once, |d| <= 2 S: u 2 S on every d[r], which the sum carries with the gain G_M: 2 G_M u S on s;
  * the n fma roundings of the sum, each on a partial sum of magnitude <= sum_r |M[r][q]| |d[r]| <= 2 G_M S: 2 n G_M u S on s;
  * the final add rounds a', |a'| <= S: u S.
  Together (2 (n + 1) G_M + 1) u S.
  Shaping (``shaping_roundings``): eps is read as it is (no d), the n fma roundings on partial sums <= G_G E give n G_G u E, and the
  final subtraction rounds eps', |eps'| <= (1 + G_G) E: together ((n + 1) G_G + 1) u E.  It enters the update multiplied by kn.
The chain bounds are the families' bounds plus ``steps`` times the largest per-step sum of the two (``extra_per_step``; a 'tile'
step takes ``volume_joint_tile_reference.tile_roundings``); for the EDM recursion it enters as further local terms of 2^-23.
Nothing is tuned against the device.

The variance identity (``variance_defect``).  B_i = k0 M_i + kp M_{i-1}; the step carries B_i A_p n_y and kn (I - G_i) eps, so where
no direction had its weight clipped at 0 with |a| > b,  B_i Cov(t) B_i^T + kn^2 (I - G_i)(I - G_i)^T = kn^2 I  on the row space of A
and kn^2 I trivially on its null space: (a_ij sigma_min / s_j)^2 + ((1 - shrink_ij) kn)^2 = kn^2 per direction.

The normals.  The float64 chains take the anchored field of tests/anchored_noise_reference.py
(``volume_joint_reference.normals``); the bit-exact step tests hand the device's fp32 normals in and assert their distance to that
field, as tests/volume_joint_noise_reference.py explains.
"""
import math

import numpy as np

from tests import edm_dpmpp2m_reference as E
from tests import volume_blend_reference as R
from tests import volume_joint_heun_reference as HN
from tests import volume_joint_noise_reference as NR
from tests import volume_joint_reference as J
from tests import volume_joint_tile_reference as TR
from tests.volume_joint_dc_reference import _cells, clamp32, fma32, fuse32, replicate     # noqa: F401  (the tests take them from here)
from tests.volume_joint_noise_reference import dispatch, rows4                             # noqa: F401

# the operators of the host tests: name -> (cell, matrix, per-row deviations); stacks take one deviation per stack
STACK_NOISE = {
    'stacks-222': ((2, 2, 2), (0, 1, 2), (0.05, 0.2, 0.1)),
    'stacks-441': ((4, 4, 1), (0, 1), (0.05, 0.15)),
    'stacks-444': ((4, 4, 4), (0, 1, 2), (0.05, 0.2, 0.1)),
}


def stack_sigma(cell, axes, per_stack):
    """One deviation per stack, repeated over that stack's rows (``stack_matrix``'s row order)."""
    n = cell[0] * cell[1] * cell[2]
    return np.concatenate([np.full(n // cell[a], float(s)) for a, s in zip(axes, per_stack)])


def case_of(name):
    """(cell, A, sigma [m]) of a named case: the stacks above, 'dense-232' of the tile module with a deviation ramp, or any name of
    ``volume_joint_tile_reference.OPERATORS`` with per-stack deviations 0.05, 0.2, 0.1 in the order of its axes."""
    if name in STACK_NOISE:
        cell, axes, per = STACK_NOISE[name]
        return cell, TR.stack_matrix(cell, axes), stack_sigma(cell, axes, per)
    cell, how = TR.OPERATORS[name]
    A = TR.matrix_of(name)[1]
    if how[0] == 'dense':
        return cell, A, np.linspace(0.05, 0.25, A.shape[0])
    return cell, A, stack_sigma(cell, how, (0.05, 0.2, 0.1)[:len(how)])


# ---- the host side, float64 ---------------------------------------------------------------------------------------------------------------
def whiten(A, sigma):
    """The whitened operator of A [m, n] under per-row deviations ``sigma`` (a number or [m]): a dict with ``omega`` [m],
    ``sigma_min``, ``S`` [rank], ``V`` [rank, n] (right singular vectors as rows), ``pinv`` = A_w+ diag(omega) [n, m] and ``P`` =
    A_w+ A_w symmetrised."""
    A = np.asarray(A, dtype=np.float64)
    sigma = np.broadcast_to(np.asarray(sigma, dtype=np.float64), (A.shape[0],)).copy()
    omega = sigma.min() / sigma
    Aw = omega[:, None] * A
    U, S, Vh = np.linalg.svd(Aw, full_matrices=False)
    rel = S / S[0]
    assert not ((rel > 1e-10) & (rel < 1e-6)).any()
    keep = rel > 1e-10
    pinv_w = (Vh[keep].T / S[keep]) @ U[:, keep].T
    P = pinv_w @ Aw
    return dict(omega=omega, sigma=sigma, sigma_min=float(sigma.min()), S=S[keep], V=Vh[keep], pinv=pinv_w * omega[None, :],
                P=(P + P.T) / 2)


def schedule64(rows, S, sigma_min, w):
    """float64 [T, rank, 2] = (lambda_ij, shrink_ij): the scalar recursion per direction (module docstring)."""
    return np.stack([NR.schedule64(rows, float(s), float(sigma_min), float(w)) for s in S], axis=1)


def tables64(V, sched):
    """float64 [T, 2, n, n] = (M_i, G_i), symmetrised; ``tables32`` rounds them once."""
    V = np.asarray(V, dtype=np.float64)
    out = np.einsum('jq,tjc,jr->tcqr', V, np.asarray(sched, dtype=np.float64), V)
    return (out + out.transpose(0, 1, 3, 2)) / 2


def tables32(V, sched):
    return tables64(V, sched).astype(np.float32)


def kinds(sched):
    """The dispatch of every step on the fp32 values of the schedule: [(kind, w)]."""
    out = []
    for step in np.asarray(sched, dtype=np.float64).astype(np.float32):
        lam, shrink = step[:, 0], step[:, 1]
        if not lam.any():
            out.append(('plain', 0.0))
        elif not shrink.any() and (lam == lam[0]).all():
            out.append(('tile', float(lam[0])))
        else:
            out.append(('noise', 0.0))
    return out


def variance_defect(wh, sched, rows):
    """Per step the largest entry of |B_i Cov(t) B_i^T + kn^2 (I - G_i)(I - G_i)^T - kn^2 I| with the float64 tables, and whether the
    step qualifies (kn != 0 and no direction clipped at 0 with |a| > b): [(defect, kn, qualifies)]."""
    rows = np.asarray(rows, dtype=np.float64)
    tabs = tables64(wh['V'], sched)
    cov = wh['pinv'] @ np.diag(wh['sigma'] ** 2) @ wh['pinv'].T
    n = cov.shape[0]
    out = []
    for i, (kx, k0, kp, kn) in enumerate(rows):
        prev = tabs[i - 1, 0] if i else np.zeros((n, n))
        lam_prev = sched[i - 1, :, 0] if i else np.zeros(len(wh['S']))
        B = k0 * tabs[i, 0] + kp * prev
        I_G = np.eye(n) - tabs[i, 1]
        defect = np.abs(B @ cov @ B.T + kn ** 2 * I_G @ I_G.T - kn ** 2 * np.eye(n)).max()
        a = k0 * sched[i, :, 0] + kp * lam_prev
        b = kn * wh['S'] / wh['sigma_min']
        out.append((float(defect), float(kn), bool(kn != 0 and (np.abs(a) <= np.abs(b) * (1 + 1e-12)).all())))
    return out


# ---- fp32 -----------------------------------------------------------------------------------------------------------------------------------
def _whole(covered, cell):
    return replicate(_cells(covered, cell).all(axis=(-5, -3, -1)), cell)


def project_noise32(a, target, eps, cell, tables, covered=None):
    """(a', eps') of [..., D, H, W] arrays in float32 (``a`` already clamped), ``tables`` [2, n, n] fp32; ``covered`` (bool
    [D,H,W]): only tiles whose voxels are ALL covered are moved and shaped."""
    f32 = np.float32
    a, target, eps = (np.asarray(v, dtype=f32) for v in (a, target, eps))
    tables = np.asarray(tables, dtype=f32)
    d = (target - a).astype(f32)
    out = (a + TR.apply32(d, cell, tables[0])).astype(f32)
    shaped = (eps - TR.apply32(eps, cell, tables[1])).astype(f32)
    if covered is None:
        return out, shaped
    whole = _whole(covered, cell)
    return np.where(whole, out, a), np.where(whole, shaped, eps)


def tile_project_noise32(x0, target, eps, cell, tables, clamp):
    """What ``diqt_tile_project_noise`` computes, bit for bit: (x0', eps'); ``clamp`` = (lo, hi, mode) or None."""
    return project_noise32(clamp32(*(clamp or (0., 0., None)))(np.asarray(x0, dtype=np.float32)), target, eps, cell, tables)


def joint_step_tile_noise32(y, slot, taps, stride, x_t, x0_prev, target, cell, tables, form, kx, k0, kp, kn, clamp, n, fused=None):
    """What ``diqt_volume_joint_consistent_tile_noise_step`` computes, bit for bit: (x_next, x0_out, covered, eps') -- the fuse, the
    arithmetic above on the tiles whose voxels are all covered, then the update of ``volume_joint_tile_reference.joint_step_tile32``
    in its operation order.  Forms 0 and 2, kn != 0; ``n`` the step's float32 normals."""
    assert form in (0, 2) and kn != 0
    f32 = np.float32
    x_t = np.asarray(x_t, dtype=f32)
    x0, covered = fused if fused is not None else fuse32(y, slot, taps, stride, x_t.shape, clamp)
    x0 = np.where(covered, x0, f32(0)).astype(f32)
    x0, eps = project_noise32(x0, target, n, cell, tables, covered)
    b = f32(k0) * x0
    if form == 0:
        u = fma32(f32(kx), x_t, b) + f32(kn) * eps
    else:
        prev = np.zeros(x_t.shape, dtype=f32) if x0_prev is None else np.asarray(x0_prev, dtype=f32)
        u = fma32(f32(kx), x_t, b) + f32(kp) * prev
        u = u + f32(kn) * eps
    return np.where(covered, u, x_t).astype(f32), x0, covered, eps


# ---- float64 --------------------------------------------------------------------------------------------------------------------------------
def project_noise64(x0, covered, target, eps, cell, tables):
    """x0 + M (t - x0) and eps - G eps on the tiles whose voxels are all covered, in float64 with the fp32 tables widened."""
    tables = np.asarray(tables, dtype=np.float64)
    whole = _whole(covered, cell)
    out = np.where(whole, x0 + TR.apply64(target - x0, cell, tables[0]), x0)
    return out, (None if eps is None else np.where(whole, eps - TR.apply64(eps, cell, tables[1]), eps))


def gain_of(table):
    return TR.gain_of(table)


def projection_roundings(cell, tables, scale):
    """(2 (n + 1) G_M + 1) 2^-24 S (module docstring)."""
    n = cell[0] * cell[1] * cell[2]
    return (2 * (n + 1) * gain_of(tables[0]) + 1) * 2.0 ** -24 * scale


def shaping_roundings(cell, tables, eps_max):
    """((n + 1) G_G + 1) 2^-24 E (module docstring)."""
    n = cell[0] * cell[1] * cell[2]
    return ((n + 1) * gain_of(tables[1]) + 1) * 2.0 ** -24 * eps_max


def extra_per_step(cell, P, tables, kind, kn, x0_scale, eps_max):
    """What one step adds to its family's bound, the largest over the steps: nothing ('plain'), the constant-weight tile
    projection's count ('tile') or this module's two counts, the shaping's times |kn| ('noise')."""
    def one(i):
        if kind[i][0] == 'plain':
            return 0.0
        if kind[i][0] == 'tile':
            return TR.tile_roundings(cell, P, x0_scale)
        return projection_roundings(cell, tables[i], x0_scale) + abs(kn[i]) * shaping_roundings(cell, tables[i], eps_max)
    return max(one(i) for i in range(len(kind)))


def _project_step(x0, covered, target, n, cell, P, tables, kind):
    if kind[0] == 'tile':
        return TR.project_tile64(x0, covered, target, cell, kind[1], P)[0], n
    if kind[0] == 'noise':
        return project_noise64(x0, covered, target, n, cell, tables)
    return x0, n


def vp_chain(vol, cfg, coefs, log_snr, clamp, blend, target, cell, P, tables, kind, seed=J.SEED, sample=0, net=J.stub64):
    """``volume_joint_noise_reference.vp_chain`` (first-order tables) with this module's per-step dispatch: ``tables`` [T, 2, n, n]
    and ``P`` the fp32 tables, ``kind`` = ``kinds``.  Returns (state, layout, largest |x0| / |x0'|, largest |eps|)."""
    vol = np.asarray(vol, dtype=np.float32)
    L = J.layout(vol, cfg)
    Pw, stride, kept, slot = L['P'], L['stride'], L['kept'], L['slot']
    mean32, std32 = np.float32(cfg['Data']['mean']), np.float32(cfg['Data']['std'])
    low = ((vol - mean32) / std32).astype(np.float64)
    taps, c = R.taps_of(Pw, blend), J.clamp_of(*clamp)
    cut = lambda a, o: a[o[0]:o[0] + Pw, o[1]:o[1] + Pw, o[2]:o[2] + Pw][None, None]
    x = J.normals(vol.shape, seed, 0, sample).copy()
    x0_max, eps_max = 0.0, 0.0
    y = np.empty((kept.shape[0], Pw, Pw, Pw), dtype=np.float64)
    for i in range(coefs.shape[0]):
        for r, o in enumerate(kept):
            y[r] = net(cut(x, o), cut(low, o), np.full(1, log_snr[i]), None).reshape(Pw, Pw, Pw)
        x0, _, covered, _ = R.blend_accumulate(c(y)[None], slot, taps, stride, vol.shape)
        x0_max = max(x0_max, float(np.abs(x0[covered]).max()))
        x0 = np.where(covered, x0, 0.0)
        kx, k0, kn = coefs[i]
        n = None
        if kn != 0:
            n = J.normals(vol.shape, seed, i + 1, sample)
            eps_max = max(eps_max, float(np.abs(n).max()))
        x0, n = _project_step(x0, covered, target, n, cell, P, tables[i], kind[i])
        x0_max = max(x0_max, float(np.abs(x0).max()))
        step = kx * x + k0 * x0
        if kn != 0:
            step = step + kn * n
        x = np.where(covered, step, x)
    return x, L, x0_max, eps_max


def edm_chain(vol, cfg, tabs, blend, dynamic, target, cell, P, tables, kind, seed=E.SEED, sample=0, net=HN.stub64):
    """``volume_joint_noise_reference.edm_chain`` with this module's per-step dispatch.  Returns (state, layout, largest |state|,
    largest |x0| / |x0'|, largest |eps|)."""
    vol = np.asarray(vol, dtype=np.float32)
    L = J.layout(vol, cfg)
    Pw, stride, kept, slot = L['P'], L['stride'], L['kept'], L['slot']
    assert not L['block']
    mean32, std32 = np.float32(cfg['Data']['mean']), np.float32(cfg['Data']['std'])
    alpha, sigma_lr = tabs['lowres']
    normal = lambda k: J.normals(vol.shape, seed, k, sample)
    low = alpha * ((vol - mean32) / std32).astype(np.float64) + sigma_lr * normal(0)
    taps = R.taps_of(Pw, blend)
    cut = lambda a, o: a[o[0]:o[0] + Pw, o[1]:o[1] + Pw, o[2]:o[2] + Pw][None, None]
    y = np.empty((kept.shape[0], Pw, Pw, Pw), dtype=np.float64)
    x = tabs['sigma0'] * normal(1)
    x0_vol, covered, state_max, x0_max, eps_max = None, None, 0.0, 0.0, 0.0
    for i, row in enumerate(tabs['coefs']):
        _, cin, cskip, cout, cnoise = tabs['pre'][i]
        for r, o in enumerate(kept):
            xw, lw = cut(x, o), cut(low, o)
            y[r] = E.threshold(cskip * xw + cout * net(cin * xw, lw, np.full(1, cnoise), None), dynamic).reshape(Pw, Pw, Pw)
        x0, covered = HN.fuse(y, slot, taps, stride, vol.shape)
        x0_max = max(x0_max, float(np.abs(x0[covered]).max()))
        x0 = np.where(covered, x0, 0.0)
        n = None
        if row[3] != 0:
            n = normal(2 + i)
            eps_max = max(eps_max, float(np.abs(n).max()))
        x0, n = _project_step(x0, covered, target, n, cell, P, tables[i], kind[i])
        x0_max = max(x0_max, float(np.abs(x0).max()))
        state_max = max(state_max, float(np.abs(x[covered]).max()))
        x = np.where(covered, E.update(x, x0, x0_vol, tuple(row), n), x)
        x0_vol = x0
    return x, L, max(state_max, float(np.abs(x[covered]).max())), x0_max, eps_max


def vp_bound(windows_per_voxel, scale, extra, steps=J.STEPS):
    return J.chain_bound(windows_per_voxel, scale) + steps * extra


def edm_bound(tabs, L, extra, state_max, lowres_max, dynamic):
    """``edm_dpmpp2m_reference.chain_bound`` with ``extra`` in the local term of every step, as further terms of 2^-23."""
    return E.chain_bound(tabs, L['windows_per_voxel'] + math.ceil(extra / 2.0 ** -23), state_max, lowres_max, dynamic, False)
