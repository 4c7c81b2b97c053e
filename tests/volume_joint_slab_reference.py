"""Specification of data consistency for OVERLAPPING slice profiles (``consistency_slab=`` of the samplers and of ``VolumeInference``)
in plain numpy, on top of tests/volume_joint_dc_reference.py.  Not a test module: tests/test_volume_slab_host.py and
tests/test_gpu_volume_slab.py import it.

The operator (include/diqt.h, above ``diqt_slab_measure``).  A cell is (fz, fy, fx) voxels; ``profile`` = (pz, py, px) with pz of
length L = fz + 2r, 1 <= r, 2r <= fz.  u_z = pz / sum pz, u_yx = py (x) px / (sum py sum px); slice s of the in-plane cell (cy, cx)
measures y_s = sum_i u_z[i] (u_yx . x[s fz - r + i, cell]).  A row is active when its whole support lies inside the domain and is
covered; the projection is DDNM on the active rows, x0' = x0 + w A_act^T (A_act A_act^T)^-1 (y_act - A_act x0).

Two restatements:
  * float64, the specification: ``project64`` builds the rows of every column as a dense matrix and applies the pseudo-inverse of the
    active ones (``numpy.linalg.pinv``); ``measure64`` is A itself.  It knows nothing of tridiagonal matrices or sweeps.
  * fp32, for the bit-exact tests: ``table`` (the host table in float64 arithmetic, rounded once -- ``ops.slab_profile`` must give the
    same bits), ``measure32``, ``project32`` and ``joint_step32``, the five steps of the kernels' one arithmetic definition with
    ``volume_joint_dc_reference.fma32`` for every fused multiply-add and ``fuse32`` for the window walk.

The rounding allowance of ONE projection, u = 2^-24.  S is the largest of |a|, |meas_up| and |a'| met, n_yx = fy fx, q = sum u_yx^2,
d = sum u_z^2, e the overlap product, kappa <= (d + 2e) / (d - 2e) the condition bound of any run (G is Toeplitz tridiagonal, its
eigenvalues lie in (d - 2e, d + 2e), and ``ops.slab_profile`` refuses d - 2e < d / 64, so kappa <= 128).  To first order in u:
  * a plane value is n_yx fused multiply-adds with weights that sum to 1: at most n_yx u S;
  * a row value is L more of them over the plane values, again with weights that sum to 1: L u S, plus the planes' n_yx u S;
  * the residual rho = y - row, |rho| <= 2 S, rounds once: 2 u S.  A residual is therefore off by at most (n_yx + L + 2) u S;
  * the solve G c = rho: |c| <= |rho| / (d - 2e) <= 2 S / (d - 2e) in the maximum norm (G is diagonally dominant by d - 2e).  An error
    of the residual enters c divided by d - 2e.  The two sweeps use, per row, the rounded m_j, e and ip_j, two fused multiply-adds and
    one product: six roundings, a relative backward error of 6 u on G, so 6 kappa u |c| <= 12 kappa u S / (d - 2e) on c;
  * a voxel adds at most two terms u_z c (it lies under at most two slices), scales by w g_yx <= max g_yx and rounds t, the product
    w g_yx and the final fused multiply-add: with K = 2 max(g_yx) max(u_z) / (d - 2e) the factor from a residual to a voxel, the
    errors of c arrive as K (n_yx + L + 2 + 12 kappa) u S, and the three local roundings are at most 3 u K S + u S <= 4 u S for
    K <= 1 -- they are charged as (3 K + 1) u S.
``slab_roundings(tab, S)`` = u S (K (n_yx + L + 5 + 12 kappa) + 1) is that number.  The host test asserts that the fp32 restatement
stays within a QUARTER of it on the inputs of the GPU tests (the GPU chains see other inputs); the chain tests add ``steps`` times it
to the family's bound.  None of these factors was tuned against the device.
"""
import contextlib

import numpy as np

from tests import volume_joint_dc_reference as DC

fma32 = DC.fma32


# ---- the host table -----------------------------------------------------------------------------------------------------------------------
def table(cell, profile, jmax):
    """The host table in float64 arithmetic with sequential sums, every entry rounded once to float32: a dict of ``uz`` [L], ``uyx``
    and ``gyx`` [fy fx], ``e``, ``m`` and ``ip`` [jmax] (float32), ``r`` and the float64 ``d``, ``e64``, ``q``, ``kappa``."""
    fz, fy, fx = cell
    pz, py, px = ([float(v) for v in p] for p in profile)
    r = (len(pz) - fz) // 2
    assert len(pz) == fz + 2 * r and 1 <= r and 2 * r <= fz and len(py) == fy and len(px) == fx
    sz = sy = sx = 0.0
    for v in pz:
        sz += v
    for v in py:
        sy += v
    for v in px:
        sx += v
    uz = [v / sz for v in pz]
    uyx = [a * b / (sy * sx) for a in py for b in px]
    q = d = e = 0.0
    for v in uyx:
        q += v * v
    for v in uz:
        d += v * v
    for i in range(2 * r):
        e += uz[i] * uz[i + fz]
    m, ip, pivot = [], [], d
    for j in range(jmax):
        if j:
            m.append(e / pivot)
            pivot = d - e * e / pivot
        else:
            m.append(0.0)
        ip.append(1.0 / pivot)
    f32 = lambda v: np.asarray(v, dtype=np.float64).astype(np.float32)
    return dict(cell=tuple(cell), r=r, jmax=jmax, uz=f32(uz), uyx=f32(uyx), gyx=f32([v / q for v in uyx]), e=f32(e), m=f32(m), ip=f32(ip),
                uz64=np.array(uz), uyx64=np.array(uyx), d=d, e64=e, q=q, kappa=(d + 2 * e) / (d - 2 * e))


def flat(tab):
    """The flat float32 layout the kernels read."""
    return np.concatenate([tab['uz'], tab['uyx'], tab['gyx'], tab['e'].reshape(1), tab['m'], tab['ip']]).astype(np.float32)


def slab_roundings(tab, scale):
    """The rounding allowance of one projection (module docstring)."""
    fz, fy, fx = tab['cell']
    K = 2.0 * float(tab['gyx'].max()) * float(tab['uz'].max()) / (tab['d'] - 2 * tab['e64'])
    return 2.0 ** -24 * scale * (K * (fy * fx + fz + 2 * tab['r'] + 5 + 12 * tab['kappa']) + 1)


# ---- float64: the specification -------------------------------------------------------------------------------------------------------------
def _rows64(tab, D):
    """The dense rows of one column: [S, D, fy fx] (a row that leaves the domain is truncated)."""
    fz, fy, fx = tab['cell']
    S, r = D // fz, tab['r']
    A = np.zeros((S, D, fy * fx))
    for s in range(S):
        for i, u in enumerate(tab['uz64']):
            z = s * fz - r + i
            if 0 <= z < D:
                A[s, z] = u * tab['uyx64']
    return A


def _columns(a, cell):
    """[D, H, W] -> [H/fy, W/fx, D, fy fx] (a copy)."""
    fz, fy, fx = cell
    D, H, W = a.shape
    return a.reshape(D, H // fy, fy, W // fx, fx).transpose(1, 3, 0, 2, 4).reshape(H // fy, W // fx, D, fy * fx)


def _uncolumns(c, cell, shape):
    fz, fy, fx = cell
    D, H, W = shape
    return c.reshape(H // fy, W // fx, D, fy, fx).transpose(2, 0, 3, 1, 4).reshape(D, H, W)


def active_rows(tab, covered):
    """bool [S, H/fy, W/fx]: the rows whose whole support lies inside the domain and is covered (``covered`` bool [D, H, W])."""
    fz, fy, fx = tab['cell']
    D = covered.shape[0]
    S, r = D // fz, tab['r']
    plane = _columns(covered, tab['cell']).all(axis=-1)                     # [ch, cw, D]
    act = np.zeros((S,) + plane.shape[:2], dtype=bool)
    for s in range(S):
        z0, z1 = s * fz - r, s * fz + fz + r
        if z0 >= 0 and z1 <= D:
            act[s] = plane[:, :, z0:z1].all(axis=-1)
    return act


def measure64(vol, tab):
    """A x in float64: [D/fz, H/fy, W/fx], truncated sums for the rows that leave the volume."""
    A = _rows64(tab, vol.shape[0])
    cols = _columns(np.asarray(vol, dtype=np.float64), tab['cell'])
    return np.einsum('szq,hwzq->shw', A, cols)


def project64(x0, meas_up, tab, w, covered=None):
    """x0 + w pinv(A_act) (y_act - A_act x0) per column of a [D, H, W] domain, in float64; returns (x0', touched) with ``touched``
    the voxels under at least one active row."""
    x0 = np.asarray(x0, dtype=np.float64)
    fz, fy, fx = tab['cell']
    D = x0.shape[0]
    covered = np.ones(x0.shape, dtype=bool) if covered is None else covered
    act = active_rows(tab, covered)
    A = _rows64(tab, D)
    cols = _columns(x0, tab['cell']).copy()
    y = np.asarray(meas_up, dtype=np.float64)[::fz, ::fy, ::fx]
    touched = np.zeros(cols.shape, dtype=bool)
    pinvs = {}
    for cy in range(cols.shape[0]):
        for cx in range(cols.shape[1]):
            on = np.flatnonzero(act[:, cy, cx])
            if on.size == 0:
                continue
            key = tuple(on)
            if key not in pinvs:
                Aa = A[on].reshape(on.size, -1)
                pinvs[key] = (Aa, np.linalg.pinv(Aa))
            Aa, Ap = pinvs[key]
            v = cols[cy, cx].reshape(-1)
            cols[cy, cx] = (v + w * (Ap @ (y[on, cy, cx] - Aa @ v))).reshape(D, -1)
            touched[cy, cx] = (Aa != 0).any(axis=0).reshape(D, -1)
    return _uncolumns(cols, tab['cell'], x0.shape), _uncolumns(touched, tab['cell'], x0.shape)


# ---- fp32: the kernels' arithmetic ------------------------------------------------------------------------------------------------------------
def _planes32(a, tab):
    """Step 1: pm [..., D, H/fy, W/fx], the fma sum of u_yx a over the cell's voxels of a plane in (y, x) order."""
    fz, fy, fx = tab['cell']
    a = np.asarray(a, dtype=np.float32)
    pm = np.zeros(a.shape[:-2] + (a.shape[-2] // fy, a.shape[-1] // fx), dtype=np.float32)
    for j in range(fy):
        for k in range(fx):
            pm = fma32(tab['uyx'][j * fx + k], a[..., j::fy, k::fx], pm)
    return pm


def measure32(vol, tab):
    """``diqt_slab_measure`` bit for bit: the planes outside the volume are skipped."""
    fz, fy, fx = tab['cell']
    D, r = vol.shape[0], tab['r']
    pm = _planes32(vol, tab)
    out = np.zeros((D // fz,) + pm.shape[1:], dtype=np.float32)
    for s in range(D // fz):
        for i in range(fz + 2 * r):
            z = s * fz - r + i
            if 0 <= z < D:
                out[s] = fma32(tab['uz'][i], pm[z], out[s])
    return out


def coeffs32(a, meas_up, tab, covered=None):
    """Steps 1 - 4 on a [..., D, H, W] (already clamped or fused): (c, active), both [..., S, H/fy, W/fx]; ``covered`` bool [D, H, W]
    or None (everything).  An uncovered plane has pm = 0, as the first joint kernel stores it."""
    f32 = np.float32
    fz, fy, fx = tab['cell']
    a = np.asarray(a, dtype=f32)
    D, r = a.shape[-3], tab['r']
    S, L = D // fz, fz + 2 * r
    pm = _planes32(a, tab)
    cov = np.ones(pm.shape[-3:], dtype=bool) if covered is None else _columns(covered, tab['cell']).all(axis=-1).transpose(2, 0, 1)
    pm = np.where(cov, pm, f32(0))
    y = np.asarray(meas_up, dtype=f32)[..., ::fz, ::fy, ::fx]
    lead = pm.shape[:-3]
    c = np.zeros(lead + (S,) + pm.shape[-2:], dtype=f32)
    act = np.zeros(c.shape, dtype=bool)
    pos = np.zeros(c.shape, dtype=np.int64)                                  # the run position j of an active row
    j = np.zeros(lead + pm.shape[-2:], dtype=np.int64)
    run = np.zeros(lead + pm.shape[-2:], dtype=f32)
    for s in range(S):
        z0 = s * fz - r
        if z0 < 0 or z0 + L > D:
            j[...] = 0
            continue
        acc = np.zeros(run.shape, dtype=f32)
        for i in range(L):
            acc = fma32(tab['uz'][i], pm[..., z0 + i, :, :], acc)
        on = np.broadcast_to(cov[z0:z0 + L].all(axis=0), run.shape)
        rho = y[..., s, :, :] - acc
        zeta = np.where(j == 0, rho, fma32(-tab['m'][j], run, rho))
        run = np.where(on, zeta, run).astype(f32)
        c[..., s, :, :] = np.where(on, zeta, f32(0))
        act[..., s, :, :] = on
        pos[..., s, :, :] = j
        j = np.where(on, j + 1, 0)
    run = np.zeros(run.shape, dtype=f32)
    for s in range(S - 1, -1, -1):
        on = act[..., s, :, :]
        cs = fma32(-tab['e'], run, c[..., s, :, :]) * tab['ip'][pos[..., s, :, :]]
        c[..., s, :, :] = np.where(on, cs, f32(0))
        run = np.where(on, cs, f32(0)).astype(f32)
    return c, act


def shift32(a, c, act, tab, w):
    """Step 5 on a [..., D, H, W]."""
    f32 = np.float32
    fz, fy, fx = tab['cell']
    a = np.asarray(a, dtype=f32)
    D, r = a.shape[-3], tab['r']
    S = D // fz
    up = lambda v: np.repeat(np.repeat(v, fy, axis=-2), fx, axis=-1)        # [..., ch, cw] -> [..., H, W]
    g = np.tile(tab['gyx'].reshape(fy, fx), (a.shape[-2] // fy, a.shape[-1] // fx))
    wg = f32(w) * g
    out = a.copy()
    for z in range(D):
        k, o = divmod(z, fz)
        t = np.zeros(c[..., 0, :, :].shape, dtype=f32)
        any_on = np.zeros(t.shape, dtype=bool)
        for s, i in ((k - 1, o + fz + r), (k, o + r), (k + 1, o - fz + r)):
            if s < 0 or s >= S or (s == k - 1 and not o < r) or (s == k + 1 and not o >= fz - r):
                continue
            on = act[..., s, :, :]
            t = np.where(on, fma32(tab['uz'][i], c[..., s, :, :], t), t).astype(f32)
            any_on = any_on | on
        out[..., z, :, :] = np.where(up(any_on), fma32(wg, up(t), a[..., z, :, :]), a[..., z, :, :])
    return out


def project32(a, meas_up, tab, w, covered=None):
    """``diqt_slab_project`` on clamped cubes a [..., P, P, P] (the domain is each cube), or the projection of the joint step on a fused
    [D, H, W] with its ``covered`` mask, bit for bit."""
    c, act = coeffs32(a, meas_up, tab, covered)
    return shift32(a, c, act, tab, w)


def joint_step32(y, slot, taps, stride, x_t, x0_prev, meas_up, tab, w, form, kx, k0, kp, kn, clamp, n, fused=None):
    """What the three launches of a joint slab step compute, bit for bit: (x_next, x0_out, covered);
    ``volume_joint_dc_reference.joint_step32`` with the slab projection in the place of the cell projection."""
    f32 = np.float32
    x_t = np.asarray(x_t, dtype=f32)
    x0, covered = fused if fused is not None else DC.fuse32(y, slot, taps, stride, x_t.shape, clamp)
    x0 = project32(x0, meas_up, tab, w, covered)
    x0 = np.where(covered, x0, f32(0)).astype(f32)
    b = f32(k0) * x0
    if form == 0:
        c = f32(kn) * (np.asarray(n, dtype=f32) if kn != 0 else np.zeros(x_t.shape, dtype=f32))
        u = fma32(f32(kx), x_t, b) + c
    else:
        prev = np.zeros(x_t.shape, dtype=f32) if x0_prev is None else np.asarray(x0_prev, dtype=f32)
        u = fma32(f32(kx), x_t, b) + f32(kp) * prev
        if form == 2 and kn != 0:
            u = u + f32(kn) * np.asarray(n, dtype=f32)
    return np.where(covered, u, x_t).astype(f32), x0, covered


# ---- the profiles and inputs the tests share ----------------------------------------------------------------------------------------------------
def gaussian_pz(fz, r, width=0.45):
    """A Gaussian-like slice profile of fz + 2r samples, full width ``width`` of its length at half maximum."""
    L = fz + 2 * r
    t = (np.arange(L) - (L - 1) / 2) / (width * L / 2.355)
    return [float(v) for v in np.exp(-0.5 * t * t)]


# (cell, profile, cube edge): the per-window cases of the GPU tests, restated on the host
PROJECT_CASES = (
    ((2, 1, 1), ([0.25, 1.0, 1.0, 0.25], [1.0], [1.0]), 8),              # S = 4: one run of two rows
    ((4, 1, 1), ([0.3, 1.0, 1.0, 1.0, 1.0, 0.3], [1.0], [1.0]), 16),      # r = 1: the middle voxels lie under one slice only
    ((4, 1, 1), (gaussian_pz(4, 2), [1.0], [1.0]), 16),                   # r = 2 = fz / 2
    ((4, 2, 2), (gaussian_pz(4, 2), [1.0, 0.5], [0.75, 1.0]), 16),        # a non-uniform in-plane profile
    ((2, 3, 1), ([0.5, 1.0, 0.8, 0.2], [0.5, 1.0, 0.5], [1.0]), 12),      # (2, 3, 1)-style cells: H = 12 allows fy = 3
)


def project_inputs(cell, P, cubes=3, seed=7):
    """(x0 [cubes, 1, P, P, P], meas_up of the same shape, constant per cell) in float32, |x0| up to about 5."""
    rng = np.random.default_rng(seed + P)
    x0 = (rng.standard_normal((cubes, 1, P, P, P)) * 1.5).astype(np.float32)
    coarse = rng.standard_normal((cubes, 1, P // cell[0], P // cell[1], P // cell[2])).astype(np.float32)
    return x0, np.ascontiguousarray(DC.replicate(coarse, cell))


@contextlib.contextmanager
def slab_chains(tab):
    """Inside the block ``volume_joint_dc_reference.vp_chain`` / ``edm_chain`` are the float64 chains of ``consistency_slab``: their
    projection between the fuse and the update is ``project64`` of this module (the ``cell`` they are given is not looked at)."""
    def project(x0, covered, meas_up, cell, w):
        return project64(x0, meas_up, tab, w, covered)
    saved, DC.project64 = DC.project64, project
    try:
        yield
    finally:
        DC.project64 = saved
