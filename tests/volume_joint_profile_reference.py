"""Specification of data-consistent sampling with a slice profile (``consistency_profile=`` of the samplers and of
``VolumeInference``) in plain numpy, on top of tests/volume_joint_dc_reference.py.  Not a test module:
tests/test_volume_profile_host.py and tests/test_gpu_volume_profile.py import it.

The operator.  A cell is (fz, fy, fx) voxels, n = fz fy fx, q the lexicographic (z, y, x) index of a voxel inside its cell.  A profile
(pz, py, px) gives the weights u_q = pz_i py_j px_k / (sum pz sum py sum px), u >= 0 and sum u = 1; the measurement of a cell is
y = u . x.  The cells are disjoint, so A A^T = |u|^2 I, A+ = A^T / |u|^2 and the projection is, per voxel,
    x0'_v = x0_v + w g_v (y - u . x0),     g = u / sum u^2.
``profile_table`` is the [2, n] table (u, g) with the arithmetic of ``ops.cell_profile``: float64, each entry rounded once to fp32.

The projection (include/diqt.h, above ``diqt_cell_wmean``), over one cell, with the measurement replicated (``meas_up``):
    s = 0;  s = fma(u[q], a[q], s) in lexicographic order;  m = s;  t = w g[q] (one rounded product);  a'[v] = fma(t, meas_up[v] - m, a[v]).

Two restatements, as in the uniform module:
  * fp32, for the bit-exact tests: ``cell_wmean32`` / ``project_profile32`` with exactly that order and ``joint_step_profile32``, the
    three updates of ``volume_joint_dc_reference.joint_step32`` behind this projection (``fuse32``, ``fma32`` and the update's
    operation order are that module's);
  * float64, for the chain tests: ``project_profile64`` and ``vp_chain`` / ``edm_chain``, that module's chains with it between the
    fuse and the update.  The float64 side takes the SAME table, widened: the rounding of the table defines the operator, it is not
    an error of the arithmetic.

The rounding count of one projection, ``profile_roundings``: ((n + 4) G + 1) 2^-24 S with G = max(1, w max g) and S the largest of
|a|, |meas_up| and |a'| in the cell.  To first order in 2^-24:
  * the n fma roundings of the sum, each on a partial sum of magnitude <= S (u >= 0 and sum u = 1: a partial sum is a sub-convex
    combination of values of magnitude <= S): n 2^-24 S on m;
  * the subtraction r = meas_up - m rounds r, |r| <= 2 S: 2 2^-24 S more, (n + 2) 2^-24 S on r;
  * the product t r carries those times t <= G, and the rounding of t = w g, relative 2^-24 on |t r| <= 2 G S, its own 2 G 2^-24 S:
    (n + 4) G 2^-24 S;
  * the final fma rounds a', |a'| <= S: 2^-24 S.
The chain bounds are the uniform families' bounds plus ``steps`` times that number, exactly as the uniform tests add theirs; for the
EDM recursion it enters as S ((n + 4) G + 1) / 2 further local terms of 2^-23 (``edm_bound``).  Checked on the CPU against float64
(profiles (1,3,3,1), (0,1,1,0), ((1,2),(1,1),(3,1)), a Gaussian over 8 voxels and (0.1,1,1,0.1)^3, w = 1 and 0.5; values of
standard deviation 2, tests/test_volume_profile_host.py prints the figures): the fp32 result sat at 0.01 - 0.09 of the count and the
w = 1 residual |u . x0' - y| at <= 3.4e-7, a tenth of the count or less.  It is not tuned against the device.
"""
import math

import numpy as np

from tests import edm_dpmpp2m_reference as E
from tests import volume_joint_dc_reference as DC
from tests.volume_joint_dc_reference import _cells, clamp32, fma32, fuse32, replicate   # noqa: F401  (the tests take them from here)

GAUSS8 = tuple(math.exp(-0.5 * ((k - 3.5) / 1.5) ** 2) for k in range(8))                # a Gaussian slice profile over 8 voxels
# the cells and profiles of the tests: trapezoid, slice gap, Gaussian, a separable non-uniform one
PROFILES = {
    'trapezoid': ((4, 1, 1), ((1, 3, 3, 1), (1,), (1,))),
    'gap': ((4, 1, 1), ((0, 1, 1, 0), (1,), (1,))),
    'gauss8': ((1, 1, 8), ((1,), (1,), GAUSS8)),
    'separable': ((2, 2, 2), ((1, 2), (1, 1), (3, 1))),
}


def profile_table(cell, profile):
    """``ops.cell_profile``'s arithmetic: float32 [2, n], row 0 u, row 1 g = u / sum u^2; float64 throughout (Python floats, sums in
    sequence order), ONE rounding to fp32 per entry."""
    sums = []
    for p in profile:
        total = 0.0
        for v in p:
            total += float(v)
        sums.append(total)
    den = sums[0] * sums[1] * sums[2]
    u = [float(a) * float(b) * float(c) / den for a in profile[0] for b in profile[1] for c in profile[2]]
    sq = 0.0
    for v in u:
        sq += v * v
    assert len(u) == cell[0] * cell[1] * cell[2]
    return np.array([u, [v / sq for v in u]], dtype=np.float64).astype(np.float32)


# ---- fp32 ---------------------------------------------------------------------------------------------------------------------------------
def cell_wmean32(a, cell, table):
    """m of every cell of a [..., D, H, W]: s = 0; s = fma(u[q], a[q], s) in (z, y, x) order, in float32.  No division."""
    fz, fy, fx = cell
    c = _cells(np.asarray(a, dtype=np.float32), cell)
    s = np.zeros(c.shape[:-6] + (c.shape[-6], c.shape[-4], c.shape[-2]), dtype=np.float32)
    q = 0
    for i in range(fz):
        for j in range(fy):
            for k in range(fx):
                s = fma32(np.float32(table[0, q]), c[..., :, i, :, j, :, k], s)
                q += 1
    return s


def gains(table, cell, shape):
    """Row 1 of the table laid over a [D,H,W] grid: every voxel holds the gain of its place inside its cell."""
    g = np.asarray(table[1]).reshape(cell)
    return np.tile(g, tuple(s // f for s, f in zip(shape[-3:], cell)))


def project_profile32(a, meas_up, cell, table, w, covered=None):
    """The projection of a [..., D, H, W] (already clamped) in float32.  ``covered`` (bool [D,H,W]): only the cells whose voxels are
    ALL covered -- whatever their weights -- are corrected, the others keep their values."""
    a = np.asarray(a, dtype=np.float32)
    m = replicate(cell_wmean32(a, cell, table), cell)
    t = np.float32(w) * gains(table, cell, a.shape).astype(np.float32)                     # one rounded product
    r = np.asarray(meas_up, dtype=np.float32) - m
    out = fma32(t, r, a)
    if covered is None:
        return out
    whole = replicate(_cells(covered, cell).all(axis=(-5, -3, -1)), cell)
    return np.where(whole, out, a)


def joint_step_profile32(y, slot, taps, stride, x_t, x0_prev, meas_up, cell, table, w, form, kx, k0, kp, kn, clamp, n, fused=None):
    """What ``diqt_volume_joint_consistent_profile_step`` computes, bit for bit: (x_next, x0_out, covered) --
    ``volume_joint_dc_reference.joint_step32`` with ``project_profile32`` in the place of ``project32``; the update's operation order
    is restated from there."""
    f32 = np.float32
    x_t = np.asarray(x_t, dtype=f32)
    x0, covered = fused if fused is not None else fuse32(y, slot, taps, stride, x_t.shape, clamp)
    x0 = project_profile32(x0, meas_up, cell, table, w, covered)
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


# ---- float64 ------------------------------------------------------------------------------------------------------------------------------
def cell_wmean64(x, cell, table):
    """u . x of every cell in float64, u the table's row 0 widened: [..., D/fz, H/fy, W/fx]."""
    u = np.asarray(table[0], dtype=np.float64).reshape(cell)
    c = _cells(np.asarray(x, dtype=np.float64), cell)
    return (c * u[:, None, :, None, :]).sum(axis=(-5, -3, -1))                             # [fz, 1, fy, 1, fx] against the last five axes


def project_profile64(x0, covered, meas_up, cell, w, table):
    """x0 + w g (y - u . x0) on the cells whose voxels are all covered, in float64: (x0', whole)."""
    m = replicate(cell_wmean64(x0, cell, table), cell)
    whole = replicate(_cells(covered, cell).all(axis=(-5, -3, -1)), cell)
    g = gains(np.asarray(table, dtype=np.float64), cell, x0.shape)
    return np.where(whole, x0 + w * g * (meas_up - m), x0), whole


def profile_roundings(cell, table, w, scale):
    """The projection's own fp32 roundings on one x0 (module docstring): ((n + 4) G + 1) 2^-24 S, G = max(1, w max g)."""
    n = cell[0] * cell[1] * cell[2]
    G = max(1.0, float(w) * float(np.max(table[1])))
    return ((n + 4) * G + 1) * 2.0 ** -24 * scale


class _projection:
    """``volume_joint_dc_reference``'s chains call its ``project64`` between the fuse and the update; inside this context that name
    is ``project_profile64`` with the table, so the chains below ARE those chains, nothing restated."""

    def __init__(self, table):
        self.table = table

    def __enter__(self):
        self.saved = DC.project64
        DC.project64 = lambda x0, covered, meas_up, cell, w: project_profile64(x0, covered, meas_up, cell, w, self.table)

    def __exit__(self, *exc):
        DC.project64 = self.saved


def vp_chain(vol, cfg, coefs, log_snr, clamp, blend, meas_up, cell, table, w, **kw):
    """``volume_joint_dc_reference.vp_chain`` with ``project_profile64`` between the fuse and the update."""
    with _projection(table):
        return DC.vp_chain(vol, cfg, coefs, log_snr, clamp, blend, meas_up, cell, w, **kw)


def edm_chain(vol, cfg, tabs, blend, dynamic, meas_up, cell, table, w, **kw):
    """``volume_joint_dc_reference.edm_chain`` with ``project_profile64`` between the fuse and the update."""
    with _projection(table):
        return DC.edm_chain(vol, cfg, tabs, blend, dynamic, meas_up, cell, w, **kw)


def edm_bound(tabs, L, cell, table, w, state_max, lowres_max, dynamic, scale):
    """``volume_joint_dc_reference.edm_bound`` with this projection's count: ((n + 4) G + 1) 2^-24 ``scale`` is
    ``scale`` ((n + 4) G + 1) / 2 further local terms of 2^-23."""
    terms = profile_roundings(cell, table, w, scale) / 2.0 ** -23
    return E.chain_bound(tabs, L['windows_per_voxel'] + math.ceil(terms), state_max, lowres_max, dynamic, False)
