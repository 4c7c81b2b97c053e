"""Specification of data-consistent sampling for a tile-local linear operator (``consistency_operator=`` of the samplers and of
``VolumeInference``) in plain numpy, on top of tests/volume_joint_dc_reference.py.  Not a test module:
tests/test_volume_tile_host.py and tests/test_gpu_volume_tile.py import it.

The operator.  The volume splits into disjoint tiles of (fz, fy, fx) voxels, n = fz fy fx, q the lexicographic (z, y, x) index of a
voxel inside its tile; every tile is measured by the same m x n matrix A.  x0' = x0 + w A+(y - A x0) = x0 + w (t - P x0) with t = A+ y
on the high-res grid and P = A+ A, the orthogonal projector onto the row space of A.  ``stack_matrix`` restates ``ops.stack_operator``
and ``projector`` restates ``ops.tile_projector`` (numpy's SVD, the same thresholds).  The fp32 table P that the arithmetic reads is
taken from ``ops.tile_operator`` itself, and the float64 side takes the SAME table, widened: the rounding of the table defines the
operator, it is not an error of the arithmetic.  (Two SVD libraries agree to about 1e-15, not to the bit; the host tests compare the
table with ``projector`` at 1e-7 and check its exact properties.)

The projection (include/diqt.h, above ``diqt_tile_measure``), over one tile, a the clamped values:
    s = 0;  s = fma(P[r][q], a[r], s) for r = 0 .. n - 1;  a'[q] = fma(w, t[q] - s, a[q]).

Two restatements, as in the uniform module:
  * fp32, for the bit-exact tests: ``apply32`` / ``project_tile32`` with exactly that order, ``joint_step_tile32`` (the three updates
    of ``volume_joint_dc_reference.joint_step32`` behind this projection), ``measure32`` (s = fma(A[row][r], x[r], s) in the order of
    r) and ``backproject32`` (s = fma(A+[q][row], y[row], s) in row order), A and A+ rounded to fp32;
  * float64, for the chain tests: ``project_tile64`` and ``vp_chain`` / ``edm_chain``, that module's chains with it between the fuse
    and the update.

The rounding count of one projection, ``tile_roundings``: ((n + 1) G + 2) 2^-24 S with G = ``gain`` = max_q sum_r |P[q][r]| (>= 1, since
P 1 = 1) and S the largest of |a|, |t| and |a'| in the tile.  It is ``volume_joint_dc_reference.projection_roundings``, (n + 3) 2^-24 S,
with G multiplying the n-term sum.  To first order in 2^-24:
  * the n fma roundings of the sum, each on a partial sum of magnitude <= sum_r |P[r][q]| |a[r]| <= G S: n G 2^-24 S on s;
  * the subtraction r = t - s rounds r, |r| <= (1 + G) S: (1 + G) 2^-24 S more;
  * the fma rounds a', |a'| <= S: 2^-24 S; the weight w <= 1 only shrinks what r carries.
Together (n G + (1 + G) + 1) 2^-24 S; G = 1 gives the uniform count.  The chain bounds are the uniform families' bounds plus ``steps``
times that number; for the EDM recursion it enters as S ((n + 1) G + 2) / 2 further local terms of 2^-23 (``edm_bound``).  It is not
tuned against the device.

The guarantee at w = 1, u = 2^-24, norms = largest absolute row sum.  The device's x0' is the exact projection a + t~ - P~ a plus
e_proj = ``tile_roundings``, with P~ = P + E the fp32 table (|E| <= u per entry, so |E a| <= n u S =: e_table) and t~ = t + d the
device's target: the back-projection's m fma roundings on partial sums <= |A+| Ymax and the rounding of A+ to fp32, (m + 1) u |A+| Ymax
in raw units, divided by std, plus the two roundings of the z-score, 2 u S (``target_roundings`` =: e_t).
  * A x0' - y (``residual_bound_A``; y = fl(A32 x) simulated by ``tile_measure`` from values <= Xmax, so y = A x + h with
    |h| <= 2 n u |A| Xmax / std =: e_y, the n fma roundings and the rounding of A, of which (I - A A+) h stays):
    A (a + t - P a) = A t = A A+ y, hence |A x0' - y| <= |A| (e_proj + e_table + e_t) + (1 + |A| |A+|) e_y.
  * P~ x0' - t~ for ANY y, also stacks that contradict each other (``residual_bound_P``): P~ P~ - P~ = P E + E P - E + O(u^2) and
    P~ t~ - t~ = (P - I) d + E t~, hence |P~ x0' - t~| <= G e_proj + (2 G + 1) e_table + (1 + G) e_t + e_table.
"""
import math

import numpy as np

from tests import edm_dpmpp2m_reference as E
from tests import volume_joint_dc_reference as DC
from tests.volume_joint_dc_reference import _cells, clamp32, fma32, fuse32, replicate   # noqa: F401  (the tests take them from here)


def stack_matrix(cell, axes):
    """``ops.stack_operator``'s A: per axis of ``axes`` one row per line of the tile along it, the lines in lexicographic order of their
    other two coordinates, weight 1 / f_axis on the line's voxels.  float64 [m, n]."""
    n = cell[0] * cell[1] * cell[2]
    q = np.arange(n).reshape(cell)
    rows = []
    for a in axes:
        for line in np.moveaxis(q, a, -1).reshape(-1, cell[a]):
            r = np.zeros(n)
            r[line] = 1.0 / cell[a]
            rows.append(r)
    return np.array(rows)


def dense_matrix(cell, m, seed):
    """A random dense m x n operator whose first row is the constant 1 / n (so the tile mean is measured)."""
    n = cell[0] * cell[1] * cell[2]
    A = np.random.default_rng(seed).standard_normal((m, n))
    A[0] = 1.0 / n
    return A


def projector(A):
    """``ops.tile_projector`` in numpy: float64 (A+, P symmetrised, rank); a singular value is zero at or below 1e-10 s_max."""
    U, S, Vh = np.linalg.svd(np.asarray(A, dtype=np.float64), full_matrices=False)
    keep = S / S[0] > 1e-10
    pinv = (Vh[keep].T / S[keep]) @ U[:, keep].T
    P = pinv @ A
    return pinv, (P + P.T) / 2, int(keep.sum())


# the tiles of the tests: (cell, axes of the stacks) or (cell, ('dense', m, seed))
OPERATORS = {
    'stacks-222': ((2, 2, 2), (0, 1, 2)),                    # m = 12 > n = 8
    'stacks-421': ((4, 2, 1), (0, 1)),
    'stack-411': ((4, 1, 1), (0,)),                          # one row: the uniform operator in other roundings
    'stacks-135': ((1, 3, 5), (1, 2)),                       # n = 15: ragged boxes
    'dense-232': ((2, 3, 2), ('dense', 5, 11)),
    'stacks-444': ((4, 4, 4), (0, 1, 2)),                    # n = 64: the full table, the longest sum
}


def matrix_of(name):
    cell, how = OPERATORS[name]
    return cell, dense_matrix(cell, *how[1:]) if how[0] == 'dense' else stack_matrix(cell, how)


# ---- fp32 ---------------------------------------------------------------------------------------------------------------------------------
def tiles(a, cell):
    """[..., D, H, W] -> [..., D/fz, H/fy, W/fx, n], the last axis in lexicographic (z, y, x) order (a copy)."""
    c = _cells(a, cell)
    nd = c.ndim
    c = c.transpose(list(range(nd - 6)) + [nd - 6, nd - 4, nd - 2, nd - 5, nd - 3, nd - 1])
    return c.reshape(c.shape[:-3] + (cell[0] * cell[1] * cell[2],))


def untile(t, cell):
    """The inverse of ``tiles``."""
    c = t.reshape(t.shape[:-1] + tuple(cell))
    nd = c.ndim
    c = c.transpose(list(range(nd - 6)) + [nd - 6, nd - 3, nd - 5, nd - 2, nd - 4, nd - 1])
    return c.reshape(c.shape[:-6] + tuple(s * f for s, f in zip((c.shape[-6], c.shape[-4], c.shape[-2]), cell)))


def apply32(a, cell, table):
    """s = P a of every tile of a [..., D, H, W] in float32: per voxel q, s = 0; s = fma(P[r][q], a[r], s) for r in order."""
    t = tiles(np.asarray(a, dtype=np.float32), cell)
    table = np.asarray(table, dtype=np.float32)
    s = np.zeros(t.shape, dtype=np.float32)
    for r in range(t.shape[-1]):
        s = fma32(table[r], t[..., r:r + 1], s)
    return untile(s, cell)


def project_tile32(a, target, cell, table, w, covered=None):
    """The projection of a [..., D, H, W] (already clamped) in float32.  ``covered`` (bool [D,H,W]): only the tiles whose voxels are
    ALL covered are corrected, the others keep their values."""
    a = np.asarray(a, dtype=np.float32)
    out = fma32(np.float32(w), np.asarray(target, dtype=np.float32) - apply32(a, cell, table), a)
    if covered is None:
        return out
    whole = replicate(_cells(covered, cell).all(axis=(-5, -3, -1)), cell)
    return np.where(whole, out, a)


def joint_step_tile32(y, slot, taps, stride, x_t, x0_prev, target, cell, table, w, form, kx, k0, kp, kn, clamp, n, fused=None):
    """What ``diqt_volume_joint_consistent_tile_step`` computes, bit for bit: (x_next, x0_out, covered) --
    ``volume_joint_dc_reference.joint_step32`` with ``project_tile32`` in the place of ``project32``; the update's operation order is
    restated from there."""
    f32 = np.float32
    x_t = np.asarray(x_t, dtype=f32)
    x0, covered = fused if fused is not None else fuse32(y, slot, taps, stride, x_t.shape, clamp)
    x0 = project_tile32(x0, target, cell, table, w, covered)
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


def measure32(x, cell, A):
    """``ops.tile_measure``: float32 [m, D/fz, H/fy, W/fx], s = fma(A[row][r], x[r], s) in the order of r, A rounded to fp32."""
    t = tiles(np.asarray(x, dtype=np.float32), cell)
    A = np.asarray(A, dtype=np.float64).astype(np.float32)
    s = np.zeros((A.shape[0],) + t.shape[:-1], dtype=np.float32)
    for r in range(t.shape[-1]):
        s = fma32(A[:, r].reshape(-1, 1, 1, 1), t[None, ..., r], s)
    return s


def backproject32(y, cell, pinv):
    """``ops.tile_backproject``: float32 [D,H,W], t[q] = the chain s = fma(A+[q][row], y[row], s) in row order, A+ rounded to fp32."""
    y = np.asarray(y, dtype=np.float32)
    Ap = np.asarray(pinv, dtype=np.float64).astype(np.float32)
    s = np.zeros(y.shape[1:] + (Ap.shape[0],), dtype=np.float32)
    for row in range(y.shape[0]):
        s = fma32(Ap[:, row], y[row][..., None], s)
    return untile(s, cell)


def target_state(y, cell, pinv, cfg):
    """t as the chains read it: back-projected in fp32, z-scored in float32 (one subtraction, one division), widened."""
    mean32, std32 = np.float32(cfg['Data']['mean']), np.float32(cfg['Data']['std'])
    return ((backproject32(y, cell, pinv) - mean32) / std32).astype(np.float64)


# ---- float64 ------------------------------------------------------------------------------------------------------------------------------
def apply64(x, cell, table):
    """P x of every tile in float64, P the fp32 table widened."""
    return untile(tiles(np.asarray(x, dtype=np.float64), cell) @ np.asarray(table, dtype=np.float64), cell)   # P is symmetric


def measure64(x, cell, A):
    """A x of every tile in float64: [m, D/fz, H/fy, W/fx]."""
    return np.moveaxis(tiles(np.asarray(x, dtype=np.float64), cell) @ np.asarray(A, dtype=np.float64).T, -1, 0)


def project_tile64(x0, covered, target, cell, w, table):
    """x0 + w (t - P x0) on the tiles whose voxels are all covered, in float64: (x0', whole)."""
    whole = replicate(_cells(covered, cell).all(axis=(-5, -3, -1)), cell)
    return np.where(whole, x0 + w * (target - apply64(x0, cell, table)), x0), whole


def gain_of(table):
    return float(np.abs(np.asarray(table, dtype=np.float64)).sum(axis=1).max())


def tile_roundings(cell, table, scale):
    """The projection's own fp32 roundings on one x0 (module docstring): ((n + 1) G + 2) 2^-24 S, G = max_q sum_r |P[q][r]|."""
    n = cell[0] * cell[1] * cell[2]
    return ((n + 1) * gain_of(table) + 2) * 2.0 ** -24 * scale


class _projection:
    """``volume_joint_dc_reference``'s chains call its ``project64`` between the fuse and the update; inside this context that name
    is ``project_tile64`` with the table, so the chains below ARE those chains, nothing restated."""

    def __init__(self, table):
        self.table = table

    def __enter__(self):
        self.saved = DC.project64
        DC.project64 = lambda x0, covered, meas_up, cell, w: project_tile64(x0, covered, meas_up, cell, w, self.table)

    def __exit__(self, *exc):
        DC.project64 = self.saved


def vp_chain(vol, cfg, coefs, log_snr, clamp, blend, target, cell, table, w, **kw):
    """``volume_joint_dc_reference.vp_chain`` with ``project_tile64`` between the fuse and the update."""
    with _projection(table):
        return DC.vp_chain(vol, cfg, coefs, log_snr, clamp, blend, target, cell, w, **kw)


def edm_chain(vol, cfg, tabs, blend, dynamic, target, cell, table, w, **kw):
    """``volume_joint_dc_reference.edm_chain`` with ``project_tile64`` between the fuse and the update."""
    with _projection(table):
        return DC.edm_chain(vol, cfg, tabs, blend, dynamic, target, cell, w, **kw)


def edm_bound(tabs, L, cell, table, state_max, lowres_max, dynamic, scale):
    """``volume_joint_dc_reference.edm_bound`` with this projection's count: ((n + 1) G + 2) 2^-24 ``scale`` is
    ``scale`` ((n + 1) G + 2) / 2 further local terms of 2^-23."""
    terms = tile_roundings(cell, table, scale) / 2.0 ** -23
    return E.chain_bound(tabs, L['windows_per_voxel'] + math.ceil(terms), state_max, lowres_max, dynamic, False)


def _norm(M):
    return float(np.abs(np.asarray(M, dtype=np.float64)).sum(axis=1).max())


def target_roundings(pinv, y_max, std, scale):
    """e_t of the module docstring: what the device's z-scored t = A+ y carries, in state units."""
    m = np.asarray(pinv).shape[1]
    return ((m + 1) * _norm(pinv) * y_max / std + 2 * scale) * 2.0 ** -24


def residual_bound_A(cell, table, A, pinv, y_max, x_max, std, scale):
    """|A x0' - y| at w = 1 for a y simulated by ``tile_measure`` (module docstring)."""
    n, u = cell[0] * cell[1] * cell[2], 2.0 ** -24
    e_y = 2 * n * u * _norm(A) * x_max / std
    return _norm(A) * (tile_roundings(cell, table, scale) + n * u * scale + target_roundings(pinv, y_max, std, scale)) + \
        (1 + _norm(A) * _norm(pinv)) * e_y


def residual_bound_P(cell, table, pinv, y_max, std, scale):
    """|P x0' - t| at w = 1 for any y, P and t as the device holds them (module docstring)."""
    n, u, G = cell[0] * cell[1] * cell[2], 2.0 ** -24, gain_of(table)
    return G * tile_roundings(cell, table, scale) + (2 * G + 2) * n * u * scale + (1 + G) * target_roundings(pinv, y_max, std, scale)
