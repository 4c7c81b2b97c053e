"""Specification of data consistency for a k-space band limit (``consistency_band=`` of the samplers and of ``VolumeInference``) in
plain numpy, on top of tests/volume_joint_dc_reference.py.  Not a test module: tests/test_volume_band_host.py and
tests/test_gpu_volume_band.py import it.

The operator (include/diqt.h, above ``diqt_band_measure``).  The measurement is the central box of the k-space of the periodic domain,
weighted per axis by h_|k| and sampled on the low-res grid with an offset of delta voxels.

Three statements:
  * float64, INDEPENDENT of the tables: ``project_spec`` is ``ifftn(mask fftn(x)).real``; ``dense_A`` sums the complex exponentials of
    the kept FFT bins into the n x N matrix of an axis, ``dense_pinv`` is ``numpy.linalg.pinv`` of it.  ``measure64`` /
    ``backproject64`` / ``project64`` apply them along the three axes.
  * ``tables64``: the closed forms of ``ops.band_table`` (d, a, g per axis, float64), restated; rounded once to fp32 they must be the
    op's table bit for bit.
  * fp32, the ONE arithmetic definition of every pass: out[i] = acc after acc = 0; acc = fma32(T[idx(i, j)], v[j], acc) over ascending
    j (``pass32``), with ``volume_joint_dc_reference.fma32`` / ``fuse32``: ``measure32``, ``backproject32``, ``project32`` and
    ``joint_step32``.  P and A take their passes in the order z, y, x, A+ in the order x, y, z; an identity axis has no pass.

The rounding allowance of ONE projection, u = 2^-24 (``allowance``).  Per pass the accumulator is a length-N fused sum whose weights
have the absolute sum Lambda = sum_m |d[m]| (on the fp32 table): with inputs bounded by S' the usual bound of a recursive sum of N
terms is N u Lambda S', and one more u Lambda S' covers the rounding of every table entry from float64 (relative u each).  The input
of a later pass is bounded by the Lambdas of the passes before it times S, S the largest |r| = |t - a|, and its inherited error is
amplified by at most its own Lambda; to first order in u the three passes add up to
    u S Lambda_z Lambda_y Lambda_x ((N_z + 1) + (N_y + 1) + (N_x + 1)) = u S gain (N_z + N_y + N_x + 3)
over the active axes (an identity axis contributes neither a factor nor a term).  The subtraction r = t - a rounds once (u S,
amplified by at most the gain: it is inside the + 3 with room to spare, since an active axis has N >= 2), and the final fma rounds
x0' once: u |x0'|.  Together
    allowance = u S gain (sum of the active N + 3) + u |x0'|.
The fp32 restatement uses 0.4 - 10 % of it on the inputs of the GPU tests (tests/test_volume_band_host.py asserts a quarter and prints
the share).
The chain tests add ``steps`` times the allowance to the family's ``chain_bound``, as the slab's and the tile operator's do.
"""
import math
from contextlib import contextmanager

import numpy as np

from tests import volume_joint_dc_reference as DC

U = 2.0 ** -24


# ---- the axes of a case --------------------------------------------------------------------------------------------------------------------
def axes_of(shape, cell, band=None, offset=None):
    """Per axis (N, f, n, h, delta, active): h the normalised weights (h[0] = 1) or None on an identity axis."""
    band = (None, None, None) if band is None else band
    if offset is None:
        offset = (0.0, 0.0, 0.0)
    elif offset == 'centre':
        offset = tuple((f - 1) / 2 for f in cell)
    out = []
    for N, f, h, delta in zip(shape, cell, band, offset):
        n = N // f
        if h is None and f == 1:
            out.append(dict(N=N, f=f, n=n, h=None, delta=0.0, active=False))
            continue
        h = [1.0] * ((n - 1) // 2 + 1) if h is None else [float(v) / float(h[0]) for v in h]
        out.append(dict(N=N, f=f, n=n, h=h, delta=float(delta), active=True))
    return out


def bins(ax, weights):
    """The weight of every FFT bin of an axis (numpy's order): h_|k| (``weights``) or 1 on the kept bins, 0 elsewhere."""
    N = ax['N']
    if not ax['active']:
        return np.ones(N)
    k = np.abs(np.fft.fftfreq(N, 1.0 / N)).round().astype(int)
    h = np.array(ax['h'] + [0.0] * (N - len(ax['h'])))
    return h[k] if weights else (h[k] > 0).astype(np.float64)


# ---- float64, independent of the tables -----------------------------------------------------------------------------------------------------
def project_spec(x, axes):
    """P x over the last three axes: the FFT, the 0 / 1 mask of the kept bins, the inverse FFT."""
    m = bins(axes[0], False)[:, None, None] * bins(axes[1], False)[None, :, None] * bins(axes[2], False)[None, None, :]
    return np.fft.ifftn(m * np.fft.fftn(np.asarray(x, dtype=np.float64), axes=(-3, -2, -1)), axes=(-3, -2, -1)).real


def dense_A(ax):
    """The n x N matrix of one axis: A[s, j] = Re (1 / N) sum_k H_k exp(2 pi i k (s f + delta - j) / N) over the FFT bins."""
    N, f, n = ax['N'], ax['f'], ax['n']
    if not ax['active']:
        return np.eye(N)
    k = np.fft.fftfreq(N, 1.0 / N)
    H = bins(ax, True)
    pos = (np.arange(n) * f + ax['delta'])[:, None] - np.arange(N)[None, :]
    return (np.exp(2j * np.pi * pos[:, :, None] * k[None, None, :] / N) * H).sum(axis=2).real / N


def dense_pinv(ax):
    """``numpy.linalg.pinv`` of ``dense_A``.  The singular values of A are h_k / sqrt(f) on the kept frequencies -- at least
    1 / (64 sqrt(64)) under the rules of the input -- and zero on a dropped one or on the unpaired Nyquist bin of an even n, which
    float64 leaves at 1e-16 or so: the cut-off lies between the two."""
    return np.linalg.pinv(dense_A(ax), rcond=1e-9)


def _along(M, x, axis):
    return np.moveaxis(np.tensordot(M, np.asarray(x, dtype=np.float64), axes=([1], [axis])), 0, axis)


def measure64(x, axes):
    for a, ax in enumerate(axes):
        x = _along(dense_A(ax), x, a - 3)
    return x


def backproject64(y, axes):
    for a, ax in enumerate(axes):
        y = _along(dense_pinv(ax), y, a - 3)
    return y


def project64(a, t, axes, w, covered=None):
    """a + w P (t - a) in float64; ``covered``: the residual is 0 where nothing covers."""
    r = np.asarray(t, dtype=np.float64) - a
    if covered is not None:
        r = np.where(covered, r, 0.0)
    return a + w * project_spec(r, axes)


# ---- the closed forms of ops.band_table ------------------------------------------------------------------------------------------------------
def tables64(ax):
    """(d, a, g) of one axis in float64: ``ops.band_table``'s expressions, term for term."""
    N, f, n, h, delta = ax['N'], ax['f'], ax['n'], ax['h'], ax['delta']
    if not ax['active']:
        one = np.zeros(N)
        one[0] = 1.0
        return one, one, one
    kept = [k for k in range(1, len(h)) if h[k] > 0]
    w = 2.0 * math.pi / N
    d = np.zeros(N)
    for m in range(N // 2 + 1):
        s = 1.0
        for k in kept:
            s += 2.0 * math.cos(w * ((k * m) % N))
        d[m] = d[(N - m) % N] = s / N
    a, g = np.zeros(N), np.zeros(N)
    for m in range(N):
        sa = sg = 1.0
        for k in kept:
            c = math.cos(w * (((k * m) % N) + k * delta))
            sa += 2.0 * h[k] * c
            sg += 2.0 * c / h[k]
        a[m], g[m] = sa / N, sg / n
    return d, a, g


def tables32(axes):
    """Per axis (d, a, g) rounded once to float32, and the flat table of include/diqt.h."""
    tabs = [tuple(t.astype(np.float32) for t in tables64(ax)) for ax in axes]
    return tabs, np.concatenate([t for tab in tabs for t in tab])


def circulant(t, rows, cols, si, sj):
    """M[i, j] = t[(i si + j sj) mod N]."""
    N = t.shape[0]
    return t[(np.arange(rows)[:, None] * si + np.arange(cols)[None, :] * sj) % N]


def gain(axes, tabs):
    g = 1.0
    for ax, (d, _, _) in zip(axes, tabs):
        if ax['active']:
            g *= float(np.abs(d.astype(np.float64)).sum())
    return g


def allowance(axes, tabs, S, out_max):
    """The rounding allowance of one projection (module docstring)."""
    return U * S * gain(axes, tabs) * (sum(ax['N'] for ax in axes if ax['active']) + 3) + U * out_max


# ---- fp32: the definition --------------------------------------------------------------------------------------------------------------------
def pass32(T, v, axis, Nout, si, sj):
    """One pass along ``axis`` of the float32 array ``v``: out[i] = the fused sum over ascending j of T[(i si + j sj) mod N] v[j]."""
    v = np.moveaxis(np.asarray(v, dtype=np.float32), axis, 0)
    N, Nin = T.shape[0], v.shape[0]
    acc = np.zeros((Nout,) + v.shape[1:], dtype=np.float32)
    shape = (Nout,) + (1,) * (v.ndim - 1)
    i = np.arange(Nout)
    for j in range(Nin):
        acc = DC.fma32(T[(i * si + j * sj) % N].reshape(shape), v[j][None], acc)
    return np.moveaxis(acc, 0, axis)


def apply32(x, axes, tabs):
    """P x: the passes z, y, x with d."""
    for a, (ax, tab) in enumerate(zip(axes, tabs)):
        if ax['active']:
            x = pass32(tab[0], x, a - 3, ax['N'], 1, -1)
    return x


def measure32(x, axes, tabs):
    for a, (ax, tab) in enumerate(zip(axes, tabs)):
        if ax['active']:
            x = pass32(tab[1], x, a - 3, ax['n'], ax['f'], -1)
    return x


def backproject32(y, axes, tabs):
    for a in (2, 1, 0):
        if axes[a]['active']:
            y = pass32(tabs[a][2], y, a - 3, axes[a]['N'], -1, axes[a]['f'])
    return y


def project32(a, t, axes, tabs, w, covered=None):
    """The projection of ``a`` (already clamped, float32): r = t - a (0 where uncovered), c = P r, fma(w, c, a)."""
    a = np.asarray(a, dtype=np.float32)
    r = np.asarray(t, dtype=np.float32) - a
    if covered is not None:
        r = np.where(covered, r, np.float32(0)).astype(np.float32)
    return DC.fma32(np.float32(w), apply32(r, axes, tabs), a)


def joint_step32(fused, x_t, x0_prev, t, axes, tabs, w, form, kx, k0, kp, kn, n):
    """What the three calls of a joint step compute, bit for bit: (x_next, x0_out).  ``fused`` = ``fuse32``'s (x0, covered); the update
    is ``volume_joint_dc_reference.joint_step32``'s."""
    f32 = np.float32
    x_t = np.asarray(x_t, dtype=f32)
    a, covered = fused
    x0 = np.where(covered, project32(a, t, axes, tabs, w, covered), f32(0)).astype(f32)
    b = f32(k0) * x0
    if form == 0:
        c = f32(kn) * (np.asarray(n, dtype=f32) if kn != 0 else np.zeros(x_t.shape, dtype=f32))
        u = DC.fma32(f32(kx), x_t, b) + c
    else:
        prev = np.zeros(x_t.shape, dtype=f32) if x0_prev is None else np.asarray(x0_prev, dtype=f32)
        u = DC.fma32(f32(kx), x_t, b) + f32(kp) * prev
        if form == 2 and kn != 0:
            u = u + f32(kn) * np.asarray(n, dtype=f32)
    return np.where(covered, u, x_t).astype(f32), x0


# ---- the float64 chains ----------------------------------------------------------------------------------------------------------------------
@contextmanager
def band_chains(axes):
    """``volume_joint_dc_reference.vp_chain`` / ``edm_chain`` with the band's projection in the place of the cell mean's: inside, their
    ``meas_up`` argument is the target t = A+ y in state space (float64)."""
    def project(x0, covered, t, cell, w):
        return project64(x0, t, axes, w, covered), covered
    keep = DC.project64
    DC.project64 = project
    try:
        yield
    finally:
        DC.project64 = keep


def target_state(meas, axes, cfg):
    """The target as the chains read it: t = A+ y of the raw measurement, z-scored, float64 (the z-score commutes with A+: A+ 1 = 1)."""
    mean, std = float(np.float32(cfg['Data']['mean'])), float(np.float32(cfg['Data']['std']))
    return (backproject64(np.asarray(meas, dtype=np.float64), axes) - mean) / std


# ---- the cases of the GPU tests --------------------------------------------------------------------------------------------------------------
# (cell, edge, band, offset): cubes of edge 8, 12 and 16; an identity axis (y and x of the first and third, x of the fourth), weights, a
# dropped frequency, an offset, an even and an odd n
PROJECT_CASES = (
    ((2, 1, 1), 8, None, None),
    ((2, 2, 2), 12, ([1.0, 0.75, 0.5], None, [1.0, 0.0, 0.5]), 'centre'),
    ((4, 1, 1), 16, ([1.0, 0.5], None, None), (1.5, 0.0, 0.0)),
    ((3, 2, 1), 12, (None, [1.0, 0.9], None), None),
    ((2, 2, 2), 16, None, (0.5, 0.0, 0.25)),
)
# the joint step: (volume, stride, taps) x cell; band and offset per cell.  (20, 18, 70): D at 20 < 32 = BAND_I, H = 18, W = 70 crosses
# BAND_C = BAND_J = 64; (12, 10, 132): W above 128, three j-panels, five output tiles; lines (D H = 120) that do not fill two blocks
STEP_VOLUMES = {'v20': ((20, 18, 70), 4, 'gaussian'), 'v12': ((12, 10, 132), 5, 'constant')}
STEP_CELLS = {(4, 1, 1): (None, None), (2, 1, 1): (([1.0, 0.5, 0.25], None, None), None), (2, 3, 1): (None, 'centre'),
              (4, 2, 2): ((None, [1.0, 0.8], None), (0.0, 0.5, 0.5)), (1, 1, 2): (None, None)}
STEP_P = 8
# every cell on every volume it divides ((2, 3, 1) does not divide H = 10)
STEP_CASES = [(name, cell) for name, (vol, _, _) in STEP_VOLUMES.items() for cell in STEP_CELLS if all(s % f == 0 for s, f in zip(vol, cell))]


def project_inputs(P, seed=11):
    """(x0, y) for B C = 3 cubes of edge P: float32 predictions of magnitude ~2 and, per cube, a high-res volume to be measured."""
    rng = np.random.default_rng(seed + P)
    return (rng.standard_normal((3, 1, P, P, P)) * 2).astype(np.float32), rng.standard_normal((3, 1, P, P, P)).astype(np.float32)


def step_case(name):
    """The inputs of the bit-exact joint step tests on ``STEP_VOLUMES[name]``: ``volume_joint_dc_reference.step_case``'s recipe on this
    shape -- one corner zeroed, so the 5 % rule drops windows and leaves uncovered voxels inside."""
    from tests import volume_blend_reference as R
    from tests import volume_joint_reference as J
    vol, stride, kind = STEP_VOLUMES[name]
    rng = np.random.default_rng(100 * stride + vol[0])
    raw = rng.integers(1, 1000, vol).astype(np.float32)
    raw[:vol[0] // 2, :vol[1] // 2, :vol[2] * 3 // 7] = 0
    L = J.layout(raw, R.shared_cfg(stride, P=STEP_P))
    N = L['kept'].shape[0]
    return dict(vol=vol, stride=stride, kind=kind, slot=L['slot'], N=N, taps=R.taps_of(STEP_P, kind).astype(np.float32),
                y=(rng.standard_normal((N, STEP_P, STEP_P, STEP_P)) * 2).astype(np.float32),
                x=(rng.standard_normal(vol) * 3).astype(np.float32), prev=(rng.standard_normal(vol) * 2).astype(np.float32),
                truth=rng.standard_normal(vol).astype(np.float32))
