"""Specification of data-consistent sampling (``consistency=`` of the samplers and of ``VolumeInference``) in plain numpy, on top of
tests/volume_joint_reference.py.  Not a test module: tests/test_volume_dc_host.py and tests/test_gpu_volume_dc.py import it.

The projection (include/diqt.h, above ``diqt_cell_mean``).  A cell is (fz, fy, fx) voxels, n = fz fy fx; over one cell, with the
measurement replicated onto the high-res grid (``meas_up``),
    s = 0;  s = s + a[v] in lexicographic (z, y, x) order;  m = s / n;  a'[v] = fma(w, meas_up[v] - m, a[v]).

Two restatements:
  * fp32, for the bit-exact tests: ``project32`` / ``cell_mean32`` with exactly that order, ``fuse32`` (the window walk of the joint
    kernels: num = fma(w, c(y), num), den = den + w over the covering kept windows in candidate order, w = (t_i t_j) t_k, then num / den)
    and ``joint_step32`` (the three updates of ``volume_joint_linear_kernel`` behind the projection).  numpy's float32 +, -, * and / are
    IEEE, correctly rounded; the fused multiply-add is ``fma32``: the exact product in float64 (48 bits), the sum brought to 53 bits
    with round-to-odd (Boldo and Melquiond 2008), then ONE rounding to float32 -- 53 >= 2 x 24 + 2, so the result is the correctly
    rounded fma.  Nothing is left out of a comparison: the existing joint tests have no fp32 reference that flags ambiguous voxels, so
    this one flags none.  The anchored normals are taken from the device (``ops.volume_joint_init``, bit for bit the field).
  * float64, for the chain tests: ``vp_chain`` (ddim, ddpm and dpmpp2m of the DDPM family) and ``edm_chain`` (DPM-Solver++ 2M in sigma
    space, ODE and SDE): ``volume_joint_reference.joint_chain`` / ``edm_dpmpp2m_reference.joint_chain`` with ``project64`` between the
    fuse and the update, and the fused x0 that self-conditioning and the history term see replaced by the projected one.

Bound of the chain tests, u = 2^-24.  The existing joint tests allow a chain the ``chain_bound`` of its family: per step a count of
fp32 operations, each 2^-23 of the largest magnitude compared (``volume_joint_reference.chain_bound``,
``dpmpp2m_reference.chain_bound``), or the recursion of ``edm_dpmpp2m_reference.chain_bound``.  The projection adds its own roundings
to the x0 of every step.  With S the largest of |a|, |meas_up| and |a'| in the cell, to first order in u:
  * the n sequential additions of s: at most (n - 1) u sum|a| <= (n - 1) u n S (the usual bound), so (n - 1) u S on m after the
    division by n;
  * the division s / n rounds m, |m| <= S: u S;
  * the subtraction r = meas_up - m rounds r, |r| <= 2 S: 2 u S;
  * the fma rounds the result a': u S.
Together (n + 3) u S.
``projection_roundings(cell, S)`` is that number, with S = the largest of |x0|, |x0'| and |meas_up| met in the chain.  The chain tests add
``steps`` times it to the family's bound (which does not follow the step coefficients either: it charges every step at the largest
magnitude).  For the EDM family, whose bound is a recursion with a per-step local term for the blend, (windows + 3) 2^-23 at |D| <= 1,
the same number enters as S (n + 3) / 2 further such terms (``edm_bound``).  The guarantee tests use it once, for the last step.  None
of these factors was tuned against the device: on the MI355X the chains sit at 1 - 2 % of their bounds.
"""
import math

import numpy as np

from tests import edm_dpmpp2m_reference as E
from tests import volume_blend_reference as R
from tests import volume_joint_heun_reference as HN
from tests import volume_joint_reference as J


# ---- fp32 ---------------------------------------------------------------------------------------------------------------------------------
def fma32(a, b, c):
    """fl32(a b + c) with ONE rounding, elementwise on float32 arrays."""
    a, b, c = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in np.broadcast_arrays(a, b, c))
    p = a * b                                                       # exact: 24 + 24 bits
    s = p + c                                                       # rounded to nearest at 53 bits, error e (TwoSum)
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    with np.errstate(invalid='ignore'):
        inexact = (e != 0) & np.isfinite(s)
    # round to odd: the truncated sum with its last bit forced to 1 whenever the sum was inexact
    away = inexact & ((e > 0) == (s > 0))                           # |exact| > |s|: s is the truncation already
    t = np.where(inexact & ~away, np.nextafter(s, 0.0), s)
    bits = t.view(np.int64) | inexact.astype(np.int64)
    return bits.view(np.float64).astype(np.float32)


def clamp32(lo, hi, mode):
    """``StepClamp``: mode 0 max(y, lo), mode 1 min(max(y, lo), hi), mode 2 / None the identity, on float32."""
    if mode in (2, None):
        return lambda v: v
    lo, hi = np.float32(lo), np.float32(hi)
    return (lambda v: np.maximum(v, lo)) if mode == 0 else (lambda v: np.minimum(np.maximum(v, lo), hi))


def _cells(a, cell):
    """[..., D, H, W] -> [..., D/fz, fz, H/fy, fy, W/fx, fx] (a view)."""
    fz, fy, fx = cell
    D, H, W = a.shape[-3:]
    assert D % fz == 0 and H % fy == 0 and W % fx == 0
    return a.reshape(a.shape[:-3] + (D // fz, fz, H // fy, fy, W // fx, fx))


def cell_mean32(a, cell):
    """m of every cell of a [..., D, H, W]: the sum in (z, y, x) order in float32, then ONE division by n."""
    fz, fy, fx = cell
    c = _cells(np.asarray(a, dtype=np.float32), cell)
    s = np.zeros(c.shape[:-6] + (c.shape[-6], c.shape[-4], c.shape[-2]), dtype=np.float32)
    for i in range(fz):
        for j in range(fy):
            for k in range(fx):
                s = s + c[..., :, i, :, j, :, k]
    return s / np.float32(fz * fy * fx)


def replicate(m, cell):
    """A+: every voxel of a cell holds the cell's value."""
    for axis, f in zip((-3, -2, -1), cell):
        m = np.repeat(m, f, axis=axis)
    return m


def project32(a, meas_up, cell, w, covered=None):
    """The projection of a [..., D, H, W] (already clamped) in float32.  ``covered`` (bool [D,H,W]): only the cells whose voxels are
    all covered are corrected, the others keep their values."""
    a = np.asarray(a, dtype=np.float32)
    m = replicate(cell_mean32(a, cell), cell)
    out = fma32(np.float32(w), np.asarray(meas_up, dtype=np.float32) - m, a)
    if covered is None:
        return out
    whole = replicate(_cells(covered, cell).all(axis=(-5, -3, -1)), cell)
    return np.where(whole, out, a)


def fuse32(y, slot, taps, stride, shape, clamp):
    """The window walk in float32: (x0, covered) with x0 = num / den on covered voxels and 0 elsewhere."""
    y = np.asarray(y, dtype=np.float32)
    t = np.asarray(taps, dtype=np.float32)
    P = t.shape[0]
    w3 = (t[:, None, None] * t[None, :, None]) * t[None, None, :]
    num, den = np.zeros(shape, dtype=np.float32), np.zeros(shape, dtype=np.float32)
    for g in np.ndindex(*slot.shape):                              # candidate order
        n = int(slot[g])
        if n < 0:
            continue
        box = tuple(slice(a * stride, a * stride + P) for a in g)
        num[box] = fma32(w3, clamp(y[n]), num[box])
        den[box] = den[box] + w3
    covered = den != 0
    with np.errstate(invalid='ignore', divide='ignore'):
        x0 = np.where(covered, num / den, np.float32(0))
    return x0.astype(np.float32), covered


def joint_step32(y, slot, taps, stride, x_t, x0_prev, meas_up, cell, w, form, kx, k0, kp, kn, clamp, n, fused=None):
    """What ``diqt_volume_joint_consistent_step`` computes, bit for bit: (x_next, x0_out, covered).  ``form`` 0: fma(kx, x, k0 x0') +
    kn n, the product added also when it is 0; 1 / 2: u = fma(kx, x, k0 x0') + kp prev, then u + kn n only when kn != 0 (form 1: never).
    ``n``: the float32 normals [D,H,W] of the step (read only where they enter); ``x0_prev`` None: zeros; ``fused``: what ``fuse32``
    returned for these windows and this clamp, when the caller has it already."""
    f32 = np.float32
    x_t = np.asarray(x_t, dtype=f32)
    x0, covered = fused if fused is not None else fuse32(y, slot, taps, stride, x_t.shape, clamp)
    x0 = project32(x0, meas_up, cell, w, covered)
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


STEP_VOL, STEP_P = (20, 18, 70), 8
STEP_TILINGS = ((4, 'gaussian'), (5, 'constant'))
STEP_CELLS = ((4, 1, 1), (1, 3, 1), (1, 1, 5), (2, 2, 2), (1, 1, 7))


def step_case(stride, kind):
    """The inputs of the bit-exact joint step tests: a (20, 18, 70) volume -- W crosses the 64-lane block, H is no multiple of the
    4-row block -- with one corner zeroed, so that the 5 % rule drops windows and leaves uncovered voxels inside; P = 8.  At stride 4
    rows 16, 17 and columns 68, 69 are covered by no window: cells (1, 3, 1) and (1, 1, 5) include partly covered cells, and
    (1, 1, 5) has a cell across x = 64."""
    rng = np.random.default_rng(100 * stride)
    raw = rng.integers(1, 1000, STEP_VOL).astype(np.float32)
    raw[:10, :9, :30] = 0
    L = J.layout(raw, R.shared_cfg(stride, P=STEP_P))
    N = L['kept'].shape[0]
    return dict(stride=stride, kind=kind, slot=L['slot'], N=N, taps=R.taps_of(STEP_P, kind).astype(np.float32),
                y=(rng.standard_normal((N, STEP_P, STEP_P, STEP_P)) * 2).astype(np.float32),
                x=(rng.standard_normal(STEP_VOL) * 3).astype(np.float32), prev=(rng.standard_normal(STEP_VOL) * 2).astype(np.float32),
                coarse=rng.standard_normal(STEP_VOL).astype(np.float32))


def step_meas(case, cell):
    """The replicated measurement of a step case for ``cell``: float32 [D,H,W], constant per cell."""
    c = case['coarse']
    return np.ascontiguousarray(replicate(c[::cell[0], ::cell[1], ::cell[2]], cell))


# ---- float64 ------------------------------------------------------------------------------------------------------------------------------
def project64(x0, covered, meas_up, cell, w):
    """x0 + w A+(y - A x0) on the cells whose voxels are all covered, in float64."""
    m = replicate(_cells(x0, cell).mean(axis=(-5, -3, -1)), cell)
    whole = replicate(_cells(covered, cell).all(axis=(-5, -3, -1)), cell)
    return np.where(whole, x0 + w * (meas_up - m), x0), whole


def projection_roundings(cell, scale):
    """The projection's own fp32 roundings on one x0 (module docstring): (n + 3) 2^-24 of the largest magnitude involved."""
    return (cell[0] * cell[1] * cell[2] + 3) * 2.0 ** -24 * scale


def measurement(vol, cell, seed=3):
    """A raw measurement for the volume ``vol``, float32 [D/fz, H/fy, W/fx]: uniform in [100, 500], which the shared configs
    (mean 300, std 200) z-score into [-1, 1] -- inside the clamp of every mode, and of magnitude <= 1 like the EDM predictions."""
    rng = np.random.default_rng(seed)
    coarse = rng.uniform(100.0, 500.0, tuple(s // f for s, f in zip(vol.shape, cell)))
    return coarse.astype(np.float32)


def measurement_state(meas, cell, cfg):
    """The measurement as the chains read it: replicated, z-scored in float32 (one subtraction, one division), widened."""
    mean32, std32 = np.float32(cfg['Data']['mean']), np.float32(cfg['Data']['std'])
    return ((replicate(np.asarray(meas, dtype=np.float32), cell) - mean32) / std32).astype(np.float64)


def vp_chain(vol, cfg, coefs, log_snr, clamp, blend, meas_up, cell, w, multistep=False, seed=J.SEED, sample=0, net=J.stub64):
    """One sample's consistent joint chain of the DDPM family (objective x_start, static clamp) in float64, before the finish:
    ``volume_joint_reference.joint_chain`` with the projection between the fuse and the update.  ``coefs`` [T,3]: rows (kx, k0, kn) of a
    first-order sampler (kn n(i + 1) added where kn != 0) or, ``multistep``, (kx, k0, kp) with the projected x0 of the step before.
    Returns (state, layout, the largest of |x0| and |x0'|, the cells corrected at the last step)."""
    vol = np.asarray(vol, dtype=np.float32)
    L = J.layout(vol, cfg)
    P, stride, kept, slot = L['P'], L['stride'], L['kept'], L['slot']
    mean32, std32 = np.float32(cfg['Data']['mean']), np.float32(cfg['Data']['std'])
    low = ((vol - mean32) / std32).astype(np.float64)
    taps, c = R.taps_of(P, blend), J.clamp_of(*clamp)
    cut = lambda a, o: a[o[0]:o[0] + P, o[1]:o[1] + P, o[2]:o[2] + P][None, None]
    rows = (lambda v: R.split_block(v, L['sub'])) if L['block'] else (lambda v: v)
    x = J.normals(vol.shape, seed, 0, sample).copy()
    prev, x0_max, whole = None, 0.0, None
    y = np.empty((kept.shape[0], P, P, P), dtype=np.float64)
    for i in range(coefs.shape[0]):
        for r, o in enumerate(kept):
            xw, lw = rows(cut(x, o)), rows(cut(low, o))
            pred = net(xw, lw, np.full(xw.shape[0], log_snr[i]), None)
            y[r] = (R.merge_block(pred, P) if L['block'] else pred).reshape(P, P, P)
        x0, _, covered, _ = R.blend_accumulate(c(y)[None], slot, taps, stride, vol.shape)
        x0_max = max(x0_max, float(np.abs(x0[covered]).max()))
        x0, whole = project64(np.where(covered, x0, 0.0), covered, meas_up, cell, w)
        x0_max = max(x0_max, float(np.abs(x0).max()))
        kx, k0, k2 = coefs[i]
        step = kx * x + k0 * x0
        if multistep:
            step = step + (k2 * prev if prev is not None else 0.0)
        elif k2 != 0:
            step = step + k2 * J.normals(vol.shape, seed, i + 1, sample)
        x, prev = np.where(covered, step, x), x0
    return x, L, x0_max, whole


def edm_chain(vol, cfg, tabs, blend, dynamic, meas_up, cell, w, seed=E.SEED, sample=0, net=HN.stub64):
    """``edm_dpmpp2m_reference.joint_chain`` (float64, no self-conditioning) with the projection between the fuse and the update."""
    vol = np.asarray(vol, dtype=np.float32)
    L = J.layout(vol, cfg)
    P, sub, stride, kept, slot = L['P'], L['sub'], L['stride'], L['kept'], L['slot']
    mean32, std32 = np.float32(cfg['Data']['mean']), np.float32(cfg['Data']['std'])
    alpha, sigma_lr = tabs['lowres']
    normal = lambda k: J.normals(vol.shape, seed, k, sample)
    low = alpha * ((vol - mean32) / std32).astype(np.float64) + sigma_lr * normal(0)
    taps = R.taps_of(P, blend)
    cut = lambda a, o: a[o[0]:o[0] + P, o[1]:o[1] + P, o[2]:o[2] + P][None, None]
    rows = (lambda v: R.split_block(v, sub)) if L['block'] else (lambda v: v)
    y = np.empty((kept.shape[0], P, P, P), dtype=np.float64)
    x = tabs['sigma0'] * normal(1)
    x0_vol, covered, state_max, x0_max, whole = None, None, 0.0, 0.0, None
    for i, row in enumerate(tabs['coefs']):
        _, cin, cskip, cout, cnoise = tabs['pre'][i]
        for r, o in enumerate(kept):
            xw, lw = rows(cut(x, o)), rows(cut(low, o))
            pred = E.threshold(cskip * xw + cout * net(cin * xw, lw, np.full(xw.shape[0], cnoise), None), dynamic)
            y[r] = (R.merge_block(pred, P) if L['block'] else pred).reshape(P, P, P)
        x0, covered = HN.fuse(y, slot, taps, stride, vol.shape)
        x0_max = max(x0_max, float(np.abs(x0[covered]).max()))
        x0, whole = project64(np.where(covered, x0, 0.0), covered, meas_up, cell, w)
        x0_max = max(x0_max, float(np.abs(x0).max()))
        state_max = max(state_max, float(np.abs(x[covered]).max()))
        x = np.where(covered, E.update(x, x0, x0_vol, tuple(row), normal(2 + i) if row[3] != 0 else None), x)
        x0_vol = x0
    return x, L, max(state_max, float(np.abs(x[covered]).max())), x0_max, whole


def finish(vol, cfg, finals, L):
    """``volume_joint_reference.joint_reference``'s end: fill, background, mean / deviation over the (already clamped) final states."""
    vol = np.asarray(vol, dtype=np.float32)
    mean32, std32 = np.float32(cfg['Data']['mean']), np.float32(cfg['Data']['std'])
    fill, min_val = (np.float32(0.) - mean32) / std32, (vol.min() - mean32) / std32
    covered = R.blend_accumulate(np.zeros((1, L['kept'].shape[0], L['P'], L['P'], L['P'])), L['slot'], np.ones(L['P']), L['stride'],
                                 vol.shape)[2]
    background = ((vol - mean32) / std32) == np.float32(min_val)
    r = np.stack([np.where(background, np.float64(min_val), np.where(covered, f, np.float64(fill))) for f in finals])
    std = r.std(axis=0, ddof=1) if len(finals) > 1 else np.zeros(vol.shape)
    return dict(mean=r.mean(axis=0), std=std, covered=covered, background=background, fill=fill, min_val=min_val,
                windows_per_voxel=L['windows_per_voxel'], scale=float(np.abs(r).max()))


def edm_bound(tabs, L, cell, state_max, lowres_max, dynamic, scale):
    """``edm_dpmpp2m_reference.chain_bound`` with the projection's roundings in the local term of every step.  That term holds the
    blend's (windows + 3) 2^-23, written for |D| <= 1; the projection's (n + 3) 2^-24 ``scale`` (``scale``: the largest of |x0|, |x0'|
    and |meas_up| in the chain) is ``scale`` (n + 3) / 2 further such terms."""
    n = cell[0] * cell[1] * cell[2]
    return E.chain_bound(tabs, L['windows_per_voxel'] + math.ceil(scale * (n + 3) / 2), state_max, lowres_max, dynamic, False)
