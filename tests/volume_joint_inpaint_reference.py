"""Float64 specification of ``VolumeInference(joint=True, inpaint=(known, mask), inpaint_resample_times=R)`` with an EDM Heun denoiser, in
plain numpy: ``volume_joint_heun_reference``'s chain (its tables, fuse, phases, stub and normals) with the RePaint loop of
``ElucidatedImagen.one_unet_sample`` (elucidated_imagen.py:473-530) on the one state.  Not a test module: the host and GPU tests of the
inpainting volume path import it, with the shared known volume / mask and the derived bound.

Every step runs R passes, r = R - 1 .. 0.  A pass: the known volume under the mask and the churn (``xh = sel(m, known, x) + kc n``), the
two fused evaluations with predictor and corrector as in ``volume_joint_heun_reference``, and -- unless r == 0 or it is the last step --
the re-noise ``x += (sigma - sigma_next) n``.  The step that ends at sigma 0 has no corrector: its passes are predictor, paste, churn.
After the chain: clamp(-1, 1), the known values under the mask, then fill and background as in every mode.

Draw numbering of the anchored field: draw 0 is the low-res augmentation noise, draw 1 the initial image, and ONE counter starting at 2
advances as ``sample(noise=source, inpaint_images=...)`` calls its source per window: per pass the eps (also where kc == 0) and, where the
pass re-noises, that normal -- the re-noise of pass r before the eps of pass r - 1.

``chain_bound`` extends ``volume_joint_heun_reference.chain_bound`` by the same rounding counts: the recursion runs per pass; a churn
adds kc eps_n + 2 u (M + 6 kc), a re-noise kr eps_n + 2 u (M + 6 kr) (one product and one sum on a value <= M + 6 k, and the normal's
own distance); a paste adds nothing (the known values are the same fp32 numbers on both sides -- a masked voxel restarts at error 0, which
the bound does not even use).
"""
import numpy as np

from tests import volume_blend_reference as R
from tests import volume_joint_heun_reference as HN
from tests import volume_joint_reference as J

SEED = HN.SEED
EPS_N, U = HN.EPS_N, HN.U


def inpaint_inputs(shape=(40, 36, 44), seed=7, box=((10, 30), (5, 27), (24, 40)), scattered=0.1):
    """The shared (known fp32 [D,H,W] in [-1, 1], mask bool [D,H,W]) for ``volume_blend_reference.shared_volume()``: a box inside its
    non-zero part that crosses window borders at strides 16, 8 and 5 of the 16-voxel windows, plus about 10 % scattered voxels."""
    rng = np.random.default_rng(seed)
    known = rng.uniform(-1.0, 1.0, size=shape).astype(np.float32)
    mask = rng.uniform(size=shape) < scattered
    mask[tuple(slice(lo, hi) for lo, hi in box)] = True
    return known, mask


def pass_plan(T, resample):
    """The passes of a chain in order, as (i, r, more, renoise): ``more`` -- another pass follows (this one's end churns for it);
    ``renoise`` -- the pass re-noises (r > 0 and not the last step)."""
    return [(i, r, r > 0 or i + 1 < T, r > 0 and i + 1 < T) for i in range(T) for r in reversed(range(resample))]


def joint_chain(vol, cfg, tabs, blend, dynamic, known, mask, resample=1, seed=SEED, sample=0, self_cond=False, dtype=np.float64,
                net=HN.stub64):
    """One sample's joint inpainting chain, before the finish, in ``dtype``.  Returns the final state [D,H,W], the layout, the largest
    |state| met on covered voxels and the number of draws of the state (after draw 0)."""
    dt = np.dtype(dtype).type
    vol = np.asarray(vol, dtype=np.float32)
    L = J.layout(vol, cfg)
    P, sub, stride, kept, slot = L['P'], L['sub'], L['stride'], L['kept'], L['slot']
    mean32, std32 = np.float32(cfg['Data']['mean']), np.float32(cfg['Data']['std'])
    shape = vol.shape
    known = np.asarray(known, dtype=np.float32).astype(dtype)
    alpha, sigma_lr = (dt(v) for v in tabs['lowres'])
    normal = lambda k: J.normals(shape, seed, k, sample).astype(dtype)
    low = alpha * ((vol - mean32) / std32).astype(dtype) + sigma_lr * normal(0)
    taps = R.taps_of(P, blend)
    coefs, pre, sched = tabs['coefs'], tabs['pre'], tabs['sched']
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
            pred = J.dynamic_threshold_rows(pred, HN.PERCENTILE, 1.0).astype(dtype) if dynamic else np.clip(pred, dt(-1), dt(1))
            y[r] = (R.merge_block(pred, P) if L['block'] else pred).reshape(P, P, P)
        return HN.fuse(y, slot, taps, stride, shape, dtype)

    draw = [1]

    def take():
        draw[0] += 1
        return draw[0] - 1

    def paste_churn(x, kc):
        u = np.where(mask, known, x)
        k = take()                                                                       # the eps is drawn also where kc == 0
        return u + dt(kc) * normal(k) if kc != 0 else u

    xh = paste_churn(dt(tabs['sigma0']) * normal(take()), coefs[0, 0])
    x0, corrected = None, False
    for i, r, more, renoise in pass_plan(T, resample):
        _, a1, b1, a2, b2, c2, d2 = (dt(v) for v in coefs[i])
        x0, covered = evaluate(xh, i, 0, x0)
        xn, x0 = HN.heun_phase1(x0, covered, xh, a1, b1)
        state_max = max(state_max, float(np.abs(xh[covered]).max()), float(np.abs(xn[covered]).max()))
        corrected = sched[i, 1] != 0
        kc = (coefs[i, 0] if r > 0 else coefs[i + 1, 0]) if more else 0.0
        if not corrected:
            assert not renoise, "a step that ends at sigma 0 before the last one"
            if more:
                xh = paste_churn(xn, kc)                                                 # every voxel: an uncovered one holds xn = xh
            continue
        x0b, covered = evaluate(xn, i, 1, x0)
        x = (a2 * xh + b2 * x0 + c2 * xn) + d2 * x0b
        if renoise:
            x = x + dt(np.float32(sched[i, 0] - sched[i, 1])) * normal(take())           # kr as the device holds it
        x = paste_churn(x, kc) if more else np.where(mask, known, x)
        xh, x0 = np.where(covered, x, xh), x0b
    return (xh if corrected else xn), L, state_max, draw[0] - 1


def joint_reference(vol, cfg, tabs, blend, dynamic, known, mask, resample=1, seed=SEED, samples=1, self_cond=False, dtype=np.float64):
    """``VolumeInference(cfg, elu.window_denoiser(), blend=blend, noise='anchored', joint=True, samples=samples, seed=seed,
    inpaint=(known, mask), inpaint_resample_times=resample)(vol, return_std=samples > 1)``: the chains, clamp(-1, 1), the known values,
    fill, background, mean / deviation over the samples.  A dict like ``volume_joint_heun_reference.joint_reference``'s plus ``mask``
    and ``draws``."""
    vol = np.asarray(vol, dtype=np.float32)
    known32 = np.asarray(known, dtype=np.float32)
    mean32, std32 = np.float32(cfg['Data']['mean']), np.float32(cfg['Data']['std'])
    fill, min_val = (np.float32(0.) - mean32) / std32, (vol.min() - mean32) / std32
    finals, state_max = [], 0.0
    for s in range(samples):
        x, L, m, draws = joint_chain(vol, cfg, tabs, blend, dynamic, known32, mask, resample, seed, s, self_cond, dtype)
        finals.append(np.where(mask, known32.astype(np.float64), np.clip(x.astype(np.float64), -1.0, 1.0)))
        state_max = max(state_max, m)
    covered = R.blend_accumulate(np.zeros((1, L['kept'].shape[0], L['P'], L['P'], L['P'])), L['slot'], np.ones(L['P']), L['stride'],
                                 vol.shape)[2]
    background = ((vol - mean32) / std32) == np.float32(min_val)
    r = np.stack([np.where(background, np.float64(min_val), np.where(covered, f, np.float64(fill))) for f in finals])
    std = r.std(axis=0, ddof=1) if samples > 1 else np.zeros(vol.shape)
    lowres_max = tabs['lowres'][0] * float(np.abs((vol - mean32) / std32).max()) + 6 * tabs['lowres'][1]
    return dict(mean=r.mean(axis=0), std=std, covered=covered, background=background, fill=fill, min_val=min_val, mask=np.asarray(mask),
                windows_per_voxel=L['windows_per_voxel'], kept=L['kept'].shape[0], candidates=L['slot'].size, state_max=state_max,
                lowres_max=lowres_max, draws=draws,
                bound=chain_bound(tabs, L['windows_per_voxel'], state_max, lowres_max, resample, dynamic, self_cond))


def chain_bound(tabs, windows_per_voxel, state_max, lowres_max, resample=1, dynamic=False, self_cond=False):
    """``volume_joint_heun_reference.chain_bound``'s recursion per pass, with the churn and re-noise terms of the module docstring."""
    M, coefs, pre, sched = state_max, tabs['coefs'], tabs['pre'], tabs['sched']
    alpha, sigma_lr = tabs['lowres']
    blend = R.tolerance(windows_per_voxel, 1.0)
    k = 2.0 if dynamic else 1.0

    def denoiser(i, stage):
        _, cin, cskip, cout, cnoise = pre[i][stage]
        fmax = 0.5 + 0.25 * lowres_max + abs(cnoise) / 64 + 0.125
        local = U * (0.5 * cout * cin * M + 8 * cout * fmax + 2 * (cskip * M + cout * fmax)) \
            + 0.25 * cout * (3 * U * lowres_max + sigma_lr * EPS_N)
        local = k * local + (4 * U if dynamic else 0.0)
        return k * (cskip + 0.5 * cout * cin), (k * cout / 8 if self_cond else 0.0), local + blend

    noise = lambda kn: kn * EPS_N + 2 * U * (M + 6 * kn)                                  # x + kn n: a churn or a re-noise
    kc0, s0 = abs(coefs[0, 0]), tabs['sigma0']
    e_h = (s0 + kc0) * EPS_N + U * (6 * s0 + 2 * (6 * s0 + 6 * kc0))
    e_sc = e_end = 0.0
    for i, r, more, renoise in pass_plan(coefs.shape[0], resample):
        _, a1, b1, a2, b2, c2, d2 = np.abs(coefs[i])
        kc = abs(coefs[i, 0] if r > 0 else coefs[i + 1, 0]) if more else 0.0
        L0, S0, local0 = denoiser(i, 0)
        e_0 = L0 * e_h + S0 * e_sc + local0
        e_n = a1 * e_h + b1 * e_0 + 2 * U * (a1 * M + b1)
        e_sc = e_0
        if sched[i, 1] == 0:
            e_end = e_n
            e_h = e_n + noise(kc)
            continue
        L1, S1, local1 = denoiser(i, 1)
        e_0b = L1 * e_n + S1 * e_sc + local1
        e_x = a2 * e_h + b2 * e_0 + c2 * e_n + d2 * e_0b + 4 * U * ((a2 + c2) * M + b2 + d2)
        if renoise:
            e_x += noise(abs(float(np.float32(sched[i, 0] - sched[i, 1]))))
        e_end = e_x
        e_h = e_x + noise(kc)
        e_sc = e_0b
    return e_end
