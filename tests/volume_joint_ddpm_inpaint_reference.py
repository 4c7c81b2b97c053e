"""Float64 specification of ``VolumeInference(joint=True, inpaint=(known, mask), inpaint_resample_times=R)`` with the ancestral denoiser of
the DDPM family (``Imagen.window_denoiser(sampler='ddpm', sample_steps=K)``), in plain numpy: ``volume_joint_reference``'s chain (its
layout, fuse, stub and normals) with the RePaint loop of ``Imagen.p_sample_loop`` (the reference's imagen_pytorch3D.py:2116-2146) on the
one state.  Not a test module: the host and GPU tests of this path import it, with the derived bound; the known volume and the mask are
``volume_joint_inpaint_reference.inpaint_inputs()``.

Every step runs R passes, r = R - 1 .. 0.  A pass: ``q_sample(known, t)`` under the mask, the fused evaluation and the posterior step
``x = kx x + k0 x0 + kn n``, and -- unless r == 0 or the step ends at t = 0 -- the re-noise ``x = kr0 x + kr1 n``
(``q_sample_from_to(x, t_next, t)``).  After the chain: the final clamp and NO paste (the reference has none; ``paste_known`` adds it),
then fill and background as in every mode.

Draw numbering of the anchored field, ONE counter that advances as ``sample(noise=source, inpaint_images=...)`` calls its source per
window: draw 0 the initial image; per pass the q-noise, the step noise (counted also where kn == 0) and, where the pass re-noises, that
normal.

The host tables are ``Imagen._sampler_tables``' (fp32 as the device holds them, widened); tests/test_volume_joint_ddpm_inpaint_host.py
checks the chain they give against the oracle's transcription of the reference loop, which forms its coefficients on its own.

``chain_bound`` is a recursion over the passes for the largest error e of a covered state voxel, with u = 2^-24, eps_n the distance of
a device normal from its float64 value, M / X0 / K the largest |state|, |fused x0| and |known| met:
  * the initial image: e = eps_n;
  * a paste, at a masked voxel: e_m = sg eps_n + 2 u (al K + 6 sg) -- the rounded product al known, the fused sg n (|n| < 6) and the
    normal's own distance; it does not depend on the error before it, and an unmasked voxel keeps its own: e = max(e, e_m);
  * the evaluation with the elementwise stub (Lipschitz 1/2 in x, 1/8 in the self-conditioning): e_0 = 1/2 e + 1/8 e_sc + 8 u fmax +
    the blend's (n + 3) 2^-23 X0, fmax the largest |network output|; under dynamic thresholding every gain and local term doubles
    (s >= 1 divides, the clip is 1-Lipschitz, the quantile moves by at most the largest error) plus 4 u;
  * the step: e = |kx| e + |k0| e_0 + |kn| eps_n + 4 u (|kx| M + |k0| X0 + 6 |kn|) -- three products and two sums;
  * a re-noise: e = kr0 e + kr1 eps_n + 2 u (kr0 M + 6 kr1) -- the two-operand update again.
The final clamp is exact.
"""
import numpy as np

from tests import volume_blend_reference as R
from tests import volume_joint_heun_reference as HN
from tests import volume_joint_reference as J

SEED = J.SEED
STEPS = J.STEPS
EPS_N, U = HN.EPS_N, HN.U


def tables(scheduler, steps=STEPS, objective='x_start'):
    """The chain's host numbers as the device holds them (fp32, widened): coefs [T,3] = (kx, k0, kn) of the posterior, x0c [T,2],
    log_snr [T], renoise [T,2] = (kr0, kr1), qs [T,2] = (alpha, sigma)."""
    from diffusioniqt_amd.imagen_pytorch3D import Imagen
    coefs, conds, x0c, _, renoise, qs = Imagen._sampler_tables(scheduler, 1, 'ddpm', steps, None, 0.0, objective)
    wide = lambda t: t.numpy()[..., 0].astype(np.float64)
    return dict(coefs=wide(coefs), x0c=wide(x0c), log_snr=wide(conds), renoise=wide(renoise), qs=wide(qs))


def pass_plan(T, resample):
    """The passes of a chain in order, as (i, r, more, renoise): ``more`` -- another pass follows (this one's launch pastes for it);
    ``renoise`` -- the pass re-noises (r > 0 and the step does not end at t = 0)."""
    plan = [(i, r) for i in range(T) for r in reversed(range(resample))]
    return [(i, r, n + 1 < len(plan), r > 0 and i + 1 < T) for n, (i, r) in enumerate(plan)]


def draws_of(T, resample):
    return 1 + 2 * T * resample + (T - 1) * (resample - 1)


def joint_chain(vol, cfg, tabs, objective, clamp, blend, known, mask, resample=1, seed=SEED, sample=0, dyn=None, self_cond=False,
                dtype=np.float64, net=None):
    """One sample's joint inpainting chain, before the finish, in ``dtype``.  ``clamp`` = (lo, hi, mode) of the step (ignored under
    ``dyn`` = (q, floor)).  Returns the final state [D,H,W], the layout, the magnitudes ``chain_bound`` needs and the draws taken."""
    dt = np.dtype(dtype).type
    net = net or (J.self_cond_stub64 if self_cond else J.stub64)
    vol = np.asarray(vol, dtype=np.float32)
    L = J.layout(vol, cfg)
    P, stride, kept, slot = L['P'], L['stride'], L['kept'], L['slot']
    mean32, std32 = np.float32(cfg['Data']['mean']), np.float32(cfg['Data']['std'])
    low = ((vol - mean32) / std32).astype(dtype)                                         # fp32 normalisation, widened
    taps = R.taps_of(P, blend)
    coefs, x0c, log_snr, renoise, qs = (tabs[k] for k in ('coefs', 'x0c', 'log_snr', 'renoise', 'qs'))
    c = J.clamp_of(-np.inf, np.inf, 1) if dyn is not None else J.clamp_of(*clamp)
    cut = lambda a, o: a[o[0]:o[0] + P, o[1]:o[1] + P, o[2]:o[2] + P][None, None]
    rows = (lambda w: R.split_block(w, L['sub'])) if L['block'] else (lambda w: w)
    known = np.asarray(known, dtype=np.float32).astype(dtype)
    normal = lambda k: J.normals(vol.shape, seed, k, sample).astype(dtype)
    paste = lambda i, k, t: np.where(mask, dt(qs[i, 0]) * known + dt(qs[i, 1]) * normal(k), t)
    x = paste(0, 1, normal(0))
    draw = 2
    x0_vol, mags = None, dict(state=0.0, x0=0.0, net=0.0)
    y = np.empty((kept.shape[0], P, P, P), dtype=dtype)
    plan = pass_plan(coefs.shape[0], resample)
    for n, (i, r, more, ren) in enumerate(plan):
        for w, o in enumerate(kept):
            xw, lw = rows(cut(x, o)), rows(cut(low, o))
            sc = rows(cut(x0_vol, o)) if self_cond and x0_vol is not None else None
            pred = np.asarray(net(xw, lw, np.full(xw.shape[0], log_snr[i]), sc)).astype(dtype)
            mags['net'] = max(mags['net'], float(np.abs(pred).max()))
            if objective != 'x_start':
                pred = dt(x0c[i, 0]) * xw + dt(x0c[i, 1]) * pred
            if dyn is not None:
                pred = J.dynamic_threshold_rows(pred, *dyn).astype(dtype)
            y[w] = (R.merge_block(pred, P) if L['block'] else pred).reshape(P, P, P)
        x0, covered = HN.fuse(c(y), slot, taps, stride, vol.shape, dtype)
        kx, k0, kn = (dt(v) for v in coefs[i])
        mags['state'] = max(mags['state'], float(np.abs(x[covered]).max()))
        u = kx * x + k0 * x0
        if kn != 0:
            u = u + kn * normal(draw)
        draw += 1                                                                        # the step noise is drawn also where kn == 0
        if ren:
            u = dt(renoise[i, 0]) * u + dt(renoise[i, 1]) * normal(draw)
            draw += 1
        mags['state'] = max(mags['state'], float(np.abs(u[covered]).max()))
        if more:
            u = paste(plan[n + 1][0], draw, u)
            draw += 1
        x, x0_vol = np.where(covered, u, x), x0
        mags['x0'] = max(mags['x0'], float(np.abs(x0).max()))
    return x, L, mags, draw


def joint_reference(vol, cfg, tabs, objective, clamp, blend, known, mask, resample=1, seed=SEED, samples=1, dyn=None, self_cond=False,
                    dtype=np.float64, paste_known=False):
    """``VolumeInference(cfg, imagen.window_denoiser(sampler='ddpm', sample_steps=T, paste_known=paste_known), blend=blend,
    noise='anchored', joint=True, samples=samples, seed=seed, inpaint=(known, mask), inpaint_resample_times=resample)(vol, return_std=
    samples > 1)``.  ``clamp``: the static clamp of the data normalisation (the step's unless ``dyn``, the final one always).  A dict like
    ``volume_joint_reference.joint_reference``'s plus ``mask``, ``draws``, the magnitudes and ``bound``."""
    vol = np.asarray(vol, dtype=np.float32)
    known32 = np.asarray(known, dtype=np.float32)
    mean32, std32 = np.float32(cfg['Data']['mean']), np.float32(cfg['Data']['std'])
    fill, min_val = (np.float32(0.) - mean32) / std32, (vol.min() - mean32) / std32
    finals, mags = [], dict(state=0.0, x0=0.0, net=0.0)
    for s in range(samples):
        x, L, m, draws = joint_chain(vol, cfg, tabs, objective, clamp, blend, known32, mask, resample, seed, s, dyn, self_cond, dtype)
        f = J.clamp_of(*clamp)(x.astype(np.float64))
        finals.append(np.where(mask, known32.astype(np.float64), f) if paste_known else f)
        mags = {k: max(mags[k], m[k]) for k in mags}
    covered = R.blend_accumulate(np.zeros((1, L['kept'].shape[0], L['P'], L['P'], L['P'])), L['slot'], np.ones(L['P']), L['stride'],
                                 vol.shape)[2]
    background = ((vol - mean32) / std32) == np.float32(min_val)
    r = np.stack([np.where(background, np.float64(min_val), np.where(covered, f, np.float64(fill))) for f in finals])
    std = r.std(axis=0, ddof=1) if samples > 1 else np.zeros(vol.shape)
    return dict(mean=r.mean(axis=0), std=std, covered=covered, background=background, fill=fill, min_val=min_val, mask=np.asarray(mask),
                windows_per_voxel=L['windows_per_voxel'], kept=L['kept'].shape[0], candidates=L['slot'].size, draws=draws, **mags,
                bound=chain_bound(tabs, L['windows_per_voxel'], mags, float(np.abs(known32).max()), resample, objective, dyn is not None,
                                  self_cond))


def chain_bound(tabs, windows_per_voxel, mags, known_max, resample=1, objective='x_start', dynamic=False, self_cond=False):
    """The recursion of the module docstring; ``mags`` = the largest |state|, |fused x0| and |network output| of the float64 chain."""
    assert objective == 'x_start', "the bound is derived for the x_start objective (no x0 conversion between the network and the clamp)"
    M, X0, fmax = mags['state'], mags['x0'], mags['net']
    coefs, renoise, qs = np.abs(tabs['coefs']), np.abs(tabs['renoise']), np.abs(tabs['qs'])
    k = 2.0 if dynamic else 1.0
    two_operand = lambda a, amag, b: b * EPS_N + 2 * U * (a * amag + 6 * b)               # a v + b n with |v| <= amag, |n| < 6
    plan = pass_plan(coefs.shape[0], resample)
    e = max(EPS_N, two_operand(qs[0, 0], known_max, qs[0, 1]))
    e_sc = 0.0
    for n, (i, r, more, ren) in enumerate(plan):
        kx, k0, kn = coefs[i]
        e_0 = k * (0.5 * e + (0.125 * e_sc if self_cond else 0.0) + (9 if self_cond else 8) * U * fmax) + (4 * U if dynamic else 0.0) \
            + R.tolerance(windows_per_voxel, X0)
        e = kx * e + k0 * e_0 + kn * EPS_N + 4 * U * (kx * M + k0 * X0 + 6 * kn)
        if ren:
            e = renoise[i, 0] * e + two_operand(renoise[i, 0], M, renoise[i, 1])
        if more:
            j = plan[n + 1][0]
            e = max(e, two_operand(qs[j, 0], known_max, qs[j, 1]))
        e_sc = e_0
    return e
