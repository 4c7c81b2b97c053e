"""Whole-volume inference — the sliding-window loop of the reference's test scripts (test_all.py:182-300, test.py) with its
dataset (`supervisedIQT_INF`, data.py:138-202), kept on the device: the raw low-res volume stays resident in HBM, patches are
gathered / normalised / rejected by one kernel, sampled in batches, stitched by a scatter kernel that applies the script's
overlap-crop rules, and the background is reset in place.  One job per volume; several volumes or patch ranges shard over
GPUs with no collective.

The script semantics (the defaults; every mode below keeps the first four lines):
* candidate origins: ``range(0, N - P + 1, overlap)`` per axis, i outermost (data.py:157-160; ``Eval.overlap`` is the STRIDE);
* a candidate is dropped when fewer than 5 % of its RAW voxels are non-zero (data.py:187-191);
* patches are z-scored with ``Data.mean/std`` (data.py:165-169); the output volume starts at ``(0 - mean) / std``;
* voxels whose normalised low-res value equals the volume minimum are reset to it (test_all.py:300);
* ``Train.batch_sample``: the window is ``patch_size_sub * batch_sample_factor`` (96), each block is split into 27 sub-volumes
  for the sampler and merged back (utils_mine.py:25-67); blocks overlap, and each writes its interior ``[op : P - op]``
  (``op = overlap // 2``) except on faces that touch the volume boundary (test_all.py:267-296);
* without ``batch_sample`` and with ``overlap >= patch`` patches are placed whole (test_all.py:262-263).  The script's
  overlap < patch branch of that mode raises on its first interior patch (a 3-element tensor in a boolean ``or``,
  test_all.py:241) — here it applies the same per-face crop rule as the block mode instead;
* ``evaluate_volume`` scores the stitched volume as the script's ``eval`` does (test_all.py:47-62): centre crop, PSNR, MS-SSIM of
  the min-max normalised pair — without LPIPS (no VGG weights here).

Blend (``blend='gaussian'`` / ``'constant'``) replaces crop-and-overwrite by weighted overlap blending: whole windows contribute (no
crop margins), each voxel is the weighted mean of the windows that cover it, with the separable weight ``taps[i] taps[j] taps[k]``
(``blend_taps``: a Gaussian importance map of sigma ``sigma_scale * P`` with maximum 1, or all ones = the plain mean).  Every kept
window's prediction stays in HBM and ONE gather-side launch (``ops.volume_blend``) reduces them per output voxel in candidate order —
no atomics, bit-reproducible, independent of ``Eval.batch_size``; the background reset is fused into it.  A voxel that no kept window
covers keeps the fill value ``(0 - mean) / std``.

Samples (``samples=S``, with a blend mode) draws every batch S times (sample 0 of a batch, then sample 1, ...); the result is the
per-voxel mean of the S blended volumes and, with ``return_std=True``, their unbiased standard deviation — the uncertainty map of a
stochastic sampler.

Anchored noise (``noise='anchored'``) hands the sampler a noise source tied to the VOLUME instead of letting every batch draw its own:
the value at global voxel (z, y, x) of draw k and sample s is a pure function of (seed, z, y, x, k, s) (``AnchoredNoise``, one
Philox4x32-10 call per voxel in ``ops.anchored_noise``), so all windows that cover a voxel start from — and, in a stochastic sampler,
are pushed by — the same numbers, whatever ``Eval.batch_size`` is, whichever windows the non-zero filter kept and in whatever order
or on whichever rank they run.  What is left of the disagreement between overlapping windows is what the network does differently
with different context; the ``samples = S`` fields are independent of each other and coherent across windows.  Any sampler that
takes ``noise=source`` works, in every mode: ``sampler='dpmpp2m'`` (DPM-Solver++ 2M, the second-order multistep solver;
``Imagen.p_sample_loop``) is only passed on to ``sample``, and ``ElucidatedImagen.sample(noise=source)`` accepts the source when
exactly one U-Net is sampled: draw 0 is the low-res augmentation noise, draw 1 the initial image, draw 2 + i the eps of Heun step i.

Joint (``joint=True``, with a blend mode and ``noise='anchored'``) removes that remainder at its source: instead of running every
window's reverse chain alone and blending finished patches, ONE noisy state of the whole volume is kept and the windows' x0
predictions are fused at EVERY step (MultiDiffusion, Bar-Tal et al. 2023).  The second constructor argument is then a window
denoiser (``Imagen.window_denoiser`` / ``ImagenTrainer.window_denoiser``: scalar step coefficients, the clamp, ``x0`` and ``finish``; the
whole protocol is in the docstring of ``VolumeInference``).  Per sample a chain runs on whole volumes: every evaluation gathers the kept
windows of the state, runs the U-Net on them in ``Eval.batch_size`` batches, and ONE fused launch blends the predictions per voxel with
the blend weights and advances the state in place; ``ops.volume_joint_finish`` applies the fill / background rules and the statistics
over the samples.  The draw numbering is ``AnchoredNoise.source``'s, so with stride = patch (no overlap) every joint chain IS the
independent one, bit for bit.  The four chains:
* first order (``window_denoiser(sampler='ddim', sample_steps=K)`` or the ancestral default): the state starts as draw 0 of the
  anchored field and ``ops.volume_joint_step`` takes the sampler step with draw ``i + 1`` — N windows x T steps evaluations, as many
  as the independent windows cost;
* multistep (``window_denoiser(sampler='dpmpp2m', sample_steps=K)``, ``den.multistep``): keeps the fused x0 volume of the previous step
  and takes ``ops.volume_joint_multistep``, x_next = kx x + k0 x0 + kp x0_prev, per step.  It is deterministic after draw 0;
* Heun (the EDM family, ``ElucidatedImagen.window_denoiser()``, ``den.heun``): the stochastic Heun sampler on three volumes --
  images_hat, images_next and the fused prediction -- fusing the windows after BOTH U-Net evaluations of a step:
  ``ops.volume_joint_heun_init`` (initial image + first churn), then per step the windows of images_hat evaluated at sigma_hat and
  ``ops.volume_joint_heun`` phase 1 (predictor), the windows of images_next evaluated at sigma_next and phase 2 (corrector + the next
  step's churn) -- 2 T - 1 fused launches for T steps, twice the U-Net evaluations of a first-order chain.  The low-res noise of a
  batch is draw 0 of the field at its windows, recomputed per evaluation; at stride = patch the chain is ``sample(noise=source)`` per
  window;
* sigma-space multistep (``ElucidatedImagen.window_denoiser(sampler='dpmpp2m', sample_steps=K, eta=...)``, ``den.multistep`` with a
  ``den.sigma0``): DPM-Solver++ 2M for the EDM family, ODE (``eta = 0``) or midpoint SDE -- the state starts as ``sigma0 n`` and
  ``ops.volume_joint_multistep_sde`` takes x_next = kx x + k0 x0 + kp x0_prev + kn n per step: T evaluations per window and T + 1
  fused launches where the Heun chain costs 2 T - 1 of each.

Inpainting (``inpaint=(known, mask)``, ``inpaint_resample_times=R``) keeps the voxels of ``known`` under ``mask`` fixed while the rest of
the volume is generated (RePaint, Lugmayr et al. 2022; the loop of the reference's ``ElucidatedImagen.one_unet_sample``).  In the crop
and blend modes every sampler call gets its windows of the two volumes and inpaints on its own -- each window resamples its own border of a
known region that crosses it.  With ``joint=True`` and the Heun denoiser the loop runs on the one state: R passes per step, the pass
boundary (re-noise, paste, churn) riding in the corrector launch (``ops.volume_joint_heun_inpaint``), 2 R T - 1 fused launches after the
initial state for T steps, and one paste per sample before ``ops.volume_joint_finish``.  With ``joint=True`` and the ancestral denoiser
of the DDPM family (``Imagen.window_denoiser(sampler='ddpm')``; the loop of the reference's ``Imagen.p_sample_loop``) it runs on the one
state too: the initial image under the first paste, then R passes per step, each one evaluation and ONE ``ops.volume_joint_step_inpaint``
launch that carries the step, the re-noise and the paste of the next pass -- 1 + R T fused launches.  That family's loop does not paste
the known values after the chain, so a known voxel comes back denoised, not exactly, unless the denoiser was made with
``paste_known=True``.

Consistency (``consistency=(measurement, cell)``, ``consistency_weight=w``) ties the generated volume to an acquisition whose
degradation is a block average -- thick slices: ``measurement`` [D/fz, H/fy, W/fx] holds the mean of every cell of ``cell`` = (fz, fy, fx)
high-res voxels, n = fz fy fx in 2 .. 64.  After every U-Net evaluation the x0 prediction is replaced by x0 + w A+(y - A x0) (DDNM, Wang,
Yu, Zhang 2023; A the cell mean, A+ replication): the cell means move onto the measurement, the detail inside a cell -- the null space
of A, what the network is for -- stays.  ``w = 1`` is DDNM, ``w < 1`` its relaxation for a noisy measurement.  The measurement is
replicated onto the high-res grid once (``ops.cell_replicate``) and z-scored like the low-res volume.  In the crop and blend modes every
sampler call gets its windows of that volume as ``consistency=(windows, cell)`` and projects on its own (``ops.cell_project``), so the
stride and the window must be multiples of the cell: no cell may straddle a window.  With ``joint=True`` the projection is part of the
fused launch (the consistent step of ``ops`` that ``consistency.Chain.joint_step`` picks, in place of the three linear steps, as many
launches as before), on the fused x0 of
the one state: it is defined for every cell of the volume whose voxels are all covered, windows that share a cell are corrected by the
same amount, and only the volume has to be a multiple of the cell.  What is exactly consistent (w = 1, to fp32 rounding) is the last
corrected prediction.  The sigma-space chain ends at sigma = 0 with (kx, k0) = (0, 1): the state it ends in IS that prediction.  The
schedules of the DDPM family end at a finite log-SNR, so their last step keeps a little of the state (4 ddim steps of the cosine
schedule end on kx = 0.032, k0 = 0.971) and the final cell means are kx A x_t + k0 y.  What comes after the chain -- the denoiser's
final clamp, and in ``ops.volume_joint_finish`` the fill of uncovered voxels and the background reset -- is not projected again, and
cells they touch are no longer exactly consistent.  Not offered: the EDM Heun sampler without ``consistency_heun`` (below), and
consistency together with inpainting.

The Heun sampler of the EDM family (``consistency_heun='both'`` or ``'predictor'``, with ``consistency``) has two predictions per
step: ``'both'`` projects the fused prediction of either evaluation, ``'predictor'`` the first alone (one launch fewer per step for a
per-window call; the corrector's prediction stays the network's).  The step that ends at sigma = 0 has no corrector and its predictor
row is (0, 1), so under either value the chain ends in its last projected prediction, as the sigma-space chain does.  The crop and
blend modes hand ``consistency_heun=`` on to the sampler call (``ElucidatedImagen.sample(sampler='heun', ...)``: one projection launch
of the mode after each projected evaluation, any of the five modes); with ``joint=True`` and ``ElucidatedImagen.window_denoiser()``
the projection rides in ``ops.volume_joint_consistent_heun``, which ``consistency.Chain.joint_heun`` puts in the place of
``ops.volume_joint_heun`` in phase 1 and, under ``'both'``, in phase 2 -- 2 T - 1 fused launches as before -- for the cell mean, a
profile or an operator; self-conditioning gathers the projected volume.  Not offered: joint Heun with the slab or the band (their
joint step launches carry the three linear update forms only), DDNM+ weights (``consistency_noise`` / ``consistency_row_noise``:
Heun's noise is the churn before the evaluation), and any sampler but Heun with the keyword.

A slice profile (``consistency_profile=(pz, py, px)``, with ``consistency``) replaces the plain mean: the measurement of a cell is
u . x, u_q = pz_i py_j px_k / (sum pz sum py sum px) -- the weights of the voxels under a slice, roughly Gaussian or trapezoidal for a
2-D multi-slice scan, with zeros where a gap between slices leaves voxels unmeasured.  ``ops.cell_profile`` validates it and makes the
host table (u, and the gains g = u / sum u^2); ``ops.cell_measure(vol, cell, table)`` is that operator and simulates the acquisition.
The cells stay disjoint, so A+ = A^T / |u|^2 and the projection is x0' = x0 + w g (y - u . x0) per voxel: a gap voxel (u = 0) is never
moved, and exact consistency at w = 1 means u . x0' = y (to fp32 rounding).  Since sum u = 1, A commutes with the z-score and
``state_space``, so the replicated measurement, its window gathers, the covered-cell rule (ALL n voxels, whatever their weights) and
the divisibility rules are those above.  The crop and blend modes hand ``consistency_profile=`` on to the sampler
(``ops.cell_project_profile`` per step); ``joint=True`` launches the profile's consistent step in the place of the plain
mean's, as many launches as before.  A uniform profile given explicitly takes this path too.  Profiles
that overlap between neighbouring cells (slice cross-talk) are ``consistency_slab``, below.

A noisy measurement (``consistency_noise=sigma``, with ``consistency``; DDNM+, Wang et al. 2023, 3.3): sigma is the standard deviation
of the measurement's noise in the raw units of the measurement.  A constant weight pastes that noise into every prediction and the
stochastic samplers add their full fresh noise on top of it.  With sigma known, ``ops.consistency_noise_schedule`` gives every step of
a chain x_next = kx x + k0 x0' + kp x0'_prev + kn eps its own weight w_i <= ``consistency_weight`` (now a cap) and a reduction of the
fresh normals in the range of A, eps' = eps - shrink_i g (u . eps) per cell, so that there the measurement noise the step carries plus
the fresh noise left is kn^2, what the sampler intends; the null space of A keeps its normals.  The budget is per step: noise already
inside the state is not tracked.  A step with kn = 0 -- the last of every chain -- gets weight 0 and runs unprojected, so the final
volume is no longer exactly consistent with the (noisy) measurement, by design.  Units: sigma / std is the z-scored value the crop and
blend modes hand on as ``consistency_noise=``; ``joint=True`` multiplies it by the slope of the denoiser's affine ``state_space`` map,
state_space(1) - state_space(0), and dispatches per step: weight 0 the family's plain launch, shrink 0 the consistent launch,
otherwise the consistent step that also shapes the normals -- one launch per step as before, the same draws.  Deterministic chains (ddim with
eta = 0, dpmpp2m without eta) and the Heun sampler are refused; sigma is given, not estimated.

A tile-local linear operator (``consistency_operator=A``, with ``consistency``) is the general case: the volume splits into disjoint
tiles of ``cell`` voxels and every tile is measured by the same m x n matrix A, any number of rows, any rank -- two or three
orthogonal thick-slice stacks of one anatomy (``ops.stack_operator``; ``ops.stack_rows`` lays the stack volumes out as the
[m, D/fz, H/fy, W/fx] measurement), a block-DCT low-pass, a partial-volume model.  ``ops.tile_operator`` validates A and makes, in
float64, A+ and the n x n orthogonal projector P = A+ A (fp32 table, symmetric to the bit); ``ops.tile_measure`` is A and simulates the
acquisition.  The projection is x0' = x0 + w (t - P x0) with t = A+ y (``ops.tile_backproject``, once per volume), a volume on the
high-res grid where the replicated measurement stood: the constant must lie in the row space of A (P 1 = 1, checked), so t passes
through the z-score and ``state_space`` as a plain volume, and the window gathers, the covered rule (ALL n voxels of a tile) and the
divisibility rules are those above.  The crop and blend modes hand windows of t and ``consistency_operator=`` on to the sampler
(``ops.tile_project`` per step); ``joint=True`` launches the tile operator's consistent step, as many launches as before.  At
w = 1 the corrected prediction satisfies P x0' = t (to fp32 rounding), which is A x0' = y when y lies in the range of A; stacks that
contradict each other are fitted in the least-squares sense.  An operator that crosses tile borders is not a tile operator: true
k-space truncation is ``consistency_band``, overlapping slice profiles are ``consistency_slab``, both below.  Not offered:
``consistency_profile`` or ``consistency_noise`` with an operator, Heun without ``consistency_heun``,
consistency together with inpainting; the stacks are taken as registered to each other and A as known.

Noisy rows (``consistency_row_noise=sigma``, with ``consistency`` and ``consistency_operator``; DDNM+ per singular direction): sigma
is the standard deviation of the noise of each row of A in raw units, one number or m of them -- for stacks one value per stack,
repeated over that stack's rows; stacks of one subject usually differ in slice thickness and with it in noise.  Whitening is
unit-free: omega_r = sigma_min / sigma_r, A_w = diag(omega) A = U S V^T (``ops.tile_noise_operator``, float64), and
t = (A_w+ diag omega) y comes from ``ops.tile_backproject`` as before.  Along v_j the noise of t has the deviation sigma_min / s_j,
so direction j takes ``ops.consistency_noise_schedule`` with s_j as it is (``ops.tile_noise_schedule``), and a step applies
x0' = x0 + M_i (t - x0), eps' = eps - G_i eps with M_i = V diag(lambda_i) V^T and G_i = V diag(shrink_i) V^T
(``ops.tile_noise_tables``: fp32, symmetric to the bit, made once per chain and uploaded as one [T, 2, n, n] tensor).  Units are
those of ``consistency_noise``: sigma / std goes to the sampler calls of the crop and blend modes, ``joint=True`` multiplies by the
|slope| of ``state_space``.  Per step, on the fp32 values: every lambda 0 is the family's plain launch (the last step: unprojected),
every shrink 0 with one common lambda the constant-weight tile launch, otherwise ``ops.tile_project_noise`` /
the fused joint step that reads the same tables -- as many launches and the same draws as before.  Not offered: correlated row
noise, sigma estimated from the data, measurement noise tracked across steps, a cell whose launch plans more than 64 KiB of LDS.

Overlapping slice profiles (``consistency_slab=(pz, py, px)``, with ``consistency``): a real slice profile is wider than the slice
spacing, so neighbouring thick slices share voxels.  ``pz`` has L = fz + 2r entries, reach r >= 1 and 2r <= fz (a slice overlaps its
two neighbours only); ``py`` / ``px`` are the in-plane profile inside the cell.  With u_z = pz / sum pz and u_yx the normalised outer
product, slice s of the in-plane cell (cy, cx) measures y_s = sum_i u_z[i] (u_yx . x[s fz - r + i, cell]); every row sums to 1, so the
z-score, ``state_space``, the replicated measurement and its window gathers are those above.  ``ops.slab_profile`` validates the
profile and makes the host table, ``ops.slab_measure`` is the operator.  Along z, A A^T = q G with G Toeplitz tridiagonal (d = sum
u_z^2, e the overlap product): the first operator here whose pseudo-inverse is not local.  A row is active when its whole support
lies inside the domain -- the window of a sampler call, the volume with ``joint=True`` -- and is covered; the first and the last
slice of a domain never are.  The projection is DDNM on the active rows, one tridiagonal solve (pivots tabulated on the host) per
maximal run of active rows of a column; a voxel under no active row keeps its bits.  A profile with d - 2e < d / 64 is refused, which
bounds the condition number of any run by 128.  The crop and blend modes hand ``consistency_slab=`` on to the sampler
(``ops.slab_project`` per step: windows enforce only their inner slices).  ``joint=True`` needs a solve along the whole depth of the
volume, which does not fit a box-of-cells block: a step is THREE launches where the tile-local operators take one --
``ops.volume_joint_slab_coeffs`` (the fused plane values, then the solve per column) and
the slab's consistent step -- and the windows are walked twice; the workspace and the coefficient volume are
allocated once per volume.  Not offered: a reach beyond half a cell, slabs along other axes (permute the volume instead),
noise-aware weights (``consistency_noise`` / ``consistency_row_noise``), rows that leave the volume, and any of the other
consistency keywords together with it.

A k-space band limit (``consistency_band=(hz, hy, hx)`` or ``(hz, hy, hx, offset)``, with ``consistency``): what a 3-D encoded
low-resolution scan is -- the central, box-shaped part of k-space, taken on the periodic field of view and sampled on the low-res
grid.  Per axis (N voxels, factor f, n = N / f) ``h`` is None, the full band |k| <= kappa = (n - 1) // 2 of the low-res grid (on an
even n the unpaired Nyquist bin is NOT part of the band), or the weights of the frequencies k = 0 .. len - 1, symmetric in +-k: finite
and >= 0, h[0] > 0 (they are divided by it), a zero drops its frequency, and a positive weight below max(h) / 64 is refused (the
back-projection would amplify by more than 64).  ``offset``: where in its cell a low-res sample sits, three numbers in high-res
voxels or 'centre' = (f - 1) / 2; default 0.  An axis with f = 1 and ``h`` None is the identity and has no pass.  The box is
separable, so A, A+ and the projector P = A+ A are Kronecker products of real circulants with Dirichlet kernels
(``ops.band_table``: N floats per table and axis, no FFT, no power-of-two shape; ``ops.band_measure`` is A and simulates the
acquisition).  Rows of A sum to 1, so t = A+ y (``ops.band_backproject``, once per volume) passes through the z-score and
``state_space`` as the tile operator's t does, and the projection is the tile operator's, x0' = a + w P (t - a) with a the clamped
prediction: at w = 1, P x0' = t.  The periodic wrap is part of the model, as it is in the scanner.  The operator is global -- every
voxel of a line feeds every output of that line -- and a window of t is not the t of a window: a one-call sampler projects on its cube
(``ops.band_project``: one launch per active axis) with ``consistency=(t, cell)``, and ``VolumeInference`` takes the keyword with
``joint=True`` only (the crop and blend modes refuse).  A joint step is three calls and up to five launches, without atomics or waits
across workgroups: ``ops.volume_joint_band_residual`` (the fuse; a = the fused clamped prediction, the covered flags, r = t - a, or 0
where nothing covers), ``ops.band_apply`` (c = P r, three dense passes along the axes) and
``ops.volume_joint_consistent_band_step`` (the three update forms on x0' = a + w c; the windows are not walked again).  A residual of
0 means the measurement is believed where nothing was generated, so exact consistency holds only on a fully covered volume.  The table
and the five-volume workspace are made once per volume; an axis is capped at 512 voxels (``ops.band_plan``).  Not offered: a
non-separable band (an ellipsoid, partial Fourier), phase or coil models, noise-aware weights, the crop and blend modes, and any of the
other consistency keywords together with it; joint Heun; Heun per window without ``consistency_heun``, inpainting, ``init_images`` and
``skip_steps`` as for ``consistency``.
"""
from types import SimpleNamespace

import numpy as np
import torch

from . import ops
from .consistency import plan as consistency_plan
from .metrics import MSSIM, PSNR
from .utils_mine import convertVolume2subVolume, merge_sub_volumes


def sliding_window_origins(shape, patch, stride):
    """data.py:157-160 -> int32 [n, 3]"""
    rng = [range(0, s - patch + 1, stride) for s in shape]
    return np.array([[i, j, k] for i in rng[0] for j in rng[1] for k in rng[2]], dtype=np.int32).reshape(-1, 3)


def crop_margins(origins, n, patch, overlap):
    """Per-patch {lo, hi} crop per axis (test_all.py:267-296): overlap//2 inside, 0 on faces at the volume boundary."""
    op = overlap // 2
    m = np.zeros((origins.shape[0], 6), dtype=np.int32)
    if overlap >= patch:
        return m
    for a in range(3):
        o = origins[:, a]
        m[:, 2 * a] = np.where(o == 0, 0, op)
        m[:, 2 * a + 1] = np.where((o + patch == n[a]) | (n[a] - patch <= o), 0, op)
    return m


BLEND_MODES = (None, 'gaussian', 'constant')


def blend_taps(P, kind='gaussian', sigma_scale=0.125):
    """The 1-D window of a blend mode, fp32 [P]: ``'gaussian'`` = exp(-(i - (P-1)/2)^2 / (2 (sigma_scale P)^2)) evaluated in float64
    and divided by its maximum; ``'constant'`` = ones.  The 3-D weight of a window voxel is the product of its three taps."""
    if kind == 'constant':
        return np.ones(int(P), dtype=np.float32)
    if kind != 'gaussian':
        raise ValueError(f"blend_taps: kind must be 'gaussian' or 'constant', got {kind!r}")
    i = np.arange(int(P), dtype=np.float64)
    t = np.exp(-(i - (P - 1) / 2.0) ** 2 / (2.0 * (float(sigma_scale) * P) ** 2))
    return (t / t.max()).astype(np.float32)


NOISE_MODES = (None, 'anchored')


class AnchoredNoise:
    """Noise anchored to a [D,H,W] volume.  ``source(origins, P, sample)`` is what a sampler takes as ``noise=``: a callable whose
    call number k (0 = the initial image, then one per stochastic step) returns draw k of the field, cut out at the windows
    ``origins`` [B,3] of edge P -- ``ops.anchored_noise(origins, C, P, D, H, W, seed, draw=k, sample=sample)``."""

    def __init__(self, volume_shape, seed=0):
        self.shape = tuple(int(s) for s in volume_shape)
        if len(self.shape) != 3:
            raise ValueError(f"AnchoredNoise: volume_shape must be (D, H, W), got {volume_shape!r}")
        self.seed = int(seed)

    def source(self, origins, P, sample=0, device=None):
        origins = np.ascontiguousarray(np.asarray(origins).reshape(-1, 3))
        state = {'draw': 0}

        def noise(shape):
            shape = tuple(shape)
            assert len(shape) == 5 and shape[0] == origins.shape[0] and shape[2:] == (P, P, P), \
                f"AnchoredNoise: the sampler asked for {shape}, the source was made for {origins.shape[0]} windows of edge {P}"
            out = ops.anchored_noise(origins, shape[1], P, *self.shape, self.seed, draw=state['draw'], sample=sample, device=device)
            state['draw'] += 1
            return out
        return noise


def sub_volume_origins(origin, factor, sub):
    """Origins of the ``factor^3`` sub-volumes of the block at ``origin`` in the order of ``convertVolume2subVolume``
    (utils_mine.py:25-42): sub-volume n = b2 + f b3 + f^2 b4 starts at origin + sub (b2, b3, b4)."""
    n = np.arange(factor ** 3)
    off = np.stack((n % factor, (n // factor) % factor, n // (factor * factor)), axis=1) * sub
    return (np.asarray(origin).reshape(1, 3) + off).astype(np.int32)


class _Windows:
    """The window plan of one ``VolumeInference`` call: the volume ``shape`` / ``device``; the candidate ``origins`` on their ``lattice``
    (candidate order = lattice order); ``keep``, the 5 % filter's verdict from ONE ``ops.patch_gather`` over all candidates; ``kept``
    [N,3] (after ``patch_slice``); ``fill`` / ``min_val``, the normalised empty voxel and volume minimum in fp32 arithmetic, as Python
    floats; under a blend mode the device ``slot`` table (a kept window's row, -1: dropped) and ``taps``; ``batches``, the ``(lo, host
    origins, device origins)`` of every sampler call -- ``Eval.batch_size`` windows, or ONE block in block mode (overlapping blocks are
    written one launch at a time in candidate order: later blocks overwrite, as in the script).  ``_joint`` adds ``x0_vol``
    and ``consistency``, the ``consistency.Chain`` of this volume (or None)."""

    def __init__(self, inf, vol, patch_slice=None):
        dev, P = vol.device, inf.patch
        self.shape, self.device = tuple(vol.shape), dev
        self.origins = sliding_window_origins(self.shape, P, inf.overlap)
        self.lattice = tuple(len(range(0, s - P + 1, inf.overlap)) for s in self.shape)
        _, nz = ops.patch_gather(vol, torch.from_numpy(self.origins).to(dev), P, inf.mean, inf.std, want_patches=False, want_nonzero=True)
        self.keep = (nz.cpu().numpy().astype(np.float64) / float(P ** 3)) >= inf.ratio      # data.py:187-191
        self.kept = self.origins[self.keep]
        if patch_slice is not None:
            rank, world = patch_slice
            self.kept = self.kept[rank::world]
        self.N = self.kept.shape[0]
        mean32, std32 = np.float32(inf.mean), np.float32(inf.std)
        self.fill = float((np.float32(0.) - mean32) / std32)
        self.min_val = float((np.float32(float(ops.min_value(vol).item())) - mean32) / std32)   # monotone map: min of the normalised volume
        self.slot = self.taps = None
        if inf.blend is not None:
            slot = np.full(self.origins.shape[0], -1, dtype=np.int32)
            slot[self.keep] = np.arange(self.N, dtype=np.int32)
            self.slot = torch.from_numpy(slot.reshape(self.lattice)).to(dev)
            self.taps = torch.from_numpy(blend_taps(P, inf.blend, inf.sigma_scale)).to(dev)
        per_call = 1 if inf.block_mode else inf.batch
        hosts = [(lo, np.ascontiguousarray(self.kept[lo:lo + per_call])) for lo in range(0, self.N, per_call)]
        self.batches = [(lo, o, torch.from_numpy(o).to(dev)) for lo, o in hosts]
        self._block = (inf.factor, inf.sub) if inf.block_mode else None

    def noise_origins(self, origins):
        """Where the noise of the batch at ``origins`` belongs: block mode (ONE block, sampled split) -> its sub-volumes' origins."""
        return sub_volume_origins(origins[0], *self._block) if self._block else origins


class VolumeInference:
    """The stitched, z-scored prediction of one raw volume; the modes are in the module docstring.  What ``joint=True`` reads of its
    window denoiser ``den``:
    * required (the constructor checks them): ``num_steps``; ``coefs``, a host tensor with one row (kx, k0, kn) per step; ``clamp = (lo,
      hi, mode)``, passed to the fused launch; ``x0(img, lowres, i, self_cond=None)``, the x0 prediction of a batch of windows at step i;
      ``finish(x)``, applied to the volume a chain ends in;
    * optional, False when absent: ``self_cond`` (the windows of the last fused x0 volume are passed as ``self_cond=``), ``multistep``
      (``coefs`` rows are (kx, k0, kp)) and ``heun``;
    * first order with ``inpaint=``: host tables ``qs`` [T,2] (alpha, sigma) and ``renoise`` [T,2], ``normalize(x)`` (a known volume
      into state space) and ``finish(x, known, mask)`` (``known`` in state space, ``mask`` 0/1; whether it pastes is the denoiser's);
    * with ``heun``: ``coefs`` rows (kc, a1, b1, a2, b2, c2, d2); ``sigma0``; ``sched`` rows (sigma, sigma_next, gamma), sigma_next == 0
      meaning no corrector; ``draw_base`` (1 when draw 0 is the low-res augmentation noise: the initial image is draw ``draw_base``, the
      eps of step i draw ``draw_base + 1 + i``); ``x0`` also takes ``stage=`` (0: at sigma_hat, 1: at sigma_next) and ``lowres_noise=``;
      with ``inpaint=`` also ``normalize(x)`` (a known volume into state space) and ``finish(x, known, mask)`` (the paste of the known
      values, state space, under the 0/1 mask between the clamp and the un-normalisation);
    * with ``multistep`` and a ``sigma0`` (the EDM family's ``sampler='dpmpp2m'``): ``coefs`` rows (kx, k0, kp, kn); the state starts as
      ``sigma0`` times draw ``draw_base`` and step i adds kn times draw ``draw_base + 1 + i`` (no Philox call where kn == 0); ``x0`` also
      takes ``lowres_noise=``.  A multistep denoiser without ``sigma0`` (``Imagen``'s) runs the chain above, unchanged."""
    _DENOISER = ('num_steps', 'coefs', 'clamp', 'x0', 'finish')

    @staticmethod
    def _protocol(den):
        """``den`` as the chains use it: the host tables as Python numbers, the optional attributes defaulted."""
        p = SimpleNamespace(num_steps=den.num_steps, coefs=den.coefs.tolist(), clamp=tuple(den.clamp), x0=den.x0, finish=den.finish,
                            **{a: bool(getattr(den, a, False)) for a in ('self_cond', 'multistep', 'heun')})
        if p.heun:
            p.draw_base, p.sigma0, p.sched = int(den.draw_base), den.sigma0, den.sched
        p.sigma_space = p.multistep and not p.heun and hasattr(den, 'sigma0')
        if p.sigma_space:
            p.draw_base, p.sigma0 = int(den.draw_base), float(den.sigma0)
        if hasattr(den, 'qs') and hasattr(den, 'renoise'):   # the ancestral sampler's inpainting tables
            p.qs, p.renoise = den.qs.tolist(), den.renoise.tolist()
        return p

    @staticmethod
    def _check_inpaint(inpaint, resample_times, joint, sample_fn):
        """The argument rules of ``inpaint`` (``ValueError``; nothing touches the device).  Returns None or (known fp32, mask bool), host
        or device tensors as they were given."""
        if inpaint is None:
            return None
        if not isinstance(inpaint, (tuple, list)) or len(inpaint) != 2:
            raise ValueError(f"VolumeInference: inpaint must be (known, mask), got {type(inpaint).__name__}")
        known, mask = (torch.as_tensor(t) for t in inpaint)
        if known.ndim != 3 or not known.is_floating_point() or mask.dtype != torch.bool or mask.shape != known.shape:
            raise ValueError(f"VolumeInference: inpaint must be (known float [D,H,W], mask bool [D,H,W]) of one shape, got {known.dtype} "
                             f"{tuple(known.shape)} and {mask.dtype} {tuple(mask.shape)}")
        if isinstance(resample_times, bool) or not isinstance(resample_times, int) or resample_times < 1:
            raise ValueError(f"VolumeInference: inpaint_resample_times must be a positive integer, got {resample_times!r}")
        heun = getattr(sample_fn, 'heun', False)
        ancestral = not heun and not getattr(sample_fn, 'multistep', False) and hasattr(sample_fn, 'qs') and hasattr(sample_fn, 'renoise')
        if joint and not ((heun or ancestral) and hasattr(sample_fn, 'normalize')):
            raise ValueError("VolumeInference: joint=True inpaints with an EDM Heun denoiser (ElucidatedImagen.window_denoiser()) or the "
                             "ancestral one of the DDPM family (Imagen.window_denoiser(sampler='ddpm')) only: the other first-order "
                             "chains and the multistep chains have no re-noising loop")
        return known.float(), mask

    @property
    def consistency(self):
        """None, or the checked ``(measurement fp32, cell, weight)`` of the plan."""
        return None if self.plan is None else (self.plan.measurement, self.plan.cell, self.plan.weight)

    # the other consistency keywords as the plan holds them: the operator (whitened under ``consistency_row_noise``), the profile's
    # host table, and the checked or as-given values
    consistency_op = property(lambda self: getattr(self.plan, 'op', None))
    consistency_table = property(lambda self: getattr(self.plan, 'profile_table', None))
    consistency_noise = property(lambda self: getattr(self.plan, 'noise', None))
    consistency_row_noise = property(lambda self: getattr(self.plan, 'row_noise', None))
    consistency_slab = property(lambda self: getattr(self.plan, 'slab', None))
    consistency_band = property(lambda self: getattr(self.plan, 'band', None))
    consistency_heun = property(lambda self: getattr(self.plan, 'heun', None))

    def _inpaint_volumes(self, win):
        """The known volume and the mask as 0/1 floats on the volume's device (``__call__`` has checked their shape)."""
        known, mask = self.inpaint
        return known.to(win.device).contiguous(), mask.to(win.device).float().contiguous()

    def _inpaint_windows(self, kw, mw):
        """What a sampler call takes besides ``x``: the batch's windows of the known volume and of the mask, thresholded."""
        return dict(inpaint_images=kw, inpaint_masks=mw[:, 0] > 0.5, inpaint_resample_times=self.resample_times)

    def __init__(self, configs, sample_fn, nonzero_ratio=0.05, blend=None, sigma_scale=0.125, samples=1, noise=None, seed=0, joint=False,
                 inpaint=None, inpaint_resample_times=5, consistency=None, consistency_weight=1.0, consistency_profile=None,
                 consistency_noise=None, consistency_operator=None, consistency_row_noise=None, consistency_slab=None,
                 consistency_band=None, consistency_heun=None):
        """``sample_fn(lr_patches [B,1,S,S,S]) -> hr_patches`` — e.g. ``lambda x: trainer.sample(batch_size=x.shape[0],
        start_image_or_video=x, start_at_unet_number=2)[0]`` (test_all.py:234).  ``blend`` / ``sigma_scale`` / ``samples``: weighted
        overlap blending and multi-sample statistics, see the module docstring.  ``noise='anchored'`` (with ``seed``): every call
        becomes ``sample_fn(lr_patches, noise=source)`` with the volume-anchored source of that batch's windows and sample index —
        e.g. ``lambda x, noise=None: trainer.sample(batch_size=x.shape[0], start_image_or_video=x, start_at_unet_number=2,
        sampler='ddim', sample_steps=50, noise=noise)[0]``.  ``joint=True`` (needs a blend mode and ``noise='anchored'``): the second
        argument is a window denoiser instead -- ``trainer.window_denoiser(sampler='ddim', sample_steps=50)`` or, second order,
        ``trainer.window_denoiser(sampler='dpmpp2m', sample_steps=16)`` -- see the class docstring.

        ``inpaint=(known, mask)`` with ``inpaint_resample_times=R``: ``known`` fp32 [D,H,W] in the units ``__call__`` returns (the
        z-scored prediction) and ``mask`` bool [D,H,W], True where ``known`` is to be kept while the rest is generated (RePaint).  In the
        crop and blend modes every call becomes ``sample_fn(x[, noise=src], inpaint_images=kw, inpaint_masks=mw,
        inpaint_resample_times=R)`` with the batch's windows of the two volumes; with ``joint=True`` and an EDM Heun denoiser
        (``ElucidatedImagen.window_denoiser()``) or the ancestral denoiser of the DDPM family
        (``Imagen.window_denoiser(sampler='ddpm')``) the loop runs on the one state, so a known region that crosses window borders is
        resampled once, not once per window.  With the EDM family -- and with ``Imagen`` in joint mode when its denoiser was made with
        ``paste_known=True`` -- a known voxel comes back exactly, except where the fill or the background reset applies: they come
        last, as in every mode, and override known values on uncovered and background voxels.  ``Imagen``'s own loop ends on a
        denoising step without a paste (as the reference's does), so there a known voxel comes back as the last step left it.
        ``ValueError`` naming "inpaint" before anything touches the device: a pair that is not (float [D,H,W], bool [D,H,W]) of one
        shape -- or, in ``__call__``, not the volume's --, ``inpaint_resample_times`` that is not a positive integer, joint mode with a
        denoiser that is neither ``heun`` nor one with the ancestral sampler's ``qs`` / ``renoise`` tables (DDIM and the multistep
        chains have no re-noising loop).

        ``consistency=(measurement, cell)`` with ``consistency_weight=w``, and ``consistency_profile``, ``consistency_noise``,
        ``consistency_operator``, ``consistency_row_noise``, ``consistency_slab``, ``consistency_band``, ``consistency_heun`` with it:
        data-consistent sampling; the measurement
        models are in the module docstring, the keywords, their rules and the launch a step takes in ``consistency.py``.
        ``measurement`` is a float tensor [D/fz, H/fy, W/fx] of RAW intensities (host or device) -- with an operator
        [m, D/fz, H/fy, W/fx], one volume per row (``ops.stack_rows`` lays stacks out so, ``ops.tile_measure`` simulates them) -- and
        the noise deviations are in raw units too.  It is put on the high-res grid once per volume (``ops.cell_replicate``, or
        t = A+ y by ``ops.tile_backproject``) and z-scored.  In the crop and blend modes every call becomes ``sample_fn(x[, noise=src],
        consistency=(windows, cell), consistency_weight=w, ...)`` with every other keyword exactly when it was given, the deviations
        divided by std; with ``joint=True`` the projection rides in the fused launch of the three linear chains (the slab: three
        launches per step), the deviations also multiplied by the slope of the denoiser's ``state_space``.  ``ValueError`` naming the
        keyword at fault, and the one that rides on it, before anything touches the device: what ``consistency.py`` lists, together
        with ``inpaint``, joint mode with a Heun denoiser and no ``consistency_heun`` or with one that has no
        ``state_space``, a joint denoiser with no stochastic step
        under a noise deviation, an operator whose rows are not the measurement's leading dimension, a stride or window the cell
        does not divide or cubes whose launch plans more than 64 KiB of LDS (crop and blend modes) -- and, in ``__call__``, a
        measurement that is not the volume's shape divided by the cell."""
        def stochastic():                                    # crop and blend modes: the sampler call knows its own chain
            if joint and hasattr(sample_fn, 'coefs') and not getattr(sample_fn, 'heun', False):
                # kn is the last entry of a first-order row (kx, k0, kn) and of a sigma-space row (kx, k0, kp, kn); the DDPM family's
                # multistep rows (kx, k0, kp) have none
                has_kn = hasattr(sample_fn, 'sigma0') or not getattr(sample_fn, 'multistep', False)
                return has_kn and any(float(r[-1]) != 0.0 for r in sample_fn.coefs.tolist())
            return True

        self.inpaint = self._check_inpaint(inpaint, inpaint_resample_times, joint, sample_fn)
        self.cfg = configs
        tr = configs['Train']
        self.sub = int(tr['patch_size_sub'])
        self.block_mode = bool(tr.get('batch_sample', False))
        self.factor = int(tr.get('batch_sample_factor', 3))
        self.patch = self.sub * self.factor if self.block_mode else self.sub
        self.overlap = int(configs['Eval']['overlap'])
        self.batch = int(configs['Eval'].get('batch_size', 27))
        self.mean, self.std = float(configs['Data']['mean']), float(configs['Data']['std'])
        # the fused launch of a joint chain rides the window's taps; a sampler call of the crop and blend modes sees cubes of `sub`
        self.plan = consistency_plan("VolumeInference", ops, consistency, consistency_weight, consistency_profile, consistency_noise,
                                     consistency_operator, consistency_row_noise, consistency_slab, consistency_band, stochastic=stochastic(),
                                     window=dict(edge=self.sub, stride=self.overlap, joint=bool(joint), denoiser=sample_fn,
                                                 inpaint=self.inpaint is not None, mean=self.mean, std=self.std), heun=consistency_heun)
        self.resample_times = inpaint_resample_times
        if noise not in NOISE_MODES:
            raise ValueError(f"VolumeInference: noise must be None or 'anchored', got {noise!r}")
        self.noise, self.seed = noise, int(seed)
        if blend not in BLEND_MODES:
            raise ValueError(f"VolumeInference: blend must be None, 'gaussian' or 'constant', got {blend!r}")
        if int(samples) != samples or samples < 1:
            raise ValueError(f"VolumeInference: samples must be a positive integer, got {samples!r}")
        if samples > 1 and blend is None:
            raise ValueError("VolumeInference: samples > 1 needs a blend mode ('gaussian' or 'constant'): crop-and-overwrite stitching "
                             "keeps one draw per voxel")
        if blend == 'gaussian' and not sigma_scale > 0:
            raise ValueError(f"VolumeInference: sigma_scale must be positive, got {sigma_scale!r}")
        self.blend, self.sigma_scale, self.samples = blend, float(sigma_scale), int(samples)
        self.joint = bool(joint)
        if self.joint:
            if blend is None or noise != 'anchored':
                raise ValueError("VolumeInference: joint=True needs a blend mode ('gaussian' or 'constant'), the weights that fuse the "
                                 "windows' predictions at every step, and noise='anchored', the volume-wide field the one state starts "
                                 "from and is pushed by")
            missing = [a for a in self._DENOISER if not hasattr(sample_fn, a)]
            if missing:
                raise ValueError(f"VolumeInference: joint=True takes a window denoiser (Imagen.window_denoiser / "
                                 f"ImagenTrainer.window_denoiser) as its second argument; {type(sample_fn).__name__} lacks {missing}")
        self.sample_fn = sample_fn
        self.ratio = nonzero_ratio

    @torch.no_grad()
    def __call__(self, lowres_raw, patch_slice=None, return_std=False):
        """lowres_raw: fp32 [D,H,W] raw intensities on the GPU.  Returns the stitched, z-scored prediction [D,H,W].
        ``patch_slice`` (rank, world) restricts the work to every world-th kept patch (multi-GPU sharding); a rank's volume holds the
        fill value ``(0 - mean) / std`` where it wrote nothing.  Without overlap (stride >= patch) a voxel has one owner and shards
        merge as ``torch.where(a != fill, a, b)``; with overlap the owner is the rank of the last kept window in candidate order whose
        cropped interior covers the voxel, and nothing here does that merge -- shard whole volumes over the ranks instead.
        ``return_std`` (blend modes, ``samples >= 2``): returns ``(mean, std)``, the per-voxel statistics over the samples."""
        if return_std and (self.blend is None or self.samples < 2):
            raise ValueError("VolumeInference: return_std needs a blend mode and samples >= 2")
        if self.inpaint is not None and tuple(self.inpaint[0].shape) != tuple(lowres_raw.shape):
            raise ValueError(f"VolumeInference: the inpaint volumes {tuple(self.inpaint[0].shape)} are not the volume's shape "
                             f"{tuple(lowres_raw.shape)}")
        if self.plan is not None:
            self.plan.admit_volume(lowres_raw.shape)
        if self.blend is not None:
            if patch_slice is not None:
                raise NotImplementedError("VolumeInference: a blend mode does not split one volume's windows over ranks (that needs a "
                                          "cross-rank merge of the weighted sums) — shard whole volumes across the GPUs instead, one "
                                          "VolumeInference call per volume and rank, as bench.py does")
            mean, dev = (self._joint if self.joint else self._blended)(lowres_raw, return_std)
            return (mean, dev) if return_std else mean
        vol = lowres_raw.float().contiguous()
        win = _Windows(self, vol, patch_slice)
        P = self.patch
        margins = crop_margins(win.kept, win.shape, P, self.overlap)
        pred = torch.full(win.shape, win.fill, dtype=torch.float32, device=win.device)
        # cropped interiors (width P - 2*(overlap//2), stride overlap) of neighbouring windows still overlap when the stride is
        # below half a patch: one scatter launch per patch, in candidate order, keeps "later overwrites" deterministic
        serial_scatter = (not self.block_mode) and self.overlap < P and P - 2 * (self.overlap // 2) > self.overlap
        known = self._inpaint_volumes(win) if self.inpaint is not None else ()
        if self.plan is not None:
            known = (self.plan.volume(win.device),)
        for lo, o, idx in win.batches:
            x, _ = ops.patch_gather(vol, idx, P, self.mean, self.std)
            kmw = [self._split(ops.patch_gather(v, idx, P, 0., 1.)[0]) for v in known]            # (v - 0) / 1: the volumes' own bits
            y = self._merge(self._sample(self._split(x), win, o, 0, *kmw)).contiguous()
            mg = torch.from_numpy(np.ascontiguousarray(margins[lo:lo + len(o)])).to(win.device)
            if serial_scatter:
                for j in range(len(o)):
                    ops.patch_scatter(y[j:j + 1], idx[j:j + 1], mg[j:j + 1], pred, P)
            else:
                ops.patch_scatter(y, idx, mg, pred, P)
        ops.background_reset(pred, vol, self.mean, self.std, win.min_val)                # test_all.py:300
        return pred

    def _split(self, w):                                      # block mode: the block as the sampler sees it (test_all.py:229-231)
        return convertVolume2subVolume(w, target_shape=(self.factor ** 3, 1, self.sub, self.sub, self.sub)) if self.block_mode else w

    def _merge(self, y):                                      # fp32; block mode: the sub-volumes back as one block (test_all.py:265-266)
        return merge_sub_volumes(y.float(), original_shape=(1, 1) + (self.patch,) * 3) if self.block_mode else y.float()

    def _sample(self, x, win, origins, s, kw=None, mw=None):
        """One sampler call on the windows at ``origins`` (block mode: ONE block, already split into its sub-volumes), sample ``s``;
        ``kw`` / ``mw``: the same windows of the known volume and of the 0/1 mask when the call inpaints -- or ``kw`` alone, the
        windows of the replicated measurement, when it is held to one."""
        inpaint = {} if kw is None else self.plan.keywords(kw, self.std) if mw is None else self._inpaint_windows(kw, mw)
        if self.noise is None:
            return self.sample_fn(x, **inpaint)
        src = AnchoredNoise(win.shape, self.seed).source(win.noise_origins(origins), self.sub, sample=s, device=x.device)
        return self.sample_fn(x, noise=src, **inpaint)

    def _evaluate(self, win, volumes, call, out):
        """The evaluation loop of the blend and joint paths.  Per batch: gather its windows from every ``(volume, mean, std)`` of
        ``volumes`` (a None volume gives None), split them in block mode, ``call(*windows, host origins)``, merge the result back and
        store it in rows ``lo : lo + n`` of ``out`` [N,P,P,P] -- of ``out[0]``, ``out[1]``, ... in turn when ``call`` yields several."""
        P = self.patch
        for lo, o, idx in win.batches:
            n = len(o)
            w = [None if v is None else self._split(ops.patch_gather(v, idx, P, m, sd)[0]) for v, m, sd in volumes]
            res = call(*w, o)
            for dst, pred in ((out, res),) if torch.is_tensor(res) else zip(out, res):
                dst[lo:lo + n] = self._merge(pred).reshape(n, P, P, P)

    def _blended(self, lowres_raw, want_std):
        """The blend modes: every kept window's S predictions are kept in ``patches`` [S,N,P,P,P]; one ``ops.volume_blend`` launch
        stitches them (weights, mean / deviation over the samples, fill and background reset)."""
        vol = lowres_raw.float().contiguous()
        win = _Windows(self, vol)
        P, S = self.patch, self.samples
        patches = torch.empty((S, win.N, P, P, P), dtype=torch.float32, device=win.device)
        known = [(v, 0., 1.) for v in self._inpaint_volumes(win)] if self.inpaint is not None else []
        if self.plan is not None:
            known = [(self.plan.volume(win.device), 0., 1.)]

        def call(x, *rest):                                  # the windows of the known volume and the mask, or of the measurement (if any), then the origins
            *kmw, o = rest
            return (self._sample(x, win, o, s, *kmw) for s in range(S))
        self._evaluate(win, [(vol, self.mean, self.std)] + known, call, patches)
        return ops.volume_blend(patches, win.slot, win.taps, vol, self.mean, self.std, win.min_val, win.fill, self.overlap, want_std)

    def _joint(self, lowres_raw, want_std):
        """``joint=True``: per sample one chain on whole volumes, then ``ops.volume_joint_finish`` (fill, background reset, running mean
        / deviation over the samples).  ``evaluate(state, cond, x0)`` sends the kept windows of the state, of the low-res volume and of
        ``cond`` (the fused x0 volume, for self-conditioning; or None) through ``x0(xw, lw, sc, origins)`` into ``y`` [N,P,P,P]."""
        vol = lowres_raw.float().contiguous()
        P, S, den = self.patch, self.samples, self._protocol(self.sample_fn)
        win = _Windows(self, vol)
        chain = self._heun_chain if den.heun else self._linear_chain
        y = torch.empty((win.N, P, P, P), dtype=torch.float32, device=win.device)          # reused by every step of every sample
        # and so is the fused x0 volume of the first-order and multistep chains; the Heun chain makes its three volumes per sample
        # (the consistent launch always writes its corrected x0)
        win.x0_vol = torch.empty_like(vol) if (den.self_cond or den.multistep or self.plan is not None) and not den.heun else None

        def evaluate(state, cond, x0):
            self._evaluate(win, [(state, 0., 1.), (vol, self.mean, self.std), (cond, 0., 1.)], x0, y)   # (v - 0) / 1: the state's own bits

        inp = ()
        if self.inpaint is not None:                         # the known volume in state space, the mask as bytes (the kernels') and 0/1
            known, mask_f = self._inpaint_volumes(win)
            inp = (self.sample_fn.normalize(known).contiguous(), mask_f.to(torch.uint8), mask_f)
        # the measurement in state space, the mode's table and the rung of every step: once per volume
        win.consistency = None if self.plan is None else self.plan.prepare(den.coefs, win.device, win.shape)
        mean_io = m2_io = out_std = None
        for s in range(S):
            x = chain(den, win, evaluate, y, s, *inp[:2])
            # with inpainting the denoiser pastes the known values between its clamp and its un-normalisation
            mean_io, m2_io, out_std = ops.volume_joint_finish(den.finish(x, *inp[::2]), win.slot, vol, P, self.overlap, self.mean, self.std,
                                                              win.min_val, win.fill, s, S, mean_io, m2_io, want_std)
        return mean_io, out_std

    def _window_x0(self, den, win, s, i, edm=False, **kw):
        """``x0(xw, lw, sc, origins)`` as ``evaluate`` calls it: the denoiser's x0 prediction of step ``i``.  An EDM denoiser (``edm``)
        also takes ``lowres_noise=``: draw 0 of the field at the batch's windows when the chain's own draws start at 1 (recomputed per
        evaluation, nothing is kept), else None."""
        def x0(xw, lw, sc, o):
            if not edm:
                return den.x0(xw, lw, i, self_cond=sc, **kw)
            ln = ops.anchored_noise(win.noise_origins(o), lw.shape[1], self.sub, *win.shape, self.seed, draw=0, sample=s,
                                    device=win.device) if den.draw_base else None
            return den.x0(xw, lw, i, self_cond=sc, lowres_noise=ln, **kw)
        return x0

    def _linear_chain(self, den, win, evaluate, y, s, known=None, mask=None):
        """Sample ``s`` of a chain whose step is ONE fused launch, in place on the state ``x`` and on ``win.x0_vol`` (the fused x0, which
        self-conditioning gathers at the next step and the multistep families read as their history term before it is overwritten).
        The family chooses the first state and the launch; the draws are the module docstring's.

        With ``known`` (fp32 [D,H,W] in state space) and ``mask`` (uint8 [D,H,W]) the ancestral chain inpaints (``_check_inpaint`` has
        admitted the denoiser): the initial image under the first paste (``ops.volume_joint_step_inpaint_init``), then T steps of
        ``self.resample_times`` passes, each one evaluation and ONE ``ops.volume_joint_step_inpaint`` launch that carries the step, the
        re-noise of a pass that is neither the last of its step nor in the step that ends at t = 0 (flags bit 0) and the paste of the
        next pass with that pass's (alpha, sigma) (bit 1) -- 1 + R T fused launches.  ONE draw counter advances as the per-window
        ``p_sample_loop`` calls its source: the initial image, then per pass the q-noise, the step noise (counted also where kn == 0)
        and, where there is one, the re-noise -- so at stride = patch the chain is ``sample(noise=source, inpaint_images=...)`` per
        window."""
        if known is not None:
            T = den.num_steps
            passes = [(i, r) for i in range(T) for r in reversed(range(self.resample_times))]
            x = ops.volume_joint_step_inpaint_init(known, mask, *den.qs[0], self.seed, draw=0, draw_q=1, sample=s)
            draw = 2                                         # the next draw of the state: the initial image and the first q-noise are taken
            for n, (i, r) in enumerate(passes):
                evaluate(x, win.x0_vol if den.self_cond and n > 0 else None, self._window_x0(den, win, s, i))
                renoise, more = r > 0 and i + 1 < T, n + 1 < len(passes)
                ops.volume_joint_step_inpaint(y, win.slot, win.taps, x, known, mask, int(renoise) + 2 * int(more), *den.coefs[i],
                                              den.renoise[i] if renoise else (0., 0.), den.qs[passes[n + 1][0]] if more else (0., 0.),
                                              *den.clamp, self.overlap, self.seed, draw=draw, draw_r=draw + 1 if renoise else 0,
                                              draw_q=draw + 1 + renoise if more else 0, sample=s, x0_out=win.x0_vol)
                draw += 1 + int(renoise) + int(more)
            return x
        if den.sigma_space:                                  # sigma0 n(draw_base)
            x, _ = ops.volume_joint_multistep_sde(None, None, None, None, None, 0., 0., 0., den.sigma0, *den.clamp, self.overlap, self.seed,
                                                  draw=den.draw_base, sample=s, shape=win.shape, device=win.device)
        else:                                                # n(0)
            x = ops.volume_joint_init(win.shape, self.seed, sample=s, device=win.device)
        head, tail, io = (y, win.slot, win.taps, x), (*den.clamp, self.overlap), dict(out=x, x0_out=win.x0_vol)
        form = 2 if den.sigma_space else 1 if den.multistep else 0
        for i in range(den.num_steps):
            evaluate(x, win.x0_vol if den.self_cond and i > 0 else None, self._window_x0(den, win, s, i, edm=den.sigma_space))
            prev = win.x0_vol if i else None
            draw = den.draw_base + 1 + i if den.sigma_space else i + 1
            # under consistency the same three updates behind the projection of the fused x0, unless the step's rung is the plain one
            if win.consistency is not None and win.consistency.joint_step(i, head, prev, form, den.coefs[i], tail, self.seed, draw, s, io):
                continue
            if den.sigma_space:                              # coefs[i] = (kx, k0, kp, kn): + kp x0_prev + kn n(draw_base + 1 + i)
                ops.volume_joint_multistep_sde(*head, prev, *den.coefs[i], *tail, self.seed, draw=draw, sample=s, **io)
            elif den.multistep:                              # (kx, k0, kp): + kp x0_prev; only draw 0 of the field is used
                ops.volume_joint_multistep(*head, prev, *den.coefs[i], *tail, **io)
            else:                                            # (kx, k0, kn): + kn n(i + 1)
                ops.volume_joint_step(*head, *den.coefs[i], *tail, self.seed, draw=draw, sample=s, **io)
        return x

    def _heun_chain(self, den, win, evaluate, y, s, known=None, mask=None):
        """Sample ``s`` of the chain of an EDM window denoiser (module docstring): ``xh`` (images_hat), ``xn`` (images_next) and ``x0_vol``
        (the fused prediction, which self-conditioning gathers) are advanced in place by ``ops.volume_joint_heun`` -- under
        ``consistency_heun`` by ``ops.volume_joint_consistent_heun`` in the phases ``consistency.Chain.joint_heun`` projects;
        ``predict`` evaluates the windows of one of them into ``y``, with draw 0 of the field at each batch as its low-res noise.
        The initial image is draw
        ``den.draw_base``, the eps of step i draw ``den.draw_base + 1 + i``.  Returns the volume the chain ends in.

        With ``known`` (fp32 [D,H,W] in state space) and ``mask`` (uint8 [D,H,W]) the chain inpaints: every step runs
        ``self.resample_times`` passes, each the two evaluations above; the pass boundary -- the re-noise of a pass that is neither the
        last of its step nor in the last step, the paste, the churn of the next pass -- rides in the corrector launch
        (``ops.volume_joint_heun_inpaint`` phase 2), or is a launch of its own (phase 3) on the step that ends at sigma 0, which has no
        corrector.  The state's draws are numbered by ONE counter that advances as the per-window sampler calls its source: the initial
        image, then per pass the eps and, where there is one, the re-noise normal -- so at stride = patch the chain is
        ``sample(noise=source, inpaint_images=...)`` per window."""
        base, T = den.draw_base, den.num_steps
        R = self.resample_times if known is not None else 1
        if known is None:
            xh = ops.volume_joint_heun_init(win.shape, den.sigma0, den.coefs[0][0], self.seed, draw=base, sample=s, device=win.device)
        else:
            xh = ops.volume_joint_heun_inpaint_init(known, mask, den.sigma0, den.coefs[0][0], self.seed, draw=base, sample=s)
        xn, x0_vol = torch.empty_like(xh), torch.empty_like(xh)
        head, tail, dc = (y, win.slot, win.taps, xh, xn, x0_vol), (*den.clamp, self.overlap), win.consistency

        def predict(state, i, stage, first):
            evaluate(state, x0_vol if den.self_cond and not first else None, self._window_x0(den, win, s, i, edm=True, stage=stage))

        corrected, draw = False, base + 2                    # the next draw of the state: the initial image and the first eps are taken
        for i in range(T):
            _, a1, b1, a2, b2, c2, d2 = den.coefs[i]
            sigma, sigma_next = float(den.sched[i][0]), float(den.sched[i][1])
            for r in reversed(range(R)):
                predict(xh, i, 0, i == 0 and r == R - 1)
                # under consistency the same update behind the projection of the fused prediction
                if dc is None or not dc.joint_heun(i, 1, head, (a1, b1), 0., tail, 0, 0, 0):      # the predictor reads no normal
                    ops.volume_joint_heun(*head, 1, (a1, b1), 0., *tail)
                corrected = sigma_next != 0
                more = r > 0 or i + 1 < T                    # another pass follows: this launch churns for it
                renoise = r > 0 and i + 1 < T
                kc = (den.coefs[i][0] if r > 0 else den.coefs[i + 1][0]) if more else 0.
                if corrected:                                # no corrector on the step that ends at sigma 0
                    predict(xn, i, 1, False)
                    if known is None:
                        if dc is None or not dc.joint_heun(i, 2, head, (a2, b2, c2, d2), kc, tail, self.seed, draw if more else 0, s):
                            ops.volume_joint_heun(*head, 2, (a2, b2, c2, d2), kc, *tail, self.seed, draw=draw if more else 0, sample=s)
                    else:
                        ops.volume_joint_heun_inpaint(y, win.slot, win.taps, xh, xn, x0_vol, known, mask, 2, (a2, b2, c2, d2),
                                                      sigma - sigma_next if renoise else 0., kc, *den.clamp, self.overlap, self.seed,
                                                      draw=draw + renoise if more else 0, draw_r=draw if renoise else 0, sample=s)
                elif known is not None and more:
                    if renoise:
                        raise ValueError("VolumeInference: inpaint: a step that ends at sigma 0 before the last one has no corrector to "
                                         "carry its re-noise")
                    ops.volume_joint_heun_inpaint(None, None, None, xh, xn, x0_vol, known, mask, 3, (), 0., kc, *den.clamp, self.overlap,
                                                  self.seed, draw=draw, sample=s)
                draw += int(renoise) + int(more)
        return xh if corrected else xn


def eval_crop(size0):
    """test_all.py:49-54: voxels cut from every face of all three axes, decided by the size of axis 0 alone."""
    return 24 if size0 == 240 else (32 if size0 == 256 else 0)


def _minmax_normalised(x):
    mm = ops.minmax(x)
    return (x - mm[0]) / (mm[1] - mm[0])


@torch.no_grad()
def evaluate_volume(gt, pred):
    """``eval(gt, pred)`` of the evaluation script (test_all.py:47-62) without LPIPS, on the device.  gt / pred: ``[D,H,W]`` numpy
    arrays or tensors — what ``VolumeInference.__call__`` returns is taken as it is, in HBM.  Both are centre-cropped (24 per face
    for a 240-voxel axis 0, 32 for 256, otherwise not at all); ``psnr = PSNR(gt, pred)`` on the cropped raw volumes; each cropped
    volume is min-max normalised by its own extrema; ``ssim = MSSIM(gt_n, pred_n)``.  Returns ``(ssim, psnr)`` in the script's
    order, 0-d tensors on the device ``gt`` came from (the CPU for numpy arrays)."""
    gt, pred = torch.as_tensor(gt), torch.as_tensor(pred)
    if gt.ndim != 3 or gt.shape != pred.shape:
        raise ValueError(f"evaluate_volume: expected two [D,H,W] volumes of one shape, got {tuple(gt.shape)} and {tuple(pred.shape)}")
    home = gt.device
    c = eval_crop(gt.shape[0])
    if c:
        gt, pred = gt[c:-c, c:-c, c:-c], pred[c:-c, c:-c, c:-c]
    if any(s // 16 <= 10 for s in gt.shape):                         # MSSIM's size rule, before anything is copied or launched
        raise ValueError(f"evaluate_volume: the cropped volume {tuple(gt.shape)} is too small for the 5-scale MS-SSIM")
    if not torch.cuda.is_available():
        raise RuntimeError("diffusioniqt_amd.inference.evaluate_volume runs on the MI355X only (no CPU fallback)")
    dev = gt.device if gt.is_cuda else torch.device('cuda')
    g = gt.to(dev).float().contiguous()[None, None]
    p = pred.to(dev).float().contiguous()[None, None]
    psnr = PSNR(g, p)
    ssim = MSSIM(_minmax_normalised(g), _minmax_normalised(p))
    return ssim.to(home), psnr.to(home)
