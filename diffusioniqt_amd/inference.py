"""Whole-volume inference — the sliding-window loop of the reference's test scripts (test_all.py:182-300, test.py) with its
dataset (`supervisedIQT_INF`, data.py:138-202), kept on the device: the raw low-res volume stays resident in HBM, patches are
gathered / normalised / rejected by one kernel, sampled in batches, stitched by a scatter kernel that applies the script's
overlap-crop rules, and the background is reset in place.  One job per volume; several volumes or patch ranges shard over
GPUs with no collective.

Semantics kept from the scripts:
* candidate origins: ``range(0, N - P + 1, overlap)`` per axis, i outermost (data.py:157-160; ``Eval.overlap`` is the STRIDE);
* a candidate is dropped when fewer than 5 % of its RAW voxels are non-zero (data.py:187-191);
* patches are z-scored with ``Data.mean/std`` (data.py:165-169); the output volume starts at ``(0 - mean) / std``;
* ``Train.batch_sample``: the window is ``patch_size_sub * batch_sample_factor`` (96), each block is split into 27 sub-volumes
  for the sampler and merged back (utils_mine.py:25-67); blocks overlap, and each writes its interior ``[op : P - op]``
  (``op = overlap // 2``) except on faces that touch the volume boundary (test_all.py:267-296);
* without ``batch_sample`` and with ``overlap >= patch`` patches are placed whole (test_all.py:262-263).  The script's
  overlap < patch branch of that mode raises on its first interior patch (a 3-element tensor in a boolean ``or``,
  test_all.py:241) — here it applies the same per-face crop rule as the block mode instead;
* voxels whose normalised low-res value equals the volume minimum are reset to it (test_all.py:300);
* ``evaluate_volume`` scores the stitched volume as the script's ``eval`` does (test_all.py:47-62): centre crop, PSNR, MS-SSIM of
  the min-max normalised pair — without LPIPS (no VGG weights here).

Beyond the scripts (``blend`` / ``samples``; the defaults leave every line above as it is):
* ``blend='gaussian'`` / ``'constant'`` replaces crop-and-overwrite by weighted overlap blending: whole windows contribute (no crop
  margins), each voxel is the weighted mean of the windows that cover it, with the separable weight ``taps[i] taps[j] taps[k]``
  (``blend_taps``: a Gaussian importance map of sigma ``sigma_scale * P`` with maximum 1, or all ones = the plain mean).  Every kept
  window's prediction stays in HBM and ONE gather-side launch (``ops.volume_blend``) reduces them per output voxel in candidate
  order — no atomics, bit-reproducible, independent of ``Eval.batch_size``; the background reset is fused into it.  A voxel that no
  kept window covers keeps the fill value ``(0 - mean) / std``;
* ``samples=S`` draws every batch S times (sample 0 of a batch, then sample 1, ...); the result is the per-voxel mean of the S
  blended volumes and, with ``return_std=True``, their unbiased standard deviation — the uncertainty map of a stochastic sampler;
* ``noise='anchored'`` hands the sampler a noise source tied to the VOLUME instead of letting every batch draw its own: the value at
  global voxel (z, y, x) of draw k and sample s is a pure function of (seed, z, y, x, k, s) (``AnchoredNoise``, one Philox4x32-10 call
  per voxel in ``ops.anchored_noise``), so all windows that cover a voxel start from — and, in a stochastic sampler, are pushed by —
  the same numbers, whatever ``Eval.batch_size`` is, whichever windows the non-zero filter kept and in whatever order or on
  whichever rank they run.  What is left of the disagreement between overlapping windows is what the network does differently with
  different context; the ``samples = S`` fields are independent of each other and coherent across windows;
* ``joint=True`` (with a blend mode and ``noise='anchored'``) removes that remainder at its source: instead of running every window's
  reverse chain alone and blending finished patches, ONE noisy state of the whole volume is kept and the windows' x0 predictions are
  fused at EVERY step (MultiDiffusion, Bar-Tal et al. 2023).  The second constructor argument is then a window denoiser
  (``Imagen.window_denoiser`` / ``ImagenTrainer.window_denoiser``: scalar step coefficients, the clamp, ``x0`` and ``finish``).  Per
  sample: the state starts as draw 0 of the anchored field; every step gathers the kept windows of the state, evaluates the U-Net on
  them in ``Eval.batch_size`` batches (N windows x T steps evaluations, as many as the independent windows cost) and ONE
  ``ops.volume_joint_step`` launch blends the predictions per voxel with the blend weights, takes the sampler step with draw
  ``i + 1`` and writes the next state in place; ``ops.volume_joint_finish`` applies the fill / background rules and the statistics
  over the samples.  The draw numbering is ``AnchoredNoise.source``'s, so with stride = patch (no overlap) the joint chain IS the
  independent one, bit for bit;
* ``sampler='dpmpp2m'`` (DPM-Solver++ 2M, the second-order multistep solver; ``Imagen.p_sample_loop``) works in every mode above: the
  non-joint modes only pass it to ``sample``; a joint chain made with ``window_denoiser(sampler='dpmpp2m', sample_steps=K)`` keeps the
  fused x0 volume of the previous step and takes ``ops.volume_joint_multistep``, x_next = kx x + k0 x0 + kp x0_prev, per step.  It is
  deterministic after draw 0, and at stride = patch again the independent chain bit for bit;
* the EDM family (``ElucidatedImagen``) takes the same modes.  ``ElucidatedImagen.sample(noise=source)`` accepts the anchored source
  (exactly one U-Net sampled): draw 0 is the low-res augmentation noise, draw 1 the initial image, draw 2 + i the eps of Heun step i.  A
  joint chain made with ``ElucidatedImagen.window_denoiser()`` / ``ImagenTrainer.window_denoiser()`` (``den.heun``) runs the stochastic
  Heun sampler on three volumes -- images_hat, images_next and the fused prediction -- and fuses the windows after BOTH U-Net
  evaluations of a step: ``ops.volume_joint_heun_init`` (initial image + first churn), then per step the windows of images_hat evaluated
  at sigma_hat and ``ops.volume_joint_heun`` phase 1 (predictor), the windows of images_next evaluated at sigma_next and phase 2
  (corrector + the next step's churn) -- 2 T - 1 fused launches for T steps, twice the U-Net evaluations of a first-order chain.  The
  low-res noise of a batch is draw 0 of the field at its windows, recomputed per evaluation; the draw numbering is the source's, so
  at stride = patch the joint chain is ``sample(noise=source)`` per window, bit for bit.
"""
import numpy as np
import torch

from . import ops
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


class VolumeInference:
    def __init__(self, configs, sample_fn, nonzero_ratio=0.05, blend=None, sigma_scale=0.125, samples=1, noise=None, seed=0, joint=False):
        """``sample_fn(lr_patches [B,1,S,S,S]) -> hr_patches`` — e.g. ``lambda x: trainer.sample(batch_size=x.shape[0],
        start_image_or_video=x, start_at_unet_number=2)[0]`` (test_all.py:234).  ``blend`` / ``sigma_scale`` / ``samples``: weighted
        overlap blending and multi-sample statistics, see the module docstring.  ``noise='anchored'`` (with ``seed``): every call
        becomes ``sample_fn(lr_patches, noise=source)`` with the volume-anchored source of that batch's windows and sample index —
        e.g. ``lambda x, noise=None: trainer.sample(batch_size=x.shape[0], start_image_or_video=x, start_at_unet_number=2,
        sampler='ddim', sample_steps=50, noise=noise)[0]``.  ``joint=True`` (needs a blend mode and ``noise='anchored'``): the second
        argument is a window denoiser instead -- ``trainer.window_denoiser(sampler='ddim', sample_steps=50)`` or, second order,
        ``trainer.window_denoiser(sampler='dpmpp2m', sample_steps=16)`` -- and the windows are sampled in lockstep on one noisy state
        of the whole volume, see the module docstring."""
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
            missing = [a for a in ('num_steps', 'coefs', 'clamp', 'x0', 'finish') if not hasattr(sample_fn, a)]
            if missing:
                raise ValueError(f"VolumeInference: joint=True takes a window denoiser (Imagen.window_denoiser / "
                                 f"ImagenTrainer.window_denoiser) as its second argument; {type(sample_fn).__name__} lacks {missing}")
        self.cfg = configs
        self.sample_fn = sample_fn
        self.ratio = nonzero_ratio
        tr = configs['Train']
        self.sub = int(tr['patch_size_sub'])
        self.block_mode = bool(tr.get('batch_sample', False))
        self.factor = int(tr.get('batch_sample_factor', 3))
        self.patch = self.sub * self.factor if self.block_mode else self.sub
        self.overlap = int(configs['Eval']['overlap'])
        self.batch = int(configs['Eval'].get('batch_size', 27))
        self.mean, self.std = float(configs['Data']['mean']), float(configs['Data']['std'])

    @torch.no_grad()
    def __call__(self, lowres_raw, patch_slice=None, return_std=False):
        """lowres_raw: fp32 [D,H,W] raw intensities on the GPU.  Returns the stitched, z-scored prediction [D,H,W].
        ``patch_slice`` (rank, world) restricts the work to every world-th kept patch (multi-GPU sharding; merge the shards with
        the returned mask-free volumes by taking, per voxel, the value of the rank that owns it — see ``shard_volumes``).
        ``return_std`` (blend modes, ``samples >= 2``): returns ``(mean, std)``, the per-voxel statistics over the samples."""
        if return_std and (self.blend is None or self.samples < 2):
            raise ValueError("VolumeInference: return_std needs a blend mode and samples >= 2")
        if self.blend is not None:
            if patch_slice is not None:
                raise NotImplementedError("VolumeInference: a blend mode does not split one volume's windows over ranks (that needs a "
                                          "cross-rank merge of the weighted sums) — shard whole volumes across the GPUs instead, one "
                                          "VolumeInference call per volume and rank, as bench.py does")
            mean, dev = (self._joint if self.joint else self._blended)(lowres_raw, return_std)
            return (mean, dev) if return_std else mean
        vol = lowres_raw.float().contiguous()
        dev = vol.device
        shape = tuple(vol.shape)
        P = self.patch
        origins = sliding_window_origins(shape, P, self.overlap)
        idx_all = torch.from_numpy(origins).to(dev)
        _, nz = ops.patch_gather(vol, idx_all, P, self.mean, self.std, want_patches=False, want_nonzero=True)
        keep = (nz.cpu().numpy().astype(np.float64) / float(P ** 3)) >= self.ratio          # data.py:187-191
        kept = origins[keep]
        if patch_slice is not None:
            rank, world = patch_slice
            kept = kept[rank::world]
        margins = crop_margins(kept, shape, P, self.overlap)
        mean32, std32 = np.float32(self.mean), np.float32(self.std)
        pred = torch.full(shape, float((np.float32(0.) - mean32) / std32), dtype=torch.float32, device=dev)
        # overlapping blocks are written one launch at a time in candidate order (later blocks overwrite, as in the script);
        # non-overlapping patches go out in one launch per batch
        per_call = 1 if self.block_mode else self.batch
        # cropped interiors (width P - 2*(overlap//2), stride overlap) of neighbouring windows still overlap when the stride is
        # below half a patch: one scatter launch per patch, in candidate order, keeps "later overwrites" deterministic
        serial_scatter = (not self.block_mode) and self.overlap < P and P - 2 * (self.overlap // 2) > self.overlap
        for lo in range(0, kept.shape[0], per_call):
            o = np.ascontiguousarray(kept[lo:lo + per_call])
            idx = torch.from_numpy(o).to(dev)
            x, _ = ops.patch_gather(vol, idx, P, self.mean, self.std)
            if self.block_mode:                                                           # test_all.py:229-231, 265-266
                sub = convertVolume2subVolume(x, target_shape=(self.factor ** 3, 1, self.sub, self.sub, self.sub))
                y = self._sample(sub, o, shape, 0)
                y = merge_sub_volumes(y.float(), original_shape=(1, 1, P, P, P))
            else:
                y = self._sample(x, o, shape, 0)
            y = y.float().contiguous()
            mg = torch.from_numpy(np.ascontiguousarray(margins[lo:lo + per_call])).to(dev)
            if serial_scatter:
                for j in range(o.shape[0]):
                    ops.patch_scatter(y[j:j + 1], idx[j:j + 1], mg[j:j + 1], pred, P)
            else:
                ops.patch_scatter(y, idx, mg, pred, P)
        min_raw = float(ops.min_value(vol).item())
        min_val = (np.float32(min_raw) - mean32) / std32                                  # monotone map: min of the normalised volume
        ops.background_reset(pred, vol, self.mean, self.std, float(min_val))             # test_all.py:300
        return pred

    def _sample(self, x, origins, volume_shape, s):
        """One sampler call on the windows at ``origins`` (block mode: ONE block, already split into its sub-volumes), sample ``s``."""
        if self.noise is None:
            return self.sample_fn(x)
        if self.block_mode:
            origins = sub_volume_origins(origins[0], self.factor, self.sub)
        src = AnchoredNoise(volume_shape, self.seed).source(origins, self.sub, sample=s, device=x.device)
        return self.sample_fn(x, noise=src)

    def _blended(self, lowres_raw, want_std):
        """The blend modes: every kept window's S predictions are kept in ``patches`` [S,N,P,P,P]; one ``ops.volume_blend`` launch
        stitches them (weights, mean / deviation over the samples, fill and background reset)."""
        vol = lowres_raw.float().contiguous()
        dev = vol.device
        shape = tuple(vol.shape)
        P, S = self.patch, self.samples
        origins = sliding_window_origins(shape, P, self.overlap)
        lattice = tuple(len(range(0, s - P + 1, self.overlap)) for s in shape)
        _, nz = ops.patch_gather(vol, torch.from_numpy(origins).to(dev), P, self.mean, self.std, want_patches=False, want_nonzero=True)
        keep = (nz.cpu().numpy().astype(np.float64) / float(P ** 3)) >= self.ratio          # data.py:187-191
        kept = origins[keep]
        N = kept.shape[0]
        slot = np.full(origins.shape[0], -1, dtype=np.int32)                                 # candidate order = lattice order
        slot[keep] = np.arange(N, dtype=np.int32)
        patches = torch.empty((S, N, P, P, P), dtype=torch.float32, device=dev)
        per_call = 1 if self.block_mode else self.batch
        for lo in range(0, N, per_call):
            o = np.ascontiguousarray(kept[lo:lo + per_call])
            idx = torch.from_numpy(o).to(dev)
            n = idx.shape[0]
            x, _ = ops.patch_gather(vol, idx, P, self.mean, self.std)
            if self.block_mode:                                                           # test_all.py:229-231, 265-266
                x = convertVolume2subVolume(x, target_shape=(self.factor ** 3, 1, self.sub, self.sub, self.sub))
            for s in range(S):
                y = self._sample(x, o, shape, s)
                if self.block_mode:
                    y = merge_sub_volumes(y.float(), original_shape=(1, 1, P, P, P))
                patches[s, lo:lo + n] = y.float().reshape(n, P, P, P)
        mean32, std32 = np.float32(self.mean), np.float32(self.std)
        fill = (np.float32(0.) - mean32) / std32
        min_val = (np.float32(float(ops.min_value(vol).item())) - mean32) / std32
        taps = torch.from_numpy(blend_taps(P, self.blend, self.sigma_scale)).to(dev)
        return ops.volume_blend(patches, torch.from_numpy(slot.reshape(lattice)).to(dev), taps, vol, self.mean, self.std,
                                float(min_val), float(fill), self.overlap, want_std)


    def _joint(self, lowres_raw, want_std):
        """``joint=True``: per sample ONE noisy state ``x`` [D,H,W] for the whole volume.  Every step gathers the kept windows of the
        state (and of the low-res volume, and of the previous fused x0 for a self-conditioned U-Net), lets the window denoiser predict
        their x0 into one [N,P,P,P] buffer, and ONE ``ops.volume_joint_step`` launch fuses the predictions per voxel, takes the sampler
        step with draw ``i + 1`` of the anchored field and writes the next state in place.  ``ops.volume_joint_finish`` ends a sample:
        fill, background reset and the running mean / deviation over the samples.  A multistep denoiser (``sampler='dpmpp2m'``,
        ``den.multistep``) takes ``ops.volume_joint_multistep`` instead: the third operand of the update is the fused x0 volume of the
        previous step (the one self-conditioning reads), kept and overwritten in place, and only draw 0 of the field is used."""
        vol = lowres_raw.float().contiguous()
        dev = vol.device
        shape = tuple(vol.shape)
        P, S, den = self.patch, self.samples, self.sample_fn
        origins = sliding_window_origins(shape, P, self.overlap)
        lattice = tuple(len(range(0, s - P + 1, self.overlap)) for s in shape)
        _, nz = ops.patch_gather(vol, torch.from_numpy(origins).to(dev), P, self.mean, self.std, want_patches=False, want_nonzero=True)
        keep = (nz.cpu().numpy().astype(np.float64) / float(P ** 3)) >= self.ratio          # data.py:187-191
        kept = origins[keep]
        N = kept.shape[0]
        slot = np.full(origins.shape[0], -1, dtype=np.int32)                                 # candidate order = lattice order
        slot[keep] = np.arange(N, dtype=np.int32)
        slot = torch.from_numpy(slot.reshape(lattice)).to(dev)
        taps = torch.from_numpy(blend_taps(P, self.blend, self.sigma_scale)).to(dev)
        per_call = 1 if self.block_mode else self.batch
        batches = [(lo, torch.from_numpy(np.ascontiguousarray(kept[lo:lo + per_call])).to(dev)) for lo in range(0, N, per_call)]
        sub_shape = (self.factor ** 3, 1, self.sub, self.sub, self.sub)
        split = (lambda w: convertVolume2subVolume(w, target_shape=sub_shape)) if self.block_mode else (lambda w: w)
        coefs = den.coefs.tolist()
        lo_c, hi_c, mode_c = den.clamp
        self_cond = bool(getattr(den, 'self_cond', False))
        mean32, std32 = np.float32(self.mean), np.float32(self.std)
        fill = (np.float32(0.) - mean32) / std32
        min_val = (np.float32(float(ops.min_value(vol).item())) - mean32) / std32
        y = torch.empty((N, P, P, P), dtype=torch.float32, device=dev)                       # reused by every step of every sample
        multistep = bool(getattr(den, 'multistep', False))                                   # 'dpmpp2m': coefs rows are (kx, k0, kp)
        x0_vol = torch.empty(shape, dtype=torch.float32, device=dev) if self_cond or multistep else None
        mean_io = m2_io = out_std = None
        for s in range(S):
            if getattr(den, 'heun', False):                  # the EDM family: three volumes, two evaluations per step (_heun_chain)
                x = self._heun_chain(den, vol, batches, kept, split, y, slot, taps, s)
                mean_io, m2_io, out_std = ops.volume_joint_finish(den.finish(x), slot, vol, P, self.overlap, self.mean, self.std,
                                                                  float(min_val), float(fill), s, S, mean_io, m2_io, want_std)
                continue
            x = ops.volume_joint_init(shape, self.seed, sample=s, device=dev)               # draw 0
            for i in range(den.num_steps):
                for lo, idx in batches:
                    n = idx.shape[0]
                    xw = split(ops.patch_gather(x, idx, P, 0., 1.)[0])                       # (v - 0) / 1: the state's own bits
                    lw = split(ops.patch_gather(vol, idx, P, self.mean, self.std)[0])
                    sc = split(ops.patch_gather(x0_vol, idx, P, 0., 1.)[0]) if self_cond and i > 0 else None
                    pred = den.x0(xw, lw, i, self_cond=sc).float()
                    if self.block_mode:                                                   # test_all.py:229-231, 265-266
                        pred = merge_sub_volumes(pred, original_shape=(1, 1, P, P, P))
                    y[lo:lo + n] = pred.reshape(n, P, P, P)
                kx, k0, kn = coefs[i]
                if multistep:                                # x0_vol is read as the previous fused x0, then overwritten with this one
                    ops.volume_joint_multistep(y, slot, taps, x, x0_vol if i else None, kx, k0, kn, lo_c, hi_c, mode_c, self.overlap,
                                               out=x, x0_out=x0_vol)
                else:
                    ops.volume_joint_step(y, slot, taps, x, kx, k0, kn, lo_c, hi_c, mode_c, self.overlap, self.seed, draw=i + 1,
                                          sample=s, out=x, x0_out=x0_vol)
            mean_io, m2_io, out_std = ops.volume_joint_finish(den.finish(x), slot, vol, P, self.overlap, self.mean, self.std,
                                                              float(min_val), float(fill), s, S, mean_io, m2_io, want_std)
        return mean_io, out_std

    def _heun_chain(self, den, vol, batches, kept, split, y, slot, taps, s):
        """Sample ``s`` of the joint chain of an EDM window denoiser (``den.heun``; ``ElucidatedImagen.window_denoiser``): the stochastic
        Heun sampler on three volumes -- ``xh`` (images_hat), ``xn`` (images_next) and ``x0`` (the fused prediction, which
        self-conditioning gathers) -- advanced in place by ``ops.volume_joint_heun``.  Phase 0 makes the initial image and the churn of
        step 0; every step gathers the ``xh`` windows, evaluates them at sigma_hat into ``y`` and takes the predictor (phase 1), then,
        unless sigma_next is 0, gathers the ``xn`` windows, evaluates them at sigma_next and takes the corrector together with the next
        step's churn (phase 2): 2 T - 1 fused launches for T steps.  The low-res augmentation noise of a batch is draw 0 of the anchored
        field at its windows, recomputed where it is used; the initial image is draw ``den.draw_base`` and the eps of step i draw
        ``den.draw_base + 1 + i`` -- the numbering ``AnchoredNoise.source`` gives ``ElucidatedImagen.sample(noise=source)``.  Returns the
        volume the chain ends in."""
        dev, shape, P = vol.device, tuple(vol.shape), self.patch
        coefs = den.coefs.tolist()
        lo_c, hi_c, mode_c = den.clamp
        self_cond, base, T = bool(getattr(den, 'self_cond', False)), int(den.draw_base), den.num_steps
        xh = ops.volume_joint_heun_init(shape, den.sigma0, coefs[0][0], self.seed, draw=base, sample=s, device=dev)
        xn, x0_vol = torch.empty_like(xh), torch.empty_like(xh)

        def evaluate(state, i, stage):
            for lo, idx in batches:
                n = idx.shape[0]
                xw = split(ops.patch_gather(state, idx, P, 0., 1.)[0])                   # (v - 0) / 1: the state's own bits
                lw = split(ops.patch_gather(vol, idx, P, self.mean, self.std)[0])
                sc = split(ops.patch_gather(x0_vol, idx, P, 0., 1.)[0]) if self_cond and (i > 0 or stage == 1) else None
                ln = None
                if base:                                     # block mode: the sub-volumes' own origins, as in _sample
                    org = sub_volume_origins(kept[lo], self.factor, self.sub) if self.block_mode else kept[lo:lo + n]
                    ln = ops.anchored_noise(org, lw.shape[1], self.sub, *shape, self.seed, draw=0, sample=s, device=dev)
                pred = den.x0(xw, lw, i, self_cond=sc, stage=stage, lowres_noise=ln).float()
                if self.block_mode:                                                   # test_all.py:229-231, 265-266
                    pred = merge_sub_volumes(pred, original_shape=(1, 1, P, P, P))
                y[lo:lo + n] = pred.reshape(n, P, P, P)

        corrected = False
        for i in range(T):
            _, a1, b1, a2, b2, c2, d2 = coefs[i]
            evaluate(xh, i, 0)
            ops.volume_joint_heun(y, slot, taps, xh, xn, x0_vol, 1, (a1, b1), 0., lo_c, hi_c, mode_c, self.overlap)
            corrected = float(den.sched[i][1]) != 0
            if corrected:                                    # no corrector on the step that ends at sigma 0
                evaluate(xn, i, 1)
                more = i + 1 < T
                ops.volume_joint_heun(y, slot, taps, xh, xn, x0_vol, 2, (a2, b2, c2, d2), coefs[i + 1][0] if more else 0., lo_c, hi_c,
                                      mode_c, self.overlap, self.seed, draw=base + 2 + i if more else 0, sample=s)
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
