"""MI355X-native counterpart of the reference's ``elucidated_imagen.ElucidatedImagen`` (EDM / Karras et al.):
preconditioning (elucidated_imagen.py:314-358), sigma schedule (:365-379), stochastic Heun sampler (:382-532),
cascade ``sample`` (:536-702) and the weighted training loss (:706-882), text-free IQT configuration.

Every per-voxel operation is a HIP kernel (``ops.axpby3`` folds the scalar coefficients of a sampler sub-step into
ONE pass; the training loss is one fused weighted-MSE kernel).  The sigma / gamma / c_* scalars are host Python
floats computed once before the loop (the reference pulls them from the device with ``.item()`` every step, :471).

Superset of the reference: it also drives the true-Conv3d Family-A ``Unet`` (``forward(x, c_noise)``), which the
reference cannot.
"""
from collections import namedtuple
from contextlib import contextmanager, nullcontext
from functools import partial
from math import exp, expm1, log, sqrt
from random import random

import torch
from torch import nn

from . import ops
from .consistency import plan as consistency_plan, slope as state_slope
from .graphs import GraphCache
from .imagen_pytorch3D import (GaussianDiffusionContinuousTimes, Unet, NullUnet, exists, default, cast_tuple, identity, maybe,
                               normalize_neg_one_to_one, unnormalize_zero_to_one, eval_decorator, to_channels_last,
                               to_channels_first, log_snr_to_alpha_sigma)
from .imagen_video import Unet3D

Hparams_fields = ['num_sample_steps', 'sigma_min', 'sigma_max', 'sigma_data', 'rho', 'P_mean', 'P_std', 'S_churn', 'S_tmin',
                  'S_tmax', 'S_noise']
Hparams = namedtuple('Hparams', Hparams_fields)


def calc_all_frame_dims(downsample_factors, frames):
    if not exists(frames):
        return (tuple(),) * len(downsample_factors)
    out = []
    for divisor in downsample_factors:
        assert frames % divisor == 0
        out.append((frames // divisor,))
    return out


class EDMWindowDenoiser:
    """The per-window half of ``ElucidatedImagen.one_unet_sample`` (the stochastic Heun sampler), callable one U-Net evaluation at a time
    (``ElucidatedImagen.window_denoiser`` makes it) -- the EDM counterpart of ``imagen_pytorch3D.WindowDenoiser``, with the attributes
    ``VolumeInference(joint=True)`` checks and ``heun = True``, which sends it down the Heun branch of the joint chain.

    * ``num_steps``; ``sched``: host [T,3] of (sigma, sigma_next, gamma) per step; ``sigma0``: the first sigma;
    * ``coefs``: host fp32 [T,7], per step ``(kc, 1 + r, -r, 1 + r/2, -r/2, r2, -r2)`` with sigma_hat = sigma + gamma sigma,
      kc = S_noise sqrt(max(sigma_hat^2 - sigma^2, 0)) (the churn, images_hat = images + kc eps), r = (sigma_next - sigma_hat) / sigma_hat
      (the predictor, images_next = (1 + r) images_hat - r out) and r2 = (sigma_next - sigma_hat) / (2 sigma_next) (the corrector,
      ((1 + r/2) images_hat - r/2 out + r2 images_next) - r2 out2; both entries 0 on the step with sigma_next == 0, which has none) --
      every entry the Python float ``one_unet_sample`` hands to its step kernel, rounded to fp32 once;
    * ``draw_base``: 1 for a low-res conditioned U-Net (draw 0 of a noise source is the low-res augmentation noise), else 0; the initial
      image is draw ``draw_base`` and the ``eps`` of step i is draw ``draw_base + 1 + i`` -- the call order of ``sample(noise=callable)``;
    * ``clamp = (-inf, inf, 1)``: ``x0`` already returns the clamped or thresholded prediction;
    * ``x0(img, lowres, i, self_cond=None, stage=0, lowres_noise=None)`` -> fp32 [B,C,P,P,P]: ``preconditioned_network_forward`` at
      sigma_hat of step i (``stage`` 0) or at its sigma_next (``stage`` 1) on the low-res windows noised with ``lowres_noise`` at
      ``lowres_sample_noise_level`` -- the tensor ``one_unet_sample`` calls ``out`` / ``out2``, hipGraph replay included;
    * ``finish(x)``: clamp(-1, 1) and ``unnormalize_img`` on a tensor of any shape; ``finish(x, known, mask)`` pastes the known values
      (state space) under the 0/1 mask between the two, and ``normalize(x)`` = ``imagen.normalize_img`` takes a known volume there -- what
      ``VolumeInference(joint=True, inpaint=...)`` needs;
    * ``self_cond``: whether the U-Net takes the last x0 estimate."""
    heun = True

    def _configure(self, imagen, unet_number, cond_scale, clamp, unet_context):
        """What every EDM window denoiser holds, whatever its sampler."""
        self.imagen, self.index, self._context = imagen, unet_number - 1, unet_context
        self.hp = imagen.hparams[self.index]
        self.cond_scale = cast_tuple(cond_scale, len(imagen.unets))[self.index]
        self.clamp_x0 = bool(clamp)
        self.dynamic_threshold = bool(imagen.dynamic_thresholding[self.index])
        unet = imagen.unets[self.index]
        self.self_cond = bool(getattr(unet, 'self_cond', False))
        self.lowres_cond = bool(getattr(unet, 'lowres_cond', False))
        self.draw_base = 1 if self.lowres_cond else 0
        self.clamp = (-float('inf'), float('inf'), 1)

    def __init__(self, imagen, unet_number, cond_scale, clamp, sigma_min, sigma_max, unet_context):
        self._configure(imagen, unet_number, cond_scale, clamp, unet_context)
        self._steps, self._hats, rows, self.sigma0 = imagen._heun_tables(self.index, sigma_min, sigma_max)   # one_unet_sample's own
        self.sched = torch.tensor(self._steps, dtype=torch.float64)                       # [T, 3] on the host: the fp32 values, widened
        self.num_steps = len(self._steps)
        self.coefs = torch.tensor(rows, dtype=torch.float64).to(torch.float32)            # [T, 7] on the host, each rounded once

    def sigma_of(self, i, stage):
        """The sigma the U-Net is evaluated at: sigma_hat of step i (stage 0) or its sigma_next (stage 1)."""
        return float(self._steps[i][1] if stage else self._hats[i])

    @torch.no_grad()
    def x0(self, img, lowres, i, self_cond=None, stage=0, lowres_noise=None):
        if not 0 <= i < self.num_steps:
            raise ValueError(f"EDMWindowDenoiser.x0: step {i} of {self.num_steps}")
        if stage not in (0, 1) or (stage == 1 and self._steps[i][1] == 0):
            raise ValueError(f"EDMWindowDenoiser.x0: stage {stage!r} of step {i} (0 = at sigma_hat, 1 = at sigma_next, when that is not 0)")
        return self._denoise(img, lowres, self.sigma_of(i, stage), self_cond, lowres_noise)

    def _denoise(self, img, lowres, sigma, self_cond, lowres_noise):
        """``preconditioned_network_forward`` of the windows ``img`` at ``sigma``, as ``sample`` sets it up for this U-Net."""
        elu = self.imagen
        if self.lowres_cond and (lowres is None or lowres_noise is None):
            raise ValueError("EDMWindowDenoiser.x0: a low-res conditioned U-Net needs the low-res windows and their augmentation noise")
        dev, B = img.device, img.shape[0]
        was_training = elu.training
        elu.eval()
        try:
            with self._context():
                elu.reset_unets_all_one_device(device=dev)                    # as ``sample`` does before it picks the U-Net
                unet = elu.unets[self.index]
                lowres_cond_img = lowres_noise_times = None
                if self.lowres_cond:
                    lowres_cond_img, lowres_noise_times = elu._lowres_conditioning(
                        lowres, elu.lowres_sample_noise_level, elu.image_sizes[self.index], img.shape[2], B, dev, lambda x: lowres_noise)
                sc = dict(self_cond=self_cond) if self.self_cond else {}
                return elu.preconditioned_network_forward(
                    unet.forward_with_cond_scale, img.float().contiguous(), sigma, sigma_data=self.hp.sigma_data,
                    clamp=self.clamp_x0, dynamic_threshold=self.dynamic_threshold, cond_scale=self.cond_scale,
                    **elu._unet_kwargs(unet, lowres_cond_img, lowres_noise_times), **sc)
        finally:
            elu.train(was_training)

    def normalize(self, x):
        """A known volume (in the units ``finish`` returns) in state space: ``imagen.normalize_img``, what ``one_unet_sample`` does to
        ``inpaint_images`` (:447)."""
        return self.imagen.normalize_img(x)

    state_space = normalize                                # the name every window denoiser has it under (``consistency=`` reads it)

    @torch.no_grad()
    def finish(self, x, known=None, mask=None):
        """``known`` (state space) / ``mask`` (0/1 fp32), both of x's shape: the chain inpainted, and the known values go under the mask
        between the clamp and ``unnormalize_img`` (:527-532): ``_finish_chain`` on the flat view, a batch of one."""
        flat = lambda t: t.contiguous().view(1, -1)
        return self.imagen._finish_chain(flat(x), *((flat(known), flat(mask)) if known is not None else ())).view(x.shape)


class EDMMultistepWindowDenoiser(EDMWindowDenoiser):
    """The per-window half of ``one_unet_sample(sampler='dpmpp2m')`` (``window_denoiser(sampler='dpmpp2m', sample_steps=K, eta=...)``):
    ONE U-Net evaluation per step.  ``multistep = True`` and ``heun = False``; ``sigma0`` tells ``VolumeInference`` that the chain lives in
    sigma space (the state starts as sigma0 n and a step may add noise).

    * ``num_steps``; ``sigmas``: host float64 [T + 1], the fp32 schedule widened; ``sigma0``;
    * ``coefs``: host fp32 [T,4], rows (kx, k0, kp, kn) of ``ElucidatedImagen.dpmpp2m_coefficients``;
    * ``draw_base``: as the Heun denoiser numbers it -- the initial image is draw ``draw_base``, the normal of step i draw
      ``draw_base + 1 + i`` (taken only where kn != 0: every step but the last with ``eta > 0``, none with ``eta == 0``);
    * ``x0(img, lowres, i, self_cond=None, lowres_noise=None)``: ``preconditioned_network_forward`` at sigma_i itself;
    * ``clamp``, ``finish``, ``self_cond``: the Heun denoiser's."""
    heun = False
    multistep = True

    def __init__(self, imagen, unet_number, cond_scale, clamp, sigma_min, sigma_max, unet_context, sample_steps, eta):
        self._configure(imagen, unet_number, cond_scale, clamp, unet_context)
        self.eta = float(eta)
        sigmas, self.coefs = imagen._dpmpp2m_tables(self.index, sample_steps, eta, sigma_min, sigma_max)
        self.sigmas = sigmas.double()
        self._sigmas = sigmas.tolist()
        self.sigma0 = self._sigmas[0]
        self.num_steps = len(self._sigmas) - 1

    def sigma_of(self, i, stage=0):
        return float(self._sigmas[i])

    @torch.no_grad()
    def x0(self, img, lowres, i, self_cond=None, lowres_noise=None):
        if not 0 <= i < self.num_steps:
            raise ValueError(f"EDMMultistepWindowDenoiser.x0: step {i} of {self.num_steps}")
        return self._denoise(img, lowres, self.sigma_of(i), self_cond, lowres_noise)


class ElucidatedImagen(nn.Module):
    def __init__(
        self, unets, *, image_sizes, text_encoder_name=None, text_embed_dim=None, channels=3, cond_drop_prob=0.1,
        random_crop_sizes=None, temporal_downsample_factor=1, lowres_sample_noise_level=0.2,
        per_sample_random_aug_noise_level=False, condition_on_text=True, auto_normalize_img=True, dynamic_thresholding=True,
        dynamic_thresholding_percentile=0.95, only_train_unet_number=None, lowres_noise_schedule='linear',
        num_sample_steps=32, sigma_min=0.002, sigma_max=80, sigma_data=0.5, rho=7, P_mean=-1.2, P_std=1.2, S_churn=80,
        S_tmin=0.05, S_tmax=50, S_noise=1.003,
    ):
        super().__init__()
        if condition_on_text:
            raise NotImplementedError('text conditioning (T5) is not part of the IQT hot path: pass condition_on_text=False')
        self.only_train_unet_number = only_train_unet_number
        self.condition_on_text = False
        self.unconditional = True
        self.channels = channels
        unets = cast_tuple(unets)
        num_unets = len(unets)
        self.random_crop_sizes = cast_tuple(random_crop_sizes, num_unets)
        assert all(r is None for r in self.random_crop_sizes), 'random crops (kornia) are outside the IQT path'
        self.lowres_noise_schedule = GaussianDiffusionContinuousTimes(noise_schedule=lowres_noise_schedule)
        self.text_embed_dim = None

        self.unets = nn.ModuleList([])
        self.unet_being_trained_index = -1
        for ind, one_unet in enumerate(unets):
            assert isinstance(one_unet, (Unet, Unet3D, NullUnet))
            one_unet = one_unet.cast_model_parameters(lowres_cond=not ind == 0, cond_on_text=False, text_embed_dim=None,
                                                      channels=self.channels, channels_out=self.channels)
            self.unets.append(one_unet)
        self.is_video = any(isinstance(u, Unet3D) for u in self.unets) or any(isinstance(u, Unet) for u in self.unets)
        self.image_sizes = cast_tuple(image_sizes)
        assert num_unets == len(self.image_sizes), \
            f'you did not supply the correct number of u-nets ({len(self.unets)}) for resolutions {self.image_sizes}'
        self.sample_channels = cast_tuple(self.channels, num_unets)
        lowres_conditions = tuple(map(lambda t: t.lowres_cond, self.unets))
        assert lowres_conditions == (False, *((True,) * (num_unets - 1))), \
            'the first unet must be unconditioned (by low resolution image), and the rest of the unets must have `lowres_cond` set to True'
        self.lowres_sample_noise_level = lowres_sample_noise_level
        self.per_sample_random_aug_noise_level = per_sample_random_aug_noise_level
        self.cond_drop_prob = cond_drop_prob
        self.can_classifier_guidance = cond_drop_prob > 0.
        self.normalize_img = normalize_neg_one_to_one if auto_normalize_img else identity
        self.unnormalize_img = unnormalize_zero_to_one if auto_normalize_img else identity
        self.input_image_range = (0. if auto_normalize_img else -1., 1.)
        self.dynamic_thresholding = cast_tuple(dynamic_thresholding, num_unets)
        self.dynamic_thresholding_percentile = dynamic_thresholding_percentile
        temporal_downsample_factor = cast_tuple(temporal_downsample_factor, num_unets)
        self.temporal_downsample_factor = temporal_downsample_factor
        assert temporal_downsample_factor[-1] == 1, 'downsample factor of last stage must be 1'
        assert all(l >= r for l, r in zip((1, *temporal_downsample_factor[:-1]), temporal_downsample_factor[1:])), \
            'temporal downssample factor must be in order of descending'
        hparams = [num_sample_steps, sigma_min, sigma_max, sigma_data, rho, P_mean, P_std, S_churn, S_tmin, S_tmax, S_noise]
        hparams = [cast_tuple(hp, num_unets) for hp in hparams]
        self.hparams = [Hparams(*unet_hp) for unet_hp in zip(*hparams)]
        self._graphs = GraphCache()           # hipGraph replay of the U-Net evaluations of a sampling loop (graphs.py)
        self.register_buffer('_temp', torch.tensor([0.]), persistent=False)
        self.to(next(self.unets.parameters()).device)

    @property
    def device(self):
        return self._temp.device

    def get_unet(self, unet_number):
        assert 0 < unet_number <= len(self.unets)
        index = unet_number - 1
        if isinstance(self.unets, nn.ModuleList):
            unets_list = [unet for unet in self.unets]
            delattr(self, 'unets')
            self.unets = unets_list
        if index != self.unet_being_trained_index:
            for unet_index, unet in enumerate(self.unets):
                unet.to(self.device if unet_index == index else 'cpu')
        self.unet_being_trained_index = index
        return self.unets[index]

    def reset_unets_all_one_device(self, device=None):
        device = default(device, self.device)
        self.unets = nn.ModuleList([*self.unets])
        self.unets.to(device)
        self.unet_being_trained_index = -1

    def state_dict(self, *args, **kwargs):
        self.reset_unets_all_one_device()
        return super().state_dict(*args, **kwargs)

    def load_state_dict(self, *args, **kwargs):
        self.reset_unets_all_one_device()
        return super().load_state_dict(*args, **kwargs)

    # ---- EDM scalars (host floats / [B] tensors) -----------------------------------------------------
    def c_skip(self, sigma_data, sigma):
        return (sigma_data ** 2) / (sigma ** 2 + sigma_data ** 2)

    def c_out(self, sigma_data, sigma):
        return sigma * sigma_data * (sigma_data ** 2 + sigma ** 2) ** -0.5

    def c_in(self, sigma_data, sigma):
        return 1 * (sigma ** 2 + sigma_data ** 2) ** -0.5

    def c_noise(self, sigma):
        return torch.log(sigma.clamp(min=1e-20)) * 0.25

    def loss_weight(self, sigma_data, sigma):
        return (sigma ** 2 + sigma_data ** 2) * (sigma * sigma_data) ** -2

    def noise_distribution(self, P_mean, P_std, batch_size):
        return (P_mean + P_std * torch.randn((batch_size,))).exp()          # host: one scalar per sample

    def sample_schedule(self, num_sample_steps, rho, sigma_min, sigma_max):
        N, inv_rho = num_sample_steps, 1 / rho
        steps = torch.arange(num_sample_steps, dtype=torch.float32)
        sigmas = (sigma_max ** inv_rho + steps / (N - 1) * (sigma_min ** inv_rho - sigma_max ** inv_rho)) ** rho
        return torch.nn.functional.pad(sigmas, (0, 1), value=0.)

    def dpmpp2m_coefficients(self, sigmas, eta=0., S_noise=1.):
        """DPM-Solver++ 2M (Lu et al. 2022) in sigma space on the chain ``sigmas`` [T + 1] (``sample_schedule``), folded into
        x_next = kx x + k0 D_i + kp D_{i-1} + kn n: host fp32 [T,4], rows (kx, k0, kp, kn).  With h = log(sigma / sigma'),
        c = -expm1(-h - eta h) and r = h_{i-1} / h_i:  kx = (sigma' / sigma) exp(-eta h), k0 = c (1 + 1/(2r)), kp = -c / (2r),
        kn = S_noise sigma' sqrt(-expm1(-2 eta h)).  ``eta == 0``: the ODE solver, kn == 0 on every row; ``eta > 0``: the midpoint
        2M-SDE.  k0 + kp = c on every row.  Row 0 has no history, (kx, c, 0, kn) -- at eta 0 the Euler predictor (1 + r, -r) of the
        Heun sampler -- and the row with sigma' == 0 (h infinite, r 0) is (0, 1, 0, 0), first order by definition.  The algebra runs in
        float64 on the widened fp32 ``sigmas``; each entry is rounded to fp32 once (the rule of ``dpmpp2m_coefficients`` in
        imagen_pytorch3D.py)."""
        s = torch.as_tensor(sigmas).detach().cpu().double().tolist()
        eta, S_noise = float(eta), float(S_noise)
        rows, h_prev = [], None
        for i, (sigma, sigma_next) in enumerate(zip(s[:-1], s[1:])):
            if sigma_next == 0:
                rows.append([0., 1., 0., 0.])
                h_prev = None
                continue
            h = log(sigma / sigma_next)
            c = -expm1(-h - eta * h)
            k0, kp = c, 0.
            if i > 0 and h_prev is not None:
                r = h_prev / h
                k0, kp = c * (1. + 1. / (2. * r)), -c / (2. * r)
            rows.append([sigma_next / sigma * exp(-eta * h), k0, kp, S_noise * sigma_next * sqrt(-expm1(-2. * eta * h))])
            h_prev = h
        return torch.tensor(rows, dtype=torch.float64).to(torch.float32)

    SAMPLERS = ('heun', 'dpmpp2m')

    @classmethod
    def _check_sampler_args(cls, sampler, sample_steps, skip_steps, eta):
        """The argument rules of ``sampler`` / ``sample_steps`` / ``eta`` for one U-Net (``ValueError``; nothing touches the device)."""
        if sampler not in cls.SAMPLERS:
            raise ValueError(f"sampler must be 'heun' or 'dpmpp2m', got {sampler!r}")
        if isinstance(eta, bool) or not isinstance(eta, (int, float)) or not 0. <= eta <= 1.:
            raise ValueError(f"eta must be a number in [0, 1], got {eta!r}")
        if sampler == 'heun':
            if eta != 0 or exists(sample_steps):
                raise ValueError("sampler='heun' takes neither eta nor sample_steps: its stochasticity is S_churn and its length "
                                 "num_sample_steps")
            return
        if exists(sample_steps) and (isinstance(sample_steps, bool) or int(sample_steps) != sample_steps or sample_steps < 2):
            raise ValueError(f"sample_steps must be an integer >= 2, got {sample_steps!r}")
        if exists(skip_steps):
            raise ValueError("sampler='dpmpp2m' takes no skip_steps: a history term over a cut chain is meaningless -- shorten the chain "
                             "with sample_steps")

    @staticmethod
    def _check_inpaint_args(sampler, inpaint_images, inpaint_masks, inpaint_resample_times):
        """The argument rules of inpainting for one U-Net (``ValueError`` naming "inpaint"; nothing touches the device).  Returns whether
        the call inpaints."""
        if exists(inpaint_images) != exists(inpaint_masks):
            raise ValueError("inpaint_images and inpaint_masks must be both passed in to do inpainting")
        if not exists(inpaint_images):
            return False
        if sampler != 'heun':
            raise ValueError(f"sampler={sampler!r} does not inpaint: the re-noising loop (inpaint_resample_times) belongs to the stochastic "
                             f"Heun sampler -- use sampler='heun'")
        R = inpaint_resample_times
        if isinstance(R, bool) or not isinstance(R, int) or R < 1:
            raise ValueError(f"inpaint_resample_times must be a positive integer, got {R!r}")
        return True

    @staticmethod
    def inpaint_draws(steps, resample_times):
        """How many normals the inpainting loop takes over ``steps`` sampler steps, after the initial image: per (step, r) the ``eps`` and,
        unless r == 0 or it is the last step, the re-noise normal."""
        return steps * resample_times + (steps - 1) * (resample_times - 1)

    def _dpmpp2m_tables(self, index, sample_steps, eta, sigma_min, sigma_max):
        """(sigmas [T + 1] fp32, coefs [T,4] fp32) of ``sampler='dpmpp2m'`` for U-Net ``index``, both on the host."""
        hp = self.hparams[index]
        sigmas = self.sample_schedule(int(default(sample_steps, hp.num_sample_steps)), hp.rho, default(sigma_min, hp.sigma_min),
                                      default(sigma_max, hp.sigma_max))
        return sigmas, self.dpmpp2m_coefficients(sigmas, eta, hp.S_noise)

    def _heun_tables(self, index, sigma_min, sigma_max, skip_steps=None):
        """The host table of the stochastic Heun sampler for U-Net ``index``, the one ``one_unet_sample`` and ``EDMWindowDenoiser`` both
        read, so the one-call and the step-at-a-time sampler cannot drift: ``(sched, hats, coefs, sigma0)`` -- per step after
        ``skip_steps`` the row (sigma, sigma_next, gamma), sigma_hat = sigma + gamma sigma and the seven scalars
        ``(kc, 1 + r, -r, 1 + r/2, -r/2, r2, -r2)`` that ``EDMWindowDenoiser`` documents, and the first sigma of the whole schedule.
        Python floats throughout: the schedule's fp32 values widened, the scalars in double (a consumer rounds them to fp32 once)."""
        hp = self.hparams[index]
        sigmas = self.sample_schedule(hp.num_sample_steps, hp.rho, default(sigma_min, hp.sigma_min), default(sigma_max, hp.sigma_max))
        gammas = torch.where((sigmas >= hp.S_tmin) & (sigmas <= hp.S_tmax), min(hp.S_churn / hp.num_sample_steps, sqrt(2) - 1), 0.)
        sched = list(zip(sigmas[:-1].tolist(), sigmas[1:].tolist(), gammas[:-1].tolist()))[default(skip_steps, 0):]
        hats, coefs = [], []
        for sigma, sigma_next, gamma in sched:
            sigma_hat = sigma + gamma * sigma
            r = (sigma_next - sigma_hat) / sigma_hat
            r2 = 0.5 * (sigma_next - sigma_hat) / sigma_next if sigma_next != 0 else 0.       # no corrector on the step to sigma 0
            hats.append(sigma_hat)
            coefs.append((hp.S_noise * sqrt(max(sigma_hat ** 2 - sigma ** 2, 0.)), 1. + r, -r, 1. + 0.5 * r, -0.5 * r, r2, -r2))
        return sched, hats, coefs, sigmas[0].item()

    def threshold_x_start(self, x_start, dynamic_threshold=True):
        """elucidated_imagen.py:298-311: clamp(-1, 1), or per-sample s = max(quantile(|x0|, p), 1) then clamp(-s, s) / s."""
        x_start = x_start.contiguous()
        if dynamic_threshold:
            s = ops.abs_quantile(x_start, self.dynamic_thresholding_percentile)
            s.clamp_(min=1.)
            return ops.dynamic_threshold(x_start, s)
        one = torch.ones(x_start.shape[0], device=x_start.device)
        return ops.axpby3(x_start, None, None, one, None, None, -1., 1., 2)

    def _unet_kwargs(self, unet, lowres_cond_img, lowres_noise_times):
        inner = unet.module if hasattr(unet, 'module') else unet
        kw = dict(lowres_cond_img=lowres_cond_img)
        if isinstance(inner, Unet3D):
            kw['lowres_noise_times'] = lowres_noise_times
        return kw

    def preconditioned_network_forward(self, unet_forward, noised_images, sigma, *, sigma_data, clamp=False,
                                       dynamic_threshold=True, _replay=True, **kwargs):
        """:329-358 with per-batch sigma as a host float or a CPU/GPU [B] tensor.  ``_replay=False``: never through the hipGraph cache
        (the no-grad self-conditioning pre-pass of a TRAINING step: its weights change every optimiser step, a capture would be retired at once)."""
        B = noised_images.shape[0]
        dev = noised_images.device
        sig = torch.full((B,), float(sigma)) if isinstance(sigma, float) else sigma.detach().float().cpu()
        cin, cskip, cout = (f(sigma_data, sig).to(dev) for f in (self.c_in, self.c_skip, self.c_out))
        x_in = ops.axpby3(noised_images.contiguous(), None, None, cin, None, None)
        owner = getattr(unet_forward, '__self__', None)
        if _replay and owner is not None and not torch.is_grad_enabled():
            # sampling: after two eager calls the U-Net evaluation replays as a hipGraph (the small stages of a cascade are launch-bound)
            net_out = self._graphs.run(owner, unet_forward, (x_in, self.c_noise(sig).to(dev)), kwargs)
        else:
            net_out = unet_forward(x_in, self.c_noise(sig).to(dev), **kwargs)
        if clamp and dynamic_threshold:
            out = ops.axpby3(noised_images.contiguous(), net_out.contiguous(), None, cskip, cout, None, 0., 0., 0)
            return self.threshold_x_start(out, True)
        return ops.axpby3(noised_images.contiguous(), net_out.contiguous(), None, cskip, cout, None, -1., 1., 2 if clamp else 0)

    @torch.no_grad()
    def one_unet_sample(self, unet, shape, *, unet_number, clamp=True, dynamic_threshold=True, cond_scale=1., use_tqdm=True,
                        inpaint_images=None, inpaint_masks=None, inpaint_resample_times=5, init_images=None,
                        skip_steps=None, sigma_min=None, sigma_max=None, noise=None, sampler='heun', sample_steps=None, eta=0.,
                        consistency=None, consistency_weight=1., consistency_profile=None, consistency_noise=None,
                        consistency_operator=None, consistency_row_noise=None, consistency_slab=None, consistency_band=None,
                        consistency_heun=None, **kwargs):
        """Stochastic Heun sampler (:382-532).  ``noise``: optional injected list [init, step_0, ...], or a callable
        ``noise(shape) -> fp32 device tensor`` whose successive calls are those draws (one ``eps`` per step, also when gamma is 0).

        ``sampler='dpmpp2m'``: DPM-Solver++ 2M in sigma space (``dpmpp2m_coefficients``) on ``sample_schedule(sample_steps or
        num_sample_steps, ...)`` -- ONE U-Net evaluation per step, at sigma_i itself, and ONE ``ops.multistep_sde_step`` launch whose
        history operand is the clamped (or thresholded) prediction of the previous step; self-conditioning reads that same tensor.
        ``eta == 0`` is the ODE solver (the draws are the initial image alone), ``0 < eta <= 1`` the midpoint 2M-SDE (one more draw per
        step whose kn != 0: every step but the last).  S_churn / S_tmin / S_tmax play no part; S_noise scales kn.  No ``skip_steps``.

        ``inpaint_images`` [B,C,D,H,W] (in the units ``sample`` returns) with ``inpaint_masks`` [B,D,H,W] (True: known): the RePaint loop
        of the Heun sampler below, ``inpaint_resample_times`` passes per step.  The draws are then the initial image and, per
        (step, r), the ``eps`` and -- unless r == 0 or it is the last step -- the re-noise normal (``inpaint_draws``).  Only with
        ``sampler='heun'``; one of the two without the other, another sampler or a count that is not a positive integer: ``ValueError``
        before anything touches the device.

        ``consistency=(meas_up, cell)`` with ``consistency_weight`` (``sampler='dpmpp2m'``, or ``'heun'`` with ``consistency_heun``),
        ``consistency_profile``, ``consistency_noise``, ``consistency_operator``, ``consistency_row_noise``, ``consistency_slab``,
        ``consistency_band``, ``consistency_heun``: data-consistent sampling
        (DDNM / DDNM+); the keywords, their rules and the launch a step takes are stated once, in ``consistency.py``.  ``meas_up``
        [B,C,P,P,P], the measurement replicated onto the high-res grid (``ops.cell_replicate``; with an operator t = A+ y,
        ``ops.tile_backproject``), and the noise deviations arrive in state space here (``sample`` takes them in the units it
        returns, like ``inpaint_images``).  Every step's clamped or thresholded prediction goes through the mode's projection before
        ``ops.multistep_sde_step``; the history operand and self-conditioning read the projected tensor.  A noise-aware step runs
        its one launch on the step's draw and hands the step the reduced normals (a new tensor); the step with kn = 0 (the last)
        skips the projection.  The draws are unchanged.  The Heun sampler has two predictions per step and is refused unless
        ``consistency_heun`` says which to project: ``'both'`` -- ``out`` (at sigma_hat) and ``out2`` (at sigma_next) each go through
        the mode's projection launch right after their evaluation, 2 T - 1 launches per chain -- or ``'predictor'`` -- ``out`` alone,
        T launches.  The predictor's ``axpby3``, the corrector's two, ``x_start`` and self-conditioning read the projected tensors;
        the last step (to sigma 0, no corrector, row (0, 1)) ends the chain in its projected prediction.  Every rung is the constant
        one: no DDNM+ weights with Heun."""
        self._check_sampler_args(sampler, sample_steps, skip_steps, eta)
        has_inpainting = self._check_inpaint_args(sampler, inpaint_images, inpaint_masks, inpaint_resample_times)
        plan = consistency_plan('one_unet_sample', ops, consistency, consistency_weight, consistency_profile, consistency_noise,
                                consistency_operator, consistency_row_noise, consistency_slab, consistency_band, shape=shape,
                                stochastic=eta != 0,
                                has_inpainting=has_inpainting, init_images=init_images, skip_steps=skip_steps, sampler=sampler,
                                heun=consistency_heun)
        if sampler == 'dpmpp2m':
            return self._dpmpp2m_sample(unet, shape, unet_number=unet_number, clamp=clamp, dynamic_threshold=dynamic_threshold,
                                        cond_scale=cond_scale, init_images=init_images, sigma_min=sigma_min, sigma_max=sigma_max,
                                        noise=noise, sample_steps=sample_steps, eta=eta, consistency=plan, **kwargs)
        # Inpainting (:441-449, 473-530; RePaint, Lugmayr et al. 2022) is this loop with ``inpaint_resample_times`` passes per step,
        # r = R - 1 .. 0, where plain sampling has one: a pass draws ``eps``, pastes the known image under the mask and churns, runs the
        # two Heun evaluations as ever and -- unless r == 0 or it is the last step -- draws once more and re-noises,
        # images += (sigma - sigma_next) n.  The re-noise that ends a pass, the paste and the churn that begins the next are ONE
        # ``ops.edm_inpaint_churn`` launch, in place; without known values the churn is ``ops.axpby3`` into a new tensor, and there
        # are no masks, no re-noise draw and no paste at the end.  The self-conditioning estimate carries across passes.
        known = mask_f = mask_b = None
        if has_inpainting:
            known, mask_f, mask_b = self._inpaint_operands(inpaint_images, inpaint_masks, shape)
        sched, hats, coefs, sigma0 = self._heun_tables(unet_number - 1, sigma_min, sigma_max, skip_steps)
        draw, images, fwd, sc = self._start_chain(unet, shape, unet_number, sigma0, noise, init_images, clamp=clamp,
                                                  dynamic_threshold=dynamic_threshold, cond_scale=cond_scale, **kwargs)
        vec = lambda v: torch.full((shape[0],), float(v), device=self.device)
        chain = plan.prepare(sched, self.device) if exists(plan) else None                        # once per chain
        x_start = renoise = kr = None
        for ind, ((sigma, sigma_next, _), sigma_hat, (kc, a, b, a_half, b_half, r2, neg_r2)) in enumerate(zip(sched, hats, coefs)):
            kc = vec(kc)
            for resample in reversed(range(int(inpaint_resample_times) if has_inpainting else 1)):
                eps = draw()
                if has_inpainting:   # the re-noise of the pass before (if it had one), the paste, the churn: one pass over the state
                    images_hat = ops.edm_inpaint_churn(images, renoise, known, mask_b, eps, kr, kc, out=images)
                    renoise = kr = None
                else:
                    images_hat = ops.axpby3(images, eps, None, vec(1.), kc, None)
                out = fwd(images_hat, float(sigma_hat), **sc(x_start))
                if exists(chain):                                                 # ``out`` arrives clamped or thresholded
                    out, _, _ = chain.project(ind, out, lambda: None)
                # x_next = x_hat + (s_next - s_hat) * (x_hat - D)/s_hat
                images_next = ops.axpby3(images_hat, out, None, vec(a), vec(b), None)
                x_start = out
                if sigma_next != 0:                                               # 2nd-order correction (:502-516)
                    out2 = fwd(images_next, float(sigma_next), **sc(out))
                    if exists(chain) and chain.heun == 'both':                    # 'predictor': the corrector's stays the network's
                        out2, _, _ = chain.project(ind, out2, lambda: None)
                    tmp = ops.axpby3(images_hat, out, images_next, vec(a_half), vec(b_half), vec(r2))
                    images_next = ops.axpby3(tmp, out2, None, vec(1.), vec(neg_r2), None)
                    x_start = out2
                images = images_next
                if has_inpainting and not (resample == 0 or ind == len(sched) - 1):   # renoise in repaint and then resample (:520-523)
                    renoise, kr = draw(), vec(sigma - sigma_next)
        return self._finish_chain(images, known, mask_f)

    def _start_chain(self, unet, shape, unet_number, sigma0, noise, init_images, **kwargs):
        """The prologue of a per-window chain, whatever its sampler: ``(draw, images, fwd, sc)`` -- ``draw()``, the next normal of
        ``noise`` (a list [init, step_0, ...], a callable ``noise(shape)`` or None for ``torch.randn``); the initial image
        ``sigma0 * draw()`` plus ``init_images``; ``fwd(images, sigma, **sc(x0))``, ``preconditioned_network_forward`` of ``unet`` under
        ``kwargs``, with ``sc(x0)`` the self-conditioning keyword (:483, 505, 524: the last x0 estimate) if the U-Net takes one."""
        dev = self.device
        if callable(noise):
            draw = lambda: noise(shape).to(dev).float().contiguous()
        else:
            noise = list(noise) if exists(noise) else None
            draw = (lambda: noise.pop(0).to(dev).float().contiguous()) if exists(noise) else (lambda: torch.randn(shape, device=dev))
        images = ops.axpby3(draw(), None, None, torch.full((shape[0],), float(sigma0), device=dev), None, None)
        if exists(init_images):
            images = ops.add(images, init_images.to(dev).float())
        fwd = partial(self.preconditioned_network_forward, unet.forward_with_cond_scale, sigma_data=self.hparams[unet_number - 1].sigma_data,
                      **kwargs)
        sc = (lambda x0: dict(self_cond=x0)) if getattr(unet, 'self_cond', False) else (lambda x0: {})
        return draw, images, fwd, sc

    def _finish_chain(self, images, known=None, mask=None):
        """The end of a chain: clamp(-1, 1) (:527), the known values (state space) under the 0/1 fp32 ``mask`` if the chain inpainted
        (:529-530), ``unnormalize_img``."""
        images = ops.axpby3(images, None, None, torch.ones(images.shape[0], device=images.device), None, None, -1., 1., 2)
        if exists(known):
            images = ops.mask_blend(images, known, mask)
        return self.unnormalize_img(images)

    def _dpmpp2m_sample(self, unet, shape, *, unet_number, clamp, dynamic_threshold, cond_scale, init_images, sigma_min, sigma_max, noise,
                        sample_steps, eta, consistency=None, **kwargs):
        """``one_unet_sample(sampler='dpmpp2m')``; the arguments are checked there (``consistency``: None or the ``consistency.Plan``
        of the call, its measurement and deviations in state space)."""
        sigmas, coefs = self._dpmpp2m_tables(unet_number - 1, sample_steps, eta, sigma_min, sigma_max)
        chain = consistency.prepare(coefs.double(), self.device) if exists(consistency) else None      # once per chain
        sigmas = sigmas.tolist()
        dev, B = self.device, shape[0]
        draw, images, fwd, sc = self._start_chain(unet, shape, unet_number, sigmas[0], noise, init_images, clamp=clamp,
                                                  dynamic_threshold=dynamic_threshold, cond_scale=cond_scale, **kwargs)
        stochastic = (coefs[:, 3] != 0).tolist()
        k = coefs[:, :, None].expand(-1, -1, B).contiguous().to(dev)              # [T,4,B]: one coefficient row per sample
        x_start = None
        for i in range(coefs.shape[0]):
            out = fwd(images, float(sigmas[i]), **sc(x_start))
            normals = lambda: draw() if stochastic[i] else None                 # the step's draw, where kn != 0
            # ``out`` arrives clamped or thresholded; a launch that shapes the normals takes the draw first
            out, eps, _ = chain.project(i, out, normals) if exists(chain) else (out, normals(), None)
            images = ops.multistep_sde_step(images, out, x_start, eps, k[i, 0], k[i, 1], k[i, 2], k[i, 3])
            x_start = out
        return self._finish_chain(images)

    def _inpaint_operands(self, inpaint_images, inpaint_masks, shape):
        """:446-449 on the device: the known images through ``normalize_img`` and the nearest resize to the U-Net's size, the masks
        [B,D,H,W] -> [B,1,D,H,W], resized as floats, then thresholded.  Returns (known fp32, mask as 0/1 fp32, mask as bytes), each of
        ``shape`` and contiguous (the mask is repeated over the channels)."""
        dev = self.device
        known = self._resize(self.normalize_img(inpaint_images.to(dev).float()), shape[-1], shape[2])
        masks = self._resize(inpaint_masks.to(dev)[:, None].float(), shape[-1], shape[2]).bool()
        if tuple(known.shape) != tuple(shape) or tuple(masks.shape) != (shape[0], 1, *shape[2:]):
            raise ValueError(f"inpaint_images {tuple(inpaint_images.shape)} / inpaint_masks {tuple(inpaint_masks.shape)} do not resize to the "
                             f"sampled shape {tuple(shape)} and its [B,D,H,W] mask")
        masks = masks.expand(shape)
        return known.contiguous(), masks.float().contiguous(), masks.to(torch.uint8).contiguous()

    def window_denoiser(self, unet_number=2, cond_scale=1., clamp=True, sigma_min=None, sigma_max=None, inpaint_images=None,
                        inpaint_masks=None, init_images=None, skip_steps=None, _unet_context=nullcontext, sampler='heun',
                        sample_steps=None, eta=0.):
        """The per-window half of ``one_unet_sample`` as an object that is called one U-Net evaluation at a time -- what
        ``VolumeInference(..., joint=True)`` drives for the EDM family; see ``EDMWindowDenoiser`` and, for ``sampler='dpmpp2m'``
        (``sample_steps`` / ``eta`` as in ``one_unet_sample``), ``EDMMultistepWindowDenoiser``.  Inpainting, ``init_images`` and
        ``skip_steps`` belong to the one-call sampler and are refused here (``ValueError``, before anything touches the device)."""
        self._check_sampler_args(sampler, sample_steps, None, eta)
        if exists(inpaint_images) or exists(inpaint_masks):
            raise ValueError("window_denoiser does not inpaint: the joint chain has no per-window re-noising loop")
        if exists(init_images):
            raise ValueError("window_denoiser takes no init_images: the joint chain starts from the volume-anchored field")
        if exists(skip_steps):
            raise ValueError("window_denoiser takes no skip_steps: thin the chain with num_sample_steps")
        if isinstance(unet_number, bool) or int(unet_number) != unet_number or not 1 <= unet_number <= len(self.unets):
            raise ValueError(f"unet_number must be 1 .. {len(self.unets)}, got {unet_number!r}")
        if isinstance(self.unets[unet_number - 1], NullUnet):
            raise ValueError('one cannot sample from null / placeholder unets')
        if sampler == 'dpmpp2m':
            return EDMMultistepWindowDenoiser(self, int(unet_number), cond_scale, clamp, sigma_min, sigma_max, _unet_context, sample_steps,
                                              eta)
        return EDMWindowDenoiser(self, int(unet_number), cond_scale, clamp, sigma_min, sigma_max, _unet_context)

    def _resize(self, x, size, frames=None):
        """resize_video_to (imagen_video.py:137-158): nearest, no-op when the spatial size already matches."""
        if x.shape[-1] == size:
            return x
        f = default(frames, x.shape[2])
        return to_channels_first(ops.nearest_resize(to_channels_last(x.float().to(self.device)), (f, size, size)))

    def _noise_lowres(self, lowres, times_cpu, noise):
        log_snr = self.lowres_noise_schedule.log_snr(times_cpu)
        alpha, sigma = log_snr_to_alpha_sigma(log_snr)
        dev = lowres.device
        return ops.q_sample(lowres.contiguous(), noise.contiguous(), alpha.to(dev), sigma.to(dev))

    def _lowres_conditioning(self, lowres, noise_level, size, frames, batch, device, draw):
        """What a low-res conditioned U-Net is handed at sampling (:652-657, 680): ``(lowres_cond_img, lowres_noise_times)`` -- ``lowres``
        resized to ``size`` / ``frames``, through ``normalize_img`` and noised at ``noise_level`` with ``draw(image)``, the augmentation
        normals for the prepared image; and the RAW time, [batch] on ``device``."""
        t_cpu = torch.full((batch,), float(noise_level))
        lowres = self.normalize_img(self._resize(lowres.to(device), size, frames)).float().to(device)
        return self._noise_lowres(lowres, t_cpu, draw(lowres).to(device).float()), t_cpu.to(device)

    @torch.no_grad()
    @eval_decorator
    def sample(self, texts=None, text_masks=None, text_embeds=None, cond_images=None, inpaint_images=None, inpaint_masks=None,
               inpaint_resample_times=5, init_images=None, skip_steps=None, sigma_min=None, sigma_max=None, video_frames=None,
               batch_size=1, cond_scale=1., lowres_sample_noise_level=None, start_at_unet_number=1, start_image_or_video=None,
               stop_at_unet_number=None, return_all_unet_outputs=False, return_pil_images=False, use_tqdm=True, device=None,
               noise=None, sampler='heun', sample_steps=None, eta=0., consistency=None, consistency_weight=1.,
               consistency_profile=None, consistency_noise=None, consistency_operator=None, consistency_row_noise=None,
               consistency_slab=None, consistency_band=None, consistency_heun=None):
        """:536-702.  ``noise``: optional injected list [lowres_noise, init, step_0, ...] per sampled unet (tests), or -- when exactly
        one U-Net is sampled -- a callable ``noise(shape) -> fp32 device tensor`` whose successive calls are those draws in that order
        (``inference.AnchoredNoise.source``: call k is draw k of the volume-anchored field).

        ``sampler`` ('heun', the default, or 'dpmpp2m'), ``sample_steps`` and ``eta`` -- one value, or one per U-Net like ``skip_steps``
        -- are ``one_unet_sample``'s.  Under 'dpmpp2m' the draws of a U-Net are the low-res augmentation noise (if it is low-res
        conditioned), the initial image, then one per step whose kn != 0 (none with ``eta == 0``); the churn hyper-parameters (S_churn,
        S_tmin, S_tmax) play no part.  Refused with ``ValueError`` before anything touches the device: an unknown sampler, ``eta``
        outside [0, 1], ``eta`` or ``sample_steps`` with 'heun', ``sample_steps < 2``, ``skip_steps`` with 'dpmpp2m'.

        ``inpaint_images`` / ``inpaint_masks`` / ``inpaint_resample_times`` (:580-592): every sampled U-Net keeps the known voxels through
        the RePaint loop of ``one_unet_sample``; ``batch_size`` 1 broadcasts to the number of images.  A U-Net's draws are then the
        low-res noise (if any), the initial image and ``inpaint_draws(steps, R)`` loop normals, in the reference's call order.  One of
        images / masks alone, inpainting with 'dpmpp2m', or a count that is not a positive integer: ``ValueError`` naming "inpaint",
        before anything touches the device.

        ``consistency=(meas_up, cell)`` / ``consistency_weight`` and the seven keywords that ride on it (``consistency_profile``,
        ``consistency_noise``, ``consistency_operator``, ``consistency_row_noise``, ``consistency_slab``, ``consistency_band``,
        ``consistency_heun`` -- with ``sampler='heun'``: ``'both'`` or ``'predictor'``, the predictions of a Heun step to project):
        ``one_unet_sample``'s, for
        every sampled U-Net (so they must generate one size).  ``meas_up`` [B,C,P,P,P] (with an operator t = A+ y) is in the units
        this returns -- ``normalize_img`` takes it to state space, as it does ``inpaint_images`` -- and the noise deviations are in
        its units as passed here: they are multiplied by the slope of ``normalize_img``.  ``consistency.py`` states the keywords and
        their refusals: ``ValueError`` naming the keyword at fault and the one that rides on it, raised here for every sampled
        U-Net before anything touches the device."""
        assert texts is None and text_embeds is None and not return_pil_images
        samplers, steps_per_unet, etas = (cast_tuple(v, len(self.unets)) for v in (sampler, sample_steps, eta))
        for args in zip(samplers, steps_per_unet, cast_tuple(skip_steps, len(self.unets)), etas):
            self._check_sampler_args(*args)
        sampled_samplers = samplers[start_at_unet_number - 1:default(stop_at_unet_number, len(self.unets))]
        has_inpainting = any([self._check_inpaint_args(s, inpaint_images, inpaint_masks, inpaint_resample_times)
                              for s in sampled_samplers or samplers[-1:]])
        frames, plan = calc_all_frame_dims(self.temporal_downsample_factor, video_frames) if exists(consistency) else None, None
        for n in range(start_at_unet_number, default(stop_at_unet_number, len(self.unets)) + 1):      # every sampled U-Net's rules, up front
            plan = consistency_plan(
                'sample', ops, consistency, consistency_weight, consistency_profile, consistency_noise, consistency_operator,
                consistency_row_noise, consistency_slab, consistency_band, stochastic=etas[n - 1] != 0, has_inpainting=exists(inpaint_images),
                shape=exists(frames) and (batch_size, self.channels, *frames[n - 1], self.image_sizes[n - 1], self.image_sizes[n - 1]),
                init_images=cast_tuple(init_images, len(self.unets))[n - 1], skip_steps=cast_tuple(skip_steps, len(self.unets))[n - 1],
                sampler=samplers[n - 1], heun=consistency_heun)
        # what ``one_unet_sample`` takes: the measurement in state space, the deviations with it by the map's slope
        consistent = plan.keywords(self.normalize_img(plan.measurement), slope=state_slope(self.normalize_img)) if exists(plan) else {}
        if has_inpainting:
            if batch_size == 1:                                                    # broadcast along the inpainted images (:580-583)
                batch_size = inpaint_images.shape[0]
            if inpaint_images.shape[0] != batch_size:
                raise ValueError(f"the number of inpaint_images ({inpaint_images.shape[0]}) must equal batch_size ({batch_size})")
        if callable(noise):
            sampled = range(start_at_unet_number, default(stop_at_unet_number, len(self.unets)) + 1)
            if len(sampled) != 1:
                raise ValueError(f"sample: a callable noise source is made for one window size, so exactly one U-Net may be sampled with "
                                 f"it (start_at_unet_number == stop_at_unet_number or the last one); this call samples {len(sampled)}")
        device = default(device, self.device)
        self.reset_unets_all_one_device(device=device)
        lowres_sample_noise_level = default(lowres_sample_noise_level, self.lowres_sample_noise_level)
        num_unets = len(self.unets)
        cond_scale = cast_tuple(cond_scale, num_unets)
        assert exists(video_frames), 'video_frames (the depth of the 3-D patch) must be passed in on sample time'
        all_frame_dims = calc_all_frame_dims(self.temporal_downsample_factor, video_frames)
        init_images = [maybe(self.normalize_img)(i) for i in cast_tuple(init_images, num_unets)]
        skip_steps, sigma_min, sigma_max = (cast_tuple(v, num_unets) for v in (skip_steps, sigma_min, sigma_max))
        noise_fn = noise if callable(noise) else None
        noise = list(noise) if exists(noise) and not exists(noise_fn) else None
        if start_at_unet_number > 1:
            assert start_at_unet_number <= num_unets, 'must start a unet that is less than the total number of unets'
            assert not exists(stop_at_unet_number) or start_at_unet_number <= stop_at_unet_number
            assert exists(start_image_or_video), 'starting image or video must be supplied if only doing upscaling'
            img = self._resize(start_image_or_video.to(device), self.image_sizes[start_at_unet_number - 2])
        outputs = []
        for (unet_number, unet, image_size, frame_dims, dynamic_threshold, unet_cond_scale, unet_init, unet_skip, smin, smax, unet_sampler,
             unet_steps, unet_eta) in zip(
                range(1, num_unets + 1), self.unets, self.image_sizes, all_frame_dims, self.dynamic_thresholding, cond_scale,
                init_images, skip_steps, sigma_min, sigma_max, samplers, steps_per_unet, etas):
            if unet_number < start_at_unet_number:
                continue
            assert not isinstance(unet, NullUnet), 'cannot sample from null unet'
            lowres_cond_img = lowres_noise_times = None
            if unet.lowres_cond:
                lowres_cond_img, lowres_noise_times = self._lowres_conditioning(
                    img, lowres_sample_noise_level, image_size, frame_dims[0], batch_size, device,
                    lambda x: noise_fn(tuple(x.shape)) if exists(noise_fn) else (noise.pop(0) if exists(noise) else torch.randn_like(x)))
            if exists(unet_init):
                unet_init = self._resize(unet_init, image_size, frame_dims[0])
            shape = (batch_size, self.channels, *frame_dims, image_size, image_size)
            multistep = dict(sampler=unet_sampler, sample_steps=unet_steps, eta=unet_eta) if unet_sampler == 'dpmpp2m' else {}
            multistep.update(consistent)
            inpaint = {}
            if has_inpainting:
                inpaint = dict(inpaint_images=inpaint_images, inpaint_masks=inpaint_masks, inpaint_resample_times=inpaint_resample_times)
            unet_noise = noise_fn
            if exists(noise):    # this U-Net's share of the list, counted on its host table: the initial image, then one draw per Heun
                if unet_sampler == 'dpmpp2m':                                      # step or per row with kn != 0
                    n_draws = int((self._dpmpp2m_tables(unet_number - 1, unet_steps, unet_eta, smin, smax)[1][:, 3] != 0).sum())
                else:
                    n_draws = len(self._heun_tables(unet_number - 1, smin, smax, unet_skip)[0])
                if has_inpainting:
                    n_draws = self.inpaint_draws(n_draws, inpaint_resample_times)
                unet_noise = [noise.pop(0) for _ in range(1 + n_draws)]
            img = self.one_unet_sample(unet, shape, unet_number=unet_number, init_images=unet_init, skip_steps=unet_skip,
                                       sigma_min=smin, sigma_max=smax, cond_scale=unet_cond_scale, dynamic_threshold=dynamic_threshold,
                                       use_tqdm=use_tqdm, noise=unet_noise, **multistep, **inpaint,
                                       **({'cond_images': cond_images.to(device).float()} if exists(cond_images) else {}),
                                       **self._unet_kwargs(unet, lowres_cond_img, lowres_noise_times))
            outputs.append(img)
            if exists(stop_at_unet_number) and stop_at_unet_number == unet_number:
                break
        return outputs[-1] if not return_all_unet_outputs else outputs

    # ---- training ------------------------------------------------------------------------------------
    def forward(self, images, unet=None, texts=None, text_embeds=None, text_masks=None, unet_number=None, cond_images=None,
                noise=None, sigmas=None, lowres_aug_times=None, lowres_noise=None, lowres_img=None, **kwargs):
        """:712-882 -> scalar loss.  ``noise`` / ``sigmas`` / ``lowres_aug_times`` / ``lowres_noise`` are optional injection
        hooks for parity tests (the reference draws them internally)."""
        assert texts is None and text_embeds is None
        assert images.shape[-1] == images.shape[-2], \
            f'the images you pass in must be a square, but received dimensions of {images.shape[2]}, {images.shape[-1]}'
        assert not (len(self.unets) > 1 and not exists(unet_number)), \
            f'you must specify which unet you want trained, from a range of 1 to {len(self.unets)}, if you are training cascading DDPM (multiple unets)'
        unet_number = default(unet_number, 1)
        assert not exists(self.only_train_unet_number) or self.only_train_unet_number == unet_number
        assert images.dtype == torch.float, f'images tensor needs to be floats but {images.dtype} dtype found instead'
        unet_index = unet_number - 1
        unet = default(unet, lambda: self.get_unet(unet_number))
        inner = unet.module if hasattr(unet, 'module') else unet
        assert not isinstance(inner, NullUnet), 'null unet cannot and should not be trained'
        target_image_size = self.image_sizes[unet_index]
        prev_image_size = self.image_sizes[unet_index - 1] if unet_index > 0 else None
        hp = self.hparams[unet_index]
        B, c, frames, h, w = images.shape
        device = images.device
        assert c == self.channels and h >= target_image_size and w >= target_image_size
        all_frame_dims = tuple(fd[0] for fd in calc_all_frame_dims(self.temporal_downsample_factor, frames))
        target_frames = all_frame_dims[unet_index]
        prev_frames = all_frame_dims[unet_index - 1] if unet_index > 0 else None

        lowres_cond_img = None
        if exists(prev_image_size):
            # the reference derives the conditioning by down/up-sampling `images` (:781-782); IQT supplies a real
            # low-quality patch through `lowres_img` (superset: ImagenTrainer's dataloader keyword)
            lowres_cond_img = self._resize(lowres_img.to(device), target_image_size, target_frames) if exists(lowres_img) else \
                self._resize(self._resize(images, prev_image_size, prev_frames), target_image_size, target_frames)
            if not exists(lowres_aug_times):
                if self.per_sample_random_aug_noise_level:
                    lowres_aug_times = self.lowres_noise_schedule.sample_random_times(B, device='cpu')
                else:
                    lowres_aug_times = self.lowres_noise_schedule.sample_random_times(1, device='cpu').repeat(B)
            lowres_aug_times = lowres_aug_times.detach().cpu().float()
        images = self.normalize_img(self._resize(images, target_image_size, target_frames)).float().contiguous()
        lowres_noise_cond = None
        if exists(lowres_cond_img):
            lowres_cond_img = self.normalize_img(lowres_cond_img).float().contiguous()
            ln = default(lowres_noise, lambda: torch.randn_like(lowres_cond_img)).to(device)
            lowres_cond_img = self._noise_lowres(lowres_cond_img, lowres_aug_times, ln)
            lowres_noise_cond = self.lowres_noise_schedule.get_condition(lowres_aug_times).to(device)   # log-SNR at training (:838)

        sig = default(sigmas, lambda: self.noise_distribution(hp.P_mean, hp.P_std, B)).detach().float().cpu()
        noise = default(noise, lambda: torch.randn_like(images)).to(device).contiguous()
        one = torch.ones(B, device=device)
        noised = ops.axpby3(images, noise, None, one, sig.to(device), None)              # alphas are 1 in EDM (:829)

        # denoised = c_skip*x + c_out*F(c_in*x, c_noise); weighted MSE folded into ONE kernel on the raw network output:
        #   w*(c_skip x + c_out F - y)^2 = (w c_out^2) * (F - (y - c_skip x)/c_out)^2
        cin, cskip, cout = (f(hp.sigma_data, sig) for f in (self.c_in, self.c_skip, self.c_out))
        x_in = ops.axpby3(noised, None, None, cin.to(device), None, None)
        ukw = {**self._unet_kwargs(unet, lowres_cond_img, lowres_noise_cond), **kwargs}
        if exists(cond_images):                                                   # image conditioning of the U-Net (:718, 844)
            ukw['cond_images'] = cond_images.to(device).float()
        # self-conditioning (:847-860): half of the steps first estimate x0 without gradients and feed it back.  The reference's gate
        # `self_cond = unet.module.self_cond if DDP else unet` (:849) is always truthy for an un-wrapped U-Net, so it consumes one
        # `random()` per call whether or not the U-Net self-conditions (a U-Net without the option ignores the estimate): the draw is
        # mirrored so Python's RNG stream matches, the wasted pre-pass is not
        draw = random() if (not hasattr(unet, 'module') or getattr(inner, 'self_cond', False)) else 1.
        if getattr(inner, 'self_cond', False) and draw < 0.5:
            with torch.no_grad():
                pred_x0 = self.preconditioned_network_forward(unet.forward, noised, sig, sigma_data=hp.sigma_data, _replay=False,
                                                              **ukw).detach()
            ukw['self_cond'] = pred_x0
        net_out = unet.forward(x_in, self.c_noise(sig).to(device), **ukw)
        target = ops.axpby3(images, noised, None, (1. / cout).to(device), (-cskip / cout).to(device), None)
        weight = (self.loss_weight(hp.sigma_data, sig) * cout ** 2).to(device)
        loss, _ = ops.mse_clamp(net_out, target, do_clamp=False, weight=weight)
        return loss
