"""TEST INFRASTRUCTURE (container-only): the DDPM inpainting fixture from the REAL reference (imagen_pytorch3D.py:2116-2146: the RePaint
loop around the ancestral sampler, with its re-noise branch).  Run: python tools/make_golden_ddpm_inpaint.py   (needs the reference
checkout that oracle/ref_shim.py imports; CPU; ~1 min).  Writes tests/golden/ddpm_inpaint.npz -- numbers only.

The network is make_golden_next.py's: the ``unetA_tiny`` kwargs with ``hash_fill_state_dict(..., 0)`` as the second U-Net of a cascade,
x_start objective, static clamp, z-score, 8^3, B = 1, ``timesteps = 3``.  One run at ``inpaint_resample_times=1`` and one at 2; per run
every normal the reference draws, in call order (``torch.randn`` / ``torch.randn_like`` are patched with a queue), the output, the two
per-step lists and the queue length consumed.  ``d1`` / ``d2``: the reference's OWN fp32-versus-float64 distance (max |difference| of
the two outputs on the same draws) for the two runs -- the scale of the tolerance of the R = 2 comparison in
tests/test_gpu_ddpm_inpaint.py.

The re-noise branch of the reference (:2139-2146) calls ``self.right_pad_dims_to_datatype``, a method its class does not define, so as it
stands the loop raises at R >= 2.  The instance gets that ONE method here, with the only meaning the call site admits -- the [B] flags
``is_last_timestep`` as [B,1,1,1,1], so that ``torch.where`` broadcasts them over the image; everything else that runs is the
reference's own code."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
import ref_shim  # noqa: E402
from make_golden import MIN_BOUND, base_configs, fill, save, unet_kwargs_train_py  # noqa: E402

S, B, STEPS, DIM = 8, 1, 3, 16


def n_draws(R):
    """The initial image, then per (step, r) the q-noise and the step noise and -- unless r == 0 or it is the last step -- the re-noise."""
    return 1 + 2 * STEPS * R + (STEPS - 1) * (R - 1)


def run(imagen, dtype, lowres, known, mask, draws, R):
    queue = [d.to(dtype) for d in draws]
    o_randn, o_like = torch.randn, torch.randn_like
    torch.randn = lambda *a, **k: queue.pop(0).clone()
    torch.randn_like = lambda *a, **k: queue.pop(0).clone()
    torch.set_default_dtype(dtype)                 # the tensors the sampler makes on the way (times, embeddings) follow
    sched = imagen.noise_schedulers[1]
    log_snr = sched.log_snr
    if dtype == torch.float64:
        # the schedule itself stays the fp32 one, widened: the cosine log-SNR is singular at t = 1 (about -34 in fp32, -74 in float64,
        # and the U-Net is conditioned on it), so a float64 schedule would be another chain, not this chain in higher precision
        sched.log_snr = lambda t: log_snr(t.float()).double()
    try:
        img, noisy, x0 = imagen.sample(batch_size=B, start_image_or_video=lowres.to(dtype), start_at_unet_number=2, use_tqdm=False,
                                       inpaint_images=known.to(dtype), inpaint_masks=mask, inpaint_resample_times=R)
    finally:
        sched.log_snr = log_snr
        torch.set_default_dtype(torch.float32)
        torch.randn, torch.randn_like = o_randn, o_like
    return img, np.stack(noisy), np.stack(x0), len(draws) - len(queue)


if __name__ == "__main__":
    r3, _, _, _ = ref_shim.import_reference()
    torch.set_num_threads(8)
    g = torch.Generator().manual_seed(2424)
    unet = r3.SRUnet256(**unet_kwargs_train_py(DIM, S))
    fill(unet)
    imagen = r3.Imagen(unets=(r3.NullUnet(), unet), configs=base_configs(), min_bound=MIN_BOUND, image_sizes=(S, S), channels=1,
                       pred_objectives='x_start', timesteps=STEPS, dynamic_thresholding=False, p2_loss_weight_gamma=0.0,
                       auto_normalize_img=False, cond_drop_prob=0.0, lpips=False, medlpips=False, boundary=False)
    imagen.unets[1].eval()
    imagen.right_pad_dims_to_datatype = lambda flags: flags.view(-1, 1, 1, 1, 1)          # see the module docstring

    lowres = torch.randn(B, 1, S, S, S, generator=g)
    known = torch.randn(B, 1, S, S, S, generator=g)
    mask = torch.zeros(B, 1, S, S, S, dtype=torch.bool)
    mask[:, :, 1:5, 2:7, 3:6] = True                                           # a box ...
    mask |= torch.rand(B, 1, S, S, S, generator=g) < 0.1                       # ... and scattered voxels
    out = dict(lowres=lowres, known=known, mask=mask.to(torch.uint8), min_bound=MIN_BOUND, timesteps=STEPS)
    for R in (1, 2):
        draws = [torch.randn(B, 1, S, S, S, generator=g) for _ in range(n_draws(R) + 2)]      # two spare: the count is measured
        img, noisy, x0, used = run(imagen, torch.float32, lowres, known, mask, draws, R)
        assert used == n_draws(R), (used, n_draws(R))
        imagen.double()
        img64, _, _, used64 = run(imagen, torch.float64, lowres, known, mask, draws, R)
        imagen.float()
        assert used64 == used and img64.dtype == torch.float64
        e = (img.double() - img64).abs()
        print(f"R = {R}: {used} draws, fp32 vs float64 of the reference: max {e.max().item():.3e}, mean {e.mean().item():.3e}; "
              f"largest |img| {img.abs().max().item():.3f}")
        out.update({f'draws{R}': torch.stack(draws[:used]), f'img{R}': img, f'noisy{R}': noisy, f'x0{R}': x0, f'consumed{R}': used,
                    f'd{R}': e.max().item()})
    save("ddpm_inpaint", **out)
