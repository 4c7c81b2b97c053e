"""TEST INFRASTRUCTURE (container-only): the EDM inpainting fixture from the REAL reference (elucidated_imagen.py:441-449, 473-530: the
RePaint loop around the stochastic Heun sampler).  Run: python tools/make_golden_edm_inpaint.py   (needs the reference checkout that
oracle/ref_shim.py imports; CPU; ~1 min).  Writes tests/golden/edm_inpaint.npz -- numbers only.

The network is make_golden_b.py's: the ``unet3d_tiny`` kwargs with ``hash_fill_state_dict(..., 11)`` as the second U-Net of a cascade,
8^3, B = 1, 3 steps, default churn (step 0 has gamma 0, step 1 gamma > 0).  One run at ``inpaint_resample_times=1`` and one at 2; per run
every normal the reference draws, in call order (``torch.randn`` / ``torch.randn_like`` are patched with a queue), the output and the
queue length consumed.  ``d1`` / ``d2``: the reference's OWN fp32-versus-float64 distance (max |difference| of the two outputs on the
same draws) for the two runs -- the scale of the tolerance of the R = 2 comparison in tests/test_gpu_edm_inpaint.py."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
import ref_shim  # noqa: E402
from iqt_oracle import hash_fill_state_dict  # noqa: E402
from make_golden import save  # noqa: E402
from make_golden_b import unet3d_kwargs  # noqa: E402

S, B, STEPS = 8, 1, 3


def n_draws(R):
    """lowres noise, initial image, then per (step, r) the eps and -- unless r == 0 or it is the last step -- the re-noise normal."""
    return 2 + STEPS * R + (STEPS - 1) * (R - 1)


def run(elu, dtype, lowres, known, mask, draws, R):
    queue = [d.to(dtype) for d in draws]
    o_randn, o_like, o_softmax = torch.randn, torch.randn_like, torch.Tensor.softmax
    torch.randn = lambda *a, **k: queue.pop(0).clone()
    torch.randn_like = lambda *a, **k: queue.pop(0).clone()
    if dtype == torch.float64:                     # the attention asks for an fp32 softmax by name: the float64 run keeps float64
        torch.Tensor.softmax = lambda self, *a, dtype=None, **k: o_softmax(self, *a, **k)
    torch.set_default_dtype(dtype)                 # the tensors the sampler makes on the way (sigma vectors, time embeddings) follow
    try:
        img = elu.sample(batch_size=B, video_frames=S, start_image_or_video=lowres.to(dtype), start_at_unet_number=2, use_tqdm=False,
                         inpaint_images=known.to(dtype), inpaint_masks=mask, inpaint_resample_times=R)
    finally:
        torch.set_default_dtype(torch.float32)
        torch.randn, torch.randn_like, torch.Tensor.softmax = o_randn, o_like, o_softmax
    return img, len(draws) - len(queue)


if __name__ == "__main__":
    r3, rv, re_, rt = ref_shim.import_reference()
    torch.set_num_threads(8)
    g = torch.Generator().manual_seed(4242)
    kw = unet3d_kwargs()
    base = rv.Unet3D(**unet3d_kwargs(lowres_cond=False, dim_mults=(1, 2), layer_attns=False))
    sr = rv.Unet3D(**kw)
    elu = re_.ElucidatedImagen(unets=(base, sr), image_sizes=(S, S), channels=1, condition_on_text=False, auto_normalize_img=False,
                               cond_drop_prob=0.0, num_sample_steps=STEPS, dynamic_thresholding=False)
    unet = elu.unets[1]
    unet.load_state_dict(hash_fill_state_dict(unet.state_dict(), 11))

    lowres = torch.randn(B, 1, S, S, S, generator=g).clamp(-1, 1)
    known = (torch.rand(B, 1, S, S, S, generator=g) * 2 - 1)
    mask = torch.zeros(B, S, S, S, dtype=torch.bool)
    mask[:, 1:5, 2:7, 3:6] = True                                              # a box ...
    mask |= torch.rand(B, S, S, S, generator=g) < 0.1                          # ... and scattered voxels
    out = dict(lowres=lowres, known=known, mask=mask.to(torch.uint8), lowres_noise_level=0.2)
    dist = {}
    for R in (1, 2):
        draws = [torch.randn(B, 1, S, S, S, generator=g) for _ in range(n_draws(R) + 2)]      # two spare: the count is measured
        img, used = run(elu, torch.float32, lowres, known, mask, draws, R)
        assert used == n_draws(R), (used, n_draws(R))
        assert torch.equal(img[mask[:, None]], known[mask[:, None]])
        elu.double()
        img64, used64 = run(elu, torch.float64, lowres, known, mask, draws, R)
        elu.float()
        assert used64 == used and img64.dtype == torch.float64
        dist[R] = (img.double() - img64).abs().max().item()
        e = (img.double() - img64).abs()
        print(f"R = {R}: {used} draws, fp32 vs float64 of the reference: max {dist[R]:.3e}, mean {e.mean().item():.3e}, "
              f"{(e > 2e-4).double().mean().item():.4f} of the voxels above 2e-4")
        out.update({f'draws{R}': torch.stack(draws[:used]), f'img{R}': img, f'consumed{R}': used, f'd{R}': dist[R]})
    save("edm_inpaint", **out)
