"""EDM inpainting per window on a real MI355X: ``ops.edm_inpaint_churn`` bit for bit against the ``ops.axpby3`` / ``ops.mask_blend``
sequence it replaces, ``ElucidatedImagen.sample(inpaint_images=..., inpaint_masks=...)`` against the real reference's run recorded in
tests/golden/edm_inpaint.npz (tools/make_golden_edm_inpaint.py), the two identities (nothing masked: today's ``sample``; everything
masked: the known image), and the draw order of the list and callable forms of ``noise``."""
import json

import numpy as np
import pytest
import torch

from tests import volume_joint_heun_reference as HN
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = lambda a: torch.from_numpy(np.asarray(a))


# ---- the kernel ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kc', [(0.0, 0.0), (0.625, 0.3)], ids=['kc-zero', 'kc'])
@pytest.mark.parametrize('renoise', [False, True], ids=['plain', 'renoise'])
def test_inpaint_churn_is_the_axpby3_mask_blend_sequence(renoise, kc):
    """B = 2, per_batch = 1000 (not a multiple of the 256-element block: a tail block per sample), one coefficient per sample."""
    from diffusioniqt_amd import ops
    g = torch.Generator().manual_seed(3)
    shape = (2, 1, 10, 10, 10)
    x, n, known, eps = (torch.randn(shape, generator=g).to(DEV) for _ in range(4))
    x.view(-1)[:4] = torch.tensor([0.0, -0.0, 0.0, -0.0])                      # signed zeros under both signs of eps
    eps.view(-1)[:4] = torch.tensor([1.0, 1.0, -1.0, -1.0])
    mask = torch.rand(shape, generator=g) < 0.4
    mask.view(-1)[:4] = False
    mask_b, mask_f = mask.to(DEV).to(torch.uint8), mask.to(DEV).float()
    one, kr, kc = torch.ones(2, device=DEV), torch.tensor([0.375, 1.25], device=DEV), torch.tensor(kc, device=DEV)
    t = ops.axpby3(x, n, None, one, kr, None) if renoise else x
    want = ops.axpby3(ops.mask_blend(t, known, mask_f), eps, None, one, kc, None)
    got = ops.edm_inpaint_churn(x, n if renoise else None, known, mask_b, eps, kr if renoise else None, kc)
    assert got.data_ptr() != x.data_ptr() and got.unique().numel() > 1000
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))           # the bits, signed zeros included
    assert torch.equal(ops.edm_inpaint_churn(x, n if renoise else None, known, mask.to(DEV), eps, kr if renoise else None, kc), got)   # a bool mask
    m = mask.to(DEV)
    assert torch.equal(got[m], ops.axpby3(known, eps, None, one, kc, None)[m])  # masked: known + kc eps, whatever x holds
    x2 = x.clone()
    same = ops.edm_inpaint_churn(x2, n if renoise else None, known, mask_b, eps, kr if renoise else None, kc, out=x2)
    assert same.data_ptr() == x2.data_ptr() and torch.equal(x2.view(torch.int32), want.view(torch.int32))


def test_inpaint_churn_argument_errors():
    from diffusioniqt_amd import ops
    x = torch.zeros(2, 1, 4, 4, 4, device=DEV)
    k, m = torch.zeros(2, device=DEV), torch.zeros(2, 1, 4, 4, 4, device=DEV, dtype=torch.uint8)
    with pytest.raises(ValueError, match="mask"):
        ops.edm_inpaint_churn(x, None, x, m.float(), x, None, k)
    with pytest.raises(ValueError, match="mask"):
        ops.edm_inpaint_churn(x, None, x, m[:, :, :3].contiguous(), x, None, k)
    with pytest.raises(ValueError, match="known"):
        ops.edm_inpaint_churn(x, None, x[:1].contiguous(), m, x, None, k)
    with pytest.raises(ValueError, match="kr"):
        ops.edm_inpaint_churn(x, x, x, m, x, None, k)
    with pytest.raises(ValueError, match="kc"):
        ops.edm_inpaint_churn(x, None, x, m, x, None, k[:1].contiguous())


# ---- sample() against the real reference ---------------------------------------------------------------------------------------------------
def _edm(steps=3):
    from tests.test_gpu_family_b import make_edm
    kw = {k: (tuple(v) if isinstance(v, list) else v) for k, v in json.loads(str(load_golden('unet3d_tiny')['kwargs'])).items()}
    return make_edm(kw, steps)


@pytest.mark.parametrize('resample', [1, 2])
def test_sample_inpaint_matches_reference_golden(resample):
    """R = 1: the rule of ``edm_sample`` (tests/test_gpu_family_b.py; the same number of evaluations): max error <= 5e-3 and fewer than
    3 % of the voxels above 2e-4.  R = 2: both thresholds times max(1, d2 / d1), d_R the reference's own fp32-versus-float64 distance of
    that run, measured when the fixture was made and stored in it.  Masked voxels are the known values exactly."""
    g = load_golden('edm_inpaint')
    elu = _edm()
    draws = list(T(g[f'draws{resample}']))
    assert len(draws) == int(g[f'consumed{resample}'])
    known, mask = T(g['known']), T(g['mask']).bool()
    img = elu.sample(batch_size=1, video_frames=8, start_image_or_video=T(g['lowres']).to(DEV), start_at_unet_number=2, use_tqdm=False,
                     noise=draws, inpaint_images=known.to(DEV), inpaint_masks=mask.to(DEV), inpaint_resample_times=resample).cpu()
    scale = 1.0 if resample == 1 else max(1.0, float(g['d2']) / float(g['d1']))
    err = (img - T(g[f'img{resample}'])).abs()
    worst, share = err.max().item(), (err > 2e-4 * scale).float().mean().item()
    print(f"sample(inpaint, R = {resample}) vs the reference: max {worst:.3e} (allowed {5e-3 * scale:.3e}), {share:.4f} of the voxels above "
          f"{2e-4 * scale:.3e} (allowed 0.03); d1 {float(g['d1']):.3e}, d2 {float(g['d2']):.3e}")
    assert torch.equal(img[mask[:, None]], known[mask[:, None]])
    assert worst <= 5e-3 * scale and share < 0.03


# ---- the two identities --------------------------------------------------------------------------------------------------------------------
def test_nothing_masked_and_one_pass_is_todays_sample():
    g = load_golden('edm_inpaint')
    elu = _edm()
    draws = list(T(g['draws1']))
    call = dict(batch_size=1, video_frames=8, start_image_or_video=T(g['lowres']).to(DEV), start_at_unet_number=2, use_tqdm=False)
    plain = elu.sample(noise=list(draws), **call)
    empty = elu.sample(noise=list(draws), inpaint_images=T(g['known']).to(DEV), inpaint_masks=torch.zeros(1, 8, 8, 8, dtype=torch.bool),
                       inpaint_resample_times=1, **call)
    assert plain.unique().numel() > 50 and torch.equal(empty, plain)            # most of the 512 voxels of this network sit at the clamp


def _stub_edm(auto_normalize, steps=3, self_cond=False):
    from diffusioniqt_amd.elucidated_imagen import ElucidatedImagen
    from diffusioniqt_amd.imagen_pytorch3D import NullUnet
    return ElucidatedImagen(unets=(NullUnet(), HN.make_stub_unet(self_cond)), image_sizes=(8, 8), channels=1, condition_on_text=False,
                            auto_normalize_img=auto_normalize, cond_drop_prob=0.0, dynamic_thresholding=False,
                            **{**HN.HP, 'S_churn': 80, 'num_sample_steps': steps}).to(DEV)


@pytest.mark.parametrize('auto_normalize', [False, True], ids=['raw', 'normalized'])
def test_everything_masked_returns_the_known_image(auto_normalize):
    elu = _stub_edm(auto_normalize)
    g = torch.Generator().manual_seed(5)
    known = torch.rand(2, 1, 8, 8, 8, generator=g).to(DEV)
    lowres = torch.rand(2, 1, 8, 8, 8, generator=g).to(DEV)
    out = elu.sample(video_frames=8, start_image_or_video=lowres, start_at_unet_number=2, use_tqdm=False, inpaint_images=known,
                     inpaint_masks=torch.ones(2, 8, 8, 8, dtype=torch.bool), inpaint_resample_times=2)       # batch_size broadcasts to 2
    assert out.shape == known.shape and torch.equal(out, elu.unnormalize_img(elu.normalize_img(known)))


# ---- draw order: list and callable forms, skip_steps and init_images ------------------------------------------------------------------------
@pytest.mark.parametrize('skip', [None, 1])
def test_noise_list_and_callable_follow_the_reference_call_order(skip):
    from diffusioniqt_amd.elucidated_imagen import ElucidatedImagen
    elu = _stub_edm(True, steps=4, self_cond=True)
    g = torch.Generator().manual_seed(6)
    R, steps = 3, 4 - (skip or 0)
    n = 2 + ElucidatedImagen.inpaint_draws(steps, R)
    draws = [torch.randn(2, 1, 8, 8, 8, generator=g) for _ in range(n)]
    known, lowres, init = (torch.rand(2, 1, 8, 8, 8, generator=g).to(DEV) for _ in range(3))
    mask = torch.rand(2, 8, 8, 8, generator=g) < 0.3
    call = dict(batch_size=2, video_frames=8, start_image_or_video=lowres, start_at_unet_number=2, use_tqdm=False, inpaint_images=known,
                inpaint_masks=mask, inpaint_resample_times=R, skip_steps=skip, init_images=init if skip else None)
    by_list = elu.sample(noise=list(draws) + [torch.full((2, 1, 8, 8, 8), float('nan'))], **call)      # the entry past the count is not taken
    calls = []

    def source(shape):
        calls.append(tuple(shape))
        return draws[len(calls) - 1].to(DEV)
    by_source = elu.sample(noise=source, **call)
    assert len(calls) == n and set(calls) == {(2, 1, 8, 8, 8)}
    assert torch.isfinite(by_list).all() and torch.equal(by_list, by_source) and by_list.unique().numel() > 100
    m = mask[:, None].to(DEV)
    assert torch.equal(by_list[m], elu.unnormalize_img(elu.normalize_img(known))[m])
    other = elu.sample(noise=list(reversed(draws)), **call)                       # the order matters
    assert not torch.equal(other, by_list)
