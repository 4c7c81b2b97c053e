"""DDPM inpainting per window on a real MI355X: ``ops.ddpm_inpaint_paste`` bit for bit against the ``ops.axpby3`` / ``ops.q_sample`` /
``ops.mask_blend`` sequence it replaces, ``Imagen.sample(inpaint_images=..., inpaint_masks=...)`` against the real reference's run with
its re-noise branch recorded in tests/golden/ddpm_inpaint.npz (tools/make_golden_ddpm_inpaint.py), and every tensor ``sample`` returns
against the unfused loop (three launches per pass boundary) assembled here from the single-purpose ops, bit for bit."""
import numpy as np
import pytest
import torch

from tests.conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = lambda a: torch.from_numpy(np.asarray(a))


# ---- the kernel ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('inplace', [False, True], ids=['fresh', 'inplace'])
@pytest.mark.parametrize('renoise', [False, True], ids=['plain', 'renoise'])
def test_inpaint_paste_is_the_q_sample_mask_blend_axpby3_sequence(renoise, inplace):
    """B = 2 rows with different coefficients, per_batch = 1000 (not a multiple of the 256-element block: a tail block per sample).
    Signed zeros in x at unmasked elements: the selection keeps them, and the re-noise maps them as axpby3 does."""
    from diffusioniqt_amd import ops
    g = torch.Generator().manual_seed(3)
    shape = (2, 1, 10, 10, 10)
    x, n, known, qn = (torch.randn(shape, generator=g).to(DEV) for _ in range(4))
    x.view(-1)[:4] = torch.tensor([0.0, -0.0, 0.0, -0.0])
    n.view(-1)[:4] = torch.tensor([0.0, 0.0, -0.0, -0.0])
    mask = torch.rand(shape, generator=g) < 0.4
    mask.view(-1)[:4] = False
    mask_b, mask_f = mask.to(DEV).to(torch.uint8), mask.to(DEV).float()
    kr0, kr1 = torch.tensor([0.625, 0.9375], device=DEV), torch.tensor([0.78125, 0.34375], device=DEV)
    al, sg = torch.tensor([0.125, 0.875], device=DEV), torch.tensor([0.96875, 0.46875], device=DEV)
    t = ops.axpby3(x, n, None, kr0, kr1, None, 0.0, 0.0, 0) if renoise else x
    want = ops.mask_blend(t, ops.q_sample(known, qn, al, sg), mask_f)
    args = (n if renoise else None, known, mask_b, qn, kr0 if renoise else None, kr1 if renoise else None, al, sg)
    src = x.clone()
    got = ops.ddpm_inpaint_paste(src, *args, out=src if inplace else None)
    assert (got.data_ptr() == src.data_ptr()) == inplace and (inplace or torch.equal(src.view(torch.int32), x.view(torch.int32)))
    assert got.unique().numel() > 1000
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))           # the bits, signed zeros included
    if not renoise:
        assert [bool(v) for v in torch.signbit(got.view(-1)[:4]).cpu()] == [False, True, False, True]
    m = mask.to(DEV)
    assert torch.equal(got[m], ops.q_sample(known, qn, al, sg)[m])              # masked: alpha known + sigma n, whatever x holds
    assert torch.equal(ops.ddpm_inpaint_paste(x, args[0], known, m, *args[3:]), got)      # a bool mask


def test_inpaint_paste_argument_errors():
    from diffusioniqt_amd import ops
    x = torch.zeros(2, 1, 4, 4, 4, device=DEV)
    k, m = torch.zeros(2, device=DEV), torch.zeros(2, 1, 4, 4, 4, device=DEV, dtype=torch.uint8)
    with pytest.raises(ValueError, match="mask"):
        ops.ddpm_inpaint_paste(x, None, x, m.float(), x, None, None, k, k)
    with pytest.raises(ValueError, match="mask"):
        ops.ddpm_inpaint_paste(x, None, x, m[:, :, :3].contiguous(), x, None, None, k, k)
    with pytest.raises(ValueError, match="known"):
        ops.ddpm_inpaint_paste(x, None, x[:1].contiguous(), m, x, None, None, k, k)
    with pytest.raises(ValueError, match="kr0"):
        ops.ddpm_inpaint_paste(x, x, x, m, x, None, k, k, k)
    with pytest.raises(ValueError, match="sg"):
        ops.ddpm_inpaint_paste(x, None, x, m, x, None, None, k, k[:1].contiguous())


# ---- sample() against the real reference ---------------------------------------------------------------------------------------------------
def _close(got, ref, tol, floor, what):
    """``tests.test_gpu_unet.close`` with its additive floor as a parameter: max error <= tol x the largest |reference| + floor."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, f"{what}: {tuple(got.shape)} vs {tuple(ref.shape)}"
    err, scale = (got - ref).abs().max().item(), ref.abs().max().item()
    print(f"{what}: max err {err:.3e} = {err / scale:.3e} of the scale {scale:.3e} (allowed {tol:.3e} of it + {floor:.1e})")
    assert err <= tol * scale + floor, f"{what}: max err {err:.3e}, scale {scale:.3e}"
    return err / scale


@pytest.mark.parametrize('resample', [1, 2])
def test_sample_inpaint_matches_reference_golden(resample):
    """R = 1: the thresholds of the ``inpaint`` case of tests/test_gpu_unet.py (the same network and objective, static clamp): max error
    <= 5e-4 of the largest reference magnitude + 1e-6, for the image and the two per-step lists.  R = 2, the run with the re-noise
    branch: both thresholds times d2 / d1, d_R the reference's own fp32-versus-float64 distance of that run, measured when the fixture
    was made and stored in it."""
    from tests.test_gpu_unet import _imagen_for
    g = load_golden('ddpm_inpaint')
    Tn, mb = int(g['timesteps']), float(g['min_bound'])
    imagen = _imagen_for(load_golden('unetA_tiny'), 'x_start', False, 'z-score', Tn, mb)
    draws = list(T(g[f'draws{resample}']))
    assert len(draws) == int(g[f'consumed{resample}']) == imagen.inpaint_draws(Tn, resample)
    img, noisy, x0 = imagen.sample(batch_size=1, start_image_or_video=T(g['lowres']).to(DEV), start_at_unet_number=2, use_tqdm=False,
                                   noise=draws, inpaint_images=T(g['known']).to(DEV), inpaint_masks=T(g['mask']).bool().to(DEV),
                                   inpaint_resample_times=resample)
    scale = 1.0 if resample == 1 else float(g['d2']) / float(g['d1'])
    tol, floor = 5e-4 * scale, 1e-6 * scale
    print(f"d1 {float(g['d1']):.3e}, d2 {float(g['d2']):.3e}, scale {scale:.4f}")
    _close(img, T(g[f'img{resample}']), tol, floor, f"R = {resample} img")
    ref_noisy = T(g[f'noisy{resample}'])
    assert len(noisy) == ref_noisy.shape[0] == Tn + 1
    _close(T(np.stack(noisy[:-2])), ref_noisy[:-2], tol, floor, f"R = {resample} noisy list")
    # the reference clamps in place, so its last two entries (one tensor) are clamped
    _close(T(np.stack(noisy[-2:])).clamp(min=mb), ref_noisy[-2:], tol, floor, f"R = {resample} noisy tail")
    _close(T(np.stack(x0)), T(g[f'x0{resample}']), tol, floor, f"R = {resample} x0 list")


# ---- sample() against the unfused loop, bit for bit ---------------------------------------------------------------------------------------
def _unfused(imagen, den, lowres, known, mask, draws, R):
    """``p_sample_loop`` with the pass boundary as three launches and two temporaries -- ``ops.q_sample``, ``ops.mask_blend`` with a float
    mask, ``ops.axpby3`` -- and the step through the window denoiser's ``x0`` and ``ops.ddpm_step``."""
    from diffusioniqt_amd import ops
    B = lowres.shape[0]
    draws = [d.to(DEV).contiguous() for d in draws]
    row = lambda t, i, j: torch.full((B,), float(t[i][j]), device=DEV)
    mask_f = mask.to(DEV).float().expand(known.shape).contiguous()
    img, x_start, noisy, x0s = draws.pop(0), None, [], []
    for i in range(den.num_steps):
        for r in reversed(range(R)):
            img = ops.mask_blend(img, ops.q_sample(known, draws.pop(0), row(den.qs, i, 0), row(den.qs, i, 1)), mask_f)
            pred = den.x0(img, lowres, i, self_cond=x_start if den.self_cond else None)
            img, x_start = ops.ddpm_step(img, pred, draws.pop(0), *(row(den.coefs, i, j) for j in range(3)), *den.clamp)
            if r > 0 and i + 1 < den.num_steps:
                img = ops.axpby3(img, draws.pop(0), None, row(den.renoise, i, 0), row(den.renoise, i, 1), None, 0.0, 0.0, 0)
        noisy.append(img)
        x0s.append(x_start)
    assert not draws
    return imagen._finish_sample(img), noisy + [img], x0s + [x_start]


@pytest.mark.parametrize('self_cond', [False, True], ids=['plain', 'selfcond'])
@pytest.mark.parametrize('mode', ['clamp-min', 'dynamic'])
@pytest.mark.parametrize('resample', [1, 3])
def test_sample_inpaint_is_the_unfused_loop_bit_for_bit(resample, mode, self_cond):
    from tests import volume_joint_reference as J
    from tests.test_gpu_volume_joint import stub_imagen
    imagen = stub_imagen('x_start', mode, size=8, unet=J.make_self_cond_unet() if self_cond else None)
    g = torch.Generator().manual_seed(8)
    steps, B = 4, 2
    n = imagen.inpaint_draws(steps, resample)
    draws = [torch.randn(B, 1, 8, 8, 8, generator=g) for _ in range(n)]
    lowres, known = (torch.randn(B, 1, 8, 8, 8, generator=g).to(DEV) for _ in range(2))
    mask = torch.rand(B, 1, 8, 8, 8, generator=g) < 0.4
    den = imagen.window_denoiser(sampler='ddpm', sample_steps=steps)
    want = _unfused(imagen, den, lowres, known, mask, list(draws), resample)
    call = dict(batch_size=B, start_image_or_video=lowres, start_at_unet_number=2, use_tqdm=False, sample_steps=steps,
                inpaint_images=known, inpaint_masks=mask, inpaint_resample_times=resample)
    got = imagen.sample(noise=list(draws) + [torch.full((B, 1, 8, 8, 8), float('nan'))], **call)   # the entry past the count is not taken
    assert got[0].unique().numel() > 500 and torch.isfinite(got[0]).all()
    assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32))
    for name, a, b in (('noisy', got[1], want[1]), ('x0', got[2], want[2])):
        assert len(a) == len(b) == steps + 1
        for k, (u, v) in enumerate(zip(a, b)):
            assert np.array_equal(u.view(np.int32), v.cpu().numpy().view(np.int32)), (name, k)
    calls = []

    def source(shape):
        calls.append(tuple(shape))
        return draws[len(calls) - 1].to(DEV)
    by_source = imagen.sample(noise=source, **call)
    assert len(calls) == n and torch.equal(by_source[0], got[0])
    if resample > 1:                                                             # the re-noise is in the chain
        once = imagen.sample(noise=list(draws), **{**call, 'inpaint_resample_times': 1})
        assert not torch.equal(once[0], got[0])
