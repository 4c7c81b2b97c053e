"""The few-step sampler of ``Imagen.p_sample_loop`` / ``Imagen.sample`` on a real MI355X: ``sampler='ddim'`` and ``sample_steps`` against
the float64 loop of tests/anchored_noise_reference.py (the network replaced by an elementwise contraction, so sampler round-off is
not amplified), the tie to the reference-pinned ancestral path (eta = 1 on the golden trajectory's network and draws), callable
``noise=``, and volume-anchored noise under the sampler."""
import numpy as np
import pytest
import torch

from tests import anchored_noise_reference as A
from tests.conftest import load_golden
from tests.test_gpu_unet import T, build, close

pytestmark = pytest.mark.gpu
DEV = "cuda"
STEPS, SHAPE = 6, (2, 1, 8, 8, 8)
MIN_BOUND = -0.75


@pytest.fixture(scope="module")
def draws():
    """Low-res conditioning, the initial image and one draw per step (read only)."""
    g = torch.Generator().manual_seed(3)
    return [torch.randn(SHAPE, generator=g) for _ in range(STEPS + 2)]


def stub_imagen(kind, objective, norm, dynamic):
    from diffusioniqt_amd.imagen_pytorch3D import Imagen, NullUnet
    configs = {'Data': {'norm': norm}, 'Train': {'batch_sample': False}}
    return Imagen(unets=(NullUnet(), A.make_stub_unet()), configs=configs, min_bound=MIN_BOUND, image_sizes=(8, 8), channels=1,
                  pred_objectives=objective, noise_schedules=('cosine', kind), dynamic_thresholding=dynamic,
                  p2_loss_weight_gamma=0.0, cond_drop_prob=0.0).to(DEV)


@pytest.mark.parametrize('eta', [0.0, 0.5])
@pytest.mark.parametrize('mode', ['clamp-min', 'clamp-box', 'dynamic'])
@pytest.mark.parametrize('objective', ['noise', 'x_start', 'v'])
@pytest.mark.parametrize('kind', ['cosine', 'linear'])
def test_ddim_matches_the_float64_loop(draws, kind, objective, mode, eta):
    """Final image and every entry of the two per-step lists within steps * 8 * 2^-23 * max|x|: 8 fp32 operations per step on values
    of that size (max|x| over everything compared).  eta = 0 runs on a one-element noise list."""
    from diffusioniqt_amd.imagen_pytorch3D import log_snr_to_alpha_sigma
    norm, dynamic = ('z-score', False) if mode == 'clamp-min' else ('min-max', mode == 'dynamic')
    imagen = stub_imagen(kind, objective, norm, dynamic)
    lowres, init, steps = draws[0], draws[1], draws[2:]
    noise = [init] + (steps if eta > 0 else [])
    img, noisy, x0 = imagen.sample(batch_size=2, start_image_or_video=lowres.to(DEV), start_at_unet_number=2, use_tqdm=False,
                                   noise=noise, sampler='ddim', sample_steps=STEPS, eta=eta)
    assert len(noisy) == len(x0) == STEPS + 1

    sch = imagen.noise_schedulers[1]
    pairs = list(sch.get_sampling_timesteps(2, device='cpu', steps=STEPS))
    coefs = torch.stack([torch.stack(sch.ddim_coefficients(t, tn, eta)) for t, tn in pairs]).numpy()
    conds = torch.stack([sch.log_snr(t) for t, _ in pairs])
    al, sg = log_snr_to_alpha_sigma(conds)                          # the x0 conversion of the ancestral branch, as it forms it (fp32)
    x0c = torch.stack((1. / al.clamp(min=1e-8), -sg / al.clamp(min=1e-8)) if objective == 'noise' else (al, -sg), dim=1).numpy()
    lo, hi = (MIN_BOUND, None) if norm == 'z-score' else (-1.0, 1.0)
    ref_img, ref_noisy, ref_x0 = A.ddim_reference_loop(
        lambda x, ls: A.stub_net64(x, lowres.numpy(), ls), init.numpy(), [s.numpy() for s in steps], coefs, x0c, conds.numpy(), objective,
        lo, hi, dyn_q=imagen.dynamic_thresholding_percentile if dynamic else None, dyn_floor=1.0)
    got = [img.cpu().numpy()] + list(noisy) + list(x0)
    ref = [ref_img] + ref_noisy + ref_x0
    scale = max(np.abs(r).max() for r in ref)
    bound = STEPS * 8 * 2.0 ** -23 * scale
    worst = max(np.abs(g.astype(np.float64) - r).max() for g, r in zip(got, ref))
    print(f"ddim {kind} {objective} {mode} eta {eta}: max err {worst:.3e}, bound {bound:.3e}, max|x| {scale:.3e}")
    for g, r in zip(got, ref):
        assert g.shape == r.shape and np.isfinite(g).all()
        assert np.abs(g.astype(np.float64) - r).max() <= bound


def test_sample_steps_thins_the_ancestral_chain_too(draws):
    """``sample_steps`` with ``sampler='ddpm'``: the ancestral loop on linspace(1, 0, K + 1), one draw per step."""
    imagen = stub_imagen('cosine', 'x_start', 'z-score', False)
    kw = dict(batch_size=2, start_image_or_video=draws[0].to(DEV), start_at_unet_number=2, use_tqdm=False)
    a = imagen.sample(noise=draws[1:2 + STEPS], sample_steps=STEPS, **kw)
    assert len(a[1]) == STEPS + 1
    b = imagen.sample(noise=draws[1:2 + STEPS], sampler='ddim', eta=1.0, sample_steps=STEPS, **kw)
    close(b[0], a[0], 5e-4, "ddim(eta=1) vs ddpm on 6 steps")
    with pytest.raises(IndexError):                                  # the ancestral chain needs its draw per step
        imagen.sample(noise=draws[1:2], sample_steps=STEPS, **kw)


# ---- the tie to the reference-pinned ancestral path -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden_sampler():
    from diffusioniqt_amd.imagen_pytorch3D import Imagen, NullUnet
    g, gu = load_golden('ddpmA_traj'), load_golden('unetA_tiny')
    unet, _, _ = build(gu, 0)
    configs = {'Data': {'norm': 'z-score'}, 'Train': {'batch_sample': False, 'patch_size_sub': 8, 'pred_obj': 'x_start'}, 'Eval': {'repeat': 1}}
    imagen = Imagen(unets=(NullUnet(), unet), configs=configs, min_bound=float(g['min_bound']), image_sizes=(8, 8), channels=1,
                    pred_objectives='x_start', timesteps=int(g['T']), dynamic_thresholding=False, p2_loss_weight_gamma=0.0,
                    cond_drop_prob=0.0).to(DEV)
    noise = [T(g['init_noise'])] + list(T(g['step_noise']))
    kw = dict(batch_size=2, start_image_or_video=T(g['lowres']).to(DEV), start_at_unet_number=2, use_tqdm=False)
    return imagen, noise, kw, int(g['T']), imagen.sample(noise=noise, **kw)


def test_ddim_at_eta_one_reproduces_the_ancestral_trajectory(golden_sampler):
    imagen, noise, kw, steps, (img, noisy, x0) = golden_sampler
    d_img, d_noisy, d_x0 = imagen.sample(noise=noise, sampler='ddim', eta=1.0, **kw)
    close(d_img, img, 5e-4, "sample img")
    close(T(np.stack(d_noisy)), T(np.stack(noisy)), 5e-4, "noisy list")
    close(T(np.stack(d_x0)), T(np.stack(x0)), 5e-4, "x0 list")


def test_sample_steps_equal_to_the_schedule_is_the_default_call(golden_sampler):
    imagen, noise, kw, steps, (img, noisy, x0) = golden_sampler
    s_img, s_noisy, s_x0 = imagen.sample(noise=noise, sampler='ddpm', sample_steps=steps, **kw)
    assert torch.equal(s_img, img)
    assert all(np.array_equal(a, b) for a, b in zip(s_noisy, noisy)) and all(np.array_equal(a, b) for a, b in zip(s_x0, x0))


def test_callable_noise_is_the_list_of_what_it_returned(golden_sampler):
    imagen, _, kw, steps, _ = golden_sampler
    gen = torch.Generator(device=DEV).manual_seed(5)
    seen = []

    def source(shape):
        seen.append(torch.randn(shape, generator=gen, device=DEV))
        return seen[-1]
    for extra in (dict(), dict(sampler='ddim', eta=0.5, sample_steps=3), dict(sampler='ddim', sample_steps=3)):
        del seen[:]
        a = imagen.sample(noise=source, **extra, **kw)
        assert len(seen) == (1 if extra.get('sampler') == 'ddim' and not extra.get('eta') else 1 + extra.get('sample_steps', steps))
        b = imagen.sample(noise=[t.clone() for t in seen], **extra, **kw)
        assert torch.equal(a[0], b[0]) and all(np.array_equal(p, q) for p, q in zip(a[1], b[1]))


def test_anchored_noise_under_ddim_does_not_depend_on_the_batching(golden_sampler):
    """Four windows sampled at once and two by two, through ``ImagenTrainer.sample`` with ``AnchoredNoise.source``: the same patches."""
    from diffusioniqt_amd.inference import AnchoredNoise
    from diffusioniqt_amd.trainer import ImagenTrainer
    imagen = golden_sampler[0]
    ImagenTrainer.locked = False
    trainer = ImagenTrainer(configs=imagen.configs, imagen=imagen, verbose=False)
    origins = np.array([(0, 0, 0), (4, 4, 4), (4, 4, 8), (12, 16, 20)], dtype=np.int32)       # two of them overlap
    field = AnchoredNoise((20, 24, 28), seed=9)
    lowres = torch.randn(4, 1, 8, 8, 8, generator=torch.Generator().manual_seed(1)).to(DEV)

    def run(rows, **extra):
        out = trainer.sample(batch_size=len(rows), start_image_or_video=lowres[rows], start_at_unet_number=2,
                             noise=field.source(origins[rows], 8, sample=1), **extra)[0]
        assert tuple(out.shape) == (len(rows), 1, 8, 8, 8)
        return out
    for extra in (dict(sampler='ddim', sample_steps=3), dict(sampler='ddim', sample_steps=3, eta=0.5)):
        whole = run([0, 1, 2, 3], **extra)
        assert torch.equal(torch.cat((run([0, 1], **extra), run([2, 3], **extra))), whole), extra
        assert torch.equal(torch.cat((run([2, 3], **extra), run([0, 1], **extra)))[[2, 3, 0, 1]], whole), extra
