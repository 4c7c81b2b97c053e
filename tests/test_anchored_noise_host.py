"""Host-side checks of the volume-anchored noise specification and of the few-step sampler's coefficients and argument rules: the
numpy Philox of tests/anchored_noise_reference.py against Random123's known answers, the statistics of the reference normals, window
consistency, ``GaussianDiffusionContinuousTimes.ddim_coefficients`` against its float64 closed form and, at eta = 1, against the
ancestral ``posterior_coefficients``, and every argument error raised before anything touches the device (no GPU here)."""
import numpy as np
import pytest
import torch

from tests import anchored_noise_reference as A
from tests import volume_blend_reference as R


def _hex(words):
    return ' '.join(f'{int(w):08x}' for w in words)


@pytest.mark.parametrize('counter, key, out', [
    ((0, 0, 0, 0), (0, 0), '6627e8d5 e169c58d bc57ac4c 9b00dbd8'),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, '408f276d 41c83b0e a20bc7c6 6d5451fd'),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), 'd16cfe09 94fdcceb 5001e420 24126ea1'),
])
def test_philox_known_answers(counter, key, out):
    """Random123's kat_vectors for philox4x32-10."""
    assert _hex(A.philox4x32_10(counter, key)) == out


def test_field_uses_the_documented_counter_and_key():
    seed = 0x123456789
    bits = A.field((3, 4, 5), 2, seed, draw=3, sample=2)
    c, z, y, x = 1, 2, 3, 4
    lin = ((c * 3 + z) * 4 + y) * 5 + x
    r = A.philox4x32_10((lin, 0, 3, 2), (seed & 0xffffffff, seed >> 32))
    assert [int(v) for v in bits[c, z, y, x]] == [int(r[0]), int(r[1])]
    big = (1 << 33) + 5                                                     # the high counter word
    r = A.philox4x32_10((5, 2, 0, 0), (0, 0))
    assert [int(v) for v in A.field_at(np.array([big], dtype=np.uint64), 0, 0, 0)[0]] == [int(r[0]), int(r[1])]
    lin = A.window_lin((2048, 2048, 2048), (2040, 2040, 2040), 8)
    assert int(lin.min()) > 1 << 32 and int(lin[0, 7, 7, 7]) == 2048 ** 3 - 1


def test_reference_normals_moments():
    """64^3 normals (N = 262144) at five standard errors: mean, variance, lag-1 correlation along each axis."""
    n = A.normals(A.field((64, 64, 64), 1, 7, 0, 0))[0]
    N = n.size
    se = 1.0 / np.sqrt(N)
    assert np.isfinite(n).all()
    assert abs(n.mean()) <= 5 * se, n.mean()
    assert abs(n.var() - 1.0) <= 5 * np.sqrt(2.0 / N), n.var()
    for axis in range(3):
        a = np.take(n, range(0, 63), axis=axis).ravel()
        b = np.take(n, range(1, 64), axis=axis).ravel()
        assert abs(np.corrcoef(a, b)[0, 1]) <= 5 * se, (axis, np.corrcoef(a, b)[0, 1])


def test_reference_windows_agree_on_their_overlap_and_fields_differ():
    shape, P, seed = (20, 24, 28), 8, 0x123456789
    f = A.field(shape, 1, seed, 3, 2)
    a, b = A.window(f, (3, 5, 7), P), A.window(f, (3, 5, 9), P)
    assert np.array_equal(a[:, :, :, 2:], b[:, :, :, :6])
    for o in ((3, 5, 7), (12, 16, 20)):                                     # the per-window index arithmetic against the whole field
        assert np.array_equal(A.field_at(A.window_lin(shape, o, P), seed, 3, 2), A.window(f, o, P))
    for other in (A.field(shape, 1, seed, 4, 2), A.field(shape, 1, seed, 3, 1), A.field(shape, 1, seed + 1, 3, 2),
                  A.field(shape, 1, seed + (1 << 32), 3, 2)):
        assert (other != f).mean() > 0.99


# ---- ddim_coefficients ---------------------------------------------------------------------------------------------------------------
def _schedule(kind, steps):
    from diffusioniqt_amd.imagen_pytorch3D import GaussianDiffusionContinuousTimes
    sch = GaussianDiffusionContinuousTimes(noise_schedule=kind, timesteps=1000)
    return sch, list(sch.get_sampling_timesteps(2, device='cpu', steps=steps))


def test_sampling_timesteps_take_a_step_count():
    from diffusioniqt_amd.imagen_pytorch3D import GaussianDiffusionContinuousTimes
    sch = GaussianDiffusionContinuousTimes(noise_schedule='cosine', timesteps=12)
    default = list(sch.get_sampling_timesteps(3, device='cpu'))
    same = list(sch.get_sampling_timesteps(3, device='cpu', steps=12))
    assert len(default) == 12 and all(torch.equal(a, b) for a, b in zip(default, same))
    few = list(sch.get_sampling_timesteps(3, device='cpu', steps=5))
    grid = torch.linspace(1., 0., 6)
    assert len(few) == 5 and few[0].shape == (2, 3)
    for i, pair in enumerate(few):
        assert torch.equal(pair[0], grid[i].expand(3)) and torch.equal(pair[1], grid[i + 1].expand(3))


@pytest.mark.parametrize('kind', ['cosine', 'linear'])
@pytest.mark.parametrize('steps', [50, 8])
@pytest.mark.parametrize('eta', [0.0, 0.5, 1.0])
def test_ddim_coefficients_equal_the_float64_closed_form(kind, steps, eta):
    sch, pairs = _schedule(kind, steps)
    for i, (t, tn) in enumerate(pairs):
        got = sch.ddim_coefficients(t, tn, eta)
        ref = A.ddim_coefficients64(sch.log_snr(t).numpy(), sch.log_snr(tn).numpy(), (tn == 0).numpy(), eta)
        for g, r, name in zip(got, ref, ('kx', 'k0', 'kn')):
            assert g.dtype == torch.float32 and g.shape == (2,)
            assert np.array_equal(g.numpy(), r.astype(np.float32)), (name, i, g.numpy(), r)
        if i == len(pairs) - 1:
            assert (got[2] == 0).all()                                      # no noise enters the last step
        if eta == 0:
            assert (got[2] == 0).all()
            _, sigma = A.alpha_sigma64(sch.log_snr(t).numpy())
            _, sigma_next = A.alpha_sigma64(sch.log_snr(tn).numpy())
            assert np.all(np.abs(got[0].numpy().astype(np.float64) * sigma - sigma_next) <= 2.0 ** -23 * sigma_next)


@pytest.mark.parametrize('kind', ['cosine', 'linear'])
@pytest.mark.parametrize('steps', [50, 8])
def test_ddim_at_eta_one_is_the_ancestral_posterior(kind, steps):
    """Every coefficient within 1e-5 of the step's largest coefficient (the residual is the fp32 expm1 cancellation of
    ``posterior_coefficients``)."""
    sch, pairs = _schedule(kind, steps)
    worst = 0.0
    for t, tn in pairs:
        got = torch.stack(sch.ddim_coefficients(t, tn, 1.0)).double()
        ref = torch.stack(sch.posterior_coefficients(t, tn)).double()
        err = ((got - ref).abs().max() / ref.abs().max()).item()
        worst = max(worst, err)
        assert err <= 1e-5, (kind, steps, err)
    print(f"ddim(eta=1) vs posterior, {kind} {steps} steps: {worst:.3e} of the largest coefficient")


# ---- argument errors: all before the device is touched --------------------------------------------------------------------------------
def _imagen():
    from diffusioniqt_amd.imagen_pytorch3D import Imagen, NullUnet
    configs = {'Data': {'norm': 'z-score'}, 'Train': {'batch_sample': False}}
    return Imagen(unets=(NullUnet(), A.make_stub_unet()), configs=configs, min_bound=-0.75, image_sizes=(8, 8), channels=1,
                  pred_objectives='x_start', timesteps=4, dynamic_thresholding=False, p2_loss_weight_gamma=0.0, cond_drop_prob=0.0)


def test_sampler_argument_errors():
    imagen = _imagen()
    lr = torch.zeros(2, 1, 8, 8, 8)
    kw = dict(batch_size=2, start_image_or_video=lr, start_at_unet_number=2, use_tqdm=False)
    with pytest.raises(ValueError, match="sample_steps and skip_steps"):
        imagen.sample(sample_steps=2, skip_steps=2, **kw)
    with pytest.raises(ValueError, match="sample_steps"):
        imagen.sample(sample_steps=0, **kw)
    for eta in (-0.1, 1.5):
        with pytest.raises(ValueError, match="eta"):
            imagen.sample(sampler='ddim', eta=eta, **kw)
    with pytest.raises(ValueError, match="inpaint"):
        imagen.sample(sampler='ddim', inpaint_images=lr, inpaint_masks=lr.bool(), **kw)
    with pytest.raises(ValueError, match="sampler"):
        imagen.sample(sampler='heun', **kw)
    sch = imagen.noise_schedulers[1]
    with pytest.raises(ValueError, match="sampler"):                         # the loop itself applies the same rules
        imagen.p_sample_loop(imagen.unets[1], (2, 1, 8, 8, 8), noise_scheduler=sch, lowres_cond_img=lr, sampler='euler')
    with pytest.raises(ValueError, match="sample_steps and skip_steps"):
        imagen.p_sample_loop(imagen.unets[1], (2, 1, 8, 8, 8), noise_scheduler=sch, lowres_cond_img=lr, sample_steps=2, skip_steps=2)


def test_anchored_noise_argument_errors():
    from diffusioniqt_amd import ops
    from diffusioniqt_amd.inference import AnchoredNoise, VolumeInference, sub_volume_origins

    def never(x, noise=None):
        raise AssertionError("the sampler must not run")
    with pytest.raises(ValueError, match="noise"):
        VolumeInference(R.shared_cfg(8), never, noise='window')
    inf = VolumeInference(R.shared_cfg(8), never)
    assert inf.noise is None and inf.seed == 0                               # the default is today's path
    for origin in ((13, 0, 0), (0, 17, 0), (0, 0, 21), (-1, 0, 0)):
        with pytest.raises(ValueError, match="leaves the volume"):
            ops.anchored_noise(np.array([[0, 0, 0], origin], dtype=np.int32), 1, 8, 20, 24, 28, seed=0)
    with pytest.raises(ValueError, match="leaves the volume"):
        AnchoredNoise((20, 24, 28), seed=1).source(np.array([[12, 16, 21]]), 8)((1, 1, 8, 8, 8))
    with pytest.raises(ValueError, match="origins"):
        ops.anchored_noise(np.zeros((2, 2), dtype=np.int32), 1, 8, 20, 24, 28, seed=0)
    with pytest.raises(ValueError, match="seed"):
        ops.anchored_noise(np.zeros((1, 3), dtype=np.int32), 1, 8, 20, 24, 28, seed=1 << 64)
    with pytest.raises(AssertionError, match="asked for"):
        AnchoredNoise((20, 24, 28)).source(np.zeros((2, 3), dtype=np.int32), 8)((3, 1, 8, 8, 8))
    # block mode: the sub-volume origins follow convertVolume2subVolume, n = b2 + f b3 + f^2 b4
    sub = sub_volume_origins((1, 2, 3), 3, 8)
    assert sub.shape == (27, 3) and sub[1].tolist() == [9, 2, 3] and sub[3].tolist() == [1, 10, 3] and sub[9].tolist() == [1, 2, 11]


def test_anchored_noise_entry_returns_error_codes():
    from diffusioniqt_amd import _lib
    lib = _lib.load()
    assert lib.diqt_anchored_noise(None, 1, 1, 8, 20, 24, 28, 0, 0, 0, 0, None, None) == -2       # DIQT_E_ALIGN
    assert b"null pointer" in lib.diqt_last_error()
    buf = (np.zeros(4, dtype=np.int32)).ctypes.data                                                 # never dereferenced: the shape is refused
    assert lib.diqt_anchored_noise(buf, 0, 1, 8, 20, 24, 28, 0, 0, 0, 0, buf, None) == -1         # DIQT_E_SHAPE
    assert lib.diqt_anchored_noise(buf, 1, 1, 0, 20, 24, 28, 0, 0, 0, 0, buf, None) == -1
    assert lib.diqt_anchored_noise(buf, 1, 1, 32, 20, 24, 28, 0, 0, 0, 0, buf, None) == -1        # a window larger than the volume
    assert lib.diqt_anchored_noise(buf, 1, 1, 8, 20, 24, 28, 0, 0, 0, 2, buf, None) == -3         # DIQT_E_UNSUPPORTED
