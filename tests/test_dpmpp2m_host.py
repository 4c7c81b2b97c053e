"""Host-side checks of the second-order multistep sampler ``sampler='dpmpp2m'`` (no GPU here): the coefficient table against the
float64 formulas of tests/dpmpp2m_reference.py, its accuracy against DDIM on an analytic problem, every argument rule raised before
anything touches the device, the error codes of ``diqt_volume_joint_multistep``, and the float64 joint chain's independence of the
tiling."""
import itertools

import numpy as np
import pytest
import torch

from tests import anchored_noise_reference as A
from tests import dpmpp2m_reference as M
from tests import volume_blend_reference as R
from tests import volume_joint_reference as J


def _scheduler(kind):
    from diffusioniqt_amd.imagen_pytorch3D import GaussianDiffusionContinuousTimes
    return GaussianDiffusionContinuousTimes(noise_schedule=kind, timesteps=1000)


def _pairs(sch, K, batch=1):
    return list(sch.get_sampling_timesteps(batch, device='cpu', steps=K))


def _ddim_table(sch, K):
    return torch.stack([torch.stack(sch.ddim_coefficients(t, tn, 0.)) for t, tn in _pairs(sch, K)])


# ---- the table ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K', [1, 2, 3, 6])
@pytest.mark.parametrize('kind', ['cosine', 'linear'])
def test_table_matches_the_float64_formulas(kind, K):
    from diffusioniqt_amd.imagen_pytorch3D import Imagen
    sch = _scheduler(kind)
    got = sch.dpmpp2m_coefficients(_pairs(sch, K, batch=2))
    assert got.dtype == torch.float32 and tuple(got.shape) == (K, 3, 2) and torch.equal(got[:, :, 0], got[:, :, 1])
    assert torch.equal(Imagen._sampler_tables(sch, 2, 'dpmpp2m', K, None, 0., 'noise')[0], got)
    want, k01 = M.table64(*M.chain_log_snr(sch, K))
    err = np.abs(got[:, :, 0].numpy().astype(np.float64) - want)
    print(f"dpmpp2m table {kind} K {K}: max error {err.max():.3e}, c {M.amplification(want, k01):.3f}")
    assert (err <= 2.0 ** -23 * np.maximum(1.0, np.abs(want))).all()
    # the first step and the first-order last step are the DDIM rows, bit for bit, with no history term
    ddim = _ddim_table(sch, K)[:, :, 0]
    for i in {0, K - 1}:
        assert torch.equal(got[i, :2, 0], ddim[i, :2]) and got[i, 2, 0] == 0
    # k0 + kp = the DDIM k0: a constant x0 makes every step first-order
    k0, kp, d = (v.numpy().astype(np.float64) for v in (got[:, 1, 0], got[:, 2, 0], ddim[:, 1]))
    ulp = np.spacing(np.abs(ddim[:, 1].numpy())).astype(np.float64)
    assert (np.abs(k0 + kp - d) <= 2 * ulp).all(), (np.abs(k0 + kp - d) / ulp).max()
    if K > 2:
        assert (got[1:K - 1, 2, 0] < 0).all() and (got[1:K - 1, 1, 0] > ddim[1:K - 1, 1]).all()


# ---- accuracy, on the product's own table -----------------------------------------------------------------------------------------------
def _errors(kind, K):
    sch = _scheduler(kind)
    ls, lsn = M.chain_log_snr(sch, K)
    two_m = sch.dpmpp2m_coefficients(_pairs(sch, K)).numpy()[:, :, 0].astype(np.float64)
    ddim = _ddim_table(sch, K).numpy()[:, :, 0].astype(np.float64)
    return M.gaussian_problem_error(ddim, ls, lsn), M.gaussian_problem_error(two_m, ls, lsn)


def test_second_order_accuracy_on_the_gaussian_problem():
    """Gaussian data (s = 0.5), exact linear predictor, closed-form probability-flow ODE (tests/dpmpp2m_reference.py).  Measured with
    the product's table -- cosine, K = 8 / 12 / 16 / 20: DDIM 8.6e-2 / 5.9e-2 / 4.5e-2 / 3.6e-2, 2M 3.8e-2 / 1.1e-2 / 2.8e-3 / 3.0e-4
    (ratios 0.45, 0.19, 0.06, 0.008); DDIM at K = 50: 1.5e-2; linear: ratios 0.81, 0.57, 0.37, 0.21."""
    for K in (8, 12, 16, 20):
        d, m = _errors('cosine', K)
        print(f"cosine K {K}: ddim {d:.3e}, dpmpp2m {m:.3e}, ratio {m / d:.3f}")
        assert m <= 0.5 * d
    d50, _ = _errors('cosine', 50)
    _, m16 = _errors('cosine', 16)
    print(f"cosine: dpmpp2m at 16 steps {m16:.3e}, ddim at 50 steps {d50:.3e}")
    assert m16 < d50
    for K in (8, 12, 16, 20):
        d, m = _errors('linear', K)
        print(f"linear K {K}: ddim {d:.3e}, dpmpp2m {m:.3e}, ratio {m / d:.3f}")
        assert m < d


# ---- argument rules, all before the device is touched -------------------------------------------------------------------------------------
class _NeverUnet(torch.nn.Module):
    lowres_cond = True
    self_cond = False

    def cast_model_parameters(self, **kwargs):
        return self

    def forward_with_cond_scale(self, *args, **kwargs):
        raise AssertionError("the U-Net must not run")


def _imagen(unet=None):
    from diffusioniqt_amd.imagen_pytorch3D import Imagen, NullUnet
    configs = {'Data': {'norm': 'z-score'}, 'Train': {'batch_sample': False, 'patch_size_sub': 16, 'pred_obj': 'x_start'},
               'Eval': {'repeat': 1}}
    return Imagen(unets=(NullUnet(), unet if unet is not None else _NeverUnet()), configs=configs, min_bound=J.MIN_BOUND,
                  image_sizes=(16, 16), channels=1, pred_objectives='x_start', noise_schedules=('cosine', 'cosine'),
                  dynamic_thresholding=False, p2_loss_weight_gamma=0.0, cond_drop_prob=0.0)


def _bad_arguments():
    lr = torch.zeros(2, 1, 16, 16, 16)
    return [("eta", dict(eta=0.5)), ("skip_steps", dict(skip_steps=2)), ("skip_steps", dict(sample_steps=4, skip_steps=2)),
            ("inpaint", dict(inpaint_images=lr, inpaint_masks=lr.bool()))]


def test_argument_rules_raise_before_the_device_is_touched():
    from diffusioniqt_amd.trainer import ImagenTrainer
    imagen = _imagen()
    ImagenTrainer.locked = False
    trainer = ImagenTrainer(configs=imagen.configs, imagen=imagen, verbose=False)
    lr = torch.zeros(2, 1, 16, 16, 16)
    for match, kw in _bad_arguments():
        with pytest.raises(ValueError, match=match):
            imagen.sample(batch_size=2, start_image_or_video=lr, start_at_unet_number=2, use_tqdm=False, sampler='dpmpp2m', **kw)
        with pytest.raises(ValueError, match=match):
            imagen.p_sample_loop(imagen.unets[1], (2, 1, 16, 16, 16), noise_scheduler=imagen.noise_schedulers[1], lowres_cond_img=lr,
                                 pred_objective='x_start', dynamic_threshold=False, use_tqdm=False, sampler='dpmpp2m', **kw)
        with pytest.raises(ValueError, match=match):
            imagen.window_denoiser(sampler='dpmpp2m', **kw)
        with pytest.raises(ValueError, match=match):
            trainer.window_denoiser(sampler='dpmpp2m', **kw)
    for sampler in ('euler', 'heun', 'dpmpp2s'):                                # an unknown sampler is still refused
        with pytest.raises(ValueError, match="sampler"):
            imagen.window_denoiser(sampler=sampler)
    with pytest.raises(ValueError, match="sample_steps"):
        imagen.window_denoiser(sampler='dpmpp2m', sample_steps=0)


def test_window_denoiser_host_tables():
    imagen = _imagen()
    sch = imagen.noise_schedulers[1]
    den = imagen.window_denoiser(sampler='dpmpp2m', sample_steps=6)
    assert den.multistep is True and den.num_steps == 6
    assert den.coefs.dtype == torch.float32 and tuple(den.coefs.shape) == (6, 3) and not den.coefs.is_cuda
    assert torch.equal(den.coefs, sch.dpmpp2m_coefficients(_pairs(sch, 6))[:, :, 0])
    assert den.clamp == (J.MIN_BOUND, 0., 0) and not den.self_cond
    for sampler in ('ddim', 'ddpm'):
        assert imagen.window_denoiser(sampler=sampler, sample_steps=3).multistep is False
    assert imagen.window_denoiser(sampler='dpmpp2m').num_steps == 1000


# ---- error codes of the entry ----------------------------------------------------------------------------------------------------------
def test_multistep_entry_returns_error_codes():
    from diffusioniqt_amd import _lib
    lib = _lib.load()
    buf = (np.zeros(4, dtype=np.int32)).ctypes.data                             # never dereferenced: every call below is refused
    geo = (40, 36, 44, 16, 8, 4, 3, 4)                                          # D, H, W, P, stride and the lattice of range(0, n - 15, 8)
    step = lambda y, slot, taps, x_t, x_next, x0_out, prev=None, geo=geo, mode=0: lib.diqt_volume_joint_multistep(
        y, slot, taps, x_t, prev, x_next, x0_out, 3, *geo, 1.0, 0.5, -0.25, -1.0, 1.0, mode, None)
    assert step(None, buf, buf, buf, buf, buf) == -2                            # DIQT_E_ALIGN
    assert b"null pointer" in lib.diqt_last_error()
    assert step(buf, None, buf, buf, buf, buf) == -2
    assert step(buf, buf, None, buf, buf, buf) == -2
    assert step(buf, buf, buf, None, buf, buf) == -2                            # no initial-state mode: x_t is required ...
    assert step(buf, buf, buf, buf, None, buf) == -2
    assert step(buf, buf, buf, buf, buf, None) == -2                            # ... and so is x0_out
    assert step(buf, buf, buf, buf, buf, None, prev=buf) == -2
    assert step(buf, buf, buf, buf, buf, buf, geo=(40, 36, 44, 16, 8, 4, 3, 5)) == -1   # DIQT_E_SHAPE: not the lattice
    assert b"lattice" in lib.diqt_last_error()
    assert step(buf, buf, buf, buf, buf, buf, geo=(40, 36, 44, 16, 0, 4, 3, 4)) == -1
    assert step(buf, buf, buf, buf, buf, buf, geo=(40, 36, 44, 48, 8, 1, 1, 1)) == -1   # a window larger than the volume
    assert step(buf, buf, buf, buf, buf, buf, geo=(0, 36, 44, 16, 8, 4, 3, 4)) == -1
    assert step(buf, buf, buf, buf, buf, buf, mode=2) == -3                     # DIQT_E_UNSUPPORTED
    assert step(buf, buf, buf, buf, buf, buf, prev=buf, mode=-1) == -3


# ---- the reference alone ------------------------------------------------------------------------------------------------------------------
def test_reference_chain_does_not_depend_on_the_tiling():
    """Stub network (elementwise), static clamp: every window predicts the same x0 at a voxel, so the fused x0 -- and with it the history
    term -- is that number whatever the stride and the weights, and the float64 multistep chains of strides 16 / 8 / 5 x constant /
    gaussian agree on the voxels covered under all six and not background (share 0.1576: geometry only)."""
    vol = R.shared_volume()
    sch = _scheduler('cosine')
    tabs = M.tables(sch, M.STEPS, 'x_start')
    assert (tabs[0][1:-1, 2] < 0).all() and tabs[0][0, 2] == 0 and tabs[0][-1, 2] == 0      # two second-order steps
    den = _imagen(A.make_stub_unet()).window_denoiser(sampler='dpmpp2m', sample_steps=M.STEPS)
    assert np.array_equal(den.coefs.numpy().astype(np.float64), tabs[0])        # the chain below runs on the denoiser's own table
    refs = {(stride, kind): M.joint_reference(vol, R.shared_cfg(stride), J.stub64, tabs, 'x_start', (J.MIN_BOUND, 0., 0), kind)
            for stride in (16, 8, 5) for kind in ('constant', 'gaussian')}
    common = np.logical_and.reduce([r['covered'] & ~r['background'] for r in refs.values()])
    share = common.mean()
    worst = max(np.abs(a['mean'] - b['mean'])[common].max() for a, b in itertools.combinations(refs.values(), 2))
    print(f"joint multistep reference, 6 tilings: common share {share:.4f}, largest difference {worst:.3e}")
    assert share >= 0.15
    assert worst <= 1e-12
    assert any(r['kept'] < r['candidates'] for r in refs.values())              # the 5 % rule drops windows: -1 slots
    assert np.ptp(refs[(8, 'gaussian')]['mean'][common]) > 0.1                  # and the compared values are not one constant
    ddim = J.joint_reference(vol, R.shared_cfg(8), J.stub64, J.tables(sch, M.STEPS, 0.0, 'x_start'), 'x_start', (J.MIN_BOUND, 0., 0),
                             'gaussian')
    assert np.abs(ddim['mean'] - refs[(8, 'gaussian')]['mean'])[common].max() > 1e-3     # the history term is visible
