"""Host-side checks of the lockstep joint sampling of overlapping windows (no GPU here): the float64 specification of
tests/volume_joint_reference.py does not depend on the tiling when the network is elementwise, every argument rule of
``Imagen.window_denoiser`` and ``VolumeInference(joint=True)`` is raised before anything touches the device, and the two C entries
return error codes for null pointers and bad lattices."""
import itertools

import numpy as np
import pytest
import torch

from tests import anchored_noise_reference as A
from tests import volume_blend_reference as R
from tests import volume_joint_reference as J


def _imagen(norm='z-score', dynamic=False, objective='x_start'):
    from diffusioniqt_amd.imagen_pytorch3D import Imagen, NullUnet
    configs = {'Data': {'norm': norm}, 'Train': {'batch_sample': False}}
    return Imagen(unets=(NullUnet(), A.make_stub_unet()), configs=configs, min_bound=J.MIN_BOUND, image_sizes=(16, 16), channels=1,
                  pred_objectives=objective, noise_schedules=('cosine', 'cosine'), dynamic_thresholding=dynamic,
                  p2_loss_weight_gamma=0.0, cond_drop_prob=0.0)


# ---- H1: the reference alone ------------------------------------------------------------------------------------------------------------
def test_reference_chain_does_not_depend_on_the_tiling():
    """Stub network (elementwise), static clamp, eta = 0.5: every window predicts the same x0 at a voxel, so the fused x0 is that
    number whatever the stride and the weights, and the float64 chains of strides 16 / 8 / 5 x constant / gaussian agree on the voxels
    covered under all six and not background.  Measured with these inputs: share 0.1576, largest difference 2.2e-15."""
    from diffusioniqt_amd.imagen_pytorch3D import GaussianDiffusionContinuousTimes
    vol = R.shared_volume()
    tabs = J.tables(GaussianDiffusionContinuousTimes(noise_schedule='cosine', timesteps=1000), J.STEPS, 0.5, 'x_start')
    assert (tabs[0][:-1, 2] > 0).all() and tabs[0][-1, 2] == 0                # noise enters every step but the last
    den = _imagen().window_denoiser(sampler='ddim', sample_steps=J.STEPS, eta=0.5)
    assert np.array_equal(den.coefs.numpy().astype(np.float64), tabs[0])        # the chain below runs on the denoiser's own table
    refs = {(stride, kind): J.joint_reference(vol, R.shared_cfg(stride), J.stub64, tabs, 'x_start', (J.MIN_BOUND, 0., 0), kind)
            for stride in (16, 8, 5) for kind in ('constant', 'gaussian')}
    common = np.logical_and.reduce([r['covered'] & ~r['background'] for r in refs.values()])
    share = common.mean()
    worst = max(np.abs(a['mean'] - b['mean'])[common].max() for a, b in itertools.combinations(refs.values(), 2))
    print(f"joint reference, 6 tilings: common share {share:.4f}, largest difference {worst:.3e}")
    assert share >= 0.15
    assert worst <= 1e-12
    assert any(r['kept'] < r['candidates'] for r in refs.values())              # the 5 % rule drops windows: -1 slots
    assert np.ptp(refs[(8, 'gaussian')]['mean'][common]) > 0.1                  # and the compared values are not one constant


# ---- H2: argument rules, all before the device is touched ---------------------------------------------------------------------------------
def test_window_denoiser_argument_errors_and_host_tables():
    imagen = _imagen()
    lr = torch.zeros(2, 1, 16, 16, 16)
    with pytest.raises(ValueError, match="sampler"):
        imagen.window_denoiser(sampler='heun')
    with pytest.raises(ValueError, match="sample_steps"):
        imagen.window_denoiser(sample_steps=0)
    for eta in (-0.1, 1.5):
        with pytest.raises(ValueError, match="eta"):
            imagen.window_denoiser(sampler='ddim', eta=eta)
    for sampler in ('ddim', 'ddpm'):
        with pytest.raises(ValueError, match="inpaint"):
            imagen.window_denoiser(sampler=sampler, inpaint_images=lr, inpaint_masks=lr.bool())
    with pytest.raises(ValueError, match="init_images"):
        imagen.window_denoiser(init_images=lr)
    with pytest.raises(ValueError, match="skip_steps"):
        imagen.window_denoiser(skip_steps=2)
    with pytest.raises(ValueError, match="skip_steps"):
        imagen.window_denoiser(sample_steps=4, skip_steps=2)
    with pytest.raises(ValueError, match="unet_number"):
        imagen.window_denoiser(unet_number=3)
    with pytest.raises(ValueError, match="null"):
        imagen.window_denoiser(unet_number=1)
    sch = imagen.noise_schedulers[1]
    for sampler, eta in (('ddim', 0.0), ('ddim', 0.5), ('ddpm', 0.0)):
        d = imagen.window_denoiser(sampler=sampler, sample_steps=J.STEPS, eta=eta)
        assert d.num_steps == J.STEPS and d.coefs.dtype == torch.float32 and tuple(d.coefs.shape) == (J.STEPS, 3) and not d.coefs.is_cuda
        pairs = list(sch.get_sampling_timesteps(1, device='cpu', steps=J.STEPS))
        want = [sch.ddim_coefficients(t, tn, eta) if sampler == 'ddim' else sch.posterior_coefficients(t, tn) for t, tn in pairs]
        assert torch.equal(d.coefs, torch.stack([torch.stack(w)[:, 0] for w in want]))
        assert d.clamp == (J.MIN_BOUND, 0., 0) and not d.self_cond
        with pytest.raises(ValueError, match="step"):
            d.x0(lr, lr, J.STEPS)
    assert imagen.window_denoiser(sample_steps=None).num_steps == 1000          # the schedule's own chain
    assert _imagen('min-max').window_denoiser(sample_steps=2).clamp == (-1., 1., 1)
    assert _imagen('min-max', dynamic=True).window_denoiser(sample_steps=2).clamp == (-float('inf'), float('inf'), 1)


def test_trainer_window_denoiser_applies_the_same_rules():
    from diffusioniqt_amd.trainer import ImagenTrainer
    assert callable(getattr(ImagenTrainer, 'window_denoiser'))
    imagen = _imagen()
    imagen.configs = {'Data': {'norm': 'z-score'}, 'Train': {'batch_sample': False, 'patch_size_sub': 16, 'pred_obj': 'x_start'},
                      'Eval': {'repeat': 1}}
    ImagenTrainer.locked = False
    trainer = ImagenTrainer(configs=imagen.configs, imagen=imagen, verbose=False)
    with pytest.raises(ValueError, match="skip_steps"):
        trainer.window_denoiser(skip_steps=2)
    with pytest.raises(ValueError, match="eta"):
        trainer.window_denoiser(sampler='ddim', eta=2.0)
    for kw in (dict(), dict(use_non_ema=True)):
        assert trainer.window_denoiser(sampler='ddim', sample_steps=3, **kw).num_steps == 3


class _NeverDenoiser:
    """A window denoiser's attributes; nothing of it may run in these tests."""
    num_steps, coefs, clamp, self_cond = 1, torch.zeros(1, 3), (0., 0., 0), False

    def x0(self, *a, **k):
        raise AssertionError("the denoiser must not run")
    finish = x0


def test_volume_inference_joint_argument_errors():
    from diffusioniqt_amd.inference import VolumeInference

    def never(x, noise=None):
        raise AssertionError("the sampler must not run")
    cfg = R.shared_cfg(8)
    for kw in (dict(blend=None, noise='anchored'), dict(blend='gaussian', noise=None), dict()):
        with pytest.raises(ValueError, match="joint"):
            VolumeInference(cfg, _NeverDenoiser(), joint=True, **kw)
    with pytest.raises(ValueError, match="window denoiser"):
        VolumeInference(cfg, never, blend='gaussian', noise='anchored', joint=True)
    with pytest.raises(ValueError, match="samples"):
        VolumeInference(cfg, _NeverDenoiser(), blend='gaussian', noise='anchored', joint=True, samples=0)
    assert VolumeInference(cfg, never).joint is False                           # the default is today's path
    inf = VolumeInference(cfg, _NeverDenoiser(), blend='gaussian', noise='anchored', joint=True, seed=3)
    assert inf.joint and inf.seed == 3
    vol = torch.zeros(40, 36, 44)
    with pytest.raises(NotImplementedError, match="ranks"):
        inf(vol, patch_slice=(0, 2))
    with pytest.raises(ValueError, match="return_std"):
        inf(vol, return_std=True)                                               # samples == 1


# ---- H3: error codes of the two entries --------------------------------------------------------------------------------------------------
def test_joint_entries_return_error_codes():
    from diffusioniqt_amd import _lib
    lib = _lib.load()
    buf = (np.zeros(4, dtype=np.int32)).ctypes.data                             # never dereferenced: every call below is refused
    geo = (40, 36, 44, 16, 8, 4, 3, 4)                                          # D, H, W, P, stride and the lattice of range(0, n - 15, 8)
    step = lambda y, slot, taps, x_t, x_next, geo=geo, mode=0: lib.diqt_volume_joint_step(
        y, slot, taps, x_t, x_next, None, 3, *geo, 1.0, 0.5, 0.0, -1.0, 1.0, mode, 0, 1, 0, None)
    assert step(buf, buf, buf, buf, None) == -2                                 # DIQT_E_ALIGN
    assert b"null pointer" in lib.diqt_last_error()
    assert step(None, buf, buf, buf, buf) == -2
    assert step(buf, None, buf, buf, buf) == -2
    assert step(buf, buf, None, buf, buf) == -2
    assert step(buf, buf, buf, buf, buf, geo=(40, 36, 44, 16, 8, 4, 3, 5)) == -1   # DIQT_E_SHAPE: not the lattice
    assert b"lattice" in lib.diqt_last_error()
    assert step(buf, buf, buf, buf, buf, geo=(40, 36, 44, 16, 0, 4, 3, 4)) == -1
    assert step(buf, buf, buf, buf, buf, geo=(40, 36, 44, 48, 8, 1, 1, 1)) == -1   # a window larger than the volume
    assert step(None, None, None, None, buf, geo=(0, 36, 44, 0, 0, 0, 0, 0)) == -1  # the initial state still needs a volume
    assert step(buf, buf, buf, buf, buf, mode=2) == -3                          # DIQT_E_UNSUPPORTED
    fin = lambda x, slot, mean_io, m2=None, std=None, s=0, S=1, geo=geo: lib.diqt_volume_joint_finish(
        x, slot, None, mean_io, m2, std, s, S, *geo, 300.0, 200.0, -1.5, -1.5, None)
    assert fin(None, buf, buf) == -2
    assert b"null pointer" in lib.diqt_last_error()
    assert fin(buf, None, buf) == -2
    assert fin(buf, buf, None) == -2
    assert fin(buf, buf, buf, geo=(40, 36, 44, 16, 8, 4, 4, 4)) == -1
    assert b"lattice" in lib.diqt_last_error()
    assert fin(buf, buf, buf, s=1, S=1) == -1                                   # sample 1 of 1
    assert fin(buf, buf, buf, m2=buf) == -1                                     # m2_io / out_std are NULL for S = 1
    assert fin(buf, buf, buf, std=buf, s=1, S=2) == -1                          # a deviation map needs m2_io
