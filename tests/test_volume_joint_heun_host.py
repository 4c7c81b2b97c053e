"""Host-side checks of the EDM volume path (no GPU here): the float64 specification of tests/volume_joint_heun_reference.py does not
depend on the tiling when the network is elementwise, its derived bound dominates an fp32 emulation of the same chain and is small
beside the signal, the specification equals the fixture-pinned oracle's ``edm_sample`` run per window at stride = patch, the host
tables of ``ElucidatedImagen.window_denoiser`` are ``one_unet_sample``'s expressions, every argument rule is raised before anything
touches the device, and ``diqt_volume_joint_heun`` returns error codes for null pointers, bad lattices and a bad phase."""
import itertools

import numpy as np
import pytest
import torch

from tests import volume_blend_reference as R
from tests import volume_joint_heun_reference as HN
from tests import volume_joint_reference as J

CASES = [(dynamic, churn, tiling) for dynamic in (False, True) for churn in HN.CHURN for tiling in ((8, 'gaussian'), (5, 'constant'))]


# ---- H1: the reference alone --------------------------------------------------------------------------------------------------------------
def test_reference_chain_does_not_depend_on_the_tiling():
    """Stub network (elementwise), static clamp, default churn: every window predicts the same x0 at a voxel in both evaluations of a
    step, so the fused predictions are those numbers whatever the stride and the weights, and the float64 chains of strides 16 / 8 / 5 x
    constant / gaussian agree on the voxels covered under all six and not background."""
    vol = R.shared_volume()
    tabs = HN.tables(HN.HP, HN.CHURN['churn-on'])
    assert (tabs['coefs'][:, 0] > 0).all() and (tabs['coefs'][:-1, 5] != 0).all() and tabs['coefs'][-1, 5] == 0
    refs = {(stride, kind): HN.joint_reference(vol, R.shared_cfg(stride), tabs, kind, False)
            for stride in (16, 8, 5) for kind in ('constant', 'gaussian')}
    common = np.logical_and.reduce([r['covered'] & ~r['background'] for r in refs.values()])
    share = common.mean()
    worst = max(np.abs(a['mean'] - b['mean'])[common].max() for a, b in itertools.combinations(refs.values(), 2))
    print(f"joint Heun reference, 6 tilings: common share {share:.4f}, largest difference {worst:.3e}")
    assert share >= 0.15
    assert worst <= 1e-12
    assert any(r['kept'] < r['candidates'] for r in refs.values())              # the 5 % rule drops windows: -1 slots
    assert np.ptp(refs[(8, 'gaussian')]['mean'][common]) > 0.1                  # and the compared values are not one constant


@pytest.mark.parametrize('dynamic,churn,tiling', CASES, ids=[f"{'dynamic' if d else 'static'}-{c}-s{t[0]}-{t[1]}" for d, c, t in CASES])
def test_chain_bound_dominates_an_fp32_emulation_and_is_small_beside_the_signal(dynamic, churn, tiling):
    """The two conditions on ``chain_bound``, on the reference alone: the same chain with every operation in np.float32 stays within half
    of it, and it is at most 1e-3 of the peak-to-peak of the reference over covered voxels -- the GPU comparison is not vacuous."""
    stride, blend = tiling
    vol, cfg = R.shared_volume(), R.shared_cfg(stride)
    tabs = HN.tables(HN.HP, HN.CHURN[churn])
    ref = HN.joint_reference(vol, cfg, tabs, blend, dynamic)
    emu = HN.joint_reference(vol, cfg, tabs, blend, dynamic, dtype=np.float32)
    live = ref['covered'] & ~ref['background']
    err = np.abs(emu['mean'] - ref['mean'])[live].max()
    ptp = np.ptp(ref['mean'][live])
    print(f"Heun chain {'dynamic' if dynamic else 'static'} {churn} stride {stride} {blend}: fp32 emulation / bound = "
          f"{err / ref['bound']:.3f} (err {err:.3e}, bound {ref['bound']:.3e}), bound / ptp = {ref['bound'] / ptp:.3e} (ptp {ptp:.3f}, "
          f"largest |state| {ref['state_max']:.2f})")
    assert err <= 0.5 * ref['bound']
    assert ref['bound'] <= 1e-3 * ptp


@pytest.mark.parametrize('churn', list(HN.CHURN))
@pytest.mark.parametrize('dynamic', [False, True], ids=['static', 'dynamic'])
def test_reference_is_the_oracle_per_window_at_stride_equal_patch(dynamic, churn):
    """Stride = patch, constant blend: every fused prediction is the one window's own, so the joint chain is ``edm_sample`` of the oracle
    (oracle/iqt_oracle_b.py, pinned by the reference's fixtures) with ``lowres_q_sample``, run per kept window in float64 on the same
    injected normals.  The two differ by the fp32 rounding of the step coefficients and of the low-res alpha / sigma (the specification
    uses the numbers the device holds) -- far inside ``chain_bound``, which is what the difference is held to."""
    from oracle import iqt_oracle_b as OB
    vol, cfg = R.shared_volume(), R.shared_cfg(16)
    tabs = HN.tables(HN.HP, HN.CHURN[churn])
    ref = HN.joint_reference(vol, cfg, tabs, 'constant', dynamic)
    L = J.layout(vol, cfg)
    hp = {**HN.HP, 'S_churn': HN.CHURN[churn]}
    T = hp['num_sample_steps']
    low = (vol - np.float32(300.0)) / np.float32(200.0)
    draws = [torch.from_numpy(J.normals(vol.shape, HN.SEED, k, 0).copy()) for k in range(T + 2)]
    cut = lambda a, o: a[o[0]:o[0] + 16, o[1]:o[1] + 16, o[2]:o[2] + 16][None, None]
    worst = 0.0
    for o in L['kept']:
        lr = OB.lowres_q_sample(torch.from_numpy(cut(low, o)).double(), torch.full((1,), HN.LOWRES_LEVEL), cut(draws[0], o))
        fn = lambda x, cn, lr=lr: 0.5 * (x / (1.0 + x.abs())) + 0.25 * lr + 0.015625 * cn.view(-1, 1, 1, 1, 1)
        want = OB.edm_sample(fn, (1, 1, 16, 16, 16), cut(draws[1], o), [cut(d, o) for d in draws[2:]], hp, dynamic=dynamic,
                             percentile=HN.PERCENTILE)
        assert want.dtype == torch.float64
        got = cut(ref['mean'], o)
        keep = ~cut(ref['background'], o)
        worst = max(worst, float(np.abs(got - want.numpy())[keep].max()))
    print(f"Heun reference vs oracle.edm_sample per window ({'dynamic' if dynamic else 'static'}, {churn}): {worst:.3e}, "
          f"bound {ref['bound']:.3e}")
    assert L['kept'].shape[0] >= 2 and worst <= ref['bound']


# ---- H2: host tables and argument rules, all before the device is touched -----------------------------------------------------------------
@pytest.mark.parametrize('churn', list(HN.CHURN))
def test_window_denoiser_host_tables(churn):
    elu = HN.make_elucidated(churn, False)
    den = elu.window_denoiser()
    tabs = HN.tables(HN.HP, HN.CHURN[churn])
    T = HN.HP['num_sample_steps']
    assert den.heun is True and den.num_steps == T and den.draw_base == 1 and not den.self_cond
    assert den.clamp == (-float('inf'), float('inf'), 1)
    assert not den.sched.is_cuda and tuple(den.sched.shape) == (T, 3)
    assert np.array_equal(np.asarray(den.sched, dtype=np.float64), tabs['sched'])
    assert den.sigma0 == tabs['sigma0'] == tabs['sched'][0, 0]
    assert den.coefs.dtype == torch.float32 and tuple(den.coefs.shape) == (T, 7) and not den.coefs.is_cuda
    assert np.array_equal(den.coefs.numpy().astype(np.float64), tabs['coefs'])
    assert (den.coefs[-1, 5:] == 0).all() and tabs['sched'][-1, 1] == 0          # no corrector on the step that ends at sigma 0
    assert (den.coefs[:, 0] == 0).all() == (churn == 'churn-off')
    for i, stage in itertools.product(range(T), (0, 1)):
        assert den.sigma_of(i, stage) == tabs['pre'][i][stage][0]
    lr = torch.zeros(2, 1, 16, 16, 16)
    with pytest.raises(ValueError, match="step"):
        den.x0(lr, lr, T, lowres_noise=lr)
    with pytest.raises(ValueError, match="stage"):
        den.x0(lr, lr, T - 1, stage=1, lowres_noise=lr)                         # sigma_next == 0: there is no second evaluation
    with pytest.raises(ValueError, match="augmentation noise"):
        den.x0(lr, lr, 0)
    other = elu.window_denoiser(sigma_min=0.1, sigma_max=1.0)                    # the per-call schedule overrides of ``sample``
    assert abs(other.sigma0 - 1.0) < 1e-6 and abs(float(other.sched[-1, 0]) - 0.1) < 1e-6
    assert HN.make_elucidated(churn, True, self_cond=True).window_denoiser().self_cond


def test_window_denoiser_and_callable_noise_argument_errors():
    elu = HN.make_elucidated('churn-on', False)
    lr = torch.zeros(2, 1, 16, 16, 16)
    with pytest.raises(ValueError, match="inpaint"):
        elu.window_denoiser(inpaint_images=lr, inpaint_masks=lr.bool())
    with pytest.raises(ValueError, match="inpaint"):
        elu.window_denoiser(inpaint_images=lr)
    with pytest.raises(ValueError, match="init_images"):
        elu.window_denoiser(init_images=lr)
    with pytest.raises(ValueError, match="skip_steps"):
        elu.window_denoiser(skip_steps=2)
    for bad in (0, 3, 1.5, True):
        with pytest.raises(ValueError, match="unet_number"):
            elu.window_denoiser(unet_number=bad)
    with pytest.raises(ValueError, match="null"):
        elu.window_denoiser(unet_number=1)

    def never(shape):
        raise AssertionError("the noise source must not be called")
    with pytest.raises(ValueError, match="exactly one U-Net"):                  # both U-Nets of the cascade would draw from the source
        elu.sample(batch_size=2, video_frames=16, use_tqdm=False, noise=never)
    with pytest.raises(ValueError, match="exactly one U-Net"):
        elu.sample(batch_size=2, video_frames=16, start_image_or_video=lr, start_at_unet_number=2, stop_at_unet_number=1,
                   use_tqdm=False, noise=never)


def test_volume_inference_takes_the_edm_denoiser_and_the_trainer_forwards_it():
    from diffusioniqt_amd.inference import VolumeInference
    from diffusioniqt_amd.trainer import ImagenTrainer
    elu = HN.make_elucidated('churn-on', False)
    den = elu.window_denoiser()
    inf = VolumeInference(R.shared_cfg(8), den, blend='gaussian', noise='anchored', joint=True)
    assert inf.joint and inf.sample_fn is den
    with pytest.raises(ValueError, match="joint"):
        VolumeInference(R.shared_cfg(8), den, blend='gaussian', joint=True)      # the joint chain needs the anchored field
    configs = {'Data': {'norm': 'z-score'}, 'Train': {'batch_sample': False, 'patch_size_sub': 16, 'pred_obj': 'x_start'},
               'Eval': {'repeat': 1}}
    ImagenTrainer.locked = False
    trainer = ImagenTrainer(configs=configs, imagen=elu, verbose=False)
    for kw in (dict(), dict(use_non_ema=True)):
        d = trainer.window_denoiser(**kw)
        assert d.heun and d.num_steps == HN.HP['num_sample_steps']
    with pytest.raises(ValueError, match="skip_steps"):
        trainer.window_denoiser(skip_steps=1)


# ---- H3: error codes of the entry ---------------------------------------------------------------------------------------------------------
def test_joint_heun_entry_returns_error_codes():
    from diffusioniqt_amd import _lib
    lib = _lib.load()
    buf = (np.zeros(4, dtype=np.int32)).ctypes.data                             # never dereferenced: every call below is refused
    geo = (40, 36, 44, 16, 8, 4, 3, 4)                                          # D, H, W, P, stride and the lattice of range(0, n - 15, 8)

    def heun(y, slot, taps, xh, xn, x0, phase=1, geo=geo, mode=1, draw=2):
        return lib.diqt_volume_joint_heun(y, slot, taps, xh, xn, x0, phase, 3, *geo, 0.5, 0.5, 0.0, 0.0, 0.0, -1.0, 1.0, mode, 0, draw, 0,
                                          None)
    for phase in (1, 2):
        for hole in range(6):
            args = [buf] * 6
            args[hole] = None
            assert heun(*args, phase=phase) == -2                               # DIQT_E_ALIGN
            assert b"null pointer" in lib.diqt_last_error()
    assert heun(None, None, None, None, None, None, phase=0) == -2              # the initial state still needs xh ...
    assert heun(None, None, None, buf, None, None, phase=0, geo=(0, 36, 44, 0, 0, 0, 0, 0)) == -1    # ... a volume ...
    assert heun(None, None, None, buf, None, None, phase=0, draw=2 ** 32 - 1) == -1                  # ... and room for draw + 1
    assert heun(buf, buf, buf, buf, buf, buf, geo=(40, 36, 44, 16, 8, 4, 3, 5)) == -1   # DIQT_E_SHAPE: not the lattice
    assert b"lattice" in lib.diqt_last_error()
    assert heun(buf, buf, buf, buf, buf, buf, geo=(40, 36, 44, 16, 0, 4, 3, 4)) == -1
    assert heun(buf, buf, buf, buf, buf, buf, geo=(40, 36, 44, 48, 8, 1, 1, 1)) == -1   # a window larger than the volume
    for phase in (3, -1):
        assert heun(buf, buf, buf, buf, buf, buf, phase=phase) == -3            # DIQT_E_UNSUPPORTED
        assert b"phase" in lib.diqt_last_error()
    assert heun(buf, buf, buf, buf, buf, buf, mode=2) == -3
