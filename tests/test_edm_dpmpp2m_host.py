"""Host-side checks of ``ElucidatedImagen(sampler='dpmpp2m')`` (no GPU here): the coefficient table against the float64 specification of
tests/edm_dpmpp2m_reference.py and its algebraic properties, every argument rule before anything touches the device, the error codes of
the two new entries, the solver's accuracy with the product's fp32 table on the analytic Gaussian problem (order two, deterministic
Heun's error at half its evaluations, the SDE's stationary variance by exact covariance propagation), the host tables of the window
denoiser, and the derived rounding bound against an fp32 emulation of the joint chain."""
import math

import numpy as np
import pytest
import torch

from tests import edm_dpmpp2m_reference as E
from tests import volume_blend_reference as R
from tests import volume_joint_heun_reference as HN

SCHEDULES = {'test-4': dict(HN.HP), 'karras-32': dict(num_sample_steps=32, sigma_min=0.002, sigma_max=80, rho=7, S_noise=1.003)}


@pytest.fixture(scope="module")
def elu():
    return HN.make_elucidated('churn-on', False)


def product_table(elu, hp, eta, S_noise, steps=None):
    sigmas = elu.sample_schedule(steps or hp['num_sample_steps'], hp['rho'], hp['sigma_min'], hp['sigma_max'])
    return sigmas, elu.dpmpp2m_coefficients(sigmas, eta, S_noise)


# ---- H1: the table ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('eta,S_noise', [(0.0, 1.0), (1.0, 1.003), (0.375, 1.0)])
@pytest.mark.parametrize('name', list(SCHEDULES))
def test_table_matches_the_specification(elu, name, eta, S_noise):
    hp = SCHEDULES[name]
    sigmas, got = product_table(elu, hp, eta, S_noise)
    T = hp['num_sample_steps']
    assert got.dtype == torch.float32 and tuple(got.shape) == (T, 4) and not got.is_cuda
    assert np.array_equal(sigmas.numpy().astype(np.float64), E.schedule(hp))
    want, c = E.table64(E.schedule(hp), eta, S_noise)
    got = got.numpy().astype(np.float64)
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    print(f"table {name} eta {eta}: largest error {err.max() / 2.0 ** -23:.3f} x 2^-23")
    assert (err <= 2.0 ** -23).all()
    ulps = np.abs((got[:, 1] + got[:, 2]) - c) / np.spacing(c.astype(np.float32)).astype(np.float64)
    print(f"table {name} eta {eta}: k0 + kp within {ulps.max():.2f} ulps of c")
    assert (ulps <= 2.0).all()
    assert got[0, 2] == 0.0 and (got[1:-1, 2] < 0).all()                        # row 0 has no history; the rows between do
    assert tuple(got[-1]) == (0.0, 1.0, 0.0, 0.0)                               # sigma' = 0: first order by definition
    assert (got[:, 3] == 0).all() == (eta == 0) and (got[:-1, 3] > 0).all() == (eta > 0)


def test_row_zero_of_the_ode_table_is_the_euler_predictor(elu):
    """eta = 0: kx = sigma' / sigma = 1 + r and k0 = 1 - sigma' / sigma = -r with r = (sigma' - sigma) / sigma, the (1 + r, -r) of the
    Heun sampler's predictor without churn -- equal up to the fp32 rounding of both."""
    hp = SCHEDULES['karras-32']
    sigmas, got = product_table(elu, hp, 0.0, 1.0)
    s = sigmas.double().numpy()
    r = (s[1] - s[0]) / s[0]
    assert abs(float(got[0, 0]) - (1 + r)) <= 2.0 ** -23 and abs(float(got[0, 1]) - (-r)) <= 2.0 ** -23


# ---- H2: refusals, all before the device is touched --------------------------------------------------------------------------------------------
def test_sampler_argument_rules(elu):
    lr = torch.zeros(2, 1, 16, 16, 16)

    def never(shape):
        raise AssertionError("the noise source must not be called")
    kw = dict(batch_size=2, video_frames=16, start_image_or_video=lr, start_at_unet_number=2, use_tqdm=False, noise=never)
    for call in (lambda **k: elu.sample(**kw, **k), lambda **k: elu.window_denoiser(**k)):
        with pytest.raises(ValueError, match="sampler must be"):
            call(sampler='ddim')
        for eta in (-0.1, 1.5, float('nan'), 'x'):
            with pytest.raises(ValueError, match="eta must be"):
                call(sampler='dpmpp2m', eta=eta)
        with pytest.raises(ValueError, match="neither eta nor sample_steps"):
            call(eta=0.5)
        with pytest.raises(ValueError, match="neither eta nor sample_steps"):
            call(sampler='heun', sample_steps=8)
        for steps in (1, 0, 2.5, True):
            with pytest.raises(ValueError, match="sample_steps must be"):
                call(sampler='dpmpp2m', sample_steps=steps)
    with pytest.raises(ValueError, match="skip_steps"):
        elu.sample(**kw, sampler='dpmpp2m', skip_steps=1)
    with pytest.raises(ValueError, match="skip_steps"):
        elu.window_denoiser(sampler='dpmpp2m', skip_steps=1)
    with pytest.raises(ValueError, match="skip_steps"):
        elu.one_unet_sample(elu.unets[1], (2, 1, 16, 16, 16), unet_number=2, sampler='dpmpp2m', skip_steps=1, noise=never)
    with pytest.raises(ValueError, match="sampler must be"):                    # one value per U-Net: the second one is wrong
        elu.sample(**kw, sampler=('heun', 'euler'))
    with pytest.raises(ValueError, match="neither eta nor sample_steps"):
        elu.sample(**kw, sampler=('heun', 'heun'), eta=(0.0, 1.0))


def test_ops_argument_checks_run_on_the_host():
    from diffusioniqt_amd import ops
    x = torch.zeros(3, 1, 7, 9, 11)
    k = torch.zeros(3)
    with pytest.raises(RuntimeError, match="no CPU fallback|HIP"):
        ops.multistep_sde_step(x, x, None, None, k, k, k, k)
    with pytest.raises(ValueError, match="seed must fit"):
        ops.volume_joint_multistep_sde(None, None, None, None, None, 0., 0., 0., 1.5, -1., 1., 1, 8, -1, 0, shape=(12, 22, 70))
    with pytest.raises(ValueError, match="draw"):
        ops.volume_joint_multistep_sde(None, None, None, None, None, 0., 0., 0., 1.5, -1., 1., 1, 8, 0, 1 << 32, shape=(12, 22, 70))
    with pytest.raises(ValueError, match="initial state needs shape"):
        ops.volume_joint_multistep_sde(None, None, None, None, None, 0., 0., 0., 1.5, -1., 1., 1, 8, 0, 0)
    with pytest.raises(ValueError, match="initial state needs shape"):
        ops.volume_joint_multistep_sde(None, None, None, None, None, 0., 0., 0., 1.5, -1., 1., 1, 8, 0, 0, shape=(12, 0, 70))


# ---- H3: error codes of the two entries ----------------------------------------------------------------------------------------------------
def test_entries_return_error_codes():
    from diffusioniqt_amd import _lib
    lib = _lib.load()
    buf = (np.zeros(4, dtype=np.int32)).ctypes.data                             # never dereferenced: every call below is refused
    for hole in (0, 1, 4, 5, 6, 7, 8):                                          # x0_prev (2) and noise (3) may be NULL
        args = [buf] * 9
        args[hole] = None
        assert lib.diqt_multistep_sde_step(*args, 3, 693, None) == -2           # DIQT_E_ALIGN
        assert b"null pointer" in lib.diqt_last_error()
    assert lib.diqt_multistep_sde_step(*([buf] * 9), 0, 693, None) == -1        # DIQT_E_SHAPE
    assert lib.diqt_multistep_sde_step(*([buf] * 9), 3, 0, None) == -1
    assert lib.diqt_multistep_sde_step(*([buf] * 9), 65536, 693, None) == -1
    geo = (12, 22, 70, 8, 5, 1, 3, 13)                                          # D, H, W, P, stride and the lattice of range(0, n - 7, 5)

    def joint(y, slot, taps, x_t, prev, x_next, x0_out, geo=geo, mode=1, N=3):
        return lib.diqt_volume_joint_multistep_sde(y, slot, taps, x_t, prev, x_next, x0_out, N, *geo, 0.5, 0.5, -0.25, 0.25, -1.0, 1.0,
                                                   mode, 0, 2, 0, None)
    for hole in (0, 1, 2, 5, 6):                                                # x0_prev (4) may be NULL; x_t (3) NULL is the initial state
        args = [buf] * 7
        args[hole] = None
        assert joint(*args) == -2
        assert b"null pointer" in lib.diqt_last_error()
    assert joint(None, None, None, None, None, None, None) == -2                # the initial state still needs x_next ...
    assert joint(None, None, None, None, None, buf, None, geo=(0, 22, 70, 0, 0, 0, 0, 0)) == -1    # ... and a volume
    assert joint(*([buf] * 7), geo=(12, 22, 70, 8, 5, 1, 3, 12)) == -1          # DIQT_E_SHAPE: not the lattice
    assert b"lattice" in lib.diqt_last_error()
    assert joint(*([buf] * 7), geo=(12, 22, 70, 8, 0, 1, 3, 13)) == -1
    assert joint(*([buf] * 7), geo=(12, 22, 70, 16, 8, 1, 1, 7)) == -1          # a window larger than the volume
    assert joint(*([buf] * 7), N=-1) == -1
    for mode in (2, -1):
        assert joint(*([buf] * 7), mode=mode) == -3                             # DIQT_E_UNSUPPORTED
        assert b"clamp_mode" in lib.diqt_last_error()


# ---- H4: accuracy with the product's fp32 table on the Gaussian problem -----------------------------------------------------------------------
def _problem(elu, K, eta):
    sigmas, table = product_table(elu, E.KARRAS, eta, 1.0, steps=K)
    return table.double().numpy(), sigmas.double().numpy()


def test_ode_solver_matches_deterministic_heun_at_half_the_evaluations(elu):
    """Same K, same schedule, same start: 2M spends K evaluations, Heun 2K - 1.  Measured ratios 1.11, 1.11 and 1.08."""
    for K in (16, 24, 32):
        table, sigmas = _problem(elu, K, 0.0)
        e2m, eheun = E.gaussian_problem_error(table, sigmas), E.heun_problem_error(sigmas)
        print(f"K {K}: 2M error {e2m:.3e} ({K} evaluations), Heun error {eheun:.3e} ({2 * K - 1} evaluations), ratio {e2m / eheun:.3f}")
        assert e2m <= 1.25 * eheun


def test_ode_solver_is_second_order(elu):
    err = {K: E.gaussian_problem_error(*_problem(elu, K, 0.0)) for K in (16, 32, 64)}
    print("2M errors " + ", ".join(f"K {K}: {e:.3e}" for K, e in err.items()) + f"; ratios {err[16] / err[32]:.2f}, {err[32] / err[64]:.2f}")
    assert err[32] <= err[16] / 3 and err[64] <= err[32] / 3


def test_sde_solver_keeps_the_data_variance(elu):
    """eta = 1 by exact propagation of the covariance of (x, D_prev): the final standard deviation against s = 0.5."""
    rel = {K: abs(E.gaussian_problem_std(*_problem(elu, K, 1.0)) - E.DATA_STD) / E.DATA_STD for K in (32, 48, 64, 128)}
    print("2M-SDE |std - s| / s " + ", ".join(f"K {K}: {v:.4f}" for K, v in rel.items()) +
          f"; factors {rel[32] / rel[64]:.2f}, {rel[64] / rel[128]:.2f}")
    assert rel[48] <= 0.03 and rel[64] <= 0.02
    assert rel[64] <= rel[32] / 3 and rel[128] <= rel[64] / 3
    assert abs(E.gaussian_problem_std(*_problem(elu, 32, 0.0)) - E.DATA_STD) / E.DATA_STD < 0.02       # the ODE transports it too


# ---- H5: the window denoiser's host tables ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('eta', list(E.ETAS))
def test_window_denoiser_host_tables(eta):
    from diffusioniqt_amd.inference import VolumeInference
    from diffusioniqt_amd.trainer import ImagenTrainer
    elu = HN.make_elucidated('churn-on', False)
    K = 6
    den = elu.window_denoiser(sampler='dpmpp2m', sample_steps=K, eta=E.ETAS[eta])
    assert den.multistep is True and den.heun is False and den.num_steps == K and den.draw_base == 1 and not den.self_cond
    assert den.clamp == (-float('inf'), float('inf'), 1)
    sigmas = E.schedule(HN.HP, K)
    assert den.sigma0 == sigmas[0] and np.array_equal(np.asarray(den.sigmas), sigmas)
    assert den.coefs.dtype == torch.float32 and tuple(den.coefs.shape) == (K, 4) and not den.coefs.is_cuda
    assert torch.equal(den.coefs, elu.dpmpp2m_coefficients(elu.sample_schedule(K, 7, 0.3, 1.5), E.ETAS[eta], HN.HP['S_noise']))
    assert [den.sigma_of(i) for i in range(K)] == list(sigmas[:-1])             # the network is evaluated at sigma_i itself
    lr = torch.zeros(2, 1, 16, 16, 16)
    with pytest.raises(ValueError, match="step"):
        den.x0(lr, lr, K, lowres_noise=lr)
    with pytest.raises(ValueError, match="augmentation noise"):
        den.x0(lr, lr, 0)
    assert elu.window_denoiser(sampler='dpmpp2m').num_steps == HN.HP['num_sample_steps']
    inf = VolumeInference(R.shared_cfg(8), den, blend='gaussian', noise='anchored', joint=True)
    p = inf._protocol(den)
    assert p.sigma_space and p.multistep and not p.heun and p.draw_base == 1 and p.sigma0 == den.sigma0
    assert not inf._protocol(elu.window_denoiser()).sigma_space                 # the Heun denoiser has a sigma0 too
    configs = {'Data': {'norm': 'z-score'}, 'Train': {'batch_sample': False, 'patch_size_sub': 16, 'pred_obj': 'x_start'},
               'Eval': {'repeat': 1}}
    ImagenTrainer.locked = False
    trainer = ImagenTrainer(configs=configs, imagen=elu, verbose=False)
    d = trainer.window_denoiser(sampler='dpmpp2m', sample_steps=K, eta=E.ETAS[eta], use_non_ema=True)
    assert d.multistep and d.num_steps == K and torch.equal(d.coefs, den.coefs)
    assert HN.make_elucidated('churn-on', True, self_cond=True).window_denoiser(sampler='dpmpp2m').self_cond


# ---- H6: the specification and its bound -------------------------------------------------------------------------------------------------------
def test_joint_reference_at_stride_equal_patch_is_the_window_loop():
    """Stride = patch, constant blend: every fused prediction is the one window's own, so the joint specification is the per-window
    loop on the same normals, window by window (to float64 round-off: the blend divides by the weight 1)."""
    from tests import volume_joint_reference as J
    vol, cfg = R.shared_volume(), R.shared_cfg(16)
    for eta in E.ETAS.values():
        tabs = E.tables(HN.HP, eta)
        ref = E.joint_reference(vol, cfg, tabs, 'constant', True, self_cond=True)
        L = J.layout(vol, cfg)
        T = tabs['coefs'].shape[0]
        draws = [J.normals(vol.shape, E.SEED, k, 0) for k in range(T + 2)]
        low = tabs['lowres'][0] * ((vol - np.float32(300.0)) / np.float32(200.0)).astype(np.float64) + tabs['lowres'][1] * draws[0]
        cut = lambda a, o: a[o[0]:o[0] + 16, o[1]:o[1] + 16, o[2]:o[2] + 16][None, None]
        worst = 0.0
        for o in L['kept']:
            want, _ = E.window_loop(HN.stub64, cut(draws[1], o), cut(low, o), tabs, True, [cut(d, o) for d in draws[2:]], self_cond=True)
            keep = ~cut(ref['background'], o)
            worst = max(worst, float(np.abs(cut(ref['mean'], o) - want)[keep].max()))
        print(f"joint specification vs window loop, eta {eta}: {worst:.3e}")
        assert L['kept'].shape[0] >= 2 and worst <= 1e-13


CASES = [(dynamic, eta, tiling) for dynamic in (False, True) for eta in E.ETAS for tiling in ((8, 'gaussian'), (5, 'constant'))]


@pytest.mark.parametrize('dynamic,eta,tiling', CASES, ids=[f"{'dynamic' if d else 'static'}-{e}-s{t[0]}-{t[1]}" for d, e, t in CASES])
def test_chain_bound_dominates_an_fp32_emulation(dynamic, eta, tiling):
    """The same chain with every operation in np.float32 stays under ``chain_bound``, and the bound is small beside the signal (at most
    1e-3 of the reference's peak-to-peak over covered voxels, as the Heun path asks of its own), so the GPU comparison is not vacuous."""
    stride, blend = tiling
    vol, cfg = R.shared_volume(), R.shared_cfg(stride)
    tabs = E.tables(HN.HP, E.ETAS[eta])
    ref = E.joint_reference(vol, cfg, tabs, blend, dynamic, self_cond=True)
    emu = E.joint_reference(vol, cfg, tabs, blend, dynamic, self_cond=True, dtype=np.float32)
    live = ref['covered'] & ~ref['background']
    err = np.abs(emu['mean'] - ref['mean'])[live].max()
    ptp = np.ptp(ref['mean'][live])
    print(f"2M chain {'dynamic' if dynamic else 'static'} {eta} stride {stride} {blend}: fp32 emulation / bound = {err / ref['bound']:.3f} "
          f"(err {err:.3e}, bound {ref['bound']:.3e}), bound / ptp = {ref['bound'] / ptp:.3e} (ptp {ptp:.3f}, largest |state| "
          f"{ref['state_max']:.2f})")
    assert err <= ref['bound']
    assert ref['bound'] <= 1e-3 * ptp
