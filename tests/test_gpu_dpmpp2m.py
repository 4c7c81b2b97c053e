"""The second-order multistep sampler ``sampler='dpmpp2m'`` on a real MI355X against the float64 specification of
tests/dpmpp2m_reference.py: ``Imagen.sample`` with the elementwise stub network (so what is measured is the sampler's round-off), the
tie to DDIM where the solver is first-order (K <= 2), the draws it consumes, volume-anchored noise under it, the new kernel
(``ops.volume_joint_multistep``) on its own, the joint chain of ``VolumeInference(joint=True)`` and its bit-for-bit tie to independent
windows at stride = patch.

Bounds.  A DDIM step is 8 fp32 operations on values of the largest magnitude compared (tests/test_gpu_ddim.py); the multistep step adds
one product and one sum (10), and its two x0 products are up to c = max_i (|k0| + |kp|) / |k0'| times the single DDIM product
(``dpmpp2m_reference.amplification``; k0' the DDIM coefficient), so a chain of K steps is allowed K x 10 c x 2^-23 x max|x|, and a joint
chain ``dpmpp2m_reference.chain_bound``: the same with the blend's n + 3 summation terms per step."""
import itertools

import numpy as np
import pytest
import torch

from tests import anchored_noise_reference as A
from tests import dpmpp2m_reference as M
from tests import volume_blend_reference as R
from tests import volume_joint_reference as J
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
STEPS, SHAPE = 6, (2, 1, 8, 8, 8)
MODES = {'clamp-min': ('z-score', False, (J.MIN_BOUND, 0., 0)), 'clamp-box': ('min-max', False, (-1., 1., 1)),
         'dynamic': ('min-max', True, (-1., 1., 1))}
_REF = {}


def _ref(key, make):
    """One float64 reference per case, shared by the tests that need it and never modified."""
    if key not in _REF:
        _REF[key] = make()
        for v in _REF[key].values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return _REF[key]


def stub_imagen(objective, mode, size=16, kind='cosine', unet=None):
    from diffusioniqt_amd.imagen_pytorch3D import Imagen, NullUnet
    norm, dynamic, _ = MODES[mode]
    configs = {'Data': {'norm': norm}, 'Train': {'batch_sample': False}}
    return Imagen(unets=(NullUnet(), unet if unet is not None else A.make_stub_unet()), configs=configs, min_bound=J.MIN_BOUND,
                  image_sizes=(size, size), channels=1, pred_objectives=objective, noise_schedules=('cosine', kind),
                  dynamic_thresholding=dynamic, p2_loss_weight_gamma=0.0, cond_drop_prob=0.0).to(DEV)


def amplification(scheduler, steps):
    return M.amplification(*M.table64(*M.chain_log_snr(scheduler, steps)))


def same(a, b):
    """Image and both per-step lists, bit for bit."""
    return torch.equal(a[0], b[0]) and len(a[1]) == len(b[1]) and len(a[2]) == len(b[2]) and \
        all(np.array_equal(p, q) for p, q in zip(a[1], b[1])) and all(np.array_equal(p, q) for p, q in zip(a[2], b[2]))


@pytest.fixture(scope="module")
def draws():
    """Low-res conditioning and the initial image (read only)."""
    g = torch.Generator().manual_seed(3)
    return [torch.randn(SHAPE, generator=g) for _ in range(2)]


# ---- G1: sample against the float64 loop ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', list(MODES))
@pytest.mark.parametrize('objective', ['noise', 'x_start', 'v'])
@pytest.mark.parametrize('kind', ['cosine', 'linear'])
def test_sample_matches_the_float64_loop(draws, kind, objective, mode):
    from diffusioniqt_amd.imagen_pytorch3D import log_snr_to_alpha_sigma
    norm, dynamic, _ = MODES[mode]
    imagen = stub_imagen(objective, mode, size=8, kind=kind)
    lowres, init = draws
    img, noisy, x0 = imagen.sample(batch_size=2, start_image_or_video=lowres.to(DEV), start_at_unet_number=2, use_tqdm=False,
                                   noise=[init], sampler='dpmpp2m', sample_steps=STEPS)
    assert len(noisy) == len(x0) == STEPS + 1

    sch = imagen.noise_schedulers[1]
    ls, lsn = M.chain_log_snr(sch, STEPS)
    table, k01 = M.table64(ls, lsn)
    c = M.amplification(table, k01)
    coefs = np.repeat(table[:, :, None], 2, axis=2)                  # the float64 table, not the product's
    conds = torch.stack([sch.log_snr(t) for t, _ in sch.get_sampling_timesteps(2, device='cpu', steps=STEPS)])
    al, sg = log_snr_to_alpha_sigma(conds)                          # the x0 conversion of the ancestral branch, as it forms it (fp32)
    x0c = torch.stack((1. / al.clamp(min=1e-8), -sg / al.clamp(min=1e-8)) if objective == 'noise' else (al, -sg), dim=1).numpy()
    lo, hi = (J.MIN_BOUND, None) if norm == 'z-score' else (-1.0, 1.0)
    ref_img, ref_noisy, ref_x0 = M.reference_loop(
        lambda x, l: A.stub_net64(x, lowres.numpy(), l), init.numpy(), coefs, x0c, conds.numpy(), objective, lo, hi,
        dyn_q=imagen.dynamic_thresholding_percentile if dynamic else None, dyn_floor=1.0)
    got = [img.cpu().numpy()] + list(noisy) + list(x0)
    ref = [ref_img] + ref_noisy + ref_x0
    scale = max(np.abs(r).max() for r in ref)
    bound = STEPS * 10 * c * 2.0 ** -23 * scale
    worst = max(np.abs(g.astype(np.float64) - r).max() for g, r in zip(got, ref))
    print(f"dpmpp2m {kind} {objective} {mode}: max err {worst:.3e}, bound {bound:.3e}, c {c:.3f}, max|x| {scale:.3e}")
    for g, r in zip(got, ref):
        assert g.shape == r.shape and np.isfinite(g).all()
        assert np.abs(g.astype(np.float64) - r).max() <= bound


# ---- G2: one and two steps are DDIM ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden_sampler():
    from diffusioniqt_amd.imagen_pytorch3D import Imagen, NullUnet
    from tests.test_gpu_unet import T, build
    g, gu = load_golden('ddpmA_traj'), load_golden('unetA_tiny')
    unet, _, _ = build(gu, 0)
    configs = {'Data': {'norm': 'z-score'}, 'Train': {'batch_sample': False, 'patch_size_sub': 8, 'pred_obj': 'x_start'}, 'Eval': {'repeat': 1}}
    imagen = Imagen(unets=(NullUnet(), unet), configs=configs, min_bound=float(g['min_bound']), image_sizes=(8, 8), channels=1,
                    pred_objectives='x_start', timesteps=int(g['T']), dynamic_thresholding=False, p2_loss_weight_gamma=0.0,
                    cond_drop_prob=0.0).to(DEV)
    kw = dict(batch_size=2, start_image_or_video=T(g['lowres']).to(DEV), start_at_unet_number=2, use_tqdm=False)
    return imagen, T(g['init_noise']), kw


@pytest.mark.parametrize('K', [1, 2])
def test_one_and_two_steps_are_ddim(draws, golden_sampler, K):
    """The first step and the last are first-order: with K <= 2 the table is DDIM's (third column 0) and so is every returned bit."""
    imagen = stub_imagen('x_start', 'clamp-min', size=8)
    kw = dict(batch_size=2, start_image_or_video=draws[0].to(DEV), start_at_unet_number=2, use_tqdm=False, sample_steps=K)
    a = imagen.sample(noise=[draws[1]], sampler='dpmpp2m', **kw)
    assert len(a[1]) == K + 1 and same(a, imagen.sample(noise=[draws[1]], sampler='ddim', eta=0.0, **kw))
    imagen, init, kw = golden_sampler
    a = imagen.sample(noise=[init], sampler='dpmpp2m', sample_steps=K, **kw)
    assert len(a[1]) == K + 1 and same(a, imagen.sample(noise=[init], sampler='ddim', eta=0.0, sample_steps=K, **kw))


def test_three_steps_are_not_ddim(draws):
    imagen = stub_imagen('x_start', 'clamp-min', size=8)
    kw = dict(batch_size=2, start_image_or_video=draws[0].to(DEV), start_at_unet_number=2, use_tqdm=False, sample_steps=3)
    a = imagen.sample(noise=[draws[1]], sampler='dpmpp2m', **kw)
    b = imagen.sample(noise=[draws[1]], sampler='ddim', **kw)
    assert np.array_equal(a[1][0], b[1][0]) and np.array_equal(a[2][1], b[2][1])      # the first step, and the x0 of the second
    assert not np.array_equal(a[1][1], b[1][1]) and not torch.equal(a[0], b[0])       # the history term


# ---- G3: the draws it consumes -----------------------------------------------------------------------------------------------------------
def test_noise_sources(draws):
    imagen = stub_imagen('x_start', 'clamp-min', size=8)
    kw = dict(batch_size=2, start_image_or_video=draws[0].to(DEV), start_at_unet_number=2, use_tqdm=False, sampler='dpmpp2m',
              sample_steps=STEPS)
    seen = []

    def source(shape):
        seen.append(tuple(shape))
        return draws[1].to(DEV)
    a = imagen.sample(noise=source, **kw)
    assert seen == [SHAPE]                                                      # called exactly once: the initial image
    assert same(a, imagen.sample(noise=[draws[1]], **kw))                       # a one-element list is the whole chain's noise
    two = [draws[1], torch.full(SHAPE, float('nan'))]
    assert same(a, imagen.sample(noise=two, **kw)) and len(two) == 2            # the second element is never taken
    assert all(np.isfinite(v).all() for v in a[1])


# ---- G4: anchored noise ------------------------------------------------------------------------------------------------------------------
def test_anchored_noise_does_not_depend_on_the_batching(golden_sampler):
    """Four windows sampled at once and two by two, through ``ImagenTrainer.sample`` with ``AnchoredNoise.source``: the same patches."""
    from diffusioniqt_amd.inference import AnchoredNoise
    from diffusioniqt_amd.trainer import ImagenTrainer
    imagen = golden_sampler[0]
    ImagenTrainer.locked = False
    trainer = ImagenTrainer(configs=imagen.configs, imagen=imagen, verbose=False)
    origins = np.array([(0, 0, 0), (4, 4, 4), (4, 4, 8), (12, 16, 20)], dtype=np.int32)       # two of them overlap
    field = AnchoredNoise((20, 24, 28), seed=9)
    lowres = torch.randn(4, 1, 8, 8, 8, generator=torch.Generator().manual_seed(1)).to(DEV)

    def run(rows):
        out = trainer.sample(batch_size=len(rows), start_image_or_video=lowres[rows], start_at_unet_number=2,
                             noise=field.source(origins[rows], 8, sample=1), sampler='dpmpp2m', sample_steps=4)[0]
        assert tuple(out.shape) == (len(rows), 1, 8, 8, 8)
        return out
    whole = run([0, 1, 2, 3])
    assert whole.unique().numel() > 1000
    assert torch.equal(torch.cat((run([0, 1]), run([2, 3]))), whole)
    assert torch.equal(torch.cat((run([2, 3]), run([0, 1])))[[2, 3, 0, 1]], whole)


# ---- G5: the kernel against the float64 specification --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def step_case():
    """Per (stride, kind): predictions y for the kept windows of the shared volume (40 x 36 x 44: W is no multiple of 64, the 5 % rule
    leaves -1 slots, stride 5 covers raggedly), a state x_t, a previous x0 and the layout (read only)."""
    rng = np.random.default_rng(16)
    vol = R.shared_volume()
    out = {}
    for stride, kind in itertools.product((8, 5), ('gaussian', 'constant')):
        L = J.layout(vol, R.shared_cfg(stride))
        assert (L['slot'] < 0).any()
        y = rng.standard_normal((L['kept'].shape[0], 16, 16, 16)).astype(np.float32) * 2
        out[stride, kind] = (L, y, rng.standard_normal(vol.shape).astype(np.float32) * 3,
                             rng.standard_normal(vol.shape).astype(np.float32) * 2, R.taps_of(16, kind))
    return out


@pytest.mark.parametrize('with_prev', [False, True], ids=['step0', 'history'])
@pytest.mark.parametrize('clamp', [(-0.75, 0., 0), (-1., 1., 1)], ids=['min', 'box'])
@pytest.mark.parametrize('kind', ['gaussian', 'constant'])
@pytest.mark.parametrize('stride', [8, 5])
def test_joint_multistep_matches_reference(step_case, stride, kind, clamp, with_prev):
    """Per voxel: the blend's own bound on x0, (n + 3) 2^-23 max|y| (``volume_blend_reference.tolerance``), scaled by |k0| <= 1, plus the
    update's four roundings (two products, the fma, the sum), each at most 2^-24 of its own result: |k0| S, |kp| S, (|kx| + |k0|) S
    and S with S = scale, the largest magnitude among the clamped predictions, x_t, x0_prev and the expected output -- 4.125 2^-24 S
    with these coefficients.  Together at most (n + 3 + 4) 2^-23 scale."""
    from diffusioniqt_amd import ops
    L, y, x_t, prev, taps = step_case[stride, kind]
    kx, k0, kp = 0.8125, 0.9375, -0.4375
    prev64 = prev.astype(np.float64) if with_prev else None
    want, want0, covered = M.joint_multistep(y, L['slot'], taps, stride, x_t.astype(np.float64), prev64, kx, k0, kp, J.clamp_of(*clamp))
    assert covered.any() and (~covered).any()
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    args = (cu(y), cu(L['slot'].astype(np.int32)), cu(taps.astype(np.float32)))
    x_dev, p_dev = cu(x_t), cu(prev) if with_prev else None
    x0 = torch.full_like(x_dev, 7.0)
    got, got0 = ops.volume_joint_multistep(*args, x_dev, p_dev, kx, k0, kp, *clamp, stride, x0_out=x0)
    assert got.data_ptr() != x_dev.data_ptr() and got0.data_ptr() == x0.data_ptr() and torch.equal(x_dev, cu(x_t))
    assert not with_prev or torch.equal(p_dev, cu(prev))
    max_y = float(np.abs(J.clamp_of(*clamp)(y.astype(np.float64))).max())
    scale = max(max_y, float(np.abs(x_t).max()), float(np.abs(prev).max()) if with_prev else 0., float(np.abs(want).max()))
    bound = (L['windows_per_voxel'] + 3 + 4) * 2.0 ** -23 * scale
    err = np.abs(got.cpu().numpy().astype(np.float64) - want).max()
    err0 = np.abs(x0.cpu().numpy().astype(np.float64) - want0).max()
    print(f"joint multistep stride {stride} {kind} clamp {clamp} history {with_prev}: max err {err:.3e} (x0 {err0:.3e}), "
          f"bound {bound:.3e}, scale {scale:.3e}")
    assert err <= bound and err0 <= R.tolerance(L['windows_per_voxel'], max_y)
    assert np.array_equal(got.cpu().numpy()[~covered], x_t[~covered])           # uncovered voxels return x_t ...
    assert not x0.cpu().numpy()[~covered].any()                                 # ... and x0_out = 0
    # in place on both pairs (x_next = x_t, x0_out = x0_prev) = out of place, bit for bit
    hist = p_dev.clone() if with_prev else torch.full_like(x_dev, 7.0)
    same_x, same_0 = ops.volume_joint_multistep(*args, x_dev, hist if with_prev else None, kx, k0, kp, *clamp, stride, out=x_dev,
                                                x0_out=hist)
    assert same_x.data_ptr() == x_dev.data_ptr() and same_0.data_ptr() == hist.data_ptr()
    assert torch.equal(x_dev, got) and torch.equal(hist, got0)


@pytest.mark.parametrize('clamp', [(-0.75, 0., 0), (-1., 1., 1)], ids=['min', 'box'])
def test_joint_multistep_without_history_is_the_step_kernel(step_case, clamp):
    """kp = 0 and no x0_prev: the bits of ``ops.volume_joint_step`` at kn = 0, state and fused x0 alike."""
    from diffusioniqt_amd import ops
    L, y, x_t, _, taps = step_case[5, 'gaussian']
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    args = (cu(y), cu(L['slot'].astype(np.int32)), cu(taps.astype(np.float32)), cu(x_t))
    a0 = torch.empty_like(args[3])
    a = ops.volume_joint_step(*args, 0.8125, 0.9375, 0.0, *clamp, 5, 0, 1, x0_out=a0)
    b, b0 = ops.volume_joint_multistep(*args, None, 0.8125, 0.9375, 0.0, *clamp, 5)
    assert torch.equal(a, b) and torch.equal(a0, b0) and a.unique().numel() > 1000


def test_joint_multistep_argument_errors(step_case):
    from diffusioniqt_amd import ops
    L, y, x_t, prev, taps = step_case[8, 'gaussian']
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    y, slot, taps, x, prev = cu(y), cu(L['slot'].astype(np.int32)), cu(taps.astype(np.float32)), cu(x_t), cu(prev)
    ok = (1.0, 0.5, -0.25, -1.0, 1.0, 1, 8)
    with pytest.raises(ValueError, match="slot names window"):
        ops.volume_joint_multistep(y[:-1].contiguous(), slot, taps, x, prev, *ok)
    with pytest.raises(ValueError, match="lattice"):
        ops.volume_joint_multistep(y, slot, taps, x, prev, 1.0, 0.5, -0.25, -1.0, 1.0, 1, 5)
    with pytest.raises(ValueError, match="clamp_mode"):
        ops.volume_joint_multistep(y, slot, taps, x, prev, 1.0, 0.5, -0.25, -1.0, 1.0, 2, 8)
    with pytest.raises(ValueError, match="cubic"):
        ops.volume_joint_multistep(y[:, :, :, :8].contiguous(), slot, taps, x, prev, *ok)
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.volume_joint_multistep(y, slot, taps, x.transpose(0, 1), prev, *ok)
    with pytest.raises(ValueError, match="x0_prev"):
        ops.volume_joint_multistep(y, slot, taps, x, prev[:-1].contiguous(), *ok)
    with pytest.raises(ValueError, match="x0_out"):
        ops.volume_joint_multistep(y, slot, taps, x, prev, *ok, x0_out=prev[:-1].contiguous())


# ---- G6: the whole joint chain against the float64 reference -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shared_vol():
    return torch.from_numpy(R.shared_volume()).to(DEV)


def chain_ref(imagen, vol_name, cfg_key, objective, mode, blend, samples=1, net=J.stub64, self_cond=False):
    vol, cfg = (R.block_volume(), R.block_cfg()) if vol_name == 'block' else (R.shared_volume(), R.shared_cfg(cfg_key))
    dyn = (imagen.dynamic_thresholding_percentile, 1.0) if MODES[mode][1] else None
    return _ref((vol_name, cfg_key, objective, mode, blend, samples, self_cond), lambda: M.joint_reference(
        vol, cfg, net, M.tables(imagen.noise_schedulers[1], M.STEPS, objective), objective, MODES[mode][2], blend, samples=samples,
        dyn=dyn, self_cond=self_cond))


def joint_run(imagen, cfg, blend, **kw):
    from diffusioniqt_amd.inference import VolumeInference
    den = imagen.window_denoiser(sampler='dpmpp2m', sample_steps=M.STEPS)
    assert den.multistep and den.num_steps == M.STEPS
    return VolumeInference(cfg, den, blend=blend, noise='anchored', joint=True, seed=kw.pop('seed', J.SEED), **kw)


def check(imagen, got, ref, what, key='mean', factor=1):
    got = got.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == ref[key].shape and np.isfinite(got).all()
    c = amplification(imagen.noise_schedulers[1], M.STEPS)
    bound = factor * M.chain_bound(ref['windows_per_voxel'], ref['scale'], c)
    err = np.abs(got.astype(np.float64) - ref[key]).max()
    print(f"{what}: max |{key} - ref| = {err:.3e}, bound {bound:.3e} (n = {ref['windows_per_voxel']}, c {c:.3f}, "
          f"scale {ref['scale']:.3e})")
    assert err <= bound, what
    return got


@pytest.mark.parametrize('tiling', [(8, 'gaussian'), (5, 'constant')], ids=['s8-gaussian', 's5-constant'])
@pytest.mark.parametrize('setting', [('x_start', 'clamp-min'), ('noise', 'dynamic')], ids=['x_start-min', 'noise-dynamic'])
def test_joint_chain_matches_the_float64_reference(shared_vol, setting, tiling):
    (objective, mode), (stride, blend) = setting, tiling
    imagen = stub_imagen(objective, mode)
    ref = chain_ref(imagen, 'shared', stride, objective, mode, blend)
    got = joint_run(imagen, R.shared_cfg(stride), blend)(shared_vol)
    got = check(imagen, got, ref, f"joint dpmpp2m {objective} {mode} stride {stride} {blend}")
    assert (got[~ref['covered'] & ~ref['background']] == ref['fill']).all() and (got[ref['background']] == ref['min_val']).all()


def test_joint_batching_and_samples(shared_vol):
    imagen = stub_imagen('x_start', 'clamp-min')
    a = joint_run(imagen, R.shared_cfg(5, batch_size=7), 'gaussian')(shared_vol)
    b = joint_run(imagen, R.shared_cfg(5, batch_size=1), 'gaussian')(shared_vol)
    assert torch.equal(a, b)
    ref = chain_ref(imagen, 'shared', 8, 'x_start', 'clamp-min', 'gaussian', samples=2)
    inf = joint_run(imagen, R.shared_cfg(8), 'gaussian', samples=2)
    mean, std = inf(shared_vol, return_std=True)
    check(imagen, mean, ref, "joint dpmpp2m S = 2 mean")
    std = check(imagen, std, ref, "joint dpmpp2m S = 2 deviation", key='std', factor=2)
    live = ref['covered'] & ~ref['background']
    assert ref['std'][live].max() > 0.05 and not std[~live].any()               # the samples differ through draw 0 alone
    assert torch.equal(inf(shared_vol), mean)


def test_joint_block_mode_matches_the_float64_reference():
    imagen = stub_imagen('x_start', 'clamp-min', size=8)
    ref = chain_ref(imagen, 'block', None, 'x_start', 'clamp-min', 'gaussian')
    assert ref['kept'] == ref['candidates'] == 27 and ref['covered'].all()
    vol = torch.from_numpy(R.block_volume()).to(DEV)
    check(imagen, joint_run(imagen, R.block_cfg(), 'gaussian')(vol), ref, "joint dpmpp2m block mode P 24 stride 16")


def test_joint_self_conditioning_shares_the_history_volume(shared_vol):
    """The fused x0 volume is both the history term of the update and what a self-conditioned U-Net reads."""
    imagen = stub_imagen('x_start', 'clamp-min', unet=J.make_self_cond_unet())
    ref = chain_ref(imagen, 'shared', 8, 'x_start', 'clamp-min', 'gaussian', net=J.self_cond_stub64, self_cond=True)
    plain = chain_ref(imagen, 'shared', 8, 'x_start', 'clamp-min', 'gaussian')
    assert np.abs(ref['mean'] - plain['mean']).max() > 1e-2                     # the self-conditioning term is visible
    check(imagen, joint_run(imagen, R.shared_cfg(8), 'gaussian')(shared_vol), ref, "joint dpmpp2m self-conditioned stride 8")


# ---- G7: the tie to independent windows ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', list(MODES))
def test_joint_at_stride_equal_patch_is_the_independent_path(shared_vol, mode):
    """No overlap, unit weights: num / den is exact, every window's chain is its own, and the update is the step kernel's operation
    order with the previous x0 as its third operand -- the joint volume equals the blended independent windows bit for bit."""
    from diffusioniqt_amd.inference import VolumeInference
    imagen = stub_imagen('x_start', mode)
    cfg = R.shared_cfg(16)

    def sample_fn(x, noise=None):
        return imagen.sample(batch_size=x.shape[0], start_image_or_video=x, start_at_unet_number=2, use_tqdm=False, sampler='dpmpp2m',
                             sample_steps=M.STEPS, noise=noise)[0]
    independent = VolumeInference(cfg, sample_fn, blend='constant', noise='anchored', seed=J.SEED)(shared_vol)
    joint = joint_run(imagen, cfg, 'constant')(shared_vol)
    assert independent.unique().numel() > 1000
    assert torch.equal(joint, independent)


def test_joint_with_a_real_network_through_the_trainer(golden_sampler):
    from diffusioniqt_amd.inference import VolumeInference
    from diffusioniqt_amd.trainer import ImagenTrainer
    imagen = golden_sampler[0]
    ImagenTrainer.locked = False
    trainer = ImagenTrainer(configs=imagen.configs, imagen=imagen, verbose=False)
    vol = torch.from_numpy(np.random.default_rng(12).integers(1, 1000, (20, 24, 28)).astype(np.float32)).to(DEV)   # every window is kept

    def sample_fn(x, noise=None):
        return trainer.sample(batch_size=x.shape[0], start_image_or_video=x, start_at_unet_number=2, sampler='dpmpp2m', sample_steps=4,
                              noise=noise)[0]
    cfg = R.shared_cfg(8, batch_size=6, P=8)
    den = trainer.window_denoiser(sampler='dpmpp2m', sample_steps=4)
    assert den.multistep and den.num_steps == 4
    independent = VolumeInference(cfg, sample_fn, blend='constant', noise='anchored', seed=4)(vol)
    joint = VolumeInference(cfg, den, blend='constant', noise='anchored', joint=True, seed=4)(vol)
    assert torch.equal(joint, independent) and joint.unique().numel() > 1000
    ddim = VolumeInference(cfg, trainer.window_denoiser(sampler='ddim', sample_steps=4), blend='constant', noise='anchored', joint=True,
                           seed=4)(vol)
    assert not torch.equal(joint, ddim)
