"""Lockstep joint sampling of overlapping windows on a real MI355X against the float64 specification of
tests/volume_joint_reference.py: the two kernels on their own (``ops.volume_joint_step`` / ``ops.volume_joint_finish``), the whole chain of
``VolumeInference(joint=True)`` with the elementwise stub network (so what is measured is the sampler's and the blend's round-off), its
invariance under the tiling, the bit-for-bit tie to the independent-window path at stride = patch, batching / seed / samples, block
mode, self-conditioning, and a real network through ``ImagenTrainer.window_denoiser``.

Chain bound (``volume_joint_reference.chain_bound``): steps x (8 + n + 3) x 2^-23 x the largest magnitude compared -- per step the
sampler's 8 fp32 operations (tests/test_gpu_ddim.py) plus the blend's n + 3 summation terms, n = ceil(P / stride)^3."""
import itertools

import numpy as np
import pytest
import torch

from tests import anchored_noise_reference as A
from tests import volume_blend_reference as R
from tests import volume_joint_reference as J
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
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


def stub_imagen(objective, mode, size=16, unet=None):
    from diffusioniqt_amd.imagen_pytorch3D import Imagen, NullUnet
    norm, dynamic, _ = MODES[mode]
    configs = {'Data': {'norm': norm}, 'Train': {'batch_sample': False}}
    return Imagen(unets=(NullUnet(), unet if unet is not None else A.make_stub_unet()), configs=configs, min_bound=J.MIN_BOUND,
                  image_sizes=(size, size), channels=1, pred_objectives=objective, noise_schedules=('cosine', 'cosine'),
                  dynamic_thresholding=dynamic, p2_loss_weight_gamma=0.0, cond_drop_prob=0.0).to(DEV)


def chain_ref(imagen, vol_name, cfg_key, objective, mode, eta, blend, samples=1, net=J.stub64, self_cond=False):
    vol, cfg = (R.block_volume(), R.block_cfg()) if vol_name == 'block' else (R.shared_volume(), R.shared_cfg(cfg_key))
    dyn = (imagen.dynamic_thresholding_percentile, 1.0) if MODES[mode][1] else None
    return _ref((vol_name, cfg_key, objective, mode, eta, blend, samples, self_cond), lambda: J.joint_reference(
        vol, cfg, net, J.tables(imagen.noise_schedulers[1], J.STEPS, eta, objective), objective, MODES[mode][2], blend,
        samples=samples, dyn=dyn, self_cond=self_cond))


def joint_run(imagen, cfg, vol, eta, blend, **kw):
    from diffusioniqt_amd.inference import VolumeInference
    den = imagen.window_denoiser(sampler='ddim', sample_steps=J.STEPS, eta=eta)
    return VolumeInference(cfg, den, blend=blend, noise='anchored', joint=True, seed=kw.pop('seed', J.SEED), **kw)


def check(got, ref, what, key='mean', factor=1):
    got = got.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == ref[key].shape and np.isfinite(got).all()
    bound = factor * J.chain_bound(ref['windows_per_voxel'], ref['scale'])
    err = np.abs(got.astype(np.float64) - ref[key]).max()
    print(f"{what}: max |{key} - ref| = {err:.3e}, bound {bound:.3e} (n = {ref['windows_per_voxel']}, scale {ref['scale']:.3e})")
    assert err <= bound, what
    return got


@pytest.fixture(scope="module")
def shared_vol():
    return torch.from_numpy(R.shared_volume()).to(DEV)


# ---- G1: the step kernel against the float64 specification ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def step_case():
    """Per (stride, kind): predictions y for the kept windows of the shared volume, a state x_t, and the layout (read only)."""
    rng = np.random.default_rng(6)
    vol = R.shared_volume()
    out = {}
    for stride, kind in itertools.product((8, 5), ('gaussian', 'constant')):
        L = J.layout(vol, R.shared_cfg(stride))
        assert (L['slot'] < 0).any()
        y = rng.standard_normal((L['kept'].shape[0], 16, 16, 16)).astype(np.float32) * 2
        out[stride, kind] = (L, y, rng.standard_normal(vol.shape).astype(np.float32) * 3, R.taps_of(16, kind))
    return out


@pytest.mark.parametrize('kn', [0.0, 0.625])
@pytest.mark.parametrize('clamp', [(-0.75, 0., 0), (-1., 1., 1), (-float('inf'), float('inf'), 1)], ids=['min', 'box', 'none'])
@pytest.mark.parametrize('kind', ['gaussian', 'constant'])
@pytest.mark.parametrize('stride', [8, 5])
def test_joint_step_matches_reference(step_case, stride, kind, clamp, kn):
    """Per voxel |k0| tolerance(n, max|y|) (the blend's own bound) + 4 2^-24 (|kx| max|x_t| + |k0| max|y| + 6 |kn|) (three products, two
    sums; |n| < 6) + 2e-5 |kn| (the normals' bound of tests/test_gpu_anchored_noise.py)."""
    from diffusioniqt_amd import ops
    L, y, x_t, taps = step_case[stride, kind]
    kx, k0, seed, draw, sample = 0.8125, -0.4375, 0x123456789, 3, 2
    n64 = J.normals(x_t.shape, seed, draw, sample)
    want, want0, covered = J.joint_step(y, L['slot'], taps, stride, x_t.astype(np.float64), kx, k0, kn, J.clamp_of(*clamp), n64)
    assert covered.any() and (~covered).any()
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    args = (cu(y), cu(L['slot'].astype(np.int32)), cu(taps.astype(np.float32)))
    x_dev = cu(x_t)
    x0 = torch.full_like(x_dev, 7.0)
    got = ops.volume_joint_step(*args, x_dev, kx, k0, kn, *clamp, stride, seed, draw, sample, x0_out=x0)
    assert got.data_ptr() != x_dev.data_ptr() and torch.equal(x_dev, cu(x_t))
    max_y, max_x = float(np.abs(y).max()), float(np.abs(x_t).max())
    bound = abs(k0) * R.tolerance(L['windows_per_voxel'], max_y) + 4 * 2.0 ** -24 * (abs(kx) * max_x + abs(k0) * max_y + 6 * abs(kn)) \
        + 2e-5 * abs(kn)
    err = np.abs(got.cpu().numpy().astype(np.float64) - want).max()
    err0 = np.abs(x0.cpu().numpy().astype(np.float64) - want0).max()
    print(f"joint step stride {stride} {kind} clamp {clamp} kn {kn}: max err {err:.3e} (x0 {err0:.3e}), bound {bound:.3e}")
    assert err <= bound and err0 <= R.tolerance(L['windows_per_voxel'], max_y)
    assert np.array_equal(got.cpu().numpy()[~covered], x_t[~covered])           # uncovered voxels return x_t ...
    assert not x0.cpu().numpy()[~covered].any()                                 # ... and x0_out = 0
    same = ops.volume_joint_step(*args, x_dev, kx, k0, kn, *clamp, stride, seed, draw, sample, out=x_dev)
    assert same.data_ptr() == x_dev.data_ptr() and torch.equal(x_dev, got)      # in place = out of place, bit for bit


def test_joint_step_initial_state_is_the_anchored_field():
    from diffusioniqt_amd import ops
    shape, seed = (20, 24, 28), 0x123456789
    for draw, sample in ((0, 0), (3, 2)):
        got = ops.volume_joint_init(shape, seed, sample=sample, draw=draw)
        g = [s // 4 for s in shape]
        org = np.array([(4 * a, 4 * b, 4 * c) for a in range(g[0]) for b in range(g[1]) for c in range(g[2])], dtype=np.int32)
        w = ops.anchored_noise(org, 1, 4, *shape, seed, draw=draw, sample=sample)
        field = w.reshape(g[0], g[1], g[2], 4, 4, 4).permute(0, 3, 1, 4, 2, 5).reshape(shape)
        assert torch.equal(got, field)
    with pytest.raises(ValueError, match="seed"):
        ops.volume_joint_init(shape, 1 << 64)


def test_joint_step_argument_errors(step_case):
    from diffusioniqt_amd import ops
    L, y, x_t, taps = step_case[8, 'gaussian']
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    y, slot, taps, x = cu(y), cu(L['slot'].astype(np.int32)), cu(taps.astype(np.float32)), cu(x_t)
    ok = (1.0, 0.5, 0.0, -1.0, 1.0, 1, 8, 0, 1)
    with pytest.raises(ValueError, match="slot names window"):
        ops.volume_joint_step(y[:-1].contiguous(), slot, taps, x, *ok)
    with pytest.raises(ValueError, match="lattice"):
        ops.volume_joint_step(y, slot, taps, x, 1.0, 0.5, 0.0, -1.0, 1.0, 1, 5, 0, 1)
    with pytest.raises(ValueError, match="clamp_mode"):
        ops.volume_joint_step(y, slot, taps, x, 1.0, 0.5, 0.0, -1.0, 1.0, 2, 8, 0, 1)
    with pytest.raises(ValueError, match="draw"):
        ops.volume_joint_step(y, slot, taps, x, 1.0, 0.5, 0.0, -1.0, 1.0, 1, 8, 0, 1 << 32)
    with pytest.raises(ValueError, match="cubic"):
        ops.volume_joint_step(y[:, :, :, :8].contiguous(), slot, taps, x, *ok)
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.volume_joint_step(y, slot, taps, x.transpose(0, 1), *ok)


# ---- G2: the finish kernel against numpy ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('S', [1, 3])
def test_joint_finish_matches_numpy(S):
    from diffusioniqt_amd import ops
    vol = R.shared_volume()
    ref = R.reference(vol, R.shared_cfg(8), lambda x: x, blend='constant')
    covered, background = ref['covered'], ref['background']
    assert (~covered & ~background).any() and background.any() and (covered & ~background).any()
    rng = np.random.default_rng(8)
    xs = rng.standard_normal((S,) + vol.shape).astype(np.float32) * 2
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    slot, v = cu(ref['slot'].astype(np.int32)), cu(vol)
    mean_io = m2 = std = None
    for s in range(S):
        mean_io, m2, std = ops.volume_joint_finish(cu(xs[s]), slot, v, 16, 8, 300.0, 200.0, float(ref['min_val']), float(ref['fill']),
                                                   s, S, mean_io, m2, want_std=S > 1)
        assert (std is not None) == (S > 1 and s == S - 1)
    r = np.where(background, np.float64(ref['min_val']), np.where(covered, xs.astype(np.float64), np.float64(ref['fill'])))
    tol = (S + 3) * 2.0 ** -23 * float(np.abs(xs).max())
    got = mean_io.cpu().numpy()
    err = np.abs(got - r.mean(axis=0)).max()
    print(f"joint finish S = {S}: max |mean - ref| = {err:.3e}, bound {tol:.3e}")
    assert err <= tol
    assert (got[~covered & ~background] == ref['fill']).all() and (got[background] == ref['min_val']).all()
    if S == 1:
        assert m2 is None and np.array_equal(got[covered & ~background], xs[0][covered & ~background])
    else:
        got_s = std.cpu().numpy()
        es = np.abs(got_s - r.std(axis=0, ddof=1)).max()
        print(f"joint finish S = {S}: max |std - ref| = {es:.3e}, bound {2 * tol:.3e}")
        assert es <= 2 * tol and not got_s[~covered | background].any()
        assert got_s[covered & ~background].min() > 0


# ---- G3: the whole chain against the float64 reference ------------------------------------------------------------------------------------
@pytest.mark.parametrize('tiling', [(8, 'gaussian'), (5, 'constant')], ids=['s8-gaussian', 's5-constant'])
@pytest.mark.parametrize('eta', [0.0, 0.5])
@pytest.mark.parametrize('mode', list(MODES))
@pytest.mark.parametrize('objective', ['x_start', 'noise'])
def test_joint_chain_matches_the_float64_reference(shared_vol, objective, mode, eta, tiling):
    stride, blend = tiling
    imagen = stub_imagen(objective, mode)
    ref = chain_ref(imagen, 'shared', stride, objective, mode, eta, blend)
    got = joint_run(imagen, R.shared_cfg(stride), shared_vol, eta, blend)(shared_vol)
    got = check(got, ref, f"joint {objective} {mode} eta {eta} stride {stride} {blend}")
    assert (got[~ref['covered'] & ~ref['background']] == ref['fill']).all() and (got[ref['background']] == ref['min_val']).all()


# ---- G4: tiling invariance on the device ------------------------------------------------------------------------------------------------
def test_joint_chain_does_not_depend_on_the_tiling(shared_vol):
    """With an elementwise network the float64 chain is the same under every tiling (tests/test_volume_joint_host.py, to 1e-12), so two
    device runs differ by at most the sum of their own chain bounds -- at most twice the larger."""
    imagen = stub_imagen('x_start', 'clamp-min')
    runs = {}
    for stride, blend in itertools.product((16, 8, 5), ('constant', 'gaussian')):
        ref = chain_ref(imagen, 'shared', stride, 'x_start', 'clamp-min', 0.5, blend)
        got = joint_run(imagen, R.shared_cfg(stride), shared_vol, 0.5, blend)(shared_vol).cpu().numpy().astype(np.float64)
        runs[stride, blend] = got, ref['covered'] & ~ref['background'], J.chain_bound(ref['windows_per_voxel'], ref['scale'])
    common = np.logical_and.reduce([m for _, m, _ in runs.values()])
    assert common.mean() >= 0.15
    for (ka, (a, _, ba)), (kb, (b, _, bb)) in itertools.combinations(runs.items(), 2):
        err = np.abs(a - b)[common].max()
        print(f"tilings {ka} vs {kb}: max difference {err:.3e}, bound {ba + bb:.3e}")
        assert err <= ba + bb, (ka, kb)


# ---- G5: the tie to the existing path -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('eta', [0.0, 0.5])
@pytest.mark.parametrize('mode', list(MODES))
def test_joint_at_stride_equal_patch_is_the_independent_path(shared_vol, mode, eta):
    """No overlap, unit weights: num / den is exact, every window's chain is its own, and the only freedom left is the operation order
    of the update -- the joint volume equals the blended independent windows at every voxel, bit for bit."""
    from diffusioniqt_amd.inference import VolumeInference
    imagen = stub_imagen('x_start', mode)
    cfg = R.shared_cfg(16)

    def sample_fn(x, noise=None):
        return imagen.sample(batch_size=x.shape[0], start_image_or_video=x, start_at_unet_number=2, use_tqdm=False, sampler='ddim',
                             sample_steps=J.STEPS, eta=eta, noise=noise)[0]
    independent = VolumeInference(cfg, sample_fn, blend='constant', noise='anchored', seed=J.SEED)(shared_vol)
    joint = joint_run(imagen, cfg, shared_vol, eta, 'constant')(shared_vol)
    assert independent.unique().numel() > 1000
    assert torch.equal(joint, independent)


# ---- G6: batching, seed and samples ------------------------------------------------------------------------------------------------------
def test_joint_batching_seed_and_samples(shared_vol):
    imagen = stub_imagen('x_start', 'clamp-min')
    a = joint_run(imagen, R.shared_cfg(5, batch_size=7), shared_vol, 0.5, 'gaussian')(shared_vol)
    b = joint_run(imagen, R.shared_cfg(5, batch_size=3), shared_vol, 0.5, 'gaussian')(shared_vol)
    assert torch.equal(a, b)
    c = joint_run(imagen, R.shared_cfg(5, batch_size=3), shared_vol, 0.5, 'gaussian', seed=J.SEED + 1)(shared_vol)
    assert not torch.equal(b, c)                                                # another seed is another volume
    ref = chain_ref(imagen, 'shared', 8, 'x_start', 'clamp-min', 0.5, 'gaussian', samples=2)
    inf = joint_run(imagen, R.shared_cfg(8), shared_vol, 0.5, 'gaussian', samples=2)
    mean, std = inf(shared_vol, return_std=True)
    check(mean, ref, "joint S = 2 mean")
    std = check(std, ref, "joint S = 2 deviation", key='std', factor=2)
    live = ref['covered'] & ~ref['background']
    assert ref['std'][live].max() > 0.05 and not std[~live].any()
    assert torch.equal(inf(shared_vol), mean)                                   # the mean alone is the same volume


# ---- G7: block mode -----------------------------------------------------------------------------------------------------------------------
def test_joint_block_mode_matches_the_float64_reference():
    imagen = stub_imagen('x_start', 'clamp-min', size=8)
    ref = chain_ref(imagen, 'block', None, 'x_start', 'clamp-min', 0.5, 'gaussian')
    assert ref['kept'] == ref['candidates'] == 27 and ref['covered'].all()
    vol = torch.from_numpy(R.block_volume()).to(DEV)
    check(joint_run(imagen, R.block_cfg(), vol, 0.5, 'gaussian')(vol), ref, "joint block mode P 24 stride 16")


# ---- G8: self-conditioning ----------------------------------------------------------------------------------------------------------------
def test_joint_self_conditioning_reads_the_fused_x0_volume(shared_vol):
    imagen = stub_imagen('x_start', 'clamp-min', unet=J.make_self_cond_unet())
    assert imagen.window_denoiser(sample_steps=J.STEPS).self_cond
    ref = chain_ref(imagen, 'shared', 8, 'x_start', 'clamp-min', 0.5, 'gaussian', net=J.self_cond_stub64, self_cond=True)
    plain = chain_ref(imagen, 'shared', 8, 'x_start', 'clamp-min', 0.5, 'gaussian')
    assert np.abs(ref['mean'] - plain['mean']).max() > 1e-2                     # the self-conditioning term is visible
    check(joint_run(imagen, R.shared_cfg(8), shared_vol, 0.5, 'gaussian')(shared_vol), ref, "joint self-conditioned stride 8")


# ---- G9: a real network -------------------------------------------------------------------------------------------------------------------
def test_joint_with_a_real_network_through_the_trainer():
    from diffusioniqt_amd.imagen_pytorch3D import Imagen, NullUnet
    from diffusioniqt_amd.inference import VolumeInference
    from diffusioniqt_amd.trainer import ImagenTrainer
    from tests.test_gpu_unet import build
    g = load_golden('ddpmA_traj')
    unet, _, _ = build(load_golden('unetA_tiny'), 0)
    configs = {'Data': {'norm': 'z-score'}, 'Train': {'batch_sample': False, 'patch_size_sub': 8, 'pred_obj': 'x_start'}, 'Eval': {'repeat': 1}}
    imagen = Imagen(unets=(NullUnet(), unet), configs=configs, min_bound=float(g['min_bound']), image_sizes=(8, 8), channels=1,
                    pred_objectives='x_start', timesteps=int(g['T']), dynamic_thresholding=False, p2_loss_weight_gamma=0.0,
                    cond_drop_prob=0.0).to(DEV)
    ImagenTrainer.locked = False
    trainer = ImagenTrainer(configs=configs, imagen=imagen, verbose=False)
    vol = torch.from_numpy(np.random.default_rng(12).integers(1, 1000, (20, 24, 28)).astype(np.float32)).to(DEV)   # every window is kept

    def sample_fn(x, noise=None):
        return trainer.sample(batch_size=x.shape[0], start_image_or_video=x, start_at_unet_number=2, sampler='ddim', sample_steps=3,
                              noise=noise)[0]

    def cfg(stride, batch):
        return R.shared_cfg(stride, batch_size=batch, P=8)
    den = trainer.window_denoiser(sampler='ddim', sample_steps=3)
    assert den.num_steps == 3
    # stride = patch, constant blend, the same windows in the same batches: the independent chains, bit for bit
    independent = VolumeInference(cfg(8, 6), sample_fn, blend='constant', noise='anchored', seed=4)(vol)
    joint = VolumeInference(cfg(8, 6), den, blend='constant', noise='anchored', joint=True, seed=4)(vol)
    assert torch.equal(joint, independent) and joint.unique().numel() > 1000
    # overlapping windows: finite, reproducible, and not what blending finished patches gives
    runs = [VolumeInference(cfg(4, 30), den, blend='gaussian', noise='anchored', joint=True, seed=4)(vol) for _ in range(2)]
    assert torch.isfinite(runs[0]).all() and torch.equal(runs[0], runs[1])
    blended = VolumeInference(cfg(4, 30), sample_fn, blend='gaussian', noise='anchored', seed=4)(vol)
    assert not torch.equal(runs[0], blended)
