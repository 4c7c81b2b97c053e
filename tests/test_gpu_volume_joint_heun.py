"""The EDM volume path on a real MI355X against the float64 specification of tests/volume_joint_heun_reference.py: the phases of
``ops.volume_joint_heun`` on their own (against float64 and, bit for bit, against the same update assembled from the single-purpose
ops), the whole chain of ``VolumeInference(joint=True)`` with ``ElucidatedImagen.window_denoiser`` and the elementwise stub network,
its bit-for-bit tie to the independent windows of ``ElucidatedImagen.sample(noise=source)`` at stride = patch (stub, Unet3D and the
Conv3d U-Net through the trainer), volume-anchored noise for the EDM sampler without ``joint``, batching / seed / samples, block
mode, self-conditioning, and overlapping windows with a real network.

Chain bound: ``volume_joint_heun_reference.chain_bound``, derived in that module's docstring; tests/test_volume_joint_heun_host.py holds
an fp32 emulation of the chain to half of it and the bound itself to 1e-3 of the signal's peak-to-peak."""
import itertools
import json

import numpy as np
import pytest
import torch

from tests import volume_blend_reference as R
from tests import volume_joint_heun_reference as HN
from tests import volume_joint_reference as J
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
_REF = {}


def _ref(key, make):
    """One float64 reference per case, shared by the tests that need it and never modified."""
    if key not in _REF:
        _REF[key] = make()
        for v in _REF[key].values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return _REF[key]


def chain_ref(vol_name, stride, dynamic, churn, blend, samples=1, self_cond=False):
    vol, cfg = (R.block_volume(), R.block_cfg()) if vol_name == 'block' else (R.shared_volume(), R.shared_cfg(stride))
    return _ref((vol_name, stride, dynamic, churn, blend, samples, self_cond), lambda: HN.joint_reference(
        vol, cfg, HN.tables(HN.HP, HN.CHURN[churn]), blend, dynamic, samples=samples, self_cond=self_cond))


def joint_run(elu, cfg, blend, **kw):
    from diffusioniqt_amd.inference import VolumeInference
    return VolumeInference(cfg, elu.window_denoiser(), blend=blend, noise='anchored', joint=True, seed=kw.pop('seed', HN.SEED), **kw)


def independent_run(elu, cfg, blend, P, **kw):
    """Every window's own chain through ``ElucidatedImagen.sample`` with the volume-anchored source, finished patches blended."""
    from diffusioniqt_amd.inference import VolumeInference

    def sample_fn(x, noise=None):
        return elu.sample(batch_size=x.shape[0], video_frames=P, start_image_or_video=x, start_at_unet_number=2, use_tqdm=False,
                          noise=noise)
    return VolumeInference(cfg, sample_fn, blend=blend, noise='anchored', seed=kw.pop('seed', HN.SEED), **kw)


def check(got, ref, what, key='mean', factor=1):
    got = got.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == ref[key].shape and np.isfinite(got).all()
    bound = factor * ref['bound']
    err = np.abs(got.astype(np.float64) - ref[key]).max()
    print(f"{what}: max |{key} - ref| = {err:.3e}, bound {bound:.3e} (n = {ref['windows_per_voxel']}, largest |state| {ref['state_max']:.2f})")
    assert err <= bound, what
    return got


@pytest.fixture(scope="module")
def shared_vol():
    return torch.from_numpy(R.shared_volume()).to(DEV)


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def field(shape, seed, draw, sample):
    """Draw ``draw`` of the anchored field over a whole volume, assembled from ``ops.anchored_noise`` windows of edge 4."""
    from diffusioniqt_amd import ops
    g = [s // 4 for s in shape]
    org = np.array([(4 * a, 4 * b, 4 * c) for a in range(g[0]) for b in range(g[1]) for c in range(g[2])], dtype=np.int32)
    w = ops.anchored_noise(org, 1, 4, *shape, seed, draw=draw, sample=sample)
    return w.reshape(g[0], g[1], g[2], 4, 4, 4).permute(0, 3, 1, 4, 2, 5).reshape(shape).contiguous()


def axpby(terms):
    """``ops.axpby3`` on whole volumes: sum of k_j v_j over up to three (k, volume) terms, in the kernel's order."""
    from diffusioniqt_amd import ops
    vec = lambda k: torch.full((1,), float(k), device=DEV)
    vs = [v.reshape(1, -1) for _, v in terms] + [None] * (3 - len(terms))
    ks = [vec(k) for k, _ in terms] + [None] * (3 - len(terms))
    return ops.axpby3(*vs, *ks).view(terms[0][1].shape)


# ---- G1: the phases against the float64 specification and against the single-purpose ops -------------------------------------------------
@pytest.fixture(scope="module")
def step_case():
    """Per (stride, kind): two sets of predictions for the kept windows of the shared volume, the three state volumes, the layout."""
    rng = np.random.default_rng(16)
    vol = R.shared_volume()
    out = {}
    for stride, kind in itertools.product((8, 5), ('gaussian', 'constant')):
        L = J.layout(vol, R.shared_cfg(stride))
        assert (L['slot'] < 0).any()
        ys = [rng.standard_normal((L['kept'].shape[0], 16, 16, 16)).astype(np.float32) * 2 for _ in range(2)]
        out[stride, kind] = (L, ys, rng.standard_normal(vol.shape).astype(np.float32) * 3, R.taps_of(16, kind))
    return out


@pytest.mark.parametrize('kc', [0.0, 0.625])
@pytest.mark.parametrize('clamp', [(-1., 1., 1), (-float('inf'), float('inf'), 1)], ids=['box', 'none'])
@pytest.mark.parametrize('kind', ['gaussian', 'constant'])
@pytest.mark.parametrize('stride', [8, 5])
def test_heun_phases_match_reference_and_the_single_purpose_ops(step_case, stride, kind, clamp, kc):
    """Phase 1 then phase 2 on one state.  Bounds per voxel, with tol = the blend's own bound on max|y|, u = 2^-24 and |n| < 6:
    xn: |b| tol + 3 u (|a| max|xh| + |b| max|y|) (two products, one sum);  x0: tol;
    xh: |d| tol + |c| (bound of xn) + |b| tol + 7 u (|a| max|xh| + (|b| + |d|) max|y| + |c| max|xn|) (four products, three sums on exact
    inputs, the device's own x0 / xn being within tol / the bound above of the float64 ones) + u (max|x| + 6 |kc|) + 2e-5 |kc| (the
    churn's product, sum and the normals' bound of tests/test_gpu_anchored_noise.py)."""
    from diffusioniqt_amd import ops
    L, ys, xh0, taps = step_case[stride, kind]
    (a1, b1), (a2, b2, c2, d2) = (0.4375, 0.5625), (0.71875, 0.28125, -0.8125, 0.8125)
    seed, draw, sample = 0x123456789, 5, 2
    u = 2.0 ** -24
    c64 = J.clamp_of(*clamp)
    shape = xh0.shape
    x0a, covered = HN.fuse(c64(ys[0].astype(np.float64)), L['slot'], taps, stride, shape)
    assert covered.any() and (~covered).any()
    want_n, _ = HN.heun_phase1(x0a, covered, xh0.astype(np.float64), a1, b1)
    x0b, _ = HN.fuse(c64(ys[1].astype(np.float64)), L['slot'], taps, stride, shape)
    want_h, _ = HN.heun_phase2(x0b, covered, xh0.astype(np.float64), want_n, x0a, (a2, b2, c2, d2), kc, J.normals(shape, seed, draw, sample))
    slot, tp = cu(L['slot'].astype(np.int32)), cu(taps.astype(np.float32))
    y0, y1 = cu(ys[0]), cu(ys[1])
    xh, xn, x0 = cu(xh0), torch.full(shape, 7.0, device=DEV), torch.full(shape, 7.0, device=DEV)
    # the same updates from the existing ops: the fused prediction is the multistep kernel's x0_out (the same walk), the sums are axpby3's
    _, f0 = ops.volume_joint_multistep(y0, slot, tp, xh, None, 0.0, 1.0, 0.0, *clamp, stride)
    _, f1 = ops.volume_joint_multistep(y1, slot, tp, xh, None, 0.0, 1.0, 0.0, *clamp, stride)
    asm_n = axpby([(a1, xh), (b1, f0)])
    asm_x = axpby([(1.0, axpby([(a2, xh), (b2, f0), (c2, asm_n)])), (d2, f1)])
    asm_h = axpby([(1.0, asm_x), (kc, field(shape, seed, draw, sample))])
    cov = cu(covered)

    max_y, max_h = float(np.abs(ys).max()), float(np.abs(xh0).max())
    tol = R.tolerance(L['windows_per_voxel'], max_y)
    r = ops.volume_joint_heun(y0, slot, tp, xh, xn, x0, 1, (a1, b1), 0.0, *clamp, stride)
    assert all(t.data_ptr() == w.data_ptr() for t, w in zip(r, (xh, xn, x0))) and torch.equal(xh, cu(xh0))
    bound_n = abs(b1) * tol + 3 * u * (abs(a1) * max_h + abs(b1) * max_y)
    err_n = np.abs(xn.cpu().numpy().astype(np.float64) - want_n).max()
    err_0 = np.abs(x0.cpu().numpy().astype(np.float64) - x0a).max()
    print(f"heun phase 1 stride {stride} {kind} clamp {clamp}: xn {err_n:.3e} (bound {bound_n:.3e}), x0 {err_0:.3e} (bound {tol:.3e})")
    assert err_n <= bound_n and err_0 <= tol
    assert torch.equal(xn[~cov], xh[~cov]) and not x0[~cov].any()               # uncovered: xn = xh, x0 = 0
    assert torch.equal(xn[cov], asm_n[cov]) and torch.equal(x0[cov], f0[cov])   # the axpby3 sequence, bit for bit

    max_n = float(np.abs(want_n).max())
    ops.volume_joint_heun(y1, slot, tp, xh, xn, x0, 2, (a2, b2, c2, d2), kc, *clamp, stride, seed, draw, sample)
    bound_h = abs(d2) * tol + abs(c2) * bound_n + abs(b2) * tol + 7 * u * (abs(a2) * max_h + (abs(b2) + abs(d2)) * max_y + abs(c2) * max_n) \
        + u * (float(np.abs(want_h).max()) + 6 * abs(kc)) + 2e-5 * abs(kc)
    err_h = np.abs(xh.cpu().numpy().astype(np.float64) - want_h).max()
    err_0 = np.abs(x0.cpu().numpy().astype(np.float64) - x0b).max()
    print(f"heun phase 2 stride {stride} {kind} clamp {clamp} kc {kc}: xh {err_h:.3e} (bound {bound_h:.3e}), x0 {err_0:.3e} (bound {tol:.3e})")
    assert err_h <= bound_h and err_0 <= tol
    assert torch.equal(xh[~cov], cu(xh0)[~cov]) and not x0[~cov].any()          # uncovered: xh is left, x0 = 0
    assert torch.equal(xn, asm_n.where(cov, cu(xh0)))                           # phase 2 does not write xn
    assert torch.equal(xh[cov], asm_h[cov]) and torch.equal(x0[cov], f1[cov])


def test_heun_argument_errors(step_case):
    from diffusioniqt_amd import ops
    L, ys, xh0, taps = step_case[8, 'gaussian']
    y, slot, tp, xh = cu(ys[0]), cu(L['slot'].astype(np.int32)), cu(taps.astype(np.float32)), cu(xh0)
    xn, x0 = torch.empty_like(xh), torch.empty_like(xh)
    ok = (-1.0, 1.0, 1, 8)
    with pytest.raises(ValueError, match="phase"):
        ops.volume_joint_heun(y, slot, tp, xh, xn, x0, 0, (1.0, 0.5), 0.0, *ok)
    with pytest.raises(ValueError, match="coefficients"):
        ops.volume_joint_heun(y, slot, tp, xh, xn, x0, 2, (1.0, 0.5), 0.0, *ok)
    with pytest.raises(ValueError, match="slot names window"):
        ops.volume_joint_heun(y[:-1].contiguous(), slot, tp, xh, xn, x0, 1, (1.0, 0.5), 0.0, *ok)
    with pytest.raises(ValueError, match="lattice"):
        ops.volume_joint_heun(y, slot, tp, xh, xn, x0, 1, (1.0, 0.5), 0.0, -1.0, 1.0, 1, 5)
    with pytest.raises(ValueError, match="clamp_mode"):
        ops.volume_joint_heun(y, slot, tp, xh, xn, x0, 1, (1.0, 0.5), 0.0, -1.0, 1.0, 2, 8)
    with pytest.raises(ValueError, match="draw"):
        ops.volume_joint_heun(y, slot, tp, xh, xn, x0, 2, (1.0, 0.5, 0.25, 0.25), 0.5, *ok, 0, 1 << 32)
    with pytest.raises(ValueError, match="cubic"):
        ops.volume_joint_heun(y[:, :, :, :8].contiguous(), slot, tp, xh, xn, x0, 1, (1.0, 0.5), 0.0, *ok)
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.volume_joint_heun(y, slot, tp, xh.transpose(0, 1), xn, x0, 1, (1.0, 0.5), 0.0, *ok)
    with pytest.raises(ValueError, match="xn must be"):
        ops.volume_joint_heun(y, slot, tp, xh, xn[:-1].contiguous(), x0, 1, (1.0, 0.5), 0.0, *ok)
    with pytest.raises(ValueError, match="three different"):
        ops.volume_joint_heun(y, slot, tp, xh, xn, xn, 1, (1.0, 0.5), 0.0, *ok)
    with pytest.raises(ValueError, match="draw"):
        ops.volume_joint_heun_init((20, 24, 28), 1.0, 0.5, 0, draw=(1 << 32) - 1)


# ---- G2: phase 0 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kc', [0.0, 0.625])
def test_heun_initial_state_is_the_axpby3_sequence_on_the_anchored_field(kc):
    from diffusioniqt_amd import ops
    shape, seed, sigma0 = (20, 24, 28), 0x123456789, 1.4999995231628418
    for draw, sample in ((0, 0), (3, 2)):
        got = ops.volume_joint_heun_init(shape, sigma0, kc, seed, draw=draw, sample=sample)
        images = axpby([(sigma0, field(shape, seed, draw, sample))])
        want = axpby([(1.0, images), (kc, field(shape, seed, draw + 1, sample))])
        assert torch.equal(got, want) and got.unique().numel() > 1000


# ---- G3: the whole chain against the float64 reference ------------------------------------------------------------------------------------
@pytest.mark.parametrize('tiling', [(8, 'gaussian'), (5, 'constant')], ids=['s8-gaussian', 's5-constant'])
@pytest.mark.parametrize('churn', list(HN.CHURN))
@pytest.mark.parametrize('dynamic', [False, True], ids=['static', 'dynamic'])
def test_heun_chain_matches_the_float64_reference(shared_vol, dynamic, churn, tiling):
    stride, blend = tiling
    elu = HN.make_elucidated(churn, dynamic).to(DEV)
    ref = chain_ref('shared', stride, dynamic, churn, blend)
    got = joint_run(elu, R.shared_cfg(stride), blend)(shared_vol)
    got = check(got, ref, f"joint Heun {'dynamic' if dynamic else 'static'} {churn} stride {stride} {blend}")
    assert (got[~ref['covered'] & ~ref['background']] == ref['fill']).all() and (got[ref['background']] == ref['min_val']).all()


# ---- G4: the tie to the per-window sampler at stride = patch ---------------------------------------------------------------------------------
@pytest.mark.parametrize('churn', list(HN.CHURN))
@pytest.mark.parametrize('dynamic', [False, True], ids=['static', 'dynamic'])
def test_heun_at_stride_equal_patch_is_the_independent_path(shared_vol, dynamic, churn):
    """No overlap, unit weights: num / den is exact, every window's chain is its own, and the only freedom left is the operation order
    of the updates -- the joint volume equals the blended independent windows at every voxel, bit for bit."""
    elu = HN.make_elucidated(churn, dynamic).to(DEV)
    cfg = R.shared_cfg(16)
    independent = independent_run(elu, cfg, 'constant', 16)(shared_vol)
    joint = joint_run(elu, cfg, 'constant')(shared_vol)
    assert independent.unique().numel() > 1000
    assert torch.equal(joint, independent)


def _real_volume():
    return torch.from_numpy(np.random.default_rng(12).integers(1, 1000, (20, 24, 28)).astype(np.float32)).to(DEV)   # every window is kept


def test_heun_tie_with_a_real_unet3d():
    from diffusioniqt_amd.inference import VolumeInference
    from tests.test_gpu_family_b import make_edm
    kw = {k: (tuple(v) if isinstance(v, list) else v) for k, v in json.loads(str(load_golden('unet3d_tiny')['kwargs'])).items()}
    elu = make_edm(kw, 3)
    vol, cfg = _real_volume(), R.shared_cfg(8, batch_size=6, P=8)
    den = elu.window_denoiser()
    assert den.num_steps == 3 and den.draw_base == 1
    independent = independent_run(elu, cfg, 'constant', 8, seed=4)(vol)
    joint = VolumeInference(cfg, den, blend='constant', noise='anchored', joint=True, seed=4)(vol)
    assert torch.equal(joint, independent) and joint.unique().numel() > 1000


def test_heun_with_the_conv3d_unet_through_the_trainer():
    """``ImagenTrainer.window_denoiser`` on an EDM trainer: the tie at stride = patch, then overlapping windows -- finite, identical on a
    second run, and not what blending finished patches gives."""
    from diffusioniqt_amd.elucidated_imagen import ElucidatedImagen
    from diffusioniqt_amd.imagen_pytorch3D import NullUnet
    from diffusioniqt_amd.inference import VolumeInference
    from diffusioniqt_amd.trainer import ImagenTrainer
    from tests.test_gpu_unet import build
    unet, _, _ = build(load_golden('unetA_tiny'), 0)
    configs = {'Data': {'norm': 'z-score'}, 'Train': {'batch_sample': False, 'patch_size_sub': 8, 'pred_obj': 'x_start'}, 'Eval': {'repeat': 1}}
    elu = ElucidatedImagen(unets=(NullUnet(), unet), image_sizes=(8, 8), channels=1, condition_on_text=False, auto_normalize_img=False,
                           cond_drop_prob=0.0, num_sample_steps=3, dynamic_thresholding=False).to(DEV)
    ImagenTrainer.locked = False
    trainer = ImagenTrainer(configs=configs, imagen=elu, verbose=False)
    vol = _real_volume()

    def sample_fn(x, noise=None):
        return trainer.sample(batch_size=x.shape[0], video_frames=8, start_image_or_video=x, start_at_unet_number=2, noise=noise)

    def cfg(stride, batch):
        return R.shared_cfg(stride, batch_size=batch, P=8)
    den = trainer.window_denoiser()
    assert den.heun and den.num_steps == 3
    independent = VolumeInference(cfg(8, 6), sample_fn, blend='constant', noise='anchored', seed=4)(vol)
    joint = VolumeInference(cfg(8, 6), den, blend='constant', noise='anchored', joint=True, seed=4)(vol)
    assert torch.equal(joint, independent) and joint.unique().numel() > 1000
    runs = [VolumeInference(cfg(4, 30), den, blend='gaussian', noise='anchored', joint=True, seed=4)(vol) for _ in range(2)]
    assert torch.isfinite(runs[0]).all() and torch.equal(runs[0], runs[1])
    blended = VolumeInference(cfg(4, 30), sample_fn, blend='gaussian', noise='anchored', seed=4)(vol)
    assert not torch.equal(runs[0], blended)


# ---- G5: anchored noise for the EDM sampler without `joint` -------------------------------------------------------------------------------
def test_edm_sampler_takes_the_anchored_source(shared_vol):
    from diffusioniqt_amd import ops
    from diffusioniqt_amd.inference import AnchoredNoise
    elu = HN.make_elucidated('churn-on', False).to(DEV)
    a = independent_run(elu, R.shared_cfg(8, batch_size=7), 'gaussian', 16)(shared_vol)
    b = independent_run(elu, R.shared_cfg(8, batch_size=3), 'gaussian', 16)(shared_vol)
    assert torch.equal(a, b) and a.unique().numel() > 1000                      # the blended volume does not depend on the batching
    shape = tuple(shared_vol.shape)
    org = J.layout(R.shared_volume(), R.shared_cfg(8))['kept'][:5].astype(np.int32)
    x, _ = ops.patch_gather(shared_vol, cu(org), 16, 300.0, 200.0)
    kw = dict(batch_size=5, video_frames=16, start_image_or_video=x, start_at_unet_number=2, use_tqdm=False)
    by_source = elu.sample(noise=AnchoredNoise(shape, HN.SEED).source(org, 16), **kw)
    draws = [ops.anchored_noise(org, 1, 16, *shape, HN.SEED, draw=k) for k in range(HN.HP['num_sample_steps'] + 2)]
    by_list = elu.sample(noise=draws, **kw)
    assert torch.equal(by_source, by_list) and by_source.unique().numel() > 1000


# ---- G6: batching, seed and samples ------------------------------------------------------------------------------------------------------
def test_heun_batching_seed_and_samples(shared_vol):
    elu = HN.make_elucidated('churn-on', False).to(DEV)
    a = joint_run(elu, R.shared_cfg(5, batch_size=7), 'gaussian')(shared_vol)
    b = joint_run(elu, R.shared_cfg(5, batch_size=3), 'gaussian')(shared_vol)
    assert torch.equal(a, b)
    c = joint_run(elu, R.shared_cfg(5, batch_size=3), 'gaussian', seed=HN.SEED + 1)(shared_vol)
    assert not torch.equal(b, c)                                                # another seed is another volume
    ref = chain_ref('shared', 8, False, 'churn-on', 'gaussian', samples=2)
    inf = joint_run(elu, R.shared_cfg(8), 'gaussian', samples=2)
    mean, std = inf(shared_vol, return_std=True)
    check(mean, ref, "joint Heun S = 2 mean")
    std = check(std, ref, "joint Heun S = 2 deviation", key='std', factor=2)
    live = ref['covered'] & ~ref['background']
    assert ref['std'][live].max() > 0.05 and std[live].max() > 0.05 and not std[~live].any()
    assert torch.equal(inf(shared_vol), mean)                                   # the mean alone is the same volume


# ---- G7: block mode -----------------------------------------------------------------------------------------------------------------------
def test_heun_block_mode_matches_the_float64_reference():
    elu = HN.make_elucidated('churn-on', False, size=8).to(DEV)
    ref = chain_ref('block', None, False, 'churn-on', 'gaussian')
    assert ref['kept'] == ref['candidates'] == 27 and ref['covered'].all()
    vol = torch.from_numpy(R.block_volume()).to(DEV)
    check(joint_run(elu, R.block_cfg(), 'gaussian')(vol), ref, "joint Heun block mode P 24 stride 16")


# ---- G8: self-conditioning ----------------------------------------------------------------------------------------------------------------
def test_heun_self_conditioning_reads_the_fused_x0_volume(shared_vol):
    elu = HN.make_elucidated('churn-on', False, self_cond=True).to(DEV)
    assert elu.window_denoiser().self_cond
    ref = chain_ref('shared', 8, False, 'churn-on', 'gaussian', self_cond=True)
    plain = chain_ref('shared', 8, False, 'churn-on', 'gaussian')
    assert np.abs(ref['mean'] - plain['mean']).max() > 1e-2                     # the self-conditioning term is visible
    check(joint_run(elu, R.shared_cfg(8), 'gaussian')(shared_vol), ref, "joint Heun self-conditioned stride 8")
