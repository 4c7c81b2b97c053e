"""DDPM inpainting on the joint volume state on a real MI355X: every phase and flag combination of ``ops.volume_joint_step_inpaint``
bit for bit against the same update assembled from ``ops.volume_joint_step``, ``ops.anchored_noise``, ``ops.axpby3``, ``ops.q_sample``
and ``ops.mask_blend``; the whole chain of ``VolumeInference(joint=True, inpaint=...)`` with the ancestral denoiser against the float64
specification of tests/volume_joint_ddpm_inpaint_reference.py; its bit-for-bit tie to independently inpainted windows
(``Imagen.sample(noise=source, inpaint_images=...)``) at stride = patch -- the stub network at R = 1, 2, 3, static and dynamic, a
self-conditioning stub, the Conv3d U-Net through ``ImagenTrainer``; and ``paste_known``.

Chain bound: ``volume_joint_ddpm_inpaint_reference.chain_bound``; tests/test_volume_joint_ddpm_inpaint_host.py holds an fp32 emulation
of the chain to it and the bound itself to 1e-3 of the signal's peak-to-peak for every case compared here."""
import numpy as np
import pytest
import torch

from tests import volume_blend_reference as R
from tests import volume_joint_ddpm_inpaint_reference as DP
from tests import volume_joint_inpaint_reference as IP
from tests import volume_joint_reference as J
from tests.conftest import load_golden
from tests.test_gpu_volume_joint import stub_imagen
from tests.test_gpu_volume_joint_heun import axpby, cu, field
from tests.test_volume_joint_ddpm_inpaint_host import CASES, IDS, MODES, tabs

pytestmark = pytest.mark.gpu
DEV = "cuda"
IMAGEN = {'static': 'clamp-min', 'dynamic': 'dynamic'}                       # the modes of tests/test_gpu_volume_joint.py
_REF = {}


def chain_ref(mode, stride, resample, blend, self_cond=False, paste_known=False):
    """One float64 reference per case, shared by the tests that need it and never modified."""
    key = (mode, stride, resample, blend, self_cond, paste_known)
    if key not in _REF:
        clamp, dyn = MODES[mode]
        known, mask = IP.inpaint_inputs()
        _REF[key] = DP.joint_reference(R.shared_volume(), R.shared_cfg(stride), tabs(), 'x_start', clamp, blend, known, mask, resample,
                                       dyn=dyn, self_cond=self_cond, paste_known=paste_known)
        for v in _REF[key].values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return _REF[key]


def joint_run(den, cfg, blend, inpaint, resample, **kw):
    from diffusioniqt_amd.inference import VolumeInference
    return VolumeInference(cfg, den, blend=blend, noise='anchored', joint=True, seed=kw.pop('seed', DP.SEED), inpaint=inpaint,
                           inpaint_resample_times=resample, **kw)


def independent_run(sample, cfg, blend, inpaint, resample, steps, **kw):
    """Every window's own inpainting chain through ``sample`` with the volume-anchored source, finished patches blended.  ``Imagen``
    takes its masks with the channel axis, as the reference multiplies them into the image."""
    from diffusioniqt_amd.inference import VolumeInference

    def sample_fn(x, noise=None, inpaint_masks=None, **inp):
        return sample(batch_size=x.shape[0], start_image_or_video=x, start_at_unet_number=2, noise=noise, sampler='ddpm', sample_steps=steps,
                      inpaint_masks=inpaint_masks[:, None], **inp)[0]
    return VolumeInference(cfg, sample_fn, blend=blend, noise='anchored', seed=kw.pop('seed', DP.SEED), inpaint=inpaint,
                           inpaint_resample_times=resample, **kw)


def check(got, ref, what):
    got = got.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == ref['mean'].shape and np.isfinite(got).all()
    err = np.abs(got.astype(np.float64) - ref['mean']).max()
    print(f"{what}: max |mean - ref| = {err:.3e}, bound {ref['bound']:.3e} (n = {ref['windows_per_voxel']}, largest |state| {ref['state']:.2f})")
    assert err <= ref['bound'], what
    return got


@pytest.fixture(scope="module")
def shared_vol():
    return torch.from_numpy(R.shared_volume()).to(DEV)


@pytest.fixture(scope="module")
def shared_inpaint():
    known, mask = IP.inpaint_inputs()
    return torch.from_numpy(known).to(DEV), torch.from_numpy(mask).to(DEV)


# ---- G1: the phases and flags against the single-purpose ops ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def step_case():
    """Per (stride, kind): predictions for the kept windows of the shared volume (16-voxel windows at strides 8 and 5, windows dropped by
    the 5 % rule, uncovered voxels), a state, and eight covered voxels with x = -0 and every covering prediction +0 -- as
    tests/test_gpu_volume_joint_bits.py plants them: with kx > 0 > k0 the step's fused part is -0 there."""
    rng = np.random.default_rng(23)
    vol = R.shared_volume()
    known, mask = IP.inpaint_inputs()
    out = {}
    for stride in (8, 5):
        for kind in ('gaussian', 'constant'):
            L = J.layout(vol, R.shared_cfg(stride))
            slot = L['slot']
            assert (slot < 0).any()
            y = rng.standard_normal((L['kept'].shape[0], 16, 16, 16)).astype(np.float32) * 2
            x = rng.standard_normal(vol.shape).astype(np.float32) * 3
            cov = np.zeros(vol.shape, dtype=bool)
            for g in np.ndindex(*slot.shape):
                if slot[g] >= 0:
                    cov[tuple(slice(a * stride, a * stride + 16) for a in g)] = True
            assert cov.any() and not cov.all()
            free, held = np.flatnonzero(cov & ~mask), np.flatnonzero(cov & mask)
            zero = [tuple(int(c) for c in np.unravel_index(idx[len(idx) * (2 * k + 1) // 9], vol.shape)) for idx in (free, held)
                    for k in range(4)]                                           # four unmasked, then four masked
            for v in zero:
                x[v] = -0.0
                for g in np.ndindex(*slot.shape):
                    o = tuple(c - a * stride for c, a in zip(v, g))
                    if slot[g] >= 0 and all(0 <= i < 16 for i in o):
                        y[(slot[g],) + o] = 0.0
            out[stride, kind] = dict(L=L, y=y, x=x, covered=cov, zero=zero, taps=R.taps_of(16, kind).astype(np.float32))
    return out


KX, K0 = 0.8125, -0.9375
KR, Q = (0.625, 0.78125), (0.375, 0.90625)
SEED, DRAW, DRAW_R, DRAW_Q, SAMPLE = 0x123456789, 5, 6, 7, 2


def q_volume(known, al, sg, n):
    from diffusioniqt_amd import ops
    vec = lambda k: torch.full((1,), float(k), device=DEV)
    return ops.q_sample(known.reshape(1, -1), n.reshape(1, -1), vec(al), vec(sg)).view(known.shape)


@pytest.mark.parametrize('flags', [0, 1, 2, 3])
@pytest.mark.parametrize('kind', ['gaussian', 'constant'])
@pytest.mark.parametrize('stride', [8, 5])
def test_step_inpaint_is_the_assembly_of_the_single_purpose_ops(step_case, stride, kind, flags):
    """Every voxel -- masked, uncovered and the planted zeros included -- for kn != 0, kn = +0 (the fused part -0 plus the +0 product:
    +0) and kn = -0 (the product is -0 too: u = -0, and the selection of an unmasked voxel keeps that sign)."""
    from diffusioniqt_amd import ops
    c = step_case[stride, kind]
    known, mask = IP.inpaint_inputs()
    kn_d, mk_b, mk_f, cov = cu(known), cu(mask.astype(np.uint8)), cu(mask.astype(np.float32)), cu(c['covered'])
    w = (cu(c['y']), cu(c['L']['slot'].astype(np.int32)), cu(c['taps']))
    shape = c['x'].shape
    n_r, n_q = field(shape, SEED, DRAW_R, SAMPLE), field(shape, SEED, DRAW_Q, SAMPLE)
    for kn, clamp in ((0.625, (-1., 1., 1)), (0.0, (-0.75, 0., 0)), (-0.0, (-float('inf'), float('inf'), 1))):
        x0_want = torch.full(shape, 7.0, device=DEV)
        u = ops.volume_joint_step(*w, cu(c['x']), KX, K0, kn, *clamp, stride, SEED, DRAW, SAMPLE, x0_out=x0_want)
        t = axpby([(KR[0], u), (KR[1], n_r)]) if flags & 1 else u
        t = ops.mask_blend(t, q_volume(kn_d, *Q, n_q), mk_f) if flags & 2 else t
        want = t.where(cov, cu(c['x']))                                          # an uncovered voxel keeps its state
        for with_x0 in (True, False):
            x, x0 = cu(c['x']), torch.full(shape, 7.0, device=DEV) if with_x0 else None
            got = ops.volume_joint_step_inpaint(*w, x, kn_d, mk_b, flags, KX, K0, kn, KR, Q, *clamp, stride, SEED, DRAW, DRAW_R, DRAW_Q,
                                                SAMPLE, x0_out=x0)
            assert got.data_ptr() == x.data_ptr()
            assert torch.equal(x.view(torch.int32), want.view(torch.int32)), (kn, with_x0)
            assert x0 is None or torch.equal(x0.view(torch.int32), x0_want.view(torch.int32))
        signs = [bool(np.signbit(v)) for v in (x.cpu().numpy()[z] for z in c['zero'])]
        if kn == 0 and not flags & 1:                                            # kn = +0 / -0, no re-noise: the planted zeros stay zeros
            free_sign = bool(np.signbit(kn))
            assert all(x.cpu().numpy()[z] == 0 for z in c['zero'][:4]) and signs[:4] == [free_sign] * 4
            if not flags & 2:
                assert signs[4:] == [free_sign] * 4
        if flags & 2:                                                            # masked and covered: alpha known + sigma n, whatever u is
            both = cov & cu(mask)
            assert both.sum() > 1000 and torch.equal(x[both], q_volume(kn_d, *Q, n_q)[both])
        assert not torch.equal(x, cu(c['x'])) and x.unique().numel() > 1000
    assert torch.equal(ops.volume_joint_step_inpaint(*w, cu(c['x']), kn_d, cu(mask), flags, KX, K0, 0.625, KR, Q, -1., 1., 1, stride, SEED,
                                                     DRAW, DRAW_R, DRAW_Q, SAMPLE), ops.volume_joint_step_inpaint(
        *w, cu(c['x']), kn_d, mk_b, flags, KX, K0, 0.625, KR, Q, -1., 1., 1, stride, SEED, DRAW, DRAW_R, DRAW_Q, SAMPLE))     # a bool mask


def test_step_inpaint_initial_state_is_the_field_under_the_first_paste():
    from diffusioniqt_amd import ops
    small = dict(shape=(20, 24, 28), box=((3, 15), (5, 19), (10, 22)))
    known, mask = IP.inpaint_inputs(**small)
    kn_d, mk = cu(known), cu(mask)
    for draw, draw_q, sample in ((0, 1, 0), (3, 9, 2)):
        got = ops.volume_joint_step_inpaint_init(kn_d, mk, *Q, SEED, draw=draw, draw_q=draw_q, sample=sample)
        n, n_q = field(small['shape'], SEED, draw, sample), field(small['shape'], SEED, draw_q, sample)
        want = ops.mask_blend(n, q_volume(kn_d, *Q, n_q), mk.float())
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and got.unique().numel() > 1000
        assert torch.equal(got[~mk], ops.volume_joint_init(small['shape'], SEED, sample=sample, draw=draw)[~mk])


def test_step_inpaint_argument_errors(step_case):
    from diffusioniqt_amd import ops
    c = step_case[8, 'gaussian']
    known, mask = IP.inpaint_inputs()
    y, slot, tp, x = cu(c['y']), cu(c['L']['slot'].astype(np.int32)), cu(c['taps']), cu(c['x'])
    kn, mk = cu(known), cu(mask)
    ok = (KX, K0, 0.5, KR, Q, -1.0, 1.0, 1, 8, 0, 2)
    with pytest.raises(ValueError, match="flags"):
        ops.volume_joint_step_inpaint(y, slot, tp, x, kn, mk, 4, *ok)
    with pytest.raises(ValueError, match="mask"):
        ops.volume_joint_step_inpaint(y, slot, tp, x, kn, mk.float(), 3, *ok)
    with pytest.raises(ValueError, match="known"):
        ops.volume_joint_step_inpaint(y, slot, tp, x, kn[:-1].contiguous(), mk, 3, *ok)
    with pytest.raises(ValueError, match="lattice"):
        ops.volume_joint_step_inpaint(y, slot, tp, x, kn, mk, 3, KX, K0, 0.5, KR, Q, -1.0, 1.0, 1, 5, 0, 2)
    with pytest.raises(ValueError, match="draw"):
        ops.volume_joint_step_inpaint(y, slot, tp, x, kn, mk, 3, *ok, draw_q=1 << 32)
    with pytest.raises(ValueError, match="x0_out"):
        ops.volume_joint_step_inpaint(y, slot, tp, x, kn, mk, 3, *ok, x0_out=x[:-1].contiguous())
    with pytest.raises(ValueError, match="draw"):
        ops.volume_joint_step_inpaint_init(kn, mk, *Q, 0, draw=1 << 32)


# ---- G2: the whole chain against the float64 reference ------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode,resample,tiling', CASES, ids=IDS)
def test_inpaint_chain_matches_the_float64_reference(shared_vol, shared_inpaint, mode, resample, tiling):
    stride, blend = tiling
    imagen = stub_imagen('x_start', IMAGEN[mode])
    ref = chain_ref(mode, stride, resample, blend)
    den = imagen.window_denoiser(sampler='ddpm', sample_steps=DP.STEPS)
    got = check(joint_run(den, R.shared_cfg(stride), blend, shared_inpaint, resample)(shared_vol), ref,
                f"joint ddpm inpaint {mode} R {resample} stride {stride} {blend}")
    assert (got[~ref['covered'] & ~ref['background']] == ref['fill']).all() and (got[ref['background']] == ref['min_val']).all()


def test_paste_known_returns_the_known_voxels(shared_vol, shared_inpaint):
    """``paste_known=True``: the chain is the same, masked voxels equal the known volume outside fill and background; by default the
    loop ends on a denoising step, as the reference's, and they do not."""
    imagen = stub_imagen('x_start', 'clamp-min')
    known, mask = IP.inpaint_inputs()
    ref = chain_ref('static', 8, 2, 'gaussian', paste_known=True)
    den = imagen.window_denoiser(sampler='ddpm', sample_steps=DP.STEPS, paste_known=True)
    got = check(joint_run(den, R.shared_cfg(8), 'gaussian', shared_inpaint, 2)(shared_vol), ref, "joint ddpm inpaint paste_known")
    live = ref['covered'] & ~ref['background']
    assert (live & mask).sum() > 1000 and np.array_equal(got[live & mask], known[live & mask])
    plain = joint_run(imagen.window_denoiser(sampler='ddpm', sample_steps=DP.STEPS), R.shared_cfg(8), 'gaussian', shared_inpaint, 2)(shared_vol)
    plain = plain.cpu().numpy()
    assert np.array_equal(plain[live & ~mask], got[live & ~mask]) and not np.array_equal(plain[live & mask], got[live & mask])
    assert (got[~ref['covered'] & ~ref['background']] == ref['fill']).all() and (got[ref['background']] == ref['min_val']).all()


def test_inpaint_self_conditioning_and_samples(shared_vol, shared_inpaint):
    imagen = stub_imagen('x_start', 'clamp-min', unet=J.make_self_cond_unet())
    den = imagen.window_denoiser(sampler='ddpm', sample_steps=DP.STEPS)
    assert den.self_cond
    ref, plain = chain_ref('static', 8, 2, 'gaussian', self_cond=True), chain_ref('static', 8, 2, 'gaussian')
    assert np.abs(ref['mean'] - plain['mean']).max() > 1e-2                     # the self-conditioning term is visible
    check(joint_run(den, R.shared_cfg(8), 'gaussian', shared_inpaint, 2)(shared_vol), ref, "joint ddpm inpaint self-conditioned stride 8, R 2")
    a = joint_run(den, R.shared_cfg(5, batch_size=7), 'gaussian', shared_inpaint, 2, samples=2)(shared_vol, return_std=True)
    b = joint_run(den, R.shared_cfg(5, batch_size=3), 'gaussian', shared_inpaint, 2, samples=2)(shared_vol, return_std=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[1].max() > 0.05


# ---- G3: the tie to the per-window sampler at stride = patch ---------------------------------------------------------------------------------
@pytest.mark.parametrize('resample', [1, 2, 3])
@pytest.mark.parametrize('mode', ['static', 'dynamic'])
def test_inpaint_at_stride_equal_patch_is_the_independent_path(shared_vol, shared_inpaint, mode, resample):
    imagen = stub_imagen('x_start', IMAGEN[mode])
    cfg = R.shared_cfg(16)
    sample = lambda **kw: imagen.sample(use_tqdm=False, **kw)
    independent = independent_run(sample, cfg, 'constant', shared_inpaint, resample, DP.STEPS)(shared_vol)
    joint = joint_run(imagen.window_denoiser(sampler='ddpm', sample_steps=DP.STEPS), cfg, 'constant', shared_inpaint, resample)(shared_vol)
    assert independent.unique().numel() > 1000
    assert torch.equal(joint, independent)


def test_inpaint_tie_with_a_self_conditioning_stub(shared_vol, shared_inpaint):
    imagen = stub_imagen('x_start', 'clamp-min', unet=J.make_self_cond_unet())
    cfg = R.shared_cfg(16)
    sample = lambda **kw: imagen.sample(use_tqdm=False, **kw)
    independent = independent_run(sample, cfg, 'constant', shared_inpaint, 2, DP.STEPS)(shared_vol)
    joint = joint_run(imagen.window_denoiser(sampler='ddpm', sample_steps=DP.STEPS), cfg, 'constant', shared_inpaint, 2)(shared_vol)
    assert torch.equal(joint, independent) and joint.unique().numel() > 1000


def test_inpaint_with_the_conv3d_unet_through_the_trainer():
    """``ImagenTrainer`` at 16^3 (eight 8-voxel windows), R = 2: the tie at stride = patch, then overlapping windows -- finite, identical
    on a second run, steered by the known region and not what blending independently inpainted windows gives."""
    from diffusioniqt_amd.imagen_pytorch3D import Imagen, NullUnet
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
    vol = torch.from_numpy(np.random.default_rng(12).integers(1, 1000, (16, 16, 16)).astype(np.float32)).to(DEV)      # every window is kept
    known, mask = (torch.from_numpy(a).to(DEV) for a in IP.inpaint_inputs((16, 16, 16), box=((3, 13), (2, 11), (5, 14))))
    inp = (known, mask)
    cfg = lambda stride, batch: R.shared_cfg(stride, batch_size=batch, P=8)
    den = trainer.window_denoiser(sampler='ddpm', sample_steps=3)
    assert den.num_steps == 3 and not den.paste_known
    independent = independent_run(trainer.sample, cfg(8, 6), 'constant', inp, 2, 3, seed=4)(vol)
    joint = joint_run(den, cfg(8, 6), 'constant', inp, 2, seed=4)(vol)
    assert torch.equal(joint, independent) and joint.unique().numel() > 1000
    runs = [joint_run(den, cfg(4, 27), 'gaussian', inp, 2, seed=4)(vol) for _ in range(2)]
    assert torch.isfinite(runs[0]).all() and torch.equal(runs[0], runs[1])
    empty = joint_run(den, cfg(4, 27), 'gaussian', (known, torch.zeros_like(mask)), 2, seed=4)(vol)
    assert not torch.equal(runs[0][~mask], empty[~mask])                        # the known region steers its surroundings
    blended = independent_run(trainer.sample, cfg(4, 27), 'gaussian', inp, 2, 3, seed=4)(vol)
    assert not torch.equal(runs[0], blended)
    kept = mask & (vol != vol.min())
    pasted = joint_run(trainer.window_denoiser(sampler='ddpm', sample_steps=3, paste_known=True), cfg(4, 27), 'gaussian', inp, 2, seed=4)(vol)
    assert kept.sum() > 500 and torch.equal(pasted[kept], known[kept]) and torch.equal(pasted[~mask], runs[0][~mask])
