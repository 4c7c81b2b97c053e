"""EDM inpainting on the joint volume state on a real MI355X, against the float64 specification of
tests/volume_joint_inpaint_reference.py: the phases of ``ops.volume_joint_heun_inpaint`` on their own (against float64 and, bit for bit,
against the same update assembled from ``ops.volume_joint_heun``, ``ops.axpby3`` and ``ops.mask_blend``), the whole chain of
``VolumeInference(joint=True, inpaint=...)`` with the elementwise stub network, its bit-for-bit tie to independently inpainted windows
(``ElucidatedImagen.sample(noise=source, inpaint_images=...)``) at stride = patch (stub, Unet3D and the Conv3d U-Net through the
trainer), overlapping windows with a real network, batching, samples, block mode and self-conditioning.

Chain bound: ``volume_joint_inpaint_reference.chain_bound``; tests/test_volume_joint_inpaint_host.py holds an fp32 emulation of the chain
to half of it and the bound itself to 1e-3 of the signal's peak-to-peak for every case compared here."""
import itertools
import json

import numpy as np
import pytest
import torch

from tests import volume_blend_reference as R
from tests import volume_joint_heun_reference as HN
from tests import volume_joint_inpaint_reference as IP
from tests import volume_joint_reference as J
from tests.conftest import load_golden
from tests.test_gpu_volume_joint_heun import axpby, cu, field
from tests.test_volume_joint_inpaint_host import CASES, IDS

pytestmark = pytest.mark.gpu
DEV = "cuda"
_REF = {}
BLOCK_BOX = ((10, 40), (12, 44), (20, 50))
SMALL = dict(shape=(20, 24, 28), box=((3, 15), (5, 19), (10, 22)))           # crosses the borders of the 8-voxel windows


def chain_ref(vol_name, stride, dynamic, resample, churn, blend, samples=1, self_cond=False):
    """One float64 reference per case, shared by the tests that need it and never modified."""
    key = (vol_name, stride, dynamic, resample, churn, blend, samples, self_cond)
    if key not in _REF:
        if vol_name == 'block':
            vol, cfg, (known, mask) = R.block_volume(), R.block_cfg(), IP.inpaint_inputs((56, 56, 56), box=BLOCK_BOX)
        else:
            vol, cfg, (known, mask) = R.shared_volume(), R.shared_cfg(stride), IP.inpaint_inputs()
        _REF[key] = IP.joint_reference(vol, cfg, HN.tables(HN.HP, HN.CHURN[churn]), blend, dynamic, known, mask, resample, samples=samples,
                                       self_cond=self_cond)
        for v in _REF[key].values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return _REF[key]


def joint_run(den, cfg, blend, inpaint, resample, **kw):
    from diffusioniqt_amd.inference import VolumeInference
    return VolumeInference(cfg, den, blend=blend, noise='anchored', joint=True, seed=kw.pop('seed', HN.SEED), inpaint=inpaint,
                           inpaint_resample_times=resample, **kw)


def independent_run(sample, cfg, blend, P, inpaint, resample, **kw):
    """Every window's own inpainting chain through ``sample`` with the volume-anchored source, finished patches blended."""
    from diffusioniqt_amd.inference import VolumeInference

    def sample_fn(x, noise=None, **inp):
        return sample(batch_size=x.shape[0], video_frames=P, start_image_or_video=x, start_at_unet_number=2, noise=noise, **inp)
    return VolumeInference(cfg, sample_fn, blend=blend, noise='anchored', seed=kw.pop('seed', HN.SEED), inpaint=inpaint,
                           inpaint_resample_times=resample, **kw)


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


@pytest.fixture(scope="module")
def shared_inpaint():
    known, mask = IP.inpaint_inputs()
    return torch.from_numpy(known).to(DEV), torch.from_numpy(mask).to(DEV)


# ---- G1: the phases against the float64 specification and against the single-purpose ops -------------------------------------------------
@pytest.fixture(scope="module")
def step_case():
    rng = np.random.default_rng(17)
    vol = R.shared_volume()
    out = {}
    for stride, kind in itertools.product((8, 5), ('gaussian', 'constant')):
        L = J.layout(vol, R.shared_cfg(stride))
        ys = [rng.standard_normal((L['kept'].shape[0], 16, 16, 16)).astype(np.float32) * 2 for _ in range(2)]
        out[stride, kind] = (L, ys, rng.standard_normal(vol.shape).astype(np.float32) * 3, R.taps_of(16, kind))
    return out


@pytest.mark.parametrize('kc', [0.0, 0.625])
@pytest.mark.parametrize('kr', [0.0, 0.375])
@pytest.mark.parametrize('kind', ['gaussian', 'constant'])
@pytest.mark.parametrize('stride', [8, 5])
def test_inpaint_phases_match_reference_and_the_single_purpose_ops(step_case, stride, kind, kr, kc):
    """The predictor (the existing phase 1), then the inpainting corrector.  The per-voxel bound is that of
    ``test_heun_phases_match_reference_and_the_single_purpose_ops`` for xh, plus the re-noise term u (max|x| + 6 |kr|) + 2e-5 |kr| (its
    product, its sum and the normals' bound); a masked voxel is known + kc n."""
    from diffusioniqt_amd import ops
    L, ys, xh0, taps = step_case[stride, kind]
    known, mask = IP.inpaint_inputs()
    (a1, b1), (a2, b2, c2, d2) = (0.4375, 0.5625), (0.71875, 0.28125, -0.8125, 0.8125)
    clamp, seed, draw, draw_r, sample = (-1., 1., 1), 0x123456789, 6, 5, 2
    u = 2.0 ** -24
    c64 = J.clamp_of(*clamp)
    shape = xh0.shape
    x0a, covered = HN.fuse(c64(ys[0].astype(np.float64)), L['slot'], taps, stride, shape)
    want_n, _ = HN.heun_phase1(x0a, covered, xh0.astype(np.float64), a1, b1)
    x0b, _ = HN.fuse(c64(ys[1].astype(np.float64)), L['slot'], taps, stride, shape)
    want_x, _ = HN.heun_phase2(x0b, covered, xh0.astype(np.float64), want_n, x0a, (a2, b2, c2, d2), 0.0, None)
    want_t = want_x + kr * J.normals(shape, seed, draw_r, sample) if kr != 0 else want_x
    want_h = np.where(mask, known.astype(np.float64), want_t)
    want_h = np.where(covered, want_h + kc * J.normals(shape, seed, draw, sample) if kc != 0 else want_h, xh0.astype(np.float64))
    slot, tp = cu(L['slot'].astype(np.int32)), cu(taps.astype(np.float32))
    y0, y1 = cu(ys[0]), cu(ys[1])
    kn, mk_b, mk_f = cu(known), cu(mask.astype(np.uint8)), cu(mask.astype(np.float32))
    cov = cu(covered)
    # the assembly: the existing corrector with kc = 0 gives x, then the two axpby3 with the selection between them
    xh, xn, x0 = cu(xh0), torch.full(shape, 7.0, device=DEV), torch.full(shape, 7.0, device=DEV)
    ops.volume_joint_heun(y0, slot, tp, xh, xn, x0, 1, (a1, b1), 0.0, *clamp, stride)
    xn_1, x0_1 = xn.clone(), x0.clone()
    ops.volume_joint_heun(y1, slot, tp, xh, xn, x0, 2, (a2, b2, c2, d2), 0.0, *clamp, stride, seed, draw, sample)
    asm_t = axpby([(1.0, xh), (kr, field(shape, seed, draw_r, sample))]) if kr != 0 else xh
    asm_h = axpby([(1.0, ops.mask_blend(asm_t, kn, mk_f)), (kc, field(shape, seed, draw, sample))]).where(cov, cu(xh0))
    asm_0 = x0.clone()

    xh, xn, x0 = cu(xh0), xn_1.clone(), x0_1.clone()
    r = ops.volume_joint_heun_inpaint(y1, slot, tp, xh, xn, x0, kn, mk_b, 2, (a2, b2, c2, d2), kr, kc, *clamp, stride, seed, draw, draw_r, sample)
    assert all(t.data_ptr() == w.data_ptr() for t, w in zip(r, (xh, xn, x0)))
    max_y, max_h, max_n = float(np.abs(ys).max()), float(np.abs(xh0).max()), float(np.abs(want_n).max())
    tol = R.tolerance(L['windows_per_voxel'], max_y)
    bound_n = abs(b1) * tol + 3 * u * (abs(a1) * max_h + abs(b1) * max_y)
    bound_h = abs(d2) * tol + abs(c2) * bound_n + abs(b2) * tol + 7 * u * (abs(a2) * max_h + (abs(b2) + abs(d2)) * max_y + abs(c2) * max_n) \
        + u * (float(np.abs(want_t).max()) + 6 * abs(kr)) + 2e-5 * abs(kr) + u * (float(np.abs(want_h).max()) + 6 * abs(kc)) + 2e-5 * abs(kc)
    err_h = np.abs(xh.cpu().numpy().astype(np.float64) - want_h).max()
    err_0 = np.abs(x0.cpu().numpy().astype(np.float64) - x0b).max()
    print(f"inpaint corrector stride {stride} {kind} kr {kr} kc {kc}: xh {err_h:.3e} (bound {bound_h:.3e}), x0 {err_0:.3e} (bound {tol:.3e})")
    assert err_h <= bound_h and err_0 <= tol
    assert torch.equal(xh, asm_h) and torch.equal(x0, asm_0) and torch.equal(xn, xn_1)       # every voxel, masked and uncovered included
    both = cov & cu(mask)
    assert both.sum() > 1000 and torch.equal(xh[both], axpby([(1.0, kn), (kc, field(shape, seed, draw, sample))])[both])
    # the re-churn of the step without a corrector: every voxel, from xn
    again = ops.volume_joint_heun_inpaint(None, None, None, xh, xn, x0, kn, mk_b, 3, (), 0.0, kc, *clamp, stride, seed, draw + 1, 0, sample)[0]
    assert torch.equal(again, axpby([(1.0, ops.mask_blend(xn_1, kn, mk_f)), (kc, field(shape, seed, draw + 1, sample))]))
    assert torch.equal(xn, xn_1) and torch.equal(x0, asm_0)


def test_inpaint_joint_argument_errors(step_case):
    from diffusioniqt_amd import ops
    L, ys, xh0, taps = step_case[8, 'gaussian']
    known, mask = IP.inpaint_inputs()
    y, slot, tp, xh = cu(ys[0]), cu(L['slot'].astype(np.int32)), cu(taps.astype(np.float32)), cu(xh0)
    xn, x0, kn, mk = torch.empty_like(xh), torch.empty_like(xh), cu(known), cu(mask)
    ok = (-1.0, 1.0, 1, 8)
    four = (1.0, 0.5, 0.25, 0.25)
    with pytest.raises(ValueError, match="phase"):
        ops.volume_joint_heun_inpaint(y, slot, tp, xh, xn, x0, kn, mk, 1, (1.0, 0.5), 0.0, 0.0, *ok)
    with pytest.raises(ValueError, match="coefficients"):
        ops.volume_joint_heun_inpaint(y, slot, tp, xh, xn, x0, kn, mk, 2, (1.0, 0.5), 0.0, 0.0, *ok)
    with pytest.raises(ValueError, match="mask"):
        ops.volume_joint_heun_inpaint(y, slot, tp, xh, xn, x0, kn, mk.float(), 2, four, 0.0, 0.0, *ok)
    with pytest.raises(ValueError, match="known"):
        ops.volume_joint_heun_inpaint(y, slot, tp, xh, xn, x0, kn[:-1].contiguous(), mk, 2, four, 0.0, 0.0, *ok)
    with pytest.raises(ValueError, match="lattice"):
        ops.volume_joint_heun_inpaint(y, slot, tp, xh, xn, x0, kn, mk, 2, four, 0.0, 0.0, -1.0, 1.0, 1, 5)
    with pytest.raises(ValueError, match="draw"):
        ops.volume_joint_heun_inpaint(y, slot, tp, xh, xn, x0, kn, mk, 2, four, 0.5, 0.5, *ok, 0, 3, 1 << 32)
    with pytest.raises(ValueError, match="three different"):
        ops.volume_joint_heun_inpaint(y, slot, tp, xh, xn, xn, kn, mk, 2, four, 0.0, 0.0, *ok)
    with pytest.raises(ValueError, match="draw"):
        ops.volume_joint_heun_inpaint_init(kn, mk, 1.0, 0.5, 0, draw=(1 << 32) - 1)


# ---- G2: phase 0 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kc', [0.0, 0.625])
def test_inpaint_initial_state_is_the_axpby3_sequence_on_the_anchored_field(kc):
    from diffusioniqt_amd import ops
    seed, sigma0 = 0x123456789, 1.4999995231628418
    known, mask = IP.inpaint_inputs(**SMALL)
    kn, mk = cu(known), cu(mask)
    for draw, sample in ((0, 0), (3, 2)):
        got = ops.volume_joint_heun_inpaint_init(kn, mk, sigma0, kc, seed, draw=draw, sample=sample)
        images = axpby([(sigma0, field(SMALL['shape'], seed, draw, sample))])
        want = axpby([(1.0, ops.mask_blend(images, kn, mk.float())), (kc, field(SMALL['shape'], seed, draw + 1, sample))])
        assert torch.equal(got, want) and got.unique().numel() > 1000
        assert torch.equal(got[mk], axpby([(1.0, kn), (kc, field(SMALL['shape'], seed, draw + 1, sample))])[mk])


# ---- G3: the whole chain against the float64 reference ------------------------------------------------------------------------------------
@pytest.mark.parametrize('dynamic,resample,churn,tiling', CASES, ids=IDS)
def test_inpaint_chain_matches_the_float64_reference(shared_vol, shared_inpaint, dynamic, resample, churn, tiling):
    stride, blend = tiling
    elu = HN.make_elucidated(churn, dynamic).to(DEV)
    ref = chain_ref('shared', stride, dynamic, resample, churn, blend)
    got = joint_run(elu.window_denoiser(), R.shared_cfg(stride), blend, shared_inpaint, resample)(shared_vol)
    got = check(got, ref, f"joint inpaint {'dynamic' if dynamic else 'static'} R {resample} {churn} stride {stride} {blend}")
    known, mask = IP.inpaint_inputs()
    live = ref['covered'] & ~ref['background']
    assert (live & mask).sum() > 1000 and np.array_equal(got[live & mask], known[live & mask])      # the known voxels, bit for bit
    assert (got[~ref['covered'] & ~ref['background']] == ref['fill']).all() and (got[ref['background']] == ref['min_val']).all()


# ---- G4: the tie to the per-window sampler at stride = patch ---------------------------------------------------------------------------------
@pytest.mark.parametrize('resample', [1, 2, 3])
@pytest.mark.parametrize('dynamic', [False, True], ids=['static', 'dynamic'])
def test_inpaint_at_stride_equal_patch_is_the_independent_path(shared_vol, shared_inpaint, dynamic, resample):
    elu = HN.make_elucidated('churn-on', dynamic).to(DEV)
    cfg = R.shared_cfg(16)
    sample = lambda **kw: elu.sample(use_tqdm=False, **kw)
    independent = independent_run(sample, cfg, 'constant', 16, shared_inpaint, resample)(shared_vol)
    joint = joint_run(elu.window_denoiser(), cfg, 'constant', shared_inpaint, resample)(shared_vol)
    assert independent.unique().numel() > 1000
    assert torch.equal(joint, independent)


def test_inpaint_crop_mode_at_stride_equal_patch_is_the_blended_independent_path(shared_vol, shared_inpaint):
    """Without a blend mode the windows are placed whole at stride = patch: the same volume as the constant blend of the same windows
    (one window per voxel, weight 1), known voxels included."""
    from diffusioniqt_amd.inference import VolumeInference
    elu = HN.make_elucidated('churn-on', False).to(DEV)
    cfg = R.shared_cfg(16)

    def sample_fn(x, noise=None, **inp):
        return elu.sample(batch_size=x.shape[0], video_frames=16, start_image_or_video=x, start_at_unet_number=2, use_tqdm=False, noise=noise,
                          **inp)
    crop = VolumeInference(cfg, sample_fn, noise='anchored', seed=HN.SEED, inpaint=shared_inpaint, inpaint_resample_times=2)(shared_vol)
    blend = independent_run(lambda **kw: elu.sample(use_tqdm=False, **kw), cfg, 'constant', 16, shared_inpaint, 2)(shared_vol)
    assert torch.equal(crop, blend) and crop.unique().numel() > 1000


def _real_volume():
    return torch.from_numpy(np.random.default_rng(12).integers(1, 1000, (20, 24, 28)).astype(np.float32)).to(DEV)   # every window is kept


def _small_inpaint():
    known, mask = IP.inpaint_inputs(**SMALL)
    return torch.from_numpy(known).to(DEV), torch.from_numpy(mask).to(DEV)


def test_inpaint_tie_with_a_real_unet3d():
    """With a real network the context matters: a paste missing from either path breaks the tie."""
    from tests.test_gpu_family_b import make_edm
    kw = {k: (tuple(v) if isinstance(v, list) else v) for k, v in json.loads(str(load_golden('unet3d_tiny')['kwargs'])).items()}
    elu = make_edm(kw, 3)
    vol, cfg, inp = _real_volume(), R.shared_cfg(8, batch_size=6, P=8), _small_inpaint()
    sample = lambda **kw: elu.sample(use_tqdm=False, **kw)
    independent = independent_run(sample, cfg, 'constant', 8, inp, 2, seed=4)(vol)
    joint = joint_run(elu.window_denoiser(), cfg, 'constant', inp, 2, seed=4)(vol)
    assert torch.equal(joint, independent) and joint.unique().numel() > 1000
    known, mask = inp
    covered = torch.zeros_like(mask)
    covered[:16, :, :24] = True                                                  # 2 x 3 x 3 windows of 8 at stride 8; the rest is fill
    covered &= vol != vol.min()                                                  # and the background reset comes last
    assert torch.equal(joint[mask & covered], known[mask & covered])
    plain = joint_run(elu.window_denoiser(), cfg, 'constant', None, 2, seed=4)(vol)
    assert not torch.equal(joint[~mask & covered], plain[~mask & covered])


def test_inpaint_with_the_conv3d_unet_through_the_trainer():
    """``ImagenTrainer`` on an EDM trainer with R = 2: the tie at stride = patch, then overlapping windows -- finite, identical on a second
    run, steered by the known region (not the run with an empty mask at unmasked voxels) and not what blending independently inpainted
    windows gives."""
    from diffusioniqt_amd.elucidated_imagen import ElucidatedImagen
    from diffusioniqt_amd.imagen_pytorch3D import NullUnet
    from diffusioniqt_amd.trainer import ImagenTrainer
    from tests.test_gpu_unet import build
    unet, _, _ = build(load_golden('unetA_tiny'), 0)
    configs = {'Data': {'norm': 'z-score'}, 'Train': {'batch_sample': False, 'patch_size_sub': 8, 'pred_obj': 'x_start'}, 'Eval': {'repeat': 1}}
    elu = ElucidatedImagen(unets=(NullUnet(), unet), image_sizes=(8, 8), channels=1, condition_on_text=False, auto_normalize_img=False,
                           cond_drop_prob=0.0, num_sample_steps=3, dynamic_thresholding=False).to(DEV)
    ImagenTrainer.locked = False
    trainer = ImagenTrainer(configs=configs, imagen=elu, verbose=False)
    vol, inp = _real_volume(), _small_inpaint()
    known, mask = inp
    cfg = lambda stride, batch: R.shared_cfg(stride, batch_size=batch, P=8)
    den = trainer.window_denoiser()
    independent = independent_run(trainer.sample, cfg(8, 6), 'constant', 8, inp, 2, seed=4)(vol)
    joint = joint_run(den, cfg(8, 6), 'constant', inp, 2, seed=4)(vol)
    assert torch.equal(joint, independent) and joint.unique().numel() > 1000
    runs = [joint_run(den, cfg(4, 30), 'gaussian', inp, 2, seed=4)(vol) for _ in range(2)]
    assert torch.isfinite(runs[0]).all() and torch.equal(runs[0], runs[1])
    kept = mask & (vol != vol.min())                                             # every voxel is covered; the background reset comes last
    assert kept.sum() > 1000 and torch.equal(runs[0][kept], known[kept])
    empty = joint_run(den, cfg(4, 30), 'gaussian', (known, torch.zeros_like(mask)), 2, seed=4)(vol)
    assert not torch.equal(runs[0][~mask], empty[~mask])                        # the known region steers its surroundings
    blended = independent_run(trainer.sample, cfg(4, 30), 'gaussian', 8, inp, 2, seed=4)(vol)
    assert not torch.equal(runs[0], blended)


# ---- G5: batching, samples, block mode, self-conditioning ---------------------------------------------------------------------------------
def test_inpaint_batching_and_samples(shared_vol, shared_inpaint):
    elu = HN.make_elucidated('churn-on', False).to(DEV)
    den = elu.window_denoiser()
    a = joint_run(den, R.shared_cfg(5, batch_size=7), 'gaussian', shared_inpaint, 2)(shared_vol)
    b = joint_run(den, R.shared_cfg(5, batch_size=3), 'gaussian', shared_inpaint, 2)(shared_vol)
    assert torch.equal(a, b)
    ref = chain_ref('shared', 8, False, 2, 'churn-on', 'gaussian', samples=2)
    mean, std = joint_run(den, R.shared_cfg(8), 'gaussian', shared_inpaint, 2, samples=2)(shared_vol, return_std=True)
    check(mean, ref, "joint inpaint S = 2 mean")
    std = check(std, ref, "joint inpaint S = 2 deviation", key='std', factor=2)
    live = ref['covered'] & ~ref['background']
    mask = ref['mask']
    assert std[live & ~mask].max() > 0.05 and not std[live & mask].any() and not std[~live].any()      # the known voxels do not vary


def test_inpaint_block_mode_matches_the_float64_reference():
    elu = HN.make_elucidated('churn-on', False, size=8).to(DEV)
    ref = chain_ref('block', None, False, 2, 'churn-on', 'gaussian')
    assert ref['kept'] == ref['candidates'] == 27 and ref['covered'].all()
    vol = torch.from_numpy(R.block_volume()).to(DEV)
    known, mask = IP.inpaint_inputs((56, 56, 56), box=BLOCK_BOX)
    got = joint_run(elu.window_denoiser(), R.block_cfg(), 'gaussian', (torch.from_numpy(known), torch.from_numpy(mask)), 2)(vol)   # host tensors
    got = check(got, ref, "joint inpaint block mode P 24 stride 16, R 2")
    live = ~ref['background']
    assert np.array_equal(got[live & mask], known[live & mask])


def test_inpaint_self_conditioning_carries_across_the_passes(shared_vol, shared_inpaint):
    elu = HN.make_elucidated('churn-on', False, self_cond=True).to(DEV)
    ref = chain_ref('shared', 8, False, 2, 'churn-on', 'gaussian', self_cond=True)
    plain = chain_ref('shared', 8, False, 2, 'churn-on', 'gaussian')
    assert np.abs(ref['mean'] - plain['mean']).max() > 1e-2                     # the self-conditioning term is visible
    check(joint_run(elu.window_denoiser(), R.shared_cfg(8), 'gaussian', shared_inpaint, 2)(shared_vol), ref,
          "joint inpaint self-conditioned stride 8, R 2")
