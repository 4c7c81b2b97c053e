"""Host-side checks of EDM inpainting (no GPU here): the float64 specification of tests/volume_joint_inpaint_reference.py is
``volume_joint_heun_reference``'s chain when nothing is masked, its derived bound dominates an fp32 emulation of the same chain and is
small beside the signal, at stride = patch it is the reference's RePaint loop (elucidated_imagen.py:473-530) transcribed per window,
every argument rule is raised before anything touches the device, ``sample`` takes from a noise list what the reference drew when the
fixture was made, and the two new entries return error codes for null pointers, bad lattices, a bad phase and a draw index with no
successor."""
import math

import numpy as np
import pytest
import torch

from tests import volume_blend_reference as R
from tests import volume_joint_heun_reference as HN
from tests import volume_joint_inpaint_reference as IP
from tests import volume_joint_reference as J
from tests.conftest import load_golden

TILINGS = ((8, 'gaussian'), (5, 'constant'))
# dynamic thresholding with R >= 2 is not compared under the bound: the thresholding doubles every gain and the bound of those chains is
# 1.7e-3 .. 2.2e-2 of the peak-to-peak -- the bit-for-bit ties of tests/test_gpu_volume_joint_inpaint.py cover them instead
CASES = [(dynamic, resample, churn, tiling) for dynamic, resample in ((False, 1), (False, 2), (True, 1)) for churn in HN.CHURN
         for tiling in TILINGS]
IDS = [f"{'dynamic' if d else 'static'}-R{r}-{c}-s{t[0]}-{t[1]}" for d, r, c, t in CASES]


# ---- H1: the reference alone --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('churn', list(HN.CHURN))
def test_an_empty_mask_and_one_pass_is_the_heun_chain(churn):
    vol, cfg = R.shared_volume(), R.shared_cfg(8)
    tabs = HN.tables(HN.HP, HN.CHURN[churn])
    known, mask = IP.inpaint_inputs()
    want, L, m, = HN.joint_chain(vol, cfg, tabs, 'gaussian', False)
    got, _, m2, draws = IP.joint_chain(vol, cfg, tabs, 'gaussian', False, known, np.zeros_like(mask), 1)
    covered = IP.joint_reference(vol, cfg, tabs, 'gaussian', False, known, np.zeros_like(mask), 1)['covered']
    assert covered.any() and np.array_equal(got[covered], want[covered]) and m == m2
    assert draws == 1 + HN.HP['num_sample_steps']                                # the initial image and one eps per step


@pytest.mark.parametrize('dynamic,resample,churn,tiling', CASES, ids=IDS)
def test_chain_bound_dominates_an_fp32_emulation_and_is_small_beside_the_signal(dynamic, resample, churn, tiling):
    """The project's pair of conditions on a derived bound, over covered, non-background, unmasked voxels (a masked one is exact)."""
    stride, blend = tiling
    vol, cfg = R.shared_volume(), R.shared_cfg(stride)
    tabs = HN.tables(HN.HP, HN.CHURN[churn])
    known, mask = IP.inpaint_inputs()
    ref = IP.joint_reference(vol, cfg, tabs, blend, dynamic, known, mask, resample)
    emu = IP.joint_reference(vol, cfg, tabs, blend, dynamic, known, mask, resample, dtype=np.float32)
    live = ref['covered'] & ~ref['background']
    free = live & ~mask
    T = HN.HP['num_sample_steps']
    assert ref['draws'] == 1 + T * resample + (T - 1) * (resample - 1)
    assert (live & mask).sum() > 1000 and free.sum() > 1000
    assert np.array_equal(ref['mean'][live & mask], known[live & mask].astype(np.float64))
    assert np.array_equal(emu['mean'][live & mask], known[live & mask].astype(np.float64))
    err = np.abs(emu['mean'] - ref['mean'])[free].max()
    ptp = np.ptp(ref['mean'][free])
    print(f"inpaint chain {'dynamic' if dynamic else 'static'} R {resample} {churn} stride {stride} {blend}: fp32 emulation / bound = "
          f"{err / ref['bound']:.3f} (err {err:.3e}, bound {ref['bound']:.3e}), bound / ptp = {ref['bound'] / ptp:.3e} (ptp {ptp:.3f}, "
          f"largest |state| {ref['state_max']:.2f})")
    assert err <= 0.5 * ref['bound']
    assert ref['bound'] <= 1e-3 * ptp


def reference_loop_per_window(fn, known, mask, draws, hp, resample):
    """elucidated_imagen.py:426-532 for one window in float64 torch, static clamp, on the injected normals ``draws`` (in call order)."""
    N, inv_rho = hp['num_sample_steps'], 1 / hp['rho']
    steps = torch.arange(N, dtype=torch.float32)
    sigmas = (hp['sigma_max'] ** inv_rho + steps / (N - 1) * (hp['sigma_min'] ** inv_rho - hp['sigma_max'] ** inv_rho)) ** hp['rho']
    sigmas = torch.nn.functional.pad(sigmas, (0, 1), value=0.)
    gammas = torch.where((sigmas >= hp['S_tmin']) & (sigmas <= hp['S_tmax']), min(hp['S_churn'] / N, math.sqrt(2) - 1), 0.)
    sd = hp['sigma_data']
    draws = list(draws)

    def denoise(x, sigma):
        c_in, c_skip = (sigma ** 2 + sd ** 2) ** -0.5, sd ** 2 / (sigma ** 2 + sd ** 2)
        c_out = sigma * sd * (sd ** 2 + sigma ** 2) ** -0.5
        c_noise = torch.log(torch.full((1,), sigma, dtype=torch.float32).clamp(min=1e-20)) * 0.25
        return (c_skip * x + c_out * fn(c_in * x, c_noise.double())).clamp(-1., 1.)

    images = sigmas[0].item() * draws.pop(0)
    pairs = list(zip(sigmas[:-1].tolist(), sigmas[1:].tolist(), gammas[:-1].tolist()))
    for ind, (sigma, sigma_next, gamma) in enumerate(pairs):
        for r in reversed(range(resample)):
            eps = hp['S_noise'] * draws.pop(0)
            sigma_hat = sigma + gamma * sigma
            added = math.sqrt(sigma_hat ** 2 - sigma ** 2) * eps
            images_hat = (images + added) * ~mask + (known + added) * mask
            out = denoise(images_hat, sigma_hat)
            d = (images_hat - out) / sigma_hat
            images_next = images_hat + (sigma_next - sigma_hat) * d
            if sigma_next != 0:
                out2 = denoise(images_next, sigma_next)
                d2 = (images_next - out2) / sigma_next
                images_next = images_hat + 0.5 * (sigma_next - sigma_hat) * (d + d2)
            images = images_next
            if not (r == 0 or ind == len(pairs) - 1):
                images = images + (sigma - sigma_next) * draws.pop(0)
    assert not draws
    images = images.clamp(-1., 1.)
    return images * ~mask + known * mask


@pytest.mark.parametrize('resample', [1, 2, 3])
def test_reference_is_the_reference_loop_per_window_at_stride_equal_patch(resample):
    """Stride = patch, constant blend, default churn: every fused prediction is the one window's own, so the joint chain is the
    reference's loop run per kept window on the window's cut of the anchored normals, numbered by the one counter."""
    from oracle import iqt_oracle_b as OB
    vol, cfg = R.shared_volume(), R.shared_cfg(16)
    hp = {**HN.HP, 'S_churn': HN.CHURN['churn-on']}
    tabs = HN.tables(HN.HP, HN.CHURN['churn-on'])
    known, mask = IP.inpaint_inputs()
    ref = IP.joint_reference(vol, cfg, tabs, 'constant', False, known, mask, resample)
    L = J.layout(vol, cfg)
    low = (vol - np.float32(300.0)) / np.float32(200.0)
    draws = [torch.from_numpy(J.normals(vol.shape, HN.SEED, k, 0).copy()) for k in range(ref['draws'] + 1)]
    cut = lambda a, o: a[o[0]:o[0] + 16, o[1]:o[1] + 16, o[2]:o[2] + 16][None, None]
    worst = 0.0
    for o in L['kept']:
        lr = OB.lowres_q_sample(torch.from_numpy(cut(low, o)).double(), torch.full((1,), HN.LOWRES_LEVEL), cut(draws[0], o))
        fn = lambda x, cn, lr=lr: 0.5 * (x / (1.0 + x.abs())) + 0.25 * lr + 0.015625 * cn.view(-1, 1, 1, 1, 1)
        want = reference_loop_per_window(fn, torch.from_numpy(cut(known, o)).double(), torch.from_numpy(cut(mask, o)),
                                         [cut(d, o).double() for d in draws[1:]], hp, resample)
        keep = ~cut(ref['background'], o)
        worst = max(worst, float(np.abs(cut(ref['mean'], o) - want.numpy())[keep].max()))
    print(f"inpaint reference vs the reference's loop per window (R {resample}): {worst:.3e}, bound {ref['bound']:.3e}")
    assert L['kept'].shape[0] >= 2 and worst <= ref['bound']


# ---- H2: argument rules, all before the device is touched --------------------------------------------------------------------------------
def test_volume_inference_inpaint_argument_errors():
    from diffusioniqt_amd.inference import VolumeInference
    elu = HN.make_elucidated('churn-on', False)
    den = elu.window_denoiser()
    known, mask = (torch.from_numpy(a) for a in IP.inpaint_inputs())
    joint = dict(blend='gaussian', noise='anchored', joint=True)
    inf = VolumeInference(R.shared_cfg(8), den, inpaint=(known, mask), inpaint_resample_times=2, **joint)
    assert inf.inpaint is not None and inf.resample_times == 2
    assert VolumeInference(R.shared_cfg(8), lambda x: x, inpaint=(known, mask)).resample_times == 5       # crop mode, the default R
    assert VolumeInference(R.shared_cfg(8), den, **joint).inpaint is None
    for bad in ((known,), known, (known, mask.float()), (known, mask[:-1]), (known[0], mask[0]), (known.long(), mask)):
        with pytest.raises(ValueError, match="inpaint"):
            VolumeInference(R.shared_cfg(8), den, inpaint=bad, **joint)
    for bad in (0, -1, 1.5, True, None, '2'):
        with pytest.raises(ValueError, match="inpaint"):
            VolumeInference(R.shared_cfg(8), den, inpaint=(known, mask), inpaint_resample_times=bad, **joint)
    multistep = elu.window_denoiser(sampler='dpmpp2m', sample_steps=4)
    first_order = type('FirstOrder', (), dict(num_steps=3, coefs=torch.zeros(3, 3), clamp=(-1., 1., 1), x0=None, finish=None))()
    for other in (multistep, first_order):
        VolumeInference(R.shared_cfg(8), other, **joint)                          # fine without inpaint ...
        with pytest.raises(ValueError, match="inpaint"):                         # ... and refused with it
            VolumeInference(R.shared_cfg(8), other, inpaint=(known, mask), **joint)
    with pytest.raises(ValueError, match="inpaint"):                             # a shape that is not the volume's, on CPU tensors
        inf(torch.zeros(40, 36, 40))
    with pytest.raises(ValueError, match="inpaint"):
        VolumeInference(R.shared_cfg(8), lambda x: x, inpaint=(known, mask))(torch.zeros(8, 36, 44))


@pytest.mark.parametrize('mode', ['crop', 'blend', 'crop-block'])
def test_crop_and_blend_modes_hand_the_sampler_the_windows_of_both_volumes(mode, monkeypatch):
    """The control flow of the independent path, on the recording stand-ins of tests/test_volume_launch_trace_host.py (``patch_gather``
    is computed for real): every sampler call gets its batch's windows of the known volume and of the mask, thresholded, and R."""
    from diffusioniqt_amd import inference
    from tests import test_volume_launch_trace_host as LT
    block = mode == 'crop-block'
    vol = torch.from_numpy(R.block_volume() if block else R.shared_volume())
    cfg = R.block_cfg() if block else R.shared_cfg(16, batch_size=3)
    known, mask = (torch.from_numpy(a) for a in IP.inpaint_inputs(tuple(vol.shape), box=((10, 30), (5, 27), (24, 40))))
    rec, calls = LT.Recorder(), []

    def sample_fn(x, noise=None, **inp):
        calls.append((x, noise, inp))
        return torch.zeros_like(x)
    split = lambda image, target_shape: torch.from_numpy(R.split_block(image.numpy(), target_shape[2]))
    monkeypatch.setattr(inference, 'ops', LT.RecordingOps(rec))
    monkeypatch.setattr(inference, 'convertVolume2subVolume', split)                       # the block as the sampler sees it, on the CPU
    monkeypatch.setattr(inference, 'merge_sub_volumes',
                        lambda sub_volumes, original_shape: torch.from_numpy(R.merge_block(sub_volumes.numpy(), original_shape[2])))
    kw = dict(blend='constant', samples=2) if mode == 'blend' else {}
    inf = inference.VolumeInference(cfg, sample_fn, noise='anchored', seed=3, inpaint=(known, mask), inpaint_resample_times=4, **kw)
    inf(vol)
    P = inf.patch
    origins = [r['idx']['index'] for r in rec.trace if r['op'] == 'patch_gather' and r['want_patches'] and r['mean'] == 300.0]
    assert len(calls) == len(origins) * (2 if mode == 'blend' else 1) >= 2
    for n, (x, noise, inp) in enumerate(calls):
        assert callable(noise) and sorted(inp) == ['inpaint_images', 'inpaint_masks', 'inpaint_resample_times']
        assert inp['inpaint_resample_times'] == 4
        kw_, mw = inp['inpaint_images'], inp['inpaint_masks']
        assert kw_.shape == x.shape and kw_.dtype == torch.float32 and mw.dtype == torch.bool and tuple(mw.shape) == (x.shape[0], *x.shape[2:])
        cut = lambda v: torch.stack([v[i:i + P, j:j + P, k:k + P] for i, j, k in origins[n // (2 if mode == 'blend' else 1)]])[:, None]
        want_k, want_m = cut(known), cut(mask)
        if block:
            shape = (inf.factor ** 3, 1, inf.sub, inf.sub, inf.sub)
            want_k, want_m = split(want_k, shape), split(want_m, shape)
        assert torch.equal(kw_, want_k) and torch.equal(mw, want_m[:, 0]) and mw.any()


def test_window_denoisers_keep_refusing_inpainting_and_gain_the_state_space_map():
    elu = HN.make_elucidated('churn-on', False)
    lr = torch.zeros(2, 1, 16, 16, 16)
    for kw in (dict(), dict(sampler='dpmpp2m', sample_steps=4)):
        with pytest.raises(ValueError, match="inpaint"):
            elu.window_denoiser(inpaint_images=lr, inpaint_masks=lr[:, 0].bool(), **kw)
    den = elu.window_denoiser()
    x = torch.linspace(-2, 2, 7)
    assert torch.equal(den.normalize(x), elu.normalize_img(x))


def test_sample_inpaint_argument_errors():
    elu = HN.make_elucidated('churn-on', False)
    lr = torch.zeros(2, 1, 16, 16, 16)
    masks = torch.zeros(2, 16, 16, 16, dtype=torch.bool)

    def never(shape):
        raise AssertionError("the noise source must not be called")
    call = dict(batch_size=2, video_frames=16, start_image_or_video=lr, start_at_unet_number=2, use_tqdm=False, noise=never)
    with pytest.raises(ValueError, match="inpaint"):
        elu.sample(inpaint_images=lr, **call)
    with pytest.raises(ValueError, match="inpaint"):
        elu.sample(inpaint_masks=masks, **call)
    with pytest.raises(ValueError, match="inpaint"):
        elu.sample(inpaint_images=lr, inpaint_masks=masks, sampler='dpmpp2m', **call)
    for bad in (0, -2, 1.5, True, None):
        with pytest.raises(ValueError, match="inpaint"):
            elu.sample(inpaint_images=lr, inpaint_masks=masks, inpaint_resample_times=bad, **call)
    with pytest.raises(ValueError, match="inpaint"):                             # three images for a batch of two
        elu.sample(inpaint_images=torch.zeros(3, 1, 16, 16, 16), inpaint_masks=torch.zeros(3, 16, 16, 16, dtype=torch.bool), **call)
    unet = elu.unets[1]
    with pytest.raises(ValueError, match="inpaint"):                             # the same rules one level down
        elu.one_unet_sample(unet, (2, 1, 16, 16, 16), unet_number=2, inpaint_images=lr, inpaint_masks=masks, sampler='dpmpp2m')
    with pytest.raises(ValueError, match="inpaint"):
        elu.one_unet_sample(unet, (2, 1, 16, 16, 16), unet_number=2, inpaint_masks=masks)


# ---- H3: the draws ``sample`` takes from a noise list ------------------------------------------------------------------------------------
@pytest.mark.parametrize('resample', [1, 2])
def test_sample_takes_the_draws_the_reference_took(resample, monkeypatch):
    """``sample`` hands ``one_unet_sample`` the entries of the ``noise`` list that are its U-Net's; with the low-res noise before them
    that is the queue length the reference consumed when tests/golden/edm_inpaint.npz was made (3 steps: 5 at R = 1, 10 at R = 2)."""
    from diffusioniqt_amd.elucidated_imagen import ElucidatedImagen
    g = load_golden('edm_inpaint')
    consumed = int(g[f'consumed{resample}'])
    assert consumed == g[f'draws{resample}'].shape[0] == 2 + ElucidatedImagen.inpaint_draws(3, resample)
    elu = HN.make_elucidated('churn-on', False, size=8, num_sample_steps=3)
    seen = {}

    def one_unet_sample(unet, shape, *, noise, inpaint_images, inpaint_masks, inpaint_resample_times, **kw):
        seen.update(n=len(noise), shape=tuple(shape), R=inpaint_resample_times, B=inpaint_images.shape[0], masks=tuple(inpaint_masks.shape))
        return torch.zeros(shape)
    monkeypatch.setattr(elu, 'one_unet_sample', one_unet_sample)
    monkeypatch.setattr(elu, '_noise_lowres', lambda lowres, times, noise: lowres)
    spare = 3
    noise = [torch.zeros(1, 1, 8, 8, 8) for _ in range(consumed + spare)]
    elu.sample(video_frames=8, start_image_or_video=torch.zeros(1, 1, 8, 8, 8), start_at_unet_number=2, use_tqdm=False, noise=noise,
               inpaint_images=torch.from_numpy(g['known']), inpaint_masks=torch.from_numpy(g['mask']).bool(),
               inpaint_resample_times=resample, device='cpu')
    assert seen == dict(n=consumed - 1, shape=(1, 1, 8, 8, 8), R=resample, B=1, masks=(1, 8, 8, 8))
    # batch_size 1 broadcasts along the inpainted images
    two = dict(inpaint_images=torch.zeros(2, 1, 8, 8, 8), inpaint_masks=torch.zeros(2, 8, 8, 8, dtype=torch.bool))
    elu.sample(video_frames=8, start_image_or_video=torch.zeros(2, 1, 8, 8, 8), start_at_unet_number=2, use_tqdm=False,
               noise=[torch.zeros(2, 1, 8, 8, 8) for _ in range(consumed)], inpaint_resample_times=resample, device='cpu', **two)
    assert seen['shape'] == (2, 1, 8, 8, 8) and seen['n'] == consumed - 1


# ---- H4: error codes of the two entries ----------------------------------------------------------------------------------------------------
def test_edm_inpaint_churn_entry_returns_error_codes():
    from diffusioniqt_amd import _lib, ops
    lib = _lib.load()
    buf = (np.zeros(4, dtype=np.int32)).ctypes.data                             # never dereferenced: every call below is refused
    for hole in (0, 2, 3, 4, 6, 7):                                              # x, known, mask, eps, kc, out
        args = [buf] * 8
        args[hole] = None
        assert lib.diqt_edm_inpaint_churn(*args, 2, 1000, None) == -2           # DIQT_E_ALIGN
        assert b"null pointer" in lib.diqt_last_error()
    assert lib.diqt_edm_inpaint_churn(buf, buf, buf, buf, buf, None, buf, buf, 2, 1000, None) == -2     # a re-noise without kr
    assert lib.diqt_edm_inpaint_churn(*([buf] * 8), 0, 1000, None) == -1        # DIQT_E_SHAPE
    assert lib.diqt_edm_inpaint_churn(*([buf] * 8), 2, 0, None) == -1
    assert lib.diqt_edm_inpaint_churn(*([buf] * 8), 65536, 1000, None) == -1
    x = torch.zeros(2, 1, 4, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):                   # the product refuses CPU tensors
        ops.edm_inpaint_churn(x, None, x, x.bool(), x, None, torch.zeros(2))


def test_joint_heun_inpaint_entry_returns_error_codes():
    from diffusioniqt_amd import _lib
    lib = _lib.load()
    buf = (np.zeros(4, dtype=np.int32)).ctypes.data                             # never dereferenced: every call below is refused
    geo = (40, 36, 44, 16, 8, 4, 3, 4)                                          # D, H, W, P, stride and the lattice of range(0, n - 15, 8)

    def entry(y, slot, taps, xh, xn, x0, known, mask, phase=2, geo=geo, mode=1, draw=2):
        return lib.diqt_volume_joint_heun_inpaint(y, slot, taps, xh, xn, x0, known, mask, phase, 3, *geo, 0.5, 0.5, 0.0, 0.0, 0.25, 0.0,
                                                  -1.0, 1.0, mode, 0, draw, draw + 1 if draw < 2 ** 32 - 1 else 0, 0, None)
    for hole in range(8):                                                        # the corrector needs all eight
        args = [buf] * 8
        args[hole] = None
        assert entry(*args) == -2                                               # DIQT_E_ALIGN
        assert b"null pointer" in lib.diqt_last_error()
    for phase, needed in ((0, (3, 6, 7)), (3, (3, 4, 6, 7))):                    # init: xh, known, mask; re-churn: xn as well
        for hole in needed:
            args = [None, None, None, buf, buf if phase == 3 else None, None, buf, buf]
            args[hole] = None
            assert entry(*args, phase=phase) == -2
    assert entry(None, None, None, buf, None, None, buf, buf, phase=0, geo=(0, 36, 44, 0, 0, 0, 0, 0)) == -1      # DIQT_E_SHAPE: a volume ...
    assert entry(None, None, None, buf, None, None, buf, buf, phase=0, draw=2 ** 32 - 1) == -1                    # ... and room for draw + 1
    assert b"draw + 1" in lib.diqt_last_error()
    assert entry(*([buf] * 8), geo=(40, 36, 44, 16, 8, 4, 3, 5)) == -1           # not the lattice
    assert b"lattice" in lib.diqt_last_error()
    assert entry(*([buf] * 8), geo=(40, 36, 44, 16, 0, 4, 3, 4)) == -1
    assert entry(*([buf] * 8), geo=(40, 36, 44, 48, 8, 1, 1, 1)) == -1           # a window larger than the volume
    for phase in (1, 4, -1):                                                     # the predictor is diqt_volume_joint_heun's
        assert entry(*([buf] * 8), phase=phase) == -3                           # DIQT_E_UNSUPPORTED
        assert b"phase" in lib.diqt_last_error()
    assert entry(*([buf] * 8), mode=2) == -3
    # and the existing entry still has no phase 3
    assert lib.diqt_volume_joint_heun(*([buf] * 6), 3, 3, *geo, 0.5, 0.5, 0.0, 0.0, 0.0, -1.0, 1.0, 1, 0, 2, 0, None) == -3
