"""Host-side checks of DDPM inpainting on the joint volume state (no GPU here): at stride = patch the float64 specification of
tests/volume_joint_ddpm_inpaint_reference.py is the reference's RePaint loop (imagen_pytorch3D.py:2116-2146, as the oracle transcribes
it) run per window, its derived bound dominates an fp32 emulation of the same chain and is small beside the signal, the draw count is
what the reference consumed when tests/golden/ddpm_inpaint.npz was made, the chain issues 1 + R T fused launches with the draw indices
and flags of the per-window loop, the two new entries return error codes, and ``VolumeInference`` admits the ancestral denoiser alone.

No case is left to the bit-for-bit ties alone: the re-noise contracts an error (kr0 < 1) and a paste resets it, so also under dynamic
thresholding, which doubles every gain of the evaluation, the bound stays below 1e-3 of the peak-to-peak (1.3e-5 .. 3.7e-5 of it in the
cases here) and the dynamic chains are compared under it like the static ones."""
import numpy as np
import pytest
import torch

from tests import volume_blend_reference as R
from tests import volume_joint_ddpm_inpaint_reference as DP
from tests import volume_joint_inpaint_reference as IP
from tests import volume_joint_reference as J
from tests.conftest import load_golden
from tests.test_volume_joint_host import _imagen

TILINGS = ((8, 'gaussian'), (5, 'constant'))
STATIC = (J.MIN_BOUND, 0., 0)
MODES = {'static': (STATIC, None), 'dynamic': ((-1., 1., 1), (0.95, 1.0))}          # (the data normalisation's clamp, (percentile, floor))
CASES = [(mode, resample, tiling) for mode, passes in (('static', (1, 2, 3)), ('dynamic', (1, 2))) for resample in passes
         for tiling in TILINGS]
IDS = [f"{m}-R{r}-s{t[0]}-{t[1]}" for m, r, t in CASES]
_TABS = {}


def tabs():
    if 'x' not in _TABS:
        from diffusioniqt_amd.imagen_pytorch3D import GaussianDiffusionContinuousTimes
        _TABS['x'] = DP.tables(GaussianDiffusionContinuousTimes(noise_schedule='cosine', timesteps=1000), DP.STEPS, 'x_start')
        for v in _TABS['x'].values():
            v.setflags(write=False)
    return _TABS['x']


# ---- H1: the specification alone ------------------------------------------------------------------------------------------------------------
def test_tables_are_the_denoisers_and_the_last_step_adds_no_noise():
    t = tabs()
    den = _imagen().window_denoiser(sampler='ddpm', sample_steps=DP.STEPS)
    for name in ('coefs', 'qs', 'renoise'):
        got = getattr(den, name)
        assert got.dtype == torch.float32 and not got.is_cuda and np.array_equal(got.numpy().astype(np.float64), t[name]), name
    assert tuple(den.qs.shape) == tuple(den.renoise.shape) == (DP.STEPS, 2)
    assert (t['coefs'][:-1, 2] > 0).all() and t['coefs'][-1, 2] == 0
    assert (t['renoise'][:-1, 0] < 1).all() and (t['renoise'][:-1, 1] > 0).all()           # kr0 = alpha / alpha_next < 1: no error gain
    x = torch.linspace(-2, 2, 7)
    assert torch.equal(den.normalize(x), x)                                               # auto_normalize_img is off: the identity


@pytest.mark.parametrize('resample', [1, 2, 3])
def test_reference_is_the_reference_loop_per_window_at_stride_equal_patch(resample, monkeypatch):
    """Stride = patch, constant blend: every fused prediction is the one window's own, so the joint chain is the reference's loop run
    per kept window on the window's cut of the anchored normals, numbered by the one counter.  The oracle forms its posterior and
    re-noise coefficients itself (``q_posterior``, ``q_sample_from_to``), in fp32 as the reference does."""
    from oracle import iqt_oracle as O
    vol, cfg = R.shared_volume(), R.shared_cfg(16)
    known, mask = IP.inpaint_inputs()
    ref = DP.joint_reference(vol, cfg, tabs(), 'x_start', STATIC, 'constant', known, mask, resample)
    assert ref['draws'] == DP.draws_of(DP.STEPS, resample)
    L = J.layout(vol, cfg)
    low = (vol - np.float32(300.0)) / np.float32(200.0)
    draws = [torch.from_numpy(J.normals(vol.shape, DP.SEED, k, 0).copy()) for k in range(ref['draws'])]
    cut = lambda a, o: a[o[0]:o[0] + 16, o[1]:o[1] + 16, o[2]:o[2] + 16][None, None]
    stub = lambda sd, cfg, img, t, log_snr, lowres_cond_img=None: 0.5 * (img / (1.0 + img.abs())) + 0.25 * lowres_cond_img \
        + 0.015625 * log_snr.double().view(-1, 1, 1, 1, 1)
    monkeypatch.setattr(O, 'unet_forward', stub)
    worst = 0.0
    for o in L['kept']:
        w = [cut(d, o).double() for d in draws]
        want, _, _ = O.p_sample_loop(None, None, torch.from_numpy(cut(low, o)).double(), w[0], w[1:], timesteps=DP.STEPS,
                                     min_bound=J.MIN_BOUND, inpaint_images=torch.from_numpy(cut(known, o)).double(),
                                     inpaint_masks=torch.from_numpy(cut(mask, o)), inpaint_resample_times=resample)
        keep = ~cut(ref['background'], o)
        worst = max(worst, float(np.abs(cut(ref['mean'], o) - want.numpy())[keep].max()))
    print(f"ddpm inpaint reference vs the reference's loop per window (R {resample}): {worst:.3e}, bound {ref['bound']:.3e}")
    assert L['kept'].shape[0] >= 2 and worst <= ref['bound']


@pytest.mark.parametrize('mode,resample,tiling', CASES, ids=IDS)
def test_chain_bound_dominates_an_fp32_emulation_and_is_small_beside_the_signal(mode, resample, tiling):
    """The project's pair of conditions on a derived bound, over covered, non-background, unmasked voxels."""
    stride, blend = tiling
    vol, cfg = R.shared_volume(), R.shared_cfg(stride)
    known, mask = IP.inpaint_inputs()
    clamp, dyn = MODES[mode]
    ref = DP.joint_reference(vol, cfg, tabs(), 'x_start', clamp, blend, known, mask, resample, dyn=dyn)
    emu = DP.joint_reference(vol, cfg, tabs(), 'x_start', clamp, blend, known, mask, resample, dyn=dyn, dtype=np.float32)
    live = ref['covered'] & ~ref['background']
    free = live & ~mask
    assert ref['draws'] == DP.draws_of(DP.STEPS, resample)
    assert (live & mask).sum() > 1000 and free.sum() > 1000
    err = np.abs(emu['mean'] - ref['mean'])[live].max()
    ptp = np.ptp(ref['mean'][free])
    print(f"ddpm inpaint chain {mode} R {resample} stride {stride} {blend}: fp32 emulation / bound = {err / ref['bound']:.3f} (err "
          f"{err:.3e}, bound {ref['bound']:.3e}), bound / ptp = {ref['bound'] / ptp:.3e} (ptp {ptp:.3f}, largest |state| "
          f"{ref['state']:.2f}, |x0| {ref['x0']:.2f})")
    assert err <= ref['bound']
    assert ref['bound'] <= 1e-3 * ptp
    # the known region steers the chain: not the chain with nothing masked
    plain = DP.joint_reference(vol, cfg, tabs(), 'x_start', clamp, blend, known, np.zeros_like(mask), resample, dyn=dyn)
    assert np.abs(plain['mean'] - ref['mean'])[live & mask].max() > 1e-2


def test_an_empty_mask_and_one_pass_is_the_plain_chain():
    """Nothing masked, R = 1: the posterior chain of ``volume_joint_reference`` on draws 0, 2, 4, ... (the q-noise is drawn and unused)."""
    vol, cfg = R.shared_volume(), R.shared_cfg(8)
    known, mask = IP.inpaint_inputs()
    t = tabs()
    got, L, _, draws = DP.joint_chain(vol, cfg, t, 'x_start', STATIC, 'gaussian', known, np.zeros_like(mask), 1)
    assert draws == 1 + 2 * DP.STEPS
    x = J.normals(vol.shape, DP.SEED, 0, 0).copy()
    taps = R.taps_of(16, 'gaussian')
    cut = lambda a, o: a[o[0]:o[0] + 16, o[1]:o[1] + 16, o[2]:o[2] + 16][None, None]
    low = ((vol - np.float32(300.0)) / np.float32(200.0)).astype(np.float64)
    for i in range(DP.STEPS):
        y = np.stack([J.stub64(cut(x, o), cut(low, o), np.full(1, t['log_snr'][i]))[0, 0] for o in L['kept']])
        n = J.normals(vol.shape, DP.SEED, 2 + 2 * i, 0) if t['coefs'][i, 2] != 0 else None
        x, _, covered = J.joint_step(y, L['slot'], taps, 8, x, *t['coefs'][i], J.clamp_of(*STATIC), n)
    assert covered.any() and np.abs(got - x)[covered].max() <= 1e-12


# ---- H2: the draws ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('resample', [1, 2])
def test_inpaint_draws_is_what_the_reference_consumed(resample):
    from diffusioniqt_amd.imagen_pytorch3D import Imagen
    g = load_golden('ddpm_inpaint')
    T = int(g['timesteps'])
    assert Imagen.inpaint_draws(T, resample) == int(g[f'consumed{resample}']) == g[f'draws{resample}'].shape[0]
    assert Imagen.inpaint_draws(T, resample) == DP.draws_of(T, resample)
    assert float(g['d1']) > 0 and float(g['d2']) > 0


# ---- H3: the launches -----------------------------------------------------------------------------------------------------------------------
class _AncestralStub:
    """Three steps of the ancestral chain with its inpainting tables; records like the stand-ins of the launch-trace test."""
    num_steps, clamp = 3, (-1.0, 1.0, 1)

    def __init__(self, rec, self_cond):
        self.rec, self.self_cond = rec, self_cond
        self.coefs = torch.tensor([[0.5, 0.25, 0.125], [0.75, 0.375, 0.0625], [0.875, 0.4375, 0.0]])
        self.qs = torch.tensor([[0.125, 0.96875], [0.5, 0.84375], [0.875, 0.46875]])
        self.renoise = torch.tensor([[0.25, 0.8125], [0.5625, 0.71875], [1.0, 0.0]])

    def normalize(self, x):
        return x

    def x0(self, img, lowres, i, self_cond=None):
        return self.rec.record('x0', {'img': img, 'lowres': lowres, 'i': i, 'self_cond': self_cond}, torch.zeros_like(img))

    def finish(self, x, known=None, mask=None):
        return self.rec.record('finish', {'x': x, 'known': known, 'mask': mask}, torch.zeros_like(x))


@pytest.mark.parametrize('self_cond', [False, True], ids=['plain', 'selfcond'])
@pytest.mark.parametrize('resample', [1, 2, 3])
def test_chain_issues_one_fused_launch_per_pass(resample, self_cond, monkeypatch):
    from diffusioniqt_amd import inference
    from tests import test_volume_launch_trace_host as LT
    monkeypatch.setitem(LT.RETURNS, 'volume_joint_step_inpaint_init', lambda a: LT.zeros(*a['known'].shape))
    monkeypatch.setitem(LT.RETURNS, 'volume_joint_step_inpaint', lambda a: a['x'])
    rec = LT.Recorder()
    monkeypatch.setattr(inference, 'ops', LT.RecordingOps(rec))
    vol = torch.from_numpy(R.shared_volume())
    known, mask = (torch.from_numpy(a) for a in IP.inpaint_inputs())
    den = _AncestralStub(rec, self_cond)
    inference.VolumeInference(R.shared_cfg(8, batch_size=3), den, blend='gaussian', noise='anchored', joint=True, seed=5,
                              inpaint=(known, mask), inpaint_resample_times=resample)(vol)
    T = 3
    names = [r['op'] for r in rec.trace]
    assert not any(n in names for n in ('volume_joint_init', 'volume_joint_step', 'volume_joint_heun', 'volume_joint_multistep'))
    init = [r for r in rec.trace if r['op'] == 'volume_joint_step_inpaint_init']
    steps = [r for r in rec.trace if r['op'] == 'volume_joint_step_inpaint']
    assert len(init) == 1 and len(steps) == resample * T                               # 1 + R T fused launches
    assert (init[0]['draw'], init[0]['draw_q'], init[0]['al'], init[0]['sg']) == (0, 1, 0.125, 0.96875)
    plan = DP.pass_plan(T, resample)
    draw = 2
    state = init[0]['->']['t']
    for n, (rcd, (i, r, more, ren)) in enumerate(zip(steps, plan)):
        assert rcd['flags'] == int(ren) + 2 * int(more)
        assert rcd['x']['t'] == state and rcd['->']['t'] == state                       # in place on the one state
        assert [rcd['kx'], rcd['k0'], rcd['kn']] == den.coefs[i].tolist()
        assert rcd['draw'] == draw
        assert rcd['draw_r'] == (draw + 1 if ren else 0)
        assert rcd['draw_q'] == (draw + 1 + ren if more else 0)
        assert rcd['kr'] == (den.renoise[i].tolist() if ren else [0.0, 0.0])
        assert rcd['q'] == (den.qs[plan[n + 1][0]].tolist() if more else [0.0, 0.0])
        assert (rcd['x0_out'] is not None) == self_cond
        draw += 1 + int(ren) + int(more)
    from diffusioniqt_amd.imagen_pytorch3D import Imagen
    assert draw == Imagen.inpaint_draws(T, resample)
    # every evaluation but the first gathers the fused x0 volume when the network self-conditions
    evals = [r for r in rec.trace if r['op'] == 'x0']
    per_pass = len(evals) // (resample * T)
    assert len(evals) == per_pass * resample * T and per_pass >= 2
    assert all((e['self_cond'] is not None) == (self_cond and k >= per_pass) for k, e in enumerate(evals))
    assert [e['i'] for e in evals[::per_pass]] == [i for i, *_ in plan]
    fin = [r for r in rec.trace if r['op'] == 'finish']
    assert len(fin) == 1 and fin[0]['x']['t'] == state and fin[0]['known'] is not None and fin[0]['mask'] is not None


# ---- H4: error codes of the two entries ------------------------------------------------------------------------------------------------------
def test_ddpm_inpaint_paste_entry_returns_error_codes():
    from diffusioniqt_amd import _lib, ops
    lib = _lib.load()
    buf = (np.zeros(4, dtype=np.int32)).ctypes.data                             # never dereferenced: every call below is refused
    for hole in (0, 2, 3, 4, 7, 8, 9):                                           # x, known, mask, qnoise, al, sg, out
        args = [buf] * 10
        args[hole] = None
        assert lib.diqt_ddpm_inpaint_paste(*args, 2, 1000, None) == -2          # DIQT_E_ALIGN
        assert b"null pointer" in lib.diqt_last_error()
    for hole in (5, 6):                                                          # a re-noise without one of its coefficients
        args = [buf] * 10
        args[hole] = None
        assert lib.diqt_ddpm_inpaint_paste(*args, 2, 1000, None) == -2
    assert lib.diqt_ddpm_inpaint_paste(*([buf] * 10), 0, 1000, None) == -1      # DIQT_E_SHAPE
    assert lib.diqt_ddpm_inpaint_paste(*([buf] * 10), 2, 0, None) == -1
    assert lib.diqt_ddpm_inpaint_paste(*([buf] * 10), 65536, 1000, None) == -1
    x = torch.zeros(2, 1, 4, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):                   # the product refuses CPU tensors
        ops.ddpm_inpaint_paste(x, None, x, x.bool(), x, None, None, torch.zeros(2), torch.zeros(2))


def test_joint_step_inpaint_entry_returns_error_codes():
    from diffusioniqt_amd import _lib
    lib = _lib.load()
    buf = (np.zeros(4, dtype=np.int32)).ctypes.data                             # never dereferenced: every call below is refused
    geo = (40, 36, 44, 16, 8, 4, 3, 4)                                          # D, H, W, P, stride and the lattice of range(0, n - 15, 8)

    def entry(y, slot, taps, x, x0, known, mask, phase=1, flags=3, geo=geo, mode=1):
        return lib.diqt_volume_joint_step_inpaint(y, slot, taps, x, x0, known, mask, phase, flags, 3, *geo, 0.5, 0.5, 0.25, 0.5, 0.5, 0.5,
                                                  0.5, -1.0, 1.0, mode, 0, 2, 3, 4, 0, None)
    for hole in (0, 1, 2, 3, 5, 6):                                              # the step needs all but x0_out
        args = [buf] * 7
        args[hole] = None
        assert entry(*args) == -2                                               # DIQT_E_ALIGN
        assert b"null pointer" in lib.diqt_last_error()
    for hole in (3, 5, 6):                                                       # the initial state: x, known, mask
        args = [None, None, None, buf, None, buf, buf]
        args[hole] = None
        assert entry(*args, phase=0) == -2
    assert entry(None, None, None, buf, None, buf, buf, phase=0, geo=(0, 36, 44, 0, 0, 0, 0, 0)) == -1          # DIQT_E_SHAPE
    assert entry(*([buf] * 7), geo=(40, 36, 44, 16, 8, 4, 3, 5)) == -1           # not the lattice
    assert b"lattice" in lib.diqt_last_error()
    assert entry(*([buf] * 7), geo=(40, 36, 44, 48, 8, 1, 1, 1)) == -1           # a window larger than the volume
    for phase in (2, -1):
        assert entry(*([buf] * 7), phase=phase) == -3                           # DIQT_E_UNSUPPORTED
        assert b"phase" in lib.diqt_last_error()
    for flags in (4, -1):
        assert entry(*([buf] * 7), flags=flags) == -3
        assert b"flags" in lib.diqt_last_error()
    assert entry(*([buf] * 7), mode=2) == -3


# ---- H5: who may inpaint on the joint state ------------------------------------------------------------------------------------------------
def test_volume_inference_admits_the_ancestral_denoiser_alone():
    from diffusioniqt_amd.inference import VolumeInference
    imagen = _imagen()
    known, mask = (torch.from_numpy(a) for a in IP.inpaint_inputs())
    joint = dict(blend='gaussian', noise='anchored', joint=True)
    for kw in (dict(), dict(paste_known=True)):
        den = imagen.window_denoiser(sampler='ddpm', sample_steps=DP.STEPS, **kw)
        assert den.paste_known == bool(kw)
        inf = VolumeInference(R.shared_cfg(8), den, inpaint=(known, mask), inpaint_resample_times=2, **joint)
        assert inf.inpaint is not None and inf.resample_times == 2
    stub = type('FirstOrder', (), dict(num_steps=3, coefs=torch.zeros(3, 3), clamp=(-1., 1., 1), x0=None, finish=None))()
    refused = [imagen.window_denoiser(sampler='ddim', sample_steps=DP.STEPS), imagen.window_denoiser(sampler='ddim', sample_steps=DP.STEPS, eta=1.0),
               imagen.window_denoiser(sampler='dpmpp2m', sample_steps=DP.STEPS), stub]
    for other in refused:
        assert not hasattr(other, 'qs') and not hasattr(other, 'renoise') and not hasattr(other, 'normalize')
        VolumeInference(R.shared_cfg(8), other, **joint)                          # fine without inpaint ...
        with pytest.raises(ValueError, match="inpaint"):                         # ... and refused with it
            VolumeInference(R.shared_cfg(8), other, inpaint=(known, mask), **joint)
    lr = torch.zeros(2, 1, 16, 16, 16)
    with pytest.raises(ValueError, match="inpaint"):                             # the denoiser itself keeps refusing images
        imagen.window_denoiser(sampler='ddpm', inpaint_images=lr, inpaint_masks=lr.bool())
    for sampler in ('ddim', 'dpmpp2m'):                                          # and sample refuses to inpaint with the others
        with pytest.raises(ValueError, match="inpaint"):
            imagen._check_sampler_args(sampler, 4, None, 0.0, True)


def test_trainer_window_denoiser_passes_paste_known_through():
    from diffusioniqt_amd.trainer import ImagenTrainer
    imagen = _imagen()
    imagen.configs = {'Data': {'norm': 'z-score'}, 'Train': {'batch_sample': False, 'patch_size_sub': 16, 'pred_obj': 'x_start'},
                      'Eval': {'repeat': 1}}
    ImagenTrainer.locked = False
    trainer = ImagenTrainer(configs=imagen.configs, imagen=imagen, verbose=False)
    assert trainer.window_denoiser(sampler='ddpm', sample_steps=3, paste_known=True).paste_known is True
    assert trainer.window_denoiser(sampler='ddpm', sample_steps=3).paste_known is False
