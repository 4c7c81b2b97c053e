"""Noise-aware data consistency (``consistency_noise=``) on a real MI355X against tests/volume_joint_noise_reference.py:
``ops.cell_project_noise`` and the fused joint step bit for bit against the fp32 restatement (no voxel is left out of a comparison) and
against the composition of the two parent ops, the joint chains of both families through ``VolumeInference(consistency_noise=...)``
against the float64 chains, and the bit-for-bit tie of the joint chain at stride = patch to ``sample(consistency=...,
consistency_noise=...)`` per window.  The shapes are those of tests/test_gpu_volume_dc.py.

Bounds: the reference module's docstring.  A chain test takes the family's ``chain_bound`` plus, per step, the projection's rounding
count for x0 plus kn times the same count taken with weight = shrink and S = max |eps|.  Observed on the MI355X: the figures each test
prints, recorded in DESIGN 4.13."""

import numpy as np
import pytest
import torch

from tests import anchored_noise_reference as A
from tests import edm_dpmpp2m_reference as E
from tests import volume_blend_reference as R
from tests import volume_joint_dc_reference as DC
from tests import volume_joint_heun_reference as HN
from tests import volume_joint_noise_reference as NR
from tests import volume_joint_profile_reference as PR
from tests import volume_joint_reference as J
from tests.test_gpu_volume_joint import stub_imagen

pytestmark = pytest.mark.gpu
DEV = "cuda"
CLAMPS = {'min': (-0.75, 0., 0), 'box': (-1., 1., 1), 'none': None}
SEED, SAMPLE = 0x123456789, 2
KX, K0, KP, KN = 0.8125, -0.9375, -0.3125, 0.625
PAIRS = {'full': (1.0, 1.0), 'partial': (0.5, 0.375)}         # (weight, shrink)
_CACHE = {}


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(t):
    return (t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)).view(np.uint32)


def cached(key, make):
    """One reference per case, shared by the tests that need it and never modified."""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def table_of(cell, profile):
    """(the reference's table, the op's table on the device), None for the plain mean; the same bits."""
    from diffusioniqt_amd import ops
    if profile is None:
        return None, None
    host, want = ops.cell_profile(cell, profile), PR.profile_table(cell, profile)
    assert np.array_equal(bits(host), bits(want))
    return want, host.to(DEV)


# ---- G1: the per-window launch, bit for bit ----------------------------------------------------------------------------------------------------
OPERATORS = {'mean-411': ((4, 1, 1), None), 'mean-118': ((1, 1, 8), None), 'mean-222': ((2, 2, 2), None), **PR.PROFILES}


@pytest.mark.parametrize('pair', list(PAIRS))
@pytest.mark.parametrize('clamp', list(CLAMPS))
@pytest.mark.parametrize('name', list(OPERATORS))
def test_cell_project_noise_is_the_reference_and_the_two_parent_ops(name, clamp, pair):
    """B C = 3 cubes of edge 8.  Fresh outputs (the inputs keep their bits), then in place on both pairs."""
    from diffusioniqt_amd import ops
    cell, profile = OPERATORS[name]
    table, dev = table_of(cell, profile)
    w, shrink = PAIRS[pair]
    rng = np.random.default_rng(5)
    x0 = (rng.standard_normal((3, 1, 8, 8, 8)) * 2).astype(np.float32)
    meas = NR.replicate(rng.standard_normal((3, 1) + tuple(8 // f for f in cell)).astype(np.float32), cell)
    eps = rng.standard_normal((3, 1, 8, 8, 8)).astype(np.float32)
    c = CLAMPS[clamp]
    want, want_n = NR.project_noise32(x0, meas, eps, cell, table, w, shrink, c)
    x, m, n = cu(x0), cu(meas), cu(eps)
    got, got_n = ops.cell_project_noise(x, m, n, cell, w, shrink, dev, clamp=c)
    assert len({t.data_ptr() for t in (x, n, got, got_n)}) == 4 and torch.equal(x, cu(x0)) and torch.equal(n, cu(eps))
    assert np.array_equal(bits(got), bits(want)) and np.array_equal(bits(got_n), bits(want_n))
    # the composition of the two parent ops: the projection of x0, and the projection of the normals onto a zero measurement
    zero = torch.zeros_like(n)
    if dev is None:
        old, old_n = ops.cell_project(x, m, cell, w, clamp=c), ops.cell_project(n, zero, cell, shrink, clamp=None)
    else:
        old, old_n = ops.cell_project_profile(x, m, cell, dev, w, clamp=c), ops.cell_project_profile(n, zero, cell, dev, shrink, clamp=None)
    assert torch.equal(got, old) and torch.equal(got_n, old_n)
    assert np.array_equal(bits(got), bits(old)) and np.array_equal(bits(got_n), bits(old_n))
    same, same_n = ops.cell_project_noise(x, m, n, cell, w, shrink, dev, clamp=c, out=x, out_noise=n)
    assert same.data_ptr() == x.data_ptr() and same_n.data_ptr() == n.data_ptr()
    assert np.array_equal(bits(x), bits(want)) and np.array_equal(bits(n), bits(want_n))
    if table is not None:
        gap = np.broadcast_to(PR.gains(table, cell, x0.shape) == 0, x0.shape)
        assert np.array_equal(bits(got_n)[gap], bits(eps)[gap]) and gap.any() == (name == 'gap')   # a gap voxel keeps its normal
    assert (bits(got_n) != bits(eps)).mean() > (0.4 if name == 'gap' else 0.9)


def test_cell_project_noise_argument_errors():
    from diffusioniqt_amd import ops
    x = torch.zeros(2, 1, 8, 8, 8, device=DEV)
    with pytest.raises(ValueError, match="consistency weight"):
        ops.cell_project_noise(x, x.clone(), x.clone(), (2, 2, 2), 0.0, 0.5)
    with pytest.raises(ValueError, match="consistency_noise"):
        ops.cell_project_noise(x, x.clone(), x.clone(), (2, 2, 2), 1.0, 0.0)
    with pytest.raises(ValueError, match="noise must have"):
        ops.cell_project_noise(x, x.clone(), x[:1].clone(), (2, 2, 2), 1.0, 0.5)
    with pytest.raises(ValueError, match="alias"):
        ops.cell_project_noise(x, x.clone(), x.clone(), (2, 2, 2), 1.0, 0.5, out_noise=x)
    with pytest.raises(ValueError, match="consistency profile table"):
        ops.cell_project_noise(x, x.clone(), x.clone(), (2, 2, 2), 1.0, 0.5, torch.zeros(2, 4, device=DEV))


# ---- G2: the fused joint step, bit for bit -------------------------------------------------------------------------------------------------
# one non-uniform profile per cell of the uniform step tests; (1, 1, 5) has zero weights at both ends
STEP_PROFILES = {(4, 1, 1): ((1, 3, 3, 1), (1,), (1,)), (1, 3, 1): ((1,), (1, 2, 1), (1,)), (1, 1, 5): ((1,), (1,), (0, 1, 2, 1, 0)),
                 (2, 2, 2): ((1, 2), (1, 1), (3, 1)), (1, 1, 7): ((1,), (1,), (1, 2, 4, 6, 4, 2, 1))}
assert tuple(STEP_PROFILES) == DC.STEP_CELLS


def _step_refs(stride, kind):
    def make():
        c = DC.step_case(stride, kind)
        c['fused'] = {name: NR.fuse32(c['y'], c['slot'], c['taps'], stride, DC.STEP_VOL, NR.clamp32(*cl))
                      for name, cl in (('min', CLAMPS['min']), ('box', CLAMPS['box']))}
        return c
    return cached(('step', stride, kind), make)


def _normals(draw):
    """The step's fp32 normals as the device draws them, checked against the float64 field of tests/anchored_noise_reference.py."""
    from diffusioniqt_amd import ops

    def make():
        n = ops.volume_joint_init(DC.STEP_VOL, SEED, sample=SAMPLE, draw=draw).cpu().numpy()
        want = A.normals(A.field(DC.STEP_VOL, 1, SEED, draw, SAMPLE))[0]
        assert np.abs(n - want).max() <= HN.EPS_N
        return n
    return cached(('n', draw), make)


@pytest.mark.parametrize('shrink', [1.0, 0.375])
@pytest.mark.parametrize('form', [0, 2])
@pytest.mark.parametrize('profiled', [False, True], ids=['mean', 'profile'])
@pytest.mark.parametrize('cell', DC.STEP_CELLS)
@pytest.mark.parametrize('tiling', DC.STEP_TILINGS, ids=['s4-gaussian', 's5-constant'])
def test_joint_noise_step_is_the_reference_bit_for_bit(tiling, cell, profiled, form, shrink):
    """Every voxel is compared: nothing is excluded.  The fresh launch, then the same launch in place (``x_next`` aliasing ``x_t`` and,
    with a history, ``x0_out`` aliasing ``x0_prev``).  A cell with an uncovered voxel keeps its plain x0 and its plain normal."""
    from diffusioniqt_amd import ops
    stride, kind = tiling
    c = _step_refs(stride, kind)
    clamp = 'min' if cell[2] != 1 else 'box'
    w, draw = (1.0, 5) if sum(cell) % 2 else (0.5, 3)
    table, dev = table_of(cell, STEP_PROFILES[cell] if profiled else None)
    meas, n = DC.step_meas(c, cell), _normals(draw)
    with_prev = form == 2
    want, want0, covered = NR.joint_step_noise32(c['y'], c['slot'], c['taps'], stride, c['x'], c['prev'] if with_prev else None, meas, cell,
                                                 table, w, shrink, form, KX, K0, KP, KN, None, n, fused=c['fused'][clamp])
    whole = NR.replicate(NR._cells(covered, cell).all(axis=(-5, -3, -1)), cell)
    assert whole.any() and (~covered).any() and (covered[:16, :16, :64] == False).any()         # uncovered voxels inside the volume too
    args = (cu(c['y']), cu(c['slot'].astype(np.int32)), cu(c['taps']))
    tail = (cu(meas), cell, dev, w, shrink, form, KX, K0, KP, KN, *CLAMPS[clamp], stride, SEED, draw, SAMPLE)
    x, prev = cu(c['x']), cu(c['prev']) if with_prev else None
    got, got0 = ops.volume_joint_consistent_noise_step(*args, x, prev, *tail)
    assert got.data_ptr() != x.data_ptr() and torch.equal(x, cu(c['x']))
    bad, bad0 = (bits(got) != bits(want)).sum(), (bits(got0) != bits(want0)).sum()
    print(f"noise step form {form} stride {stride} {kind} cell {cell} {'profile' if profiled else 'mean'} w {w} shrink {shrink}: "
          f"{bad} / {bad0} of {want.size} voxels differ; corrected share {whole.mean():.3f}")
    assert bad == 0 and bad0 == 0
    assert np.array_equal(bits(got)[~covered], bits(c['x'])[~covered]) and not got0.cpu().numpy()[~covered].any()
    # against the constant-weight launch: the same x0', another state exactly where a normal was shaped
    old = (ops.volume_joint_consistent_step(*args, x, prev, cu(meas), cell, *tail[3:4], *tail[5:]) if dev is None else
           ops.volume_joint_consistent_profile_step(*args, x, prev, cu(meas), cell, dev, *tail[3:4], *tail[5:]))
    assert torch.equal(got0, old[1])
    moved = bits(got) != bits(old[0])
    assert not moved[~whole].any() and moved[whole].mean() > 0.5
    ops.volume_joint_consistent_noise_step(*args, x, prev, *tail, out=x, x0_out=prev)
    assert torch.equal(x, got) and (prev is None or torch.equal(prev, got0))


def test_joint_noise_step_refusals():
    """Form 1, kn = 0 and shrink = 0 are DIQT_E_UNSUPPORTED (-3) at the entry, with real device buffers; ``ops`` refuses them first."""
    from diffusioniqt_amd import _lib, ops
    c = _step_refs(4, 'gaussian')
    y, slot, taps, x = cu(c['y']), cu(c['slot'].astype(np.int32)), cu(c['taps']), cu(c['x'])
    meas, out, out0 = cu(DC.step_meas(c, (2, 2, 2))), torch.empty_like(x), torch.empty_like(x)
    lib = _lib.load()

    def entry(form, kn, shrink):
        ptr = lambda t: None if t is None else t.data_ptr()
        return lib.diqt_volume_joint_consistent_noise_step(ptr(y), ptr(slot), ptr(taps), ptr(x), None, ptr(meas), None, ptr(out), ptr(out0),
                                                           form, y.shape[0], *x.shape, 8, 4, *slot.shape, 2, 2, 2, 1.0, shrink, KX, 0.5, 0.0,
                                                           kn, -1.0, 1.0, 1, SEED, 1, 0, None)
    assert entry(1, KN, 0.5) == -3 and entry(0, 0.0, 0.5) == -3 and entry(2, 0.0, 0.5) == -3 and entry(0, KN, 0.0) == -3
    assert entry(0, KN, 1.5) == -3
    torch.cuda.synchronize()
    for form, kn, shrink in ((1, KN, 0.5), (0, 0.0, 0.5), (0, KN, 0.0)):
        with pytest.raises(ValueError, match="volume_joint_consistent_noise_step"):
            ops.volume_joint_consistent_noise_step(y, slot, taps, x, None, meas, (2, 2, 2), None, 1.0, shrink, form, KX, 0.5, 0.0, kn, -1.0,
                                                   1.0, 1, 4)
    with pytest.raises(ValueError, match="consistency weight"):
        ops.volume_joint_consistent_noise_step(y, slot, taps, x, None, meas, (2, 2, 2), None, 0.0, 0.5, 0, KX, 0.5, 0.0, KN, -1.0, 1.0, 1, 4)


# ---- G3: the chains through VolumeInference against the float64 reference ----------------------------------------------------------------------
CHAIN_VOL, CHAIN_P, CHAIN_STRIDE = (16, 16, 24), 8, 4
CHAIN_CELLS = [(2, 2, 2), (4, 1, 1)]
SIGMA_STATE = 0.2


def chain_volume():
    vol = np.random.default_rng(7).integers(1, 1000, CHAIN_VOL).astype(np.float32)
    vol[:8, :8, :12] = 0                                       # the 5 % rule drops two windows: 4 x 4 x 8 voxels are covered by none
    return vol


def chain_cfg(stride=CHAIN_STRIDE, batch_size=7):
    return R.shared_cfg(stride, batch_size=batch_size, P=CHAIN_P)


def raw_sigma(den, cfg):
    """(the raw sigma whose state-space value is 0.2, that value as the chain computes it)."""
    unit = den.state_space(torch.tensor([0., 1.], dtype=torch.float64))
    slope, std = abs(float(unit[1] - unit[0])), float(cfg['Data']['std'])
    raw = SIGMA_STATE * std / slope
    return raw, raw / std * slope


VP = {'ddpm': ('ddpm', 0.0), 'ddim-eta0.5': ('ddim', 0.5)}


def vp_denoiser(imagen, sampler, eta):
    return imagen.window_denoiser(sampler=sampler, sample_steps=J.STEPS, eta=eta)


def check(got, ref, what):
    got = got.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == ref['mean'].shape and np.isfinite(got).all()
    err = np.abs(got.astype(np.float64) - ref['mean']).max()
    print(f"{what}: max |mean - ref| = {err:.3e}, bound {ref['bound']:.3e}; dispatch {ref['sched'].tolist()}")
    assert err <= ref['bound'], what
    return got


@pytest.mark.parametrize('cell', CHAIN_CELLS)
@pytest.mark.parametrize('name', list(VP))
def test_noise_aware_joint_chain_matches_the_float64_reference(name, cell):
    from diffusioniqt_amd.inference import VolumeInference
    imagen = stub_imagen('x_start', 'clamp-min', size=CHAIN_P)
    vol, cfg, w = chain_volume(), chain_cfg(), 1.0 if cell == (2, 2, 2) else 0.5
    den = vp_denoiser(imagen, *VP[name])
    raw, sigma = raw_sigma(den, cfg)
    meas = DC.measurement(vol, cell)

    def make():
        coefs = den.coefs.numpy().astype(np.float64)
        sched = NR.dispatch(NR.schedule64(NR.rows4(coefs), NR.cell_norm64(cell), sigma, w))
        log_snr = J.tables(imagen.noise_schedulers[1], J.STEPS, 0.0, 'x_start')[2]
        meas_up = DC.measurement_state(meas, cell, cfg)
        x, L, x0_max, eps_max = NR.vp_chain(vol, cfg, coefs, log_snr, (J.MIN_BOUND, 0., 0), 'gaussian', meas_up, cell, None, sched,
                                            seed=J.SEED)
        ref = DC.finish(vol, cfg, [np.maximum(x, J.MIN_BOUND)], L)
        ref.update(sched=sched, bound=NR.vp_bound(ref['windows_per_voxel'], ref['scale'], cell, None, sched, coefs[:, 2],
                                                  max(x0_max, float(np.abs(meas_up).max())), eps_max))
        return ref
    ref = cached(('vp', name, cell), make)
    assert (ref['sched'][:-1, 0] > 0).all() and ref['sched'][-1, 0] == 0 and (ref['sched'][:-1, 1] > 0).all()
    common = dict(blend='gaussian', noise='anchored', joint=True, seed=J.SEED, consistency=(torch.from_numpy(meas), cell), consistency_weight=w)
    got = check(VolumeInference(cfg, den, consistency_noise=raw, **common)(cu(vol)), ref, f"noise-aware joint {name} cell {cell} w {w}")
    constant = VolumeInference(cfg, den, **common)(cu(vol)).cpu().numpy()
    live = ref['covered'] & ~ref['background']
    assert (~ref['covered']).any() and np.abs(got - constant)[live].max() > 0.01            # and it is not the constant-weight chain


@pytest.mark.parametrize('cell', CHAIN_CELLS)
@pytest.mark.parametrize('eta', [1.0, 0.5])
def test_noise_aware_edm_joint_chain_matches_the_float64_reference(eta, cell):
    from diffusioniqt_amd.inference import VolumeInference
    elu = HN.make_elucidated('churn-on', False, size=CHAIN_P).to(DEV)
    den = elu.window_denoiser(sampler='dpmpp2m', eta=eta)
    vol, cfg = chain_volume(), chain_cfg()
    raw, sigma = raw_sigma(den, cfg)
    meas = DC.measurement(vol, cell)

    def make():
        tabs = E.tables(HN.HP, eta, coefs=den.coefs.numpy())
        rows = den.coefs.numpy().astype(np.float64)
        sched = NR.dispatch(NR.schedule64(rows, NR.cell_norm64(cell), sigma, 1.0))
        meas_up = DC.measurement_state(meas, cell, cfg)
        x, L, state_max, x0_max, eps_max = NR.edm_chain(vol, cfg, tabs, 'gaussian', False, meas_up, cell, None, sched)
        ref = DC.finish(vol, cfg, [np.clip(x, -1.0, 1.0)], L)
        mean32, std32 = np.float32(cfg['Data']['mean']), np.float32(cfg['Data']['std'])
        lowres_max = tabs['lowres'][0] * float(np.abs((vol - mean32) / std32).max()) + 6 * tabs['lowres'][1]
        ref.update(sched=sched, bound=NR.edm_bound(tabs, L, cell, None, sched, rows[:, 3], state_max, lowres_max, False,
                                                   max(x0_max, float(np.abs(meas_up).max())), eps_max))
        return ref
    ref = cached(('edm', eta, cell), make)
    assert (ref['sched'][:-1, 0] > 0).all() and ref['sched'][-1, 0] == 0
    inf = VolumeInference(cfg, den, blend='gaussian', noise='anchored', joint=True, seed=E.SEED, consistency=(torch.from_numpy(meas), cell),
                          consistency_noise=raw)
    check(inf(cu(vol)), ref, f"noise-aware joint EDM dpmpp2m eta {eta} cell {cell}")


# ---- G4: stride = patch: the joint chain is the per-window sampler ------------------------------------------------------------------------------
TIE = {'mean-222': ((2, 2, 2), None), 'mean-411': ((4, 1, 1), None), 'profile-222': ((2, 2, 2), ((1, 2), (1, 1), (3, 1))),
       'gap-411': ((4, 1, 1), ((0, 1, 1, 0), (1,), (1,)))}


def _tie_kw(cell, profile, raw):
    kw = dict(consistency=(torch.from_numpy(DC.measurement(chain_volume(), cell)), cell), consistency_weight=0.75, consistency_noise=raw)
    if profile is not None:
        kw.update(consistency_profile=profile)
    return kw


@pytest.mark.parametrize('operator', list(TIE))
@pytest.mark.parametrize('name', list(VP))
def test_noise_aware_joint_at_stride_equal_patch_is_the_independent_path(name, operator):
    """No overlap, unit weights: num / den is exact, no cell straddles a window, and a window's normals are the volume's: the fused
    launch is ``ops.cell_project_noise`` and the per-window step on every window -- one schedule, the same ``__device__`` projection
    for x0 and for the normals -- equal at every voxel, bit for bit."""
    from diffusioniqt_amd.inference import VolumeInference
    sampler, eta = VP[name]
    cell, profile = TIE[operator]
    for mode in ('clamp-min', 'dynamic'):
        imagen = stub_imagen('x_start', mode, size=CHAIN_P)
        vol, cfg = cu(chain_volume()), chain_cfg(stride=CHAIN_P)
        den = vp_denoiser(imagen, sampler, eta)
        cons = _tie_kw(cell, profile, raw_sigma(den, cfg)[0])

        def sample_fn(x, noise=None, **kw):
            assert set(kw) == set(cons)
            return imagen.sample(batch_size=x.shape[0], start_image_or_video=x, start_at_unet_number=2, use_tqdm=False, sampler=sampler,
                                 sample_steps=J.STEPS, eta=eta, noise=noise, **kw)[0]
        independent = VolumeInference(cfg, sample_fn, blend='constant', noise='anchored', seed=J.SEED, **cons)(vol)
        joint = VolumeInference(cfg, den, blend='constant', noise='anchored', joint=True, seed=J.SEED, **cons)(vol)
        constant = VolumeInference(cfg, den, blend='constant', noise='anchored', joint=True, seed=J.SEED,
                                   **{k: v for k, v in cons.items() if k != 'consistency_noise'})(vol)
        assert independent.unique().numel() > 1000 and not torch.equal(joint, constant)
        assert torch.equal(joint, independent), mode


@pytest.mark.parametrize('operator', list(TIE))
@pytest.mark.parametrize('eta', [1.0, 0.5])
def test_noise_aware_edm_joint_at_stride_equal_patch_is_the_independent_path(eta, operator):
    from diffusioniqt_amd.inference import VolumeInference
    cell, profile = TIE[operator]
    for dynamic in (False, True):
        elu = HN.make_elucidated('churn-on', dynamic, self_cond=True, size=CHAIN_P).to(DEV)
        vol, cfg = cu(chain_volume()), chain_cfg(stride=CHAIN_P)
        den = elu.window_denoiser(sampler='dpmpp2m', eta=eta)
        cons = _tie_kw(cell, profile, raw_sigma(den, cfg)[0])

        def sample_fn(x, noise=None, **kw):
            assert set(kw) == set(cons)
            return elu.sample(batch_size=x.shape[0], video_frames=CHAIN_P, start_image_or_video=x, start_at_unet_number=2, noise=noise,
                              sampler='dpmpp2m', eta=eta, use_tqdm=False, **kw)
        independent = VolumeInference(cfg, sample_fn, blend='constant', noise='anchored', seed=E.SEED, **cons)(vol)
        joint = VolumeInference(cfg, den, blend='constant', noise='anchored', joint=True, seed=E.SEED, **cons)(vol)
        assert independent.unique().numel() > 1000
        assert torch.equal(joint, independent), dynamic
