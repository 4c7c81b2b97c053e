"""Data consistency for overlapping slice profiles on a real MI355X against tests/volume_joint_slab_reference.py:
``ops.slab_measure`` / ``ops.slab_project`` and the three launches of the joint step bit for bit against the fp32 restatement (no
voxel is left out of a comparison), the joint chains of both families through ``VolumeInference(consistency_slab=...)`` against the
float64 chains, the bit-for-bit tie of the joint chain on a volume of one window to ``sample(consistency=..., consistency_slab=...)``,
and the argument errors of the ops.

Bounds: the reference's docstring.  The chain tests take the family's ``chain_bound`` plus ``steps`` times ``slab_roundings``, the
allowance of one projection, of which the fp32 restatement uses less than a quarter on the inputs of these tests
(tests/test_volume_slab_host.py)."""
import math

import numpy as np
import pytest
import torch

from tests import dpmpp2m_reference as M
from tests import edm_dpmpp2m_reference as E
from tests import volume_blend_reference as R
from tests import volume_joint_dc_reference as DC
from tests import volume_joint_heun_reference as HN
from tests import volume_joint_reference as J
from tests import volume_joint_slab_reference as SL
from tests.test_gpu_volume_joint import stub_imagen

pytestmark = pytest.mark.gpu
DEV = "cuda"
CLAMPS = {'min': (-0.75, 0., 0), 'box': (-1., 1., 1), 'none': None}
SEED, SAMPLE = 0x123456789, 2
KX, K0, KP = 0.8125, -0.9375, -0.3125
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


def table_of(cell, profile, jmax):
    """(the reference's table, the op's table on the device); they are the same bits (tests/test_volume_slab_host.py)."""
    from diffusioniqt_amd import ops
    host = ops.slab_profile(cell, profile, jmax=jmax)
    want = SL.table(cell, profile, jmax)
    assert np.array_equal(bits(host.table), bits(SL.flat(want)))
    return want, host.to(DEV)


# ---- G1: the operator and the per-window projection, bit for bit --------------------------------------------------------------------------
@pytest.mark.parametrize('case', range(len(SL.PROJECT_CASES)))
def test_slab_measure_is_the_reference_bit_for_bit(case):
    """The cubes stacked along z as one volume: the slices at its two ends take truncated sums."""
    from diffusioniqt_amd import ops
    cell, profile, P = SL.PROJECT_CASES[case]
    tab, dev = table_of(cell, profile, 3 * P // cell[0])
    x = SL.project_inputs(cell, P)[0].reshape(3 * P, P, P)
    got = ops.slab_measure(cu(x), cell, dev)
    want = SL.measure32(x, tab)
    assert tuple(got.shape) == want.shape == (3 * P // cell[0], P // cell[1], P // cell[2]) and np.array_equal(bits(got), bits(want))
    assert np.abs(want - SL.measure64(x, tab)).max() <= 32 * 2.0 ** -24 * np.abs(x).max()


@pytest.mark.parametrize('w', [1.0, 0.5])
@pytest.mark.parametrize('clamp', list(CLAMPS))
@pytest.mark.parametrize('case', range(len(SL.PROJECT_CASES)))
def test_slab_project_is_the_reference_bit_for_bit(case, clamp, w):
    """B C = 3 cubes; fresh output and in place (``out`` aliasing ``x0``)."""
    from diffusioniqt_amd import ops
    cell, profile, P = SL.PROJECT_CASES[case]
    tab, dev = table_of(cell, profile, P // cell[0])
    x0, meas = SL.project_inputs(cell, P)
    c = CLAMPS[clamp]
    a = DC.clamp32(*(c or (0., 0., None)))(x0)
    want = cached(('project', case, clamp, w), lambda: SL.project32(a, meas, tab, w))
    x = cu(x0)
    got = ops.slab_project(x, cu(meas), cell, dev, w, clamp=c)
    assert got.data_ptr() != x.data_ptr() and torch.equal(x, cu(x0))
    bad = (bits(got) != bits(want)).sum()
    print(f"slab_project {cell} r {tab['r']} P {P} clamp {clamp} w {w}: {bad} of {want.size} voxels differ")
    assert bad == 0
    same = ops.slab_project(x, cu(meas), cell, dev, w, clamp=c, out=x)
    assert same.data_ptr() == x.data_ptr() and torch.equal(x, got)
    outer = cell[0] - tab['r']                                # the planes under the first and the last slice alone: never moved
    assert np.array_equal(bits(got)[:, :, :outer], bits(a)[:, :, :outer]) and np.array_equal(bits(got)[:, :, P - outer:], bits(a)[:, :, P - outer:])
    assert (bits(got)[:, :, outer:P - outer] != bits(a)[:, :, outer:P - outer]).mean() > 0.9
    if w == 1.0 and c is None:                                # what it is for: A_act x0' = y_act
        scale = max(float(np.abs(x0).max()), float(np.abs(meas).max()), float(np.abs(want).max()))
        for b in range(3):
            y = meas[b, 0][::cell[0], ::cell[1], ::cell[2]]
            err = np.abs(SL.measure64(got[b, 0].cpu().numpy(), tab) - y)[1:-1].max()
            assert err <= SL.slab_roundings(tab, scale)


def test_slab_ops_argument_errors():
    from diffusioniqt_amd import ops
    x = torch.zeros(2, 1, 8, 8, 8, device=DEV)
    profile = ([0.25, 1.0, 1.0, 0.25], [1.0, 0.5], [0.75, 1.0])
    _, table = table_of((2, 2, 2), profile, 4)
    with pytest.raises(ValueError, match="consistency cell"):
        ops.slab_project(x, x.clone(), (3, 1, 1), table)
    with pytest.raises(ValueError, match="consistency weight"):
        ops.slab_project(x, x.clone(), (2, 2, 2), table, 0.0)
    with pytest.raises(ValueError, match="consistency_slab table"):
        ops.slab_project(x, x.clone(), (2, 2, 1), table)                                   # made for another cell
    with pytest.raises(ValueError, match="consistency_slab table"):
        ops.slab_project(x, x.clone(), (2, 2, 2), table.table)                             # the bare tensor
    with pytest.raises(ValueError, match="consistency_slab table"):
        ops.slab_project(x, x.clone(), (2, 2, 2), ops.slab_profile((2, 2, 2), profile, jmax=4))     # on the host
    with pytest.raises(ValueError, match="run positions"):
        ops.slab_project(x, x.clone(), (2, 2, 2), ops.slab_profile((2, 2, 2), profile, jmax=3).to(DEV))
    with pytest.raises(ValueError, match="clamp mode"):
        ops.slab_project(x, x.clone(), (2, 2, 2), table, clamp=(-1., 1., 2))
    with pytest.raises(ValueError, match="meas_up"):
        ops.slab_project(x, x[:1].clone(), (2, 2, 2), table)
    with pytest.raises(ValueError, match="consistency_slab table"):
        ops.slab_measure(x[0, 0], (2, 2, 2), table.table)
    with pytest.raises(ValueError, match="consistency cell"):
        ops.slab_measure(torch.zeros(9, 8, 8, device=DEV), (2, 2, 2), table)
    with pytest.raises(RuntimeError):
        ops.slab_measure(x[0, 0].cpu(), (2, 2, 2), table)


# ---- G2: the three launches of the joint step, bit for bit ---------------------------------------------------------------------------------
# D = 20: S = 5 for fz = 4 and S = 10 for fz = 2; W = 70 crosses the 64-lane block; H = 18 is no multiple of 4
STEP_PROFILES = {(4, 1, 1): SL.PROJECT_CASES[2][1], (2, 1, 1): SL.PROJECT_CASES[0][1], (2, 3, 1): SL.PROJECT_CASES[4][1],
                 (4, 2, 2): ([0.3, 1.0, 1.0, 1.0, 1.0, 0.3], [1.0, 0.5], [0.75, 1.0])}


def _step_refs(stride, kind):
    """The case and the fused x0 per clamp (the walk does not depend on the cell)."""
    def make():
        c = DC.step_case(stride, kind)
        c['fused'] = {name: DC.fuse32(c['y'], c['slot'], c['taps'], stride, DC.STEP_VOL, DC.clamp32(*cl))
                      for name, cl in (('min', CLAMPS['min']), ('box', CLAMPS['box']))}
        return c
    return cached(('step', stride, kind), make)


def _normals(draw):
    from diffusioniqt_amd import ops
    return cached(('n', draw), lambda: ops.volume_joint_init(DC.STEP_VOL, SEED, sample=SAMPLE, draw=draw).cpu().numpy())


FORMS = {'step-kn0': (0, False, 0.0), 'step-kn': (0, False, 0.625), 'multistep-noprev': (1, False, 0.0), 'multistep-prev': (1, True, 0.0),
         'sde-prev-kn': (2, True, 0.625)}


@pytest.mark.parametrize('form', list(FORMS))
@pytest.mark.parametrize('cell', list(STEP_PROFILES))
@pytest.mark.parametrize('tiling', DC.STEP_TILINGS, ids=['s4-gaussian', 's5-constant'])
def test_joint_slab_step_is_the_reference_bit_for_bit(tiling, cell, form):
    """Every voxel is compared: nothing is excluded.  The coefficients, then the fresh step launch, then the same launch in place
    (``x_next`` aliasing ``x_t`` and, where there is a history, ``x0_out`` aliasing ``x0_prev``).  The volume has dropped windows, so
    runs restart inside columns; a covered voxel under no active row reports the fused x0 itself."""
    from diffusioniqt_amd import ops
    stride, kind = tiling
    c = _step_refs(stride, kind)
    f, with_prev, kn = FORMS[form]
    clamp = 'min' if cell[2] != 1 else 'box'
    w, draw = (1.0, 5) if sum(cell) % 2 else (0.5, 3)
    tab, dev = table_of(cell, STEP_PROFILES[cell], DC.STEP_VOL[0] // cell[0])
    meas = DC.step_meas(c, cell)
    n = _normals(draw) if kn != 0 else None
    fused, covered = c['fused'][clamp]
    coef, act = cached(('coef', tiling, cell, clamp), lambda: SL.coeffs32(fused, meas, tab, covered))
    want, want0, _ = SL.joint_step32(c['y'], c['slot'], c['taps'], stride, c['x'], c['prev'] if with_prev else None, meas, tab, w, f, KX,
                                     K0, KP, kn, None, n, fused=c['fused'][clamp])
    patterns = {tuple(act[:, cy, cx]) for cy in range(act.shape[1]) for cx in range(act.shape[2])}
    assert len(patterns) > 1 and act.any() and (~covered).any() and (covered[:16, :16, :64] == False).any()
    args = (cu(c['y']), cu(c['slot'].astype(np.int32)), cu(c['taps']))
    workspace, cf = ops.slab_workspace(DC.STEP_VOL, cell, DEV)
    cl = CLAMPS[clamp]
    assert ops.volume_joint_slab_coeffs(*args, cu(meas), cell, dev, workspace, cf, *cl, stride) is cf
    assert tuple(cf.shape) == coef.shape and np.array_equal(bits(cf), bits(coef))
    tail = (cell, dev, workspace, cf, w, f, KX, K0, KP, kn, *cl, stride, SEED, draw, SAMPLE)
    x, prev = cu(c['x']), cu(c['prev']) if with_prev else None
    got, got0 = ops.volume_joint_consistent_slab_step(*args, x, prev, *tail)
    assert got.data_ptr() != x.data_ptr() and torch.equal(x, cu(c['x']))
    bad, bad0 = (bits(got) != bits(want)).sum(), (bits(got0) != bits(want0)).sum()
    print(f"slab step {form} stride {stride} {kind} cell {cell} w {w}: {bad} / {bad0} of {want.size} voxels differ; active rows "
          f"{act.mean():.3f}, {len(patterns)} activity patterns")
    assert bad == 0 and bad0 == 0
    assert np.array_equal(bits(got)[~covered], bits(c['x'])[~covered]) and not got0.cpu().numpy()[~covered].any()
    touched = np.zeros(DC.STEP_VOL, dtype=bool)                # under at least one active row
    up = lambda v: np.repeat(np.repeat(v, cell[1], axis=-2), cell[2], axis=-1)
    for s in range(act.shape[0]):
        touched[s * cell[0] - tab['r']:s * cell[0] + cell[0] + tab['r']] |= up(act[s])[None]
    plain = covered & ~touched
    assert plain.any() and np.array_equal(bits(got0)[plain], bits(fused)[plain])              # the plain update: x0 as fused
    ops.volume_joint_consistent_slab_step(*args, x, prev, *tail, out=x, x0_out=prev)
    assert torch.equal(x, got) and (prev is None or torch.equal(prev, got0))


def test_joint_slab_argument_errors():
    from diffusioniqt_amd import ops
    c = _step_refs(4, 'gaussian')
    y, slot, taps, x = cu(c['y']), cu(c['slot'].astype(np.int32)), cu(c['taps']), cu(c['x'])
    cell = (2, 1, 1)
    _, table = table_of(cell, STEP_PROFILES[cell], 10)
    ws, cf = ops.slab_workspace(DC.STEP_VOL, cell, DEV)
    ok = (0, KX, K0, 0.0, 0.0, -1.0, 1.0, 1, 4)
    with pytest.raises(ValueError, match="consistency cell"):
        ops.volume_joint_consistent_slab_step(y, slot, taps, x, None, (3, 1, 1), table, ws, cf, 1.0, *ok)            # 20 % 3
    with pytest.raises(ValueError, match="consistency weight"):
        ops.volume_joint_consistent_slab_step(y, slot, taps, x, None, cell, table, ws, cf, 0.0, *ok)
    with pytest.raises(ValueError, match="consistency_slab table"):
        ops.volume_joint_consistent_slab_step(y, slot, taps, x, None, (4, 1, 1), table, ws, cf, 1.0, *ok)
    with pytest.raises(ValueError, match="run positions"):
        ops.volume_joint_consistent_slab_step(y, slot, taps, x, None, cell, ops.slab_profile(cell, STEP_PROFILES[cell], jmax=9).to(DEV),
                                              ws, cf, 1.0, *ok)
    with pytest.raises(ValueError, match="workspace"):
        ops.volume_joint_consistent_slab_step(y, slot, taps, x, None, cell, table, ws[:-1], cf, 1.0, *ok)
    with pytest.raises(ValueError, match="workspace"):
        ops.volume_joint_slab_coeffs(y, slot, taps, x.clone(), cell, table, ws, cf[:-1], -1.0, 1.0, 1, 4)
    with pytest.raises(ValueError, match="form"):
        ops.volume_joint_consistent_slab_step(y, slot, taps, x, None, cell, table, ws, cf, 1.0, 3, *ok[1:])
    with pytest.raises(ValueError, match="lattice"):
        ops.volume_joint_slab_coeffs(y, slot, taps, x[:10].clone(), cell, table, ws, cf, -1.0, 1.0, 1, 4)


# ---- G3: the chains through VolumeInference against the float64 reference ----------------------------------------------------------------------
CHAIN_VOL, CHAIN_P, CHAIN_STRIDE = (16, 16, 24), 8, 4
CHAIN_PROFILES = {(2, 2, 2): ([0.25, 1.0, 1.0, 0.25], [1.0, 0.5], [0.75, 1.0]), (4, 1, 1): SL.PROJECT_CASES[2][1]}


def chain_volume():
    vol = np.random.default_rng(7).integers(1, 1000, CHAIN_VOL).astype(np.float32)
    vol[:8, :8, :12] = 0                                       # the 5 % rule drops two windows: 4 x 4 x 8 voxels are covered by none
    return vol


def chain_cfg(stride=CHAIN_STRIDE, batch_size=7):
    return R.shared_cfg(stride, batch_size=batch_size, P=CHAIN_P)


VP = {'ddim-eta0': ('ddim', 0.0), 'ddim-eta0.5': ('ddim', 0.5), 'ddpm': ('ddpm', 0.0), 'dpmpp2m': ('dpmpp2m', 0.0)}


def vp_denoiser(imagen, sampler, eta):
    return imagen.window_denoiser(sampler=sampler, sample_steps=J.STEPS, eta=eta)


def vp_reference(imagen, name, cell, profile, w, vol, cfg, blend):
    sampler, eta = VP[name]
    sched = imagen.noise_schedulers[1]
    coefs = vp_denoiser(imagen, sampler, eta).coefs.numpy().astype(np.float64)             # the chain's host numbers, widened
    log_snr = J.tables(sched, J.STEPS, 0.0, 'x_start')[2]
    tab = SL.table(cell, profile, vol.shape[0] // cell[0])
    meas = DC.measurement(vol, cell)
    meas_up = DC.measurement_state(meas, cell, cfg)
    with SL.slab_chains(tab):
        x, L, x0_max, touched = DC.vp_chain(vol, cfg, coefs, log_snr, (J.MIN_BOUND, 0., 0), blend, meas_up, cell, w,
                                            multistep=sampler == 'dpmpp2m', seed=J.SEED, sample=0)
    ref = DC.finish(vol, cfg, [np.maximum(x, J.MIN_BOUND)], L)
    if sampler == 'dpmpp2m':
        t64, k01 = M.table64(*M.chain_log_snr(sched, J.STEPS))
        bound = M.chain_bound(ref['windows_per_voxel'], ref['scale'], M.amplification(t64, k01))
    else:
        bound = J.chain_bound(ref['windows_per_voxel'], ref['scale'])
    ref.update(bound=bound + J.STEPS * SL.slab_roundings(tab, max(x0_max, float(np.abs(meas_up).max()))), meas=meas, touched=touched)
    return ref


def check(got, ref, what, key='mean', factor=1):
    got = got.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == ref[key].shape and np.isfinite(got).all()
    err = np.abs(got.astype(np.float64) - ref[key]).max()
    print(f"{what}: max |{key} - ref| = {err:.3e}, bound {factor * ref['bound']:.3e}")
    assert err <= factor * ref['bound'], what
    return got


@pytest.mark.parametrize('cell', list(CHAIN_PROFILES))
@pytest.mark.parametrize('name', list(VP))
def test_slab_joint_chain_matches_the_float64_reference(name, cell):
    from diffusioniqt_amd.inference import VolumeInference
    imagen = stub_imagen('x_start', 'clamp-min', size=CHAIN_P)
    vol, cfg, w = chain_volume(), chain_cfg(), 1.0 if cell == (2, 2, 2) else 0.5
    ref = cached(('vp', name, cell), lambda: vp_reference(imagen, name, cell, CHAIN_PROFILES[cell], w, vol, cfg, 'gaussian'))
    common = dict(blend='gaussian', noise='anchored', joint=True, seed=J.SEED, consistency=(torch.from_numpy(ref['meas']), cell),
                  consistency_weight=w)
    inf = VolumeInference(cfg, vp_denoiser(imagen, *VP[name]), consistency_slab=CHAIN_PROFILES[cell], **common)
    got = check(inf(cu(vol)), ref, f"slab joint {name} cell {cell} w {w}")
    uniform = cached(('vp-none', name, cell), lambda: VolumeInference(cfg, vp_denoiser(imagen, *VP[name]), **common)(cu(vol)).cpu().numpy())
    live = ref['covered'] & ~ref['background'] & ref['touched']
    assert (~ref['covered']).any() and ref['touched'].any() and np.abs(got - uniform)[live].max() > 0.01     # not the cell-mean chain


@pytest.mark.parametrize('cell', list(CHAIN_PROFILES))
@pytest.mark.parametrize('eta', list(E.ETAS))
def test_slab_edm_joint_chain_matches_the_float64_reference(eta, cell):
    from diffusioniqt_amd.inference import VolumeInference
    eta = E.ETAS[eta]
    elu = HN.make_elucidated('churn-on', False, size=CHAIN_P).to(DEV)
    den = elu.window_denoiser(sampler='dpmpp2m', eta=eta)
    vol, cfg = chain_volume(), chain_cfg()
    meas = DC.measurement(vol, cell)
    tab = SL.table(cell, CHAIN_PROFILES[cell], vol.shape[0] // cell[0])

    def make():
        tabs = E.tables(HN.HP, eta, coefs=den.coefs.numpy())
        meas_up = DC.measurement_state(meas, cell, cfg)
        with SL.slab_chains(tab):
            x, L, state_max, x0_max, _ = DC.edm_chain(vol, cfg, tabs, 'gaussian', False, meas_up, cell, 1.0)
        ref = DC.finish(vol, cfg, [np.clip(x, -1.0, 1.0)], L)
        mean32, std32 = np.float32(cfg['Data']['mean']), np.float32(cfg['Data']['std'])
        lowres_max = tabs['lowres'][0] * float(np.abs((vol - mean32) / std32).max()) + 6 * tabs['lowres'][1]
        # the family's bound is a recursion with a local term of (windows + 3) 2^-23 per step at |D| <= 1: the allowance of one
        # projection enters as that many further such terms, as ``volume_joint_dc_reference.edm_bound`` has it for the cell mean
        extra = math.ceil(SL.slab_roundings(tab, max(x0_max, float(np.abs(meas_up).max()))) / 2.0 ** -23)
        ref['bound'] = E.chain_bound(tabs, L['windows_per_voxel'] + extra, state_max, lowres_max, False, False)
        return ref
    ref = cached(('edm', eta, cell), make)
    inf = VolumeInference(cfg, den, blend='gaussian', noise='anchored', joint=True, seed=E.SEED, consistency=(torch.from_numpy(meas), cell),
                          consistency_slab=CHAIN_PROFILES[cell])
    check(inf(cu(vol)), ref, f"slab joint EDM dpmpp2m eta {eta} cell {cell}")


# ---- G4: a volume of one window: the joint chain is the per-window sampler ----------------------------------------------------------------------
# P = 8: fz = 2 gives S = 4 slices, two of them active
TIE_PROFILES = {(2, 2, 2): CHAIN_PROFILES[(2, 2, 2)], (2, 1, 1): SL.PROJECT_CASES[0][1]}


def one_window_volume():
    return np.random.default_rng(9).integers(1, 1000, (CHAIN_P,) * 3).astype(np.float32)


@pytest.mark.parametrize('cell', list(TIE_PROFILES))
@pytest.mark.parametrize('name', ['ddim-eta0.5', 'ddpm', 'dpmpp2m'])
def test_slab_joint_on_one_window_is_the_independent_path(name, cell):
    """D = H = W = P, unit weights: num / den is exact and the domain of the joint path is the sampler's cube, so the same rows are
    active and both paths take the same ``__device__`` arithmetic and update -- equal at every voxel, bit for bit."""
    from diffusioniqt_amd.inference import VolumeInference
    sampler, eta = VP[name]
    for mode in ('clamp-min', 'dynamic'):
        imagen = stub_imagen('x_start', mode, size=CHAIN_P)
        vol, cfg = cu(one_window_volume()), chain_cfg(stride=CHAIN_P)
        cons = dict(consistency=(torch.from_numpy(DC.measurement(one_window_volume(), cell)), cell), consistency_weight=0.75,
                    consistency_slab=TIE_PROFILES[cell])

        def sample_fn(x, noise=None, **kw):
            assert set(kw) == {'consistency', 'consistency_weight', 'consistency_slab'}
            return imagen.sample(batch_size=x.shape[0], start_image_or_video=x, start_at_unet_number=2, use_tqdm=False, sampler=sampler,
                                 sample_steps=J.STEPS, eta=eta, noise=noise, **kw)[0]
        independent = VolumeInference(cfg, sample_fn, blend='constant', noise='anchored', seed=J.SEED, **cons)(vol)
        joint = VolumeInference(cfg, vp_denoiser(imagen, sampler, eta), blend='constant', noise='anchored', joint=True, seed=J.SEED,
                                **cons)(vol)
        plain = VolumeInference(cfg, vp_denoiser(imagen, sampler, eta), blend='constant', noise='anchored', joint=True, seed=J.SEED,
                                consistency=cons['consistency'], consistency_weight=0.75)(vol)
        assert independent.unique().numel() > 100 and not torch.equal(joint, plain)
        assert torch.equal(joint, independent), mode


@pytest.mark.parametrize('cell', list(TIE_PROFILES))
@pytest.mark.parametrize('eta', list(E.ETAS))
def test_slab_edm_joint_on_one_window_is_the_independent_path(eta, cell):
    from diffusioniqt_amd.inference import VolumeInference
    eta = E.ETAS[eta]
    for dynamic in (False, True):
        elu = HN.make_elucidated('churn-on', dynamic, self_cond=True, size=CHAIN_P).to(DEV)
        vol, cfg = cu(one_window_volume()), chain_cfg(stride=CHAIN_P)
        cons = dict(consistency=(torch.from_numpy(DC.measurement(one_window_volume(), cell)), cell), consistency_weight=0.75,
                    consistency_slab=TIE_PROFILES[cell])

        def sample_fn(x, noise=None, **kw):
            assert set(kw) == {'consistency', 'consistency_weight', 'consistency_slab'}
            return elu.sample(batch_size=x.shape[0], video_frames=CHAIN_P, start_image_or_video=x, start_at_unet_number=2, noise=noise,
                              sampler='dpmpp2m', eta=eta, use_tqdm=False, **kw)
        independent = VolumeInference(cfg, sample_fn, blend='constant', noise='anchored', seed=E.SEED, **cons)(vol)
        joint = VolumeInference(cfg, elu.window_denoiser(sampler='dpmpp2m', eta=eta), blend='constant', noise='anchored', joint=True,
                                seed=E.SEED, **cons)(vol)
        assert independent.unique().numel() > 100
        assert torch.equal(joint, independent), dynamic
