"""Data-consistent sampling with a slice profile on a real MI355X against tests/volume_joint_profile_reference.py:
``ops.cell_measure`` / ``ops.cell_project_profile`` and the fused joint step bit for bit against the fp32 restatement (no voxel is left
out of a comparison), the joint chains of both families through ``VolumeInference(consistency_profile=...)`` against the float64
chains, the bit-for-bit tie of the joint chain at stride = patch to ``sample(consistency=..., consistency_profile=...)`` per window,
the guarantee (weighted cell means of the last corrected prediction = the measurement, gap voxels never moved) and a uniform profile
through the profile path.  The shapes are those of tests/test_gpu_volume_dc.py.

Bounds: that module's docstring.  The chain tests take the family's ``chain_bound`` plus ``steps`` times the projection's own
roundings, ((n + 4) G + 1) 2^-24 of the largest magnitude involved, G = max(1, w max g); the guarantee tests take that number once."""

import numpy as np
import pytest
import torch

from tests import dpmpp2m_reference as M
from tests import edm_dpmpp2m_reference as E
from tests import volume_blend_reference as R
from tests import volume_joint_dc_reference as DC
from tests import volume_joint_heun_reference as HN
from tests import volume_joint_profile_reference as PR
from tests import volume_joint_reference as J
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


def table_of(cell, profile):
    """(the reference's table, the op's table on the device); they are the same bits (tests/test_volume_profile_host.py)."""
    from diffusioniqt_amd import ops
    host = ops.cell_profile(cell, profile)
    want = PR.profile_table(cell, profile)
    assert np.array_equal(bits(host), bits(want))
    return want, host.to(DEV)


# ---- G1: the operator and the per-window projection, bit for bit --------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(PR.PROFILES))
def test_cell_measure_is_the_reference_bit_for_bit(name):
    from diffusioniqt_amd import ops
    cell, profile = PR.PROFILES[name]
    table, dev = table_of(cell, profile)
    x = (np.random.default_rng(4).standard_normal((24, 8, 8)) * 3).astype(np.float32)        # the 3 cubes of edge 8, stacked along z
    got = ops.cell_measure(cu(x), cell, dev)
    want = PR.cell_wmean32(x, cell, table)
    assert tuple(got.shape) == want.shape and np.array_equal(bits(got), bits(want))


@pytest.mark.parametrize('w', [1.0, 0.5])
@pytest.mark.parametrize('clamp', list(CLAMPS))
@pytest.mark.parametrize('name', list(PR.PROFILES))
def test_cell_project_profile_is_the_reference_bit_for_bit(name, clamp, w):
    """B C = 3 cubes of edge 8; fresh output and in place (``out`` aliasing ``x0``)."""
    from diffusioniqt_amd import ops
    cell, profile = PR.PROFILES[name]
    table, dev = table_of(cell, profile)
    rng = np.random.default_rng(5)
    x0 = (rng.standard_normal((3, 1, 8, 8, 8)) * 2).astype(np.float32)
    meas = PR.replicate(rng.standard_normal((3, 1) + tuple(8 // f for f in cell)).astype(np.float32), cell)
    c = CLAMPS[clamp]
    a = PR.clamp32(*(c or (0., 0., None)))(x0)
    want = PR.project_profile32(a, meas, cell, table, w)
    x = cu(x0)
    got = ops.cell_project_profile(x, cu(meas), cell, dev, w, clamp=c)
    assert got.data_ptr() != x.data_ptr() and torch.equal(x, cu(x0))
    assert np.array_equal(bits(got), bits(want))
    same = ops.cell_project_profile(x, cu(meas), cell, dev, w, clamp=c, out=x)
    assert same.data_ptr() == x.data_ptr() and torch.equal(x, got)
    gap = np.broadcast_to(PR.gains(table, cell, x0.shape) == 0, x0.shape)
    assert np.array_equal(bits(got)[gap], bits(a)[gap]) and gap.any() == (name == 'gap')     # a gap voxel is never moved
    if w == 1.0 and c is None:                                # what it is for: u . x0' = y
        y = meas[..., ::cell[0], ::cell[1], ::cell[2]]
        err = np.abs(PR.cell_wmean64(got.cpu().numpy(), cell, table) - y).max()
        scale = max(float(np.abs(x0).max()), float(np.abs(meas).max()), float(np.abs(want).max()))
        assert err <= PR.profile_roundings(cell, table, w, scale)


def test_profile_ops_argument_errors():
    from diffusioniqt_amd import ops
    x = torch.zeros(2, 1, 8, 8, 8, device=DEV)
    _, table = table_of((2, 2, 2), ((1, 2), (1, 1), (3, 1)))
    with pytest.raises(ValueError, match="consistency cell"):
        ops.cell_project_profile(x, x.clone(), (3, 1, 1), table)
    with pytest.raises(ValueError, match="consistency weight"):
        ops.cell_project_profile(x, x.clone(), (2, 2, 2), table, 0.0)
    with pytest.raises(ValueError, match="consistency profile table"):
        ops.cell_project_profile(x, x.clone(), (4, 1, 1), table)                            # [2, 8] is not [2, 4]
    with pytest.raises(ValueError, match="consistency profile table"):
        ops.cell_project_profile(x, x.clone(), (2, 2, 2), table.cpu())
    with pytest.raises(ValueError, match="consistency profile table"):
        ops.cell_measure(x[0, 0], (2, 2, 2), table.double())
    with pytest.raises(ValueError, match="clamp mode"):
        ops.cell_project_profile(x, x.clone(), (2, 2, 2), table, clamp=(-1., 1., 2))


# ---- G2: the fused joint step, bit for bit -------------------------------------------------------------------------------------------------
# one non-uniform profile per cell of the uniform step tests; (1, 1, 5) has zero weights at both ends
STEP_PROFILES = {(4, 1, 1): ((1, 3, 3, 1), (1,), (1,)), (1, 3, 1): ((1,), (1, 2, 1), (1,)), (1, 1, 5): ((1,), (1,), (0, 1, 2, 1, 0)),
                 (2, 2, 2): ((1, 2), (1, 1), (3, 1)), (1, 1, 7): ((1,), (1,), (1, 2, 4, 6, 4, 2, 1))}
assert tuple(STEP_PROFILES) == DC.STEP_CELLS


def _step_refs(stride, kind):
    """The case, its device tensors' sources and the fused x0 per clamp (the walk does not depend on the cell)."""
    def make():
        c = DC.step_case(stride, kind)
        c['fused'] = {name: PR.fuse32(c['y'], c['slot'], c['taps'], stride, DC.STEP_VOL, PR.clamp32(*cl))
                      for name, cl in (('min', CLAMPS['min']), ('box', CLAMPS['box']))}
        return c
    return cached(('step', stride, kind), make)


def _normals(draw):
    from diffusioniqt_amd import ops
    return cached(('n', draw), lambda: ops.volume_joint_init(DC.STEP_VOL, SEED, sample=SAMPLE, draw=draw).cpu().numpy())


FORMS = {'step-kn0': (0, False, 0.0), 'step-kn': (0, False, 0.625), 'multistep-noprev': (1, False, 0.0), 'multistep-prev': (1, True, 0.0),
         'sde-prev-kn': (2, True, 0.625)}


@pytest.mark.parametrize('form', list(FORMS))
@pytest.mark.parametrize('cell', DC.STEP_CELLS)
@pytest.mark.parametrize('tiling', DC.STEP_TILINGS, ids=['s4-gaussian', 's5-constant'])
def test_joint_profile_step_is_the_reference_bit_for_bit(tiling, cell, form):
    """Every voxel is compared: nothing is excluded.  The fresh launch, then the same launch in place (``x_next`` aliasing ``x_t`` and,
    where there is a history, ``x0_out`` aliasing ``x0_prev``).  A cell with an uncovered voxel keeps the plain update: its covered
    voxels report the fused x0 itself."""
    from diffusioniqt_amd import ops
    stride, kind = tiling
    c = _step_refs(stride, kind)
    f, with_prev, kn = FORMS[form]
    clamp = 'min' if cell[2] != 1 else 'box'
    w, draw = (1.0, 5) if sum(cell) % 2 else (0.5, 3)
    table, dev = table_of(cell, STEP_PROFILES[cell])
    meas = DC.step_meas(c, cell)
    n = _normals(draw) if kn != 0 else None
    want, want0, covered = PR.joint_step_profile32(c['y'], c['slot'], c['taps'], stride, c['x'], c['prev'] if with_prev else None, meas,
                                                   cell, table, w, f, KX, K0, KP, kn, None, n, fused=c['fused'][clamp])
    whole = PR.replicate(PR._cells(covered, cell).all(axis=(-5, -3, -1)), cell)
    assert whole.any() and (~covered).any() and (covered[:16, :16, :64] == False).any()         # uncovered voxels inside the volume too
    args = (cu(c['y']), cu(c['slot'].astype(np.int32)), cu(c['taps']))
    tail = (cu(meas), cell, dev, w, f, KX, K0, KP, kn, *CLAMPS[clamp], stride, SEED, draw, SAMPLE)
    x, prev = cu(c['x']), cu(c['prev']) if with_prev else None
    got, got0 = ops.volume_joint_consistent_profile_step(*args, x, prev, *tail)
    assert got.data_ptr() != x.data_ptr() and torch.equal(x, cu(c['x']))
    bad, bad0 = (bits(got) != bits(want)).sum(), (bits(got0) != bits(want0)).sum()
    print(f"profile step {form} stride {stride} {kind} cell {cell} w {w}: {bad} / {bad0} of {want.size} voxels differ; corrected "
          f"share {whole.mean():.3f}, covered voxels of partly covered cells {(covered & ~whole).sum()}")
    assert bad == 0 and bad0 == 0
    assert np.array_equal(bits(got)[~covered], bits(c['x'])[~covered]) and not got0.cpu().numpy()[~covered].any()
    partly = covered & ~whole
    assert np.array_equal(bits(got0)[partly], bits(c['fused'][clamp][0])[partly])             # the plain update: x0 as fused
    ops.volume_joint_consistent_profile_step(*args, x, prev, *tail, out=x, x0_out=prev)
    assert torch.equal(x, got) and (prev is None or torch.equal(prev, got0))


def test_joint_profile_step_argument_errors():
    from diffusioniqt_amd import ops
    c = _step_refs(4, 'gaussian')
    y, slot, taps, x = cu(c['y']), cu(c['slot'].astype(np.int32)), cu(c['taps']), cu(c['x'])
    _, table = table_of((2, 2, 2), STEP_PROFILES[(2, 2, 2)])
    ok = (0, KX, K0, 0.0, 0.0, -1.0, 1.0, 1, 4)
    with pytest.raises(ValueError, match="consistency cell"):
        ops.volume_joint_consistent_profile_step(y, slot, taps, x, None, x.clone(), (3, 1, 1), table, 1.0, *ok)      # 20 % 3
    with pytest.raises(ValueError, match="consistency weight"):
        ops.volume_joint_consistent_profile_step(y, slot, taps, x, None, x.clone(), (2, 2, 2), table, 0.0, *ok)
    with pytest.raises(ValueError, match="meas_up"):
        ops.volume_joint_consistent_profile_step(y, slot, taps, x, None, x[:10].clone(), (2, 2, 2), table, 1.0, *ok)
    with pytest.raises(ValueError, match="consistency profile table"):
        ops.volume_joint_consistent_profile_step(y, slot, taps, x, None, x.clone(), (4, 1, 1), table, 1.0, *ok)
    with pytest.raises(ValueError, match="form"):
        ops.volume_joint_consistent_profile_step(y, slot, taps, x, None, x.clone(), (2, 2, 2), table, 1.0, 3, *ok[1:])


# ---- G3: the chains through VolumeInference against the float64 reference ----------------------------------------------------------------------
CHAIN_VOL, CHAIN_P, CHAIN_STRIDE = (16, 16, 24), 8, 4
CHAIN_PROFILES = {(2, 2, 2): ((1, 2), (1, 1), (3, 1)), (4, 1, 1): ((1, 3, 3, 1), (1,), (1,))}


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
    table = PR.profile_table(cell, profile)
    meas = DC.measurement(vol, cell)
    meas_up = DC.measurement_state(meas, cell, cfg)
    x, L, x0_max, whole = PR.vp_chain(vol, cfg, coefs, log_snr, (J.MIN_BOUND, 0., 0), blend, meas_up, cell, table, w,
                                      multistep=sampler == 'dpmpp2m', seed=J.SEED, sample=0)
    ref = DC.finish(vol, cfg, [np.maximum(x, J.MIN_BOUND)], L)
    if sampler == 'dpmpp2m':
        tab, k01 = M.table64(*M.chain_log_snr(sched, J.STEPS))
        bound = M.chain_bound(ref['windows_per_voxel'], ref['scale'], M.amplification(tab, k01))
    else:
        bound = J.chain_bound(ref['windows_per_voxel'], ref['scale'])
    ref.update(bound=bound + J.STEPS * PR.profile_roundings(cell, table, w, max(x0_max, float(np.abs(meas_up).max()))), meas=meas,
               whole=whole, state=x)
    return ref


def check(got, ref, what, key='mean', factor=1):
    got = got.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == ref[key].shape and np.isfinite(got).all()
    err = np.abs(got.astype(np.float64) - ref[key]).max()
    print(f"{what}: max |{key} - ref| = {err:.3e}, bound {factor * ref['bound']:.3e}")
    assert err <= factor * ref['bound'], what
    return got


def _uniform_run(name, cell, w, imagen, vol, cfg):
    from diffusioniqt_amd.inference import VolumeInference
    meas = DC.measurement(vol, cell)
    return cached(('vp-none', name, cell, w), lambda: VolumeInference(
        cfg, vp_denoiser(imagen, *VP[name]), blend='gaussian', noise='anchored', joint=True, seed=J.SEED,
        consistency=(torch.from_numpy(meas), cell), consistency_weight=w)(cu(vol)).cpu().numpy())


@pytest.mark.parametrize('cell', list(CHAIN_PROFILES))
@pytest.mark.parametrize('name', list(VP))
def test_profile_joint_chain_matches_the_float64_reference(name, cell):
    from diffusioniqt_amd.inference import VolumeInference
    imagen = stub_imagen('x_start', 'clamp-min', size=CHAIN_P)
    vol, cfg, w = chain_volume(), chain_cfg(), 1.0 if cell == (2, 2, 2) else 0.5
    ref = cached(('vp', name, cell), lambda: vp_reference(imagen, name, cell, CHAIN_PROFILES[cell], w, vol, cfg, 'gaussian'))
    inf = VolumeInference(cfg, vp_denoiser(imagen, *VP[name]), blend='gaussian', noise='anchored', joint=True, seed=J.SEED,
                          consistency=(torch.from_numpy(ref['meas']), cell), consistency_weight=w,
                          consistency_profile=CHAIN_PROFILES[cell])
    got = check(inf(cu(vol)), ref, f"profile joint {name} cell {cell} w {w}")
    live = ref['covered'] & ~ref['background']
    uniform = _uniform_run(name, cell, w, imagen, vol, cfg)
    assert (~ref['covered']).any() and np.abs(got - uniform)[live].max() > 0.01            # and it is not the uniform operator's chain


@pytest.mark.parametrize('cell', list(CHAIN_PROFILES))
@pytest.mark.parametrize('eta', list(E.ETAS))
def test_profile_edm_joint_chain_matches_the_float64_reference(eta, cell):
    from diffusioniqt_amd.inference import VolumeInference
    eta = E.ETAS[eta]
    elu = HN.make_elucidated('churn-on', False, size=CHAIN_P).to(DEV)
    den = elu.window_denoiser(sampler='dpmpp2m', eta=eta)
    vol, cfg = chain_volume(), chain_cfg()
    meas = DC.measurement(vol, cell)
    table = PR.profile_table(cell, CHAIN_PROFILES[cell])

    def make():
        tabs = E.tables(HN.HP, eta, coefs=den.coefs.numpy())
        x, L, state_max, x0_max, _ = PR.edm_chain(vol, cfg, tabs, 'gaussian', False, DC.measurement_state(meas, cell, cfg), cell, table, 1.0)
        ref = DC.finish(vol, cfg, [np.clip(x, -1.0, 1.0)], L)
        mean32, std32 = np.float32(cfg['Data']['mean']), np.float32(cfg['Data']['std'])
        lowres_max = tabs['lowres'][0] * float(np.abs((vol - mean32) / std32).max()) + 6 * tabs['lowres'][1]
        meas_max = float(np.abs(DC.measurement_state(meas, cell, cfg)).max())
        ref['bound'] = PR.edm_bound(tabs, L, cell, table, 1.0, state_max, lowres_max, False, max(x0_max, meas_max))
        return ref
    ref = cached(('edm', eta, cell), make)
    inf = VolumeInference(cfg, den, blend='gaussian', noise='anchored', joint=True, seed=E.SEED, consistency=(torch.from_numpy(meas), cell),
                          consistency_profile=CHAIN_PROFILES[cell])
    check(inf(cu(vol)), ref, f"profile joint EDM dpmpp2m eta {eta} cell {cell}")


# ---- G4: stride = patch: the joint chain is the per-window sampler ------------------------------------------------------------------------------
TIE_PROFILES = {(4, 1, 1): ((0, 1, 1, 0), (1,), (1,)), (2, 2, 2): ((1, 2), (1, 1), (3, 1)), (1, 1, 8): ((1,), (1,), PR.GAUSS8)}


@pytest.mark.parametrize('cell', list(TIE_PROFILES))
@pytest.mark.parametrize('name', ['ddim-eta0.5', 'ddpm', 'dpmpp2m'])
def test_profile_joint_at_stride_equal_patch_is_the_independent_path(name, cell):
    """No overlap, unit weights: num / den is exact and no cell straddles a window, so the fused projection is
    ``ops.cell_project_profile`` on every window and both paths take the same ``__device__`` projection and update -- equal at every
    voxel, bit for bit."""
    from diffusioniqt_amd.inference import VolumeInference
    sampler, eta = VP[name]
    for mode in ('clamp-min', 'dynamic'):
        imagen = stub_imagen('x_start', mode, size=CHAIN_P)
        vol, cfg = cu(chain_volume()), chain_cfg(stride=CHAIN_P)
        cons = dict(consistency=(torch.from_numpy(DC.measurement(chain_volume(), cell)), cell), consistency_weight=0.75,
                    consistency_profile=TIE_PROFILES[cell])

        def sample_fn(x, noise=None, **kw):
            assert set(kw) == {'consistency', 'consistency_weight', 'consistency_profile'}
            return imagen.sample(batch_size=x.shape[0], start_image_or_video=x, start_at_unet_number=2, use_tqdm=False, sampler=sampler,
                                 sample_steps=J.STEPS, eta=eta, noise=noise, **kw)[0]
        independent = VolumeInference(cfg, sample_fn, blend='constant', noise='anchored', seed=J.SEED, **cons)(vol)
        joint = VolumeInference(cfg, vp_denoiser(imagen, sampler, eta), blend='constant', noise='anchored', joint=True, seed=J.SEED,
                                **cons)(vol)
        assert independent.unique().numel() > 1000
        assert torch.equal(joint, independent), mode


@pytest.mark.parametrize('cell', list(TIE_PROFILES))
@pytest.mark.parametrize('eta', list(E.ETAS))
def test_profile_edm_joint_at_stride_equal_patch_is_the_independent_path(eta, cell):
    from diffusioniqt_amd.inference import VolumeInference
    eta = E.ETAS[eta]
    for dynamic in (False, True):
        elu = HN.make_elucidated('churn-on', dynamic, self_cond=True, size=CHAIN_P).to(DEV)
        vol, cfg = cu(chain_volume()), chain_cfg(stride=CHAIN_P)
        cons = dict(consistency=(torch.from_numpy(DC.measurement(chain_volume(), cell)), cell), consistency_weight=0.75,
                    consistency_profile=TIE_PROFILES[cell])

        def sample_fn(x, noise=None, **kw):
            assert set(kw) == {'consistency', 'consistency_weight', 'consistency_profile'}
            return elu.sample(batch_size=x.shape[0], video_frames=CHAIN_P, start_image_or_video=x, start_at_unet_number=2, noise=noise,
                              sampler='dpmpp2m', eta=eta, use_tqdm=False, **kw)
        independent = VolumeInference(cfg, sample_fn, blend='constant', noise='anchored', seed=E.SEED, **cons)(vol)
        joint = VolumeInference(cfg, elu.window_denoiser(sampler='dpmpp2m', eta=eta), blend='constant', noise='anchored', joint=True,
                                seed=E.SEED, **cons)(vol)
        assert independent.unique().numel() > 1000
        assert torch.equal(joint, independent), dynamic


# ---- G5: the guarantee -------------------------------------------------------------------------------------------------------------------------
# (1, 1, 3) straddles the windows (P 8, stride 4): only the joint state projects it; (4, 1, 1) has the slice gap
GUARANTEE = {(2, 2, 2): ((1, 2), (1, 1), (3, 1)), (4, 1, 1): ((0, 1, 1, 0), (1,), (1,)), (1, 1, 3): ((1,), (1,), (1, 2, 1))}


def _whole_cells(vol, cfg, cell):
    L = J.layout(vol, cfg)
    covered = R.blend_accumulate(np.zeros((1, L['kept'].shape[0], CHAIN_P, CHAIN_P, CHAIN_P)), L['slot'], np.ones(CHAIN_P), L['stride'],
                                 vol.shape)[2]
    whole = PR._cells(covered, cell).all(axis=(-5, -3, -1))
    assert 0 < whole.sum() < whole.size
    return whole


@pytest.mark.parametrize('cell', list(GUARANTEE))
def test_final_state_has_the_measurements_weighted_cell_means(cell):
    """The EDM family's DPM-Solver++ 2M ODE ends at sigma = 0 with (kx, k0) = (0, 1), no step clamp, w = 1: the state the chain ends
    in IS the projected x0, and its weighted cell means u . x, recomputed in float64, are the measurement's on every fully covered
    cell, within the projection's roundings of ONE step."""
    from diffusioniqt_amd.inference import VolumeInference
    elu = HN.make_elucidated('churn-on', False, size=CHAIN_P).to(DEV)
    den = elu.window_denoiser(sampler='dpmpp2m', eta=0.0)
    assert den.clamp == (-float('inf'), float('inf'), 1) and den.coefs[-1].tolist() == [0.0, 1.0, 0.0, 0.0]
    vol, cfg = chain_volume(), chain_cfg()
    meas = DC.measurement(vol, cell)
    table = PR.profile_table(cell, GUARANTEE[cell])
    states = []
    den.finish = lambda x: states.append(x.clone()) or x                                  # the state the chain ends in, before any finish
    VolumeInference(cfg, den, blend='gaussian', noise='anchored', joint=True, seed=E.SEED, consistency=(torch.from_numpy(meas), cell),
                    consistency_profile=GUARANTEE[cell])(cu(vol))
    x = states[0].cpu().numpy()
    whole = _whole_cells(vol, cfg, cell)
    want = DC.measurement_state(meas, cell, cfg)[::cell[0], ::cell[1], ::cell[2]]
    err = np.abs(PR.cell_wmean64(x, cell, table) - want)[whole].max()
    bound = PR.profile_roundings(cell, table, 1.0, max(1.0, float(np.abs(x).max()), float(np.abs(want).max())))   # 1: the clamped prediction
    print(f"guarantee EDM ODE cell {cell}: max |u . x - y| = {err:.3e} on {whole.sum()} of {whole.size} cells, bound {bound:.3e}")
    assert err <= bound
    i, j, k = (int(v[0]) for v in whole.nonzero())
    assert np.ptp(PR._cells(x, cell)[i, :, j, :, k, :]) > 0                                # the detail inside a cell is the network's


@pytest.mark.parametrize('cell', list(GUARANTEE))
def test_ddim_chain_ends_on_a_consistent_prediction(cell, monkeypatch):
    """The deterministic ddim chain with no clamp and w = 1: the last corrected prediction x0' (``x0_out`` of the last fused launch)
    has the measurement's weighted cell means on every fully covered cell, within the projection's roundings of one step."""
    from diffusioniqt_amd import ops
    from diffusioniqt_amd.inference import VolumeInference
    imagen = stub_imagen('x_start', 'dynamic', size=CHAIN_P)                              # dynamic: the step clamp is (-inf, inf)
    den = vp_denoiser(imagen, 'ddim', 0.0)
    assert den.clamp == (-float('inf'), float('inf'), 1)
    vol, cfg = chain_volume(), chain_cfg()
    meas = DC.measurement(vol, cell)
    table = PR.profile_table(cell, GUARANTEE[cell])
    real, calls = ops.volume_joint_consistent_profile_step, []

    def recording(*a, **kw):
        out, x0 = real(*a, **kw)
        calls.append(x0.clone())
        return out, x0
    monkeypatch.setattr(ops, 'volume_joint_consistent_profile_step', recording)
    VolumeInference(cfg, den, blend='gaussian', noise='anchored', joint=True, seed=J.SEED, consistency=(torch.from_numpy(meas), cell),
                    consistency_profile=GUARANTEE[cell])(cu(vol))
    assert len(calls) == J.STEPS
    x0 = calls[-1].cpu().numpy()
    whole = _whole_cells(vol, cfg, cell)
    want = DC.measurement_state(meas, cell, cfg)[::cell[0], ::cell[1], ::cell[2]]
    scale = max(1.0, float(np.abs(x0).max()), float(np.abs(want).max()))                  # 1: the thresholded prediction before the projection
    err0 = np.abs(PR.cell_wmean64(x0, cell, table) - want)[whole].max()
    bound0 = PR.profile_roundings(cell, table, 1.0, scale)
    print(f"ddim cell {cell}: max |u . x0' - y| = {err0:.3e} (bound {bound0:.3e})")
    assert err0 <= bound0


@pytest.mark.parametrize('tiling', DC.STEP_TILINGS, ids=['s4-gaussian', 's5-constant'])
def test_a_gap_voxel_is_never_moved(tiling):
    """One fused step with the slice gap (0, 1, 1, 0) along z: on every gap voxel the corrected prediction is the uncorrected fused x0
    of the plain launch, bit for bit -- also inside corrected cells, whose measured voxels do move."""
    from diffusioniqt_amd import ops
    stride, kind = tiling
    c = _step_refs(stride, kind)
    cell = (4, 1, 1)
    table, dev = table_of(cell, GUARANTEE[cell])
    args = (cu(c['y']), cu(c['slot'].astype(np.int32)), cu(c['taps']), cu(c['x']))
    _, plain0 = ops.volume_joint_multistep(*args, None, KX, K0, 0.0, *CLAMPS['box'], stride)
    _, got0 = ops.volume_joint_consistent_profile_step(*args, None, cu(DC.step_meas(c, cell)), cell, dev, 1.0, 1, KX, K0, 0.0, 0.0,
                                                       *CLAMPS['box'], stride)
    covered = c['fused']['box'][1]
    whole = PR.replicate(PR._cells(covered, cell).all(axis=(-5, -3, -1)), cell)
    gap = PR.gains(table, cell, DC.STEP_VOL) == 0
    assert np.array_equal(bits(plain0), bits(c['fused']['box'][0]))                          # the plain launch reports the fused x0
    assert (gap & whole).sum() > 1000 and np.array_equal(bits(got0)[gap], bits(plain0)[gap])
    moved = bits(got0) != bits(plain0)
    assert moved[whole & ~gap].mean() > 0.99 and not moved[~whole].any()


# ---- G6: a uniform profile through the profile path ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['ddim-eta0.5', 'dpmpp2m'])
def test_a_uniform_profile_is_the_uniform_chain_within_the_bound(name):
    """``consistency_profile`` = all ones takes the profile path: u = 1 / n and g = 1 exactly, the same operator in other roundings,
    so its float64 chain is the uniform operator's.  The result stays within the chain bound (with the profile's count) of that chain,
    and within the two chains' bounds of the ``consistency_profile=None`` result; whether the bits differ is not asserted."""
    from diffusioniqt_amd.inference import VolumeInference
    from tests.test_gpu_volume_dc import vp_reference as uniform_reference
    imagen = stub_imagen('x_start', 'clamp-min', size=CHAIN_P)
    vol, cfg, cell, w = chain_volume(), chain_cfg(), (2, 2, 2), 1.0
    ones = ((1, 1),) * 3
    ref = cached(('vp-ones', name), lambda: vp_reference(imagen, name, cell, ones, w, vol, cfg, 'gaussian'))
    old = cached(('vp-uniform', name), lambda: uniform_reference(imagen, name, cell, w, vol, cfg, 'gaussian'))
    assert np.abs(ref['mean'] - old['mean']).max() <= 1e-12                                  # one float64 chain
    inf = VolumeInference(cfg, vp_denoiser(imagen, *VP[name]), blend='gaussian', noise='anchored', joint=True, seed=J.SEED,
                          consistency=(torch.from_numpy(ref['meas']), cell), consistency_weight=w, consistency_profile=ones)
    got = check(inf(cu(vol)), ref, f"uniform profile through the profile path, {name}")
    none = _uniform_run(name, cell, w, imagen, vol, cfg)
    diff = np.abs(got.astype(np.float64) - none).max()
    print(f"uniform profile vs consistency_profile=None, {name}: max difference {diff:.3e}, bounds {ref['bound']:.3e} + {old['bound']:.3e}")
    assert diff <= ref['bound'] + old['bound']
