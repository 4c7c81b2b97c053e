"""Data-consistent sampling on a real MI355X against tests/volume_joint_dc_reference.py: ``ops.cell_mean`` / ``ops.cell_project`` and
the fused joint step bit for bit against the fp32 restatement (no voxel is left out of a comparison), the consistent joint chains of
both families through ``VolumeInference`` against the float64 chains, the bit-for-bit tie of the joint chain at stride = patch to
``sample(consistency=...)`` per window, the guarantee (cell means of the final state = the measurement), block mode and samples.

Bounds: that module's docstring.  The chain tests take the family's ``chain_bound`` plus ``steps`` times the projection's own
roundings, (n + 3) 2^-24 of the largest magnitude involved; the guarantee test takes that number once, for the last step."""

import numpy as np
import pytest
import torch

from tests import dpmpp2m_reference as M
from tests import edm_dpmpp2m_reference as E
from tests import volume_blend_reference as R
from tests import volume_joint_dc_reference as DC
from tests import volume_joint_heun_reference as HN
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


# ---- G1: the operator and the per-window projection, bit for bit --------------------------------------------------------------------------
@pytest.mark.parametrize('cell', [(4, 1, 1), (1, 1, 8), (2, 2, 2), (1, 3, 1), (1, 1, 5)])
def test_cell_mean_is_the_reference_bit_for_bit(cell):
    from diffusioniqt_amd import ops
    shape = (8, 12, 80)                                       # every cell divides it; more than one block of 256 cells
    x = (np.random.default_rng(4).standard_normal(shape) * 3).astype(np.float32)
    got = ops.cell_mean(cu(x), cell)
    want = DC.cell_mean32(x, cell)
    assert tuple(got.shape) == want.shape and np.array_equal(bits(got), bits(want))
    up = ops.cell_replicate(got, cell)                        # A+: every voxel its cell's value
    assert np.array_equal(bits(up), bits(DC.replicate(want, cell)))


@pytest.mark.parametrize('w', [1.0, 0.5])
@pytest.mark.parametrize('clamp', list(CLAMPS))
@pytest.mark.parametrize('cell', [(4, 1, 1), (1, 1, 8), (2, 2, 2)])
def test_cell_project_is_the_reference_bit_for_bit(cell, clamp, w):
    """B C = 3 cubes of edge 8; fresh output and in place (``out`` aliasing ``x0``)."""
    from diffusioniqt_amd import ops
    rng = np.random.default_rng(5)
    x0 = (rng.standard_normal((3, 1, 8, 8, 8)) * 2).astype(np.float32)
    meas = DC.replicate(rng.standard_normal((3, 1) + tuple(8 // f for f in cell)).astype(np.float32), cell)
    c = CLAMPS[clamp]
    want = DC.project32(DC.clamp32(*(c or (0., 0., None)))(x0), meas, cell, w)
    x = cu(x0)
    got = ops.cell_project(x, cu(meas), cell, w, clamp=c)
    assert got.data_ptr() != x.data_ptr() and torch.equal(x, cu(x0))
    assert np.array_equal(bits(got), bits(want))
    same = ops.cell_project(x, cu(meas), cell, w, clamp=c, out=x)
    assert same.data_ptr() == x.data_ptr() and torch.equal(x, got)
    if w == 1.0 and c is None:                                # what it is for: the cell means are the measurement's
        err = np.abs(DC.cell_mean32(got.cpu().numpy(), cell).astype(np.float64) - DC.cell_mean32(meas, cell)).max()
        assert err <= 2 * DC.projection_roundings(cell, max(float(np.abs(x0).max()), float(np.abs(meas).max())))


def test_cell_project_argument_errors():
    from diffusioniqt_amd import ops
    x = torch.zeros(2, 1, 8, 8, 8, device=DEV)
    with pytest.raises(ValueError, match="consistency cell"):
        ops.cell_project(x, x.clone(), (3, 1, 1))
    with pytest.raises(ValueError, match="consistency weight"):
        ops.cell_project(x, x.clone(), (2, 2, 2), 0.0)
    with pytest.raises(ValueError, match="meas_up must have"):
        ops.cell_project(x, x[:1].clone(), (2, 2, 2))
    with pytest.raises(ValueError, match="clamp mode"):
        ops.cell_project(x, x.clone(), (2, 2, 2), clamp=(-1., 1., 2))
    with pytest.raises(ValueError, match="consistency cell"):
        ops.cell_mean(x[0, 0], (1, 1, 3))


# ---- G2: the fused joint step, bit for bit -------------------------------------------------------------------------------------------------
def _step_refs(stride, kind):
    """The case, its device tensors' sources and the fused x0 per clamp (the walk does not depend on the cell)."""
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
@pytest.mark.parametrize('cell', DC.STEP_CELLS)
@pytest.mark.parametrize('tiling', DC.STEP_TILINGS, ids=['s4-gaussian', 's5-constant'])
def test_joint_consistent_step_is_the_reference_bit_for_bit(tiling, cell, form):
    """Every voxel is compared: nothing is excluded.  The fresh launch, then the same launch in place (``x_next`` aliasing ``x_t`` and,
    where there is a history, ``x0_out`` aliasing ``x0_prev``)."""
    from diffusioniqt_amd import ops
    stride, kind = tiling
    c = _step_refs(stride, kind)
    f, with_prev, kn = FORMS[form]
    clamp = 'min' if cell[2] != 1 else 'box'
    w, draw = (1.0, 5) if sum(cell) % 2 else (0.5, 3)
    meas = DC.step_meas(c, cell)
    n = _normals(draw) if kn != 0 else None
    want, want0, covered = DC.joint_step32(c['y'], c['slot'], c['taps'], stride, c['x'], c['prev'] if with_prev else None, meas, cell, w,
                                           f, KX, K0, KP, kn, None, n, fused=c['fused'][clamp])
    whole = DC.replicate(DC._cells(covered, cell).all(axis=(-5, -3, -1)), cell)
    assert whole.any() and (~covered).any() and (covered[:16, :16, :64] == False).any()         # uncovered voxels inside the volume too
    args = (cu(c['y']), cu(c['slot'].astype(np.int32)), cu(c['taps']))
    tail = (cu(meas), cell, w, f, KX, K0, KP, kn, *CLAMPS[clamp], stride, SEED, draw, SAMPLE)
    x, prev = cu(c['x']), cu(c['prev']) if with_prev else None
    got, got0 = ops.volume_joint_consistent_step(*args, x, prev, *tail)
    assert got.data_ptr() != x.data_ptr() and torch.equal(x, cu(c['x']))
    bad, bad0 = (bits(got) != bits(want)).sum(), (bits(got0) != bits(want0)).sum()
    print(f"consistent step {form} stride {stride} {kind} cell {cell} w {w}: {bad} / {bad0} of {want.size} voxels differ; corrected "
          f"share {whole.mean():.3f}, covered voxels of partly covered cells {(covered & ~whole).sum()}")
    assert bad == 0 and bad0 == 0
    assert np.array_equal(bits(got)[~covered], bits(c['x'])[~covered]) and not got0.cpu().numpy()[~covered].any()
    ops.volume_joint_consistent_step(*args, x, prev, *tail, out=x, x0_out=prev)
    assert torch.equal(x, got) and (prev is None or torch.equal(prev, got0))


def test_joint_consistent_step_argument_errors():
    from diffusioniqt_amd import ops
    c = _step_refs(4, 'gaussian')
    y, slot, taps, x = cu(c['y']), cu(c['slot'].astype(np.int32)), cu(c['taps']), cu(c['x'])
    ok = (0, KX, K0, 0.0, 0.0, -1.0, 1.0, 1, 4)
    with pytest.raises(ValueError, match="consistency cell"):
        ops.volume_joint_consistent_step(y, slot, taps, x, None, x.clone(), (3, 1, 1), 1.0, *ok)      # 20 % 3
    with pytest.raises(ValueError, match="consistency weight"):
        ops.volume_joint_consistent_step(y, slot, taps, x, None, x.clone(), (2, 2, 2), 0.0, *ok)
    with pytest.raises(ValueError, match="meas_up"):
        ops.volume_joint_consistent_step(y, slot, taps, x, None, x[:10].clone(), (2, 2, 2), 1.0, *ok)
    with pytest.raises(ValueError, match="form"):
        ops.volume_joint_consistent_step(y, slot, taps, x, None, x.clone(), (2, 2, 2), 1.0, 3, *ok[1:])


# ---- G3: the chains through VolumeInference against the float64 reference ----------------------------------------------------------------------
CHAIN_VOL, CHAIN_P, CHAIN_STRIDE = (16, 16, 24), 8, 4
CHAIN_CELLS = [(2, 2, 2), (4, 1, 1)]


def chain_volume():
    vol = np.random.default_rng(7).integers(1, 1000, CHAIN_VOL).astype(np.float32)
    vol[:8, :8, :12] = 0                                       # the 5 % rule drops two windows: 4 x 4 x 8 voxels are covered by none
    return vol


def chain_cfg(stride=CHAIN_STRIDE, batch_size=7):
    return R.shared_cfg(stride, batch_size=batch_size, P=CHAIN_P)


VP = {'ddim-eta0': ('ddim', 0.0), 'ddim-eta0.5': ('ddim', 0.5), 'ddpm': ('ddpm', 0.0), 'dpmpp2m': ('dpmpp2m', 0.0)}


def vp_denoiser(imagen, sampler, eta):
    return imagen.window_denoiser(sampler=sampler, sample_steps=J.STEPS, eta=eta)


def vp_reference(imagen, name, cell, w, vol, cfg, blend, samples=1):
    sampler, eta = VP[name]
    sched = imagen.noise_schedulers[1]
    coefs = vp_denoiser(imagen, sampler, eta).coefs.numpy().astype(np.float64)             # the chain's host numbers, widened
    log_snr = J.tables(sched, J.STEPS, 0.0, 'x_start')[2]
    meas = DC.measurement(vol, cell)
    meas_up = DC.measurement_state(meas, cell, cfg)
    finals, x0_max = [], 0.0
    for s in range(samples):
        x, L, m, whole = DC.vp_chain(vol, cfg, coefs, log_snr, (J.MIN_BOUND, 0., 0), blend, meas_up, cell, w, sampler == 'dpmpp2m', J.SEED, s)
        finals.append(np.maximum(x, J.MIN_BOUND))
        x0_max = max(x0_max, m)
    ref = DC.finish(vol, cfg, finals, L)
    if sampler == 'dpmpp2m':
        table, k01 = M.table64(*M.chain_log_snr(sched, J.STEPS))
        bound = M.chain_bound(ref['windows_per_voxel'], ref['scale'], M.amplification(table, k01))
    else:
        bound = J.chain_bound(ref['windows_per_voxel'], ref['scale'])
    ref.update(bound=bound + J.STEPS * DC.projection_roundings(cell, max(x0_max, float(np.abs(meas_up).max()))), meas=meas, whole=whole,
               state=x)
    return ref


def check(got, ref, what, key='mean', factor=1):
    got = got.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == ref[key].shape and np.isfinite(got).all()
    err = np.abs(got.astype(np.float64) - ref[key]).max()
    print(f"{what}: max |{key} - ref| = {err:.3e}, bound {factor * ref['bound']:.3e}")
    assert err <= factor * ref['bound'], what
    return got


@pytest.mark.parametrize('cell', CHAIN_CELLS)
@pytest.mark.parametrize('name', list(VP))
def test_consistent_joint_chain_matches_the_float64_reference(name, cell):
    from diffusioniqt_amd.inference import VolumeInference
    imagen = stub_imagen('x_start', 'clamp-min', size=CHAIN_P)
    vol, cfg, w = chain_volume(), chain_cfg(), 1.0 if cell == (2, 2, 2) else 0.5
    ref = cached(('vp', name, cell), lambda: vp_reference(imagen, name, cell, w, vol, cfg, 'gaussian'))
    plain = cached(('vp-plain', name), lambda: VolumeInference(cfg, vp_denoiser(imagen, *VP[name]), blend='gaussian', noise='anchored',
                                                                joint=True, seed=J.SEED)(cu(vol)).cpu().numpy())
    inf = VolumeInference(cfg, vp_denoiser(imagen, *VP[name]), blend='gaussian', noise='anchored', joint=True, seed=J.SEED,
                          consistency=(torch.from_numpy(ref['meas']), cell), consistency_weight=w)
    got = check(inf(cu(vol)), ref, f"consistent joint {name} cell {cell} w {w}")
    live = ref['covered'] & ~ref['background']
    assert (~ref['covered']).any() and np.abs(got - plain)[live].max() > 0.05            # and it is not the plain chain


@pytest.mark.parametrize('cell', CHAIN_CELLS)
@pytest.mark.parametrize('eta', list(E.ETAS))
def test_consistent_edm_joint_chain_matches_the_float64_reference(eta, cell):
    from diffusioniqt_amd.inference import VolumeInference
    eta = E.ETAS[eta]
    elu = HN.make_elucidated('churn-on', False, size=CHAIN_P).to(DEV)
    den = elu.window_denoiser(sampler='dpmpp2m', eta=eta)
    vol, cfg = chain_volume(), chain_cfg()
    meas = DC.measurement(vol, cell)

    def make():
        tabs = E.tables(HN.HP, eta, coefs=den.coefs.numpy())
        x, L, state_max, x0_max, _ = DC.edm_chain(vol, cfg, tabs, 'gaussian', False, DC.measurement_state(meas, cell, cfg), cell, 1.0)
        ref = DC.finish(vol, cfg, [np.clip(x, -1.0, 1.0)], L)
        mean32, std32 = np.float32(cfg['Data']['mean']), np.float32(cfg['Data']['std'])
        lowres_max = tabs['lowres'][0] * float(np.abs((vol - mean32) / std32).max()) + 6 * tabs['lowres'][1]
        meas_max = float(np.abs(DC.measurement_state(meas, cell, cfg)).max())
        assert 1.0 < x0_max <= 3.0 and meas_max <= 1.0                                     # |D| <= 1, so |x0'| <= 1 + 2
        ref['bound'] = DC.edm_bound(tabs, L, cell, state_max, lowres_max, False, max(x0_max, meas_max))
        return ref
    ref = cached(('edm', eta, cell), make)
    inf = VolumeInference(cfg, den, blend='gaussian', noise='anchored', joint=True, seed=E.SEED, consistency=(torch.from_numpy(meas), cell))
    check(inf(cu(vol)), ref, f"consistent joint EDM dpmpp2m eta {eta} cell {cell}")


# ---- G4: stride = patch: the joint chain is the per-window sampler ------------------------------------------------------------------------------
@pytest.mark.parametrize('cell', [(4, 1, 1), (2, 2, 2), (1, 1, 8)])
@pytest.mark.parametrize('name', ['ddim-eta0.5', 'ddpm', 'dpmpp2m'])
def test_consistent_joint_at_stride_equal_patch_is_the_independent_path(name, cell):
    """No overlap, unit weights: num / den is exact and no cell straddles a window, so the fused projection is ``ops.cell_project`` on
    every window and both paths take the same ``__device__`` projection and update -- equal at every voxel, bit for bit."""
    from diffusioniqt_amd.inference import VolumeInference
    sampler, eta = VP[name]
    for mode in ('clamp-min', 'dynamic'):
        imagen = stub_imagen('x_start', mode, size=CHAIN_P)
        vol, cfg = cu(chain_volume()), chain_cfg(stride=CHAIN_P)
        cons = dict(consistency=(torch.from_numpy(DC.measurement(chain_volume(), cell)), cell), consistency_weight=0.75)

        def sample_fn(x, noise=None, **kw):
            assert set(kw) == {'consistency', 'consistency_weight'}
            return imagen.sample(batch_size=x.shape[0], start_image_or_video=x, start_at_unet_number=2, use_tqdm=False, sampler=sampler,
                                 sample_steps=J.STEPS, eta=eta, noise=noise, **kw)[0]
        independent = VolumeInference(cfg, sample_fn, blend='constant', noise='anchored', seed=J.SEED, **cons)(vol)
        joint = VolumeInference(cfg, vp_denoiser(imagen, sampler, eta), blend='constant', noise='anchored', joint=True, seed=J.SEED,
                                **cons)(vol)
        assert independent.unique().numel() > 1000
        assert torch.equal(joint, independent), mode


@pytest.mark.parametrize('cell', [(4, 1, 1), (2, 2, 2), (1, 1, 8)])
@pytest.mark.parametrize('eta', list(E.ETAS))
def test_consistent_edm_joint_at_stride_equal_patch_is_the_independent_path(eta, cell):
    from diffusioniqt_amd.inference import VolumeInference
    eta = E.ETAS[eta]
    for dynamic in (False, True):
        elu = HN.make_elucidated('churn-on', dynamic, self_cond=True, size=CHAIN_P).to(DEV)
        vol, cfg = cu(chain_volume()), chain_cfg(stride=CHAIN_P)
        cons = dict(consistency=(torch.from_numpy(DC.measurement(chain_volume(), cell)), cell), consistency_weight=0.75)

        def sample_fn(x, noise=None, **kw):
            return elu.sample(batch_size=x.shape[0], video_frames=CHAIN_P, start_image_or_video=x, start_at_unet_number=2, noise=noise,
                              sampler='dpmpp2m', eta=eta, use_tqdm=False, **kw)
        independent = VolumeInference(cfg, sample_fn, blend='constant', noise='anchored', seed=E.SEED, **cons)(vol)
        joint = VolumeInference(cfg, elu.window_denoiser(sampler='dpmpp2m', eta=eta), blend='constant', noise='anchored', joint=True,
                                seed=E.SEED, **cons)(vol)
        assert independent.unique().numel() > 1000
        assert torch.equal(joint, independent), dynamic


# ---- G5: the guarantee -------------------------------------------------------------------------------------------------------------------------
GUARANTEE_CELLS = [(2, 2, 2), (4, 1, 1), (1, 1, 3)]          # (1, 1, 3) straddles the windows (P 8, stride 4): only the joint state projects it


def _cell_means64(x, cell):
    return DC._cells(np.asarray(x, dtype=np.float64), cell).mean(axis=(-5, -3, -1))


def _whole_cells(vol, cfg, cell):
    L = J.layout(vol, cfg)
    covered = R.blend_accumulate(np.zeros((1, L['kept'].shape[0], CHAIN_P, CHAIN_P, CHAIN_P)), L['slot'], np.ones(CHAIN_P), L['stride'],
                                 vol.shape)[2]
    whole = DC._cells(covered, cell).all(axis=(-5, -3, -1))
    assert 0 < whole.sum() < whole.size
    return whole


@pytest.mark.parametrize('cell', GUARANTEE_CELLS)
def test_final_state_has_the_measurements_cell_means(cell):
    """A deterministic chain whose last step has kx = 0 and k0 = 1 -- the EDM family's DPM-Solver++ 2M ODE, which ends at sigma = 0 --
    with no step clamp and w = 1, taken from the ops-level chain before ``finish``: the state IS the projected x0, and its cell means,
    recomputed in float64, are the measurement's on every fully covered cell, within the projection's roundings of ONE step."""
    from diffusioniqt_amd.inference import VolumeInference
    elu = HN.make_elucidated('churn-on', False, size=CHAIN_P).to(DEV)
    den = elu.window_denoiser(sampler='dpmpp2m', eta=0.0)
    assert den.clamp == (-float('inf'), float('inf'), 1) and den.coefs[-1].tolist() == [0.0, 1.0, 0.0, 0.0]
    vol, cfg = chain_volume(), chain_cfg()
    meas = DC.measurement(vol, cell)
    states = []
    den.finish = lambda x: states.append(x.clone()) or x                                  # the state the chain ends in, before any finish
    VolumeInference(cfg, den, blend='gaussian', noise='anchored', joint=True, seed=E.SEED, consistency=(torch.from_numpy(meas), cell))(cu(vol))
    x = states[0].cpu().numpy()
    whole = _whole_cells(vol, cfg, cell)
    want = DC.measurement_state(meas, cell, cfg)[::cell[0], ::cell[1], ::cell[2]]
    err = np.abs(_cell_means64(x, cell) - want)[whole].max()
    bound = DC.projection_roundings(cell, max(1.0, float(np.abs(x).max()), float(np.abs(want).max())))   # 1: the clamped prediction
    print(f"guarantee EDM ODE cell {cell}: max |A x - y| = {err:.3e} on {whole.sum()} of {whole.size} cells, bound {bound:.3e}")
    assert err <= bound
    i, j, k = (int(v[0]) for v in whole.nonzero())
    assert np.ptp(DC._cells(x, cell)[i, :, j, :, k, :]) > 0                                # the detail inside a cell is the network's


@pytest.mark.parametrize('cell', GUARANTEE_CELLS)
def test_ddim_chain_ends_on_a_consistent_prediction(cell, monkeypatch):
    """The deterministic ddim chain with no clamp and w = 1.  The schedule of the DDPM family ends at a finite log-SNR, so its last step
    is NOT (kx, k0) = (0, 1) -- 4 steps of the cosine schedule end on (0.0319, 0.9706) -- and the final state is kx x_t + k0 x0', not
    x0' itself.  What holds exactly is DDNM's own statement: the last corrected prediction x0' (``x0_out`` of the last fused launch) has
    the measurement's cell means on every fully covered cell, within the projection's roundings of one step; and the cell means of the
    final state are kx A x_t + k0 y, within that plus the update's three roundings."""
    from diffusioniqt_amd import ops
    from diffusioniqt_amd.inference import VolumeInference
    imagen = stub_imagen('x_start', 'dynamic', size=CHAIN_P)                              # dynamic: the step clamp is (-inf, inf)
    den = vp_denoiser(imagen, 'ddim', 0.0)
    kx, k0, kn = den.coefs[-1].tolist()
    assert den.clamp == (-float('inf'), float('inf'), 1) and kn == 0 and 0 < kx < 0.05 and 0.95 < k0 < 1
    vol, cfg = chain_volume(), chain_cfg()
    meas = DC.measurement(vol, cell)
    real, calls = ops.volume_joint_consistent_step, []

    def recording(y, slot, taps, x_t, *a, **kw):
        before = x_t.clone()
        out, x0 = real(y, slot, taps, x_t, *a, **kw)
        calls.append((before, out.clone(), x0.clone()))
        return out, x0
    monkeypatch.setattr(ops, 'volume_joint_consistent_step', recording)
    VolumeInference(cfg, den, blend='gaussian', noise='anchored', joint=True, seed=J.SEED, consistency=(torch.from_numpy(meas), cell))(cu(vol))
    assert len(calls) == J.STEPS
    x_t, x, x0 = (t.cpu().numpy() for t in calls[-1])
    whole = _whole_cells(vol, cfg, cell)
    want = DC.measurement_state(meas, cell, cfg)[::cell[0], ::cell[1], ::cell[2]]
    scale = max(1.0, float(np.abs(x0).max()), float(np.abs(want).max()))                  # 1: the thresholded prediction before the projection
    err0 = np.abs(_cell_means64(x0, cell) - want)[whole].max()
    err = np.abs(_cell_means64(x, cell) - (kx * _cell_means64(x_t, cell) + k0 * want))[whole].max()
    bound0 = DC.projection_roundings(cell, scale)
    bound = k0 * bound0 + 3 * 2.0 ** -24 * (kx * float(np.abs(x_t).max()) + k0 * scale)
    print(f"ddim cell {cell}: max |A x0' - y| = {err0:.3e} (bound {bound0:.3e}), max |A x - (kx A x_t + k0 y)| = {err:.3e} (bound {bound:.3e})")
    assert err0 <= bound0 and err <= bound


# ---- G6: block mode and samples ----------------------------------------------------------------------------------------------------------------
def test_consistent_joint_block_mode_matches_the_float64_reference():
    from diffusioniqt_amd.inference import VolumeInference
    imagen = stub_imagen('x_start', 'clamp-min', size=8)
    vol, cfg, cell = R.block_volume(), R.block_cfg(), (2, 2, 2)                             # sub 8, P 24, stride 16
    ref = cached(('vp-block',), lambda: vp_reference(imagen, 'ddim-eta0.5', cell, 1.0, vol, cfg, 'gaussian'))
    inf = VolumeInference(cfg, vp_denoiser(imagen, 'ddim', 0.5), blend='gaussian', noise='anchored', joint=True, seed=J.SEED,
                          consistency=(torch.from_numpy(ref['meas']), cell))
    check(inf(cu(vol)), ref, "consistent joint block mode P 24 stride 16")


def test_consistent_blend_block_mode_projects_every_sub_volume():
    """``batch_sample`` outside the joint mode: the sampler sees the block split into its sub-volumes, and the windows of the
    measurement split the same way (``sub`` and the stride are multiples of the cell)."""
    from diffusioniqt_amd.inference import VolumeInference
    imagen = stub_imagen('x_start', 'dynamic', size=8)
    vol, cfg, cell = R.block_volume(), R.block_cfg(), (2, 2, 2)
    meas = DC.measurement(vol, cell)
    seen = []

    def sample_fn(x, noise=None, consistency=None, consistency_weight=None):
        seen.append(tuple(consistency[0].shape))
        return imagen.sample(batch_size=x.shape[0], start_image_or_video=x, start_at_unet_number=2, use_tqdm=False, sampler='ddim',
                             sample_steps=J.STEPS, noise=noise, consistency=consistency, consistency_weight=consistency_weight)[0]
    VolumeInference(cfg, sample_fn, noise='anchored', seed=J.SEED, consistency=(torch.from_numpy(meas), cell))(cu(vol))
    assert len(seen) == 27 and set(seen) == {(27, 1, 8, 8, 8)}


def test_consistent_joint_samples_are_deterministic():
    from diffusioniqt_amd.inference import VolumeInference
    imagen = stub_imagen('x_start', 'clamp-min', size=CHAIN_P)
    vol, cfg, cell = chain_volume(), chain_cfg(), (2, 2, 2)
    ref = cached(('vp-s2',), lambda: vp_reference(imagen, 'ddim-eta0.5', cell, 1.0, vol, cfg, 'gaussian', samples=2))
    make = lambda: VolumeInference(cfg, vp_denoiser(imagen, 'ddim', 0.5), blend='gaussian', noise='anchored', joint=True, seed=J.SEED,
                                   samples=2, consistency=(torch.from_numpy(ref['meas']), cell))
    mean, std = make()(cu(vol), return_std=True)
    check(mean, ref, "consistent joint S = 2 mean")
    check(std, ref, "consistent joint S = 2 deviation", key='std', factor=2)
    again, again_std = make()(cu(vol), return_std=True)
    assert torch.equal(mean, again) and torch.equal(std, again_std) and float(std.max()) > 0
