"""Data consistency for a tile-local linear operator on a real MI355X against tests/volume_joint_tile_reference.py:
``ops.tile_measure`` / ``ops.tile_backproject`` / ``ops.tile_project`` and the fused joint step bit for bit against the fp32 restatement
(no voxel is left out of a comparison), the joint chains of both families through ``VolumeInference(consistency_operator=...)``
against the float64 chains, the bit-for-bit tie of the joint chain at stride = patch to ``sample(consistency_operator=...)`` per
window, the guarantee (A x = y for a y in the range of A, P x = t for stacks that contradict each other) and a one-row operator
against the ``consistency=`` path.  The shapes are those of tests/test_gpu_volume_dc.py.

Bounds: that module's docstring.  The chain tests take the family's ``chain_bound`` plus ``steps`` times the projection's own
roundings, ((n + 1) G + 2) 2^-24 of the largest magnitude involved, G the operator's gain; the guarantee tests take
``residual_bound_A`` / ``residual_bound_P``."""

import numpy as np
import pytest
import torch

from tests import dpmpp2m_reference as M
from tests import edm_dpmpp2m_reference as E
from tests import volume_blend_reference as R
from tests import volume_joint_dc_reference as DC
from tests import volume_joint_heun_reference as HN
from tests import volume_joint_reference as J
from tests import volume_joint_tile_reference as TR
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


def operator_of(name):
    """(cell, A, the host operator, its table as numpy, its table on the device), made once per name."""
    def make():
        from diffusioniqt_amd import ops
        cell, A = TR.matrix_of(name)
        op = ops.tile_operator(cell, A)
        return cell, A, op, op.table.numpy(), op.table.to(DEV)
    return cached(('op', name), make)


# ---- G1: the operator, the back-projection and the per-window projection, bit for bit -----------------------------------------------------
@pytest.mark.parametrize('name', list(TR.OPERATORS))
def test_tile_measure_and_backproject_are_the_reference_bit_for_bit(name):
    from diffusioniqt_amd import ops
    cell, A, op, _, _ = operator_of(name)
    shape = tuple(f * k for f, k in zip(cell, (3, 2, 5)))
    x = (np.random.default_rng(4).standard_normal(shape) * 3).astype(np.float32)
    y = ops.tile_measure(cu(x), op)
    want = TR.measure32(x, cell, A)
    assert tuple(y.shape) == want.shape == (op.m, 3, 2, 5) and np.array_equal(bits(y), bits(want))
    t = ops.tile_backproject(y, op)
    want_t = TR.backproject32(want, cell, op.pinv.numpy())
    assert tuple(t.shape) == shape and np.array_equal(bits(t), bits(want_t))
    with pytest.raises(ValueError, match="consistency_operator"):
        ops.tile_backproject(y[:-1].contiguous() if op.m > 1 else y[None], op)


@pytest.mark.parametrize('w', [1.0, 0.5])
@pytest.mark.parametrize('clamp', list(CLAMPS))
@pytest.mark.parametrize('name', ['stacks-222', 'stacks-421', 'stack-411'])
def test_tile_project_is_the_reference_bit_for_bit(name, clamp, w):
    """B C = 3 cubes of edge 8; fresh output and in place (``out`` aliasing ``x0``).  Every voxel is compared."""
    from diffusioniqt_amd import ops
    cell, A, op, table, dev = operator_of(name)
    rng = np.random.default_rng(5)
    x0 = (rng.standard_normal((3, 1, 8, 8, 8)) * 2).astype(np.float32)
    target = rng.standard_normal((3, 1, 8, 8, 8)).astype(np.float32)
    c = CLAMPS[clamp]
    a = TR.clamp32(*(c or (0., 0., None)))(x0)
    want = TR.project_tile32(a, target, cell, table, w)
    x = cu(x0)
    got = ops.tile_project(x, cu(target), cell, dev, w, clamp=c)
    assert got.data_ptr() != x.data_ptr() and torch.equal(x, cu(x0))
    assert np.array_equal(bits(got), bits(want))
    same = ops.tile_project(x, cu(target), cell, dev, w, clamp=c, out=x)
    assert same.data_ptr() == x.data_ptr() and torch.equal(x, got)


def test_tile_ops_argument_errors():
    from diffusioniqt_amd import ops
    x = torch.zeros(2, 1, 8, 8, 8, device=DEV)
    cell, _, op, _, table = operator_of('stacks-222')
    with pytest.raises(ValueError, match="consistency cell"):
        ops.tile_project(x, x.clone(), (3, 1, 1), table)
    with pytest.raises(ValueError, match="consistency weight"):
        ops.tile_project(x, x.clone(), cell, table, 0.0)
    with pytest.raises(ValueError, match="consistency_operator table"):
        ops.tile_project(x, x.clone(), (4, 1, 1), table)                                   # [8, 8] is not [4, 4]
    with pytest.raises(ValueError, match="consistency_operator table"):
        ops.tile_project(x, x.clone(), cell, table.cpu())
    with pytest.raises(ValueError, match="clamp mode"):
        ops.tile_project(x, x.clone(), cell, table, clamp=(-1., 1., 2))
    with pytest.raises(ValueError, match="consistency_operator"):
        ops.tile_measure(x[0, 0], table)                                                   # the table is not the operator
    with pytest.raises(ValueError, match="consistency cell"):
        ops.tile_measure(torch.zeros(8, 8, 7, device=DEV), op)


# ---- G2: the fused joint step, bit for bit -------------------------------------------------------------------------------------------------
STEP_OPERATORS = ['stacks-222', 'stack-411', 'stacks-135', 'dense-232']
FORMS = {'step-kn0': (0, False, 0.0), 'step-kn': (0, False, 0.625), 'multistep-noprev': (1, False, 0.0), 'multistep-prev': (1, True, 0.0),
         'sde-prev-kn': (2, True, 0.625)}
BIG_VOL = (12, 16, 72)                                         # the n = 64 case: every edge a multiple of 4


def _step_refs(stride, kind, shape=DC.STEP_VOL):
    """The case, its device tensors' sources and the fused x0 per clamp (the walk does not depend on the cell)."""
    def make():
        if shape == DC.STEP_VOL:
            c = DC.step_case(stride, kind)
        else:                                                  # ``step_case`` on another volume, its corner zeroed likewise
            rng = np.random.default_rng(100 * stride + 1)
            raw = rng.integers(1, 1000, shape).astype(np.float32)
            raw[:8, :8, :32] = 0
            L = J.layout(raw, R.shared_cfg(stride, P=DC.STEP_P))
            N = L['kept'].shape[0]
            c = dict(stride=stride, kind=kind, slot=L['slot'], N=N, taps=R.taps_of(DC.STEP_P, kind).astype(np.float32),
                     y=(rng.standard_normal((N,) + (DC.STEP_P,) * 3) * 2).astype(np.float32),
                     x=(rng.standard_normal(shape) * 3).astype(np.float32), prev=(rng.standard_normal(shape) * 2).astype(np.float32),
                     coarse=rng.standard_normal(shape).astype(np.float32))
        c['fused'] = {name: TR.fuse32(c['y'], c['slot'], c['taps'], stride, shape, TR.clamp32(*cl))
                      for name, cl in (('min', CLAMPS['min']), ('box', CLAMPS['box']))}
        return c
    return cached(('step', stride, kind, shape), make)


def _normals(draw, shape=DC.STEP_VOL):
    from diffusioniqt_amd import ops
    return cached(('n', draw, shape), lambda: ops.volume_joint_init(shape, SEED, sample=SAMPLE, draw=draw).cpu().numpy())


def _check_step(c, stride, name, form, shape):
    from diffusioniqt_amd import ops
    cell, A, op, table, dev = operator_of(name)
    f, with_prev, kn = FORMS[form]
    clamp = 'min' if cell[2] != 1 else 'box'
    w, draw = (1.0, 5) if sum(cell) % 2 else (0.5, 3)
    target = c['coarse']                                       # any volume: t need not be constant over a tile
    n = _normals(draw, shape) if kn != 0 else None
    want, want0, covered = TR.joint_step_tile32(c['y'], c['slot'], c['taps'], stride, c['x'], c['prev'] if with_prev else None, target,
                                                cell, table, w, f, KX, K0, KP, kn, None, n, fused=c['fused'][clamp])
    whole = TR.replicate(TR._cells(covered, cell).all(axis=(-5, -3, -1)), cell)
    assert whole.any() and (~covered).any() and (covered[:8, :8, :8] == False).any()             # uncovered voxels inside the volume too
    args = (cu(c['y']), cu(c['slot'].astype(np.int32)), cu(c['taps']))
    tail = (cu(target), cell, dev, w, f, KX, K0, KP, kn, *CLAMPS[clamp], stride, SEED, draw, SAMPLE)
    x, prev = cu(c['x']), cu(c['prev']) if with_prev else None
    got, got0 = ops.volume_joint_consistent_tile_step(*args, x, prev, *tail)
    assert got.data_ptr() != x.data_ptr() and torch.equal(x, cu(c['x']))
    bad, bad0 = (bits(got) != bits(want)).sum(), (bits(got0) != bits(want0)).sum()
    print(f"tile step {form} stride {stride} {name} w {w}: {bad} / {bad0} of {want.size} voxels differ; corrected share "
          f"{whole.mean():.3f}, covered voxels of partly covered tiles {(covered & ~whole).sum()}")
    assert bad == 0 and bad0 == 0
    assert np.array_equal(bits(got)[~covered], bits(c['x'])[~covered]) and not got0.cpu().numpy()[~covered].any()
    partly = covered & ~whole
    assert np.array_equal(bits(got0)[partly], bits(c['fused'][clamp][0])[partly])             # the plain update: x0 as fused
    assert (bits(got0) != bits(c['fused'][clamp][0]))[whole].mean() > 0.9                      # and the whole tiles did move
    ops.volume_joint_consistent_tile_step(*args, x, prev, *tail, out=x, x0_out=prev)
    assert torch.equal(x, got) and (prev is None or torch.equal(prev, got0))


@pytest.mark.parametrize('form', list(FORMS))
@pytest.mark.parametrize('name', STEP_OPERATORS)
@pytest.mark.parametrize('tiling', DC.STEP_TILINGS, ids=['s4-gaussian', 's5-constant'])
def test_joint_tile_step_is_the_reference_bit_for_bit(tiling, name, form):
    """Every voxel is compared: nothing is excluded.  The fresh launch, then the same launch in place (``x_next`` aliasing ``x_t`` and,
    where there is a history, ``x0_out`` aliasing ``x0_prev``).  A tile with an uncovered voxel keeps the plain update: its covered
    voxels report the fused x0 itself."""
    stride, kind = tiling
    _check_step(_step_refs(stride, kind), stride, name, form, DC.STEP_VOL)


@pytest.mark.parametrize('form', ['step-kn', 'sde-prev-kn'])
def test_joint_tile_step_with_the_full_table_is_the_reference_bit_for_bit(form):
    """n = 64: tile (4, 4, 4) with all three stacks, the 16 KiB table and the longest sum, on a (12, 16, 72) volume."""
    _check_step(_step_refs(4, 'gaussian', BIG_VOL), 4, 'stacks-444', form, BIG_VOL)


def test_joint_tile_step_argument_errors():
    from diffusioniqt_amd import ops
    c = _step_refs(4, 'gaussian')
    y, slot, taps, x = cu(c['y']), cu(c['slot'].astype(np.int32)), cu(c['taps']), cu(c['x'])
    cell, _, _, _, table = operator_of('stacks-222')
    ok = (0, KX, K0, 0.0, 0.0, -1.0, 1.0, 1, 4)
    with pytest.raises(ValueError, match="consistency cell"):
        ops.volume_joint_consistent_tile_step(y, slot, taps, x, None, x.clone(), (3, 1, 1), table, 1.0, *ok)         # 20 % 3
    with pytest.raises(ValueError, match="consistency weight"):
        ops.volume_joint_consistent_tile_step(y, slot, taps, x, None, x.clone(), cell, table, 0.0, *ok)
    with pytest.raises(ValueError, match="meas_up"):
        ops.volume_joint_consistent_tile_step(y, slot, taps, x, None, x[:10].clone(), cell, table, 1.0, *ok)
    with pytest.raises(ValueError, match="consistency_operator table"):
        ops.volume_joint_consistent_tile_step(y, slot, taps, x, None, x.clone(), (4, 1, 1), table, 1.0, *ok)
    with pytest.raises(ValueError, match="form"):
        ops.volume_joint_consistent_tile_step(y, slot, taps, x, None, x.clone(), cell, table, 1.0, 3, *ok[1:])


# ---- G3: the chains through VolumeInference against the float64 reference ----------------------------------------------------------------------
CHAIN_VOL, CHAIN_P, CHAIN_STRIDE = (16, 16, 24), 8, 4
CHAIN_OPERATORS = ['stacks-222', 'stacks-421']


def chain_volume():
    vol = np.random.default_rng(7).integers(1, 1000, CHAIN_VOL).astype(np.float32)
    vol[:8, :8, :12] = 0                                       # the 5 % rule drops two windows: 4 x 4 x 8 voxels are covered by none
    return vol


def chain_cfg(stride=CHAIN_STRIDE, batch_size=7):
    return R.shared_cfg(stride, batch_size=batch_size, P=CHAIN_P)


def chain_rows(op, seed=3):
    """A raw measurement [m, D/fz, H/fy, W/fx]: every row uniform in [100, 500] on its own, so the stacks contradict each other."""
    return np.random.default_rng(seed).uniform(100.0, 500.0, (op.m,) + tuple(s // f for s, f in zip(CHAIN_VOL, op.cell))).astype(np.float32)


VP = {'ddim-eta0': ('ddim', 0.0), 'ddim-eta0.5': ('ddim', 0.5), 'ddpm': ('ddpm', 0.0), 'dpmpp2m': ('dpmpp2m', 0.0)}


def vp_denoiser(imagen, sampler, eta):
    return imagen.window_denoiser(sampler=sampler, sample_steps=J.STEPS, eta=eta)


def vp_reference(imagen, name, op_name, w, vol, cfg, blend, rows=None):
    sampler, eta = VP[name]
    cell, A, op, table, _ = operator_of(op_name)
    sched = imagen.noise_schedulers[1]
    coefs = vp_denoiser(imagen, sampler, eta).coefs.numpy().astype(np.float64)             # the chain's host numbers, widened
    log_snr = J.tables(sched, J.STEPS, 0.0, 'x_start')[2]
    rows = chain_rows(op) if rows is None else rows
    target = TR.target_state(rows, cell, op.pinv.numpy(), cfg)
    x, L, x0_max, whole = TR.vp_chain(vol, cfg, coefs, log_snr, (J.MIN_BOUND, 0., 0), blend, target, cell, table, w,
                                      multistep=sampler == 'dpmpp2m', seed=J.SEED, sample=0)
    ref = DC.finish(vol, cfg, [np.maximum(x, J.MIN_BOUND)], L)
    if sampler == 'dpmpp2m':
        tab, k01 = M.table64(*M.chain_log_snr(sched, J.STEPS))
        bound = M.chain_bound(ref['windows_per_voxel'], ref['scale'], M.amplification(tab, k01))
    else:
        bound = J.chain_bound(ref['windows_per_voxel'], ref['scale'])
    own = J.STEPS * TR.tile_roundings(cell, table, max(x0_max, float(np.abs(target).max())))
    ref.update(bound=bound + own, rows=rows, whole=whole, state=x)
    return ref


def check(got, ref, what, key='mean', factor=1):
    got = got.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == ref[key].shape and np.isfinite(got).all()
    err = np.abs(got.astype(np.float64) - ref[key]).max()
    print(f"{what}: max |{key} - ref| = {err:.3e}, bound {factor * ref['bound']:.3e}")
    assert err <= factor * ref['bound'], what
    return got


@pytest.mark.parametrize('op_name', CHAIN_OPERATORS)
@pytest.mark.parametrize('name', list(VP))
def test_tile_joint_chain_matches_the_float64_reference(name, op_name):
    from diffusioniqt_amd.inference import VolumeInference
    imagen = stub_imagen('x_start', 'clamp-min', size=CHAIN_P)
    cell, A, op, _, _ = operator_of(op_name)
    vol, cfg, w = chain_volume(), chain_cfg(), 1.0 if op_name == 'stacks-222' else 0.5
    ref = cached(('vp', name, op_name), lambda: vp_reference(imagen, name, op_name, w, vol, cfg, 'gaussian'))
    inf = VolumeInference(cfg, vp_denoiser(imagen, *VP[name]), blend='gaussian', noise='anchored', joint=True, seed=J.SEED,
                          consistency=(torch.from_numpy(ref['rows']), cell), consistency_weight=w, consistency_operator=A)
    got = check(inf(cu(vol)), ref, f"tile joint {name} {op_name} w {w}")
    plain = cached(('vp-plain', name), lambda: VolumeInference(cfg, vp_denoiser(imagen, *VP[name]), blend='gaussian', noise='anchored',
                                                              joint=True, seed=J.SEED)(cu(vol)).cpu().numpy())
    live = ref['covered'] & ~ref['background']
    assert (~ref['covered']).any() and np.abs(got - plain)[live].max() > 0.01              # and it is not the unconstrained chain


@pytest.mark.parametrize('op_name', CHAIN_OPERATORS)
@pytest.mark.parametrize('eta', list(E.ETAS))
def test_tile_edm_joint_chain_matches_the_float64_reference(eta, op_name):
    from diffusioniqt_amd.inference import VolumeInference
    eta = E.ETAS[eta]
    elu = HN.make_elucidated('churn-on', False, size=CHAIN_P).to(DEV)
    den = elu.window_denoiser(sampler='dpmpp2m', eta=eta)
    cell, A, op, table, _ = operator_of(op_name)
    vol, cfg = chain_volume(), chain_cfg()
    rows = chain_rows(op)

    def make():
        tabs = E.tables(HN.HP, eta, coefs=den.coefs.numpy())
        target = TR.target_state(rows, cell, op.pinv.numpy(), cfg)
        x, L, state_max, x0_max, _ = TR.edm_chain(vol, cfg, tabs, 'gaussian', False, target, cell, table, 1.0)
        ref = DC.finish(vol, cfg, [np.clip(x, -1.0, 1.0)], L)
        mean32, std32 = np.float32(cfg['Data']['mean']), np.float32(cfg['Data']['std'])
        lowres_max = tabs['lowres'][0] * float(np.abs((vol - mean32) / std32).max()) + 6 * tabs['lowres'][1]
        ref['bound'] = TR.edm_bound(tabs, L, cell, table, state_max, lowres_max, False, max(x0_max, float(np.abs(target).max())))
        return ref
    ref = cached(('edm', eta, op_name), make)
    inf = VolumeInference(cfg, den, blend='gaussian', noise='anchored', joint=True, seed=E.SEED, consistency=(torch.from_numpy(rows), cell),
                          consistency_operator=op)
    check(inf(cu(vol)), ref, f"tile joint EDM dpmpp2m eta {eta} {op_name}")


# ---- G4: stride = patch: the joint chain is the per-window sampler ------------------------------------------------------------------------------
@pytest.mark.parametrize('op_name', CHAIN_OPERATORS)
@pytest.mark.parametrize('name', ['ddim-eta0.5', 'ddpm', 'dpmpp2m'])
def test_tile_joint_at_stride_equal_patch_is_the_independent_path(name, op_name):
    """No overlap, unit weights: num / den is exact and no tile straddles a window, so the fused projection is ``ops.tile_project`` on
    every window and both paths take the same ``__device__`` projection and update -- equal at every voxel, bit for bit."""
    from diffusioniqt_amd.inference import VolumeInference
    sampler, eta = VP[name]
    cell, A, op, _, _ = operator_of(op_name)
    for mode in ('clamp-min', 'dynamic'):
        imagen = stub_imagen('x_start', mode, size=CHAIN_P)
        vol, cfg = cu(chain_volume()), chain_cfg(stride=CHAIN_P)
        cons = dict(consistency=(torch.from_numpy(chain_rows(op)), cell), consistency_weight=0.75, consistency_operator=A)

        def sample_fn(x, noise=None, **kw):
            assert set(kw) == {'consistency', 'consistency_weight', 'consistency_operator'}
            return imagen.sample(batch_size=x.shape[0], start_image_or_video=x, start_at_unet_number=2, use_tqdm=False, sampler=sampler,
                                 sample_steps=J.STEPS, eta=eta, noise=noise, **kw)[0]
        independent = VolumeInference(cfg, sample_fn, blend='constant', noise='anchored', seed=J.SEED, **cons)(vol)
        joint = VolumeInference(cfg, vp_denoiser(imagen, sampler, eta), blend='constant', noise='anchored', joint=True, seed=J.SEED,
                                **cons)(vol)
        assert independent.unique().numel() > 1000
        assert torch.equal(joint, independent), mode


@pytest.mark.parametrize('op_name', CHAIN_OPERATORS)
@pytest.mark.parametrize('eta', list(E.ETAS))
def test_tile_edm_joint_at_stride_equal_patch_is_the_independent_path(eta, op_name):
    from diffusioniqt_amd.inference import VolumeInference
    eta = E.ETAS[eta]
    cell, A, op, _, _ = operator_of(op_name)
    for dynamic in (False, True):
        elu = HN.make_elucidated('churn-on', dynamic, self_cond=True, size=CHAIN_P).to(DEV)
        vol, cfg = cu(chain_volume()), chain_cfg(stride=CHAIN_P)
        cons = dict(consistency=(torch.from_numpy(chain_rows(op)), cell), consistency_weight=0.75, consistency_operator=op)

        def sample_fn(x, noise=None, **kw):
            assert set(kw) == {'consistency', 'consistency_weight', 'consistency_operator'}
            return elu.sample(batch_size=x.shape[0], video_frames=CHAIN_P, start_image_or_video=x, start_at_unet_number=2, noise=noise,
                              sampler='dpmpp2m', eta=eta, use_tqdm=False, **kw)
        independent = VolumeInference(cfg, sample_fn, blend='constant', noise='anchored', seed=E.SEED, **cons)(vol)
        joint = VolumeInference(cfg, elu.window_denoiser(sampler='dpmpp2m', eta=eta), blend='constant', noise='anchored', joint=True,
                                seed=E.SEED, **cons)(vol)
        assert independent.unique().numel() > 1000
        assert torch.equal(joint, independent), dynamic


# ---- G5: the guarantee -------------------------------------------------------------------------------------------------------------------------
def _whole_tiles(vol, cfg, cell):
    L = J.layout(vol, cfg)
    covered = R.blend_accumulate(np.zeros((1, L['kept'].shape[0], CHAIN_P, CHAIN_P, CHAIN_P)), L['slot'], np.ones(CHAIN_P), L['stride'],
                                 vol.shape)[2]
    whole = TR._cells(covered, cell).all(axis=(-5, -3, -1))
    assert 0 < whole.sum() < whole.size
    return whole


def _simulated_rows(op):
    """y = A x of a high-res volume of raw values in [100, 500], by ``ops.tile_measure``: it lies in the range of A (to rounding)."""
    from diffusioniqt_amd import ops
    hr = np.random.default_rng(9).uniform(100.0, 500.0, CHAIN_VOL).astype(np.float32)
    return ops.tile_measure(cu(hr), op).cpu().numpy(), float(np.abs(hr).max())


def _residual_A(x, rows, name, cfg, whole):
    """max |A x - y| over the fully covered tiles in float64, y z-scored (the rows of a stack operator sum to 1), and its bound."""
    cell, A, op, table, _ = operator_of(name)
    assert np.abs(A.sum(1) - 1).max() <= 1e-15
    mean, std = float(cfg['Data']['mean']), float(cfg['Data']['std'])
    want = (rows.astype(np.float64) - mean) / std
    err = np.abs(TR.measure64(x, cell, A) - want)[:, whole].max()
    scale = max(1.0, float(np.abs(x).max()), float(np.abs(want).max()))                   # 1: the clamped prediction
    return err, TR.residual_bound_A(cell, table, A, op.pinv.numpy(), float(np.abs(rows).max()), 500.0, std, scale)


@pytest.mark.parametrize('op_name', CHAIN_OPERATORS)
def test_final_state_reproduces_the_measurement(op_name):
    """The EDM family's DPM-Solver++ 2M ODE ends at sigma = 0 with (kx, k0) = (0, 1), no step clamp, w = 1: the state the chain ends
    in IS the projected x0, and A x recomputed in float64 is the measurement on every fully covered tile, within the derived bound of
    ONE step."""
    from diffusioniqt_amd.inference import VolumeInference
    cell, A, op, _, _ = operator_of(op_name)
    elu = HN.make_elucidated('churn-on', False, size=CHAIN_P).to(DEV)
    den = elu.window_denoiser(sampler='dpmpp2m', eta=0.0)
    assert den.clamp == (-float('inf'), float('inf'), 1) and den.coefs[-1].tolist() == [0.0, 1.0, 0.0, 0.0]
    vol, cfg = chain_volume(), chain_cfg()
    rows, _ = _simulated_rows(op)
    states = []
    den.finish = lambda x: states.append(x.clone()) or x                                  # the state the chain ends in, before any finish
    VolumeInference(cfg, den, blend='gaussian', noise='anchored', joint=True, seed=E.SEED, consistency=(torch.from_numpy(rows), cell),
                    consistency_operator=op)(cu(vol))
    x = states[0].cpu().numpy()
    whole = _whole_tiles(vol, cfg, cell)
    err, bound = _residual_A(x, rows, op_name, cfg, whole)
    print(f"guarantee EDM ODE {op_name}: max |A x - y| = {err:.3e} on {whole.sum()} of {whole.size} tiles, bound {bound:.3e}")
    assert err <= bound
    i, j, k = (int(v[0]) for v in whole.nonzero())
    null = x - TR.apply64(x, cell, operator_of(op_name)[3])
    assert np.abs(TR._cells(null, cell)[i, :, j, :, k, :]).max() > 1e-3                    # the null space of A is the network's


@pytest.mark.parametrize('op_name', CHAIN_OPERATORS)
def test_ddim_chain_ends_on_a_consistent_prediction(op_name, monkeypatch):
    """The deterministic ddim chain with no clamp and w = 1: the last corrected prediction x0' (``x0_out`` of the last fused launch)
    satisfies A x0' = y on every fully covered tile, within the derived bound of one step."""
    from diffusioniqt_amd import ops
    from diffusioniqt_amd.inference import VolumeInference
    cell, A, op, _, _ = operator_of(op_name)
    imagen = stub_imagen('x_start', 'dynamic', size=CHAIN_P)                              # dynamic: the step clamp is (-inf, inf)
    den = vp_denoiser(imagen, 'ddim', 0.0)
    assert den.clamp == (-float('inf'), float('inf'), 1)
    vol, cfg = chain_volume(), chain_cfg()
    rows, _ = _simulated_rows(op)
    real, calls = ops.volume_joint_consistent_tile_step, []

    def recording(*a, **kw):
        out, x0 = real(*a, **kw)
        calls.append(x0.clone())
        return out, x0
    monkeypatch.setattr(ops, 'volume_joint_consistent_tile_step', recording)
    VolumeInference(cfg, den, blend='gaussian', noise='anchored', joint=True, seed=J.SEED, consistency=(torch.from_numpy(rows), cell),
                    consistency_operator=op)(cu(vol))
    assert len(calls) == J.STEPS
    err, bound = _residual_A(calls[-1].cpu().numpy(), rows, op_name, cfg, _whole_tiles(vol, cfg, cell))
    print(f"ddim {op_name}: max |A x0' - y| = {err:.3e} (bound {bound:.3e})")
    assert err <= bound


@pytest.mark.parametrize('op_name', CHAIN_OPERATORS)
def test_contradicting_stacks_are_fitted_in_the_least_squares_sense(op_name):
    """Independent noise on every row: y is no longer in the range of A and A x = y cannot hold.  What holds at w = 1 is P x = t with
    t = A+ y, the least-squares fit -- tested on the final state of the EDM ODE chain with P and t as the device holds them."""
    from diffusioniqt_amd.inference import VolumeInference
    cell, A, op, table, _ = operator_of(op_name)
    elu = HN.make_elucidated('churn-on', False, size=CHAIN_P).to(DEV)
    den = elu.window_denoiser(sampler='dpmpp2m', eta=0.0)
    vol, cfg = chain_volume(), chain_cfg()
    rows, _ = _simulated_rows(op)
    rows = (rows + np.random.default_rng(10).normal(0.0, 20.0, rows.shape)).astype(np.float32)
    states = []
    den.finish = lambda x: states.append(x.clone()) or x
    VolumeInference(cfg, den, blend='gaussian', noise='anchored', joint=True, seed=E.SEED, consistency=(torch.from_numpy(rows), cell),
                    consistency_operator=op)(cu(vol))
    x = states[0].cpu().numpy()
    whole = TR.replicate(_whole_tiles(vol, cfg, cell), cell)
    target = TR.target_state(rows, cell, op.pinv.numpy(), cfg)
    err = np.abs(TR.apply64(x, cell, table) - target)[whole].max()
    scale = max(1.0, float(np.abs(x).max()), float(np.abs(target).max()))
    bound = TR.residual_bound_P(cell, table, op.pinv.numpy(), float(np.abs(rows).max()), float(cfg['Data']['std']), scale)
    mean, std = float(cfg['Data']['mean']), float(cfg['Data']['std'])
    off = np.abs(TR.measure64(x, cell, A) - (rows.astype(np.float64) - mean) / std)[:, whole[::cell[0], ::cell[1], ::cell[2]]].max()
    print(f"contradicting stacks {op_name}: max |P x - t| = {err:.3e} (bound {bound:.3e}); |A x - y| = {off:.3e}")
    assert err <= bound and off > 100 * bound                                              # A x = y is not what holds here


# ---- G6: a one-row operator against the ``consistency=`` path --------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['ddim-eta0.5', 'dpmpp2m'])
def test_a_one_row_operator_is_the_uniform_chain_within_the_bound(name):
    """The operator of ONE stack along z, tile (4, 1, 1), is the uniform cell mean: P = 1 / n exactly and t = the replicated
    measurement, so its float64 chain is the ``consistency=`` chain.  The arithmetic differs -- n products with 1 / n inside the sum
    where ``cell_mean`` adds and divides once -- so what is promised is agreement within the two chains' derived bounds, NOT bit for
    bit.  (The count of differing voxels is printed, not asserted: with n = 4 every product with 1 / n is exact, and on the MI355X
    these inputs came out equal in every bit.)"""
    from diffusioniqt_amd.inference import VolumeInference
    from tests.test_gpu_volume_dc import vp_reference as uniform_reference
    imagen = stub_imagen('x_start', 'clamp-min', size=CHAIN_P)
    cell, A, op, table, _ = operator_of('stack-411')
    vol, cfg, w = chain_volume(), chain_cfg(), 1.0
    meas = DC.measurement(vol, cell)
    ref = cached(('vp-one-row', name), lambda: vp_reference(imagen, name, 'stack-411', w, vol, cfg, 'gaussian', rows=meas[None]))
    old = cached(('vp-uniform', name), lambda: uniform_reference(imagen, name, cell, w, vol, cfg, 'gaussian'))
    assert np.abs(ref['mean'] - old['mean']).max() <= 1e-12                                  # one float64 chain
    common = dict(blend='gaussian', noise='anchored', joint=True, seed=J.SEED, consistency_weight=w)
    got = check(VolumeInference(cfg, vp_denoiser(imagen, *VP[name]), consistency=(torch.from_numpy(meas[None]), cell),
                                consistency_operator=op, **common)(cu(vol)), ref, f"one-row operator, {name}")
    none = VolumeInference(cfg, vp_denoiser(imagen, *VP[name]), consistency=(torch.from_numpy(meas), cell), **common)(cu(vol)).cpu().numpy()
    diff = np.abs(got.astype(np.float64) - none).max()
    print(f"one-row operator vs consistency= alone, {name}: max difference {diff:.3e}, bounds {ref['bound']:.3e} + {old['bound']:.3e}; "
          f"{(bits(got) != bits(none)).sum()} of {got.size} voxels differ in bits")
    assert diff <= ref['bound'] + old['bound']
