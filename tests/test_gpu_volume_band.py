"""Data consistency for a k-space band limit on a real MI355X against tests/volume_joint_band_reference.py: ``ops.band_measure`` /
``ops.band_backproject`` / ``ops.band_project`` and the three calls of the joint step bit for bit against the fp32 restatement (no voxel
is left out of a comparison), the joint chains of both families through ``VolumeInference(consistency_band=...)`` against the float64
chains, the bit-for-bit tie of the joint chain on a volume of one window to ``sample(consistency=..., consistency_band=...)``, and the
argument errors of the ops.

Bounds: the reference's docstring.  The chain tests take the family's ``chain_bound`` plus ``steps`` times ``allowance``, the rounding
allowance of one projection, of which the fp32 restatement uses at most a tenth on the inputs of these tests
(tests/test_volume_band_host.py).

The blocking constants of ``band_pass_kernel`` (csrc/datapath.hip) and the shapes on both sides of each: BAND_C = 64 columns per block
(8^3 cubes: 64 columns of a cube's z pass, 3 x 8 = 24 lines of its x pass; the volumes: 1260 and 360); BAND_I = 32 outputs per block and
BAND_R = 8 per thread (N = 8, 16 at the register block, 10, 12, 18, 20 off it and below 32, 70 and 132 above); BAND_J = 64 values of j
per panel (N = 70: a second panel of 6; 132: a third of 4); BAND_PAD = 64 floats of table padding (N below and above it);
BAND_MAX_N = 512, the largest axis (``test_band_ops_at_the_largest_axis``)."""
import math

import numpy as np
import pytest
import torch

from tests import dpmpp2m_reference as M
from tests import edm_dpmpp2m_reference as E
from tests import volume_blend_reference as R
from tests import volume_joint_band_reference as BD
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


def table_of(shape, cell, band, off):
    """(the reference's axes, its fp32 tables, the op's table on the device); the same bits (tests/test_volume_band_host.py)."""
    from diffusioniqt_amd import ops
    host = ops.band_table(shape, cell, band, off)
    axes = BD.axes_of(shape, cell, band, off)
    tabs, flat = BD.tables32(axes)
    assert np.array_equal(bits(host.table), bits(flat))
    return axes, tabs, host.to(DEV)


def project_case(case):
    """The per-window inputs: x0, the high-res truth per cube, its fp32 measurement y and the target t = A+ y."""
    def make():
        cell, P, band, off = BD.PROJECT_CASES[case]
        axes = BD.axes_of((P, P, P), cell, band, off)
        tabs, _ = BD.tables32(axes)
        x0, truth = BD.project_inputs(P)
        y = BD.measure32(truth, axes, tabs)
        return dict(x0=x0, truth=truth, y=y, t=BD.backproject32(y, axes, tabs))
    return cached(('project-case', case), make)


# ---- G1: the operator and the per-window projection, bit for bit --------------------------------------------------------------------------
@pytest.mark.parametrize('case', range(len(BD.PROJECT_CASES)))
def test_band_measure_and_backproject_are_the_reference_bit_for_bit(case):
    from diffusioniqt_amd import ops
    cell, P, band, off = BD.PROJECT_CASES[case]
    axes, tabs, dev = table_of((P, P, P), cell, band, off)
    c = project_case(case)
    rows = tuple(P // f for f in cell)
    ws = torch.empty(2 * P ** 3, device=DEV)
    for b in range(3):
        y = ops.band_measure(cu(c['truth'][b, 0]), dev, workspace=ws if b else None)
        assert tuple(y.shape) == rows and np.array_equal(bits(y), bits(c['y'][b, 0]))
        t = ops.band_backproject(y, dev, workspace=ws if b else None)
        assert tuple(t.shape) == (P, P, P) and np.array_equal(bits(t), bits(c['t'][b, 0]))
    assert np.abs(c['y'] - BD.measure64(c['truth'], axes)).max() <= 64 * 2.0 ** -24 * np.abs(c['truth']).max()


@pytest.mark.parametrize('w', [1.0, 0.5])
@pytest.mark.parametrize('clamp', list(CLAMPS))
@pytest.mark.parametrize('case', range(len(BD.PROJECT_CASES)))
def test_band_project_is_the_reference_bit_for_bit(case, clamp, w):
    """B C = 3 cubes; fresh output and in place (``out`` aliasing ``x0``), with the workspace made by the op and given."""
    from diffusioniqt_amd import ops
    cell, P, band, off = BD.PROJECT_CASES[case]
    axes, tabs, dev = table_of((P, P, P), cell, band, off)
    c = project_case(case)
    cl = CLAMPS[clamp]
    a = DC.clamp32(*(cl or (0., 0., None)))(c['x0'])
    want = cached(('project', case, clamp, w), lambda: BD.project32(a, c['t'], axes, tabs, w))
    x, t = cu(c['x0']), cu(c['t'])
    got = ops.band_project(x, t, cell, dev, w, clamp=cl)
    assert got.data_ptr() != x.data_ptr() and torch.equal(x, cu(c['x0'])) and torch.equal(t, cu(c['t']))
    bad = (bits(got) != bits(want)).sum()
    print(f"band_project {cell} P {P} active {dev.active} clamp {clamp} w {w}: {bad} of {want.size} voxels differ")
    assert bad == 0
    same = ops.band_project(x, t, cell, dev, w, clamp=cl, out=x, workspace=torch.empty(2 * x.numel(), device=DEV))
    assert same.data_ptr() == x.data_ptr() and torch.equal(x, got)
    assert (bits(got) != bits(a)).mean() > 0.9
    if w == 1.0 and cl is None:                                # what it is for: A x0' = y (the measurement behind the target)
        allow = BD.allowance(axes, tabs, float(np.abs(c['t'] - a).max()), float(np.abs(want).max()))
        err = np.abs(BD.measure64(got.cpu().numpy(), axes) - BD.measure64(c['t'], axes)).max()
        assert err <= allow


def test_band_ops_at_the_largest_axis():
    """N = BAND_MAX_N = 512 along z (eight j-panels, sixteen output tiles), A, A+ and P, bit for bit."""
    from diffusioniqt_amd import ops
    shape, cell = (512, 4, 4), (4, 1, 2)
    axes, tabs, dev = table_of(shape, cell, ([1.0, 0.5] + [1.0] * 40, None, None), 'centre')
    x = np.random.default_rng(5).standard_normal(shape).astype(np.float32)
    y = ops.band_measure(cu(x), dev)
    assert np.array_equal(bits(y), bits(BD.measure32(x, axes, tabs)))
    assert np.array_equal(bits(ops.band_backproject(y, dev)), bits(BD.backproject32(y.cpu().numpy(), axes, tabs)))
    out, ws = torch.empty(shape, device=DEV), torch.empty(shape, device=DEV)
    assert np.array_equal(bits(ops.band_apply(cu(x), dev, out, ws)), bits(BD.apply32(x, axes, tabs)))


def test_band_ops_argument_errors():
    from diffusioniqt_amd import ops
    x = torch.zeros(2, 1, 8, 8, 8, device=DEV)
    _, _, table = table_of((8, 8, 8), (2, 2, 2), None, None)
    with pytest.raises(ValueError, match="consistency cell"):
        ops.band_project(x, x.clone(), (3, 1, 1), table)
    with pytest.raises(ValueError, match="consistency weight"):
        ops.band_project(x, x.clone(), (2, 2, 2), table, 0.0)
    with pytest.raises(ValueError, match="consistency_band table"):
        ops.band_project(x, x.clone(), (2, 2, 1), table)                                   # made for another cell
    with pytest.raises(ValueError, match="consistency_band table"):
        ops.band_project(x, x.clone(), (2, 2, 2), table.table)                             # the bare tensor
    with pytest.raises(ValueError, match="consistency_band table"):
        ops.band_project(x, x.clone(), (2, 2, 2), ops.band_table((8, 8, 8), (2, 2, 2)))    # on the host
    with pytest.raises(ValueError, match="consistency_band table"):
        ops.band_project(x, x.clone(), (2, 2, 2), ops.band_table((16, 16, 16), (2, 2, 2)).to(DEV))     # another domain
    with pytest.raises(ValueError, match="consistency_band workspace"):
        ops.band_project(x, x.clone(), (2, 2, 2), table, workspace=torch.empty(2 * x.numel() - 1, device=DEV))
    with pytest.raises(ValueError, match="clamp mode"):
        ops.band_project(x, x.clone(), (2, 2, 2), table, clamp=(-1., 1., 2))
    with pytest.raises(ValueError, match="target"):
        ops.band_project(x, x[:1].clone(), (2, 2, 2), table)
    with pytest.raises(ValueError, match="consistency_band table"):
        ops.band_measure(x[0, 0], table.table)
    with pytest.raises(ValueError, match="consistency_band domain"):
        ops.band_measure(torch.zeros(8, 8, 4, device=DEV), table)
    with pytest.raises(ValueError, match="consistency_band domain"):
        ops.band_backproject(x[0, 0], table)                                              # the high-res shape where the rows belong
    with pytest.raises(RuntimeError):
        ops.band_measure(x[0, 0].cpu(), table)
    v = x[0, 0]
    with pytest.raises(ValueError, match="three different volumes"):
        ops.band_apply(v, table, v, torch.empty_like(v))
    with pytest.raises(ValueError, match="consistency_band workspace"):
        ops.volume_joint_consistent_band_step(torch.zeros(1, 8, 8, 8, device=DEV), torch.zeros(1, 1, 1, dtype=torch.int32, device=DEV),
                                              torch.ones(8, device=DEV), v, None, (2, 2, 2), table, torch.empty(4, 8, 8, 8, device=DEV), 1.0,
                                              0, KX, K0, 0.0, 0.0, -1.0, 1.0, 1, 8)


# ---- G2: the three calls of the joint step, bit for bit ------------------------------------------------------------------------------------
def _step_refs(name):
    """The case and the fused x0 per clamp (the walk does not depend on the cell)."""
    def make():
        c = BD.step_case(name)
        c['fused'] = {k: DC.fuse32(c['y'], c['slot'], c['taps'], c['stride'], c['vol'], DC.clamp32(*cl))
                      for k, cl in (('min', CLAMPS['min']), ('box', CLAMPS['box']))}
        return c
    return cached(('step', name), make)


def _normals(vol, draw):
    from diffusioniqt_amd import ops
    return cached(('n', vol, draw), lambda: ops.volume_joint_init(vol, SEED, sample=SAMPLE, draw=draw).cpu().numpy())


FORMS = {'step-kn0': (0, False, 0.0), 'step-kn': (0, False, 0.625), 'multistep-noprev': (1, False, 0.0), 'multistep-prev': (1, True, 0.0),
         'sde-prev-kn': (2, True, 0.625)}


@pytest.mark.parametrize('form', list(FORMS))
@pytest.mark.parametrize('name,cell', BD.STEP_CASES)
def test_joint_band_step_is_the_reference_bit_for_bit(name, cell, form):
    """Every voxel is compared: nothing is excluded.  The residual volumes, c = P r, then the fresh step launch, then the same launch
    in place (``x_next`` aliasing ``x_t`` and, where there is a history, ``x0_out`` aliasing ``x0_prev``).  The volumes have dropped
    windows: an uncovered voxel has residual 0, keeps x_t and reports x0 = 0."""
    from diffusioniqt_amd import ops
    c = _step_refs(name)
    vol, stride = c['vol'], c['stride']
    f, with_prev, kn = FORMS[form]
    clamp = 'min' if cell[2] != 1 else 'box'
    w, draw = (1.0, 5) if sum(cell) % 2 else (0.5, 3)
    band, off = BD.STEP_CELLS[cell]
    axes, tabs, dev = table_of(vol, cell, band, off)
    t = cached(('t', name, cell), lambda: BD.backproject32(BD.measure32(c['truth'], axes, tabs), axes, tabs))
    n = _normals(vol, draw) if kn != 0 else None
    a, covered = c['fused'][clamp]
    r = np.where(covered, t - a, np.float32(0)).astype(np.float32)
    pr = cached(('Pr', name, cell, clamp), lambda: BD.apply32(r, axes, tabs))
    want, want0 = BD.joint_step32(c['fused'][clamp], c['x'], c['prev'] if with_prev else None, t, axes, tabs, w, f, KX, K0, KP, kn, n)
    assert (~covered).any() and covered.any()
    args = (cu(c['y']), cu(c['slot'].astype(np.int32)), cu(c['taps']))
    ws = ops.band_workspace(vol, DEV)
    cl = CLAMPS[clamp]
    assert ops.volume_joint_band_residual(*args, cu(t), dev, ws, *cl, stride) is ws
    assert np.array_equal(bits(ws[0]), bits(a)) and np.array_equal(ws[1].cpu().numpy() != 0, covered) and np.array_equal(bits(ws[2]), bits(r))
    assert ops.band_apply(ws[2], dev, ws[3], ws[4]).data_ptr() == ws[3].data_ptr()
    bad_c = (bits(ws[3]) != bits(pr)).sum()
    tail = (cell, dev, ws, w, f, KX, K0, KP, kn, *cl, stride, SEED, draw, SAMPLE)
    x, prev = cu(c['x']), cu(c['prev']) if with_prev else None
    got, got0 = ops.volume_joint_consistent_band_step(*args, x, prev, *tail)
    assert got.data_ptr() != x.data_ptr() and torch.equal(x, cu(c['x']))
    bad, bad0 = (bits(got) != bits(want)).sum(), (bits(got0) != bits(want0)).sum()
    print(f"band step {form} {name} cell {cell} active {dev.active} w {w}: {bad_c} / {bad} / {bad0} of {want.size} voxels differ")
    assert bad_c == 0 and bad == 0 and bad0 == 0
    assert np.array_equal(bits(got)[~covered], bits(c['x'])[~covered]) and not got0.cpu().numpy()[~covered].any()
    ops.volume_joint_consistent_band_step(*args, x, prev, *tail, out=x, x0_out=prev)
    assert torch.equal(x, got) and (prev is None or torch.equal(prev, got0))


# ---- G3: the chains through VolumeInference against the float64 reference ----------------------------------------------------------------------
CHAIN_VOL, CHAIN_P, CHAIN_STRIDE = (16, 16, 24), 8, 4
CHAIN_BANDS = {(2, 2, 2): ([1.0, 0.75, 0.5], None, [1.0, 1.0, 0.0, 0.5], 'centre'), (4, 1, 1): (None, None, None)}


def chain_volume():
    vol = np.random.default_rng(7).integers(1, 1000, CHAIN_VOL).astype(np.float32)
    vol[:8, :8, :12] = 0                                       # the 5 % rule drops two windows: 4 x 4 x 8 voxels are covered by none
    return vol


def chain_cfg(stride=CHAIN_STRIDE, batch_size=7):
    return R.shared_cfg(stride, batch_size=batch_size, P=CHAIN_P)


def chain_axes(cell, shape=CHAIN_VOL):
    band = CHAIN_BANDS[cell]
    axes = BD.axes_of(shape, cell, band[:3], *band[3:])
    return axes, BD.tables32(axes)[0]


VP = {'ddim-eta0': ('ddim', 0.0), 'ddim-eta0.5': ('ddim', 0.5), 'ddpm': ('ddpm', 0.0), 'dpmpp2m': ('dpmpp2m', 0.0)}


def vp_denoiser(imagen, sampler, eta):
    return imagen.window_denoiser(sampler=sampler, sample_steps=J.STEPS, eta=eta)


def vp_reference(imagen, name, cell, w, vol, cfg, blend):
    sampler, eta = VP[name]
    sched = imagen.noise_schedulers[1]
    coefs = vp_denoiser(imagen, sampler, eta).coefs.numpy().astype(np.float64)             # the chain's host numbers, widened
    log_snr = J.tables(sched, J.STEPS, 0.0, 'x_start')[2]
    axes, tabs = chain_axes(cell)
    meas = DC.measurement(vol, cell)
    t = BD.target_state(meas, axes, cfg)
    with BD.band_chains(axes):
        x, L, x0_max, _ = DC.vp_chain(vol, cfg, coefs, log_snr, (J.MIN_BOUND, 0., 0), blend, t, cell, w, multistep=sampler == 'dpmpp2m',
                                      seed=J.SEED, sample=0)
    ref = DC.finish(vol, cfg, [np.maximum(x, J.MIN_BOUND)], L)
    if sampler == 'dpmpp2m':
        t64, k01 = M.table64(*M.chain_log_snr(sched, J.STEPS))
        bound = M.chain_bound(ref['windows_per_voxel'], ref['scale'], M.amplification(t64, k01))
    else:
        bound = J.chain_bound(ref['windows_per_voxel'], ref['scale'])
    ref.update(bound=bound + J.STEPS * BD.allowance(axes, tabs, x0_max + float(np.abs(t).max()), x0_max), meas=meas)
    return ref


def check(got, ref, what, key='mean', factor=1):
    got = got.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == ref[key].shape and np.isfinite(got).all()
    err = np.abs(got.astype(np.float64) - ref[key]).max()
    print(f"{what}: max |{key} - ref| = {err:.3e}, bound {factor * ref['bound']:.3e}")
    assert err <= factor * ref['bound'], what
    return got


@pytest.mark.parametrize('cell', list(CHAIN_BANDS))
@pytest.mark.parametrize('name', list(VP))
def test_band_joint_chain_matches_the_float64_reference(name, cell):
    from diffusioniqt_amd.inference import VolumeInference
    imagen = stub_imagen('x_start', 'clamp-min', size=CHAIN_P)
    vol, cfg, w = chain_volume(), chain_cfg(), 1.0 if cell == (2, 2, 2) else 0.5
    ref = cached(('vp', name, cell), lambda: vp_reference(imagen, name, cell, w, vol, cfg, 'gaussian'))
    common = dict(blend='gaussian', noise='anchored', joint=True, seed=J.SEED, consistency=(torch.from_numpy(ref['meas']), cell),
                  consistency_weight=w)
    inf = VolumeInference(cfg, vp_denoiser(imagen, *VP[name]), consistency_band=CHAIN_BANDS[cell], **common)
    got = check(inf(cu(vol)), ref, f"band joint {name} cell {cell} w {w}")
    uniform = cached(('vp-none', name, cell), lambda: VolumeInference(cfg, vp_denoiser(imagen, *VP[name]), **common)(cu(vol)).cpu().numpy())
    live = ref['covered'] & ~ref['background']
    assert (~ref['covered']).any() and np.abs(got - uniform)[live].max() > 0.01            # not the cell-mean chain


@pytest.mark.parametrize('cell', list(CHAIN_BANDS))
@pytest.mark.parametrize('eta', list(E.ETAS))
def test_band_edm_joint_chain_matches_the_float64_reference(eta, cell):
    from diffusioniqt_amd.inference import VolumeInference
    eta = E.ETAS[eta]
    elu = HN.make_elucidated('churn-on', False, size=CHAIN_P).to(DEV)
    den = elu.window_denoiser(sampler='dpmpp2m', eta=eta)
    vol, cfg = chain_volume(), chain_cfg()
    meas = DC.measurement(vol, cell)
    axes, tabs = chain_axes(cell)

    def make():
        edm = E.tables(HN.HP, eta, coefs=den.coefs.numpy())
        t = BD.target_state(meas, axes, cfg)
        with BD.band_chains(axes):
            x, L, state_max, x0_max, _ = DC.edm_chain(vol, cfg, edm, 'gaussian', False, t, cell, 1.0)
        ref = DC.finish(vol, cfg, [np.clip(x, -1.0, 1.0)], L)
        mean32, std32 = np.float32(cfg['Data']['mean']), np.float32(cfg['Data']['std'])
        lowres_max = edm['lowres'][0] * float(np.abs((vol - mean32) / std32).max()) + 6 * edm['lowres'][1]
        # the family's bound is a recursion with a local term of (windows + 3) 2^-23 per step at |D| <= 1: the allowance of one
        # projection enters as that many further such terms, as ``volume_joint_dc_reference.edm_bound`` has it for the cell mean
        extra = math.ceil(BD.allowance(axes, tabs, x0_max + float(np.abs(t).max()), x0_max) / 2.0 ** -23)
        ref['bound'] = E.chain_bound(edm, L['windows_per_voxel'] + extra, state_max, lowres_max, False, False)
        return ref
    ref = cached(('edm', eta, cell), make)
    inf = VolumeInference(cfg, den, blend='gaussian', noise='anchored', joint=True, seed=E.SEED, consistency=(torch.from_numpy(meas), cell),
                          consistency_band=CHAIN_BANDS[cell])
    check(inf(cu(vol)), ref, f"band joint EDM dpmpp2m eta {eta} cell {cell}")


# ---- G4: a volume of one window: the joint chain is the per-window sampler ----------------------------------------------------------------------
# P = 8: n = 4 keeps k <= 1 at fz = 2, n = 2 only the mean at fz = 4
TIE_BANDS = {(2, 2, 2): ([1.0, 0.5], None, None, 'centre'), (4, 1, 1): (None, None, None)}


def one_window_volume():
    return np.random.default_rng(9).integers(1, 1000, (CHAIN_P,) * 3).astype(np.float32)


def one_window_target(inf, meas, cell):
    """The target of the window as ``VolumeInference`` makes it for the joint chain: t = A+ y on the device, z-scored."""
    from diffusioniqt_amd import ops
    band = TIE_BANDS[cell]
    table = ops.band_table((CHAIN_P,) * 3, cell, band[:3], *band[3:]).to(DEV)
    return ((ops.band_backproject(cu(meas), table) - inf.mean) / inf.std).contiguous()[None, None]


@pytest.mark.parametrize('cell', list(TIE_BANDS))
@pytest.mark.parametrize('name', ['ddim-eta0.5', 'ddpm', 'dpmpp2m'])
def test_band_joint_on_one_window_is_the_sampler_call(name, cell):
    """D = H = W = P, unit weights: num / den is exact and the periodic domain of the joint path is the sampler's cube, so both paths
    take the same ``__device__`` arithmetic and update -- equal at every voxel, bit for bit.  The window-by-window modes do not take
    the keyword, so the independent side hands ``consistency=(t, cell)`` and ``consistency_band=`` to ``sample`` itself."""
    from diffusioniqt_amd.inference import VolumeInference
    sampler, eta = VP[name]
    for mode in ('clamp-min', 'dynamic'):
        imagen = stub_imagen('x_start', mode, size=CHAIN_P)
        vol, cfg = cu(one_window_volume()), chain_cfg(stride=CHAIN_P)
        meas = DC.measurement(one_window_volume(), cell)
        cons = dict(consistency=(torch.from_numpy(meas), cell), consistency_weight=0.75)
        jv = VolumeInference(cfg, vp_denoiser(imagen, sampler, eta), blend='constant', noise='anchored', joint=True, seed=J.SEED,
                             consistency_band=TIE_BANDS[cell], **cons)
        joint = jv(vol)
        t = one_window_target(jv, meas, cell)

        def sample_fn(x, noise=None):
            return imagen.sample(batch_size=x.shape[0], start_image_or_video=x, start_at_unet_number=2, use_tqdm=False, sampler=sampler,
                                 sample_steps=J.STEPS, eta=eta, noise=noise, consistency=(t, cell), consistency_weight=0.75,
                                 consistency_band=TIE_BANDS[cell])[0]
        independent = VolumeInference(cfg, sample_fn, blend='constant', noise='anchored', seed=J.SEED)(vol)
        plain = VolumeInference(cfg, vp_denoiser(imagen, sampler, eta), blend='constant', noise='anchored', joint=True, seed=J.SEED,
                                **cons)(vol)
        assert independent.unique().numel() > 100 and not torch.equal(joint, plain)
        assert torch.equal(joint, independent), mode


@pytest.mark.parametrize('cell', list(TIE_BANDS))
@pytest.mark.parametrize('eta', list(E.ETAS))
def test_band_edm_joint_on_one_window_is_the_sampler_call(eta, cell):
    from diffusioniqt_amd.inference import VolumeInference
    eta = E.ETAS[eta]
    for dynamic in (False, True):
        elu = HN.make_elucidated('churn-on', dynamic, self_cond=True, size=CHAIN_P).to(DEV)
        vol, cfg = cu(one_window_volume()), chain_cfg(stride=CHAIN_P)
        meas = DC.measurement(one_window_volume(), cell)
        jv = VolumeInference(cfg, elu.window_denoiser(sampler='dpmpp2m', eta=eta), blend='constant', noise='anchored', joint=True,
                             seed=E.SEED, consistency=(torch.from_numpy(meas), cell), consistency_weight=0.75,
                             consistency_band=TIE_BANDS[cell])
        joint = jv(vol)

        def sample_fn(x, noise=None):
            return elu.sample(batch_size=x.shape[0], video_frames=CHAIN_P, start_image_or_video=x, start_at_unet_number=2, noise=noise,
                              sampler='dpmpp2m', eta=eta, use_tqdm=False, consistency=(one_window_target(jv, meas, cell), cell),
                              consistency_weight=0.75, consistency_band=TIE_BANDS[cell])
        independent = VolumeInference(cfg, sample_fn, blend='constant', noise='anchored', seed=E.SEED)(vol)
        assert independent.unique().numel() > 100
        assert torch.equal(joint, independent), dynamic
