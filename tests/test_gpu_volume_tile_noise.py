"""Noise-aware data consistency for a tile operator (``consistency_row_noise=``) on a real MI355X against
tests/volume_joint_tile_noise_reference.py: ``ops.tile_project_noise`` and the fused joint step bit for bit against the fp32
restatement (no voxel is left out of a comparison), the joint chains of both families through
``VolumeInference(joint=True, consistency_row_noise=...)`` against the float64 chains, and the bit-for-bit tie of the joint chain at
stride = patch to blend mode calling ``sample(consistency_row_noise=...)`` per window.  The shapes are those of
tests/test_gpu_volume_tile.py.

Bounds: the reference module's docstring.  A chain test takes the family's ``chain_bound`` plus, per step, the projection's rounding
count (2 (n + 1) G_M + 1) 2^-24 S plus kn times the shaping's ((n + 1) G_G + 1) 2^-24 E.  Observed on the MI355X: the figures each
test prints, recorded in DESIGN 4.15."""

import numpy as np
import pytest
import torch

from tests import anchored_noise_reference as A
from tests import edm_dpmpp2m_reference as E
from tests import volume_joint_dc_reference as DC
from tests import volume_joint_heun_reference as HN
from tests import volume_joint_reference as J
from tests import volume_joint_tile_noise_reference as TN
from tests.test_gpu_volume_joint import stub_imagen
from tests.test_gpu_volume_tile import (BIG_VOL, CHAIN_P, CLAMPS, K0, KP, KX, SAMPLE, SEED, _step_refs, bits, cached, chain_cfg, chain_rows,
                                        chain_volume, cu, vp_denoiser)

pytestmark = pytest.mark.gpu
DEV = "cuda"
KN = 0.625
# rows (kx, k0, kp, kn) of a short stochastic chain with sigma_min = 0.1.  The step whose tables a launch test takes: row 2 leaves the
# badly measured directions below the cap -- mixed lambda, and shrink = 1 exactly there (an uncapped direction has a = b) -- row 1 caps
# (nearly) every direction at the weight with fractional shrinks
ROWS = np.array([[0.9, 0.3, 0.0, 0.5], [0.8, 0.4, 0.0, 0.3], [0.6, 0.5, 0.0, 0.1], [0.0, 1.0, 0.0, 0.0]])
SETS = {'mixed': 2, 'capped': 1}


def noise_operator(name):
    """(cell, the operator, its tables [T, 2, n, n] as numpy and on the device, the schedule), made once per name."""
    def make():
        from diffusioniqt_amd import ops
        cell, A_, sigma = TN.case_of(name)
        op = ops.tile_noise_operator(cell, A_, (sigma * 2).tolist())                        # sigma_min = 0.1
        sched = ops.tile_noise_schedule(op, ROWS, 0.1, 1.0)
        tables, kinds = ops.tile_noise_tables(op, sched)
        assert [k for k, _ in kinds] == ['noise'] * 3 + ['plain']
        return cell, op, tables.numpy(), tables.to(DEV), sched.numpy()
    return cached(('noise-op', name), make)


def test_the_table_sets_are_what_their_names_say():
    for name in ('stacks-222', 'stacks-421', 'stacks-135', 'dense-232', 'stacks-444'):
        sched = noise_operator(name)[4]
        lam, shrink = sched[SETS['mixed'], :, 0], sched[SETS['mixed'], :, 1]
        assert lam.max() > 1.5 * lam.min() > 0 and (shrink > 0).all()                       # one shaped row with mixed lambda
        assert shrink.max() >= 1 - 1e-7 and shrink.min() < 0.7                             # and shrink = 1 somewhere, not everywhere
        capped = sched[SETS['capped']]
        assert (capped[:, 0] == 1).mean() >= 0.5 and ((capped[:, 1] > 0) & (capped[:, 1] < 1)).mean() >= 0.5
    one = noise_operator('stack-411')[4]                                                   # the one-row operator: one direction
    assert one[SETS['mixed'], 0, 1] >= 1 - 1e-7 and 0 < one[SETS['capped'], 0, 1] < 1


# ---- G1: the per-window launch, bit for bit ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('which', list(SETS))
@pytest.mark.parametrize('clamp', list(CLAMPS))
@pytest.mark.parametrize('name', ['stacks-222', 'stacks-421', 'stack-411'])
def test_tile_project_noise_is_the_reference_bit_for_bit(name, clamp, which):
    """B C = 3 cubes of edge 8.  Fresh outputs (the inputs keep their bits), then in place on both pairs.  Every voxel is compared."""
    from diffusioniqt_amd import ops
    cell, op, tables, dev, _ = noise_operator(name)
    i = SETS[which]
    rng = np.random.default_rng(5)
    x0 = (rng.standard_normal((3, 1, 8, 8, 8)) * 2).astype(np.float32)
    target = rng.standard_normal((3, 1, 8, 8, 8)).astype(np.float32)
    eps = rng.standard_normal((3, 1, 8, 8, 8)).astype(np.float32)
    c = CLAMPS[clamp]
    want, want_n = TN.tile_project_noise32(x0, target, eps, cell, tables[i], c)
    x, t, n = cu(x0), cu(target), cu(eps)
    got, got_n = ops.tile_project_noise(x, t, n, cell, dev[i], clamp=c)
    assert len({v.data_ptr() for v in (x, n, got, got_n)}) == 4 and torch.equal(x, cu(x0)) and torch.equal(n, cu(eps))
    bad, bad_n = (bits(got) != bits(want)).sum(), (bits(got_n) != bits(want_n)).sum()
    print(f"tile_project_noise {name} {clamp} {which}: {bad} / {bad_n} of {want.size} voxels differ")
    assert bad == 0 and bad_n == 0
    assert (bits(got_n) != bits(eps)).mean() > 0.9 and (bits(got) != bits(x0)).mean() > 0.9
    same, same_n = ops.tile_project_noise(x, t, n, cell, dev[i], clamp=c, out=x, out_noise=n)
    assert same.data_ptr() == x.data_ptr() and same_n.data_ptr() == n.data_ptr()
    assert np.array_equal(bits(x), bits(want)) and np.array_equal(bits(n), bits(want_n))


def test_tile_project_noise_argument_errors():
    from diffusioniqt_amd import ops
    x = torch.zeros(2, 1, 8, 8, 8, device=DEV)
    cell, _, _, dev, _ = noise_operator('stacks-222')
    with pytest.raises(ValueError, match="consistency cell"):
        ops.tile_project_noise(x, x.clone(), x.clone(), (3, 1, 1), dev[0])
    with pytest.raises(ValueError, match="consistency_row_noise tables"):
        ops.tile_project_noise(x, x.clone(), x.clone(), (4, 1, 1), dev[0])                  # [2, 8, 8] is not [2, 4, 4]
    with pytest.raises(ValueError, match="consistency_row_noise tables"):
        ops.tile_project_noise(x, x.clone(), x.clone(), cell, dev[0].cpu())
    with pytest.raises(ValueError, match="noise must have"):
        ops.tile_project_noise(x, x.clone(), x[:1].clone(), cell, dev[0])
    with pytest.raises(ValueError, match="alias"):
        ops.tile_project_noise(x, x.clone(), x.clone(), cell, dev[0], out_noise=x)
    with pytest.raises(ValueError, match="clamp mode"):
        ops.tile_project_noise(x, x.clone(), x.clone(), cell, dev[0], clamp=(-1., 1., 2))


# ---- G2: the fused joint step, bit for bit -------------------------------------------------------------------------------------------------
def _normals(draw, shape):
    """The step's fp32 normals as the device draws them, checked against the float64 field of tests/anchored_noise_reference.py."""
    from diffusioniqt_amd import ops

    def make():
        n = ops.volume_joint_init(shape, SEED, sample=SAMPLE, draw=draw).cpu().numpy()
        want = A.normals(A.field(shape, 1, SEED, draw, SAMPLE))[0]
        assert np.abs(n - want).max() <= HN.EPS_N == 5e-6
        return n
    return cached(('row-n', draw, shape), make)


def _check_step(c, stride, name, form, which, shape):
    from diffusioniqt_amd import ops
    cell, op, tables, dev, _ = noise_operator(name)
    i = SETS[which]
    with_prev = form == 2
    clamp = 'min' if cell[2] != 1 else 'box'
    draw = 5 if sum(cell) % 2 else 3
    target, n = c['coarse'], _normals(draw, shape)               # any volume: t need not be constant over a tile
    want, want0, covered, shaped = TN.joint_step_tile_noise32(c['y'], c['slot'], c['taps'], stride, c['x'], c['prev'] if with_prev else None,
                                                              target, cell, tables[i], form, KX, K0, KP, KN, None, n,
                                                              fused=c['fused'][clamp])
    whole = TN.replicate(TN._cells(covered, cell).all(axis=(-5, -3, -1)), cell)
    assert whole.any() and (~covered).any() and (covered[:8, :8, :8] == False).any()             # uncovered voxels inside the volume too
    args = (cu(c['y']), cu(c['slot'].astype(np.int32)), cu(c['taps']))
    tail = (cu(target), cell, dev[i], form, KX, K0, KP, KN, *CLAMPS[clamp], stride, SEED, draw, SAMPLE)
    x, prev = cu(c['x']), cu(c['prev']) if with_prev else None
    got, got0 = ops.volume_joint_consistent_tile_noise_step(*args, x, prev, *tail)
    assert got.data_ptr() != x.data_ptr() and torch.equal(x, cu(c['x']))
    bad, bad0 = (bits(got) != bits(want)).sum(), (bits(got0) != bits(want0)).sum()
    print(f"tile noise step form {form} stride {stride} {name} {which}: {bad} / {bad0} of {want.size} voxels differ; corrected share "
          f"{whole.mean():.3f}, covered voxels of partly covered tiles {(covered & ~whole).sum()}")
    assert bad == 0 and bad0 == 0
    assert np.array_equal(bits(got)[~covered], bits(c['x'])[~covered]) and not got0.cpu().numpy()[~covered].any()
    partly = covered & ~whole
    assert np.array_equal(bits(got0)[partly], bits(c['fused'][clamp][0])[partly])             # the plain update: x0 as fused
    assert np.array_equal(bits(shaped)[~whole], bits(n)[~whole]) and (bits(shaped) != bits(n))[whole].mean() > 0.9
    assert (bits(got0) != bits(c['fused'][clamp][0]))[whole].mean() > 0.9                      # and the whole tiles did move
    ops.volume_joint_consistent_tile_noise_step(*args, x, prev, *tail, out=x, x0_out=prev)
    assert torch.equal(x, got) and (prev is None or torch.equal(prev, got0))


@pytest.mark.parametrize('which', list(SETS))
@pytest.mark.parametrize('form', [0, 2])
@pytest.mark.parametrize('name', ['stacks-222', 'stack-411', 'stacks-135', 'dense-232'])
@pytest.mark.parametrize('tiling', DC.STEP_TILINGS, ids=['s4-gaussian', 's5-constant'])
def test_joint_tile_noise_step_is_the_reference_bit_for_bit(tiling, name, form, which):
    """Every voxel is compared: nothing is excluded.  The fresh launch, then the same launch in place (``x_next`` aliasing ``x_t`` and,
    with a history, ``x0_out`` aliasing ``x0_prev``).  A tile with an uncovered voxel keeps its plain x0 and its plain normals."""
    stride, kind = tiling
    _check_step(_step_refs(stride, kind), stride, name, form, which, DC.STEP_VOL)


@pytest.mark.parametrize('form', [0, 2])
def test_joint_tile_noise_step_with_the_full_tables_is_the_reference_bit_for_bit(form):
    """n = 64: tile (4, 4, 4) with all three stacks, 32 KiB of tables and the longest sums, on a (12, 16, 72) volume."""
    _check_step(_step_refs(4, 'gaussian', BIG_VOL), 4, 'stacks-444', form, 'mixed', BIG_VOL)


def test_joint_tile_noise_step_refusals():
    """Form 1 and kn = 0 are DIQT_E_UNSUPPORTED (-3) at the entry, with real device buffers; ``ops`` refuses them first."""
    from diffusioniqt_amd import _lib, ops
    c = _step_refs(4, 'gaussian')
    y, slot, taps, x = cu(c['y']), cu(c['slot'].astype(np.int32)), cu(c['taps']), cu(c['x'])
    cell, _, _, dev, _ = noise_operator('stacks-222')
    meas, out, out0 = cu(c['coarse']), torch.empty_like(x), torch.empty_like(x)
    lib = _lib.load()

    def entry(form, kn):
        ptr = lambda t: None if t is None else t.data_ptr()
        return lib.diqt_volume_joint_consistent_tile_noise_step(ptr(y), ptr(slot), ptr(taps), ptr(x), None, ptr(meas), ptr(dev[0]), ptr(out),
                                                                ptr(out0), form, y.shape[0], *x.shape, 8, 4, *slot.shape, 2, 2, 2, KX, 0.5,
                                                                0.0, kn, -1.0, 1.0, 1, SEED, 1, 0, None)
    assert entry(1, KN) == -3 and entry(0, 0.0) == -3 and entry(2, 0.0) == -3 and entry(3, KN) == -3
    torch.cuda.synchronize()
    for form, kn in ((1, KN), (0, 0.0)):
        with pytest.raises(ValueError, match="volume_joint_consistent_tile_noise_step"):
            ops.volume_joint_consistent_tile_noise_step(y, slot, taps, x, None, meas, cell, dev[0], form, KX, 0.5, 0.0, kn, -1.0, 1.0, 1, 4)
    with pytest.raises(ValueError, match="consistency_row_noise tables"):
        ops.volume_joint_consistent_tile_noise_step(y, slot, taps, x, None, meas, cell, dev, 0, KX, 0.5, 0.0, KN, -1.0, 1.0, 1, 4)


# ---- G3: the chains through VolumeInference against the float64 reference ----------------------------------------------------------------------
CHAIN_OPERATORS = ['stacks-222', 'stacks-421']
VP = {'ddpm': ('ddpm', 0.0), 'ddim-eta0.5': ('ddim', 0.5)}
SIGMA_STATE = 0.1                                             # the smallest row deviation, in state units


def raw_sigma(den, cfg, name):
    """(the raw per-row deviations whose smallest is 0.1 in state space, that value as the chain computes it)."""
    _, _, sigma = TN.case_of(name)
    unit = den.state_space(torch.tensor([0., 1.], dtype=torch.float64))
    slope, std = abs(float(unit[1] - unit[0])), float(cfg['Data']['std'])
    raw = (sigma / sigma.min() * (SIGMA_STATE * std / slope)).tolist()
    return raw, min(raw) / std * slope


def _reference_tables(name, raw, sigma_state, rows, w):
    """(cell, operator, P, tables, kinds) of the chain.  As in tests/test_gpu_volume_tile.py the float64 side takes the fp32 tables
    the device reads, widened -- their rounding defines the step -- and the host tests compare them with the restatement; the
    dispatch is cross-checked against the restatement's own whitening and schedule here."""
    from diffusioniqt_amd import ops
    cell, A_, _ = TN.case_of(name)
    op = ops.tile_noise_operator(cell, A_, raw)
    tables, kinds = ops.tile_noise_tables(op, ops.tile_noise_schedule(op, rows, sigma_state, w))
    wh = TN.whiten(A_, raw)
    assert [k for k, _ in kinds] == [k for k, _ in TN.kinds(TN.schedule64(rows, wh['S'], sigma_state, w))]
    assert np.abs(op.pinv.numpy() - wh['pinv']).max() <= 1e-12 * np.abs(wh['pinv']).max()
    return cell, op, op.table.numpy(), tables.numpy(), kinds


def check(got, ref, what):
    got = got.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == ref['mean'].shape and np.isfinite(got).all()
    err = np.abs(got.astype(np.float64) - ref['mean']).max()
    print(f"{what}: max |mean - ref| = {err:.3e}, bound {ref['bound']:.3e}; dispatch {[k for k, _ in ref['kinds']]}")
    assert err <= ref['bound'], what
    return got


@pytest.mark.parametrize('op_name', CHAIN_OPERATORS)
@pytest.mark.parametrize('name', list(VP))
def test_row_noise_joint_chain_matches_the_float64_reference(name, op_name):
    from diffusioniqt_amd.inference import VolumeInference
    from tests import volume_joint_tile_reference as TR
    imagen = stub_imagen('x_start', 'clamp-min', size=CHAIN_P)
    vol, cfg, w = chain_volume(), chain_cfg(), 1.0 if op_name == 'stacks-222' else 0.5
    den = vp_denoiser(imagen, *VP[name])
    raw, sigma = raw_sigma(den, cfg, op_name)

    def make():
        coefs = den.coefs.numpy().astype(np.float64)
        cell, op, P, tables, kinds = _reference_tables(op_name, raw, sigma, TN.rows4(coefs), w)
        rows = chain_rows(op)
        log_snr = J.tables(imagen.noise_schedulers[1], J.STEPS, 0.0, 'x_start')[2]
        target = TR.target_state(rows, cell, op.pinv.numpy(), cfg)
        x, L, x0_max, eps_max = TN.vp_chain(vol, cfg, coefs, log_snr, (J.MIN_BOUND, 0., 0), 'gaussian', target, cell, P, tables, kinds,
                                            seed=J.SEED)
        ref = DC.finish(vol, cfg, [np.maximum(x, J.MIN_BOUND)], L)
        extra = TN.extra_per_step(cell, P, tables, kinds, coefs[:, 2], max(x0_max, float(np.abs(target).max())), eps_max)
        ref.update(kinds=kinds, rows=rows, bound=TN.vp_bound(ref['windows_per_voxel'], ref['scale'], extra))
        return ref
    ref = cached(('row-vp', name, op_name), make)
    assert [k for k, _ in ref['kinds']] == ['noise'] * (J.STEPS - 1) + ['plain']
    cell = TN.case_of(op_name)[0]
    common = dict(blend='gaussian', noise='anchored', joint=True, seed=J.SEED, consistency=(torch.from_numpy(ref['rows']), cell),
                  consistency_weight=w, consistency_operator=TN.case_of(op_name)[1])
    got = check(VolumeInference(cfg, den, consistency_row_noise=raw, **common)(cu(vol)), ref, f"row-noise joint {name} {op_name} w {w}")
    constant = VolumeInference(cfg, den, **common)(cu(vol)).cpu().numpy()
    live = ref['covered'] & ~ref['background']
    assert (~ref['covered']).any() and np.abs(got - constant)[live].max() > 0.01            # and it is not the constant-weight chain


@pytest.mark.parametrize('op_name', CHAIN_OPERATORS)
def test_row_noise_edm_joint_chain_matches_the_float64_reference(op_name):
    from diffusioniqt_amd.inference import VolumeInference
    from tests import volume_joint_tile_reference as TR
    eta = 1.0
    elu = HN.make_elucidated('churn-on', False, size=CHAIN_P).to(DEV)
    den = elu.window_denoiser(sampler='dpmpp2m', eta=eta)
    vol, cfg = chain_volume(), chain_cfg()
    raw, sigma = raw_sigma(den, cfg, op_name)

    def make():
        tabs = E.tables(HN.HP, eta, coefs=den.coefs.numpy())
        coefs = den.coefs.numpy().astype(np.float64)
        cell, op, P, tables, kinds = _reference_tables(op_name, raw, sigma, coefs, 1.0)
        rows = chain_rows(op)
        target = TR.target_state(rows, cell, op.pinv.numpy(), cfg)
        x, L, state_max, x0_max, eps_max = TN.edm_chain(vol, cfg, tabs, 'gaussian', False, target, cell, P, tables, kinds)
        ref = DC.finish(vol, cfg, [np.clip(x, -1.0, 1.0)], L)
        mean32, std32 = np.float32(cfg['Data']['mean']), np.float32(cfg['Data']['std'])
        lowres_max = tabs['lowres'][0] * float(np.abs((vol - mean32) / std32).max()) + 6 * tabs['lowres'][1]
        extra = TN.extra_per_step(cell, P, tables, kinds, coefs[:, 3], max(x0_max, float(np.abs(target).max())), eps_max)
        ref.update(kinds=kinds, rows=rows, bound=TN.edm_bound(tabs, L, extra, state_max, lowres_max, False))
        return ref
    ref = cached(('row-edm', op_name), make)
    assert ref['kinds'][-1][0] == 'plain' and 'noise' in [k for k, _ in ref['kinds']]
    cell, A_, _ = TN.case_of(op_name)
    inf = VolumeInference(cfg, den, blend='gaussian', noise='anchored', joint=True, seed=E.SEED,
                          consistency=(torch.from_numpy(ref['rows']), cell), consistency_operator=A_, consistency_row_noise=raw)
    check(inf(cu(vol)), ref, f"row-noise joint EDM dpmpp2m eta {eta} {op_name}")


# ---- G4: stride = patch: the joint chain is the per-window sampler ------------------------------------------------------------------------------
def _tie_kw(op_name, raw):
    cell, A_, _ = TN.case_of(op_name)
    rows = chain_rows(type('shape', (), dict(m=A_.shape[0], cell=cell)))
    return dict(consistency=(torch.from_numpy(rows), cell), consistency_weight=0.75, consistency_operator=A_, consistency_row_noise=raw)


@pytest.mark.parametrize('op_name', CHAIN_OPERATORS)
@pytest.mark.parametrize('name', list(VP))
def test_row_noise_joint_at_stride_equal_patch_is_the_independent_path(name, op_name):
    """No overlap, unit weights: num / den is exact, no tile straddles a window, and a window's normals are the volume's: the fused
    launch is ``ops.tile_project_noise`` and the per-window step on every window -- one set of tables, the same ``__device__`` sums
    -- equal at every voxel, bit for bit."""
    from diffusioniqt_amd.inference import VolumeInference
    sampler, eta = VP[name]
    for mode in ('clamp-min', 'dynamic'):
        imagen = stub_imagen('x_start', mode, size=CHAIN_P)
        vol, cfg = cu(chain_volume()), chain_cfg(stride=CHAIN_P)
        den = vp_denoiser(imagen, sampler, eta)
        cons = _tie_kw(op_name, raw_sigma(den, cfg, op_name)[0])

        def sample_fn(x, noise=None, **kw):
            assert set(kw) == set(cons)
            return imagen.sample(batch_size=x.shape[0], start_image_or_video=x, start_at_unet_number=2, use_tqdm=False, sampler=sampler,
                                 sample_steps=J.STEPS, eta=eta, noise=noise, **kw)[0]
        independent = VolumeInference(cfg, sample_fn, blend='constant', noise='anchored', seed=J.SEED, **cons)(vol)
        joint = VolumeInference(cfg, den, blend='constant', noise='anchored', joint=True, seed=J.SEED, **cons)(vol)
        constant = VolumeInference(cfg, den, blend='constant', noise='anchored', joint=True, seed=J.SEED,
                                   **{k: v for k, v in cons.items() if k != 'consistency_row_noise'})(vol)
        assert independent.unique().numel() > 1000 and not torch.equal(joint, constant)
        assert torch.equal(joint, independent), mode


@pytest.mark.parametrize('op_name', CHAIN_OPERATORS)
def test_row_noise_edm_joint_at_stride_equal_patch_is_the_independent_path(op_name):
    from diffusioniqt_amd.inference import VolumeInference
    eta = 1.0
    for dynamic in (False, True):
        elu = HN.make_elucidated('churn-on', dynamic, self_cond=True, size=CHAIN_P).to(DEV)
        vol, cfg = cu(chain_volume()), chain_cfg(stride=CHAIN_P)
        den = elu.window_denoiser(sampler='dpmpp2m', eta=eta)
        cons = _tie_kw(op_name, raw_sigma(den, cfg, op_name)[0])

        def sample_fn(x, noise=None, **kw):
            assert set(kw) == set(cons)
            return elu.sample(batch_size=x.shape[0], video_frames=CHAIN_P, start_image_or_video=x, start_at_unet_number=2, noise=noise,
                              sampler='dpmpp2m', eta=eta, use_tqdm=False, **kw)
        independent = VolumeInference(cfg, sample_fn, blend='constant', noise='anchored', seed=E.SEED, **cons)(vol)
        joint = VolumeInference(cfg, den, blend='constant', noise='anchored', joint=True, seed=E.SEED, **cons)(vol)
        assert independent.unique().numel() > 1000
        assert torch.equal(joint, independent), dynamic
