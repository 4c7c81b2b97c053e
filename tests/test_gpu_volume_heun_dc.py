"""Data-consistent sampling for the stochastic Heun sampler on a real MI355X against tests/volume_joint_heun_dc_reference.py: the
fused launch ``ops.volume_joint_consistent_heun`` bit for bit against the fp32 restatement (no voxel is left out of a comparison), the
consistent joint Heun chains through ``VolumeInference(consistency_heun=...)`` against the float64 chains, the bit-for-bit tie of the
joint chain at stride = patch to ``sample(sampler='heun', consistency_heun=...)`` per window, the five modes of the per-window loop
against the float64 loop, and the guarantee (cell means of the final state = the measurement).

Bounds: that module's docstring.  The chain tests take the Heun reference's ``chain_bound`` plus, per projection performed, the mode's
own roundings; the per-window tests put the mode's allowance into the local term of every fused evaluation, as the per-mode tests of
the EDM family's multistep chains do; the guarantee test takes one projection's roundings."""
import math
from contextlib import nullcontext

import numpy as np
import pytest
import torch

from tests import volume_blend_reference as R
from tests import volume_joint_band_reference as BD
from tests import volume_joint_dc_reference as DC
from tests import volume_joint_heun_dc_reference as HD
from tests import volume_joint_heun_reference as HN
from tests import volume_joint_profile_reference as PR
from tests import volume_joint_reference as J
from tests import volume_joint_slab_reference as SL
from tests import volume_joint_tile_reference as TR

pytestmark = pytest.mark.gpu
DEV = "cuda"
INF, CLAMPS, COEFS1, COEFS2, KC, MODES = HD.INF, HD.CLAMPS, HD.COEFS1, HD.COEFS2, HD.KC, HD.MODES
SEED, SAMPLE, DRAW = 0x123456789, 2, 5
ramp, stacks = HD.ramp, HD.stacks
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


def table_of(mode, cell):
    """The shared host table of a mode; a profile's is also the reference module's own table, bit for bit."""
    table = HD.table_of(mode, cell)
    if mode == 'profile':
        assert np.array_equal(bits(table), bits(PR.profile_table(cell, ramp(cell))))
    return table


# ---- G1: the fused launch, bit for bit ---------------------------------------------------------------------------------------------------------
BIG_VOL, _step_refs = HD.BIG_VOL, HD.step_refs             # the cases, their second predictions and fused x0: the host test's too


def _normals(shape):
    from diffusioniqt_amd import ops
    return cached(('n', shape), lambda: ops.volume_joint_init(shape, SEED, sample=SAMPLE, draw=DRAW).cpu().numpy())


def _check_launch(c, stride, shape, cell, mode, clamp, w):
    """Phase 1, then phase 2 without and with a churn from the state phase 1 left; ``xh``, ``xn`` and ``x0v`` at every voxel."""
    from diffusioniqt_amd import ops
    table = table_of(mode, cell)
    meas, xh0, xn0, x0v0 = HD.step_operands(c, cell, mode)
    f1, f2 = c['fused'][clamp]
    covered = f1[1]
    whole = DC.replicate(DC._cells(covered, cell).all(axis=(-5, -3, -1)), cell)
    # corrected cells and uncovered voxels in every case; partly covered cells wherever the cell does not divide the stride
    assert whole.any() and (~covered).any() and ((covered & ~whole).any() or all(stride % f == 0 for f in cell))
    kw = dict(mode=mode, table=table)
    want1 = HD.heun_phase32(1, f1, xh0, xn0, x0v0, meas, cell, w, COEFS1, **kw)
    args = (cu(c['y']), cu(c['slot'].astype(np.int32)), cu(c['taps']))
    args2 = (cu(c['y2']),) + args[1:]
    dev_table = None if table is None else cu(table)
    tail = (*CLAMPS[clamp], stride, SEED, DRAW, SAMPLE)
    xh, xn, x0v, m = cu(xh0), cu(xn0), cu(x0v0), cu(meas)
    r = ops.volume_joint_consistent_heun(*args, xh, xn, x0v, m, cell, dev_table, w, 1, COEFS1, 0., *tail, mode=mode)
    assert all(t.data_ptr() == v.data_ptr() for t, v in zip(r, (xh, xn, x0v)))
    bad = [int((bits(g) != bits(v)).sum()) for g, v in zip((xh, xn, x0v), want1)]
    print(f"heun dc phase 1 stride {stride} cell {cell} {mode} clamp {clamp} w {w}: {bad} of {covered.size} voxels differ; corrected share "
          f"{whole.mean():.3f}, covered voxels of partly covered cells {(covered & ~whole).sum()}")
    assert bad == [0, 0, 0]
    assert np.array_equal(bits(xn)[~covered], bits(xh0)[~covered]) and not x0v.cpu().numpy()[~covered].any()
    partly = covered & ~whole
    assert np.array_equal(bits(x0v)[partly], bits(f1[0])[partly])                          # a partly covered cell: x0 as fused
    assert (bits(x0v) != bits(f1[0]))[whole].mean() > 0.9                                   # and the whole cells did move
    state = [t.clone() for t in (xh, xn, x0v)]
    for kc in (0.0, KC):
        n = _normals(shape) if kc != 0 else None
        want2 = HD.heun_phase32(2, f2, *want1, meas, cell, w, COEFS2, kc, n, **kw)
        xh, xn, x0v = (t.clone() for t in state)
        ops.volume_joint_consistent_heun(*args2, xh, xn, x0v, m, cell, dev_table, w, 2, COEFS2, kc, *tail, mode=mode)
        bad = [int((bits(g) != bits(v)).sum()) for g, v in zip((xh, xn, x0v), want2)]
        print(f"heun dc phase 2 kc {kc}: {bad} voxels differ")
        assert bad == [0, 0, 0]
        assert torch.equal(xn, state[1])                                                   # phase 2 does not write xn
        assert np.array_equal(bits(xh)[~covered], bits(xh0)[~covered]) and not x0v.cpu().numpy()[~covered].any()


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('cell', DC.STEP_CELLS)
@pytest.mark.parametrize('tiling', DC.STEP_TILINGS, ids=['s4-gaussian', 's5-constant'])
def test_joint_consistent_heun_is_the_reference_bit_for_bit(tiling, cell, mode):
    """Every voxel of the three volumes is compared: nothing is excluded.  The clamp and the weight rotate over the cases so that min,
    box and none, and w = 1 and 0.5, each meet every mode and both tilings."""
    stride, kind = tiling
    _check_launch(_step_refs(stride, kind), stride, DC.STEP_VOL, cell, mode, *HD.step_rotation(stride, cell, mode))


@pytest.mark.parametrize('clamp,w', HD.BIG_CASES)
def test_joint_consistent_heun_with_the_full_table_is_the_reference_bit_for_bit(clamp, w):
    """n = 64: tile (4, 4, 4) with all three stacks, the 16 KiB table and the longest sum, on a (12, 16, 72) volume."""
    _check_launch(_step_refs(4, 'gaussian', BIG_VOL), 4, BIG_VOL, HD.BIG_CELL, 'tile', clamp, w)


def test_joint_consistent_heun_argument_errors():
    from diffusioniqt_amd import ops
    c = _step_refs(4, 'gaussian')
    y, slot, taps, xh = cu(c['y']), cu(c['slot'].astype(np.int32)), cu(c['taps']), cu(c['x'])
    xn, x0, m = torch.empty_like(xh), torch.empty_like(xh), torch.zeros_like(xh)
    table = cu(table_of('tile', (2, 2, 2)))
    ok = (0.0, -1.0, 1.0, 1, 4)
    call = ops.volume_joint_consistent_heun
    with pytest.raises(ValueError, match="phase"):
        call(y, slot, taps, xh, xn, x0, m, (2, 2, 2), None, 1.0, 0, COEFS1, *ok)
    with pytest.raises(ValueError, match="mode"):
        call(y, slot, taps, xh, xn, x0, m, (2, 2, 2), None, 1.0, 1, COEFS1, *ok, mode='slab')
    with pytest.raises(ValueError, match="coefficients"):
        call(y, slot, taps, xh, xn, x0, m, (2, 2, 2), None, 1.0, 2, COEFS1, *ok)
    with pytest.raises(ValueError, match="consistency cell"):
        call(y, slot, taps, xh, xn, x0, m, (3, 1, 1), None, 1.0, 1, COEFS1, *ok)                           # 20 % 3
    with pytest.raises(ValueError, match="consistency weight"):
        call(y, slot, taps, xh, xn, x0, m, (2, 2, 2), None, 0.0, 1, COEFS1, *ok)
    with pytest.raises(ValueError, match="meas_up must be"):
        call(y, slot, taps, xh, xn, x0, m[:10].contiguous(), (2, 2, 2), None, 1.0, 1, COEFS1, *ok)
    with pytest.raises(ValueError, match="four different"):
        call(y, slot, taps, xh, xn, xn, m, (2, 2, 2), None, 1.0, 1, COEFS1, *ok)
    with pytest.raises(ValueError, match="takes no table"):
        call(y, slot, taps, xh, xn, x0, m, (2, 2, 2), table, 1.0, 1, COEFS1, *ok)
    with pytest.raises(ValueError, match="consistency_operator table"):
        call(y, slot, taps, xh, xn, x0, m, (4, 1, 1), table, 1.0, 1, COEFS1, *ok, mode='tile')             # [8, 8] is not [4, 4]
    with pytest.raises(ValueError, match="consistency profile table"):
        call(y, slot, taps, xh, xn, x0, m, (2, 2, 2), table, 1.0, 1, COEFS1, *ok, mode='profile')
    with pytest.raises(ValueError, match="clamp_mode"):
        call(y, slot, taps, xh, xn, x0, m, (2, 2, 2), None, 1.0, 1, COEFS1, 0.0, -1.0, 1.0, 2, 4)
    with pytest.raises(ValueError, match="lattice"):
        call(y, slot, taps, xh, xn, x0, m, (2, 2, 2), None, 1.0, 1, COEFS1, 0.0, -1.0, 1.0, 1, 5)


# ---- G2: the chains through VolumeInference against the float64 reference ----------------------------------------------------------------------
CHAIN_P, CHAIN_CELLS = HD.CHAIN_P, HD.CHAIN_CELLS
chain_volume, chain_cfg, chain_case = HD.chain_volume, HD.chain_cfg, HD.chain_case      # shared with the host emulation


def check(got, ref, what, key='mean'):
    got = got.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == ref[key].shape and np.isfinite(got).all()
    err = np.abs(got.astype(np.float64) - ref[key]).max()
    print(f"{what}: max |{key} - ref| = {err:.3e}, bound {ref['bound']:.3e} (share {err / ref['bound']:.4f})")
    assert err <= ref['bound'], what
    return got


@pytest.mark.parametrize('which', HD.WHICH)
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('cell', CHAIN_CELLS)
@pytest.mark.parametrize('churn', list(HN.CHURN))
def test_consistent_joint_heun_chain_matches_the_float64_reference(churn, cell, mode, which):
    from diffusioniqt_amd.inference import VolumeInference
    elu = HN.make_elucidated(churn, False, size=CHAIN_P).to(DEV)
    vol, cfg, w = chain_volume(), chain_cfg(), HD.chain_weight(cell)
    meas, kw, meas_up, table = chain_case(mode, cell)
    tabs = HN.tables(HN.HP, HN.CHURN[churn])
    ref = cached(('chain', churn, cell, mode, which),
                 lambda: HD.joint_reference(vol, cfg, tabs, 'gaussian', False, mode, meas_up, cell, w, which, table))
    assert ref['projections'] == (2 * HN.HP['num_sample_steps'] - 1 if which == 'both' else HN.HP['num_sample_steps'])
    inf = VolumeInference(cfg, elu.window_denoiser(), blend='gaussian', noise='anchored', joint=True, seed=HN.SEED,
                          consistency=(torch.from_numpy(meas), cell), consistency_weight=w, consistency_heun=which, **kw)
    got = check(inf(cu(vol)), ref, f"consistent joint Heun {churn} cell {cell} {mode} {which} w {w}")
    plain = cached(('plain', churn), lambda: VolumeInference(cfg, elu.window_denoiser(), blend='gaussian', noise='anchored', joint=True,
                                                             seed=HN.SEED)(cu(vol)).cpu().numpy())
    live = ref['covered'] & ~ref['background']
    assert (~ref['covered']).any() and np.abs(got - plain)[live].max() > 0.05            # and it is not the plain chain


# ---- G3: stride = patch: the joint chain is the per-window sampler ------------------------------------------------------------------------------
@pytest.mark.parametrize('which', HD.WHICH)
@pytest.mark.parametrize('mode', ['cell', 'tile'])
def test_consistent_joint_heun_at_stride_equal_patch_is_the_independent_path(mode, which):
    """No overlap, unit weights: num / den is exact and no cell straddles a window, so the fused projection is the per-window launch on
    every window and both paths take the same ``__device__`` projection and updates -- equal at every voxel, bit for bit, under the
    static clamp and dynamic thresholding, with a self-conditioning U-Net."""
    from diffusioniqt_amd.inference import VolumeInference
    cell = (2, 2, 2)
    for dynamic in (False, True):
        elu = HN.make_elucidated('churn-on', dynamic, self_cond=True, size=CHAIN_P).to(DEV)
        vol, cfg = cu(chain_volume()), chain_cfg(stride=CHAIN_P)
        meas, kw, _, _ = chain_case(mode, cell)
        cons = dict(consistency=(torch.from_numpy(meas), cell), consistency_weight=0.75, consistency_heun=which, **kw)

        def sample_fn(x, noise=None, **given):
            assert set(given) == set(cons)
            return elu.sample(batch_size=x.shape[0], video_frames=CHAIN_P, start_image_or_video=x, start_at_unet_number=2, noise=noise,
                              sampler='heun', use_tqdm=False, **given)
        independent = VolumeInference(cfg, sample_fn, blend='constant', noise='anchored', seed=HN.SEED, **cons)(vol)
        joint = VolumeInference(cfg, elu.window_denoiser(), blend='constant', noise='anchored', joint=True, seed=HN.SEED, **cons)(vol)
        plain = VolumeInference(cfg, elu.window_denoiser(), blend='constant', noise='anchored', joint=True, seed=HN.SEED)(vol)
        other = VolumeInference(cfg, elu.window_denoiser(), blend='constant', noise='anchored', joint=True, seed=HN.SEED,
                                **{**cons, 'consistency_heun': HD.WHICH[1 - HD.WHICH.index(which)]})(vol)
        assert independent.unique().numel() > 1000 and not torch.equal(joint, plain) and not torch.equal(joint, other)
        assert torch.equal(joint, independent), dynamic


# ---- G4: the per-window loop, five modes ---------------------------------------------------------------------------------------------------------
WINDOW_P, WINDOW_STEPS = 8, 3
WINDOW_CELL = (2, 2, 2)
WINDOW_SLAB = ([0.25, 1.0, 1.0, 0.25], [1.0, 0.5], [0.75, 1.0])
WINDOW_BAND = ([1.0, 0.5], None, None, 'centre')


def one_window_volume():
    return np.random.default_rng(9).integers(1, 1000, (WINDOW_P,) * 3).astype(np.float32)


def window_case(mode):
    """Per mode: the keywords of ``sample``, the measurement operand in state space (float32 [P,P,P] on the host), the context in which
    ``volume_joint_dc_reference.project64`` is the mode's float64 projection, and ``allowance(scale)`` of one projection."""
    from diffusioniqt_amd import ops
    vol, cfg, cell = one_window_volume(), chain_cfg(stride=WINDOW_P), WINDOW_CELL
    meas = DC.measurement(vol, cell)
    up = DC.measurement_state(meas, cell, cfg)
    if mode == 'cell':
        return {}, up, nullcontext(), lambda S, out: DC.projection_roundings(cell, S)
    if mode == 'profile':
        table = table_of('profile', cell)
        return dict(consistency_profile=ramp(cell)), up, PR._projection(table), lambda S, out: PR.profile_roundings(cell, table, 1.0, S)
    if mode == 'tile':
        rows, kw, t, table = chain_case('tile', cell, vol, cfg)
        return kw, t, TR._projection(table), lambda S, out: TR.tile_roundings(cell, table, S)
    if mode == 'slab':
        tab = SL.table(cell, WINDOW_SLAB, WINDOW_P // cell[0])
        return dict(consistency_slab=WINDOW_SLAB), up, SL.slab_chains(tab), lambda S, out: SL.slab_roundings(tab, S)
    axes = BD.axes_of((WINDOW_P,) * 3, cell, WINDOW_BAND[:3], WINDOW_BAND[3])
    tabs, _ = BD.tables32(axes)
    dev = ops.band_table((WINDOW_P,) * 3, cell, WINDOW_BAND[:3], WINDOW_BAND[3]).to(DEV)
    mean, std = float(cfg['Data']['mean']), float(cfg['Data']['std'])
    t = ((ops.band_backproject(cu(meas), dev) - mean) / std).cpu().numpy()                 # the target as the device makes it
    assert np.abs(t - BD.target_state(meas, axes, cfg)).max() <= 1e-5
    return dict(consistency_band=WINDOW_BAND), t, BD.band_chains(axes), lambda S, out: BD.allowance(axes, tabs, 2 * S, out)


@pytest.mark.parametrize('mode', ['cell', 'profile', 'tile', 'slab', 'band'])
def test_per_window_heun_sampler_matches_the_float64_loop(mode):
    """``ElucidatedImagen.sample(sampler='heun', consistency_heun='both')`` on one window of edge 8, three Heun steps, with the
    volume-anchored draws, against the float64 loop (the joint reference on a volume of one window with unit weights IS the per-window
    loop).  The bound is the Heun ``chain_bound`` with the mode's allowance in the local term of every fused evaluation."""
    from diffusioniqt_amd.inference import VolumeInference
    hp = {**HN.HP, 'num_sample_steps': WINDOW_STEPS}
    elu = HN.make_elucidated('churn-on', False, size=WINDOW_P, num_sample_steps=WINDOW_STEPS).to(DEV)
    vol, cfg, cell = one_window_volume(), chain_cfg(stride=WINDOW_P), WINDOW_CELL
    kw, target, context, allowance = window_case(mode)
    tabs = HN.tables(hp, HN.CHURN['churn-on'])
    with context:
        ref = HD.joint_reference(vol, cfg, tabs, 'constant', False, 'cell', target.astype(np.float64), cell, 1.0, 'both')
    assert ref['projections'] == 2 * WINDOW_STEPS - 1 and ref['covered'].all()
    extra = math.ceil(allowance(ref['scale'], ref['scale']) / 2.0 ** -23)
    ref['bound'] = HN.chain_bound(tabs, ref['windows_per_voxel'] + extra, ref['state_max'], ref['lowres_max'], False, False)
    t = cu(target.astype(np.float32))[None, None]

    def sample_fn(x, noise=None):
        return elu.sample(batch_size=x.shape[0], video_frames=WINDOW_P, start_image_or_video=x, start_at_unet_number=2, noise=noise,
                          sampler='heun', use_tqdm=False, consistency=(t, cell), consistency_heun='both', **kw)
    got = VolumeInference(cfg, sample_fn, blend='constant', noise='anchored', seed=HN.SEED)(cu(vol))
    got = check(got, ref, f"per-window Heun {mode}, {2 * WINDOW_STEPS - 1} projections")
    plain = HN.joint_reference(vol, cfg, tabs, 'constant', False)
    assert np.abs(got - plain['mean'])[~ref['background']].max() > 0.01                   # and it is not the plain loop


# ---- G5: the guarantee -------------------------------------------------------------------------------------------------------------------------
GUARANTEE_CELLS = [(2, 2, 2), (4, 1, 1), (1, 1, 3)]          # (1, 1, 3) straddles the windows (P 8, stride 4): only the joint state projects it


def _cell_means64(x, cell):
    return DC._cells(np.asarray(x, dtype=np.float64), cell).mean(axis=(-5, -3, -1))


@pytest.mark.parametrize('which', HD.WHICH)
@pytest.mark.parametrize('cell', GUARANTEE_CELLS)
def test_final_state_has_the_measurements_cell_means(cell, which, monkeypatch):
    """No clamp, every voxel covered, w = 1.  The last Heun step ends at sigma = 0 with (a1, b1) = (0, 1) and no corrector, so the state
    the chain ends in IS its last projected prediction: its cell means, recomputed in float64, are the measurement's within the
    roundings of ONE projection, under either keyword value.  The deviation of the same prediction before its projection (the fused
    x0 of the last launch, made again by the multistep launch's walk) is printed beside it."""
    from diffusioniqt_amd import ops
    from diffusioniqt_amd.inference import VolumeInference
    elu = HN.make_elucidated('churn-on', False, size=CHAIN_P).to(DEV)
    den = elu.window_denoiser(clamp=False)
    assert den.clamp == (-INF, INF, 1) and den.coefs[-1].tolist()[1:3] == [0.0, 1.0] and float(den.sched[-1][1]) == 0.0
    vol, cfg = chain_volume(full=True), chain_cfg()
    assert (J.layout(vol, cfg)['slot'] >= 0).all()                                         # every window kept: every voxel covered
    meas = DC.measurement(vol, cell)
    want = DC.measurement_state(meas, cell, cfg)[::cell[0], ::cell[1], ::cell[2]]
    real, fused, states = ops.volume_joint_consistent_heun, [], []

    def recording(y, slot, taps, xh, xn, x0, meas_up, cell_, table, weight, phase, coefs, kc, lo, hi, clamp_mode, stride, *a, **k):
        fused.append(ops.volume_joint_multistep(y, slot, taps, xh, None, 0.0, 1.0, 0.0, lo, hi, clamp_mode, stride)[1])
        return real(y, slot, taps, xh, xn, x0, meas_up, cell_, table, weight, phase, coefs, kc, lo, hi, clamp_mode, stride, *a, **k)
    monkeypatch.setattr(ops, 'volume_joint_consistent_heun', recording)
    den.finish = lambda x: states.append(x.clone()) or x                                  # the state the chain ends in, before any finish
    VolumeInference(cfg, den, blend='gaussian', noise='anchored', joint=True, seed=HN.SEED, consistency=(torch.from_numpy(meas), cell),
                    consistency_heun=which)(cu(vol))
    T = HN.HP['num_sample_steps']
    assert len(fused) == (2 * T - 1 if which == 'both' else T) and len(states) == 1
    x, x0 = states[0].cpu().numpy(), fused[-1].cpu().numpy()
    err = np.abs(_cell_means64(x, cell) - want).max()
    dev = np.abs(_cell_means64(x0, cell) - want).max()
    bound = DC.projection_roundings(cell, max(float(np.abs(x).max()), float(np.abs(x0).max()), float(np.abs(want).max())))
    print(f"guarantee Heun {which} cell {cell}: max |A x - y| = {err:.3e} on {want.size} cells, bound {bound:.3e}; before the projection "
          f"{dev:.3e}")
    assert err <= bound and dev > 0.1
    assert np.ptp(DC._cells(x, cell)[0, :, 0, :, 0, :]) > 0                                # the detail inside a cell is the network's
