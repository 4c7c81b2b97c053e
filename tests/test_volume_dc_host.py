"""Host-side checks of data-consistent sampling (no GPU here): the projection of tests/volume_joint_dc_reference.py has the properties
DDNM rests on, every argument rule of ``consistency=`` is raised before anything touches the device, the three C entries return the
error codes of include/diqt.h, and a consistent joint chain makes as many fused launches as the plain one."""
import collections

import numpy as np
import pytest
import torch

from tests import volume_blend_reference as R
from tests import volume_joint_dc_reference as DC
from tests import volume_joint_heun_reference as HN
from tests.test_volume_joint_host import _imagen

CELLS = [(4, 1, 1), (1, 3, 1), (1, 1, 5), (2, 2, 2), (1, 1, 7)]
SHAPE = (8, 12, 70)                                          # every cell above divides it


def _inputs(cell, seed=0):
    rng = np.random.default_rng(seed)
    x0 = (rng.standard_normal(SHAPE) * 2).astype(np.float32)
    meas = DC.replicate(rng.standard_normal(tuple(s // f for s, f in zip(SHAPE, cell))).astype(np.float32), cell)
    return x0, meas


# ---- H1: the projection of the reference ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cell', CELLS)
def test_projection_puts_the_cell_means_on_the_measurement_and_keeps_the_detail(cell):
    x0, meas = _inputs(cell)
    covered = np.ones(SHAPE, dtype=bool)
    out64, whole = DC.project64(x0.astype(np.float64), covered, meas.astype(np.float64), cell, 1.0)
    assert whole.all()
    means = DC._cells(out64, cell).mean(axis=(-5, -3, -1))
    assert np.abs(DC.replicate(means, cell) - meas).max() <= 1e-12                         # A x0' = y at w = 1
    shift = DC._cells(out64 - x0, cell)
    assert np.abs(shift - shift[:, :1, :, :1, :, :1]).max() <= 1e-12                       # x0' - x0 is constant per cell
    again, _ = DC.project64(out64, covered, meas.astype(np.float64), cell, 1.0)
    assert np.abs(again - out64).max() <= 1e-12                                            # idempotent at w = 1
    half, _ = DC.project64(x0.astype(np.float64), covered, meas.astype(np.float64), cell, 0.5)
    assert np.abs(half - 0.5 * (out64 + x0)).max() <= 1e-12                                # w < 1 goes that share of the way
    # the fp32 restatement: the same numbers within its own roundings, and exactly constant shifts are not promised (one fma per voxel)
    out32 = DC.project32(x0, meas, cell, 1.0)
    scale = max(float(np.abs(x0).max()), float(np.abs(meas).max()))
    assert out32.dtype == np.float32 and np.abs(out32.astype(np.float64) - out64).max() <= DC.projection_roundings(cell, scale)
    means32 = DC.replicate(DC.cell_mean32(out32, cell), cell).astype(np.float64)           # and its cell means are the measurement's
    assert np.abs(means32 - meas).max() <= 2 * DC.projection_roundings(cell, scale)        # (the roundings of A x0', then of this A)


@pytest.mark.parametrize('cell', CELLS)
def test_a_cell_with_an_uncovered_voxel_is_untouched(cell):
    x0, meas = _inputs(cell, 1)
    covered = np.ones(SHAPE, dtype=bool)
    covered[3, 7, 33] = False                                                              # one voxel of one cell
    out64, whole = DC.project64(x0.astype(np.float64), covered, meas.astype(np.float64), cell, 1.0)
    out32 = DC.project32(x0, meas, cell, 1.0, covered)
    n = cell[0] * cell[1] * cell[2]
    assert (~whole).sum() == n and not whole[3, 7, 33]
    assert np.array_equal(out64[~whole], x0[~whole].astype(np.float64)) and np.array_equal(out32[~whole], x0[~whole])
    assert (out32[whole] != x0[whole]).mean() > 0.99


def test_fma32_rounds_once():
    """Against the exact rational value, on products that cancel, that are swamped and that sit near rounding ties."""
    from fractions import Fraction
    rng = np.random.default_rng(2)
    a = (rng.standard_normal(3000) * rng.choice([1e-3, 1.0, 1e3], 3000)).astype(np.float32)
    b = rng.standard_normal(3000).astype(np.float32)
    c = rng.standard_normal(3000).astype(np.float32)
    c[1::3] = (-(a[1::3].astype(np.float64) * b[1::3])).astype(np.float32)
    c[2::3] = (a[2::3].astype(np.float64) * b[2::3] * 2.0 ** -30).astype(np.float32)
    got = DC.fma32(a, b, c)
    for i in range(a.size):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        near = np.float32(float(exact))
        cands = (np.nextafter(near, np.float32(-np.inf)), near, np.nextafter(near, np.float32(np.inf)))
        want = min(cands, key=lambda v: (abs(Fraction(float(v)) - exact), int(v.view(np.uint32)) & 1))
        assert got[i].view(np.uint32) == want.view(np.uint32), i


def test_the_step_inputs_are_what_the_bit_exact_cases_need():
    """The fp32 reference alone, before any GPU run: it excludes no voxel from a comparison (the existing joint tests have no fp32
    reference that does, so the cap is zero), both tilings leave uncovered voxels inside the volume and past its covered rows /
    columns, every cell has corrected cells, and the cells that do not divide the covered extent have partly covered ones."""
    assert DC.STEP_VOL[2] > 64 and DC.STEP_VOL[1] % 4
    partly = {}
    for stride, kind in DC.STEP_TILINGS:
        c = DC.step_case(stride, kind)
        assert (c['slot'] < 0).any() and c['N'] == c['slot'].max() + 1
        x0, covered = DC.fuse32(c['y'], c['slot'], c['taps'], stride, DC.STEP_VOL, DC.clamp32(-1., 1., 1))
        assert x0.dtype == np.float32 and np.isfinite(x0).all() and not x0[~covered].any()
        assert (~covered[:10, :9, :30]).any() and not covered[:, :, 68:].any()
        for cell in DC.STEP_CELLS:
            want, want0, cov = DC.joint_step32(c['y'], c['slot'], c['taps'], stride, c['x'], c['prev'], DC.step_meas(c, cell), cell, 1.0,
                                               2, 0.8125, -0.9375, -0.3125, 0.625, None, c['coarse'], fused=(x0, covered))
            whole = DC.replicate(DC._cells(cov, cell).all(axis=(-5, -3, -1)), cell)
            partly[stride, cell] = int((cov & ~whole).sum())
            assert whole.mean() > 0.7 and np.isfinite(want).all() and want.dtype == want0.dtype == np.float32
            assert np.array_equal(want[~cov], c['x'][~cov]) and (want0[whole] != x0[whole]).mean() > 0.99
            m = DC.cell_mean32(want0, cell).astype(np.float64)
            y = DC.step_meas(c, cell)[::cell[0], ::cell[1], ::cell[2]]
            assert np.abs(m - y)[whole[::cell[0], ::cell[1], ::cell[2]]].max() <= 2 * DC.projection_roundings(cell, 6.0)
    assert not covered[18:].any()                                                         # stride 5: the last two planes
    assert all(partly[4, cell] > 0 for cell in ((1, 3, 1), (1, 1, 5), (1, 1, 7))) and partly[4, (2, 2, 2)] == 0
    assert all(partly[5, cell] > 0 for cell in DC.STEP_CELLS)


# ---- H2: argument rules, all before the device is touched -----------------------------------------------------------------------------------
def _meas(P=16, B=2):
    return torch.zeros(B, 1, P, P, P)


def test_sample_refuses_consistency_it_cannot_honour():
    imagen = _imagen()
    lr = torch.zeros(2, 1, 16, 16, 16)
    base = dict(batch_size=2, start_image_or_video=lr, start_at_unet_number=2, use_tqdm=False, sampler='ddim', sample_steps=2)
    bad = [dict(consistency=(_meas(), (2, 2, 2)), consistency_weight=0.0), dict(consistency=(_meas(), (2, 2, 2)), consistency_weight=1.5),
           dict(consistency=(_meas(), (2, 2, 2)), consistency_weight=True),
           dict(consistency=(_meas(), (3, 1, 1))),                                         # 3 does not divide 16
           dict(consistency=(_meas(), (1, 1, 1))), dict(consistency=(_meas(), (8, 4, 4))),  # n = 1, n = 128
           dict(consistency=(_meas(), (2, 2))), dict(consistency=(_meas(), (2.0, 2, 2))), dict(consistency=(_meas(), (0, 2, 2))),
           dict(consistency=(_meas(P=8), (2, 2, 2))), dict(consistency=(_meas(B=3), (2, 2, 2))),
           dict(consistency=(_meas().long(), (2, 2, 2))), dict(consistency=(np.zeros((2, 1, 16, 16, 16), np.float32), (2, 2, 2))),
           dict(consistency=_meas()),
           dict(consistency=(_meas(), (2, 2, 2)), init_images=lr),
           dict(consistency=(_meas(), (2, 2, 2)), sampler='ddpm', sample_steps=None, skip_steps=2),
           dict(consistency=(_meas(), (2, 2, 2)), sampler='ddpm', inpaint_images=lr, inpaint_masks=lr[:, 0].bool())]
    for kw in bad:
        with pytest.raises(ValueError, match="consistency"):
            imagen.sample(**{**base, **kw})
    with pytest.raises(ValueError, match="consistency"):                                   # the loop itself applies the same rules
        imagen.p_sample_loop(imagen.unets[1], (2, 1, 16, 16, 16), noise_scheduler=imagen.noise_schedulers[1],
                             consistency=(_meas(), (2, 2, 2)), consistency_weight=0.0)


def test_edm_sample_refuses_consistency_it_cannot_honour():
    elu = HN.make_elucidated('churn-on', False)
    lr = torch.zeros(2, 1, 16, 16, 16)
    base = dict(batch_size=2, video_frames=16, start_image_or_video=lr, start_at_unet_number=2, use_tqdm=False, sampler='dpmpp2m')
    ok = (_meas(), (2, 2, 2))
    bad = [dict(consistency=ok, sampler='heun'),                                           # two predictions per step: a later piece of work
           dict(consistency=ok, consistency_weight=0.0), dict(consistency=ok, consistency_weight=2),
           dict(consistency=(_meas(), (3, 1, 1))), dict(consistency=(_meas(), (1, 1, 1))), dict(consistency=(_meas(P=8), (2, 2, 2))),
           dict(consistency=ok, init_images=lr)]
    for kw in bad:
        with pytest.raises(ValueError, match="consistency"):
            elu.sample(**{**base, **kw})
    with pytest.raises(ValueError, match="consistency"):
        elu.sample(**{**base, 'sampler': 'heun', 'consistency': ok, 'inpaint_images': lr, 'inpaint_masks': lr[:, 0].bool()})
    with pytest.raises(ValueError, match="consistency"):                                   # the loop itself applies the same rules
        elu.one_unet_sample(elu.unets[1], (2, 1, 16, 16, 16), unet_number=2, sampler='dpmpp2m', consistency=ok, consistency_weight=0)


def test_window_denoisers_expose_the_state_space_map():
    imagen, elu = _imagen(), HN.make_elucidated('churn-on', False)
    x = torch.linspace(-2, 2, 7)
    dens = [imagen.window_denoiser(sampler=s, sample_steps=3) for s in ('ddpm', 'ddim', 'dpmpp2m')]
    dens += [elu.window_denoiser(), elu.window_denoiser(sampler='dpmpp2m')]
    for den in dens:
        assert torch.equal(den.state_space(x), x)                                          # auto_normalize_img is off in both: the identity
    from diffusioniqt_amd.imagen_pytorch3D import normalize_neg_one_to_one
    imagen.normalize_img = normalize_neg_one_to_one
    assert torch.equal(imagen.window_denoiser(sampler='ddim', sample_steps=3).state_space(x), 2 * x - 1)


class _NeverDenoiser:
    num_steps, coefs, clamp = 3, torch.zeros(3, 3), (-1., 1., 1)

    def x0(self, *a, **k):
        raise AssertionError("the network must not run")
    finish = x0
    state_space = x0


def test_volume_inference_consistency_argument_errors():
    from diffusioniqt_amd.inference import VolumeInference

    def never(x, **kw):
        raise AssertionError("the sampler must not run")
    cfg = R.shared_cfg(8)                                                                  # P 16, stride 8, volume (40, 36, 44)
    meas = torch.zeros(20, 18, 22)
    ok = (meas, (2, 2, 2))
    joint = dict(blend='gaussian', noise='anchored', joint=True)
    known = (torch.zeros(40, 36, 44), torch.zeros(40, 36, 44, dtype=torch.bool))
    for kw in (dict(consistency=ok, consistency_weight=0.0), dict(consistency=ok, consistency_weight=1.25),
               dict(consistency=(meas, (1, 1, 1))), dict(consistency=(meas, (4, 4, 8))), dict(consistency=(meas, (2, 2))),
               dict(consistency=(meas.long(), (2, 2, 2))), dict(consistency=(meas[0], (2, 2, 2))), dict(consistency=meas),
               dict(consistency=ok, inpaint=known),
               dict(consistency=(meas, (1, 1, 3))),                                        # 3 divides neither the stride nor the window
               dict(consistency=(meas, (1, 1, 16)))):                                      # divides the window, not the stride
        with pytest.raises(ValueError, match="consistency"):
            VolumeInference(cfg, never, **kw)
    with pytest.raises(ValueError, match="consistency"):                                   # the Heun denoiser: a later piece of work
        VolumeInference(cfg, HN.make_elucidated('churn-on', False).window_denoiser(), consistency=ok, **joint)
    ancestral = _imagen().window_denoiser(sampler='ddpm', sample_steps=3)
    with pytest.raises(ValueError, match="consistency"):
        VolumeInference(cfg, ancestral, consistency=ok, inpaint=known, **joint)
    lacking = type('NoMap', (), dict(num_steps=3, coefs=torch.zeros(3, 3), clamp=(-1., 1., 1), x0=None, finish=None))()
    with pytest.raises(ValueError, match="consistency"):
        VolumeInference(cfg, lacking, consistency=ok, **joint)
    # on the joint state cells may straddle windows: only the volume has to be a multiple of the cell -- checked in __call__
    inf = VolumeInference(cfg, _NeverDenoiser(), consistency=(torch.zeros(40, 12, 44), (1, 3, 1)), consistency_weight=0.5, **joint)
    assert inf.consistency[1:] == ((1, 3, 1), 0.5)
    with pytest.raises(ValueError, match="consistency"):
        inf(torch.zeros(40, 36, 40))
    with pytest.raises(ValueError, match="consistency"):
        VolumeInference(cfg, never, consistency=ok)(torch.zeros(40, 36, 48))
    assert VolumeInference(cfg, never).consistency is None                                 # the default is today's path


# ---- H3: error codes of the three entries ---------------------------------------------------------------------------------------------------
def test_consistency_entries_return_error_codes():
    from diffusioniqt_amd import _lib
    lib = _lib.load()
    buf = (np.zeros(4, dtype=np.int32)).ctypes.data                             # never dereferenced: every call below is refused
    mean = lambda x, out, shape=(8, 12, 70), cell=(2, 2, 2): lib.diqt_cell_mean(x, out, *shape, *cell, None)
    assert mean(None, buf) == -2 and mean(buf, None) == -2                      # DIQT_E_ALIGN
    assert b"null pointer" in lib.diqt_last_error()
    assert mean(buf, buf, cell=(1, 1, 1)) == -3 and mean(buf, buf, cell=(1, 1, 65)) == -3 and mean(buf, buf, cell=(0, 2, 2)) == -3
    assert mean(buf, buf, cell=(3, 1, 1)) == -1 and mean(buf, buf, cell=(1, 1, 4)) == -1 and mean(buf, buf, shape=(0, 12, 70)) == -1
    proj = lambda x0, m, out, cubes=3, P=8, cell=(2, 2, 2), w=1.0, mode=2: lib.diqt_cell_project(x0, m, out, cubes, P, *cell, w, -1.0, 1.0,
                                                                                                mode, None)
    assert proj(None, buf, buf) == -2 and proj(buf, None, buf) == -2 and proj(buf, buf, None) == -2
    assert proj(buf, buf, buf, cell=(1, 1, 3)) == -1                            # DIQT_E_SHAPE: P % fx != 0
    assert b"does not divide" in lib.diqt_last_error()
    assert proj(buf, buf, buf, cell=(3, 1, 1)) == -1 and proj(buf, buf, buf, cubes=0) == -1
    assert proj(buf, buf, buf, cell=(1, 1, 1)) == -3 and proj(buf, buf, buf, cell=(8, 8, 2)) == -3      # n = 1, n = 128
    assert proj(buf, buf, buf, w=0.0) == -3 and proj(buf, buf, buf, w=1.5) == -3 and proj(buf, buf, buf, w=-0.5) == -3
    assert b"weight" in lib.diqt_last_error()
    assert proj(buf, buf, buf, mode=3) == -3
    geo = (40, 36, 44, 16, 8, 4, 3, 4)                                          # D, H, W, P, stride and the lattice of range(0, n - 15, 8)

    def step(ptrs=(buf,) * 8, form=0, geo=geo, cell=(2, 2, 2), w=1.0, mode=0):
        return lib.diqt_volume_joint_consistent_step(*ptrs, form, 3, *geo, *cell, w, 1.0, 0.5, 0.0, 0.0, -1.0, 1.0, mode, 0, 1, 0, None)
    for k in (0, 1, 2, 3, 5, 6, 7):                                             # every pointer but x0_prev is required; no initial state
        assert step(tuple(None if i == k else buf for i in range(8))) == -2, k
    assert step(cell=(1, 1, 1)) == -3 and step(cell=(4, 4, 8)) == -3 and step(w=0.0) == -3 and step(w=1.0001) == -3
    assert step(form=3) == -3 and step(mode=2) == -3
    assert step(cell=(3, 1, 1)) == -1 and step(cell=(1, 5, 1)) == -1 and step(cell=(1, 1, 8)) == -1     # D % 3, H % 5, W % 8
    assert b"does not divide" in lib.diqt_last_error()
    assert step(geo=(40, 36, 44, 16, 8, 4, 3, 5)) == -1
    assert b"lattice" in lib.diqt_last_error()


# ---- H4: the launches of a consistent joint chain -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('chain', ['step', 'multistep', 'sigma-base1'])
def test_consistent_joint_chain_makes_the_plain_chains_launches(chain, monkeypatch):
    """Per sample the T fused launches of the plain chain become T ``volume_joint_consistent_step`` launches on the same buffers --
    the initial state, the evaluations, the draws and the finish are the plain chain's -- plus ONE ``cell_replicate`` per call."""
    from tests import test_volume_launch_trace_host as T
    plain_op = {'step': 'volume_joint_step', 'multistep': 'volume_joint_multistep', 'sigma-base1': 'volume_joint_multistep_sde'}[chain]
    from diffusioniqt_amd import ops
    monkeypatch.setitem(T.RETURNS, 'cell_replicate', lambda a: ops.cell_replicate(a['meas'], a['cell']))
    monkeypatch.setitem(T.RETURNS, 'consistency_cell', lambda a: ops.consistency_cell(**a))      # host only: the real rules
    monkeypatch.setitem(T.RETURNS, 'volume_joint_consistent_step', lambda a: (a['out'], a['x0_out']))
    name = f'joint-{chain}-selfcond'
    plain = T.run_case(name)
    case = dict(T.CASES[name])
    state_space = lambda self, x: self.rec.record('state_space', {'x': x}, x)
    monkeypatch.setattr(T.StubDenoiser, 'state_space', state_space, raising=False)
    case['kw'] = dict(case['kw'], consistency=(torch.full((20, 18, 22), 300.0), (2, 2, 2)), consistency_weight=0.5)
    monkeypatch.setitem(T.CASES, name, case)
    got = T.run_case(name)
    a, b = (collections.Counter(r['op'] for r in t) for t in (plain, got))
    T_steps, S = 3, 2
    init = S if chain == 'sigma-base1' else 0                                   # that family makes its first state with the same entry
    assert a[plain_op] == S * T_steps + init and b[plain_op] == init and b['volume_joint_consistent_step'] == S * T_steps
    assert b['cell_replicate'] == 1 and b['state_space'] == 1
    rest = lambda c: {k: v for k, v in c.items() if k not in (plain_op, 'volume_joint_consistent_step', 'cell_replicate', 'consistency_cell', 'state_space')}
    assert rest(a) == rest(b)
    old = [r for r in plain if r['op'] == plain_op and r['x_t'] is not None]
    new = [r for r in got if r['op'] == 'volume_joint_consistent_step']
    # a buffer first seen by the fused launch is tagged with that launch's name: compare such tags by their number
    same = lambda d: {**d, 't': d['t'].replace(plain_op, 'volume_joint_consistent_step')} if isinstance(d, dict) else d
    for o, n in zip(old, new):                                                  # the same buffers, coefficients, clamp and draws
        assert n['form'] == {'step': 0, 'multistep': 1, 'sigma-base1': 2}[chain] and n['cell'] == [2, 2, 2] and n['weight'] == 0.5
        for k in ('y', 'x_t', 'out', 'x0_out', 'kx', 'k0', 'lo', 'hi', 'clamp_mode', 'stride'):
            assert same(o[k]) == same(n[k]), k
        assert n['out']['t'] == n['x_t']['t'] and n['meas_up']['t'] == 'state_space.x#0'   # in place, on the one measurement volume
        if chain != 'step':
            assert same(o['x0_prev']) == same(n['x0_prev']) and o['kp'] == n['kp']
            assert n['x0_prev'] is None or n['x0_prev']['t'] == n['x0_out']['t']
        if chain != 'multistep':
            assert (o['kn'], o['seed'], o['draw'], o['sample']) == (n['kn'], n['seed'], n['draw'], n['sample'])
