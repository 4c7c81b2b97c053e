"""Host-side checks of data-consistent sampling with a slice profile (no GPU here): ``ops.cell_profile`` makes the table of
tests/volume_joint_profile_reference.py bit for bit and refuses what it must, every argument rule of ``consistency_profile=`` is raised
before anything touches the device, the fp32 restatement of the projection is exact rational arithmetic rounded once per operation, and
with a profile every sampler and the joint chain make the launches they made without one -- each ``cell_project`` /
``volume_joint_consistent_step`` replaced by its profile twin on the same operands."""
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import launch_trace as LT
from tests import volume_blend_reference as R
from tests import volume_joint_heun_reference as HN
from tests import volume_joint_profile_reference as PR
from tests.test_volume_joint_host import _imagen

WIDE = ((4, 4, 4), ((0.1, 1, 1, 0.1),) * 3)                  # (0.1, 1, 1, 0.1)^3: n = 64, gains far from 1
TABLES = {**PR.PROFILES, 'wide': WIDE}


# ---- P1: the table ----------------------------------------------------------------------------------------------------------------------
def test_cell_profile_known_tables():
    from diffusioniqt_amd import ops
    t = ops.cell_profile((2, 2, 2), ((1, 1), (1, 1), (1, 1)))
    assert t.dtype == torch.float32 and tuple(t.shape) == (2, 8) and t.is_contiguous() and t.device.type == 'cpu'
    assert t[0].tolist() == [0.125] * 8 and t[1].tolist() == [1.0] * 8                     # the uniform profile: today's operator
    t = ops.cell_profile((4, 1, 1), ([0, 1, 1, 0], [1], [1]))
    assert t[0].tolist() == [0.0, 0.5, 0.5, 0.0] and t[1].tolist() == [0.0, 1.0, 1.0, 0.0]
    assert ops.cell_profile((4, 1, 1), ((0, 7.5, 7.5, 0), (3,), (0.25,))).equal(t)          # the scale of an axis does not matter


@pytest.mark.parametrize('name', list(TABLES))
def test_cell_profile_is_the_reference_table_bit_for_bit(name):
    from diffusioniqt_amd import ops
    cell, profile = TABLES[name]
    got, want = ops.cell_profile(cell, profile).numpy(), PR.profile_table(cell, profile)
    assert got.shape == want.shape == (2, cell[0] * cell[1] * cell[2]) and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    u = got[0].astype(np.float64)
    assert abs(u.sum() - 1) <= 64 * 2.0 ** -24 and abs((u * got[1]).sum() - 1) <= 64 * 2.0 ** -23      # sum u = 1 and u . g = 1


BAD_PROFILES = [None, (1, 1, 1), ((1, 1), (1, 1)), ((1, 1), (1, 1), (1, 1), (1, 1)), ((1, 1, 1), (1, 1), (1, 1)), ((1,), (1, 1), (1, 1)),
                ((1, -1), (1, 1), (1, 1)), ((1, float('nan')), (1, 1), (1, 1)), ((1, float('inf')), (1, 1), (1, 1)),
                ((0, 0), (1, 1), (1, 1)), ((1, 1), (1, 1), (0.0, 0)), ((1, 'a'), (1, 1), (1, 1)), ((1, True), (1, 1), (1, 1)),
                (1.0, (1, 1), (1, 1)), 'abc']


def test_cell_profile_refusals():
    from diffusioniqt_amd import ops
    for bad in BAD_PROFILES:
        with pytest.raises(ValueError, match="consistency"):
            ops.cell_profile((2, 2, 2), bad)
    for cell in ((1, 1, 1), (2, 2), (8, 4, 4), (2.0, 2, 2)):                               # the cell's own rules
        with pytest.raises(ValueError, match="consistency"):
            ops.cell_profile(cell, ((1, 1), (1, 1), (1, 1)))


# ---- P2: argument rules, all before the device is touched -----------------------------------------------------------------------------------
OK_PROFILE = ((1, 2), (1, 1), (3, 1))


def _meas(P=16, B=2):
    return torch.zeros(B, 1, P, P, P)


def test_sample_refuses_a_profile_it_cannot_honour():
    imagen = _imagen()
    lr = torch.zeros(2, 1, 16, 16, 16)
    base = dict(batch_size=2, start_image_or_video=lr, start_at_unet_number=2, use_tqdm=False, sampler='ddim', sample_steps=2)
    ok = (_meas(), (2, 2, 2))
    bad = [dict(consistency_profile=OK_PROFILE),                                           # a profile without consistency
           *[dict(consistency=ok, consistency_profile=p) for p in BAD_PROFILES if p is not None],
           dict(consistency=(_meas(), (4, 1, 1)), consistency_profile=OK_PROFILE),         # the lengths are another cell's
           # every existing refusal stays
           dict(consistency=ok, consistency_profile=OK_PROFILE, consistency_weight=0.0),
           dict(consistency=ok, consistency_profile=OK_PROFILE, init_images=lr),
           dict(consistency=ok, consistency_profile=OK_PROFILE, sampler='ddpm', sample_steps=None, skip_steps=2),
           dict(consistency=ok, consistency_profile=OK_PROFILE, sampler='ddpm', inpaint_images=lr, inpaint_masks=lr[:, 0].bool())]
    for kw in bad:
        with pytest.raises(ValueError, match="consistency"):
            imagen.sample(**{**base, **kw})
    for kw in (dict(consistency_profile=OK_PROFILE), dict(consistency=ok, consistency_profile=((1, 2), (1, 1), (0, 0)))):
        with pytest.raises(ValueError, match="consistency"):                               # the loop itself applies the same rules
            imagen.p_sample_loop(imagen.unets[1], (2, 1, 16, 16, 16), noise_scheduler=imagen.noise_schedulers[1], **kw)


def test_edm_sample_refuses_a_profile_it_cannot_honour():
    elu = HN.make_elucidated('churn-on', False)
    lr = torch.zeros(2, 1, 16, 16, 16)
    base = dict(batch_size=2, video_frames=16, start_image_or_video=lr, start_at_unet_number=2, use_tqdm=False, sampler='dpmpp2m')
    ok = (_meas(), (2, 2, 2))
    bad = [dict(consistency_profile=OK_PROFILE), dict(consistency_profile=OK_PROFILE, sampler='heun'),
           dict(consistency=ok, consistency_profile=((1, 2), (1, 1), (1, -3))), dict(consistency=ok, consistency_profile=((1, 2), (1, 1))),
           dict(consistency=ok, consistency_profile=OK_PROFILE, sampler='heun'),           # every existing refusal stays
           dict(consistency=ok, consistency_profile=OK_PROFILE, init_images=lr),
           dict(consistency=ok, consistency_profile=OK_PROFILE, consistency_weight=2),
           dict(consistency=ok, consistency_profile=OK_PROFILE, sampler='heun', inpaint_images=lr, inpaint_masks=lr[:, 0].bool())]
    for kw in bad:
        with pytest.raises(ValueError, match="consistency"):
            elu.sample(**{**base, **kw})
    for kw in (dict(consistency_profile=OK_PROFILE), dict(consistency=ok, consistency_profile=((0, 0), (1, 1), (1, 1)))):
        with pytest.raises(ValueError, match="consistency"):
            elu.one_unet_sample(elu.unets[1], (2, 1, 16, 16, 16), unet_number=2, sampler='dpmpp2m', **kw)


def test_volume_inference_profile_argument_errors():
    from diffusioniqt_amd.inference import VolumeInference

    def never(x, **kw):
        raise AssertionError("the sampler must not run")
    cfg = R.shared_cfg(8)                                                                  # P 16, stride 8, volume (40, 36, 44)
    meas = torch.zeros(20, 18, 22)
    ok = (meas, (2, 2, 2))
    known = (torch.zeros(40, 36, 44), torch.zeros(40, 36, 44, dtype=torch.bool))
    for kw in (dict(consistency_profile=OK_PROFILE),                                       # a profile without consistency
               dict(consistency=ok, consistency_profile=((1, 2), (1, 1))), dict(consistency=ok, consistency_profile=((1, 2), (1, 1), (1, -1))),
               dict(consistency=ok, consistency_profile=((1, 2, 1), (1, 1), (1, 1))),
               dict(consistency=ok, consistency_profile=OK_PROFILE, inpaint=known),        # every existing refusal stays
               dict(consistency=ok, consistency_profile=OK_PROFILE, consistency_weight=0.0),
               dict(consistency=(meas, (1, 1, 3)), consistency_profile=((1,), (1,), (1, 2, 1)))):      # divisibility: unchanged
        with pytest.raises(ValueError, match="consistency"):
            VolumeInference(cfg, never, **kw)
    with pytest.raises(ValueError, match="consistency"):
        VolumeInference(cfg, HN.make_elucidated('churn-on', False).window_denoiser(), consistency=ok, consistency_profile=OK_PROFILE,
                        blend='gaussian', noise='anchored', joint=True)
    inf = VolumeInference(cfg, never, consistency=ok, consistency_profile=OK_PROFILE)
    assert np.array_equal(inf.consistency_table.numpy(), PR.profile_table((2, 2, 2), OK_PROFILE))
    assert VolumeInference(cfg, never, consistency=ok).consistency_table is None           # the default is today's path


# ---- P3: the fp32 restatement ---------------------------------------------------------------------------------------------------------------
def _rn32(x):
    """A Fraction rounded to the nearest float32, ties to even."""
    near = np.float32(float(x))
    cands = (np.nextafter(near, np.float32(-np.inf)), near, np.nextafter(near, np.float32(np.inf)))
    return min(cands, key=lambda v: (abs(Fraction(float(v)) - x), int(v.view(np.uint32)) & 1))


@pytest.mark.parametrize('w', [1.0, 0.5])
@pytest.mark.parametrize('name', list(TABLES))
def test_project_profile32_is_exact_arithmetic_rounded_once_per_operation(name, w):
    """On random cells: s = rn(u[q] a[q] + s) in order, t = rn(w g[q]), r = rn(meas - s), a' = rn(t r + a), every rn ONE rounding of
    the exact rational value; and, at the reference's own precision, the result is within the one-projection count of float64, the
    w = 1 residual |u . x0' - y| under that count too, and a gap voxel keeps its bits."""
    cell, profile = TABLES[name]
    table = PR.profile_table(cell, profile)
    n = table.shape[1]
    rng = np.random.default_rng(len(name))
    cells = 12 if n < 64 else 3
    shape = (cell[0], cell[1], cell[2] * cells)                                            # `cells` cells along x
    a = (rng.standard_normal(shape) * 2).astype(np.float32)
    meas = PR.replicate(rng.standard_normal((1, 1, cells)).astype(np.float32), cell)
    got = PR.project_profile32(a, meas, cell, table, w)
    F = lambda v: Fraction(float(v))
    for c in range(cells):
        vals = a[:, :, c * cell[2]:(c + 1) * cell[2]].reshape(-1)                          # lexicographic (z, y, x)
        s = np.float32(0)
        for q in range(n):
            s = _rn32(F(table[0, q]) * F(vals[q]) + F(s))
        y = meas[0, 0, c * cell[2]]
        r = _rn32(F(y) - F(s))
        for q in range(n):
            t = _rn32(F(np.float32(w)) * F(table[1, q]))
            want = _rn32(F(t) * F(r) + F(vals[q]))
            have = got[:, :, c * cell[2]:(c + 1) * cell[2]].reshape(-1)[q]
            assert have.view(np.uint32) == want.view(np.uint32), (c, q)
    ones = np.ones(shape, dtype=bool)
    ref, whole = PR.project_profile64(a.astype(np.float64), ones, meas.astype(np.float64), cell, w, table)
    scale = max(float(np.abs(a).max()), float(np.abs(meas).max()), float(np.abs(got).max()))
    count = PR.profile_roundings(cell, table, w, scale)
    err = np.abs(got.astype(np.float64) - ref).max()
    print(f"profile {name} w {w}: fp32 - float64 = {err:.3e}, count {count:.3e} ({err / count:.3f})")
    assert whole.all() and err <= count
    gap = PR.gains(table, cell, shape) == 0
    assert np.array_equal(got.view(np.uint32)[gap], a.view(np.uint32)[gap]) and gap.any() == (name == 'gap')
    assert (got[~gap] != a[~gap]).mean() > 0.9
    if w == 1.0:                                                                           # u . x0' = y
        res = np.abs(PR.cell_wmean64(got, cell, table) - meas[::cell[0], ::cell[1], ::cell[2]]).max()
        assert np.abs(PR.cell_wmean64(ref, cell, table) - meas[::cell[0], ::cell[1], ::cell[2]]).max() <= 1e-6 * scale   # the table's own rounding
        print(f"profile {name}: w = 1 residual {res:.3e}, count {count:.3e}")
        assert res <= count


def test_a_uniform_profile_is_the_uniform_projection_within_the_count():
    from tests import volume_joint_dc_reference as DC
    cell = (2, 2, 2)
    table = PR.profile_table(cell, ((1, 1),) * 3)
    rng = np.random.default_rng(8)
    a = (rng.standard_normal((8, 8, 8)) * 2).astype(np.float32)
    meas = PR.replicate(rng.standard_normal((4, 4, 4)).astype(np.float32), cell)
    got, old = PR.project_profile32(a, meas, cell, table, 1.0), DC.project32(a, meas, cell, 1.0)
    scale = max(float(np.abs(a).max()), float(np.abs(meas).max()), float(np.abs(got).max()))
    assert np.abs(got.astype(np.float64) - old).max() <= PR.profile_roundings(cell, table, 1.0, scale) + DC.projection_roundings(cell, scale)


# ---- P4: routing, with recording stand-ins ----------------------------------------------------------------------------------------------------
HOST_ONLY = ('consistency_cell', 'cell_profile')


def _as_uniform(trace, new, old):
    """The canonical trace with every ``new`` record turned into the ``old`` record it stands for: the table operand dropped (it must be
    the one [2, n] table of the chain), the op and the buffer tags made from its name renamed.  Host-only calls are left out."""
    out, tables = [], set()
    for r in trace:
        if r['op'] in HOST_ONLY:
            continue
        r = dict(r)
        if r['op'] == new:
            t = r.pop('table')
            tables.add((t['t'], tuple(t['shape']), t['dtype']))
        out.append(r)
    return LT.canonical(out).replace(new, old), tables


def _imagen_trace(sampler, eta, profile):
    from diffusioniqt_amd import imagen_pytorch3D, ops
    into = lambda key: (lambda a: a['out'] if a.get('out') is not None else torch.zeros_like(a[key]))
    returns = {'axpby3': lambda a: torch.zeros_like(a['a']), 'ddpm_step': lambda a: (torch.zeros_like(a['x_t']), torch.zeros_like(a['x_t'])),
               'cell_project': into('x0'), 'cell_project_profile': into('x0'),
               'consistency_cell': lambda a: ops.consistency_cell(**a), 'cell_profile': lambda a: ops.cell_profile(**a)}
    rec = LT.Recorder()
    imagen = _imagen()
    lr, meas = torch.zeros(2, 1, 16, 16, 16), torch.full((2, 1, 16, 16, 16), 0.125)
    rec.tag(lr, 'lowres'), rec.tag(meas, 'meas_up')
    noise = [LT.zeros(2, 1, 16, 16, 16) for _ in range(8)]
    for k, t in enumerate(noise):
        rec.tag(t, f'noise{k}')
    kw = dict(consistency=(meas, (2, 2, 4)), consistency_weight=0.5)
    if profile is not None:
        kw.update(consistency_profile=profile)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(imagen_pytorch3D, 'ops', LT.RecordingOps(rec, returns))
        out = imagen.sample(batch_size=2, start_image_or_video=lr, start_at_unet_number=2, use_tqdm=False, device='cpu', sampler=sampler,
                            sample_steps=3, eta=eta, noise=noise, **kw)[0]
    rec.record('return', {}, out)
    return rec.trace


@pytest.mark.parametrize('sampler,eta', [('ddim', 0.0), ('ddim', 0.5), ('ddpm', 0.0), ('dpmpp2m', 0.0)])
def test_imagen_sample_with_a_profile_makes_the_same_launches(sampler, eta):
    plain = _imagen_trace(sampler, eta, None)
    got = _imagen_trace(sampler, eta, ((1, 2), (1, 1), (1, 3, 3, 1)))
    assert sum(r['op'] == 'cell_project' for r in plain) == 3 and not any(r['op'] == 'cell_project_profile' for r in plain)
    assert sum(r['op'] == 'cell_project_profile' for r in got) == 3 and not any(r['op'] == 'cell_project' for r in got)
    a, none = _as_uniform(plain, 'cell_project_profile', 'cell_project')
    b, tables = _as_uniform(got, 'cell_project_profile', 'cell_project')
    assert a == b and not none and len(tables) == 1 and next(iter(tables))[1:] == ((2, 16), 'torch.float32')


@pytest.mark.parametrize('eta,self_cond', [(0.0, False), (0.5, True)])
def test_edm_sample_with_a_profile_makes_the_same_launches(eta, self_cond, monkeypatch):
    from tests import test_edm_sampler_trace_host as T
    monkeypatch.setitem(T.RETURNS, 'cell_project_profile', T._into('x0'))
    base = dict(model=dict(self_cond=self_cond), sampler='dpmpp2m', eta=eta, consistency=0.5)
    monkeypatch.setitem(T.CASES, 'profile-off', T.sample_case(**base))
    monkeypatch.setitem(T.CASES, 'profile-on', T.sample_case(**base, consistency_profile=((1, 2), (1, 1), (1, 3, 3, 1))))
    plain, got = T.run_case('profile-off')[0], T.run_case('profile-on')[0]
    steps = sum(r['op'] == 'multistep_sde_step' for r in plain)
    assert steps > 0 and sum(r['op'] == 'cell_project' for r in plain) == steps
    assert sum(r['op'] == 'cell_project_profile' for r in got) == steps and not any(r['op'] == 'cell_project' for r in got)
    a, none = _as_uniform(plain, 'cell_project_profile', 'cell_project')
    b, tables = _as_uniform(got, 'cell_project_profile', 'cell_project')
    assert a == b and not none and len(tables) == 1 and next(iter(tables))[1:] == ((2, 16), 'torch.float32')


def _volume_case(monkeypatch, name, fn=None, **extra):
    """One ``VolumeInference`` case of the launch-trace module with consistency (and what ``extra`` adds) switched on."""
    from diffusioniqt_amd import ops
    from tests import test_volume_launch_trace_host as T
    monkeypatch.setitem(T.RETURNS, 'cell_replicate', lambda a: ops.cell_replicate(a['meas'], a['cell']))
    monkeypatch.setitem(T.RETURNS, 'consistency_cell', lambda a: ops.consistency_cell(**a))
    monkeypatch.setitem(T.RETURNS, 'cell_profile', lambda a: ops.cell_profile(**a))
    for op in ('volume_joint_consistent_step', 'volume_joint_consistent_profile_step'):
        monkeypatch.setitem(T.RETURNS, op, lambda a: (a['out'], a['x0_out']))
    monkeypatch.setattr(T.StubDenoiser, 'state_space', lambda self, x: self.rec.record('state_space', {'x': x}, x), raising=False)
    case = dict(T.CASES[name])
    case['kw'] = dict(case['kw'], consistency=(torch.full((20, 18, 22), 300.0), (2, 2, 2)), consistency_weight=0.5, **extra)
    if fn is not None:
        case['fn'] = fn
    monkeypatch.setitem(T.CASES, 'profile-case', case)
    return T.run_case('profile-case')


@pytest.mark.parametrize('chain', ['step', 'multistep', 'sigma-base1'])
def test_joint_chain_with_a_profile_makes_the_same_launches(chain, monkeypatch):
    name = f'joint-{chain}-selfcond'
    plain = _volume_case(monkeypatch, name)
    got = _volume_case(monkeypatch, name, consistency_profile=OK_PROFILE)
    old, new = 'volume_joint_consistent_step', 'volume_joint_consistent_profile_step'
    launches = sum(r['op'] == old for r in plain)
    assert launches == 2 * 3 and not any(r['op'] == new for r in plain)                    # S = 2 samples of T = 3 steps
    assert sum(r['op'] == new for r in got) == launches and not any(r['op'] == old for r in got)
    a, none = _as_uniform(plain, new, old)
    b, tables = _as_uniform(got, new, old)
    assert a == b and not none and len(tables) == 1 and next(iter(tables))[1:] == ((2, 8), 'torch.float32')


@pytest.mark.parametrize('profile', [None, OK_PROFILE])
def test_blend_mode_hands_the_profile_on_exactly_when_one_was_given(profile, monkeypatch):
    seen = []

    def sampler_of(rec):
        def sample(x, noise=None, **kw):
            seen.append(kw)
            return torch.zeros_like(x)
        return sample
    extra = {} if profile is None else dict(consistency_profile=profile)
    _volume_case(monkeypatch, 'blend-gaussian-s2-anchored', fn=sampler_of, **extra)
    assert seen
    for kw in seen:
        assert set(kw) == {'consistency', 'consistency_weight'} | set(extra)
        assert profile is None or kw['consistency_profile'] == profile
