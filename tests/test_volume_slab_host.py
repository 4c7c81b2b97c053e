"""Host-side checks of data consistency for overlapping slice profiles (no GPU here): ``ops.slab_profile`` against
tests/volume_joint_slab_reference.py bit for bit and every refusal of ``consistency_slab=`` raised before anything touches the device;
the fp32 restatement of the kernels' arithmetic against the float64 specification (a dense pseudo-inverse) on the inputs of the GPU
tests, within a quarter of the derived rounding allowance; the guarantee A_act x0' = y_act at w = 1; the error codes of the four new
entries; and -- with recording stand-ins -- the keyword reaching ``ops.slab_project`` once per step in both sampler families, the
crop / blend modes handing it on, and the joint chain dispatching its two ops per step."""
import numpy as np
import pytest
import torch

from tests import launch_trace as LT
from tests import volume_joint_dc_reference as DC
from tests import volume_joint_heun_reference as HN
from tests import volume_joint_slab_reference as SL
from tests.test_volume_joint_host import _imagen

PZ4 = [0.25, 1.0, 1.0, 0.25]                                                              # fz = 2, r = 1
SLAB222 = (PZ4, [1.0, 0.5], [0.75, 1.0])
SLAB224 = (PZ4, [1.0, 1.0], [1.0, 2.0, 2.0, 1.0])


# ---- S1: the host table ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', range(len(SL.PROJECT_CASES)))
def test_slab_profile_is_the_reference_table_bit_for_bit(case):
    from diffusioniqt_amd import ops
    cell, profile, P = SL.PROJECT_CASES[case]
    for jmax in (1, P // cell[0], 40):
        tab, want = ops.slab_profile(cell, profile, jmax=jmax), SL.table(cell, profile, jmax)
        assert (tab.cell, tab.reach, tab.jmax) == (cell, want['r'], jmax) and tab.table.dtype == torch.float32
        assert tab.table.is_contiguous() and tab.table.device.type == 'cpu'
        assert np.array_equal(tab.table.numpy().view(np.uint32), SL.flat(want).view(np.uint32))
        for name in ('uz', 'uyx', 'gyx', 'm', 'ip'):
            assert np.array_equal(tab.part(name).numpy().view(np.uint32), want[name].view(np.uint32)), name
        assert tab.part('m')[0] == 0 and tab.cond == want['kappa'] and 1 <= tab.cond <= 128
        assert abs(float(tab.part('uz').double().sum()) - 1) <= 1e-6 and abs(float(tab.part('uyx').double().sum()) - 1) <= 1e-6
        assert 0 <= tab.e <= tab.d / 2
    # the pivots converge: the table of a long run repeats its last entries
    long = ops.slab_profile(cell, profile, jmax=64)
    assert long.part('ip')[-1] == long.part('ip')[-2] and long.part('m')[-1] == long.part('m')[-2]


def test_slab_profile_refusals():
    from diffusioniqt_amd import ops
    ok_y, ok_x = [1.0, 1.0], [1.0]
    bad = [None, 'abc', (PZ4, ok_y), (PZ4, ok_y, ok_x, ok_x), (PZ4, None, ok_x),
           ([1.0, 1.0], ok_y, ok_x),                                                        # no reach at all
           ([0.5, 1.0, 0.5], ok_y, ok_x),                                                   # fz + 1: not fz + 2r
           ([0.1, 0.5, 1.0, 1.0, 0.5, 0.1], ok_y, ok_x),                                    # r = 2 > fz / 2
           ([0.5, 1.0, -1.0, 0.5], ok_y, ok_x), ([0.5, float('nan'), 1.0, 0.5], ok_y, ok_x), ([0.5, float('inf'), 1.0, 0.5], ok_y, ok_x),
           ([0.5, True, 1.0, 0.5], ok_y, ok_x), ([0.0] * 4, ok_y, ok_x), (PZ4, [0.0, 0.0], ok_x), (PZ4, [1.0], ok_x), (PZ4, ok_y, [1.0, 1.0]),
           ([1.0, 1.0, 1.0, 1.0], ok_y, ok_x),                                              # flat across the border: d - 2e = 0
           ([0.84, 1.0, 1.0, 0.84], ok_y, ok_x)]                                            # just past the rule: it binds at 0.8370
    for profile in bad:
        with pytest.raises(ValueError, match="consistency"):
            ops.slab_profile((2, 2, 1), profile)
    with pytest.raises(ValueError, match="d - 2e"):
        ops.slab_profile((2, 2, 1), bad[-1])
    assert 100 < ops.slab_profile((2, 2, 1), ([0.83, 1.0, 1.0, 0.83], ok_y, ok_x)).cond <= 128
    for cell in ((1, 1, 1), (2, 2), (8, 4, 4), (2.0, 1, 1)):                               # the cell's own rules
        with pytest.raises(ValueError, match="consistency"):
            ops.slab_profile(cell, (PZ4, ok_y, ok_x))
    with pytest.raises(ValueError, match="consistency"):
        ops.slab_profile((1, 2, 1), ([0.5, 1.0, 0.5], ok_y, ok_x))                          # fz = 1 admits no reach (2r <= fz)
    for jmax in (0, -1, 2.0, True, 70000):
        with pytest.raises(ValueError, match="consistency_slab"):
            ops.slab_profile((2, 2, 1), (PZ4, ok_y, ok_x), jmax=jmax)
    with pytest.raises(ValueError, match="consistency_slab.*LDS"):
        ops.slab_plan("who", (2, 1, 1), 130)
    ops.slab_plan("who", (2, 1, 1), 128)
    assert ops.slab_lds((2, 1, 1), 128) == 65536


def test_the_condition_rule_is_a_rule_on_the_input():
    """d - 2e >= d / 64 and e <= d / 2 bound the condition number of every run by (d + 2e) / (d - 2e) <= 128."""
    from diffusioniqt_amd import ops
    for edge in (0.1, 0.5, 0.8, 0.83):
        tab = ops.slab_profile((2, 1, 2), ([edge, 1.0, 1.0, edge], [1.0], [1.0, 1.0]), jmax=12)
        n = 12
        G = tab.d * np.eye(n) + tab.e * (np.eye(n, k=1) + np.eye(n, k=-1))
        assert np.linalg.cond(G) <= tab.cond <= 128
        # the tabulated pivots are those of G's LDL^T
        piv = [G[0, 0]]
        for j in range(1, n):
            piv.append(G[j, j] - G[j, j - 1] ** 2 / piv[-1])
        assert np.allclose(1.0 / tab.part('ip').double().numpy(), piv, rtol=1e-6)


# ---- S2: the restatement is the specification, within a quarter of the derived allowance -------------------------------------------------------
@pytest.mark.parametrize('case', range(len(SL.PROJECT_CASES)))
@pytest.mark.parametrize('w', [1.0, 0.5])
def test_project_restatement_is_the_float64_projection(case, w):
    cell, profile, P = SL.PROJECT_CASES[case]
    tab = SL.table(cell, profile, P // cell[0])
    x0, meas = SL.project_inputs(cell, P)
    got = SL.project32(x0, meas, tab, w)
    err = scale = 0.0
    for b in range(x0.shape[0]):
        ref, touched = SL.project64(x0[b, 0], meas[b, 0], tab, w)
        err = max(err, float(np.abs(got[b, 0] - ref).max()))
        scale = max(scale, float(np.abs(ref).max()), float(np.abs(x0[b]).max()), float(np.abs(meas[b]).max()))
        # voxels under no active row keep their bits; with r >= 1 those are the outer fz - r planes at both ends of the cube
        assert np.array_equal(got[b, 0][~touched].view(np.uint32), x0[b, 0][~touched].view(np.uint32))
        assert touched[cell[0] - tab['r']:P - cell[0] + tab['r']].all() and not touched[:cell[0] - tab['r']].any()
        assert not touched[P - cell[0] + tab['r']:].any()
    allowance = SL.slab_roundings(tab, scale)
    print(f"slab {cell} r {tab['r']} w {w}: fp32 - float64 = {err:.3e} at scale {scale:.2f}, allowance {allowance:.3e} "
          f"({err / allowance:.4f}), condition bound {tab['kappa']:.2f}")
    assert err <= allowance / 4 and (got != x0).mean() > 0.5


def test_the_documented_case():
    """Cell (4, 2, 2), r = 2, D = 32, a Gaussian-like pz, one uncovered plane: the figures of DESIGN 4.16."""
    cell, P = (4, 2, 2), 32
    tab = SL.table(cell, (SL.gaussian_pz(4, 2), [1.0, 0.5], [0.75, 1.0]), P // 4)
    rng = np.random.default_rng(11)
    x0 = (rng.standard_normal((P, 8, 8)) * 1.5).astype(np.float32)
    meas = DC.replicate(rng.standard_normal((P // 4, 4, 4)).astype(np.float32), cell)
    covered = np.ones(x0.shape, dtype=bool)
    covered[13] = False                                                                    # rows 2 and 3 lose their support: two runs
    got = SL.project32(x0, meas, tab, 1.0, covered)
    ref, touched = SL.project64(x0, meas, tab, 1.0, covered)
    act = SL.active_rows(tab, covered)
    assert act[:, 0, 0].tolist() == [False, True, False, False, True, True, True, False]
    err, scale = float(np.abs(got - ref).max()), max(float(np.abs(ref).max()), float(np.abs(x0).max()), float(np.abs(meas).max()))
    allowance = SL.slab_roundings(tab, scale)
    print(f"documented case: fp32 - float64 = {err:.3e} at scale {scale:.2f}, allowance {allowance:.3e}, bound {tab['kappa']:.2f}")
    assert err <= allowance / 4 and 2 <= tab['kappa'] <= 3
    assert np.array_equal(got[~touched].view(np.uint32), x0[~touched].view(np.uint32)) and not touched[10:14].any()
    assert touched[2:10].all() and touched[14:30].all()                                     # rows 1 and 4 .. 6 reach planes 2 .. 9, 14 .. 29


@pytest.mark.parametrize('stride,kind', DC.STEP_TILINGS)
@pytest.mark.parametrize('cell,profile', [((4, 1, 1), SL.PROJECT_CASES[2][1]), ((2, 1, 1), SL.PROJECT_CASES[0][1]),
                                          ((2, 3, 1), SL.PROJECT_CASES[4][1])])
def test_joint_restatement_is_the_float64_projection(stride, kind, cell, profile):
    """On ``step_case``'s volume, whose dropped windows restart runs inside columns."""
    case = DC.step_case(stride, kind)
    tab = SL.table(cell, profile, DC.STEP_VOL[0] // cell[0])
    meas = DC.step_meas(case, cell)
    x0, covered = DC.fuse32(case['y'], case['slot'], case['taps'], stride, DC.STEP_VOL, DC.clamp32(-2.0, 2.0, 1))
    got = SL.project32(x0, meas, tab, 1.0, covered)
    ref, touched = SL.project64(x0, meas, tab, 1.0, covered)
    act = SL.active_rows(tab, covered)
    runs = {tuple(act[:, cy, cx]) for cy in range(act.shape[1]) for cx in range(act.shape[2])}
    assert len(runs) > 1 and act.any() and not act[0].any() and not act[-1].any()
    err = float(np.abs(got - ref)[covered].max())
    scale = max(float(np.abs(ref[covered]).max()), float(np.abs(meas).max()))
    allowance = SL.slab_roundings(tab, scale)
    print(f"joint {cell} stride {stride}: fp32 - float64 = {err:.3e}, allowance {allowance:.3e} ({err / allowance:.4f}), "
          f"{len(runs)} activity patterns")
    assert err <= allowance / 4
    assert np.array_equal(got[~touched].view(np.uint32), x0[~touched].view(np.uint32))
    # the measured rows land on the measurement
    res = np.abs(SL.measure64(got.astype(np.float64) * covered, tab) - meas[::cell[0], ::cell[1], ::cell[2]])[act].max()
    assert res <= allowance


@pytest.mark.parametrize('case', range(len(SL.PROJECT_CASES)))
def test_the_guarantee_at_weight_one(case):
    """A_act x0' = y_act within the allowance, and the measurement operator's restatement is the float64 operator."""
    cell, profile, P = SL.PROJECT_CASES[case]
    tab = SL.table(cell, profile, P // cell[0])
    x0, meas = SL.project_inputs(cell, P)
    got = SL.project32(x0, meas, tab, 1.0)
    scale = max(float(np.abs(got).max()), float(np.abs(x0).max()), float(np.abs(meas).max()))
    for b in range(x0.shape[0]):
        y = meas[b, 0][::cell[0], ::cell[1], ::cell[2]]
        before = np.abs(SL.measure64(x0[b, 0], tab) - y)[1:-1].max()
        after = np.abs(SL.measure64(got[b, 0], tab) - y)[1:-1].max()
        assert after <= SL.slab_roundings(tab, scale) < before
        m32 = SL.measure32(x0[b, 0], tab)
        assert np.abs(m32 - SL.measure64(x0[b, 0], tab)).max() <= (cell[1] * cell[2] + cell[0] + 2 * tab['r']) * 2.0 ** -24 * scale


# ---- S3: the error codes of the entries ---------------------------------------------------------------------------------------------------------
def test_slab_entries_return_error_codes():
    from diffusioniqt_amd import _lib
    lib = _lib.load()
    buf = (np.zeros(4, dtype=np.int32)).ctypes.data                             # never dereferenced: every call below is refused

    def measure(ptrs=(buf,) * 3, vol=(8, 8, 8), cell=(2, 2, 2), r=1, jmax=4):
        return lib.diqt_slab_measure(*ptrs, *vol, *cell, r, jmax, None)
    for k in range(3):
        assert measure(tuple(None if i == k else buf for i in range(3))) == -2, k
    assert b"null pointer" in lib.diqt_last_error()
    assert measure(cell=(1, 1, 1)) == -3 and measure(cell=(8, 8, 2)) == -3 and measure(r=0) == -3 and measure(r=2) == -3
    assert measure(jmax=0) == -3 and measure(cell=(3, 1, 1)) == -1 and measure(vol=(8, 0, 8)) == -1

    def proj(ptrs=(buf,) * 4, cubes=3, P=8, cell=(2, 2, 2), r=1, jmax=4, w=1.0, mode=2):
        return lib.diqt_slab_project(*ptrs, cubes, P, *cell, r, jmax, w, -1.0, 1.0, mode, None)
    for k in range(4):
        assert proj(tuple(None if i == k else buf for i in range(4))) == -2, k
    assert proj(w=0.0) == -3 and proj(w=1.5) == -3 and proj(mode=3) == -3 and proj(r=0) == -3 and proj(r=2) == -3
    assert proj(cell=(1, 1, 1)) == -3 and proj(cell=(2, 1, 3)) == -1 and proj(cubes=0) == -1
    assert proj(jmax=3) == -1 and b"run positions" in lib.diqt_last_error()
    assert proj(P=130, cell=(2, 1, 1), jmax=65) == -1 and b"LDS" in lib.diqt_last_error()     # 65 slices: 66560 bytes
    geo = (40, 36, 44, 16, 8, 4, 3, 4)                                          # D, H, W, P, stride and the lattice of range(0, n - 15, 8)
    need = (2 * 40 + 20) * 18 * 22

    def coeffs(ptrs=(buf,) * 6, coef=buf, floats=need, geo=geo, cell=(2, 2, 2), r=1, jmax=20, mode=0):
        return lib.diqt_volume_joint_slab_coeffs(*ptrs, floats, coef, 3, *geo, *cell, r, jmax, -1.0, 1.0, mode, None)
    for k in range(6):
        assert coeffs(tuple(None if i == k else buf for i in range(6))) == -2, k
    assert coeffs(coef=None) == -2 and coeffs(r=0) == -3 and coeffs(cell=(1, 1, 1)) == -3 and coeffs(mode=2) == -3
    assert coeffs(cell=(3, 1, 1), r=1) == -1 and coeffs(geo=(40, 36, 44, 16, 8, 4, 3, 5)) == -1
    assert coeffs(jmax=19) == -1 and coeffs(floats=need - 1) == -1 and b"workspace" in lib.diqt_last_error()

    def step(ptrs=(buf,) * 8, outs=(buf, buf), floats=need, form=0, geo=geo, cell=(2, 2, 2), r=1, jmax=20, w=1.0, mode=0):
        return lib.diqt_volume_joint_consistent_slab_step(*ptrs, floats, *outs, form, 3, *geo, *cell, r, jmax, w, 1.0, 0.5, 0.0, 0.25,
                                                          -1.0, 1.0, mode, 0, 1, 0, None)
    assert step(form=3) == -3 and step(form=-1) == -3 and step(w=0.0) == -3 and step(r=2) == -3 and step(mode=2) == -3
    for k in (0, 1, 2, 3, 5, 6, 7):                                             # x0_prev alone may be NULL
        assert step(tuple(None if i == k else buf for i in range(8))) == -2, k
    assert step(outs=(None, buf)) == -2 and step(outs=(buf, None)) == -2
    assert step(cell=(3, 1, 1)) == -1 and step(geo=(40, 36, 44, 16, 8, 4, 3, 5)) == -1 and step(jmax=19) == -1
    assert step(floats=need - 1) == -1


# ---- S4: argument rules, all before the device is touched --------------------------------------------------------------------------------------
def _meas(P=16, B=2):
    return torch.zeros(B, 1, P, P, P)


def test_sample_refuses_a_slab_it_cannot_honour():
    imagen = _imagen()
    lr = torch.zeros(2, 1, 16, 16, 16)
    base = dict(batch_size=2, start_image_or_video=lr, start_at_unet_number=2, use_tqdm=False, sampler='ddim', sample_steps=2)
    ok = (_meas(), (2, 2, 2))
    named = [dict(consistency_slab=SLAB222),                                               # a slab without consistency
             dict(consistency=ok, consistency_slab=SLAB222, consistency_profile=((1, 2), (1, 1), (3, 1))),
             dict(consistency=ok, consistency_slab=SLAB222, consistency_noise=0.1, eta=0.5),
             dict(consistency=ok, consistency_slab=SLAB222, consistency_operator=np.full((1, 8), 0.125)),
             dict(consistency=ok, consistency_slab=SLAB222, consistency_operator=np.full((1, 8), 0.125), consistency_row_noise=0.1,
                  eta=0.5),
             dict(consistency=ok, consistency_slab=([1.0, 1.0], [1.0, 1.0], [1.0, 1.0])),   # a bad reach
             dict(consistency=ok, consistency_slab=([1.0] * 4, [1.0, 1.0], [1.0, 1.0])),    # the condition rule
             dict(consistency=ok, consistency_slab=SLAB222, consistency_weight=0.0),        # what consistency refuses names it too
             dict(consistency=ok, consistency_slab=SLAB222, init_images=lr),
             dict(consistency=ok, consistency_slab=SLAB222, sampler='ddpm', sample_steps=None, skip_steps=2),
             dict(consistency=ok, consistency_slab=SLAB222, sampler='ddpm', inpaint_images=lr, inpaint_masks=lr[:, 0].bool()),
             dict(consistency=(_meas(), (4, 1, 1)), consistency_slab=SLAB222)]              # made for another cell
    for kw in named:
        with pytest.raises(ValueError, match="consistency_slab"):
            imagen.sample(**{**base, **kw})
    kept = [(dict(consistency_weight=0.0), "consistency weight"), (dict(init_images=lr), "neither init_images nor skip_steps"),
            (dict(sampler='ddpm', inpaint_images=lr, inpaint_masks=lr[:, 0].bool()), "inpainting are not offered together")]
    for kw, wording in kept:                                                               # every existing refusal keeps its wording
        with pytest.raises(ValueError, match=wording):
            imagen.sample(**{**base, 'consistency': ok, 'consistency_slab': SLAB222, **kw})
    for kw in (dict(consistency_slab=SLAB222), dict(consistency=ok, consistency_slab=(PZ4, [1.0], [1.0]))):
        with pytest.raises(ValueError, match="consistency_slab"):                          # the loop itself applies the same rules
            imagen.p_sample_loop(imagen.unets[1], (2, 1, 16, 16, 16), noise_scheduler=imagen.noise_schedulers[1], **kw)


def test_edm_sample_refuses_a_slab_it_cannot_honour():
    elu = HN.make_elucidated('churn-on', False)
    lr = torch.zeros(2, 1, 16, 16, 16)
    base = dict(batch_size=2, video_frames=16, start_image_or_video=lr, start_at_unet_number=2, use_tqdm=False, sampler='dpmpp2m',
                sample_steps=3)
    ok = (_meas(), (2, 2, 2))
    named = [dict(consistency_slab=SLAB222), dict(consistency=ok, consistency_slab=SLAB222, sampler='heun', sample_steps=None),
             dict(consistency=ok, consistency_slab=SLAB222, consistency_profile=((1, 2), (1, 1), (3, 1))),
             dict(consistency=ok, consistency_slab=SLAB222, consistency_noise=0.1, eta=0.5),
             dict(consistency=ok, consistency_slab=SLAB222, consistency_operator=np.full((1, 8), 0.125)),
             dict(consistency=ok, consistency_slab=([1.0] * 4, [1.0, 1.0], [1.0, 1.0])),
             dict(consistency=ok, consistency_slab=SLAB222, init_images=lr)]
    for kw in named:
        with pytest.raises(ValueError, match="consistency_slab"):
            elu.sample(**{**base, **kw})
    with pytest.raises(ValueError, match="Heun sampler"):
        elu.sample(**{**base, **named[1]})


def _volume_inference(**kw):
    from diffusioniqt_amd.inference import VolumeInference
    from tests import volume_blend_reference as R
    return VolumeInference(R.shared_cfg(8), lambda x, **k: x, **kw)


def test_volume_inference_refuses_a_slab_it_cannot_honour():
    meas = torch.zeros(20, 18, 22)
    ok = dict(consistency=(meas, (2, 2, 2)), consistency_slab=SLAB222)
    assert _volume_inference(**ok).consistency_slab is SLAB222
    named = [dict(consistency_slab=SLAB222), {**ok, 'consistency_profile': ((1, 2), (1, 1), (3, 1))}, {**ok, 'consistency_noise': 0.1},
             {**ok, 'consistency_operator': np.full((1, 8), 0.125)},
             {**ok, 'consistency_operator': np.full((1, 8), 0.125), 'consistency_row_noise': 0.1},
             {**ok, 'consistency_slab': ([1.0, 1.0], [1.0, 1.0], [1.0, 1.0])}, {**ok, 'consistency_slab': ([1.0] * 4, [1.0, 1.0], [1.0, 1.0])},
             {**ok, 'consistency_weight': 2.0}, {**ok, 'inpaint': (torch.zeros(40, 36, 44), torch.zeros(40, 36, 44, dtype=torch.bool))},
             {**ok, 'consistency': (meas, (16, 2, 2)), 'consistency_slab': ([0.5] * 8 + [1.0] * 16 + [0.5] * 8, [1.0, 1.0], [1.0, 1.0])}]
    for kw in named:
        with pytest.raises(ValueError, match="consistency_slab"):
            _volume_inference(**kw)
    vi = _volume_inference(**ok)
    with pytest.raises(ValueError, match="consistency_slab"):                               # the measurement of another volume
        vi(torch.zeros(40, 36, 40))


# ---- S5: routing, with recording stand-ins --------------------------------------------------------------------------------------------------------
def _real(name):
    from diffusioniqt_amd import ops
    return lambda a: getattr(ops, name)(**a)


HOST = {name: _real(name) for name in ('consistency_cell', 'slab_profile', 'slab_plan')}


def _imagen_trace(sampler, eta, slab):
    from diffusioniqt_amd import imagen_pytorch3D
    into = lambda key: (lambda a: a['out'] if a.get('out') is not None else torch.zeros_like(a[key]))
    returns = {'axpby3': lambda a: torch.zeros_like(a['a']), 'ddpm_step': lambda a: (torch.zeros_like(a['x_t']), torch.zeros_like(a['x_t'])),
               'cell_project': into('x0'), 'slab_project': into('x0'), **HOST}
    rec = LT.Recorder()
    imagen = _imagen()
    lr, meas = torch.zeros(2, 1, 16, 16, 16), torch.full((2, 1, 16, 16, 16), 0.125)
    rec.tag(lr, 'lowres'), rec.tag(meas, 'meas_up')
    noise = [LT.zeros(2, 1, 16, 16, 16) for _ in range(8)]
    for k, t in enumerate(noise):
        rec.tag(t, f'noise{k}')
    kw = dict(consistency=(meas, (2, 2, 4)), consistency_weight=0.5)
    if slab is not None:
        kw.update(consistency_slab=slab)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(imagen_pytorch3D, 'ops', LT.RecordingOps(rec, returns))
        imagen.sample(batch_size=2, start_image_or_video=lr, start_at_unet_number=2, use_tqdm=False, device='cpu', sampler=sampler,
                      sample_steps=3, eta=eta, noise=noise, **kw)
    return rec.trace


def _launches(trace):
    return [r for r in trace if r['op'] not in HOST]


@pytest.mark.parametrize('sampler,eta', [('ddim', 0.0), ('ddim', 0.5), ('ddpm', 0.0), ('dpmpp2m', 0.0)])
def test_imagen_sample_projects_with_the_slab_once_per_step(sampler, eta):
    plain, got = _launches(_imagen_trace(sampler, eta, None)), _launches(_imagen_trace(sampler, eta, SLAB224))
    assert sum(r['op'] == 'cell_project' for r in plain) == 3 and not any(r['op'] == 'slab_project' for r in plain)
    assert sum(r['op'] == 'slab_project' for r in got) == 3 and not any(r['op'] == 'cell_project' for r in got)
    tables = {r.pop('table') for r in got if r['op'] == 'slab_project'}                     # ONE table per chain, made for its cubes
    assert len(tables) == 1 and 'SlabTable(cell=(2, 2, 4), reach=1, jmax=8' in next(iter(tables))
    # the same launches on the same operands: only the op (and the buffer tags made from its name) differs
    assert LT.canonical(got).replace('slab_project', 'cell_project') == LT.canonical(plain)


@pytest.mark.parametrize('eta,self_cond', [(0.0, False), (0.5, True)])
def test_edm_sample_projects_with_the_slab_once_per_step(eta, self_cond, monkeypatch):
    from tests import test_edm_sampler_trace_host as T
    monkeypatch.setitem(T.RETURNS, 'slab_project', T._into('x0'))
    base = dict(model=dict(self_cond=self_cond), sampler='dpmpp2m', eta=eta, consistency=0.5)
    monkeypatch.setitem(T.CASES, 'slab-off', T.sample_case(**base))
    monkeypatch.setitem(T.CASES, 'slab-on', T.sample_case(**base, consistency_slab=SLAB224))
    plain, got = T.run_case('slab-off')[0], T.run_case('slab-on')[0]
    steps = sum(r['op'] == 'multistep_sde_step' for r in plain)
    assert steps > 0 and sum(r['op'] == 'cell_project' for r in plain) == steps
    assert sum(r['op'] == 'slab_project' for r in got) == steps and not any(r['op'] == 'cell_project' for r in got)
    assert [r['op'].replace('slab_project', 'cell_project') for r in got] == [r['op'] for r in plain]


def _volume_case(monkeypatch, name, fn=None, slab=None):
    """One ``VolumeInference`` case of the launch-trace module with consistency (and the slab, if any) switched on."""
    from diffusioniqt_amd import ops
    from tests import test_volume_launch_trace_host as T
    monkeypatch.setitem(T.RETURNS, 'cell_replicate', lambda a: ops.cell_replicate(a['meas'], a['cell']))
    for host in HOST:
        monkeypatch.setitem(T.RETURNS, host, HOST[host])
    monkeypatch.setitem(T.RETURNS, 'slab_workspace', lambda a: (LT.zeros((2 * 40 + 20) * 18 * 22), LT.zeros(20, 18, 22)))
    monkeypatch.setitem(T.RETURNS, 'volume_joint_slab_coeffs', lambda a: a['coef'])
    for op in ('volume_joint_consistent_step', 'volume_joint_consistent_slab_step'):
        monkeypatch.setitem(T.RETURNS, op, lambda a: (a['out'], a['x0_out']))
    monkeypatch.setattr(T.StubDenoiser, 'state_space', lambda self, x: self.rec.record('state_space', {'x': x}, x), raising=False)
    case = dict(T.CASES[name])
    extra = dict(consistency=(torch.full((20, 18, 22), 300.0), (2, 2, 2)))
    if slab is not None:
        extra.update(consistency_slab=slab)
    case['kw'] = dict(case['kw'], consistency_weight=0.5, **extra)
    if fn is not None:
        case['fn'] = fn
    monkeypatch.setitem(T.CASES, 'slab-case', case)
    return T.run_case('slab-case')


@pytest.mark.parametrize('chain', ['step', 'multistep', 'sigma-base1'])
def test_joint_chain_dispatches_the_two_slab_ops_per_step(chain, monkeypatch):
    name = f'joint-{chain}-selfcond'
    plain = _launches(_volume_case(monkeypatch, name))
    got = _launches(_volume_case(monkeypatch, name, slab=SLAB222))
    old, new, pre = 'volume_joint_consistent_step', 'volume_joint_consistent_slab_step', 'volume_joint_slab_coeffs'
    launches = sum(r['op'] == old for r in plain)
    assert launches == 2 * 3 and not any(r['op'] in (new, pre) for r in plain)              # S = 2 samples of T = 3 steps
    assert sum(r['op'] == new for r in got) == sum(r['op'] == pre for r in got) == launches and not any(r['op'] == old for r in got)
    assert sum(r['op'] == 'slab_workspace' for r in got) == 1                               # once per volume, not per sample or step
    # without the once-per-volume allocation and the coefficient launches the chain is the plain consistent one, launch for launch
    steps, coefs = [dict(r) for r in got if r['op'] == new], [r for r in got if r['op'] == pre]
    for a, b, c in zip([r for r in plain if r['op'] == old], steps, coefs):
        assert c['meas_up'] == a['meas_up'] and c['y'] == b['y'] and c['coef'] == b['coef'] and c['workspace'] == b['workspace']
        assert (c['lo'], c['hi'], c['clamp_mode'], c['stride']) == (b['lo'], b['hi'], b['clamp_mode'], b['stride'])
        assert 'reach=1, jmax=20' in b['table'] and b['table'] == c['table'] and c['cell'] == b['cell'] == a['cell']
    # every other operand is the plain consistent launch's: drop what only one side has, then only names differ
    rest = [{k: v for k, v in r.items() if k not in ('table', 'coef', 'workspace', 'meas_up')} for r in got
            if r['op'] not in (pre, 'slab_workspace')]
    bare = [{k: v for k, v in r.items() if k != 'meas_up'} for r in plain]
    assert LT.canonical(rest).replace(pre, old).replace(new, old) == LT.canonical(bare)
    order = [r['op'] for r in got if r['op'] in (new, pre)]
    assert order == [pre, new] * launches                                                  # the coefficients of a step precede its update


@pytest.mark.parametrize('slab', [None, SLAB222])
def test_blend_mode_hands_the_slab_on_exactly_when_one_was_given(slab, monkeypatch):
    seen = []

    def sampler_of(rec):
        def sample(x, noise=None, **kw):
            seen.append(kw)
            return torch.zeros_like(x)
        return sample
    _volume_case(monkeypatch, 'blend-gaussian-s2-anchored', fn=sampler_of, slab=slab)
    assert seen
    for kw in seen:
        assert set(kw) == {'consistency', 'consistency_weight'} | ({'consistency_slab'} if slab is not None else set())
        assert slab is None or (kw['consistency_slab'] is slab and tuple(kw['consistency'][0].shape[1:]) == (1, 16, 16, 16))
