"""Data consistency for a k-space band limit, the part that needs no GPU: ``ops.band_table`` against the closed forms and against the
float64 specification of tests/volume_joint_band_reference.py (FFT, dense A, ``numpy.linalg.pinv``), every refusal, the fp32 restatement
against the specification on the inputs of the GPU tests, the guarantee at weight 1, the error codes of the entries, and -- with
recording stand-ins for ``ops`` -- the routing of ``consistency_band`` through the samplers and ``VolumeInference``."""
import numpy as np
import pytest
import torch

from tests import launch_trace as LT
from tests import volume_joint_band_reference as BD
from tests import volume_joint_dc_reference as DC
from tests import volume_joint_heun_reference as HN
from tests.test_volume_joint_host import _imagen

# (shape, cell, band, offset): the cases of the GPU tests, then N = 70 with n = 35 and 14, an even n with weights and a zero, f = 1 with
# weights (a pure filter), an identity axis, the largest axis
TABLE_CASES = [((P, P, P), cell, band, off) for cell, P, band, off in BD.PROJECT_CASES] + \
              [(vol, cell, *BD.STEP_CELLS[cell]) for vol, _, _ in BD.STEP_VOLUMES.values() for cell in BD.STEP_CELLS
               if all(s % f == 0 for s, f in zip(vol, cell))] + \
              [((70, 70, 70), (2, 5, 1), None, 'centre'), ((16, 24, 8), (2, 2, 2), ([1, 0.5, 0, 0.25], [1, 1, 0, 0, 1], None), (0.5, 0.5, 0)),
               ((10, 9, 8), (1, 1, 2), ([1, 0.9, 0.8], None, None), None), ((512, 4, 4), (4, 1, 2), None, None)]
BAND222 = ([1.0, 0.5], None, [1.0, 0.75])


def bits(t):
    return (t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)).view(np.uint32)


# ---- B1: the table -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', range(len(TABLE_CASES)))
def test_band_table_is_the_reference_table_bit_for_bit(case):
    from diffusioniqt_amd import ops
    shape, cell, band, off = TABLE_CASES[case]
    t = ops.band_table(shape, cell, band, off)
    axes = BD.axes_of(shape, cell, band, off)
    tabs, flat = BD.tables32(axes)
    assert t.table.dtype == torch.float32 and t.table.is_contiguous() and np.array_equal(bits(t.table), bits(flat))
    assert t.shape == tuple(shape) and t.cell == tuple(cell) and t.active == sum(1 << a for a, ax in enumerate(axes) if ax['active'])
    assert abs(t.gain - BD.gain(axes, tabs)) <= 1e-12 * t.gain
    for ax, ref, (d, a, g) in zip(t.axes, axes, tabs):
        assert (ax['N'], ax['n'], ax['f'], ax['active']) == (ref['N'], ref['n'], ref['f'], ref['active'])
        assert np.array_equal(bits(ax['d']), bits(d)) and np.array_equal(bits(ax['a']), bits(a)) and np.array_equal(bits(ax['g']), bits(g))
        N = ax['N']
        assert np.array_equal(bits(ax['d']), bits(ax['d'])[(-np.arange(N)) % N])            # d[m] = d[-m]: P is symmetric to the bit
    assert t.to('cpu').table is not None and t.to('cpu').active == t.active


@pytest.mark.parametrize('case', range(len(TABLE_CASES)))
def test_band_table_is_the_float64_specification(case):
    """P^2 = P, P = the FFT mask, A = the sum of the kept exponentials, A+ = pinv(A), A+ A = P, A 1 = 1 and P 1 = 1, to float64
    rounding, on the float64 values the table was rounded from."""
    from diffusioniqt_amd import ops
    shape, cell, band, off = TABLE_CASES[case]
    t = ops.band_table(shape, cell, band, off)
    for ax, ref in zip(t.axes, BD.axes_of(shape, cell, band, off)):
        if not ax['active']:
            assert ax['f'] == 1 and ax['d'].tolist() == [1.0] + [0.0] * (ax['N'] - 1)
            continue
        N, n, f = ax['N'], ax['n'], ax['f']
        d, a, g = (ax[k].numpy() for k in ('d64', 'a64', 'g64'))
        P, A, Ap = BD.circulant(d, N, N, 1, -1), BD.circulant(a, n, N, f, -1), BD.circulant(g, n, N, f, -1).T
        eye = np.eye(N)
        spec = np.stack([BD.project_spec(e[:, None, None], [ref, dict(N=1, active=False), dict(N=1, active=False)])[:, 0, 0] for e in eye], 1)
        tol = 1e-12
        assert np.abs(P @ P - P).max() <= tol and np.abs(P - spec).max() <= tol and np.abs(P - P.T).max() == 0
        assert np.abs(A - BD.dense_A(ref)).max() <= tol and np.abs(Ap - BD.dense_pinv(ref)).max() <= 64 * tol
        assert np.abs(Ap @ A - P).max() <= 64 * tol
        assert np.abs(A.sum(axis=1) - 1).max() <= tol and np.abs(P.sum(axis=1) - 1).max() <= tol
        kept = {k for k in range(1, len(ref['h'])) if ref['h'][k] > 0}
        assert set(ax['kept']) == kept and np.linalg.matrix_rank(P, tol=1e-9) == 1 + 2 * len(kept)


def test_band_table_refusals():
    from diffusioniqt_amd import ops
    ok = ((16, 16, 16), (2, 2, 2))
    bad = [(((16, 16), (2, 2, 2)), {}), (((16, 16, 15), (2, 2, 2)), {}), (((16, 16, 16), (2, 2)), {}), (((16, 16, 16), (1, 1, 1)), {}),
           (ok, dict(band=([1.0], [1.0]))), (ok, dict(band=([1.0], 'x', None))), (ok, dict(band=([], None, None))),
           (ok, dict(band=([1.0, -0.5], None, None))), (ok, dict(band=([1.0, float('nan')], None, None))),
           (ok, dict(band=([0.0, 1.0], None, None))),                                      # the mean must be kept
           (ok, dict(band=([1.0] * 5, None, None))),                                       # n = 8: kappa = 3, at most 4 weights
           (ok, dict(band=([1.0, 1.0 / 65], None, None))),                                 # a positive weight below max / 64
           (ok, dict(band=([1.0, 2.0, 1.0 / 33], None, None))),                            # ... of the LARGEST weight
           (ok, dict(offset=(0.0, 0.0))), (ok, dict(offset='center')), (ok, dict(offset=(0.0, float('inf'), 0.0))),
           (((16, 16, 16), (2, 2, 1)), dict(offset=(0.0, 0.0, 0.5)))]                      # an identity axis takes no offset
    for args, kw in bad:
        with pytest.raises(ValueError, match="consistency_band"):
            ops.band_table(*args, **kw)
    assert ops.band_table(*ok, band=([1.0, 1.0 / 64], None, None)).axes[0]['kept'] == (1,)  # the rule's edge is admitted
    assert ops.band_table(*ok, band=([2.0, 0.0, 1.0], None, None)).axes[0]['h'] == (1.0, 0.0, 0.5)
    with pytest.raises(ValueError, match="consistency_band"):
        ops.band_plan("here", (513, 8, 8))
    ops.band_plan("here", (512, 512, 512))
    assert ops.band_lds(512) <= 65536


def test_the_amplification_rule_is_a_rule_on_the_input():
    """max |g| / min over the kept weights: the back-projection of an admitted band amplifies no frequency by more than 64."""
    from diffusioniqt_amd import ops
    t = ops.band_table((32, 8, 8), (2, 1, 1), ([1.0, 1.0 / 64, 0.5], None, None))
    ax = t.axes[0]
    A, Ap = BD.circulant(ax['a64'].numpy(), ax['n'], ax['N'], ax['f'], -1), BD.circulant(ax['g64'].numpy(), ax['n'], ax['N'], ax['f'], -1).T
    assert np.linalg.svd(Ap, compute_uv=False).max() <= 64 * np.sqrt(ax['f']) * (1 + 1e-9)


# ---- B2: the fp32 restatement against the specification, on the inputs of the GPU tests -------------------------------------------------------
def project_reference(case, clamp, w):
    """(a, t, axes, tabs, the fp32 projection) of a per-window case."""
    cell, P, band, off = BD.PROJECT_CASES[case]
    axes = BD.axes_of((P, P, P), cell, band, off)
    tabs, _ = BD.tables32(axes)
    x0, truth = BD.project_inputs(P)
    t = BD.backproject32(BD.measure32(truth, axes, tabs), axes, tabs)
    a = DC.clamp32(*(clamp or (0., 0., None)))(x0)
    return a, t, axes, tabs, BD.project32(a, t, axes, tabs, w)


@pytest.mark.parametrize('w', [1.0, 0.5])
@pytest.mark.parametrize('case', range(len(BD.PROJECT_CASES)))
def test_project_restatement_is_the_float64_projection(case, w):
    """Within a quarter of the allowance.  Observed shares (the printed figure): 0.4 - 10 % of the allowance, the largest where one axis
    is active (the allowance is smallest there)."""
    a, t, axes, tabs, got = project_reference(case, (-1.0, 1.0, 1), w)
    want = BD.project64(a.astype(np.float64), t.astype(np.float64), axes, w)
    allow = BD.allowance(axes, tabs, float(np.abs(t - a).max()), float(np.abs(want).max()))
    err = np.abs(got - want).max()
    print(f"band project32 case {case} w {w}: error {err:.3e}, allowance {allow:.3e}, share {err / allow:.4f}")
    assert err <= allow / 4
    y32 = BD.measure32(BD.project_inputs(BD.PROJECT_CASES[case][1])[1], axes, tabs)
    assert np.abs(y32 - BD.measure64(BD.project_inputs(BD.PROJECT_CASES[case][1])[1], axes)).max() <= allow / 4


@pytest.mark.parametrize('name,cell', BD.STEP_CASES)
def test_joint_restatement_is_the_float64_projection(name, cell):
    """The joint step's projection with uncovered voxels (their residual is 0), within a quarter of the allowance.  Observed shares:
    0.4 - 9 %."""
    c = BD.step_case(name)
    band, off = BD.STEP_CELLS[cell]
    axes = BD.axes_of(c['vol'], cell, band, off)
    tabs, _ = BD.tables32(axes)
    t = BD.backproject32(BD.measure32(c['truth'], axes, tabs), axes, tabs)
    a, covered = DC.fuse32(c['y'], c['slot'], c['taps'], c['stride'], c['vol'], DC.clamp32(-1.0, 1.0, 1))
    assert (~covered).any() and covered.any()
    got = BD.project32(a, t, axes, tabs, 1.0, covered)
    want = BD.project64(a.astype(np.float64), t.astype(np.float64), axes, 1.0, covered)
    allow = BD.allowance(axes, tabs, float(np.abs(t - a)[covered].max()), float(np.abs(want).max()))
    err = np.abs(got - want).max()
    print(f"band joint project32 {name} cell {cell}: error {err:.3e}, allowance {allow:.3e}, share {err / allow:.4f}")
    assert err <= allow / 4


@pytest.mark.parametrize('case', range(len(BD.PROJECT_CASES)))
def test_the_guarantee_at_weight_one(case):
    """w = 1, no clamp, everything covered: A x0' = A t, the measurement behind the target, within the allowance."""
    a, t, axes, tabs, got = project_reference(case, None, 1.0)
    allow = BD.allowance(axes, tabs, float(np.abs(t - a).max()), float(np.abs(got).max()))
    err = np.abs(BD.measure64(got, axes) - BD.measure64(t, axes)).max()
    before = np.abs(BD.measure64(a, axes) - BD.measure64(t, axes)).max()
    print(f"band guarantee case {case}: |A x0' - y| = {err:.3e} (before: {before:.3e}), allowance {allow:.3e}")
    assert err <= allow and before > 0.1
    # and P x0' = P t: what the projection is defined by
    assert np.abs(BD.project_spec(got, axes) - BD.project_spec(t, axes)).max() <= allow


# ---- B3: the entries' error codes (the host side of the launchers: nothing is launched) -----------------------------------------------------------
def test_band_entries_return_error_codes():
    from diffusioniqt_amd import _lib
    lib = _lib.load()
    p = 4096                                               # a non-null address that is never read: every call fails before its launch
    assert lib.diqt_band_measure(None, p, p, p, 0, 8, 8, 8, 2, 2, 2, 7, None) == -2
    assert lib.diqt_band_measure(p, p, p, p, 0, 8, 8, 8, 2, 2, 2, 0, None) == -3          # an empty mask
    assert lib.diqt_band_measure(p, p, p, p, 0, 8, 8, 8, 2, 2, 2, 3, None) == -3          # x has a factor and no pass
    assert lib.diqt_band_measure(p, p, p, p, 0, 9, 8, 8, 2, 2, 2, 7, None) == -1          # 9 % 2
    assert lib.diqt_band_backproject(p, p, p, p, 0, 513, 8, 8, 1, 2, 2, 7, None) == -1    # above 512 voxels
    assert lib.diqt_band_backproject(p, p, p, p, 2 * 4 * 8 * 8 - 1, 8, 8, 8, 2, 2, 2, 7, None) == -1      # the workspace
    assert b"workspace" in lib.diqt_last_error()
    project = lambda **k: lib.diqt_band_project(*[k.get(n, v) for n, v in (
        ('x0', p), ('t', p), ('table', p), ('ws', p + 65536), ('out', p), ('cubes', 1), ('P', 8), ('fz', 2), ('fy', 2), ('fx', 2),
        ('floats', 1024), ('active', 7), ('w', 1.0), ('lo', 0.0), ('hi', 0.0), ('mode', 2), ('stream', None))])
    assert project(table=None) == -2 and project(w=0.0) == -3 and project(mode=3) == -3 and project(fz=3) == -1
    assert project(floats=1023) == -1 and project(ws=p) == -2 and project(active=8) == -3
    assert lib.diqt_band_apply(p, p, p, p + 65536, 512, 8, 8, 8, 7, None) == -2           # out aliases x
    assert lib.diqt_band_apply(p, p, p + 4096, p + 65536, 511, 8, 8, 8, 7, None) == -1
    assert lib.diqt_volume_joint_band_residual(None, p, p, p, p, p, p, 0, 8, 8, 8, 8, 8, 1, 1, 1, -1.0, 1.0, 2, None) == -3    # the clamp
    assert lib.diqt_volume_joint_band_residual(None, p, p, p, p, p, p, 0, 8, 8, 8, 8, 8, 2, 1, 1, -1.0, 1.0, 1, None) == -1    # the lattice
    step = lambda form=0, w=1.0, c=p: lib.diqt_volume_joint_consistent_band_step(None, None, None, p, None, p, p, c, p, p, form, 0, 8, 8, 8,
                                                                                  8, 8, 1, 1, 1, 2, 2, 2, w, 1.0, 1.0, 0.0, 0.0, -1.0, 1.0,
                                                                                  1, 0, 0, 0, None)
    assert step(c=None) == -2 and step(form=3) == -3 and step(w=1.5) == -3


# ---- B4: argument rules, all before the device is touched ------------------------------------------------------------------------------------------
def _meas(P=16, B=2):
    return torch.zeros(B, 1, P, P, P)


def test_sample_refuses_a_band_it_cannot_honour():
    imagen = _imagen()
    lr = torch.zeros(2, 1, 16, 16, 16)
    base = dict(batch_size=2, start_image_or_video=lr, start_at_unet_number=2, use_tqdm=False, sampler='ddim', sample_steps=2)
    ok = (_meas(), (2, 2, 2))
    named = [dict(consistency_band=BAND222),                                               # a band without consistency
             dict(consistency=ok, consistency_band=BAND222, consistency_profile=((1, 2), (1, 1), (3, 1))),
             dict(consistency=ok, consistency_band=BAND222, consistency_noise=0.1, eta=0.5),
             dict(consistency=ok, consistency_band=BAND222, consistency_operator=np.full((1, 8), 0.125)),
             dict(consistency=ok, consistency_band=BAND222, consistency_operator=np.full((1, 8), 0.125), consistency_row_noise=0.1,
                  eta=0.5),
             dict(consistency=ok, consistency_band=BAND222, consistency_slab=([0.25, 1.0, 1.0, 0.25], [1.0, 0.5], [0.75, 1.0])),
             dict(consistency=ok, consistency_band=([1.0] * 5, None, None)),                # beyond the measurement grid
             dict(consistency=ok, consistency_band=([1.0, 0.01], None, None)),              # the amplification rule
             dict(consistency=ok, consistency_band=(None, None)),
             dict(consistency=ok, consistency_band=(None, None, None, 'middle')),
             dict(consistency=ok, consistency_band=BAND222, consistency_weight=0.0),        # what consistency refuses names it too
             dict(consistency=ok, consistency_band=BAND222, init_images=lr),
             dict(consistency=ok, consistency_band=BAND222, sampler='ddpm', sample_steps=None, skip_steps=2),
             dict(consistency=ok, consistency_band=BAND222, sampler='ddpm', inpaint_images=lr, inpaint_masks=lr[:, 0].bool())]
    for kw in named:
        with pytest.raises(ValueError, match="consistency_band"):
            imagen.sample(**{**base, **kw})
    kept = [(dict(consistency_weight=0.0), "consistency weight"), (dict(init_images=lr), "neither init_images nor skip_steps"),
            (dict(sampler='ddpm', inpaint_images=lr, inpaint_masks=lr[:, 0].bool()), "inpainting are not offered together")]
    for kw, wording in kept:                                                               # every existing refusal keeps its wording
        with pytest.raises(ValueError, match=wording):
            imagen.sample(**{**base, 'consistency': ok, 'consistency_band': BAND222, **kw})
    with pytest.raises(ValueError, match="consistency_band"):                              # the loop itself applies the same rules
        imagen.p_sample_loop(imagen.unets[1], (2, 1, 16, 16, 16), noise_scheduler=imagen.noise_schedulers[1], consistency_band=BAND222)


def test_edm_sample_refuses_a_band_it_cannot_honour():
    elu = HN.make_elucidated('churn-on', False)
    lr = torch.zeros(2, 1, 16, 16, 16)
    base = dict(batch_size=2, video_frames=16, start_image_or_video=lr, start_at_unet_number=2, use_tqdm=False, sampler='dpmpp2m',
                sample_steps=3)
    ok = (_meas(), (2, 2, 2))
    named = [dict(consistency_band=BAND222), dict(consistency=ok, consistency_band=BAND222, sampler='heun', sample_steps=None),
             dict(consistency=ok, consistency_band=BAND222, consistency_noise=0.1, eta=0.5),
             dict(consistency=ok, consistency_band=([1.0, 0.01], None, None)), dict(consistency=ok, consistency_band=BAND222, init_images=lr)]
    for kw in named:
        with pytest.raises(ValueError, match="consistency_band"):
            elu.sample(**{**base, **kw})
    with pytest.raises(ValueError, match="Heun sampler"):
        elu.sample(**{**base, **named[1]})


def _volume_inference(**kw):
    from diffusioniqt_amd.inference import VolumeInference
    from tests import volume_blend_reference as R
    return VolumeInference(R.shared_cfg(8), lambda x, **k: x, **kw)


def test_volume_inference_takes_a_band_with_joint_only():
    """The crop mode and the blend modes refuse, naming the keyword and the reason; the other rules are checked before a joint chain."""
    meas = torch.zeros(20, 18, 22)
    ok = dict(consistency=(meas, (2, 2, 2)), consistency_band=BAND222)
    for mode in (dict(), dict(blend='gaussian'), dict(blend='constant', noise='anchored')):
        with pytest.raises(ValueError, match="consistency_band needs joint=True.*window"):
            _volume_inference(**ok, **mode)
    for kw in (dict(consistency_band=BAND222), {**ok, 'consistency_noise': 0.1}, {**ok, 'consistency_profile': ((1, 2), (1, 1), (3, 1))},
               {**ok, 'consistency_band': (None,)}):
        with pytest.raises(ValueError, match="consistency_band"):
            _volume_inference(joint=True, blend='gaussian', noise='anchored', **kw)


# ---- B5: routing, with recording stand-ins --------------------------------------------------------------------------------------------------------
def _imagen_trace(sampler, eta, band):
    from diffusioniqt_amd import imagen_pytorch3D
    into = lambda key: (lambda a: a['out'] if a.get('out') is not None else torch.zeros_like(a[key]))
    returns = {'axpby3': lambda a: torch.zeros_like(a['a']), 'ddpm_step': lambda a: (torch.zeros_like(a['x_t']), torch.zeros_like(a['x_t'])),
               'cell_project': into('x0'), 'band_project': into('x0')}
    rec = LT.Recorder()
    imagen = _imagen()
    lr, meas = torch.zeros(2, 1, 16, 16, 16), torch.full((2, 1, 16, 16, 16), 0.125)
    rec.tag(lr, 'lowres'), rec.tag(meas, 'meas_up')
    noise = [LT.zeros(2, 1, 16, 16, 16) for _ in range(8)]
    for k, t in enumerate(noise):
        rec.tag(t, f'noise{k}')
    kw = dict(consistency=(meas, (2, 2, 4)), consistency_weight=0.5)
    if band is not None:
        kw.update(consistency_band=band)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(imagen_pytorch3D, 'ops', LT.RecordingOps(rec, returns))
        imagen.sample(batch_size=2, start_image_or_video=lr, start_at_unet_number=2, use_tqdm=False, device='cpu', sampler=sampler,
                      sample_steps=3, eta=eta, noise=noise, **kw)
    return rec.trace


BAND224 = (None, [1.0, 0.5], None, 'centre')


@pytest.mark.parametrize('sampler,eta', [('ddim', 0.0), ('ddim', 0.5), ('ddpm', 0.0), ('dpmpp2m', 0.0)])
def test_imagen_sample_projects_with_the_band_once_per_step(sampler, eta):
    plain, got = _imagen_trace(sampler, eta, None), _imagen_trace(sampler, eta, BAND224)
    assert sum(r['op'] == 'cell_project' for r in plain) == 3 and not any(r['op'] == 'band_project' for r in plain)
    assert sum(r['op'] == 'band_project' for r in got) == 3 and not any(r['op'] == 'cell_project' for r in got)
    tables = {r.pop('table') for r in got if r['op'] == 'band_project'}                     # ONE table per chain, made for its cubes
    assert len(tables) == 1 and 'BandTable(shape=(16, 16, 16), cell=(2, 2, 4), kept=[3, 1, 1]' in next(iter(tables))
    for r in got:
        if r['op'] == 'band_project':
            assert r.pop('workspace') is None and r.pop('target') == [q for q in plain if q['op'] == 'cell_project'][0]['meas_up']
    for r in plain:
        r.pop('meas_up', None)
    # the same launches on the same operands: only the op (and the buffer tags made from its name) differs
    assert LT.canonical(got).replace('band_project', 'cell_project') == LT.canonical(plain)


@pytest.mark.parametrize('eta,self_cond', [(0.0, False), (0.5, True)])
def test_edm_sample_projects_with_the_band_once_per_step(eta, self_cond, monkeypatch):
    from tests import test_edm_sampler_trace_host as T
    monkeypatch.setitem(T.RETURNS, 'band_project', T._into('x0'))
    base = dict(model=dict(self_cond=self_cond), sampler='dpmpp2m', eta=eta, consistency=0.5)
    monkeypatch.setitem(T.CASES, 'band-off', T.sample_case(**base))
    monkeypatch.setitem(T.CASES, 'band-on', T.sample_case(**base, consistency_band=BAND224))
    plain, got = T.run_case('band-off')[0], T.run_case('band-on')[0]
    steps = sum(r['op'] == 'multistep_sde_step' for r in plain)
    assert steps > 0 and sum(r['op'] == 'cell_project' for r in plain) == steps
    assert sum(r['op'] == 'band_project' for r in got) == steps and not any(r['op'] == 'cell_project' for r in got)
    assert [r['op'].replace('band_project', 'cell_project') for r in got] == [r['op'] for r in plain]


def _volume_case(monkeypatch, name, band=None, counts=None):
    """One ``VolumeInference`` case of the launch-trace module with consistency (and the band, if any) switched on."""
    from diffusioniqt_amd import ops
    from tests import test_volume_launch_trace_host as T
    real = ops.band_table
    if counts is not None:
        monkeypatch.setattr(ops, 'band_table', lambda *a, **k: (counts.append(a[0]), real(*a, **k))[1])
    monkeypatch.setitem(T.RETURNS, 'cell_replicate', lambda a: ops.cell_replicate(a['meas'], a['cell']))
    monkeypatch.setitem(T.RETURNS, 'band_backproject', lambda a: LT.zeros(*a['table'].shape))
    monkeypatch.setitem(T.RETURNS, 'band_workspace', lambda a: LT.zeros(5, *a['shape']))
    monkeypatch.setitem(T.RETURNS, 'volume_joint_band_residual', lambda a: a['workspace'])
    monkeypatch.setitem(T.RETURNS, 'band_apply', lambda a: a['out'])
    for op in ('volume_joint_consistent_step', 'volume_joint_consistent_band_step'):
        monkeypatch.setitem(T.RETURNS, op, lambda a: (a['out'], a['x0_out']))
    monkeypatch.setattr(T.StubDenoiser, 'state_space', lambda self, x: self.rec.record('state_space', {'x': x}, x), raising=False)
    case = dict(T.CASES[name])
    extra = dict(consistency=(torch.full((20, 18, 22), 300.0), (2, 2, 2)))
    if band is not None:
        extra.update(consistency_band=band)
    case['kw'] = dict(case['kw'], consistency_weight=0.5, **extra)
    monkeypatch.setitem(T.CASES, 'band-case', case)
    return T.run_case('band-case')


@pytest.mark.parametrize('chain', ['step', 'multistep', 'sigma-base1'])
def test_joint_chain_dispatches_the_three_band_ops_per_step(chain, monkeypatch):
    name = f'joint-{chain}-selfcond'
    plain = _volume_case(monkeypatch, name)
    made = []
    got = _volume_case(monkeypatch, name, band=BAND222, counts=made)
    old, new, pre, mid = 'volume_joint_consistent_step', 'volume_joint_consistent_band_step', 'volume_joint_band_residual', 'band_apply'
    launches = sum(r['op'] == old for r in plain)
    assert launches == 2 * 3 and not any(r['op'].startswith('band') or 'band' in r['op'] for r in plain)     # S = 2 samples of T = 3 steps
    assert [sum(r['op'] == op for r in got) for op in (new, pre, mid)] == [launches] * 3 and not any(r['op'] == old for r in got)
    # once per volume, not per sample or step: one table (for the volume's shape), one back-projection, one workspace
    assert made == [(40, 36, 44)]
    assert sum(r['op'] == 'band_workspace' for r in got) == 1 and sum(r['op'] == 'band_backproject' for r in got) == 1
    assert not any(r['op'] == 'cell_replicate' for r in got)
    order = [r['op'] for r in got if r['op'] in (new, pre, mid)]
    assert order == [pre, mid, new] * launches                                             # residual -> apply -> step, at every step
    steps, res, app = ([dict(r) for r in got if r['op'] == op] for op in (new, pre, mid))
    for a, b, c, d in zip([r for r in plain if r['op'] == old], steps, res, app):
        assert c['y'] == b['y'] and c['workspace'] == b['workspace'] and c['table'] == b['table'] == d['table']
        assert 'BandTable(shape=(40, 36, 44), cell=(2, 2, 2)' in b['table'] and b['cell'] == a['cell']
        assert (c['lo'], c['hi'], c['clamp_mode'], c['stride']) == (b['lo'], b['hi'], b['clamp_mode'], b['stride'])
        ws = c['workspace']
        per = 40 * 36 * 44
        assert ws['shape'] == [5, 40, 36, 44] and (d['x']['t'], d['out']['t'], d['workspace']['t']) == (ws['t'],) * 3
        assert (d['x']['off'], d['out']['off'], d['workspace']['off']) == (2 * per, 3 * per, 4 * per)
    # every other operand is the plain consistent launch's: drop what only one side has, then only names differ
    rest = [{k: v for k, v in r.items() if k not in ('table', 'workspace', 'meas_up')} for r in got
            if r['op'] not in (pre, mid, 'band_workspace', 'band_backproject', 'cell_replicate', 'state_space')]
    bare = [{k: v for k, v in r.items() if k != 'meas_up'} for r in plain if r['op'] not in ('cell_replicate', 'state_space')]
    assert LT.canonical(rest).replace(pre, old).replace(new, old) == LT.canonical(bare)        # (buffer tags carry the op that saw them first)
