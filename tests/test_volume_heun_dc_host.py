"""Data-consistent sampling for the stochastic Heun sampler (``consistency_heun='both'`` / ``'predictor'``), the part that needs no
GPU: every admission and refusal of the keyword, that nothing changes without it, the error codes of
``diqt_volume_joint_consistent_heun``, the fp32 restatement of tests/volume_joint_heun_dc_reference.py against the float64
specification on the inputs of the GPU tests, the fp32 emulation of the chains against their bound, and -- with recording stand-ins
for ``ops`` -- which launches the per-window loop, the joint chain and the crop and blend modes make."""
import numpy as np
import pytest
import torch

from tests import volume_blend_reference as R
from tests import volume_joint_dc_reference as DC
from tests import volume_joint_heun_dc_reference as HD
from tests import volume_joint_heun_reference as HN
from tests import volume_joint_profile_reference as PR
from tests import volume_joint_tile_reference as TR
from tests.test_volume_joint_host import _imagen

T_STEPS = HN.HP['num_sample_steps']
PROFILE224 = ((1, 3), (1, 1), (1, 2, 2, 1))
SLAB224 = ([0.25, 1.0, 1.0, 0.25], [1.0, 0.5], [0.5, 1.0, 1.0, 0.5])
BAND224 = (None, [1.0, 0.5], None, 'centre')
A224 = TR.stack_matrix((2, 2, 4), (0, 2))
# per mode: the keyword that selects it and the projection launch a one-call sampler makes
MODES = {'cell': ({}, 'cell_project'), 'profile': (dict(consistency_profile=PROFILE224), 'cell_project_profile'),
         'tile': (dict(consistency_operator=A224), 'tile_project'), 'slab': (dict(consistency_slab=SLAB224), 'slab_project'),
         'band': (dict(consistency_band=BAND224), 'band_project')}


# ---- H1: admission and refusal, all before the device is touched ---------------------------------------------------------------------------
def _meas(P=16, B=2):
    return torch.zeros(B, 1, P, P, P)


def _plan(**kw):
    from diffusioniqt_amd import consistency, ops
    args = dict(consistency=(_meas(), (2, 2, 4)), shape=(2, 1, 16, 16, 16), sampler='heun', stochastic=False)
    args.update(kw)
    names = ('consistency', 'weight', 'profile', 'noise', 'operator', 'row_noise', 'slab', 'band')
    positional = [args.pop(n, 1.0 if n == 'weight' else None) for n in names]
    return consistency.plan('here', ops, *positional, **args)


@pytest.mark.parametrize('which', HD.WHICH)
@pytest.mark.parametrize('mode', list(MODES))
def test_the_heun_sampler_admits_all_five_modes_per_window(mode, which):
    extra = {k[len('consistency_'):]: v for k, v in MODES[mode][0].items()}
    p = _plan(heun=which, **extra)
    assert p.heun == which and p.mode == mode
    kw = p.keywords(p.measurement)
    assert kw['consistency_heun'] == which and set(kw) == {'consistency', 'consistency_weight', 'consistency_heun'} | set(MODES[mode][0])
    chain = p.prepare([(1.5, 0.75, 0.25), (0.75, 0.0, 0.0)], 'cpu')
    assert chain.heun == which and chain.steps == [('constant', 1.0, 0.)] * 2                # every rung is the constant one


def test_keywords_carry_consistency_heun_exactly_when_it_was_given():
    p = _plan(sampler='dpmpp2m')
    assert p.heun is None and 'consistency_heun' not in p.keywords(p.measurement)


def test_edm_sample_refusals_name_the_keyword():
    elu = HN.make_elucidated('churn-on', False)
    lr = torch.zeros(2, 1, 16, 16, 16)
    base = dict(batch_size=2, video_frames=16, start_image_or_video=lr, start_at_unet_number=2, use_tqdm=False)
    ok = (_meas(), (2, 2, 2))
    named = [(dict(consistency_heun='both'), "consistency_heun needs consistency"),
             (dict(consistency=ok, consistency_heun='corrector'), "consistency_heun must be 'both'"),
             (dict(consistency=ok, consistency_heun=True), "consistency_heun must be 'both'"),
             (dict(consistency=ok, consistency_heun='both', sampler='dpmpp2m'), "consistency_heun goes with the Heun sampler"),
             (dict(consistency=ok, consistency_heun='predictor', sampler='dpmpp2m', eta=0.5), "consistency_heun goes with the Heun sampler"),
             (dict(consistency=ok, consistency_heun='both', consistency_noise=0.1), "consistency_heun and consistency_noise"),
             (dict(consistency=ok, consistency_heun='both', consistency_operator=np.full((1, 8), 0.125), consistency_row_noise=0.1),
              "consistency_heun and consistency_row_noise"),
             (dict(consistency=ok, consistency_heun='both', init_images=lr), "neither init_images nor skip_steps"),
             (dict(consistency=ok, consistency_heun='both', skip_steps=1), "neither init_images nor skip_steps"),
             (dict(consistency=ok, consistency_heun='both', inpaint_images=lr, inpaint_masks=lr[:, 0].bool()),
              "inpainting are not offered together"),
             (dict(consistency=ok, consistency_heun='both', consistency_weight=0.0), "consistency weight"),
             (dict(consistency=(_meas(), (3, 1, 1)), consistency_heun='both'), "consistency cell")]
    for kw, wording in named:
        with pytest.raises(ValueError, match=wording) as err:
            elu.sample(**{**base, **kw})
        assert 'consistency_heun' in str(err.value), kw                                    # what consistency refuses names its rider too
    with pytest.raises(ValueError, match="consistency_heun"):                              # the loop itself applies the same rules
        elu.one_unet_sample(elu.unets[1], (2, 1, 16, 16, 16), unet_number=2, consistency=ok, consistency_heun='half')


def test_refusals_without_the_keyword_are_unchanged():
    """The Heun sampler and the Heun denoiser stay refused under ``consistency`` alone, with the phrases the existing tests match."""
    from diffusioniqt_amd.inference import VolumeInference
    elu = HN.make_elucidated('churn-on', False)
    lr = torch.zeros(2, 1, 16, 16, 16)
    base = dict(batch_size=2, video_frames=16, start_image_or_video=lr, start_at_unet_number=2, use_tqdm=False)
    for extra in ({}, dict(consistency_slab=([0.25, 1.0, 1.0, 0.25], [1.0, 0.5], [0.75, 1.0])), dict(consistency_band=([1.0, 0.5], None, None))):
        with pytest.raises(ValueError, match="consistency is not offered with the Heun sampler .two predictions per step.: use "
                                             "sampler='dpmpp2m'") as err:
            elu.sample(consistency=(_meas(), (2, 2, 2)), **extra, **base)
        assert all(k in str(err.value) for k in extra)
    with pytest.raises(ValueError, match="consistency is not offered with the EDM Heun denoiser .two predictions per step and three joint "
                                         "volumes.: use window_denoiser.sampler='dpmpp2m'."):
        VolumeInference(R.shared_cfg(8), elu.window_denoiser(), blend='gaussian', noise='anchored', joint=True,
                        consistency=(torch.zeros(20, 18, 22), (2, 2, 2)))


def test_imagen_refuses_the_keyword_with_every_sampler():
    imagen = _imagen()
    lr = torch.zeros(2, 1, 16, 16, 16)
    base = dict(batch_size=2, start_image_or_video=lr, start_at_unet_number=2, use_tqdm=False, consistency=(_meas(), (2, 2, 2)))
    for sampler, steps, eta in (('ddpm', None, 0.0), ('ddim', 2, 0.0), ('ddim', 2, 0.5), ('dpmpp2m', 2, 0.0)):
        with pytest.raises(ValueError, match="consistency_heun goes with the Heun sampler"):
            imagen.sample(sampler=sampler, sample_steps=steps, eta=eta, consistency_heun='both', **base)
    with pytest.raises(ValueError, match="consistency_heun needs consistency"):
        imagen.sample(batch_size=2, start_image_or_video=lr, start_at_unet_number=2, use_tqdm=False, consistency_heun='both')
    with pytest.raises(ValueError, match="consistency_heun"):
        imagen.p_sample_loop(imagen.unets[1], (2, 1, 16, 16, 16), noise_scheduler=imagen.noise_schedulers[1],
                             consistency=(_meas(), (2, 2, 2)), consistency_heun='predictor')


def _volume_inference(fn=None, **kw):
    from diffusioniqt_amd.inference import VolumeInference
    return VolumeInference(R.shared_cfg(8), fn if fn is not None else (lambda x, **k: x), **kw)


def test_volume_inference_admissions_and_refusals():
    elu = HN.make_elucidated('churn-on', False)
    heun, multistep = elu.window_denoiser(), elu.window_denoiser(sampler='dpmpp2m')
    meas = torch.zeros(20, 18, 22)
    ok = dict(consistency=(meas, (2, 2, 2)), consistency_heun='both')
    joint = dict(blend='gaussian', noise='anchored', joint=True)
    # joint: cell, profile and tile
    for extra in ({}, dict(consistency_profile=((1, 2), (1, 1), (3, 1))),
                  dict(consistency=(meas.expand(12, -1, -1, -1).contiguous(), (2, 2, 2)), consistency_operator=TR.stack_matrix((2, 2, 2), (0, 1, 2)))):
        for which in HD.WHICH:
            inf = _volume_inference(heun, **{**ok, **extra, 'consistency_heun': which}, **joint)
            assert inf.consistency_heun == which and inf.plan.mode == ('tile' if 'consistency_operator' in extra else
                                                                       'profile' if extra else 'cell')
    # joint: the slab and the band are refused, with the reason
    for extra, name in ((dict(consistency_slab=([0.25, 1.0, 1.0, 0.25], [1.0, 0.5], [0.75, 1.0])), 'consistency_slab'),
                        (dict(consistency_band=([1.0, 0.5], None, None)), 'consistency_band')):
        with pytest.raises(ValueError, match=f"consistency_heun and {name} are not offered together with joint=True.*three linear update forms"):
            _volume_inference(heun, **ok, **extra, **joint)
        assert _volume_inference(multistep, consistency=ok['consistency'], **extra, **joint).plan.mode == name[12:]     # as before
    # a joint denoiser without ``heun``
    for den in (multistep, _imagen().window_denoiser(sampler='ddim', sample_steps=2)):
        with pytest.raises(ValueError, match="consistency_heun goes with the Heun sampler"):
            _volume_inference(den, **ok, **joint)
    with pytest.raises(ValueError, match="consistency_heun needs consistency"):
        _volume_inference(heun, consistency_heun='both', **joint)
    with pytest.raises(ValueError, match="consistency_heun must be"):
        _volume_inference(heun, **{**ok, 'consistency_heun': 'corrector'}, **joint)
    with pytest.raises(ValueError, match="consistency_heun and consistency_noise"):
        _volume_inference(heun, **ok, consistency_noise=0.1, **joint)
    with pytest.raises(ValueError, match="inpaint are not offered together.*consistency_heun"):
        _volume_inference(heun, **ok, inpaint=(torch.zeros(20, 18, 22), torch.zeros(20, 18, 22, dtype=torch.bool)), **joint)
    # crop and blend modes: the sampler call decides; the four window-local modes pass, the band still needs joint=True
    for mode in (dict(), dict(blend='gaussian'), dict(blend='constant', noise='anchored')):
        for extra in ({}, dict(consistency_profile=((1, 2), (1, 1), (3, 1))), dict(consistency_slab=([0.25, 1.0, 1.0, 0.25], [1.0, 0.5], [0.75, 1.0]))):
            assert _volume_inference(**ok, **extra, **mode).consistency_heun == 'both'
        with pytest.raises(ValueError, match="consistency_band needs joint=True.*window"):
            _volume_inference(**ok, consistency_band=([1.0, 0.5], None, None), **mode)


# ---- H2: the error codes of the entry (the host side of the launcher: nothing is launched) -----------------------------------------------------
def test_joint_consistent_heun_entry_returns_error_codes():
    from diffusioniqt_amd import _lib
    lib = _lib.load()
    buf = (np.zeros(4, dtype=np.int32)).ctypes.data                             # never dereferenced: every call below is refused
    geo = (40, 36, 44, 16, 8, 4, 3, 4)                                          # D, H, W, P, stride and the lattice of range(0, n - 15, 8)

    def call(ptrs=(buf,) * 8, phase=1, mode=0, geo=geo, cell=(2, 2, 2), w=1.0, clamp=1):
        return lib.diqt_volume_joint_consistent_heun(*ptrs, phase, mode, 3, *geo, *cell, w, 1.0, 0.5, 0.25, -0.25, 0.125, -1.0, 1.0, clamp, 0,
                                                     1, 0, None)
    for k in range(7):                                                          # y, slot, taps, xh, xn, x0, meas_up
        assert call(tuple(None if i == k else buf for i in range(8))) == -2, k
    assert b"null pointer" in lib.diqt_last_error()
    assert call((buf,) * 7 + (None,), mode=1) == -2 and call((buf,) * 7 + (None,), mode=2) == -2       # the table, where the mode reads one
    assert call(phase=0) == -3 and b"phase 0" in lib.diqt_last_error()
    assert call(phase=3) == -3 and call(phase=-1) == -3
    assert call(mode=3) == -3 and b"mode 3" in lib.diqt_last_error()
    assert call(mode=-1) == -3
    assert call(cell=(1, 1, 1)) == -3 and call(cell=(5, 13, 1)) == -3 and call(cell=(0, 2, 2)) == -3     # n = 1, n = 65
    assert call(w=0.0) == -3 and call(w=1.5) == -3 and call(clamp=2) == -3
    assert call(cell=(3, 1, 1)) == -1 and b"does not divide" in lib.diqt_last_error()                      # 40 % 3
    assert call(cell=(1, 1, 8)) == -1                                                                        # 44 % 8
    assert call(geo=(40, 36, 44, 16, 8, 4, 3, 5)) == -1                                                      # the lattice
    # a plan above 64 KiB of LDS is an error code, not a launch (the case of diqt_volume_joint_consistent_tile_step)
    big = (4160, 4104, 4104, 4104, 4104, 1, 1, 1)
    assert call(geo=big, cell=(64, 1, 1), mode=2) == -1 and b"LDS" in lib.diqt_last_error()


def test_the_lds_plan_of_the_wrapper_is_the_entrys():
    from diffusioniqt_amd import ops
    assert ops.volume_joint_consistent_heun_lds((64, 1, 1), 4104, 'tile') == 65536 + 32
    assert ops.volume_joint_consistent_heun_lds((2, 2, 2), 8, 'cell') == 4 * (8 + 2 * 2 * 2 * 64)
    assert ops.volume_joint_consistent_heun_lds((1, 3, 1), 8, 'profile') == 4 * (8 + 2 * 6 * 64 + 6)
    assert ops.volume_joint_consistent_heun_lds((1, 1, 5), 16, 'tile') == 4 * (16 + 2 * 4 * 65 + 25)


# ---- H3: the fp32 restatement against the float64 specification, on the inputs of the GPU tests --------------------------------------------------
# the launches of tests/test_gpu_volume_heun_dc.py: both tilings x five cells x three modes with their clamp and weight, and the two
# n = 64 launches on the (12, 16, 72) volume
LAUNCHES = [(stride, kind, DC.STEP_VOL, cell, mode, *HD.step_rotation(stride, cell, mode))
            for stride, kind in DC.STEP_TILINGS for cell in DC.STEP_CELLS for mode in HD.MODES] + \
           [(4, 'gaussian', HD.BIG_VOL, HD.BIG_CELL, 'tile', clamp, w) for clamp, w in HD.BIG_CASES]


@pytest.mark.parametrize('stride,kind,shape,cell,mode,clamp,w', LAUNCHES,
                         ids=[f"s{c[0]}-{'x'.join(map(str, c[3]))}-{c[4]}-{c[5]}-w{c[6]}" for c in LAUNCHES])
def test_phase_restatement_is_the_float64_update(stride, kind, shape, cell, mode, clamp, w):
    """Both phases of every launch the GPU test makes -- the same predictions, state, measurement, table, clamp and weight -- against
    the same update in float64 on the float64 walk, within a quarter of: the blend's bound on the fused x0, through the projection's
    gain and the coefficients, plus the projection's roundings and the update's (two products and a sum; four products, three sums
    and the churn).  Only the churn's normals are a host array here (the restatement takes any).  Observed shares of that allowance
    over the 32 launches: x0' 0.5 - 6.4 %, xn 0.5 - 9.6 %, xh 0.2 - 4.6 %."""
    c = HD.step_refs(stride, kind, shape)
    table = HD.table_of(mode, cell)
    meas, xh0, xn0, x0v0 = HD.step_operands(c, cell, mode)
    kc, u = HD.KC, 2.0 ** -24
    n = np.random.default_rng(1).standard_normal(shape).astype(np.float32)
    fused = c['fused'][clamp]
    kw = dict(mode=mode, table=table)
    xh, xn1, x0a = HD.heun_phase32(1, fused[0], xh0, xn0, x0v0, meas, cell, w, HD.COEFS1, **kw)
    xh2, _, x0b = HD.heun_phase32(2, fused[1], xh, xn1, x0a, meas, cell, w, HD.COEFS2, kc, n, **kw)
    covered = fused[0][1]
    # float64, from the float64 walk
    c64 = DC.J.clamp_of(*HD.CLAMPS[clamp])
    ys = [c64(y.astype(np.float64)) for y in (c['y'], c['y2'])]
    proj = HD.projector(mode, meas.astype(np.float64), cell, w, table)
    f64 = [HN.fuse(y, c['slot'], c['taps'].astype(np.float64), stride, shape) for y in ys]
    assert np.array_equal(f64[0][1], covered)
    p0, p1 = proj(*f64[0]), proj(*f64[1])
    want_n, _ = HN.heun_phase1(p0, covered, xh0.astype(np.float64), *HD.COEFS1)
    want_h, _ = HN.heun_phase2(p1, covered, xh0.astype(np.float64), want_n, p0, HD.COEFS2, kc, n.astype(np.float64))
    y_max = max(float(np.abs(y).max()) for y in ys)
    blend = R.tolerance(8, y_max)                                                     # at most two windows per axis cover a voxel
    gain = TR.gain_of(table) if mode == 'tile' else max(1.0, float(np.max(table[1]))) if mode == 'profile' else 1.0
    S = max(float(np.abs(p0).max()), float(np.abs(p1).max()), float(np.abs(meas).max()), y_max)
    own = HD.roundings(mode, cell, table, S) if mode != 'profile' else PR.profile_roundings(cell, table, w, S)
    e0 = (1 + 2 * gain) * blend + own                                                 # |x0' - its float64| of one evaluation
    a1, b1 = np.abs(HD.COEFS1)
    a2, b2, c2, d2 = np.abs(HD.COEFS2)
    M = max(float(np.abs(xh0).max()), float(np.abs(want_n).max()), float(np.abs(want_h).max()))
    e_n = b1 * e0 + 3 * u * (a1 * M + b1 * S)
    e_h = b2 * e0 + c2 * e_n + d2 * e0 + 7 * u * ((a2 + c2) * M + (b2 + d2) * S) + 2 * u * (M + 6 * kc)
    err0 = max(np.abs(x0a - p0).max(), np.abs(x0b - p1).max())
    err_n, err_h = np.abs(xn1 - want_n).max(), np.abs(xh2 - want_h).max()
    print(f"heun dc restatement stride {stride} cell {cell} {mode} clamp {clamp} w {w}: x0' {err0:.3e} / {e0:.3e} ({err0 / e0:.3f}), "
          f"xn {err_n:.3e} / {e_n:.3e} ({err_n / e_n:.3f}), xh {err_h:.3e} / {e_h:.3e} ({err_h / e_h:.3f})")
    assert err0 <= e0 / 4 and err_n <= e_n / 4 and err_h <= e_h / 4
    assert np.array_equal(xh2[~covered], xh0[~covered]) and np.array_equal(xn1[~covered], xh0[~covered])
    assert not x0a[~covered].any() and not x0b[~covered].any()


# ---- H4: the fp32 emulation of the chains against their bound ---------------------------------------------------------------------------------
@pytest.mark.parametrize('which', HD.WHICH)
@pytest.mark.parametrize('mode', HD.MODES)
@pytest.mark.parametrize('cell', HD.CHAIN_CELLS)
@pytest.mark.parametrize('churn', list(HN.CHURN))
def test_fp32_emulation_of_the_chain_stays_under_a_quarter_of_the_bound(churn, cell, mode, which):
    """The chain of the GPU test (``HD.chain_volume`` / ``chain_cfg`` / ``chain_case`` / ``chain_weight``: its inputs) in float32
    numpy against the float64 chain.  Observed: 1.6e-7 - 4.5e-7, 0.1 - 0.9 % of the bound."""
    vol, cfg = HD.chain_volume(), HD.chain_cfg()
    tabs = HN.tables(HN.HP, HN.CHURN[churn])
    _, _, meas_up, table = HD.chain_case(mode, cell)
    w = HD.chain_weight(cell)
    ref = HD.joint_reference(vol, cfg, tabs, 'gaussian', False, mode, meas_up, cell, w, which, table)
    emu = HD.joint_reference(vol, cfg, tabs, 'gaussian', False, mode, meas_up, cell, w, which, table, dtype=np.float32)
    assert ref['projections'] == (2 * T_STEPS - 1 if which == 'both' else T_STEPS)
    err = np.abs(emu['mean'] - ref['mean']).max()
    print(f"heun dc fp32 emulation {churn} cell {cell} {mode} {which}: {err:.3e}, bound {ref['bound']:.3e} (Heun {ref['heun_bound']:.3e}, "
          f"{ref['projections']} projections at scale {ref['scale']:.2f}), share {err / ref['bound']:.4f}")
    assert err <= ref['bound'] / 4
    plain = HN.joint_reference(vol, cfg, tabs, 'gaussian', False)
    live = ref['covered'] & ~ref['background']
    assert np.abs(ref['mean'] - plain['mean'])[live].max() > 0.05                          # and it is not the plain chain


# ---- H5: routing, with recording stand-ins -------------------------------------------------------------------------------------------------------
def _edm_trace(monkeypatch, mode, which, self_cond=False):
    from tests import test_edm_sampler_trace_host as T
    for op in ('cell_project_profile', 'tile_project', 'slab_project', 'band_project'):
        monkeypatch.setitem(T.RETURNS, op, T._into('x0'))
    extra = dict(MODES[mode][0], **({} if which is None else dict(consistency_heun=which)))
    monkeypatch.setitem(T.CASES, 'heun-dc', T.sample_case(dict(self_cond=self_cond), consistency=None if which is None else 0.5, **extra))
    return T.run_case('heun-dc')[0]


@pytest.mark.parametrize('which', HD.WHICH)
@pytest.mark.parametrize('mode', list(MODES))
def test_per_window_loop_projects_after_each_projected_evaluation(mode, which, monkeypatch):
    """One projection launch of the mode after every projected evaluation, on the operands ``cell_project`` would get -- the clamped
    prediction the preconditioning just made, the measurement, the cell, the weight, no clamp, a fresh output -- and everything
    downstream reads the projected tensor.  Draws and every other launch are the plain loop's."""
    plain = _edm_trace(monkeypatch, 'cell', None, self_cond=True)
    got = _edm_trace(monkeypatch, mode, which, self_cond=True)
    op = MODES[mode][1]
    every = [m[1] for m in MODES.values()]
    assert not any(r['op'] in every for r in plain)
    want = 2 * T_STEPS - 1 if which == 'both' else T_STEPS
    assert sum(r['op'] == op for r in got) == want and not any(r['op'] in every and r['op'] != op for r in got)
    assert [r['op'] for r in got if r['op'] != op] == [r['op'] for r in plain]               # nothing else is added, dropped or moved
    tables, evaluations, last = set(), 0, None
    for k, r in enumerate(got):
        if r['op'] == 'unet':
            evaluations += 1
        if r['op'] != op:
            continue
        before = got[k - 1]
        assert before['op'] == 'axpby3' and r['x0'] == before['->']                        # the prediction, as it left the clamp
        assert r['cell'] == [2, 2, 4] and r['weight'] == 0.5 and r['clamp'] is None and r['out'] is None
        assert r['target' if mode in ('tile', 'band') else 'meas_up']['t'].startswith('meas_up')
        if 'table' in r:
            tables.add(str(r['table']))
        # what reads the prediction next reads the projected one: the predictor update, or the corrector's two launches (the first
        # reads the projected predictor prediction again), and the self-conditioning of the next evaluation
        updates = [q for q in got[k + 1:] if q['op'] == 'axpby3']
        if evaluations % 2:                                                                # stage 0: at sigma_hat
            assert updates[0]['b'] == r['->']
        else:
            assert updates[0]['b'] == last and updates[1]['b'] == r['->']
        following = [q for q in got[k + 1:] if q['op'] == 'unet'][:1]
        assert all(q['self_cond'] == r['->'] for q in following)
        last = r['->']
    assert evaluations == 2 * T_STEPS - 1 and len(tables) == (0 if mode == 'cell' else 1)     # one table per chain
    if which == 'predictor':                                                               # the corrector's prediction stays the network's
        stage1 = [k for k, r in enumerate(got) if r['op'] == 'unet'][1::2]
        assert all(got[k + 2]['op'] != op for k in stage1)


def _volume_case(monkeypatch, name, fn=None, **extra):
    """One ``VolumeInference`` case of the launch-trace module with consistency switched on; returns (trace, the chains made)."""
    from diffusioniqt_amd import consistency, ops
    from tests import test_volume_launch_trace_host as T
    monkeypatch.setitem(T.RETURNS, 'cell_replicate', lambda a: ops.cell_replicate(a['meas'], a['cell']))
    monkeypatch.setitem(T.RETURNS, 'tile_backproject', lambda a: torch.full((40, 36, 44), 300.0))
    monkeypatch.setitem(T.RETURNS, 'volume_joint_consistent_heun', lambda a: (a['xh'], a['xn'], a['x0']))
    monkeypatch.setattr(T.StubDenoiser, 'state_space', lambda self, x: self.rec.record('state_space', {'x': x}, x), raising=False)
    made = []
    real = getattr(consistency.Chain.__init__, 'real', consistency.Chain.__init__)        # a second case of one test counts afresh

    def counted(self, *a, **k):
        made.append(self)
        real(self, *a, **k)
    counted.real = real
    monkeypatch.setattr(consistency.Chain, '__init__', counted)
    case = dict(T.CASES[name])
    case['kw'] = dict(case['kw'], **extra)
    if fn is not None:
        case['fn'] = fn
    monkeypatch.setitem(T.CASES, 'heun-dc-case', case)
    return T.run_case('heun-dc-case'), made


OK_A = TR.stack_matrix((2, 2, 2), (0, 1, 2))
JOINT_MODES = {'cell': {}, 'profile': dict(consistency_profile=((1, 2), (1, 1), (3, 1))), 'tile': dict(consistency_operator=OK_A)}


@pytest.mark.parametrize('which', HD.WHICH)
@pytest.mark.parametrize('mode', list(JOINT_MODES))
def test_joint_chain_takes_the_fused_launch_in_the_projected_phases(mode, which, monkeypatch):
    """S = 2 samples of T = 3 Heun steps, the last without a corrector: 2 (2 T - 1) phase launches as without consistency, phase 1
    always the consistent one, phase 2 under ``'both'``; ONE chain per volume; every operand the plain launch's."""
    plain, none = _volume_case(monkeypatch, 'joint-heun-selfcond')
    meas = torch.full((20, 18, 22), 300.0)
    if mode == 'tile':
        meas = meas.expand(OK_A.shape[0], -1, -1, -1).contiguous()
    got, made = _volume_case(monkeypatch, 'joint-heun-selfcond', consistency=(meas, (2, 2, 2)), consistency_weight=0.5,
                             consistency_heun=which, **JOINT_MODES[mode])
    old, new = 'volume_joint_heun', 'volume_joint_consistent_heun'
    assert not none and len(made) == 1                                                     # one Chain per volume
    assert sum(r['op'] == old for r in plain) == 2 * (2 * 3 - 1) and not any(r['op'] == new for r in plain)
    phases = [(r['op'], r['phase']) for r in got if r['op'] in (old, new)]
    assert phases == [(new if p == 1 or which == 'both' else old, p) for _, p in phases]
    assert [p for _, p in phases] == [r['phase'] for r in plain if r['op'] == old] == [1, 2, 1, 2, 1] * 2
    assert sum(r['op'] in ('cell_replicate', 'tile_backproject') for r in got) == 1 and sum(r['op'] == 'state_space' for r in got) == 1
    fused = [r for r in got if r['op'] == new]
    assert {r['mode'] for r in fused} == {mode} and {r['weight'] for r in fused} == {0.5} and {tuple(r['cell']) for r in fused} == {(2, 2, 2)}
    assert len({str(r['meas_up']) for r in fused}) == 1 and len({str(r['table']) for r in fused}) == 1
    assert (fused[0]['table'] is None) == (mode == 'cell')
    if mode != 'cell':
        assert fused[0]['table']['shape'] == ([2, 8] if mode == 'profile' else [8, 8])
    # every other operand is the plain launch's: drop what only the consistent one has, then only the name differs
    own = ('meas_up', 'cell', 'table', 'weight', 'mode')
    rest = [{k: v for k, v in r.items() if k not in own} for r in got if r['op'] not in ('cell_replicate', 'tile_backproject', 'state_space')]
    from tests import launch_trace as LT
    assert LT.canonical(rest).replace(new, old) == LT.canonical(plain)


@pytest.mark.parametrize('which', [None, 'both', 'predictor'])
def test_crop_and_blend_modes_hand_the_keyword_on_exactly_when_it_was_given(which, monkeypatch):
    for name in ('blend-gaussian-s2-anchored', 'crop-s16'):
        seen = []

        def sampler_of(rec):
            def sample(x, noise=None, **kw):
                seen.append(kw)
                return torch.zeros_like(x)
            return sample
        extra = {} if which is None else dict(consistency_heun=which)
        _volume_case(monkeypatch, name, fn=sampler_of, consistency=(torch.full((20, 18, 22), 300.0), (2, 2, 2)), consistency_weight=0.5, **extra)
        assert seen
        for kw in seen:
            assert set(kw) == {'consistency', 'consistency_weight'} | set(extra) and kw.get('consistency_heun') == which
