"""Host-side checks of noise-aware data consistency, ``consistency_noise=`` (no GPU here): ``ops.consistency_noise_schedule`` against
the float64 restatement of tests/volume_joint_noise_reference.py, the variance identity DDNM+ rests on (analytically, no sampling),
the shaped normals of the fp32 restatement, every refusal before anything touches the device, the error codes of the two new entries
and -- with the recording stand-ins of tests/launch_trace.py -- the per-step dispatch of both sampler families and of the joint chain,
row by row."""
import math

import numpy as np
import pytest
import torch

from tests import edm_dpmpp2m_reference as E
from tests import launch_trace as LT
from tests import volume_blend_reference as R
from tests import volume_joint_heun_reference as HN
from tests import volume_joint_noise_reference as NR
from tests import volume_joint_profile_reference as PR
from tests.test_volume_joint_host import _imagen

SIGMA = 0.2                                                  # in state units
CELL = (2, 2, 2)


def _tables():
    """The project's own host tables as rows (kx, k0, kp, kn), float64: cosine ddpm and ddim eta 0.5 at 4 steps, the EDM Karras
    chain 80 -> 0.002 at 4 steps with eta 1 and 0.5."""
    from diffusioniqt_amd.elucidated_imagen import ElucidatedImagen
    from diffusioniqt_amd.imagen_pytorch3D import GaussianDiffusionContinuousTimes, Imagen
    sch = GaussianDiffusionContinuousTimes(noise_schedule='cosine', timesteps=1000)
    out = {}
    for name, sampler, eta in (('ddpm', 'ddpm', 0.0), ('ddim-0.5', 'ddim', 0.5)):
        coefs = Imagen._sampler_tables(sch, 2, sampler, 4, None, eta, 'x_start')[0]
        assert bool((coefs == coefs[:, :, :1]).all())        # batch-uniform
        out[name] = NR.rows4(coefs[:, :, 0].numpy())
    sigmas = torch.tensor(E.karras64(4), dtype=torch.float32)
    for eta in (1.0, 0.5):
        out[f'edm-{eta}'] = ElucidatedImagen.dpmpp2m_coefficients(None, sigmas, eta).numpy().astype(np.float64)
    return out


TABLES = _tables()
OPERATORS = {'plain': None, 'profile': NR.PROFILE_222}


def _table(kind):
    return None if OPERATORS[kind] is None else PR.profile_table(CELL, OPERATORS[kind])


# ---- N1: the schedule -------------------------------------------------------------------------------------------------------------------------
def test_cell_norm_is_the_restatement():
    from diffusioniqt_amd import ops
    for cell in ((2, 2, 2), (4, 1, 1), (1, 1, 7)):
        assert ops.cell_norm(cell) == 1.0 / math.sqrt(cell[0] * cell[1] * cell[2]) == NR.cell_norm64(cell)
    for cell, profile in list(PR.PROFILES.values()) + [(CELL, NR.PROFILE_222)]:
        host = ops.cell_profile(cell, profile)
        s = ops.cell_norm(cell, host)
        assert isinstance(s, float) and s == NR.cell_norm64(cell, PR.profile_table(cell, profile))
        u = host[0].double().numpy()
        assert abs(s * s - float((u * u).sum())) <= 1e-15 and s >= 1.0 / math.sqrt(len(u)) - 1e-7      # the uniform profile has the least norm
    with pytest.raises(ValueError, match="consistency"):
        ops.cell_norm((1, 1, 1))
    with pytest.raises(ValueError, match="consistency profile table"):
        ops.cell_norm((2, 2, 2), torch.zeros(2, 4))


@pytest.mark.parametrize('w', [1.0, 0.5])
@pytest.mark.parametrize('kind', list(OPERATORS))
@pytest.mark.parametrize('name', list(TABLES))
def test_schedule_is_the_restatement(name, kind, w):
    from diffusioniqt_amd import ops
    rows, table = TABLES[name], _table(kind)
    s = ops.cell_norm(CELL, None if table is None else torch.from_numpy(table))
    got = ops.consistency_noise_schedule(torch.from_numpy(rows), s, SIGMA, w)
    want = NR.schedule64(rows, NR.cell_norm64(CELL, table), SIGMA, w)
    assert got.dtype == torch.float64 and tuple(got.shape) == (4, 2) and not got.is_cuda
    got = got.numpy()
    print(f"{name} {kind} w {w}: (w_i, shrink_i) = {[(round(a, 4), round(b, 4)) for a, b in got.tolist()]}")
    assert np.abs(got - want).max() <= 1e-15 * np.abs(want).max()
    assert np.array_equal(got, ops.consistency_noise_schedule(rows.tolist(), s, SIGMA, w).numpy())       # a list of rows is the same call
    weight, shrink = got[:, 0], got[:, 1]
    assert ((0 <= weight) & (weight <= w)).all() and ((0 <= shrink) & (shrink <= 1)).all()
    assert rows[-1, 3] == 0 and weight[-1] == 0              # the plain last step
    for i in range(4):
        assert (weight[i] == 0) == (rows[i, 3] == 0)
    assert any(weight[i] == w and 0 < shrink[i] < 1 for i in range(4))                      # full weight with a partial shrink


def test_the_inputs_exercise_every_kind_of_row():
    """Over the inputs above together: a row with weight = w and 0 < shrink < 1, a row with weight < w and shrink = 1, a last row
    with weight 0 -- for both caps."""
    from diffusioniqt_amd import ops
    for w in (1.0, 0.5):
        full = reduced = last = 0
        for rows in TABLES.values():
            for kind in OPERATORS:
                table = _table(kind)
                s = ops.cell_norm(CELL, None if table is None else torch.from_numpy(table))
                sched = ops.consistency_noise_schedule(rows, s, SIGMA, w).tolist()
                full += sum(a == w and 0 < b < 1 for a, b in sched)
                reduced += sum(0 < a < w and b == 1 for a, b in sched)
                last += sched[-1] == [0.0, 0.0]
        assert full and reduced and last == len(TABLES) * len(OPERATORS), (w, full, reduced, last)


def test_the_schedule_of_the_issue():
    """The figures the method was checked with: 4-step cosine ddpm and the 4-step EDM eta = 1 chain, cell (2, 2, 2), sigma_y = 0.2."""
    from diffusioniqt_amd import ops
    s = ops.cell_norm(CELL)
    ddpm = ops.consistency_noise_schedule(TABLES['ddpm'], s, SIGMA, 1.0).numpy()
    assert np.abs(ddpm - [[1, 0.027], [1, 0.139], [0.828, 1], [0, 0]]).max() <= 5e-4
    edm = ops.consistency_noise_schedule(TABLES['edm-1.0'], s, SIGMA, 1.0).numpy()
    assert np.abs(edm - [[1, 0.002], [0.902, 1], [0.429, 1], [0, 0]]).max() <= 5e-4


def test_a_tiny_sigma_is_the_constant_weight_with_no_shrink_in_fp32():
    from diffusioniqt_amd import ops
    for name, rows in TABLES.items():
        sched = ops.consistency_noise_schedule(rows, ops.cell_norm(CELL), 1e-12, 0.5)
        rows32 = ops.consistency_noise_dispatch(sched)
        assert all(isinstance(v, float) for r in rows32 for v in r)
        assert [r for r in rows32[:-1]] == [(0.5, 0.0)] * 3 and rows32[-1] == (0.0, 0.0), name          # the existing launch


def test_schedule_argument_errors():
    from diffusioniqt_amd import ops
    with pytest.raises(ValueError, match="consistency_noise"):
        ops.consistency_noise_schedule([[0.5, -0.25, 0.0, 0.125]], 0.5, 0.2, 1.0)
    with pytest.raises(ValueError, match="consistency_noise"):
        ops.consistency_noise_schedule([[0.5, 0.0, 0.0, 0.125]], 0.5, 0.2, 1.0)
    assert ops.consistency_noise_schedule([[0.5, -0.25, 0.0, 0.0]], 0.5, 0.2, 1.0).tolist() == [[0.0, 0.0]]    # kn == 0: k0 is not looked at
    with pytest.raises(ValueError, match="rows"):
        ops.consistency_noise_schedule([[0.5, 0.25, 0.125]], 0.5, 0.2, 1.0)


# ---- N2: the variance identity, analytically -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('w', [1.0, 0.5])
@pytest.mark.parametrize('sigma', [0.05, 0.2, 1.0])
@pytest.mark.parametrize('kind', list(OPERATORS) + ['trapezoid'])
@pytest.mark.parametrize('name', list(TABLES))
def test_variance_identity(name, kind, sigma, w):
    """Per scheduled row, on one cell: the measurement noise the step carries, a_i A+ n_y with A+ n_y = g n_y, plus the fresh noise
    kn Phi eps, Phi = I - shrink g u^T, has the covariance (a_i sigma_y)^2 g g^T + kn^2 Phi Phi^T.  Wherever the weight is not capped
    (rho = 0 or a_i = b) or rho closes the budget this is kn^2 I exactly: the range of A gets kn^2, the null space keeps kn^2."""
    from diffusioniqt_amd import ops
    cell, profile = (CELL, OPERATORS[kind]) if kind in OPERATORS else PR.PROFILES[kind]
    n = cell[0] * cell[1] * cell[2]
    table = None if profile is None else ops.cell_profile(cell, profile)
    u = np.full(n, 1.0 / n) if table is None else table[0].double().numpy()
    g = u / (u * u).sum()
    rows = TABLES[name]
    sched = ops.consistency_noise_schedule(rows, ops.cell_norm(cell, table), sigma, w).numpy()
    w_prev, checked = 0.0, 0
    for (kx, k0, kp, kn), (w_i, shrink) in zip(rows.tolist(), sched.tolist()):
        if w_i > 0:
            a = k0 * w_i + kp * w_prev
            phi = np.eye(n) - shrink * np.outer(g, u)
            cov = (a * sigma) ** 2 * np.outer(g, g) + kn ** 2 * phi @ phi.T
            assert np.abs(cov - kn ** 2 * np.eye(n)).max() <= 1e-12 * kn ** 2, (name, kind, sigma, w, w_i, shrink)
            checked += 1
        w_prev = w_i
    assert checked >= 2


# ---- N3: the shaped normals of the fp32 restatement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('row', [0, 1, 2, 'full'])
@pytest.mark.parametrize('name', ['uniform-222', 'uniform-411'] + list(PR.PROFILES))
def test_shaped_normals_keep_rho_of_the_measured_component(name, row):
    """u . eps' = rho (u . eps) on every fully covered cell, within the rounding count of ONE projection (weight = shrink, S = the
    largest |eps|); a gap voxel (g = 0) keeps its bits, and so does every voxel of a cell with an uncovered voxel.  The shrink is the
    one the library schedules for this operator on row ``row`` of the 4-step ddpm chain, in fp32 as a launch gets it ('full': 1, rho = 0)."""
    from diffusioniqt_amd import ops
    cell, profile = {'uniform-222': ((2, 2, 2), None), 'uniform-411': ((4, 1, 1), None)}.get(name) or PR.PROFILES[name]
    table = None if profile is None else PR.profile_table(cell, profile)
    s = ops.cell_norm(cell, None if profile is None else ops.cell_profile(cell, profile))
    sched = ops.consistency_noise_dispatch(ops.consistency_noise_schedule(TABLES['ddpm'], s, SIGMA, 1.0))
    w, shrink = (1.0, 1.0) if row == 'full' else sched[row]
    assert w > 0 and 0 < shrink <= 1
    rng = np.random.default_rng(3)
    eps = rng.standard_normal((8, 8, 16)).astype(np.float32)
    covered = np.ones(eps.shape, dtype=bool)
    covered[5, 3, 9] = False
    got = NR.shape_noise32(eps, cell, table, shrink, covered)
    assert got.dtype == np.float32
    whole = NR.replicate(NR._cells(covered, cell).all(axis=(-5, -3, -1)), cell)
    assert np.array_equal(got.view(np.uint32)[~whole], eps.view(np.uint32)[~whole]) and (~whole).sum() == cell[0] * cell[1] * cell[2]
    wide = np.full((2, cell[0] * cell[1] * cell[2]), 1.0 / (cell[0] * cell[1] * cell[2])) if table is None else table
    before, after = PR.cell_wmean64(eps, cell, wide), PR.cell_wmean64(got, cell, wide)
    cells = whole[::cell[0], ::cell[1], ::cell[2]]
    count = NR.shaping_roundings(cell, table, shrink, float(np.abs(eps).max()))
    err = np.abs(after - (1.0 - shrink) * before)[cells].max()
    print(f"{name} shrink {shrink}: |u . eps' - rho u . eps| = {err:.3e}, count {count:.3e}")
    assert err <= count
    assert np.array_equal(after[~cells], before[~cells])
    if table is not None:
        gap = PR.gains(table, cell, eps.shape) == 0
        assert np.array_equal(got.view(np.uint32)[gap], eps.view(np.uint32)[gap]) and gap.any() == (name == 'gap')
    ref = NR.shape_noise64(eps, covered, cell, table if table is None else table.astype(np.float64), shrink)
    assert np.abs(got - ref).max() <= count                  # and the whole field is the float64 shaping within that count
    x0 = (rng.standard_normal(eps.shape) * 2).astype(np.float32)
    meas = NR.replicate(rng.standard_normal(tuple(s // f for s, f in zip(eps.shape, cell))).astype(np.float32), cell)
    a, b = NR.project_noise32(x0, meas, eps, cell, table, 0.5, shrink, (-1., 1., 1))
    assert np.array_equal(a, NR.project32(np.clip(x0, -1, 1), meas, cell, table, 0.5)) and np.array_equal(b[whole], got[whole])


# ---- N4: refusals, all before the device is touched -----------------------------------------------------------------------------------------
def _meas(P=16, B=2):
    return torch.zeros(B, 1, P, P, P)


BAD_VALUES = (True, False, 'high', [0.2], float('nan'), float('inf'), 0, 0.0, -0.1)


def test_sample_refuses_consistency_noise_it_cannot_honour():
    imagen = _imagen()
    lr = torch.zeros(2, 1, 16, 16, 16)
    base = dict(batch_size=2, start_image_or_video=lr, start_at_unet_number=2, use_tqdm=False, sampler='ddim', sample_steps=2, eta=0.5)
    ok = (_meas(), (2, 2, 2))
    bad = [dict(consistency_noise=0.2)]                                                     # without consistency
    bad += [dict(consistency=ok, consistency_noise=v) for v in BAD_VALUES]
    bad += [dict(consistency=ok, consistency_noise=0.2, eta=0.0),                           # no stochastic row
            dict(consistency=ok, consistency_noise=0.2, sampler='dpmpp2m', eta=0.0),
            dict(consistency=ok, consistency_noise=0.2, init_images=lr),                    # what consistency already refuses
            dict(consistency=ok, consistency_noise=0.2, sampler='ddpm', sample_steps=None, eta=0.0, skip_steps=2),
            dict(consistency=ok, consistency_noise=0.2, sampler='ddpm', eta=0.0, inpaint_images=lr, inpaint_masks=lr[:, 0].bool()),
            dict(consistency=ok, consistency_noise=0.2, consistency_weight=0.0),
            dict(consistency=(_meas(), (3, 1, 1)), consistency_noise=0.2)]
    for kw in bad:
        with pytest.raises(ValueError, match="consistency_noise"):
            imagen.sample(**{**base, **kw})
    with pytest.raises(ValueError, match="consistency_weight"):                            # the deterministic refusal says what to use
        imagen.sample(**{**base, 'consistency': ok, 'consistency_noise': 0.2, 'eta': 0.0})
    loop = dict(noise_scheduler=imagen.noise_schedulers[1], pred_objective='x_start', sampler='ddim', sample_steps=2)
    for kw in (dict(consistency_noise=0.2, eta=0.5), dict(consistency=ok, consistency_noise=0.0, eta=0.5),
               dict(consistency=ok, consistency_noise=0.2, eta=0.0)):
        with pytest.raises(ValueError, match="consistency_noise"):                         # the loop itself applies the same rules
            imagen.p_sample_loop(imagen.unets[1], (2, 1, 16, 16, 16), **loop, **kw)


def test_edm_sample_refuses_consistency_noise_it_cannot_honour():
    elu = HN.make_elucidated('churn-on', False)
    lr = torch.zeros(2, 1, 16, 16, 16)
    base = dict(batch_size=2, video_frames=16, start_image_or_video=lr, start_at_unet_number=2, use_tqdm=False, sampler='dpmpp2m', eta=1.0)
    ok = (_meas(), (2, 2, 2))
    bad = [dict(consistency_noise=0.2)]
    bad += [dict(consistency=ok, consistency_noise=v) for v in BAD_VALUES]
    bad += [dict(consistency=ok, consistency_noise=0.2, eta=0.0),                           # the ODE solver: no stochastic row
            dict(consistency=ok, consistency_noise=0.2, sampler='heun', eta=0.0),
            dict(consistency=ok, consistency_noise=0.2, init_images=lr),
            dict(consistency=ok, consistency_noise=0.2, consistency_weight=2),
            dict(consistency=(_meas(P=8), (2, 2, 2)), consistency_noise=0.2)]
    for kw in bad:
        with pytest.raises(ValueError, match="consistency_noise"):
            elu.sample(**{**base, **kw})
    with pytest.raises(ValueError, match="consistency_noise"):
        elu.sample(**{**base, 'sampler': 'heun', 'eta': 0.0, 'consistency': ok, 'consistency_noise': 0.2, 'inpaint_images': lr,
                      'inpaint_masks': lr[:, 0].bool()})
    with pytest.raises(ValueError, match="consistency_weight"):
        elu.sample(**{**base, 'consistency': ok, 'consistency_noise': 0.2, 'eta': 0.0})
    for kw in (dict(consistency_noise=0.2, eta=1.0), dict(consistency=ok, consistency_noise=-1.0, eta=1.0),
               dict(consistency=ok, consistency_noise=0.2, eta=0.0)):
        with pytest.raises(ValueError, match="consistency_noise"):
            elu.one_unet_sample(elu.unets[1], (2, 1, 16, 16, 16), unet_number=2, sampler='dpmpp2m', **kw)


class _NeverDenoiser:
    num_steps, clamp = 3, (-1., 1., 1)

    def __init__(self, coefs, **attrs):
        self.coefs = torch.tensor(coefs)
        self.__dict__.update(attrs)

    def x0(self, *a, **k):
        raise AssertionError("the network must not run")
    finish = x0
    state_space = x0


def test_volume_inference_consistency_noise_argument_errors():
    from diffusioniqt_amd.inference import VolumeInference

    def never(x, **kw):
        raise AssertionError("the sampler must not run")
    cfg = R.shared_cfg(8)
    ok = (torch.zeros(20, 18, 22), (2, 2, 2))
    joint = dict(blend='gaussian', noise='anchored', joint=True)
    with pytest.raises(ValueError, match="consistency_noise"):
        VolumeInference(cfg, never, consistency_noise=40.0)
    for v in BAD_VALUES:
        with pytest.raises(ValueError, match="consistency_noise"):
            VolumeInference(cfg, never, consistency=ok, consistency_noise=v)
    noisy = [[0.5, 0.25, 0.125]] * 3
    for den in (_NeverDenoiser([[0.5, 0.25, 0.0]] * 3),                                     # ddim eta 0: kn == 0 on every row
                _NeverDenoiser(noisy, multistep=True),                                      # the DDPM family's dpmpp2m: (kx, k0, kp)
                _NeverDenoiser([[0.5, 0.25, -0.1, 0.0]] * 3, multistep=True, sigma0=1.5, draw_base=1)):   # EDM dpmpp2m eta 0
        with pytest.raises(ValueError, match="consistency_weight"):
            VolumeInference(cfg, den, consistency=ok, consistency_noise=40.0, **joint)
        with pytest.raises(ValueError, match="consistency_noise"):
            VolumeInference(cfg, den, consistency=ok, consistency_noise=40.0, **joint)
    # everything consistency refuses names consistency_noise too while one is given
    known = (torch.zeros(40, 36, 44), torch.zeros(40, 36, 44, dtype=torch.bool))
    meas = ok[0]
    for kw in (dict(consistency=ok, inpaint=known), dict(consistency=(meas, (1, 1, 1))), dict(consistency=(meas, (4, 4, 8))),
               dict(consistency=(meas, (2, 2))), dict(consistency=ok, consistency_weight=0.0), dict(consistency=ok, consistency_weight=1.25),
               dict(consistency=(meas.long(), (2, 2, 2))), dict(consistency=(meas[0], (2, 2, 2))), dict(consistency=meas),
               dict(consistency=(meas, (1, 1, 3))),                                        # 3 divides neither the stride nor the window
               dict(consistency=ok, consistency_profile=((1, 2), (1, 1), (1, -1)))):
        with pytest.raises(ValueError, match="consistency_noise"):
            VolumeInference(cfg, never, consistency_noise=40.0, **kw)
    with pytest.raises(ValueError, match="consistency_noise"):                             # the Heun denoiser stays refused
        VolumeInference(cfg, HN.make_elucidated('churn-on', False).window_denoiser(), consistency=ok, consistency_noise=40.0, **joint)
    with pytest.raises(ValueError, match="consistency_noise"):                             # joint, together with inpainting
        VolumeInference(cfg, _imagen().window_denoiser(sampler='ddpm', sample_steps=3), consistency=ok, inpaint=known,
                        consistency_noise=40.0, **joint)
    lacking = type('NoMap', (), dict(num_steps=3, coefs=torch.tensor(noisy), clamp=(-1., 1., 1), x0=None, finish=None))()
    with pytest.raises(ValueError, match="consistency_noise"):                             # no state_space map
        VolumeInference(cfg, lacking, consistency=ok, consistency_noise=40.0, **joint)
    with pytest.raises(ValueError, match="consistency_noise"):                             # in __call__: not the volume's shape
        VolumeInference(cfg, never, consistency=ok, consistency_noise=40.0)(torch.zeros(40, 36, 48))
    with pytest.raises(ValueError, match="consistency") as plain:                          # and without one the message is as it was
        VolumeInference(cfg, never, consistency=ok, inpaint=known)
    assert 'consistency_noise' not in str(plain.value)
    inf = VolumeInference(cfg, _NeverDenoiser(noisy), consistency=ok, consistency_noise=40, **joint)
    assert inf.consistency_noise == 40.0 and isinstance(inf.consistency_noise, float)
    assert VolumeInference(cfg, never, consistency=ok).consistency_noise is None           # the default is today's path


def test_ops_refuse_a_bad_shrink_before_the_library():
    from diffusioniqt_amd import ops
    x = torch.zeros(2, 1, 8, 8, 8)
    for shrink in (0.0, -0.5, 1.5, True, None):
        with pytest.raises(ValueError, match="consistency_noise"):
            ops.cell_project_noise(x, x.clone(), x.clone(), (2, 2, 2), 1.0, shrink)
    vol = torch.zeros(8, 8, 8)
    for form, kn, shrink in ((1, 0.5, 0.5), (0, 0.0, 0.5), (2, 0.5, 0.0), (3, 0.5, 0.5)):
        with pytest.raises(ValueError, match="volume_joint_consistent_noise_step"):
            ops.volume_joint_consistent_noise_step(None, None, None, vol, None, vol, (2, 2, 2), None, 1.0, shrink, form, 1.0, 0.5, 0.0, kn,
                                                   -1.0, 1.0, 1, 4)


def test_noise_entries_return_error_codes():
    from diffusioniqt_amd import _lib
    lib = _lib.load()
    buf = (np.zeros(4, dtype=np.int32)).ctypes.data                             # never dereferenced: every call below is refused

    def proj(ptrs=(buf, buf, buf, None, buf, buf), cubes=3, P=8, cell=(2, 2, 2), w=1.0, shrink=0.5, mode=2):
        return lib.diqt_cell_project_noise(*ptrs, cubes, P, *cell, w, shrink, -1.0, 1.0, mode, None)
    for k in (0, 1, 2, 4, 5):                                                   # the table alone may be NULL: the plain mean
        assert proj(tuple(None if i == k else p for i, p in enumerate((buf, buf, buf, buf, buf, buf)))) == -2, k
    assert b"null pointer" in lib.diqt_last_error()
    assert proj(w=0.0) == -3 and proj(w=1.5) == -3
    assert proj(shrink=0.0) == -3 and proj(shrink=-0.25) == -3 and proj(shrink=1.0001) == -3
    assert b"shrink" in lib.diqt_last_error()
    assert proj(cell=(1, 1, 1)) == -3 and proj(cell=(8, 8, 2)) == -3 and proj(mode=3) == -3
    assert proj(cell=(1, 1, 3)) == -1 and proj(cubes=0) == -1
    geo = (40, 36, 44, 16, 8, 4, 3, 4)                                          # D, H, W, P, stride and the lattice of range(0, n - 15, 8)

    def step(ptrs=(buf,) * 9, form=0, geo=geo, cell=(2, 2, 2), w=1.0, shrink=0.5, kn=0.25, mode=0):
        return lib.diqt_volume_joint_consistent_noise_step(*ptrs, form, 3, *geo, *cell, w, shrink, 1.0, 0.5, 0.0, kn, -1.0, 1.0, mode, 0, 1,
                                                           0, None)
    assert step(form=1) == -3                                                   # the multistep form has no normal
    assert b"form" in lib.diqt_last_error()
    assert step(form=3) == -3 and step(form=-1) == -3
    assert step(kn=0.0) == -3 and step(form=2, kn=0.0) == -3
    assert b"kn" in lib.diqt_last_error()
    assert step(shrink=0.0) == -3 and step(shrink=1.5) == -3 and step(shrink=-1.0) == -3
    assert b"shrink" in lib.diqt_last_error()
    assert step(w=0.0) == -3 and step(cell=(1, 1, 1)) == -3 and step(mode=2) == -3
    for k in (0, 1, 2, 3, 5, 7, 8):                                             # x0_prev and the table may be NULL
        assert step(tuple(None if i == k else buf for i in range(9))) == -2, k
    assert step(cell=(3, 1, 1)) == -1 and step(geo=(40, 36, 44, 16, 8, 4, 3, 5)) == -1


# ---- N5: the dispatch, with recording stand-ins -------------------------------------------------------------------------------------------
HOST_ONLY = ('consistency_cell', 'cell_profile', 'cell_norm', 'consistency_noise_sigma', 'consistency_noise_schedule',
             'consistency_noise_dispatch')


def _host(returns):
    from diffusioniqt_amd import ops
    for name in HOST_ONLY:
        returns[name] = (lambda f: lambda a: f(**a))(getattr(ops, name))                    # host only: the real rules
    return returns


def _launches(trace):
    return [r for r in trace if r['op'] not in HOST_ONLY]


def _imagen_trace(sampler, eta, **extra):
    from diffusioniqt_amd import imagen_pytorch3D
    into = lambda key: (lambda a: a['out'] if a.get('out') is not None else torch.zeros_like(a[key]))
    both = lambda a: (a['out'] if a['out'] is not None else torch.zeros_like(a['x0']),
                      a['out_noise'] if a['out_noise'] is not None else torch.zeros_like(a['noise']))
    returns = _host({'axpby3': lambda a: torch.zeros_like(a['a']), 'ddpm_step': lambda a: (torch.zeros_like(a['x_t']), torch.zeros_like(a['x_t'])),
                     'cell_project': into('x0'), 'cell_project_profile': into('x0'), 'cell_project_noise': both})
    rec = LT.Recorder()
    imagen = _imagen()
    lr, meas = torch.zeros(2, 1, 16, 16, 16), torch.full((2, 1, 16, 16, 16), 0.125)
    rec.tag(lr, 'lowres'), rec.tag(meas, 'meas_up')
    noise = [LT.zeros(2, 1, 16, 16, 16) for _ in range(8)]
    for k, t in enumerate(noise):
        rec.tag(t, f'noise{k}')
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(imagen_pytorch3D, 'ops', LT.RecordingOps(rec, returns))
        out = imagen.sample(batch_size=2, start_image_or_video=lr, start_at_unet_number=2, use_tqdm=False, device='cpu', sampler=sampler,
                            sample_steps=4, eta=eta, noise=noise, consistency=(meas, (2, 2, 4)), consistency_weight=0.75, **extra)[0]
    rec.record('return', {}, out)
    return rec.trace, imagen


@pytest.mark.parametrize('sampler,eta', [('ddpm', 0.0), ('ddim', 0.5), ('ddim', 0.0), ('dpmpp2m', 0.0)])
def test_imagen_sample_without_a_value_is_the_trace_with_the_keyword_absent(sampler, eta):
    absent, _ = _imagen_trace(sampler, eta)
    none, _ = _imagen_trace(sampler, eta, consistency_noise=None)
    assert LT.canonical(absent) == LT.canonical(none) and not any(r['op'] in HOST_ONLY[2:] or r['op'] == 'cell_project_noise' for r in none)


def _want_dispatch(rows, cell, table, sigma, cap):
    sched = NR.dispatch(NR.schedule64(rows, NR.cell_norm64(cell, table), sigma, cap))
    return [(float(w), float(s)) for w, s in sched]


@pytest.mark.parametrize('profile', [None, ((1, 2), (1, 1), (1, 3, 3, 0))])
@pytest.mark.parametrize('sigma', [SIGMA, 1e-12])
@pytest.mark.parametrize('sampler,eta', [('ddpm', 0.0), ('ddim', 0.5)])
def test_imagen_sample_dispatches_row_by_row(sampler, eta, sigma, profile):
    from diffusioniqt_amd.imagen_pytorch3D import Imagen
    extra = {} if profile is None else dict(consistency_profile=profile)
    plain, imagen = _imagen_trace(sampler, eta, **extra)
    got, _ = _imagen_trace(sampler, eta, consistency_noise=sigma, **extra)
    coefs = Imagen._sampler_tables(imagen.noise_schedulers[1], 2, sampler, 4, None, eta, 'x_start')[0][:, :, 0].numpy()
    cell = (2, 2, 4)
    table = None if profile is None else PR.profile_table(cell, profile)
    want = _want_dispatch(NR.rows4(coefs), cell, table, sigma, 0.75)
    lo, hi, mode = imagen._clamp_cfg()
    project = 'cell_project' if profile is None else 'cell_project_profile'
    steps = [r for r in _launches(got) if r['op'] == 'ddpm_step']
    projections = [r for r in _launches(got) if r['op'] in ('cell_project', 'cell_project_profile', 'cell_project_noise')]
    assert len(steps) == 4 and [r['op'] for r in _launches(plain) if r['op'] != 'ddpm_step' and r['op'] != 'return'].count(project) == 4
    kinds = []
    for i, (w, shrink) in enumerate(want):
        step = steps[i]
        if w == 0:                                            # the plain step with the chain's own clamp, no projection launch
            kinds.append('plain')
            assert (step['lo'], step['hi'], step['clamp_mode']) == (LT.f32(lo), LT.f32(hi), mode)
            assert step['noise']['t'] == f'noise{i + 1}#0'
            continue
        p = projections.pop(0)
        assert (step['lo'], step['hi'], step['clamp_mode']) == ('-inf', 'inf', 1)           # a projected step clamps no more
        assert step['pred']['t'] == (p['->'][0]['t'] if p['op'] == 'cell_project_noise' else p['->']['t'])
        assert p['weight'] == w and p['clamp'] == [LT.f32(lo), LT.f32(hi), mode] and p['cell'] == [2, 2, 4]
        assert (p.get('table') is None) == (profile is None)
        if shrink == 0:                                       # the existing consistent launch with that weight
            kinds.append('constant')
            assert p['op'] == project and step['noise']['t'] == f'noise{i + 1}#0'
        else:                                                 # the new launch: the step reads the shaped normals, the draw is untouched
            kinds.append('shaped')
            assert p['op'] == 'cell_project_noise' and p['shrink'] == shrink and p['noise']['t'] == f'noise{i + 1}#0'
            assert p['out_noise'] is None and step['noise']['t'] == p['->'][1]['t'] != p['noise']['t']
    assert not projections
    assert kinds == (['shaped', 'shaped', 'shaped', 'plain'] if sigma == SIGMA else ['constant'] * 3 + ['plain'])
    # everything that is not a projection or a step -- the U-Net's conversions, the final clamp -- is the constant-weight chain's
    rest = lambda t: [r['op'] for r in _launches(t) if r['op'] not in ('cell_project', 'cell_project_profile', 'cell_project_noise')]
    assert rest(got) == rest(plain)


@pytest.mark.parametrize('sigma', [SIGMA, 1e-12])
def test_edm_sample_dispatches_row_by_row(sigma, monkeypatch):
    from tests import test_edm_sampler_trace_host as T
    both = lambda a: (a['out'] if a['out'] is not None else torch.zeros_like(a['x0']),
                      a['out_noise'] if a['out_noise'] is not None else torch.zeros_like(a['noise']))
    for name, fn in _host({'cell_project_noise': both}).items():
        monkeypatch.setitem(T.RETURNS, name, fn)
    base = dict(model=dict(self_cond=True), sampler='dpmpp2m', eta=1.0, consistency=0.75)
    monkeypatch.setitem(T.CASES, 'noise-absent', T.sample_case(**base))
    monkeypatch.setitem(T.CASES, 'noise-none', T.sample_case(**base, consistency_noise=None))
    monkeypatch.setitem(T.CASES, 'noise-on', T.sample_case(**base, consistency_noise=sigma))
    absent, none, got = (T.run_case(n)[0] for n in ('noise-absent', 'noise-none', 'noise-on'))
    assert LT.canonical(absent) == LT.canonical(none)
    elu = HN.make_elucidated('churn-on', False, size=T.P)
    rows = elu._dpmpp2m_tables(1, None, 1.0, None, None)[1].numpy().astype(np.float64)
    assert float(elu.normalize_img(torch.tensor(1.0)) - elu.normalize_img(torch.tensor(0.0))) == 1.0     # sigma is in state units already
    want = _want_dispatch(rows, (2, 2, 4), None, sigma, 0.75)
    steps = [r for r in _launches(got) if r['op'] == 'multistep_sde_step']
    old = [r for r in _launches(absent) if r['op'] == 'multistep_sde_step']
    projections = [r for r in _launches(got) if r['op'] in ('cell_project', 'cell_project_noise')]
    assert len(steps) == len(want) == len(old) and sum(r['op'] == 'cell_project' for r in absent) == len(want)
    kinds = []
    for i, ((w, shrink), step, before) in enumerate(zip(want, steps, old)):
        if w == 0:
            kinds.append('plain')
            assert (step['noise'] is None) == (rows[i, 3] == 0)
            continue
        p = projections.pop(0)
        assert p['weight'] == w and p['clamp'] is None and p.get('table') is None
        if shrink == 0:
            kinds.append('constant')
            assert p['op'] == 'cell_project' and step['x0']['t'] == p['->']['t'] and step['noise'] == before['noise']
        else:
            kinds.append('shaped')
            assert p['op'] == 'cell_project_noise' and p['shrink'] == shrink
            assert p['noise'] == before['noise'] and p['out_noise'] is None                 # the draw the constant chain hands to its step
            assert step['x0']['t'] == p['->'][0]['t'] and step['noise']['t'] == p['->'][1]['t'] != p['noise']['t']
    assert not projections and kinds[-1] == 'plain' and rows[-1, 3] == 0
    assert set(kinds[:-1]) == ({'shaped'} if sigma == SIGMA else {'constant'})
    rest = lambda t: [r['op'] for r in _launches(t) if r['op'] not in ('cell_project', 'cell_project_noise')]
    assert rest(got) == rest(absent)


def _volume_case(monkeypatch, name, fn=None, **extra):
    """One ``VolumeInference`` case of the launch-trace module with consistency (and what ``extra`` adds) switched on."""
    from diffusioniqt_amd import ops
    from tests import test_volume_launch_trace_host as T
    monkeypatch.setitem(T.RETURNS, 'cell_replicate', lambda a: ops.cell_replicate(a['meas'], a['cell']))
    for op, f in _host({}).items():
        monkeypatch.setitem(T.RETURNS, op, f)
    for op in ('volume_joint_consistent_step', 'volume_joint_consistent_profile_step', 'volume_joint_consistent_noise_step'):
        monkeypatch.setitem(T.RETURNS, op, lambda a: (a['out'], a['x0_out']))
    monkeypatch.setattr(T.StubDenoiser, 'state_space', lambda self, x: self.rec.record('state_space', {'x': x}, 2 * x - 1), raising=False)
    case = dict(T.CASES[name])
    case['kw'] = dict(case['kw'], consistency=(torch.full((20, 18, 22), 300.0), (2, 2, 2)), consistency_weight=0.5, **extra)
    if fn is not None:
        case['fn'] = fn
    monkeypatch.setitem(T.CASES, 'noise-case', case)
    return T.run_case('noise-case'), case['cfg']


@pytest.mark.parametrize('chain', ['step', 'multistep', 'sigma-base1'])
def test_joint_chain_without_a_value_is_the_trace_with_the_keyword_absent(chain, monkeypatch):
    absent, _ = _volume_case(monkeypatch, f'joint-{chain}-selfcond')
    none, _ = _volume_case(monkeypatch, f'joint-{chain}-selfcond', consistency_noise=None)
    assert LT.canonical(absent) == LT.canonical(none) and not any(r['op'] == 'volume_joint_consistent_noise_step' for r in none)


@pytest.mark.parametrize('profile', [None, ((1, 2), (1, 1), (3, 0))])
@pytest.mark.parametrize('sigma_state', [0.01, 0.03, 1e-12])
@pytest.mark.parametrize('chain', ['step', 'sigma-base1'])
def test_joint_chain_dispatches_row_by_row(chain, sigma_state, profile, monkeypatch):
    """The stub denoisers' tables: three stochastic rows (first order) / an ODE row and two SDE rows (sigma space).  ``state_space`` is
    2 x - 1 here, so the raw sigma is divided by the z-score's std and doubled."""
    from tests import test_volume_launch_trace_host as T
    name = f'joint-{chain}-selfcond'
    extra = {} if profile is None else dict(consistency_profile=profile)
    plain, cfg = _volume_case(monkeypatch, name, **extra)
    raw = sigma_state * float(cfg['Data']['std']) / 2.0
    got, _ = _volume_case(monkeypatch, name, consistency_noise=raw, **extra)
    den = T.CASES[name]['fn'](LT.Recorder())
    rows = NR.rows4(den.coefs.numpy())
    table = None if profile is None else PR.profile_table((2, 2, 2), profile)
    sigma = raw / float(cfg['Data']['std']) * 2.0
    want = _want_dispatch(rows, (2, 2, 2), table, sigma, 0.5)
    form = 0 if chain == 'step' else 2
    plain_op = 'volume_joint_step' if chain == 'step' else 'volume_joint_multistep_sde'
    const_op = 'volume_joint_consistent_step' if profile is None else 'volume_joint_consistent_profile_step'
    fused = (plain_op, 'volume_joint_consistent_step', 'volume_joint_consistent_profile_step', 'volume_joint_consistent_noise_step')
    new = [r for r in _launches(got) if r['op'] in fused and r.get('x_t') is not None]
    old = [r for r in _launches(plain) if r['op'] in fused and r.get('x_t') is not None]
    S = 2
    assert len(new) == len(old) == S * 3 and all(r['op'] == const_op for r in old)
    kinds = set()
    for k, (n, o) in enumerate(zip(new, old)):
        w, shrink = want[k % 3]
        for key in ('y', 'x_t', 'out', 'x0_out', 'kx', 'k0', 'lo', 'hi', 'clamp_mode', 'stride'):   # the same buffers, coefficients and clamp
            assert n[key] == o[key] or (isinstance(n[key], dict) and n[key]['t'].split('#')[1] == o[key]['t'].split('#')[1]), key
        if form == 2 or w > 0:
            assert n['kn'] == o['kn']
        if w == 0:
            kinds.add('plain')
            assert n['op'] == plain_op and (n['kn'], n['draw'], n['sample']) == (o['kn'], o['draw'], o['sample'])
            continue
        assert n['weight'] == w and n['form'] == form and n['cell'] == [2, 2, 2] and n['meas_up']['t'] == o['meas_up']['t']
        assert (n['seed'], n['draw'], n['sample']) == (o['seed'], o['draw'], o['sample'])           # the draw numbers are unchanged
        if shrink == 0:
            kinds.add('constant')
            assert n['op'] == const_op
        else:
            kinds.add('shaped')
            assert n['op'] == 'volume_joint_consistent_noise_step' and n['shrink'] == shrink
            assert (n['table'] is None) == (profile is None)
    print(f"{chain} sigma {sigma_state}: dispatch {want} -> {sorted(kinds)}")
    if sigma_state == 1e-12:
        assert kinds == ({'constant'} if chain == 'step' else {'constant', 'plain'})
    else:
        assert 'shaped' in kinds
    rest = lambda t: [r['op'] for r in _launches(t) if r['op'] not in fused[1:] and not (r['op'] == plain_op and r.get('x_t') is not None)
                      and r['op'] != 'state_space']
    assert rest(got) == rest(plain)
    assert sum(r['op'] == 'state_space' for r in got) == sum(r['op'] == 'state_space' for r in plain) + 1   # the slope, on two host numbers


@pytest.mark.parametrize('sigma', [None, 50.0])
def test_blend_mode_hands_the_noise_on_exactly_when_one_was_given(sigma, monkeypatch):
    seen = []

    def sampler_of(rec):
        def sample(x, noise=None, **kw):
            seen.append(kw)
            return torch.zeros_like(x)
        return sample
    extra = {} if sigma is None else dict(consistency_noise=sigma)
    _, cfg = _volume_case(monkeypatch, 'blend-gaussian-s2-anchored', fn=sampler_of, **extra)
    assert seen
    for kw in seen:
        assert set(kw) == {'consistency', 'consistency_weight'} | set(extra)
        assert sigma is None or kw['consistency_noise'] == sigma / float(cfg['Data']['std'])   # z-scored like the measurement
