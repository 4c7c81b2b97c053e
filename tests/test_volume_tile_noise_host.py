"""Host-side checks of noise-aware data consistency for a tile operator (``consistency_row_noise=``; no GPU here):
``ops.tile_noise_operator`` / ``ops.tile_noise_schedule`` / ``ops.tile_noise_tables`` against
tests/volume_joint_tile_noise_reference.py, the variance identity, the fp32 restatement as exact rational arithmetic rounded once per
operation and within its derived counts of float64, every argument rule raised before anything touches the device, the error codes
of the two new entries, and -- with recording stand-ins -- the samplers and the joint chain: ``None`` is the trace with the keyword
absent, a value dispatches row by row.

Two comparisons take the singular values of ``ops`` where the restatement has its own: the recursion's
shrink = 1 - sqrt(1 - (a / b)^2) is evaluated AT a = b on every uncapped step, where one ulp of s moves it by 1.5e-8, so 1e-15 can
only be asked of the recursion given the same s; the singular values themselves are compared at 1e-12."""
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import launch_trace as LT
from tests import volume_blend_reference as R
from tests import volume_joint_heun_reference as HN
from tests import volume_joint_tile_noise_reference as TN
from tests import volume_joint_tile_reference as TR
from tests.test_volume_joint_host import _imagen
from tests.test_volume_noise_host import TABLES as ALL_TABLES, _NeverDenoiser

CASES = ['stacks-222', 'stacks-441', 'stacks-444', 'dense-232']
TABLES = {k: ALL_TABLES[k] for k in ('ddpm', 'ddim-0.5', 'edm-1.0')}
_CACHE = {}


def _op(name):
    """(cell, A, sigma, the operator of ``ops``, the restatement's whitening), made once per case."""
    if name not in _CACHE:
        from diffusioniqt_amd import ops
        cell, A, sigma = TN.case_of(name)
        _CACHE[name] = (cell, A, sigma, ops.tile_noise_operator(cell, A, sigma.tolist()), TN.whiten(A, sigma))
    return _CACHE[name]


def _as_whitening(op):
    """The operator of ``ops`` in the dict the restatement's functions take."""
    return dict(V=op.basis.numpy(), S=op.singular.numpy(), pinv=op.pinv.numpy(), sigma=op.row_noise.numpy(),
                sigma_min=float(op.row_noise.min()), omega=op.weights.numpy())


# ---- R1: the operator ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', CASES)
def test_noise_operator_is_the_restatement(name):
    from diffusioniqt_amd import ops
    cell, A, sigma, op, wh = _op(name)
    n, m = A.shape[1], A.shape[0]
    assert isinstance(op, ops.TileOperator) and (op.m, op.n, op.cell) == (m, n, cell) and np.array_equal(op.A.numpy(), A)
    assert op.rank == len(wh['S']) and tuple(op.singular.shape) == (op.rank,) and tuple(op.basis.shape) == (op.rank, n)
    assert all(t.dtype == torch.float64 for t in (op.singular, op.basis, op.weights, op.row_noise, op.pinv))
    assert np.array_equal(op.row_noise.numpy(), sigma) and np.array_equal(op.weights.numpy(), wh['omega'])
    assert 0 < op.weights.min() and op.weights.max() == 1.0 and len(set(sigma.tolist())) > 1
    assert np.abs(op.singular.numpy() - wh['S']).max() <= 1e-12 and np.abs(op.pinv.numpy() - wh['pinv']).max() <= 1e-12
    P = op.table.numpy()
    assert P.dtype == np.float32 and np.array_equal(P.view(np.uint32), P.T.copy().view(np.uint32))
    assert np.abs(P - wh['P']).max() <= 1e-7 and op.gain == TR.gain_of(P)
    plain = ops.tile_operator(cell, A)                                                     # the same row space: the same projector
    assert np.abs(P.astype(np.float64) - plain.table.numpy()).max() <= 2.0 ** -23 and plain.rank == op.rank
    # t = A_p y is the weighted least-squares solution: a y in the range of A comes back whatever the weights
    x = np.random.default_rng(1).standard_normal(n)
    assert np.abs(op.pinv.numpy() @ (A @ x) - wh['P'] @ x).max() <= 1e-12
    assert ops.tile_noise_operator(cell, op, sigma.tolist()).pinv.equal(op.pinv)            # an operator gives its matrix


@pytest.mark.parametrize('name', CASES)
def test_one_number_is_the_plain_operator(name):
    from diffusioniqt_amd import ops
    cell, A, _, _, _ = _op(name)
    plain, op = ops.tile_operator(cell, A), ops.tile_noise_operator(cell, A, 0.3)
    assert np.abs(op.pinv.numpy() - plain.pinv.numpy()).max() <= 1e-12 and torch.equal(op.table, plain.table)
    assert op.weights.tolist() == [1.0] * op.m and op.row_noise.tolist() == [0.3] * op.m and op.rank == plain.rank


BAD_VALUES = (True, False, 'high', None, float('nan'), float('inf'), 0, 0.0, -0.1, [0.2], [0.1] * 11, [0.1] * 11 + [0.0],
              [0.1] * 11 + [True], [0.1] * 11 + ['x'], [0.1] * 11 + [float('nan')])


def test_noise_operator_argument_errors():
    from diffusioniqt_amd import ops
    A = TR.stack_matrix((2, 2, 2), (0, 1, 2))
    for v in BAD_VALUES:
        with pytest.raises(ValueError, match="consistency_row_noise"):
            ops.tile_noise_operator((2, 2, 2), A, v)
    for cell, M in (((2, 2, 2), A[:, :7]), ((1, 1, 1), A), ((2, 2, 2), np.zeros((3, 8))), ((4, 1, 1), [[1., 3., 3., 1.]]),
                    ((2, 2, 2), 'matrix')):                                                # whatever tile_operator refuses
        with pytest.raises(ValueError, match="consistency_row_noise") as err:
            ops.tile_noise_operator(cell, M, 0.1)
        assert 'consistency' in str(err.value)
    op = ops.tile_noise_operator((2, 2, 2), A, 0.1)
    for bad in (ops.tile_operator((2, 2, 2), A), A, None):
        with pytest.raises(ValueError, match="consistency_row_noise"):
            ops.tile_noise_schedule(bad, TABLES['ddpm'], 0.1, 1.0)
        with pytest.raises(ValueError, match="consistency_row_noise"):
            ops.tile_noise_tables(bad, torch.zeros(4, 7, 2, dtype=torch.float64))
    with pytest.raises(ValueError, match="consistency_row_noise"):
        ops.tile_noise_tables(op, torch.zeros(4, 8, 2, dtype=torch.float64))                 # rank is 7


# ---- R2: the schedule and the tables ------------------------------------------------------------------------------------------------------
def _close(a, b, rel):
    return bool((np.abs(a - b) <= rel * np.maximum(np.abs(a), np.abs(b))).all())


@pytest.mark.parametrize('w', [1.0, 0.5])
@pytest.mark.parametrize('table', list(TABLES))
@pytest.mark.parametrize('name', CASES)
def test_schedule_and_tables_are_the_restatement(name, table, w):
    from diffusioniqt_amd import ops
    cell, A, sigma, op, wh = _op(name)
    rows = TABLES[table]
    sched = ops.tile_noise_schedule(op, rows, float(sigma.min()), w)
    assert sched.dtype == torch.float64 and tuple(sched.shape) == (len(rows), op.rank, 2)
    want = TN.schedule64(rows, op.singular.numpy(), wh['sigma_min'], w)                      # the module docstring: the same s
    assert _close(sched.numpy(), want, 1e-15)
    for j, s in enumerate(op.singular.tolist()):                                           # per direction it IS the scalar schedule
        assert torch.equal(sched[:, j], ops.consistency_noise_schedule(rows, s, float(sigma.min()), w))
    assert (sched.numpy()[rows[:, 3] == 0] == 0).all() and sched[:, :, 0].max() <= w and (sched[:-1, :, 0] > 0).all()
    tables, kinds = ops.tile_noise_tables(op, sched)
    n = op.n
    assert tables.dtype == torch.float32 and tuple(tables.shape) == (len(rows), 2, n, n) and tables.is_contiguous()
    T = tables.numpy()
    assert np.array_equal(T.view(np.uint32), T.transpose(0, 1, 3, 2).copy().view(np.uint32))   # symmetric to the bit
    # The restatement forms the tables from (s, V) in its own way.  M with the restatement's OWN SVD: lambda is continuous in s, so
    # the basis inside a repeated singular value does not matter.  G is another matter (module docstring): inside a repeated
    # singular value the s_j differ in their last bits, on an uncapped step the shrink_j then differ by up to sqrt(2 delta), and
    # G = sum_j shrink_j v_j v_j^T depends on the basis by that much.  So G is compared at 1e-12 given the decomposition of
    # ``ops``, and with the restatement's own SVD within 2 sqrt(2 delta) + one fp32 rounding, delta = 1e-12 the tolerance on s above.
    own = TN.tables64(wh['V'], TN.schedule64(rows, wh['S'], wh['sigma_min'], w)).astype(np.float32)
    same = TN.tables64(op.basis.numpy(), want).astype(np.float32)
    err_m, err_g, own_g = np.abs(T[:, 0] - own[:, 0]).max(), np.abs(T[:, 1] - same[:, 1]).max(), np.abs(T[:, 1] - own[:, 1]).max()
    print(f"{name} {table} w {w}: M - restatement (own SVD) = {err_m:.3e}; G - restatement = {err_g:.3e} (own SVD: {own_g:.3e}); "
          f"kinds {[k for k, _ in kinds]}")
    assert err_m <= 1e-12 and err_g <= 1e-12 and np.abs(T[:, 0] - same[:, 0]).max() <= 1e-12
    assert own_g <= 2 * np.sqrt(2e-12) + 2.0 ** -24 * np.abs(T).max()
    assert kinds == TN.kinds(sched.numpy()) and kinds[-1] == ('plain', 0.0) and all(k == 'noise' for k, _ in kinds[:-1])
    # the tables act as V diag(.) V^T: M v_j = lambda_j v_j, G v_j = shrink_j v_j, the null space goes to zero
    V = op.basis.numpy()
    for i in range(len(rows)):
        for c in (0, 1):
            assert np.abs(T[i, c].astype(np.float64) @ V.T - V.T * sched[i, :, c].numpy()).max() <= n * 2.0 ** -23
    null = np.eye(n) - wh['P']
    assert np.abs(T.astype(np.float64) @ null).max() <= n * 2.0 ** -23


def test_one_row_over_four_voxels_is_the_scalar_schedule():
    from diffusioniqt_amd import ops
    op = ops.tile_noise_operator((4, 1, 1), [[0.25] * 4], 0.2)
    assert op.rank == 1 and abs(float(op.singular[0]) - ops.cell_norm((4, 1, 1))) <= 1e-15
    for name, rows in TABLES.items():
        for w in (1.0, 0.5):
            got = ops.tile_noise_schedule(op, rows, 0.2, w)[:, 0]
            want = ops.consistency_noise_schedule(rows, float(op.singular[0]), 0.2, w)
            assert torch.equal(got, want), name
            # and against s = |u| = 1 / 2 itself the weights agree to rounding (the shrink only where it is well conditioned)
            exact = ops.consistency_noise_schedule(rows, ops.cell_norm((4, 1, 1)), 0.2, w)
            assert _close(got[:, 0].numpy(), exact[:, 0].numpy(), 1e-15)


def test_all_three_dispatch_kinds_occur():
    from diffusioniqt_amd import ops
    cell, A, sigma, op, _ = _op('stacks-222')
    seen = set()
    for s_min in (float(sigma.min()), 1e-12):
        quiet = ops.tile_noise_operator(cell, A, (sigma * s_min / sigma.min()).tolist())
        for rows in TABLES.values():
            _, kinds = ops.tile_noise_tables(quiet, ops.tile_noise_schedule(quiet, rows, s_min, 0.75))
            seen |= {k for k, _ in kinds}
            assert all(w == 0.75 for k, w in kinds if k == 'tile') and all(w == 0.0 for k, w in kinds if k != 'tile')
    assert seen == {'plain', 'tile', 'noise'}


# ---- R3: the statistics ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('w', [1.0, 0.5])
@pytest.mark.parametrize('table', list(TABLES))
@pytest.mark.parametrize('name', CASES + ['scalar-222'])
def test_variance_identity(name, table, w):
    """B_i Cov(t) B_i^T + kn^2 (I - G_i)(I - G_i)^T = kn^2 I on every scheduled row where no direction was clipped at 0 with
    |a| > b, with the operator and the schedule of ``ops`` and the tables formed in float64."""
    from diffusioniqt_amd import ops
    if name == 'scalar-222':
        cell, A, _, _, _ = _op('stacks-222')
        op = ops.tile_noise_operator(cell, A, 0.2)
    else:
        op = _op(name)[3]
    rows = TABLES[table]
    sched = ops.tile_noise_schedule(op, rows, float(op.row_noise.min()), w).numpy()
    out = TN.variance_defect(_as_whitening(op), sched, rows)
    qualifying = [(d, kn) for d, kn, ok in out if ok]
    worst = max(d / kn ** 2 for d, kn in qualifying)
    print(f"{name} {table} w {w}: {len(qualifying)} of {len(rows)} rows qualify, worst defect / kn^2 = {worst:.3e}; "
          f"lambda range {sched[:-1, :, 0].min():.3g} .. {sched[:-1, :, 0].max():.3g}")
    assert len(qualifying) >= len(rows) - 2 and worst <= 1e-10
    if name != 'scalar-222':                                                               # no scalar expresses one step
        assert max(sched[i, :, 1].max() / sched[i, :, 1].min() for i in range(len(rows) - 1)) > 2


@pytest.mark.parametrize('name', CASES)
def test_shaped_normals_keep_one_minus_shrink_of_every_direction(name):
    """v_j . eps' = (1 - shrink_j) v_j . eps on the fp32 restatement: within |v_j|_1 times (the shaping's count + the rounding of the
    table, u G_G E); a null-space direction keeps its component within the same."""
    from diffusioniqt_amd import ops
    cell, A, sigma, op, wh = _op(name)
    sched = ops.tile_noise_schedule(op, TABLES['ddim-0.5'], float(sigma.min()), 1.0)
    tables, _ = ops.tile_noise_tables(op, sched)
    step = 1
    T, shrink, V, n = tables[step].numpy(), sched[step, :, 1].numpy(), op.basis.numpy(), op.n
    assert 0 < shrink.min() and shrink.max() <= 1
    count = 5
    eps = np.random.default_rng(2).standard_normal((cell[0], cell[1], cell[2] * count)).astype(np.float32)
    _, got = TN.project_noise32(np.zeros_like(eps), np.zeros_like(eps), eps, cell, T)
    e, g = TR.tiles(eps, cell)[0, 0].astype(np.float64), TR.tiles(got, cell)[0, 0].astype(np.float64)      # [count, n]
    E = float(np.abs(eps).max())
    slack = TN.shaping_roundings(cell, T, E) + 2.0 ** -24 * TN.gain_of(T[1]) * E
    err = np.abs(g @ V.T - (1 - shrink) * (e @ V.T))
    assert (err <= np.abs(V).sum(1) * slack).all()
    null = np.linalg.svd(np.eye(n) - wh['P'])[0][:, :n - op.rank].T                          # an orthonormal basis of the null space
    assert (np.abs(g @ null.T - e @ null.T) <= np.abs(null).sum(1) * slack).all()
    print(f"{name}: largest |v . eps' - (1 - shrink) v . eps| = {err.max():.3e}, slack {slack:.3e} |v|_1")


# ---- R4: the fp32 restatement ---------------------------------------------------------------------------------------------------------------
def _rn32(x):
    """A Fraction rounded to the nearest float32, ties to even."""
    near = np.float32(float(x))
    cands = (np.nextafter(near, np.float32(-np.inf)), near, np.nextafter(near, np.float32(np.inf)))
    return min(cands, key=lambda v: (abs(Fraction(float(v)) - x), int(v.view(np.uint32)) & 1))


@pytest.mark.parametrize('name', CASES + ['stack-411', 'stacks-135'])
def test_project_noise32_is_exact_arithmetic_rounded_once_per_operation(name):
    """d = rn(t - a); s = rn(M[r][q] d[r] + s) in the order of r; a' = rn(a + s); g = rn(G[r][q] eps[r] + g); eps' = rn(eps - g) --
    every rn ONE rounding of the exact rational value.  And both results lie within the derived counts of float64."""
    from diffusioniqt_amd import ops
    cell, A, sigma = TN.case_of(name)
    op = ops.tile_noise_operator(cell, A, sigma.tolist())
    sched = ops.tile_noise_schedule(op, TABLES['ddpm'], float(sigma.min()), 1.0)
    T = ops.tile_noise_tables(op, sched)[0][1].numpy()
    n = op.n
    rng = np.random.default_rng(len(name))
    count = 6 if n < 64 else 2
    shape = (cell[0], cell[1], cell[2] * count)
    a = (rng.standard_normal(shape) * 2).astype(np.float32)
    t = rng.standard_normal(shape).astype(np.float32)
    eps = rng.standard_normal(shape).astype(np.float32)
    got, shaped = TN.project_noise32(a, t, eps, cell, T)
    F = lambda v: Fraction(float(v))
    for c in range(count):
        sl = np.s_[:, :, c * cell[2]:(c + 1) * cell[2]]
        av, tv, ev, have, have_e = (v[sl].reshape(-1) for v in (a, t, eps, got, shaped))       # lexicographic (z, y, x)
        d = [_rn32(F(tv[r]) - F(av[r])) for r in range(n)]
        for q in range(n if n < 64 else 5):
            s, g = np.float32(0), np.float32(0)
            for r in range(n):
                s = _rn32(F(T[0, r, q]) * F(d[r]) + F(s))
                g = _rn32(F(T[1, r, q]) * F(ev[r]) + F(g))
            assert have[q].view(np.uint32) == _rn32(F(av[q]) + F(s)).view(np.uint32), (c, q)
            assert have_e[q].view(np.uint32) == _rn32(F(ev[q]) - F(g)).view(np.uint32), (c, q)
    ones = np.ones(shape, dtype=bool)
    ref, ref_e = TN.project_noise64(a.astype(np.float64), ones, t.astype(np.float64), eps.astype(np.float64), cell, T)
    scale = max(float(np.abs(a).max()), float(np.abs(t).max()), float(np.abs(got).max()))
    bound, bound_e = TN.projection_roundings(cell, T, scale), TN.shaping_roundings(cell, T, float(np.abs(eps).max()))
    err, err_e = np.abs(got - ref).max(), np.abs(shaped - ref_e).max()
    print(f"tile noise {name}: x0 fp32 - float64 = {err:.3e}, count {bound:.3e} ({err / bound:.3f}); normals {err_e:.3e}, count "
          f"{bound_e:.3e} ({err_e / bound_e:.3f}); gains {TN.gain_of(T[0]):.3f} / {TN.gain_of(T[1]):.3f}")
    assert err <= bound and err_e <= bound_e and (got != a).mean() > 0.9 and (shaped != eps).mean() > 0.9
    part = np.zeros(shape, dtype=bool)
    part[:, :, :cell[2]] = True                                                            # only the first tile is covered
    p, pe = TN.project_noise32(a, t, eps, cell, T, part)
    assert np.array_equal(p[part], got[part]) and np.array_equal(p[~part], a[~part]) and np.array_equal(pe[~part], eps[~part])


# ---- R5: refusals, all before the device is touched -----------------------------------------------------------------------------------------
A222 = TR.stack_matrix((2, 2, 2), (0, 1, 2))
SIG222 = TN.stack_sigma((2, 2, 2), (0, 1, 2), (0.05, 0.2, 0.1)).tolist()


def _meas(P=16, B=2):
    return torch.zeros(B, 1, P, P, P)


def test_sample_refuses_row_noise_it_cannot_honour():
    imagen = _imagen()
    lr = torch.zeros(2, 1, 16, 16, 16)
    base = dict(batch_size=2, start_image_or_video=lr, start_at_unet_number=2, use_tqdm=False, sampler='ddim', sample_steps=2, eta=0.5)
    ok = dict(consistency=(_meas(), (2, 2, 2)), consistency_operator=A222)
    bad = [dict(consistency_row_noise=0.2), dict(consistency=ok['consistency'], consistency_row_noise=0.2)]     # without the operator
    bad += [dict(**ok, consistency_row_noise=v) for v in BAD_VALUES if v is not None]
    bad += [dict(**ok, consistency_row_noise=0.2, consistency_noise=0.2),
            dict(**ok, consistency_row_noise=0.2, consistency_profile=((1, 2), (1, 1), (1, 1))),
            dict(**ok, consistency_row_noise=0.2, eta=0.0),                                 # no stochastic row
            dict(**ok, consistency_row_noise=0.2, sampler='dpmpp2m', eta=0.0),
            dict(**ok, consistency_row_noise=0.2, init_images=lr),                          # what consistency already refuses
            dict(**ok, consistency_row_noise=0.2, sampler='ddpm', eta=0.0, inpaint_images=lr, inpaint_masks=lr[:, 0].bool()),
            dict(**ok, consistency_row_noise=0.2, consistency_weight=0.0),
            dict(consistency=(_meas(), (2, 2, 2)), consistency_operator=A222[:, :7], consistency_row_noise=0.2),
            dict(consistency=(_meas(), (3, 1, 1)), consistency_operator=[[1 / 3] * 3], consistency_row_noise=0.2)]
    for kw in bad:
        with pytest.raises(ValueError, match="consistency_row_noise"):
            imagen.sample(**{**base, **kw})
    with pytest.raises(ValueError, match="consistency_weight"):                            # the deterministic refusal says what to use
        imagen.sample(**{**base, **ok, 'consistency_row_noise': 0.2, 'eta': 0.0})
    with pytest.raises(ValueError, match="init_images"):                                   # in its existing wording
        imagen.sample(**{**base, **ok, 'consistency_row_noise': 0.2, 'init_images': lr})
    with pytest.raises(ValueError, match="consistency_operator") as pinned:                # the scalar model stays refused, and points here
        imagen.sample(**{**base, **ok, 'consistency_noise': 0.2})
    assert 'consistency_row_noise' in str(pinned.value)
    loop = dict(noise_scheduler=imagen.noise_schedulers[1], pred_objective='x_start', sampler='ddim', sample_steps=2)
    for kw in (dict(consistency_row_noise=0.2, eta=0.5), dict(**ok, consistency_row_noise=0.0, eta=0.5),
               dict(**ok, consistency_row_noise=SIG222[:-1], eta=0.5), dict(**ok, consistency_row_noise=SIG222, eta=0.0)):
        with pytest.raises(ValueError, match="consistency_row_noise"):                     # the loop itself applies the same rules
            imagen.p_sample_loop(imagen.unets[1], (2, 1, 16, 16, 16), **loop, **kw)


def test_edm_sample_refuses_row_noise_it_cannot_honour():
    elu = HN.make_elucidated('churn-on', False)
    lr = torch.zeros(2, 1, 16, 16, 16)
    base = dict(batch_size=2, video_frames=16, start_image_or_video=lr, start_at_unet_number=2, use_tqdm=False, sampler='dpmpp2m', eta=1.0)
    ok = dict(consistency=(_meas(), (2, 2, 2)), consistency_operator=A222)
    bad = [dict(consistency_row_noise=0.2), dict(consistency=ok['consistency'], consistency_row_noise=SIG222)]
    bad += [dict(**ok, consistency_row_noise=v) for v in BAD_VALUES if v is not None]
    bad += [dict(**ok, consistency_row_noise=0.2, consistency_noise=0.2),
            dict(**ok, consistency_row_noise=0.2, consistency_profile=((1, 2), (1, 1), (1, 1))),
            dict(**ok, consistency_row_noise=0.2, eta=0.0),                                 # the ODE solver: no stochastic row
            dict(**ok, consistency_row_noise=0.2, sampler='heun', eta=0.0),
            dict(**ok, consistency_row_noise=0.2, init_images=lr),
            dict(**ok, consistency_row_noise=0.2, consistency_weight=2),
            dict(consistency=(_meas(P=8), (2, 2, 2)), consistency_operator=A222, consistency_row_noise=0.2)]
    for kw in bad:
        with pytest.raises(ValueError, match="consistency_row_noise"):
            elu.sample(**{**base, **kw})
    with pytest.raises(ValueError, match="consistency_weight"):
        elu.sample(**{**base, **ok, 'consistency_row_noise': 0.2, 'eta': 0.0})
    for kw in (dict(consistency_row_noise=0.2, eta=1.0), dict(**ok, consistency_row_noise=-1.0, eta=1.0),
               dict(**ok, consistency_row_noise=SIG222, eta=0.0)):
        with pytest.raises(ValueError, match="consistency_row_noise"):
            elu.one_unet_sample(elu.unets[1], (2, 1, 16, 16, 16), unet_number=2, sampler='dpmpp2m', **kw)


def test_volume_inference_row_noise_argument_errors():
    from diffusioniqt_amd import ops
    from diffusioniqt_amd.inference import VolumeInference

    def never(x, **kw):
        raise AssertionError("the sampler must not run")
    cfg = R.shared_cfg(8)
    y = torch.zeros(12, 20, 18, 22)
    ok = dict(consistency=(y, (2, 2, 2)), consistency_operator=A222)
    joint = dict(blend='gaussian', noise='anchored', joint=True)
    for kw in (dict(consistency_row_noise=40.0), dict(consistency=(y[0], (2, 2, 2)), consistency_row_noise=40.0),
               dict(**ok, consistency_row_noise=40.0, consistency_noise=40.0),
               dict(consistency=(y[0], (2, 2, 2)), consistency_row_noise=40.0, consistency_profile=((1, 2), (1, 1), (1, 1)))):
        with pytest.raises(ValueError, match="consistency_row_noise"):
            VolumeInference(cfg, never, **kw)
    for v in BAD_VALUES:
        if v is not None:
            with pytest.raises(ValueError, match="consistency_row_noise"):
                VolumeInference(cfg, never, **ok, consistency_row_noise=v)
    noisy = [[0.5, 0.25, 0.125]] * 3
    for den in (_NeverDenoiser([[0.5, 0.25, 0.0]] * 3), _NeverDenoiser(noisy, multistep=True),
                _NeverDenoiser([[0.5, 0.25, -0.1, 0.0]] * 3, multistep=True, sigma0=1.5, draw_base=1)):
        with pytest.raises(ValueError, match="consistency_weight"):
            VolumeInference(cfg, den, **ok, consistency_row_noise=40.0, **joint)
        with pytest.raises(ValueError, match="consistency_row_noise"):
            VolumeInference(cfg, den, **ok, consistency_row_noise=40.0, **joint)
    known = (torch.zeros(40, 36, 44), torch.zeros(40, 36, 44, dtype=torch.bool))
    for kw in (dict(**ok, inpaint=known), dict(**ok, consistency_weight=0.0), dict(consistency=(y[:5], (2, 2, 2)), consistency_operator=A222),
               dict(consistency=(y, (2, 2, 2)), consistency_operator=A222[:, :7]), dict(consistency=(y.long(), (2, 2, 2)),
                                                                                      consistency_operator=A222)):
        with pytest.raises(ValueError, match="consistency_row_noise"):                     # what consistency and the operator refuse
            VolumeInference(cfg, never, consistency_row_noise=40.0, **kw)
    with pytest.raises(ValueError, match="consistency_row_noise"):                         # the Heun denoiser stays refused
        VolumeInference(cfg, HN.make_elucidated('churn-on', False).window_denoiser(), **ok, consistency_row_noise=40.0, **joint)
    with pytest.raises(ValueError, match="consistency_row_noise"):                         # in __call__: not the volume's shape
        VolumeInference(cfg, never, **ok, consistency_row_noise=40.0)(torch.zeros(40, 36, 48))
    with pytest.raises(ValueError, match="consistency_operator") as pinned:
        VolumeInference(cfg, never, **ok, consistency_noise=40.0)
    assert 'consistency_row_noise' in str(pinned.value)
    # the LDS plan: n = 64 with a box of 2048 voxels or more is refused for the fused launch, here (8, 8, 1): 4 x 4096 + 2 x 4096 floats
    wide = dict(consistency=(torch.zeros(64, 5, 4, 44), (8, 8, 1)), consistency_operator=np.eye(64))
    with pytest.raises(ValueError, match="consistency_row_noise.*LDS"):
        VolumeInference(R.shared_cfg(8), _NeverDenoiser(noisy), **wide, consistency_row_noise=40.0, **joint)
    assert VolumeInference(R.shared_cfg(8), _NeverDenoiser(noisy), **wide, **joint).consistency_op.n == 64      # without it: as before
    assert ops.tile_noise_lds((4, 4, 4), 4096) == 4 * (4096 + 4 * 1024 + 2 * 4096) <= 65536                    # 16 KiB + 16 KiB + 32 KiB
    refused = [c for c in ((64, 1, 1), (1, 64, 1), (1, 1, 64), (8, 8, 1), (1, 8, 8), (8, 1, 8), (32, 2, 1), (2, 32, 1), (16, 4, 1),
                           (4, 16, 1), (4, 4, 4), (2, 2, 16), (2, 4, 8), (16, 2, 2)) if ops.tile_noise_lds(c, 16) > 65536]
    assert (4, 4, 4) not in refused and (64, 1, 1) in refused and (8, 8, 1) in refused
    for c in refused:                                                                       # n = 64 and boxes of 2048 voxels or more
        by, bx = c[1] * -(-4 // (c[0] * c[1])), c[2] * -(-64 // c[2])
        assert c[0] * by * bx >= 2048
    inf = VolumeInference(cfg, _NeverDenoiser(noisy), **ok, consistency_row_noise=SIG222, **joint)
    assert isinstance(inf.consistency_op, ops.TileNoiseOperator) and inf.consistency_row_noise == SIG222
    assert VolumeInference(cfg, never, **ok).consistency_row_noise is None                 # the default is today's path


def test_ops_refuse_bad_steps_before_the_library():
    from diffusioniqt_amd import ops
    x = torch.zeros(2, 1, 8, 8, 8)
    tabs = torch.zeros(2, 8, 8)
    with pytest.raises(ValueError, match="consistency_row_noise"):
        ops.tile_project_noise(x, x.clone(), x.clone(), (2, 2, 2), tabs[0])
    with pytest.raises(ValueError, match="consistency_row_noise"):
        ops.tile_project_noise(x, x.clone(), x.clone(), (4, 1, 1), tabs)
    with pytest.raises(ValueError, match="consistency cell"):
        ops.tile_project_noise(x, x.clone(), x.clone(), (1, 1, 1), tabs)
    vol = torch.zeros(8, 8, 8)
    for form, kn in ((1, 0.5), (0, 0.0), (3, 0.5)):
        with pytest.raises(ValueError, match="volume_joint_consistent_tile_noise_step"):
            ops.volume_joint_consistent_tile_noise_step(None, None, None, vol, None, vol, (2, 2, 2), tabs, form, 1.0, 0.5, 0.0, kn, -1.0,
                                                        1.0, 1, 4)


def test_tile_noise_entries_return_error_codes():
    from diffusioniqt_amd import _lib
    lib = _lib.load()
    buf = (np.zeros(4, dtype=np.int32)).ctypes.data                             # never dereferenced: every call below is refused

    def proj(ptrs=(buf,) * 6, cubes=3, P=8, cell=(2, 2, 2), mode=2):
        return lib.diqt_tile_project_noise(*ptrs, cubes, P, *cell, -1.0, 1.0, mode, None)
    for k in range(6):
        assert proj(tuple(None if i == k else buf for i in range(6))) == -2, k
    assert b"null pointer" in lib.diqt_last_error()
    assert proj(cell=(1, 1, 1)) == -3 and proj(cell=(8, 8, 2)) == -3 and proj(mode=3) == -3 and proj(mode=-1) == -3
    assert proj(cell=(1, 1, 3)) == -1 and proj(cubes=0) == -1
    # three box arrays of 64 x 1 x 64 voxels and two 64 x 64 tables: 80 KiB
    assert proj(P=64, cell=(64, 1, 1)) == -1 and b"LDS" in lib.diqt_last_error()
    geo = (40, 36, 44, 16, 8, 4, 3, 4)                                          # D, H, W, P, stride and the lattice of range(0, n - 15, 8)

    def step(ptrs=(buf,) * 9, form=0, geo=geo, cell=(2, 2, 2), kn=0.25, mode=0):
        return lib.diqt_volume_joint_consistent_tile_noise_step(*ptrs, form, 3, *geo, *cell, 1.0, 0.5, 0.0, kn, -1.0, 1.0, mode, 0, 1, 0,
                                                                None)
    assert step(form=1) == -3 and b"form" in lib.diqt_last_error()
    assert step(form=3) == -3 and step(form=-1) == -3
    assert step(kn=0.0) == -3 and step(form=2, kn=0.0) == -3 and b"kn" in lib.diqt_last_error()
    assert step(cell=(1, 1, 1)) == -3 and step(cell=(4, 4, 8)) == -3 and step(mode=2) == -3
    for k in (0, 1, 2, 3, 5, 6, 7, 8):                                          # x0_prev alone may be NULL
        assert step(tuple(None if i == k else buf for i in range(9))) == -2, k
    assert step(cell=(3, 1, 1)) == -1 and step(geo=(40, 36, 44, 16, 8, 4, 3, 5)) == -1
    # n = 64 with a box of 4096 voxels: four box arrays are 64 KiB on their own
    assert step(geo=(64, 40, 64, 16, 8, 7, 4, 7), cell=(8, 8, 1)) == -1 and b"LDS" in lib.diqt_last_error()
    assert step(geo=(64, 40, 64, 16, 8, 7, 4, 7), cell=(4, 4, 4), ptrs=(None,) + (buf,) * 8) == -2              # (4, 4, 4) plans 48 KiB


# ---- R6: the dispatch, with recording stand-ins ---------------------------------------------------------------------------------------------
HOST_ONLY = ('consistency_cell', 'tile_operator', 'tile_noise_operator', 'tile_noise_plan', 'tile_noise_schedule', 'tile_noise_tables')
NEW = ('tile_noise_operator', 'tile_noise_plan', 'tile_noise_schedule', 'tile_noise_tables', 'tile_project_noise',
       'volume_joint_consistent_tile_noise_step')
A224 = TR.stack_matrix((2, 2, 4), (0, 2))
SIG224 = TN.stack_sigma((2, 2, 4), (0, 2), (0.2, 0.6)).tolist()


def _host(returns):
    from diffusioniqt_amd import ops
    for name in HOST_ONLY:
        returns[name] = (lambda f: lambda a: f(**a))(getattr(ops, name))                    # host only: the real rules
    return returns


def _launches(trace):
    return [r for r in trace if r['op'] not in HOST_ONLY]


def _both(a):
    return (a['out'] if a['out'] is not None else torch.zeros_like(a['x0']),
            a['out_noise'] if a['out_noise'] is not None else torch.zeros_like(a['noise']))


def _want_kinds(A, sigma, rows, cap, scale=1.0):
    wh = TN.whiten(A, sigma)
    return TN.kinds(TN.schedule64(rows, wh['S'], wh['sigma_min'] * scale, cap))


def _imagen_trace(sampler, eta, **extra):
    from diffusioniqt_amd import imagen_pytorch3D
    into = lambda key: (lambda a: a['out'] if a.get('out') is not None else torch.zeros_like(a[key]))
    returns = _host({'axpby3': lambda a: torch.zeros_like(a['a']), 'ddpm_step': lambda a: (torch.zeros_like(a['x_t']), torch.zeros_like(a['x_t'])),
                     'tile_project': into('x0'), 'tile_project_noise': _both})
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
                            sample_steps=4, eta=eta, noise=noise, consistency=(meas, (2, 2, 4)), consistency_weight=0.75,
                            consistency_operator=A224, **extra)[0]
    rec.record('return', {}, out)
    return rec.trace, imagen


@pytest.mark.parametrize('sampler,eta', [('ddpm', 0.0), ('ddim', 0.5), ('ddim', 0.0), ('dpmpp2m', 0.0)])
def test_imagen_sample_without_a_value_is_the_trace_with_the_keyword_absent(sampler, eta):
    absent, _ = _imagen_trace(sampler, eta)
    none, _ = _imagen_trace(sampler, eta, consistency_row_noise=None)
    assert LT.canonical(absent) == LT.canonical(none) and not any(r['op'] in NEW for r in none)


@pytest.mark.parametrize('sigma', [SIG224, 1e-12])
@pytest.mark.parametrize('sampler,eta', [('ddpm', 0.0), ('ddim', 0.5)])
def test_imagen_sample_dispatches_row_by_row(sampler, eta, sigma):
    from diffusioniqt_amd.imagen_pytorch3D import Imagen
    plain, imagen = _imagen_trace(sampler, eta)
    got, _ = _imagen_trace(sampler, eta, consistency_row_noise=sigma)
    coefs = Imagen._sampler_tables(imagen.noise_schedulers[1], 2, sampler, 4, None, eta, 'x_start')[0][:, :, 0].numpy()
    want = _want_kinds(A224, sigma, TN.rows4(coefs), 0.75)
    lo, hi, mode = imagen._clamp_cfg()
    steps = [r for r in _launches(got) if r['op'] == 'ddpm_step']
    projections = [r for r in _launches(got) if r['op'] in ('tile_project', 'tile_project_noise')]
    assert len(steps) == 4 and sum(r['op'] == 'tile_project' for r in plain) == 4
    tables = set()
    for i, (kind, w) in enumerate(want):
        step = steps[i]
        if kind == 'plain':                                   # the plain step with the chain's own clamp, no projection launch
            assert (step['lo'], step['hi'], step['clamp_mode']) == (LT.f32(lo), LT.f32(hi), mode)
            assert step['noise']['t'] == f'noise{i + 1}#0'
            continue
        p = projections.pop(0)
        assert (step['lo'], step['hi'], step['clamp_mode']) == ('-inf', 'inf', 1)           # a projected step clamps no more
        assert p['clamp'] == [LT.f32(lo), LT.f32(hi), mode] and p['cell'] == [2, 2, 4] and p['target']['t'] == 'meas_up#0'
        if kind == 'tile':                                    # the existing tile launch with that weight
            assert p['op'] == 'tile_project' and p['weight'] == LT.f32(w) and p['table']['shape'] == [16, 16]
            assert step['pred']['t'] == p['->']['t'] and step['noise']['t'] == f'noise{i + 1}#0'
        else:                                                 # the new launch: the step reads the shaped normals, the draw is untouched
            assert p['op'] == 'tile_project_noise' and p['noise']['t'] == f'noise{i + 1}#0' and p['out_noise'] is None
            assert p['tables_i']['shape'] == [2, 16, 16] and p['tables_i']['off'] == i * 2 * 16 * 16   # step i of the ONE upload
            tables.add(p['tables_i']['t'])
            assert step['pred']['t'] == p['->'][0]['t'] and step['noise']['t'] == p['->'][1]['t'] != p['noise']['t']
    assert not projections and len(tables) <= 1
    assert [k for k, _ in want] == (['noise'] * 3 + ['plain'] if sigma is SIG224 else ['tile'] * 3 + ['plain'])
    rest = lambda t: [r['op'] for r in _launches(t) if r['op'] not in ('tile_project', 'tile_project_noise')]
    assert rest(got) == rest(plain)


@pytest.mark.parametrize('sigma', [SIG224, 1e-12])
def test_edm_sample_dispatches_row_by_row(sigma, monkeypatch):
    from tests import test_edm_sampler_trace_host as T
    for name, fn in _host({'tile_project_noise': _both, 'tile_project': T._into('x0')}).items():
        monkeypatch.setitem(T.RETURNS, name, fn)
    base = dict(model=dict(self_cond=True), sampler='dpmpp2m', eta=1.0, consistency=0.75, consistency_operator=A224)
    monkeypatch.setitem(T.CASES, 'row-absent', T.sample_case(**base))
    monkeypatch.setitem(T.CASES, 'row-none', T.sample_case(**base, consistency_row_noise=None))
    monkeypatch.setitem(T.CASES, 'row-on', T.sample_case(**base, consistency_row_noise=sigma))
    absent, none, got = (T.run_case(n)[0] for n in ('row-absent', 'row-none', 'row-on'))
    assert LT.canonical(absent) == LT.canonical(none) and not any(r['op'] in NEW for r in none)
    elu = HN.make_elucidated('churn-on', False, size=T.P)
    rows = elu._dpmpp2m_tables(1, None, 1.0, None, None)[1].numpy().astype(np.float64)
    assert float(elu.normalize_img(torch.tensor(1.0)) - elu.normalize_img(torch.tensor(0.0))) == 1.0     # sigma is in state units already
    want = _want_kinds(A224, sigma, rows, 0.75)
    steps = [r for r in _launches(got) if r['op'] == 'multistep_sde_step']
    old = [r for r in _launches(absent) if r['op'] == 'multistep_sde_step']
    projections = [r for r in _launches(got) if r['op'] in ('tile_project', 'tile_project_noise')]
    assert len(steps) == len(want) == len(old) and sum(r['op'] == 'tile_project' for r in absent) == len(want)
    for i, ((kind, w), step, before) in enumerate(zip(want, steps, old)):
        if kind == 'plain':
            assert (step['noise'] is None) == (rows[i, 3] == 0)
            continue
        p = projections.pop(0)
        assert p['clamp'] is None
        if kind == 'tile':
            assert p['op'] == 'tile_project' and p['weight'] == LT.f32(w) and step['x0']['t'] == p['->']['t']
            assert step['noise'] == before['noise']
        else:
            assert p['op'] == 'tile_project_noise' and p['tables_i']['off'] == i * 2 * 16 * 16
            assert p['noise'] == before['noise'] and p['out_noise'] is None                 # the draw the constant chain hands to its step
            assert step['x0']['t'] == p['->'][0]['t'] and step['noise']['t'] == p['->'][1]['t'] != p['noise']['t']
    kinds = [k for k, _ in want]
    assert not projections and kinds[-1] == 'plain' and rows[-1, 3] == 0
    assert set(kinds[:-1]) == ({'noise'} if sigma is SIG224 else {'tile'})
    rest = lambda t: [r['op'] for r in _launches(t) if r['op'] not in ('tile_project', 'tile_project_noise')]
    assert rest(got) == rest(absent)


def _volume_case(monkeypatch, name, fn=None, **extra):
    """One ``VolumeInference`` case of the launch-trace module with an operator (and what ``extra`` adds) switched on."""
    from tests import test_volume_launch_trace_host as T
    monkeypatch.setitem(T.RETURNS, 'tile_backproject', lambda a: torch.full((40, 36, 44), 300.0))
    for op, f in _host({}).items():
        monkeypatch.setitem(T.RETURNS, op, f)
    for op in ('volume_joint_consistent_tile_step', 'volume_joint_consistent_tile_noise_step'):
        monkeypatch.setitem(T.RETURNS, op, lambda a: (a['out'], a['x0_out']))
    monkeypatch.setattr(T.StubDenoiser, 'state_space', lambda self, x: self.rec.record('state_space', {'x': x}, 2 * x - 1), raising=False)
    case = dict(T.CASES[name])
    case['kw'] = dict(case['kw'], consistency=(torch.full((12, 20, 18, 22), 300.0), (2, 2, 2)), consistency_weight=0.5,
                      consistency_operator=A222, **extra)
    if fn is not None:
        case['fn'] = fn
    monkeypatch.setitem(T.CASES, 'row-case', case)
    return T.run_case('row-case'), case['cfg']


@pytest.mark.parametrize('chain', ['step', 'multistep', 'sigma-base1'])
def test_joint_chain_without_a_value_is_the_trace_with_the_keyword_absent(chain, monkeypatch):
    absent, _ = _volume_case(monkeypatch, f'joint-{chain}-selfcond')
    none, _ = _volume_case(monkeypatch, f'joint-{chain}-selfcond', consistency_row_noise=None)
    assert LT.canonical(absent) == LT.canonical(none) and not any(r['op'] in NEW for r in none)


@pytest.mark.parametrize('sigma_state', [0.01, 0.03, 1e-12])
@pytest.mark.parametrize('chain', ['step', 'sigma-base1'])
def test_joint_chain_dispatches_row_by_row(chain, sigma_state, monkeypatch):
    """``state_space`` is 2 x - 1 here, so the raw deviations are divided by the z-score's std and doubled; ``sigma_state`` is the
    smallest of them in state units."""
    from tests import test_volume_launch_trace_host as T
    name = f'joint-{chain}-selfcond'
    plain, cfg = _volume_case(monkeypatch, name)
    per_row = np.array(SIG222) / min(SIG222)
    raw = (per_row * sigma_state * float(cfg['Data']['std']) / 2.0).tolist()
    got, _ = _volume_case(monkeypatch, name, consistency_row_noise=raw)
    den = T.CASES[name]['fn'](LT.Recorder())
    wh = TN.whiten(A222, raw)
    want = TN.kinds(TN.schedule64(TN.rows4(den.coefs.numpy()), wh['S'], wh['sigma_min'] / float(cfg['Data']['std']) * 2.0, 0.5))
    form = 0 if chain == 'step' else 2
    plain_op = 'volume_joint_step' if chain == 'step' else 'volume_joint_multistep_sde'
    fused = (plain_op, 'volume_joint_consistent_tile_step', 'volume_joint_consistent_tile_noise_step')
    new = [r for r in _launches(got) if r['op'] in fused and r.get('x_t') is not None]
    old = [r for r in _launches(plain) if r['op'] in fused and r.get('x_t') is not None]
    assert len(new) == len(old) == 2 * 3 and all(r['op'] == fused[1] for r in old)          # S = 2 samples of T = 3 steps
    kinds, uploads = set(), set()
    for k, (n, o) in enumerate(zip(new, old)):
        kind, w = want[k % 3]
        kinds.add(kind)
        for key in ('y', 'x_t', 'out', 'x0_out', 'kx', 'k0', 'lo', 'hi', 'clamp_mode', 'stride'):   # the same buffers, coefficients and clamp
            assert n[key] == o[key] or (isinstance(n[key], dict) and n[key]['t'].split('#')[1] == o[key]['t'].split('#')[1]), key
        if kind == 'plain':
            assert n['op'] == plain_op and (n['kn'], n['draw'], n['sample']) == (o['kn'], o['draw'], o['sample'])
            continue
        assert n['form'] == form and n['cell'] == [2, 2, 2] and n['meas_up']['t'] == o['meas_up']['t'] and n['kn'] == o['kn']
        assert (n['seed'], n['draw'], n['sample']) == (o['seed'], o['draw'], o['sample'])           # the draw numbers are unchanged
        if kind == 'tile':
            assert n['op'] == fused[1] and n['weight'] == LT.f32(w) and n['table']['shape'] == [8, 8]
        else:
            assert n['op'] == fused[2] and n['tables_i']['shape'] == [2, 8, 8] and n['tables_i']['off'] == (k % 3) * 2 * 64
            uploads.add(n['tables_i']['t'])
    print(f"{chain} sigma {sigma_state}: dispatch {want}")
    assert len(uploads) <= 1                                                               # one [T, 2, n, n] tensor per volume
    if sigma_state == 1e-12:
        assert kinds == ({'tile'} if chain == 'step' else {'tile', 'plain'})
    else:
        assert 'noise' in kinds
    rest = lambda t: [r['op'] for r in _launches(t) if r['op'] not in fused[1:] and not (r['op'] == plain_op and r.get('x_t') is not None)
                      and r['op'] != 'state_space']
    assert rest(got) == rest(plain)
    assert sum(r['op'] == 'state_space' for r in got) == sum(r['op'] == 'state_space' for r in plain) + 1   # the slope, on two host numbers


@pytest.mark.parametrize('sigma', [None, SIG222])
def test_blend_mode_hands_the_row_noise_on_exactly_when_one_was_given(sigma, monkeypatch):
    seen = []

    def sampler_of(rec):
        def sample(x, noise=None, **kw):
            seen.append(kw)
            return torch.zeros_like(x)
        return sample
    extra = {} if sigma is None else dict(consistency_row_noise=sigma)
    _, cfg = _volume_case(monkeypatch, 'blend-gaussian-s2-anchored', fn=sampler_of, **extra)
    assert seen
    for kw in seen:
        assert set(kw) == {'consistency', 'consistency_weight', 'consistency_operator'} | set(extra)
        if sigma is not None:                                 # z-scored like the measurement
            assert np.allclose(kw['consistency_row_noise'], np.array(sigma) / float(cfg['Data']['std']), rtol=1e-15)
            assert kw['consistency_operator'].pinv.shape == (8, 12) and hasattr(kw['consistency_operator'], 'singular')
