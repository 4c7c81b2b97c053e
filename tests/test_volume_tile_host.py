"""Host-side checks of data consistency for a tile-local linear operator (no GPU here): ``ops.tile_operator`` /
``ops.stack_operator`` / ``ops.stack_rows`` against tests/volume_joint_tile_reference.py and the numbers of their docstrings, every
argument rule of ``consistency_operator=`` raised before anything touches the device, the fp32 restatement of the projection as exact
rational arithmetic rounded once per operation and within its derived count of float64, the error codes of the four new entries, and
-- with recording stand-ins -- every sampler and the joint chain making the launches they made without an operator, each
``cell_project`` / ``volume_joint_consistent_step`` replaced by its tile twin on the same operands."""
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import launch_trace as LT
from tests import volume_blend_reference as R
from tests import volume_joint_heun_reference as HN
from tests import volume_joint_tile_reference as TR
from tests.test_volume_joint_host import _imagen


# ---- T1: the operator -------------------------------------------------------------------------------------------------------------------
STACKS = {((4, 4, 1), (0, 1)): (8, 7), ((2, 2, 2), (0, 1, 2)): (12, 7), ((4, 4, 4), (0, 1, 2)): (48, 37), ((3, 2, 1), (0, 1)): (5, 4)}


@pytest.mark.parametrize('cell,axes', list(STACKS))
def test_stack_operator_has_the_documented_rows_and_rank(cell, axes):
    from diffusioniqt_amd import ops
    op = ops.stack_operator(cell, axes)
    n = cell[0] * cell[1] * cell[2]
    assert (op.m, op.rank) == STACKS[(cell, axes)] and op.n == n and op.cell == cell
    assert np.array_equal(op.A.numpy(), TR.stack_matrix(cell, axes))
    P = op.table.numpy()
    assert P.dtype == np.float32 and P.shape == (n, n) and op.table.is_contiguous() and op.table.device.type == 'cpu'
    assert np.array_equal(P.view(np.uint32), P.T.copy().view(np.uint32))                   # symmetric to the bit
    P64 = P.astype(np.float64)
    assert np.abs(P64 @ P64 - P64).max() <= 4 * n * 2.0 ** -24 and np.abs(P64.sum(1) - 1).max() <= n * 2.0 ** -24
    assert 1.65 <= op.gain < 3.65 and op.gain == TR.gain_of(P)                             # 1.7 .. 3.6 to one decimal ((3, 2, 1): 5 / 3)
    pinv, want, rank = TR.projector(op.A.numpy())
    assert rank == op.rank and np.abs(P64 - want).max() <= 1e-7 and np.abs(op.pinv.numpy() - pinv).max() <= 1e-12
    assert np.abs(want.sum(1) - 1).max() <= 1e-13                                          # the accuracy of a pseudo-inverse of this size


def test_one_row_operators_give_the_exact_uniform_table():
    from diffusioniqt_amd import ops
    for f in (2, 3, 4, 5, 7):
        a = ops.stack_operator((f, 1, 1), (0,))
        b = ops.tile_operator((1, 1, f), [[1.0 / f] * f])
        want = np.full((f, f), 1.0 / f).astype(np.float32)
        assert (a.m, a.rank, b.m, b.rank) == (1, 1, 1, 1)
        assert np.array_equal(a.table.numpy().view(np.uint32), want.view(np.uint32))
        assert np.array_equal(b.table.numpy().view(np.uint32), want.view(np.uint32))
    assert ops.tile_operator((4, 1, 1), a_op := ops.stack_operator((4, 1, 1), (0,))) is a_op       # an operator passes through


def test_a_profile_row_has_the_rank_one_projector_and_belongs_to_consistency_profile():
    """P of the single row u is u u^T / |u|^2 (``ops.tile_projector``).  As an operator it is blind to the tile mean unless u is
    constant, so ``tile_operator`` refuses it and names the keyword that offers it."""
    from diffusioniqt_amd import ops
    u = np.array([1.0, 3.0, 3.0, 1.0]) / 8
    pinv, P, rank = ops.tile_projector(torch.from_numpy(u[None]))
    assert rank == 1 and np.abs(P.numpy() - np.outer(u, u) / (u @ u)).max() <= 1e-15
    assert np.abs(pinv.numpy()[:, 0] - u / (u @ u)).max() <= 1e-15
    with pytest.raises(ValueError, match="consistency_operator.*blind to the tile mean.*consistency_profile"):
        ops.tile_operator((4, 1, 1), u[None])


def test_tile_operator_refusals():
    from diffusioniqt_amd import ops
    ok = [[0.5, 0.5]]
    for cell in ((1, 1, 1), (2, 2), (8, 4, 4), (2.0, 1, 1)):                               # the cell's own rules
        with pytest.raises(ValueError, match="consistency_operator"):
            ops.tile_operator(cell, ok)
    bad = [None, 'abc', [[0.5, 0.5, 0.5]], [0.5, 0.5], np.zeros((0, 2)), [[float('nan'), 1.0]], [[float('inf'), 1.0]],
           [[0.0, 0.0]],                                                                    # rank 0
           [[1.0, 1.0], [1.0, 1.0 + 1e-8]],                                                 # a singular value of 2.5e-9 s_max: ambiguous
           [[1.0, -1.0]], [[1.0, 0.0]]]                                                     # blind to the tile mean
    for A in bad:
        with pytest.raises(ValueError, match="consistency_operator"):
            ops.tile_operator((1, 1, 2), A)
    assert ops.tile_operator((1, 1, 2), [[1.0, 1.0], [1.0, 1.0 + 1e-12]]).rank == 1         # at or below 1e-10 s_max: a zero
    assert ops.tile_operator((1, 1, 2), [[1.0, 1.0], [1.0, 1.0 + 1e-5]]).rank == 2
    with pytest.raises(ValueError, match="consistency_operator"):
        ops.tile_operator((2, 1, 1), ops.stack_operator((1, 1, 2), (2,)))                   # made for another cell
    for axes in ((), (0, 0), (3,), 0, (True,)):
        with pytest.raises(ValueError, match="consistency_operator"):
            ops.stack_operator((2, 2, 2), axes)


def test_stack_rows_is_the_layout_of_the_measurement():
    from diffusioniqt_amd import ops
    cell, axes = (2, 3, 2), (2, 0, 1)
    v = np.random.default_rng(1).standard_normal((4, 6, 8))
    stacks = [v.reshape(4, 6, 4, 2).mean(3), v.reshape(2, 2, 6, 8).mean(1), v.reshape(4, 2, 3, 8).mean(2)]
    got = ops.stack_rows([torch.from_numpy(s) for s in stacks], cell, axes)
    want = TR.measure64(v, cell, TR.stack_matrix(cell, axes))
    assert tuple(got.shape) == want.shape == (6 + 6 + 4, 2, 2, 4) and got.is_contiguous()
    assert np.abs(got.numpy() - want).max() <= 1e-15
    with pytest.raises(ValueError, match="consistency_operator"):
        ops.stack_rows([torch.from_numpy(stacks[0])], cell, axes)
    with pytest.raises(ValueError, match="consistency_operator"):
        ops.stack_rows([torch.from_numpy(s) for s in stacks[::-1]], cell, axes)


# ---- T2: argument rules, all before the device is touched -----------------------------------------------------------------------------------
OK_A = TR.stack_matrix((2, 2, 2), (0, 1, 2))


def _meas(P=16, B=2):
    return torch.zeros(B, 1, P, P, P)


def test_sample_refuses_an_operator_it_cannot_honour():
    imagen = _imagen()
    lr = torch.zeros(2, 1, 16, 16, 16)
    base = dict(batch_size=2, start_image_or_video=lr, start_at_unet_number=2, use_tqdm=False, sampler='ddim', sample_steps=2)
    ok = (_meas(), (2, 2, 2))
    named = [dict(consistency_operator=OK_A),                                              # an operator without consistency
             dict(consistency=ok, consistency_operator=OK_A, consistency_profile=((1, 2), (1, 1), (3, 1))),
             dict(consistency=ok, consistency_operator=OK_A, consistency_noise=0.1, eta=0.5),
             dict(consistency=ok, consistency_operator=OK_A[:, :4]),                        # n of another cell
             dict(consistency=ok, consistency_operator=[[1.0, 0, 0, 0, 0, 0, 0, 0]])]       # blind to the mean
    for kw in named:
        with pytest.raises(ValueError, match="consistency_operator"):
            imagen.sample(**{**base, **kw})
    with pytest.raises(ValueError, match="a profile is the single row"):
        imagen.sample(**{**base, **named[1]})
    kept = [(dict(consistency_weight=0.0), "consistency weight"), (dict(init_images=lr), "neither init_images nor skip_steps"),
            (dict(sampler='ddpm', sample_steps=None, skip_steps=2), "neither init_images nor skip_steps"),
            (dict(sampler='ddpm', inpaint_images=lr, inpaint_masks=lr[:, 0].bool()), "inpainting are not offered together"),
            (dict(consistency=(_meas(), (3, 1, 1))), "does not divide")]
    for kw, wording in kept:                                                               # every existing refusal keeps its wording
        with pytest.raises(ValueError, match=wording):
            imagen.sample(**{**base, 'consistency': ok, 'consistency_operator': OK_A, **kw})
    for kw in (dict(consistency_operator=OK_A), dict(consistency=ok, consistency_operator=np.zeros((2, 8)))):
        with pytest.raises(ValueError, match="consistency_operator"):                      # the loop itself applies the same rules
            imagen.p_sample_loop(imagen.unets[1], (2, 1, 16, 16, 16), noise_scheduler=imagen.noise_schedulers[1], **kw)


def test_edm_sample_refuses_an_operator_it_cannot_honour():
    elu = HN.make_elucidated('churn-on', False)
    lr = torch.zeros(2, 1, 16, 16, 16)
    base = dict(batch_size=2, video_frames=16, start_image_or_video=lr, start_at_unet_number=2, use_tqdm=False, sampler='dpmpp2m')
    ok = (_meas(), (2, 2, 2))
    for kw in (dict(consistency_operator=OK_A), dict(consistency_operator=OK_A, sampler='heun'),
               dict(consistency=ok, consistency_operator=OK_A, consistency_profile=((1, 2), (1, 1), (3, 1))),
               dict(consistency=ok, consistency_operator=OK_A, consistency_noise=0.1, eta=0.5),
               dict(consistency=ok, consistency_operator=[[1.0] * 8, [1.0] * 7 + [1 + 1e-8]])):     # an ambiguous rank
        with pytest.raises(ValueError, match="consistency_operator"):
            elu.sample(**{**base, **kw})
    kept = [(dict(sampler='heun'), "Heun sampler"), (dict(init_images=lr), "neither init_images nor skip_steps"),
            (dict(consistency_weight=2), "consistency weight"),
            (dict(sampler='heun', inpaint_images=lr, inpaint_masks=lr[:, 0].bool()), "consistency")]
    for kw, wording in kept:
        with pytest.raises(ValueError, match=wording):
            elu.sample(**{**base, 'consistency': ok, 'consistency_operator': OK_A, **kw})
    for kw in (dict(consistency_operator=OK_A), dict(consistency=ok, consistency_operator=OK_A, consistency_noise=0.5, eta=0.5)):
        with pytest.raises(ValueError, match="consistency_operator"):
            elu.one_unet_sample(elu.unets[1], (2, 1, 16, 16, 16), unet_number=2, sampler='dpmpp2m', **kw)


def test_volume_inference_operator_argument_errors():
    from diffusioniqt_amd import ops
    from diffusioniqt_amd.inference import VolumeInference

    def never(x, **kw):
        raise AssertionError("the sampler must not run")
    cfg = R.shared_cfg(8)                                                                  # P 16, stride 8, volume (40, 36, 44)
    y = torch.zeros(12, 20, 18, 22)
    ok = (y, (2, 2, 2))
    known = (torch.zeros(40, 36, 44), torch.zeros(40, 36, 44, dtype=torch.bool))
    for kw in (dict(consistency_operator=OK_A),                                            # an operator without consistency
               dict(consistency=ok, consistency_operator=OK_A, consistency_profile=((1, 2), (1, 1), (3, 1))),
               dict(consistency=ok, consistency_operator=OK_A, consistency_noise=3.0),
               dict(consistency=(y[:11], (2, 2, 2)), consistency_operator=OK_A),           # the leading dimension is not m
               dict(consistency=(y[0], (2, 2, 2)), consistency_operator=OK_A),             # no leading dimension at all
               dict(consistency=ok, consistency_operator=OK_A[:, :4]),
               dict(consistency=ok, consistency_operator=np.eye(8)[:1])):                  # blind to the mean
        with pytest.raises(ValueError, match="consistency_operator"):
            VolumeInference(cfg, never, **kw)
    kept = [(dict(inpaint=known), "consistency and inpaint are not offered together"), (dict(consistency_weight=0.0), "consistency weight"),
            (dict(consistency=(torch.zeros(5, 40, 36, 22), (1, 1, 3)), consistency_operator=TR.stack_matrix((1, 1, 3), (2,))[[0] * 5]),
             "must divide the stride")]
    for kw, wording in kept:                                                               # every existing refusal keeps its wording
        with pytest.raises(ValueError, match=wording):
            VolumeInference(cfg, never, **{'consistency': ok, 'consistency_operator': OK_A, **kw})
    with pytest.raises(ValueError, match="EDM Heun denoiser"):
        VolumeInference(cfg, HN.make_elucidated('churn-on', False).window_denoiser(), consistency=ok, consistency_operator=OK_A,
                        blend='gaussian', noise='anchored', joint=True)
    inf = VolumeInference(cfg, never, consistency=ok, consistency_operator=OK_A)
    assert inf.consistency_op.m == 12 and inf.consistency_table is None
    with pytest.raises(ValueError, match="is not the volume's shape"):                      # in __call__, before the device too
        VolumeInference(cfg, never, consistency=(y[:, :19], (2, 2, 2)), consistency_operator=OK_A)(torch.zeros(40, 36, 44))
    assert VolumeInference(cfg, never, consistency=(y[0], (2, 2, 2))).consistency_op is None        # the default is today's path
    op = ops.tile_operator((2, 2, 2), OK_A)
    assert VolumeInference(cfg, never, consistency=ok, consistency_operator=op).consistency_op is op


# ---- T3: the fp32 restatement ---------------------------------------------------------------------------------------------------------------
def _rn32(x):
    """A Fraction rounded to the nearest float32, ties to even."""
    near = np.float32(float(x))
    cands = (np.nextafter(near, np.float32(-np.inf)), near, np.nextafter(near, np.float32(np.inf)))
    return min(cands, key=lambda v: (abs(Fraction(float(v)) - x), int(v.view(np.uint32)) & 1))


def _table(name):
    from diffusioniqt_amd import ops
    cell, A = TR.matrix_of(name)
    return cell, A, ops.tile_operator(cell, A)


@pytest.mark.parametrize('w', [1.0, 0.5])
@pytest.mark.parametrize('name', list(TR.OPERATORS))
def test_project_tile32_is_exact_arithmetic_rounded_once_per_operation(name, w):
    """On random tiles: s = rn(P[r][q] a[r] + s) in the order of r, d = rn(t[q] - s), a' = rn(w d + a[q]), every rn ONE rounding of the
    exact rational value; and the result is within the one-projection count of float64, the w = 1 residual |P x0' - t| of a t in the
    row space under the derived bound too."""
    cell, A, op = _table(name)
    P, n = op.table.numpy(), op.n
    rng = np.random.default_rng(len(name))
    count = 6 if n < 64 else 2
    shape = (cell[0], cell[1], cell[2] * count)                                            # `count` tiles along x
    a = (rng.standard_normal(shape) * 2).astype(np.float32)
    y = rng.standard_normal((op.m, 1, 1, count)).astype(np.float32)
    t = TR.backproject32(y, cell, op.pinv.numpy())
    assert t.shape == shape
    got = TR.project_tile32(a, t, cell, P, w)
    F = lambda v: Fraction(float(v))
    for c in range(count):
        sl = np.s_[:, :, c * cell[2]:(c + 1) * cell[2]]
        vals, tv, have = a[sl].reshape(-1), t[sl].reshape(-1), got[sl].reshape(-1)          # lexicographic (z, y, x)
        for q in range(n if n < 64 else 5):
            s = np.float32(0)
            for r in range(n):
                s = _rn32(F(P[r, q]) * F(vals[r]) + F(s))
            want = _rn32(F(np.float32(w)) * F(_rn32(F(tv[q]) - F(s))) + F(vals[q]))
            assert have[q].view(np.uint32) == want.view(np.uint32), (c, q)
    ones = np.ones(shape, dtype=bool)
    ref, whole = TR.project_tile64(a.astype(np.float64), ones, t.astype(np.float64), cell, w, P)
    scale = max(float(np.abs(a).max()), float(np.abs(t).max()), float(np.abs(got).max()))
    bound = TR.tile_roundings(cell, P, scale)
    err = np.abs(got.astype(np.float64) - ref).max()
    print(f"tile {name} w {w}: fp32 - float64 = {err:.3e}, count {bound:.3e} ({err / bound:.3f}), gain {op.gain:.3f}")
    assert whole.all() and err <= bound and (got != a).mean() > 0.9
    if w == 1.0:                                                                           # P x0' = t
        res = np.abs(TR.apply64(got, cell, P) - t).max()
        limit = TR.residual_bound_P(cell, P, op.pinv.numpy(), float(np.abs(y).max()), 1.0, scale)
        print(f"tile {name}: w = 1 residual |P x0' - t| = {res:.3e}, bound {limit:.3e}")
        assert res <= limit


def test_measure_and_backproject_restatements_are_the_float64_operator():
    for name in TR.OPERATORS:
        cell, A, op = _table(name)
        x = (np.random.default_rng(3).standard_normal(tuple(2 * f for f in cell)) * 2).astype(np.float32)
        y = TR.measure32(x, cell, A)
        want = TR.measure64(x, cell, A)
        norm = np.abs(A).sum(1).max()
        assert y.shape == want.shape == (op.m, 2, 2, 2) and np.abs(y - want).max() <= 2 * op.n * 2.0 ** -24 * norm * np.abs(x).max()
        t = TR.backproject32(y, cell, op.pinv.numpy())
        t64 = TR.untile(np.moveaxis(y.astype(np.float64), 0, -1) @ op.pinv.numpy().T, cell)
        assert np.abs(t - t64).max() <= (op.m + 1) * 2.0 ** -24 * np.abs(op.pinv.numpy()).sum(1).max() * np.abs(y).max()
        assert np.abs(TR.apply64(x, cell, op.table.numpy()) - t64).max() <= 1e-5 * np.abs(x).max()          # A+ A x = P x


def test_a_one_row_operator_is_the_uniform_projection_within_the_counts():
    """The arithmetic differs from ``cell_mean`` / ``cell_shift`` (products with 1 / n in the sum, no division), so the bits do too."""
    from tests import volume_joint_dc_reference as DC
    cell, A, op = _table('stack-411')
    rng = np.random.default_rng(8)
    a = (rng.standard_normal((8, 8, 8)) * 2).astype(np.float32)
    meas = TR.replicate(rng.standard_normal((2, 8, 8)).astype(np.float32), cell)
    got, old = TR.project_tile32(a, meas, cell, op.table.numpy(), 1.0), DC.project32(a, meas, cell, 1.0)
    scale = max(float(np.abs(a).max()), float(np.abs(meas).max()), float(np.abs(got).max()))
    assert op.gain == 1.0 and TR.tile_roundings(cell, op.table.numpy(), scale) == DC.projection_roundings(cell, scale)
    assert np.abs(got.astype(np.float64) - old).max() <= 2 * DC.projection_roundings(cell, scale)


# ---- T4: the error codes of the entries ---------------------------------------------------------------------------------------------------
def test_tile_entries_return_error_codes():
    from diffusioniqt_amd import _lib
    lib = _lib.load()
    buf = (np.zeros(4, dtype=np.int32)).ctypes.data                             # never dereferenced: every call below is refused

    for entry in (lib.diqt_tile_measure, lib.diqt_tile_backproject):
        def op(ptrs=(buf, buf, buf), m=3, vol=(8, 8, 8), cell=(2, 2, 2)):
            return entry(*ptrs, m, *vol, *cell, None)
        for k in range(3):
            assert op(tuple(None if i == k else buf for i in range(3))) == -2, k
        assert b"null pointer" in lib.diqt_last_error()
        assert op(cell=(1, 1, 1)) == -3 and op(cell=(8, 8, 2)) == -3 and op(cell=(0, 2, 2)) == -3
        assert op(cell=(3, 1, 1)) == -1 and op(vol=(8, 0, 8)) == -1 and op(m=0) == -1

    def proj(ptrs=(buf,) * 4, cubes=3, P=8, cell=(2, 2, 2), w=1.0, mode=2):
        return lib.diqt_tile_project(*ptrs, cubes, P, *cell, w, -1.0, 1.0, mode, None)
    for k in range(4):
        assert proj(tuple(None if i == k else buf for i in range(4))) == -2, k
    assert proj(w=0.0) == -3 and proj(w=1.5) == -3 and proj(mode=3) == -3
    assert proj(cell=(1, 1, 1)) == -3 and proj(cell=(8, 8, 2)) == -3
    assert proj(cell=(1, 1, 3)) == -1 and proj(cubes=0) == -1
    geo = (40, 36, 44, 16, 8, 4, 3, 4)                                          # D, H, W, P, stride and the lattice of range(0, n - 15, 8)

    def step(ptrs=(buf,) * 9, form=0, geo=geo, cell=(2, 2, 2), w=1.0, mode=0):
        return lib.diqt_volume_joint_consistent_tile_step(*ptrs, form, 3, *geo, *cell, w, 1.0, 0.5, 0.0, 0.25, -1.0, 1.0, mode, 0, 1, 0, None)
    assert step(form=3) == -3 and step(form=-1) == -3
    assert step(w=0.0) == -3 and step(cell=(1, 1, 1)) == -3 and step(cell=(4, 4, 8)) == -3 and step(mode=2) == -3
    for k in (0, 1, 2, 3, 5, 6, 7, 8):                                          # x0_prev alone may be NULL
        assert step(tuple(None if i == k else buf for i in range(9))) == -2, k
    assert step(cell=(3, 1, 1)) == -1 and step(geo=(40, 36, 44, 16, 8, 4, 3, 5)) == -1
    # a plan above 64 KiB of LDS is an error code, not a launch: the box of the cell (64, 1, 1) is 64 x 1 x 64 = 4096 voxels, x0s and
    # dens 32 KiB, the table 16 KiB, and 4104 taps make it 64 KiB + 32 bytes; every other check passes
    big = (4160, 4104, 4104, 4104, 4104, 1, 1, 1)
    assert (4104 + 2 * 4096 + 64 * 64) * 4 == 65536 + 32 and 4160 % 64 == 0
    assert step(geo=big, cell=(64, 1, 1)) == -1 and b"LDS" in lib.diqt_last_error()


# ---- T5: routing, with recording stand-ins ----------------------------------------------------------------------------------------------------
HOST_ONLY = ('consistency_cell', 'tile_operator')


def _as_uniform(trace, new, old):
    """The canonical trace with every ``new`` record turned into the ``old`` record it stands for: the table operand dropped (it must be
    the one [n, n] table of the chain), ``target`` named ``meas_up``, the op and the buffer tags made from its name renamed; the
    once-per-volume ``tile_backproject`` stands where ``cell_replicate`` stood.  Host-only calls are left out."""
    out, tables = [], set()
    for r in trace:
        if r['op'] in HOST_ONLY:
            continue
        r = dict(r)
        if r['op'] == new:
            t = r.pop('table')
            tables.add((t['t'], tuple(t['shape']), t['dtype']))
            if 'target' in r:
                r['meas_up'] = r.pop('target')
        if r['op'] in ('tile_backproject', 'cell_replicate'):
            r = {'op': 'cell_replicate', '->': r['->']}
        out.append(r)
    return LT.canonical(out).replace(new, old).replace('tile_backproject', 'cell_replicate'), tables


def _imagen_trace(sampler, eta, operator):
    from diffusioniqt_amd import imagen_pytorch3D, ops
    into = lambda key: (lambda a: a['out'] if a.get('out') is not None else torch.zeros_like(a[key]))
    returns = {'axpby3': lambda a: torch.zeros_like(a['a']), 'ddpm_step': lambda a: (torch.zeros_like(a['x_t']), torch.zeros_like(a['x_t'])),
               'cell_project': into('x0'), 'tile_project': into('x0'),
               'consistency_cell': lambda a: ops.consistency_cell(**a), 'tile_operator': lambda a: ops.tile_operator(**a)}
    rec = LT.Recorder()
    imagen = _imagen()
    lr, meas = torch.zeros(2, 1, 16, 16, 16), torch.full((2, 1, 16, 16, 16), 0.125)
    rec.tag(lr, 'lowres'), rec.tag(meas, 'meas_up')
    noise = [LT.zeros(2, 1, 16, 16, 16) for _ in range(8)]
    for k, t in enumerate(noise):
        rec.tag(t, f'noise{k}')
    kw = dict(consistency=(meas, (2, 2, 4)), consistency_weight=0.5)
    if operator is not None:
        kw.update(consistency_operator=operator)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(imagen_pytorch3D, 'ops', LT.RecordingOps(rec, returns))
        out = imagen.sample(batch_size=2, start_image_or_video=lr, start_at_unet_number=2, use_tqdm=False, device='cpu', sampler=sampler,
                            sample_steps=3, eta=eta, noise=noise, **kw)[0]
    rec.record('return', {}, out)
    return rec.trace


A224 = TR.stack_matrix((2, 2, 4), (0, 2))


@pytest.mark.parametrize('sampler,eta', [('ddim', 0.0), ('ddim', 0.5), ('ddpm', 0.0), ('dpmpp2m', 0.0)])
def test_imagen_sample_with_an_operator_makes_the_same_launches(sampler, eta):
    plain = _imagen_trace(sampler, eta, None)
    got = _imagen_trace(sampler, eta, A224)
    assert sum(r['op'] == 'cell_project' for r in plain) == 3 and not any(r['op'] == 'tile_project' for r in plain)
    assert sum(r['op'] == 'tile_project' for r in got) == 3 and not any(r['op'] == 'cell_project' for r in got)
    a, none = _as_uniform(plain, 'tile_project', 'cell_project')
    b, tables = _as_uniform(got, 'tile_project', 'cell_project')
    assert a == b and not none and len(tables) == 1 and next(iter(tables))[1:] == ((16, 16), 'torch.float32')


@pytest.mark.parametrize('eta,self_cond', [(0.0, False), (0.5, True)])
def test_edm_sample_with_an_operator_makes_the_same_launches(eta, self_cond, monkeypatch):
    from diffusioniqt_amd import ops
    from tests import test_edm_sampler_trace_host as T
    monkeypatch.setitem(T.RETURNS, 'tile_project', T._into('x0'))
    monkeypatch.setitem(T.RETURNS, 'tile_operator', lambda a: ops.tile_operator(**a))
    base = dict(model=dict(self_cond=self_cond), sampler='dpmpp2m', eta=eta, consistency=0.5)
    monkeypatch.setitem(T.CASES, 'tile-off', T.sample_case(**base))
    monkeypatch.setitem(T.CASES, 'tile-on', T.sample_case(**base, consistency_operator=A224))
    plain, got = T.run_case('tile-off')[0], T.run_case('tile-on')[0]
    steps = sum(r['op'] == 'multistep_sde_step' for r in plain)
    assert steps > 0 and sum(r['op'] == 'cell_project' for r in plain) == steps
    assert sum(r['op'] == 'tile_project' for r in got) == steps and not any(r['op'] == 'cell_project' for r in got)
    a, none = _as_uniform(plain, 'tile_project', 'cell_project')
    b, tables = _as_uniform(got, 'tile_project', 'cell_project')
    assert a == b and not none and len(tables) == 1 and next(iter(tables))[1:] == ((16, 16), 'torch.float32')


def _volume_case(monkeypatch, name, fn=None, operator=None):
    """One ``VolumeInference`` case of the launch-trace module with consistency (and the operator, if any) switched on."""
    from diffusioniqt_amd import ops
    from tests import test_volume_launch_trace_host as T
    monkeypatch.setitem(T.RETURNS, 'cell_replicate', lambda a: ops.cell_replicate(a['meas'], a['cell']))
    monkeypatch.setitem(T.RETURNS, 'tile_backproject', lambda a: torch.full((40, 36, 44), 300.0))
    monkeypatch.setitem(T.RETURNS, 'consistency_cell', lambda a: ops.consistency_cell(**a))
    monkeypatch.setitem(T.RETURNS, 'tile_operator', lambda a: ops.tile_operator(**a))
    for op in ('volume_joint_consistent_step', 'volume_joint_consistent_tile_step'):
        monkeypatch.setitem(T.RETURNS, op, lambda a: (a['out'], a['x0_out']))
    monkeypatch.setattr(T.StubDenoiser, 'state_space', lambda self, x: self.rec.record('state_space', {'x': x}, x), raising=False)
    case = dict(T.CASES[name])
    meas = torch.full((20, 18, 22), 300.0)
    if operator is None:
        extra = dict(consistency=(meas, (2, 2, 2)))
    else:
        extra = dict(consistency=(meas.expand(operator.shape[0], -1, -1, -1).contiguous(), (2, 2, 2)), consistency_operator=operator)
    case['kw'] = dict(case['kw'], consistency_weight=0.5, **extra)
    if fn is not None:
        case['fn'] = fn
    monkeypatch.setitem(T.CASES, 'tile-case', case)
    return T.run_case('tile-case')


@pytest.mark.parametrize('chain', ['step', 'multistep', 'sigma-base1'])
def test_joint_chain_with_an_operator_makes_the_same_launches(chain, monkeypatch):
    name = f'joint-{chain}-selfcond'
    plain = _volume_case(monkeypatch, name)
    got = _volume_case(monkeypatch, name, operator=OK_A)
    old, new = 'volume_joint_consistent_step', 'volume_joint_consistent_tile_step'
    launches = sum(r['op'] == old for r in plain)
    assert launches == 2 * 3 and not any(r['op'] == new for r in plain)                    # S = 2 samples of T = 3 steps
    assert sum(r['op'] == new for r in got) == launches and not any(r['op'] == old for r in got)
    assert sum(r['op'] == 'tile_backproject' for r in got) == sum(r['op'] == 'cell_replicate' for r in plain) == 1     # once per volume
    a, none = _as_uniform(plain, new, old)
    b, tables = _as_uniform(got, new, old)
    assert a == b and not none and len(tables) == 1 and next(iter(tables))[1:] == ((8, 8), 'torch.float32')


@pytest.mark.parametrize('operator', [None, OK_A])
def test_blend_mode_hands_the_operator_on_exactly_when_one_was_given(operator, monkeypatch):
    seen = []

    def sampler_of(rec):
        def sample(x, noise=None, **kw):
            seen.append(kw)
            return torch.zeros_like(x)
        return sample
    _volume_case(monkeypatch, 'blend-gaussian-s2-anchored', fn=sampler_of, operator=operator)
    assert seen
    for kw in seen:
        assert set(kw) == {'consistency', 'consistency_weight'} | ({'consistency_operator'} if operator is not None else set())
        assert operator is None or (kw['consistency_operator'].m == 12 and tuple(kw['consistency'][0].shape[1:]) == (1, 16, 16, 16))
