"""``ElucidatedImagen(sampler='dpmpp2m')`` on a real MI355X against the float64 specification of tests/edm_dpmpp2m_reference.py: the two
new kernels on their own (``ops.multistep_sde_step``, ``ops.volume_joint_multistep_sde``), ``sample(sampler='dpmpp2m')`` with the stub
network and with the two real tiny networks (the specification driven by the fixture-pinned oracle networks of oracle/), the draws it
consumes, and the joint chain of ``VolumeInference(joint=True)`` with its bit-for-bit tie to independent windows at stride = patch.

Bounds.  Kernels: per test below.  Chains with the stub network: ``edm_dpmpp2m_reference.chain_bound``, derived in that module's
docstring; tests/test_edm_dpmpp2m_host.py holds an fp32 emulation of the chain under it and the bound to 1e-3 of the signal.  Chains with
a real network: no Lipschitz constant is known for it, so the comparison is held to what tests/test_gpu_family_b.py holds the Heun
sampler of the same two networks to against the same oracles (max error 5e-3, at most 3 % of the voxels above 2e-4) -- that chain has
5 network evaluations, this one has 4."""
import itertools
import json
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import edm_dpmpp2m_reference as E
from tests import volume_blend_reference as R
from tests import volume_joint_heun_reference as HN
from tests import volume_joint_reference as J
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
K = HN.HP['num_sample_steps']                 # 4 steps, sigma from 1.5 to 0.3
_REF = {}


def _ref(key, make):
    """One float64 reference per case, shared by the tests that need it and never modified."""
    if key not in _REF:
        _REF[key] = make()
        for v in _REF[key].values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return _REF[key]


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def fmaf_host(a, x, b):
    """fl32(a x + b) with ONE rounding, elementwise on fp32 arrays: the exact rational value, then the nearest fp32 (ties to even)."""
    out = np.empty(x.shape, dtype=np.float32)
    for idx in np.ndindex(*x.shape):
        exact = Fraction(float(a[idx])) * Fraction(float(x[idx])) + Fraction(float(b[idx]))
        c = np.float32(float(exact))
        best = None
        for cand in (np.nextafter(c, np.float32(-np.inf)), c, np.nextafter(c, np.float32(np.inf))):
            key = (abs(Fraction(float(cand)) - exact), int(cand.view(np.uint32)) & 1)
            if best is None or key < best[0]:
                best = (key, cand)
        out[idx] = best[1]
    return out


# ---- G1: the per-window kernel ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def step_case():
    """B = 3 samples with a coefficient row each, per = 1 x 7 x 9 x 11 = 693 elements (a multiple of nothing); read only."""
    rng = np.random.default_rng(21)
    shape = (3, 1, 7, 9, 11)
    t = {k: (rng.standard_normal(shape) * s).astype(np.float32) for k, s in (('x', 3.0), ('x0', 1.0), ('prev', 1.0), ('noise', 1.0))}
    t['coefs'] = np.array([[0.8125, 0.9375, -0.4375, 0.25], [0.3125, 1.21875, -0.53125, 0.0], [0.5, 0.75, -0.25, 1.0]], dtype=np.float32)
    return t


@pytest.mark.parametrize('case', ['full', 'no-history', 'no-noise', 'neither'])
def test_step_kernel_matches_reference(step_case, case):
    """With S = scale, the largest magnitude among the operands and the expected output, and A = sum_j |k_j| of a row: the three
    rounded products cost at most 2^-24 of their own magnitudes, together <= 2^-24 A S; the fma and the two sums round a partial
    sum, each <= 2^-24 A S.  In all 4 A 2^-24 S <= 5 2^-23 S, since A <= 2.5 in every row of the fixture."""
    from diffusioniqt_amd import ops
    c = step_case
    prev = c['prev'] if case in ('full', 'no-noise') else None
    noise = c['noise'] if case in ('full', 'no-history') else None
    col = lambda j: c['coefs'][:, j].astype(np.float64).reshape(3, 1, 1, 1, 1)
    want = col(0) * c['x'] + col(1) * c['x0']
    if prev is not None:
        want = want + col(2) * prev
    if noise is not None:
        want = want + col(3) * noise
    k = [cu(c['coefs'][:, j].copy()) for j in range(4)]
    x = cu(c['x'])
    got = ops.multistep_sde_step(x, cu(c['x0']), None if prev is None else cu(prev), None if noise is None else cu(noise), *k)
    assert got.data_ptr() != x.data_ptr() and torch.equal(x, cu(c['x']))
    scale = max(float(np.abs(c[n]).max()) for n in ('x', 'x0', 'prev', 'noise'))
    scale = max(scale, float(np.abs(want).max()))
    err = np.abs(got.cpu().numpy().astype(np.float64) - want).max()
    print(f"multistep_sde_step {case}: max err {err:.3e}, bound {5 * 2.0 ** -23 * scale:.3e}")
    assert err <= 5 * 2.0 ** -23 * scale
    if noise is not None:                                                       # the row with kn == 0 does not read its noise
        poisoned = c['noise'].copy()
        poisoned[1] = np.nan
        again = ops.multistep_sde_step(x, cu(c['x0']), None if prev is None else cu(prev), cu(poisoned), *k)
        assert torch.equal(again, got)
    same = ops.multistep_sde_step(x, cu(c['x0']), None if prev is None else cu(prev), None if noise is None else cu(noise), *k, out=x)
    assert same.data_ptr() == x.data_ptr() and torch.equal(x, got)             # in place = out of place, bit for bit


def test_step_kernel_without_history_and_noise_is_one_fma(step_case):
    """kn = kp = 0: the bits of fmaf(kx, x, k0 x0) with the product k0 x0 rounded first, computed on the host."""
    from diffusioniqt_amd import ops
    c = step_case
    bc = lambda j: np.broadcast_to(c['coefs'][:, j].reshape(3, 1, 1, 1, 1), c['x'].shape)
    want = fmaf_host(bc(0), c['x'], bc(1) * c['x0'])
    zero = torch.zeros(3, device=DEV)
    k = [cu(c['coefs'][:, j].copy()) for j in range(2)]
    for prev, noise in ((None, None), (cu(c['prev']), cu(c['noise']))):
        got = ops.multistep_sde_step(cu(c['x']), cu(c['x0']), prev, noise, *k, zero, zero)
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))


def test_step_kernel_argument_errors(step_case):
    from diffusioniqt_amd import ops
    x, k = cu(step_case['x']), torch.ones(3, device=DEV)
    with pytest.raises(ValueError, match="x0 must have"):
        ops.multistep_sde_step(x, x[:2].contiguous(), None, None, k, k, k, k)
    with pytest.raises(ValueError, match="noise must have"):
        ops.multistep_sde_step(x, x, None, x[:, :, :3].contiguous(), k, k, k, k)
    with pytest.raises(ValueError, match=r"kp must be a \[B\]"):
        ops.multistep_sde_step(x, x, None, None, k, k, k[:2].contiguous(), k)
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.multistep_sde_step(x.transpose(2, 3), x, None, None, k, k, k, k)
    with pytest.raises(RuntimeError, match="fp32"):
        ops.multistep_sde_step(x, x, None, None, k.double(), k, k, k)


# ---- G2: the joint kernel --------------------------------------------------------------------------------------------------------------------
VOL, P = (12, 22, 70), 8        # H is no multiple of 4, W spans two x-blocks (one partial); planes 8 .. 11 are covered by no window


@pytest.fixture(scope="module")
def joint_case():
    """Per (stride, kind): the slot lattice with ONE dropped window, predictions for the kept ones, a state, a history volume, the taps
    and the float64 normals of the step's draw (read only).  Stride 5 does not divide P."""
    rng = np.random.default_rng(22)
    out = {}
    for stride, kind in itertools.product((8, 5), ('gaussian', 'constant')):
        lattice = tuple(len(range(0, s - P + 1, stride)) for s in VOL)
        slot = np.arange(int(np.prod(lattice)), dtype=np.int64)
        drop = slot.size // 2
        slot = np.where(slot == drop, -1, slot - (slot > drop)).reshape(lattice)
        y = (rng.standard_normal((slot.size - 1, P, P, P)) * 2).astype(np.float32)
        out[stride, kind] = dict(slot=slot, y=y, x=(rng.standard_normal(VOL) * 3).astype(np.float32),
                                 prev=(rng.standard_normal(VOL) * 2).astype(np.float32), taps=R.taps_of(P, kind),
                                 n=int(np.ceil(P / stride)) ** 2)                # the windows are one deep along D
    return out


SEED, DRAW, SAMPLE = 0x123456789, 5, 2
CLAMPS = {'min': (-0.75, 0., 0), 'box': (-1., 1., 1)}


def _joint_args(c):
    return cu(c['y']), cu(c['slot'].astype(np.int32)), cu(c['taps'].astype(np.float32))


@pytest.mark.parametrize('clamp', list(CLAMPS))
@pytest.mark.parametrize('kind', ['gaussian', 'constant'])
@pytest.mark.parametrize('stride', [8, 5])
def test_joint_kernel_matches_reference(joint_case, stride, kind, clamp):
    """Per voxel, with S = scale: the blend's own bound on x0, (n + 3) 2^-23 max|y|, scaled by |k0| <= 1; the update as in
    ``test_step_kernel_matches_reference``, 4 A 2^-24 S with A = sum |k_j| = 2.3125 here, under 5 2^-23 S; and the normal's distance from
    the float64 transform of the same bits (tests/test_gpu_anchored_noise.py), 5e-6 |kn| = 6.3e-7 < 2^-23 S for S >= 6.  In all
    (n + 5 + 4) 2^-23 scale is allowed."""
    from diffusioniqt_amd import ops
    c, cl = joint_case[stride, kind], CLAMPS[clamp]
    row = (0.8125, 0.9375, -0.4375, 0.125)
    normal = J.normals(VOL, SEED, DRAW, SAMPLE)
    want, want0, covered = E.joint_step(c['y'], c['slot'], c['taps'], stride, c['x'].astype(np.float64), c['prev'].astype(np.float64), row,
                                        J.clamp_of(*cl), normal)
    assert not covered[P:].any() and covered[:P].mean() > 0.5 and not covered[:P].all()    # the margins, and the planes past the windows
    args = _joint_args(c)
    x_dev, p_dev = cu(c['x']), cu(c['prev'])
    got, got0 = ops.volume_joint_multistep_sde(*args, x_dev, p_dev, *row, *cl, stride, SEED, DRAW, SAMPLE)
    assert got.data_ptr() != x_dev.data_ptr() and torch.equal(x_dev, cu(c['x'])) and torch.equal(p_dev, cu(c['prev']))
    max_y = float(np.abs(J.clamp_of(*cl)(c['y'].astype(np.float64))).max())
    scale = max(max_y, float(np.abs(c['x']).max()), float(np.abs(c['prev']).max()), float(np.abs(want).max()))
    bound = (c['n'] + 5 + 4) * 2.0 ** -23 * scale
    err = np.abs(got.cpu().numpy().astype(np.float64) - want).max()
    err0 = np.abs(got0.cpu().numpy().astype(np.float64) - want0).max()
    print(f"joint multistep sde stride {stride} {kind} clamp {clamp}: max err {err:.3e} (x0 {err0:.3e}), bound {bound:.3e}")
    assert err <= bound and err0 <= R.tolerance(c['n'], max_y)
    assert np.array_equal(got.cpu().numpy()[~covered], c['x'][~covered])        # uncovered voxels keep x_t ...
    assert not got0.cpu().numpy()[~covered].any()                               # ... and get x0_out = 0
    # in place on both pairs = out of place, bit for bit
    same_x, same_0 = ops.volume_joint_multistep_sde(*args, x_dev, p_dev, *row, *cl, stride, SEED, DRAW, SAMPLE, out=x_dev, x0_out=p_dev)
    assert same_x.data_ptr() == x_dev.data_ptr() and same_0.data_ptr() == p_dev.data_ptr()
    assert torch.equal(x_dev, got) and torch.equal(p_dev, got0)


@pytest.mark.parametrize('with_prev', [False, True], ids=['step0', 'history'])
@pytest.mark.parametrize('clamp', list(CLAMPS))
@pytest.mark.parametrize('tiling', [(8, 'constant'), (5, 'gaussian')], ids=['s8-constant', 's5-gaussian'])
def test_joint_kernel_without_noise_is_the_multistep_kernel(joint_case, tiling, clamp, with_prev):
    """kn = 0: no Philox call, and the bits of ``ops.volume_joint_multistep`` on the same inputs, state and fused x0 alike."""
    from diffusioniqt_amd import ops
    c, cl = joint_case[tiling], CLAMPS[clamp]
    args = _joint_args(c)
    x, prev = cu(c['x']), cu(c['prev']) if with_prev else None
    a, a0 = ops.volume_joint_multistep(*args, x, prev, 0.8125, 0.9375, -0.4375, *cl, tiling[0])
    b, b0 = ops.volume_joint_multistep_sde(*args, x, prev, 0.8125, 0.9375, -0.4375, 0.0, *cl, tiling[0], SEED, DRAW, SAMPLE)
    assert torch.equal(a, b) and torch.equal(a0, b0) and a.unique().numel() > 1000
    c2, _ = ops.volume_joint_multistep_sde(*args, x, prev, 0.8125, 0.9375, -0.4375, 0.625, *cl, tiling[0], SEED, DRAW, SAMPLE)
    assert not torch.equal(b, c2)


def field(shape, seed, draw, sample, edge=2):
    """Draw ``draw`` of the anchored field over a whole volume, assembled from ``ops.anchored_noise`` windows of edge 2."""
    from diffusioniqt_amd import ops
    g = [s // edge for s in shape]
    org = np.array([(edge * a, edge * b, edge * c) for a in range(g[0]) for b in range(g[1]) for c in range(g[2])], dtype=np.int32)
    w = ops.anchored_noise(org, 1, edge, *shape, seed, draw=draw, sample=sample)
    return w.reshape(*g, edge, edge, edge).permute(0, 3, 1, 4, 2, 5).reshape(shape).contiguous()


def test_joint_initial_state_is_sigma0_times_the_anchored_field():
    from diffusioniqt_amd import ops
    sigma0 = 1.4999995231628418
    for draw, sample in ((0, 0), (3, 2)):
        got, none = ops.volume_joint_multistep_sde(None, None, None, None, None, 0., 0., 0., sigma0, -1., 1., 1, 8, SEED, draw, sample,
                                                   shape=VOL)
        want = torch.tensor(sigma0, dtype=torch.float32, device=DEV) * field(VOL, SEED, draw, sample)
        assert none is None and tuple(got.shape) == VOL and torch.equal(got, want) and got.unique().numel() > 1000


def test_joint_kernel_argument_errors(joint_case):
    from diffusioniqt_amd import ops
    c = joint_case[8, 'gaussian']
    y, slot, taps = _joint_args(c)
    x, prev = cu(c['x']), cu(c['prev'])
    ok = (1.0, 0.5, -0.25, 0.5, -1.0, 1.0, 1, 8, 0, 1)
    with pytest.raises(ValueError, match="slot names window"):
        ops.volume_joint_multistep_sde(y[:-1].contiguous(), slot, taps, x, prev, *ok)
    with pytest.raises(ValueError, match="lattice"):
        ops.volume_joint_multistep_sde(y, slot, taps, x, prev, 1.0, 0.5, -0.25, 0.5, -1.0, 1.0, 1, 5, 0, 1)
    with pytest.raises(ValueError, match="clamp_mode"):
        ops.volume_joint_multistep_sde(y, slot, taps, x, prev, 1.0, 0.5, -0.25, 0.5, -1.0, 1.0, 2, 8, 0, 1)
    with pytest.raises(ValueError, match="draw"):
        ops.volume_joint_multistep_sde(y, slot, taps, x, prev, 1.0, 0.5, -0.25, 0.5, -1.0, 1.0, 1, 8, 0, 1 << 32)
    with pytest.raises(ValueError, match="cubic"):
        ops.volume_joint_multistep_sde(y[:, :, :, :4].contiguous(), slot, taps, x, prev, *ok)
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.volume_joint_multistep_sde(y, slot, taps, x.transpose(0, 1), prev, *ok)
    with pytest.raises(ValueError, match="x0_prev"):
        ops.volume_joint_multistep_sde(y, slot, taps, x, prev[:-1].contiguous(), *ok)
    with pytest.raises(ValueError, match="x0_out"):
        ops.volume_joint_multistep_sde(y, slot, taps, x, prev, *ok, x0_out=prev[:-1].contiguous())


# ---- G3: sample(sampler='dpmpp2m') against the float64 loop ------------------------------------------------------------------------------------
SHAPE = (2, 1, 8, 8, 8)


@pytest.fixture(scope="module")
def draws():
    """The low-res windows and K + 2 normals: low-res augmentation noise, initial image, one per step (read only)."""
    g = torch.Generator().manual_seed(7)
    return torch.randn(SHAPE, generator=g).clamp(-1, 1), [torch.randn(SHAPE, generator=g) for _ in range(K + 2)]


def sample_kw(lowres, **kw):
    return dict(batch_size=SHAPE[0], video_frames=8, start_image_or_video=lowres.to(DEV), start_at_unet_number=2, use_tqdm=False, **kw)


def n_draws(eta):
    """Low-res noise and the initial image, then one per step whose kn != 0: every step but the last under eta > 0."""
    return 2 + (K - 1 if eta > 0 else 0)


def window_reference(elu, net, lowres, noise, eta, dynamic, self_cond=False):
    """The float64 loop on the product's own fp32 table: (image, largest |state|, tables)."""
    den = elu.window_denoiser(sampler='dpmpp2m', eta=eta)
    tabs = E.tables(HN.HP, eta, coefs=den.coefs.numpy())
    alpha, sigma_lr = tabs['lowres']
    low = alpha * lowres.numpy().astype(np.float64) + sigma_lr * noise[0].numpy().astype(np.float64)
    img, state_max = E.window_loop(net, noise[1].numpy(), low, tabs, dynamic, [n.numpy() for n in noise[2:]], self_cond)
    return img, state_max, tabs, float(np.abs(low).max())


@pytest.mark.parametrize('self_cond', [False, True], ids=['plain', 'self-cond'])
@pytest.mark.parametrize('eta', list(E.ETAS))
@pytest.mark.parametrize('dynamic', [False, True], ids=['static', 'dynamic'])
def test_sample_matches_the_float64_loop(draws, dynamic, eta, self_cond):
    lowres, noise = draws
    eta = E.ETAS[eta]
    elu = HN.make_elucidated('churn-on', dynamic, self_cond=self_cond, size=8).to(DEV)
    used = noise[:n_draws(eta)]
    got = elu.sample(**sample_kw(lowres, noise=[n.clone() for n in used], sampler='dpmpp2m', eta=eta)).cpu().numpy()
    want, state_max, tabs, low_max = window_reference(elu, HN.stub64, lowres, noise, eta, dynamic, self_cond)
    bound = E.chain_bound(tabs, 0, state_max, low_max, dynamic, self_cond)
    err = np.abs(got.astype(np.float64) - want).max()
    print(f"sample dpmpp2m {'dynamic' if dynamic else 'static'} eta {eta} self_cond {self_cond}: max err {err:.3e}, bound {bound:.3e}, "
          f"largest |state| {state_max:.2f}")
    assert got.shape == SHAPE and np.isfinite(got).all() and np.ptp(want) > 1.0
    assert err <= bound


def test_noise_sources_and_the_draws_consumed(draws):
    lowres, noise = draws
    elu = HN.make_elucidated('churn-on', False, size=8).to(DEV)
    for eta in E.ETAS.values():
        seen = []

        def source(shape):
            seen.append(tuple(shape))
            return noise[len(seen) - 1].to(DEV)
        a = elu.sample(**sample_kw(lowres, noise=source, sampler='dpmpp2m', eta=eta))
        assert seen == [SHAPE] * n_draws(eta)                                   # low-res noise, initial image, one per kn != 0
        given = [n.clone() for n in noise[:n_draws(eta)]] + [torch.full(SHAPE, float('nan'))]
        b = elu.sample(**sample_kw(lowres, noise=given, sampler='dpmpp2m', eta=eta))
        assert torch.equal(a, b) and torch.isfinite(a).all() and a.unique().numel() > 500
    ode = elu.sample(**sample_kw(lowres, noise=[n.clone() for n in noise], sampler='dpmpp2m'))
    sde = elu.sample(**sample_kw(lowres, noise=[n.clone() for n in noise], sampler='dpmpp2m', eta=1.0))
    more = elu.sample(**sample_kw(lowres, noise=[n.clone() for n in noise], sampler='dpmpp2m', sample_steps=6))
    assert not torch.equal(ode, sde) and not torch.equal(ode, more)


def test_heun_keyword_is_the_default_path(draws):
    lowres, noise = draws
    elu = HN.make_elucidated('churn-on', True, self_cond=True, size=8).to(DEV)
    a = elu.sample(**sample_kw(lowres, noise=[n.clone() for n in noise]))
    b = elu.sample(**sample_kw(lowres, noise=[n.clone() for n in noise], sampler='heun'))
    c = elu.sample(**sample_kw(lowres, noise=[n.clone() for n in noise], sampler='dpmpp2m', eta=1.0))
    assert torch.equal(a, b) and a.unique().numel() > 500 and not torch.equal(a, c)


def conv3d_edm(dynamic=False):
    """The tiny true-Conv3d U-Net under ``ElucidatedImagen`` and its float64 oracle (oracle/iqt_oracle.py on the same weights)."""
    from oracle import iqt_oracle as O
    from diffusioniqt_amd.elucidated_imagen import ElucidatedImagen
    from diffusioniqt_amd.imagen_pytorch3D import NullUnet, SRUnet256
    kwa = json.loads(str(load_golden('unetA_tiny')['kwargs']))
    elu = ElucidatedImagen(unets=(NullUnet(), SRUnet256(**kwa)), image_sizes=(8, 8), channels=1, condition_on_text=False,
                           auto_normalize_img=False, cond_drop_prob=0.0, dynamic_thresholding=dynamic,
                           dynamic_thresholding_percentile=HN.PERCENTILE, **HN.HP)
    sd = O.hash_fill_state_dict(elu.unets[1].state_dict(), 0)
    elu.unets[1].load_state_dict(sd)
    sd64, cfg = {k: v.double() for k, v in sd.items()}, O.unet_config(**kwa)

    def net(x, lowres, c_noise, self_cond=None):
        with torch.no_grad():
            return O.unet_forward(sd64, cfg, torch.from_numpy(x), None, torch.from_numpy(c_noise),
                                  lowres_cond_img=torch.from_numpy(lowres)).numpy()
    return elu.to(DEV), net


def unet3d_edm(dynamic=False):
    """The tiny ``Unet3D`` of the Heun tests and its oracle (oracle/iqt_oracle_b.py, which computes in fp32) on the same weights."""
    from oracle import iqt_oracle as O
    from oracle import iqt_oracle_b as OB
    from diffusioniqt_amd.elucidated_imagen import ElucidatedImagen
    from diffusioniqt_amd.imagen_video import Unet3D
    kw = {k: (tuple(v) if isinstance(v, list) else v) for k, v in json.loads(str(load_golden('unet3d_tiny')['kwargs'])).items()}
    base = Unet3D(**{**kw, 'lowres_cond': False, 'dim_mults': (1, 2), 'layer_attns': False})
    elu = ElucidatedImagen(unets=(base, Unet3D(**kw)), image_sizes=(8, 8), channels=1, condition_on_text=False, auto_normalize_img=False,
                           cond_drop_prob=0.0, dynamic_thresholding=dynamic, dynamic_thresholding_percentile=HN.PERCENTILE, **HN.HP)
    sd = O.hash_fill_state_dict(elu.unets[1].state_dict(), 11)
    elu.unets[1].load_state_dict(sd)
    cfg = OB.unet3d_config(**kw)

    def net(x, lowres, c_noise, self_cond=None):
        f = lambda a: torch.from_numpy(np.asarray(a)).float()
        with torch.no_grad():
            return OB.unet3d_forward(sd, cfg, f(x), f(c_noise), lowres_cond_img=f(lowres),
                                     lowres_noise_times=torch.full((x.shape[0],), float(HN.LOWRES_LEVEL))).double().numpy()
    return elu.to(DEV), net


@pytest.mark.parametrize('eta', list(E.ETAS))
@pytest.mark.parametrize('dynamic', [False, True], ids=['static', 'dynamic'])
@pytest.mark.parametrize('make', [conv3d_edm, unet3d_edm], ids=['conv3d-unet', 'unet3d'])
def test_sample_with_a_real_network_matches_the_oracle_driven_loop(draws, make, dynamic, eta):
    """The float64 loop of the specification around the oracle network, against ``sample`` on the product network with the same
    weights; the tolerance is the module docstring's."""
    lowres, noise = draws
    eta = E.ETAS[eta]
    elu, net = make(dynamic)
    got = elu.sample(**sample_kw(lowres, noise=[n.clone() for n in noise[:n_draws(eta)]], sampler='dpmpp2m', eta=eta)).cpu().numpy()
    want, state_max, _, _ = window_reference(elu, net, lowres, noise, eta, dynamic)
    err = np.abs(got.astype(np.float64) - want)
    print(f"sample dpmpp2m {make.__name__} {'dynamic' if dynamic else 'static'} eta {eta}: max err {err.max():.3e}, "
          f"share above 2e-4 {(err > 2e-4).mean():.4f}, "
          f"largest |state| {state_max:.2f}")
    assert np.ptp(want) > 0.5
    assert err.max() <= 5e-3 and (err > 2e-4).mean() < 0.03


# ---- G4: the joint chain -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shared_vol():
    return torch.from_numpy(R.shared_volume()).to(DEV)


def joint_run(elu, cfg, blend, eta, den=None, **kw):
    from diffusioniqt_amd.inference import VolumeInference
    den = den if den is not None else elu.window_denoiser(sampler='dpmpp2m', eta=eta)
    assert den.multistep and not den.heun and den.num_steps == K
    return VolumeInference(cfg, den, blend=blend, noise='anchored', joint=True, seed=kw.pop('seed', E.SEED), **kw)


def independent_run(sample, cfg, blend, P, eta, **kw):
    """Every window's own chain through ``sample(sampler='dpmpp2m', noise=source)``, finished patches blended."""
    from diffusioniqt_amd.inference import VolumeInference

    def sample_fn(x, noise=None):
        return sample(batch_size=x.shape[0], video_frames=P, start_image_or_video=x, start_at_unet_number=2, noise=noise,
                      sampler='dpmpp2m', eta=eta)
    return VolumeInference(cfg, sample_fn, blend=blend, noise='anchored', seed=kw.pop('seed', E.SEED), **kw)


def chain_ref(elu, vol_name, stride, dynamic, eta, blend, samples=1, self_cond=False):
    vol, cfg = (R.block_volume(), R.block_cfg()) if vol_name == 'block' else (R.shared_volume(), R.shared_cfg(stride))
    coefs = elu.window_denoiser(sampler='dpmpp2m', eta=eta).coefs.numpy()
    return _ref((vol_name, stride, dynamic, eta, blend, samples, self_cond), lambda: E.joint_reference(
        vol, cfg, E.tables(HN.HP, eta, coefs=coefs), blend, dynamic, samples=samples, self_cond=self_cond))


def check(got, ref, what, key='mean', factor=1):
    got = got.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == ref[key].shape and np.isfinite(got).all()
    bound = factor * ref['bound']
    err = np.abs(got.astype(np.float64) - ref[key]).max()
    print(f"{what}: max |{key} - ref| = {err:.3e}, bound {bound:.3e} (n = {ref['windows_per_voxel']}, largest |state| {ref['state_max']:.2f})")
    assert err <= bound, what
    return got


@pytest.mark.parametrize('eta', list(E.ETAS))
@pytest.mark.parametrize('dynamic', [False, True], ids=['static', 'dynamic'])
def test_joint_at_stride_equal_patch_is_the_independent_path(shared_vol, dynamic, eta):
    """No overlap, unit weights: num / den is exact, every window's chain is its own, and both paths take the same ``__device__`` update
    -- the joint volume equals the blended independent windows at every voxel, bit for bit."""
    eta = E.ETAS[eta]
    elu = HN.make_elucidated('churn-on', dynamic, self_cond=True).to(DEV)
    cfg = R.shared_cfg(16)
    independent = independent_run(lambda **k: elu.sample(use_tqdm=False, **k), cfg, 'constant', 16, eta)(shared_vol)
    joint = joint_run(elu, cfg, 'constant', eta)(shared_vol)
    assert independent.unique().numel() > 1000
    assert torch.equal(joint, independent)


@pytest.mark.parametrize('eta', list(E.ETAS))
def test_joint_tie_with_the_conv3d_unet_through_the_trainer(eta):
    """``ImagenTrainer.window_denoiser(sampler='dpmpp2m')``: the tie at stride = patch, then overlapping windows -- finite, identical on a
    second run, and not what blending finished patches gives."""
    from diffusioniqt_amd.trainer import ImagenTrainer
    eta = E.ETAS[eta]
    elu, _ = conv3d_edm()
    configs = {'Data': {'norm': 'z-score'}, 'Train': {'batch_sample': False, 'patch_size_sub': 8, 'pred_obj': 'x_start'}, 'Eval': {'repeat': 1}}
    ImagenTrainer.locked = False
    trainer = ImagenTrainer(configs=configs, imagen=elu, verbose=False)
    vol = torch.from_numpy(np.random.default_rng(12).integers(1, 1000, (20, 24, 28)).astype(np.float32)).to(DEV)   # every window is kept
    cfg = lambda stride, batch: R.shared_cfg(stride, batch_size=batch, P=8)
    den = trainer.window_denoiser(sampler='dpmpp2m', eta=eta)
    independent = independent_run(trainer.sample, cfg(8, 6), 'constant', 8, eta, seed=4)(vol)
    joint = joint_run(elu, cfg(8, 6), 'constant', eta, den=den, seed=4)(vol)
    assert torch.equal(joint, independent) and joint.unique().numel() > 1000
    runs = [joint_run(elu, cfg(4, 30), 'gaussian', eta, den=den, seed=4)(vol) for _ in range(2)]
    assert torch.isfinite(runs[0]).all() and torch.equal(runs[0], runs[1])
    blended = independent_run(trainer.sample, cfg(4, 30), 'gaussian', 8, eta, seed=4)(vol)
    assert not torch.equal(runs[0], blended)


@pytest.mark.parametrize('tiling', [(8, 'gaussian'), (5, 'gaussian')], ids=['s8-gaussian', 's5-gaussian'])
@pytest.mark.parametrize('eta', list(E.ETAS))
@pytest.mark.parametrize('dynamic', [False, True], ids=['static', 'dynamic'])
def test_joint_chain_matches_the_float64_reference(shared_vol, dynamic, eta, tiling):
    """Overlapping windows, Gaussian taps, two samples, self-conditioning: mean and deviation within the chain bound (the deviation is
    allowed twice it, as in ``volume_blend_reference.tolerance``), and the deviation is non-zero only where windows cover."""
    (stride, blend), eta = tiling, E.ETAS[eta]
    elu = HN.make_elucidated('churn-on', dynamic, self_cond=True).to(DEV)
    ref = chain_ref(elu, 'shared', stride, dynamic, eta, blend, samples=2, self_cond=True)
    inf = joint_run(elu, R.shared_cfg(stride), blend, eta, samples=2)
    mean, std = inf(shared_vol, return_std=True)
    what = f"joint dpmpp2m {'dynamic' if dynamic else 'static'} eta {eta} stride {stride} {blend} S = 2"
    got = check(mean, ref, what + " mean")
    std = check(std, ref, what + " deviation", key='std', factor=2)
    assert (got[~ref['covered'] & ~ref['background']] == ref['fill']).all() and (got[ref['background']] == ref['min_val']).all()
    live = ref['covered'] & ~ref['background']
    assert ref['std'][live].max() > 0.05 and std[live].max() > 0.05 and not std[~live].any()


def test_joint_batching_and_seed(shared_vol):
    elu = HN.make_elucidated('churn-on', False).to(DEV)
    a = joint_run(elu, R.shared_cfg(5, batch_size=7), 'gaussian', 1.0)(shared_vol)
    b = joint_run(elu, R.shared_cfg(5, batch_size=3), 'gaussian', 1.0)(shared_vol)
    assert torch.equal(a, b)
    c = joint_run(elu, R.shared_cfg(5, batch_size=3), 'gaussian', 1.0, seed=E.SEED + 1)(shared_vol)
    assert not torch.equal(b, c)                                                # another seed is another volume
    d = joint_run(elu, R.shared_cfg(5, batch_size=3), 'gaussian', 0.0)(shared_vol)
    assert not torch.equal(b, d)                                                # and the SDE is not the ODE


@pytest.mark.parametrize('eta', list(E.ETAS))
def test_joint_block_mode_matches_the_float64_reference(eta):
    eta = E.ETAS[eta]
    elu = HN.make_elucidated('churn-on', False, self_cond=True, size=8).to(DEV)
    ref = chain_ref(elu, 'block', None, False, eta, 'gaussian', self_cond=True)
    assert ref['kept'] == ref['candidates'] == 27 and ref['covered'].all()
    vol = torch.from_numpy(R.block_volume()).to(DEV)
    check(joint_run(elu, R.block_cfg(), 'gaussian', eta)(vol), ref, f"joint dpmpp2m eta {eta} block mode P 24 stride 16")
