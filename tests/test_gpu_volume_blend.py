"""Blend modes of the whole-volume inference on the device against the float64 specification (tests/volume_blend_reference.py).

Tolerance (derived, see ``volume_blend_reference.tolerance``): a blended voxel is a ratio of two fp32 sums of at most
n = ceil(P / stride)^3 non-negative-weight terms, so |b - b64| <= (n + 3) 2^-23 max|y|; the deviation map gets twice that at S = 3.
A missed window or a wrong weight moves a voxel by about 1e-1, four orders of magnitude above the bound.  Every voxel is compared."""
import numpy as np
import pytest
import torch

from tests import volume_blend_reference as R

pytestmark = pytest.mark.gpu

_REF = {}


def _ref(key, make):
    """One float64 reference per case, shared by the tests that need it and never modified."""
    if key not in _REF:
        _REF[key] = make()
        for v in _REF[key].values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return _REF[key]


def _shared_ref(stride, kind, samples):
    return _ref(('shared', stride, kind, samples),
                lambda: R.reference(R.shared_volume(), R.shared_cfg(stride), R.make_sampler(samples), samples=samples, blend=kind))


def _check_mean(got, ref, what):
    got = got.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == ref['mean'].shape
    tol = R.tolerance(ref['windows_per_voxel'], ref['max_abs_y'])
    err = np.abs(got.astype(np.float64) - ref['mean'])
    print(f"{what}: max |mean - ref| = {err.max():.3e}, bound {tol:.3e} (n = {ref['windows_per_voxel']}, max|y| = {ref['max_abs_y']:.4f})")
    assert err.max() <= tol, what
    assert (got[~ref['covered'] & ~ref['background']] == ref['fill']).all(), f'{what}: uncovered voxels must hold the fill value'
    assert (got[ref['background']] == ref['min_val']).all(), f'{what}: background voxels must hold min_val'
    return tol


@pytest.mark.parametrize("kind", ['gaussian', 'constant'])
@pytest.mark.parametrize("stride", [8, 5])
def test_blended_mean_matches_reference(stride, kind):
    from diffusioniqt_amd.inference import VolumeInference
    ref = _shared_ref(stride, kind, 1)
    assert (~ref['covered']).any() and ref['background'].any() and ref['kept'] < ref['candidates']
    vol = torch.from_numpy(R.shared_volume()).cuda()
    got = VolumeInference(R.shared_cfg(stride), R.make_sampler(1), blend=kind)(vol)
    _check_mean(got, ref, f'stride {stride} {kind}')


def test_blended_block_mode_matches_reference():
    from diffusioniqt_amd.inference import VolumeInference
    ref = _ref('block', lambda: R.reference(R.block_volume(), R.block_cfg(), R.make_sampler(1), blend='gaussian'))
    assert ref['kept'] == ref['candidates'] == 27 and ref['covered'].all()
    vol = torch.from_numpy(R.block_volume()).cuda()
    got = VolumeInference(R.block_cfg(), R.make_sampler(1), blend='gaussian')(vol)
    _check_mean(got, ref, 'block mode P 24 stride 16')


def test_three_samples_mean_and_std_match_reference():
    from diffusioniqt_amd.inference import VolumeInference
    ref = _shared_ref(8, 'gaussian', 3)
    vol = torch.from_numpy(R.shared_volume()).cuda()
    inf = VolumeInference(R.shared_cfg(8), R.make_sampler(3), blend='gaussian', samples=3)
    mean, std = inf(vol, return_std=True)
    tol = _check_mean(mean, ref, 'stride 8 gaussian S=3')
    std = std.cpu().numpy()
    err = np.abs(std.astype(np.float64) - ref['std'])
    print(f"S=3: max |std - ref| = {err.max():.3e}, bound {2 * tol:.3e}; largest std {ref['std'].max():.4f}")
    assert ref['std'].max() > 0.1
    assert err.max() <= 2 * tol
    assert not std[~ref['covered'] | ref['background']].any(), 'std must be exactly 0 on uncovered and background voxels'
    inf = VolumeInference(R.shared_cfg(8), R.make_sampler(3), blend='gaussian', samples=3)
    assert torch.equal(inf(vol), mean), 'the mean alone is the same volume'


def test_blend_is_deterministic_and_independent_of_batching():
    from diffusioniqt_amd.inference import VolumeInference
    vol = torch.from_numpy(R.shared_volume()).cuda()
    runs = []
    for batch in (7, 7, 1):
        inf = VolumeInference(R.shared_cfg(5, batch_size=batch), R.make_window_sampler(2), blend='gaussian', samples=2)
        runs.append(inf(vol, return_std=True))
    for m, s in runs[1:]:
        assert torch.equal(m, runs[0][0]) and torch.equal(s, runs[0][1])
    ref = _ref('window', lambda: R.reference(R.shared_volume(), R.shared_cfg(5), R.make_window_sampler(2), samples=2))
    _check_mean(runs[0][0], ref, 'stride 5 gaussian S=2, per-window sampler')


def test_non_overlapping_constant_blend_equals_plain_placement():
    """Degenerate overlap (stride = P): one term of weight 1 per voxel, (1 y) / 1 = y -- bit-identical to the default path."""
    from diffusioniqt_amd.inference import VolumeInference
    rng = np.random.default_rng(3)
    v = rng.integers(0, 1000, (64, 64, 64)).astype(np.float32)
    v[:, :32, 32:] = 0                                                  # some windows are rejected, and zeros make background
    vol = torch.from_numpy(v).cuda()
    cfg = R.shared_cfg(32, batch_size=3, P=32)
    sampler = lambda x: x * 0.5 + 0.25
    plain = VolumeInference(cfg, sampler)(vol)
    blended = VolumeInference(cfg, sampler, blend='constant')(vol)
    assert torch.equal(plain, blended)
    assert plain.unique().numel() > 3


def test_ops_volume_blend_against_reference_accumulation():
    """The C ABI apart from the Python class: a hand-made slot table with interior holes, two samples."""
    from diffusioniqt_amd import ops
    rng = np.random.default_rng(4)
    shape, P, stride = (25, 22, 70), 8, 3                               # W spans two 64-voxel workgroups; stride does not divide P
    lattice = tuple(len(range(0, s - P + 1, stride)) for s in shape)
    slot = np.full(lattice, -1, dtype=np.int32)
    keep = rng.random(lattice) < 0.7
    keep[2, 2, 5:9] = False                                             # interior holes
    keep[:, :, -1] = False
    N = int(keep.sum())
    slot[keep] = rng.permutation(N).astype(np.int32)                    # any row order
    patches = rng.standard_normal((2, N, P, P, P)).astype(np.float32)
    taps = rng.uniform(0.25, 1.0, P).astype(np.float32)
    vol = rng.integers(0, 5, shape).astype(np.float32)                  # a fifth of the voxels is background (raw 0 = the minimum)
    mean, std = np.float32(2.0), np.float32(1.5)
    min_val, fill = (np.float32(0.) - mean) / std, np.float32(-7.25)
    want_m, want_s, covered, background = R.blend_accumulate(patches, slot, taps, stride, shape, vol, mean, std, min_val, fill)
    assert (~covered).any() and background.any() and (covered & ~background).any()
    cu = lambda a: torch.from_numpy(a).cuda()
    got_m, got_s = ops.volume_blend(cu(patches), cu(slot), cu(taps), cu(vol), float(mean), float(std), float(min_val), float(fill),
                                    stride, True)
    got_m, got_s = got_m.cpu().numpy(), got_s.cpu().numpy()
    tol = R.tolerance(-(-P // stride) ** 3, float(np.abs(patches).max()))
    em, es = np.abs(got_m - want_m).max(), np.abs(got_s - want_s).max()
    print(f"ops.volume_blend: max |mean - ref| = {em:.3e} (bound {tol:.3e}), max |std - ref| = {es:.3e} (bound {2 * tol:.3e})")
    assert em <= tol and es <= 2 * tol
    assert (got_m[~covered & ~background] == fill).all() and (got_m[background] == min_val).all()
    assert not got_s[~covered | background].any()
    only_m, none = ops.volume_blend(cu(patches[:1].copy()), cu(slot), cu(taps), cu(vol), float(mean), float(std), float(min_val),
                                    float(fill), stride, False)
    assert none is None
    want_1 = R.blend_accumulate(patches[:1], slot, taps, stride, shape, vol, mean, std, min_val, fill)[0]
    assert np.abs(only_m.cpu().numpy() - want_1).max() <= tol
    with pytest.raises(ValueError, match="slot"):
        bad = slot.copy()
        bad[0, 0, 0] = N
        ops.volume_blend(cu(patches), cu(bad), cu(taps), cu(vol), 2.0, 1.5, float(min_val), float(fill), stride, False)
