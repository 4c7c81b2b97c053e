"""``ops.anchored_noise`` (diqt_anchored_noise) on a real MI355X against the numpy specification of tests/anchored_noise_reference.py:
raw Philox words bit for bit (also past 2^32 voxels), the normals against the float64 Box-Muller transform of the same bits, window
overlap and block-mode consistency on the device, and ``VolumeInference(noise='anchored')`` end to end with a "sampler" that returns
its first draw, so the stitched volume must BE the reference field."""
import numpy as np
import pytest
import torch

from tests import anchored_noise_reference as A
from tests import volume_blend_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"

SHAPE, P = (20, 24, 28), 8                         # non-cubic: an axis mix-up shows
ORIGINS = np.array([(0, 0, 0), (12, 16, 20), (3, 5, 7), (3, 5, 9)], dtype=np.int32)      # corner, far corner, two that overlap
SEED, DRAW, SAMPLE = 0x123456789, 3, 2             # a seed above 2^32


@pytest.fixture(scope="module")
def spec():
    """The reference field of the small volume, two channels: bits [2,D,H,W,2] and float64 normals [2,D,H,W] (read only)."""
    bits = A.field(SHAPE, 2, SEED, DRAW, SAMPLE)
    return bits, A.normals(bits)


def _cut(field, C):
    return np.stack([A.window(field[:C], tuple(o), P) for o in ORIGINS])


@pytest.mark.parametrize('C', [1, 2])
def test_raw_bits_equal_the_reference(spec, C):
    from diffusioniqt_amd import ops
    got = ops.anchored_noise(ORIGINS, C, P, *SHAPE, SEED, draw=DRAW, sample=SAMPLE, raw=True)
    assert got.dtype == torch.int32 and tuple(got.shape) == (4, C, P, P, P, 2) and got.is_contiguous()
    assert np.array_equal(got.cpu().numpy().view(np.uint32), _cut(spec[0], C))


def test_raw_bits_past_two_to_the_32_voxels():
    from diffusioniqt_amd import ops
    shape, origin = (2048, 2048, 2048), (2040, 2040, 2040)
    got = ops.anchored_noise(np.array([origin], dtype=np.int32), 1, 8, *shape, SEED, draw=DRAW, sample=SAMPLE, raw=True)
    ref = A.field_at(A.window_lin(shape, origin, 8), SEED, DRAW, SAMPLE)
    assert np.array_equal(got.cpu().numpy().view(np.uint32)[0], ref)


@pytest.mark.parametrize('C', [1, 2])
def test_normals_match_the_float64_transform(spec, C):
    """u1, u2 are exact; r = sqrt(-2 ln u1) <= 5.8 carries a relative error of a few 2^-24 from logf / sqrtf, cospif(2 u2) a few ulp
    absolute on an exact argument: the product is within 5e-6, the bound leaves 4x."""
    from diffusioniqt_amd import ops
    got = ops.anchored_noise(ORIGINS, C, P, *SHAPE, SEED, draw=DRAW, sample=SAMPLE)
    assert got.dtype == torch.float32 and tuple(got.shape) == (4, C, P, P, P)
    err = np.abs(got.cpu().numpy().astype(np.float64) - _cut(spec[1], C)).max()
    print(f"anchored normals, C = {C}: max |n - n64| = {err:.3e}")
    assert err <= 2e-5


def test_overlapping_windows_agree_on_the_device():
    from diffusioniqt_amd import ops
    for raw in (True, False):
        got = ops.anchored_noise(ORIGINS, 1, P, *SHAPE, SEED, draw=DRAW, sample=SAMPLE, raw=raw)
        assert torch.equal(got[2, :, :, :, 2:], got[3, :, :, :, :6])          # (3,5,7) and (3,5,9): x in [9, 15)
        assert not torch.equal(got[2], got[3])
    alone = ops.anchored_noise(ORIGINS[3:], 1, P, *SHAPE, SEED, draw=DRAW, sample=SAMPLE)
    assert torch.equal(alone[0], got[3])                                       # nor on the batch a window comes in


def test_block_mode_sub_volumes_tile_the_window():
    """f = 3, A = 8: merging the noise of the 27 sub-volume origins gives the noise of the 24^3 window itself."""
    from diffusioniqt_amd import ops
    from diffusioniqt_amd.inference import sub_volume_origins
    from diffusioniqt_amd.utils_mine import merge_sub_volumes
    shape, origin = (30, 32, 34), (5, 7, 9)
    whole = ops.anchored_noise(np.array([origin], dtype=np.int32), 1, 24, *shape, SEED, draw=1, sample=0)
    sub = ops.anchored_noise(sub_volume_origins(origin, 3, 8), 1, 8, *shape, SEED, draw=1, sample=0)
    assert tuple(sub.shape) == (27, 1, 8, 8, 8)
    assert torch.equal(merge_sub_volumes(sub, original_shape=(1, 1, 24, 24, 24)), whole)


def test_block_mode_volume_inference_hands_out_the_sub_volume_origins():
    """Block mode end to end (f = 3, sub-volumes of 8, windows of 24): the stitched first draw is the field."""
    from diffusioniqt_amd.inference import VolumeInference
    vol = R.block_volume()
    got = VolumeInference(R.block_cfg(), first_draw, blend='constant', noise='anchored', seed=5)(torch.from_numpy(vol).to(DEV))
    ref = A.normals(A.field(vol.shape, 1, 5, 0, 0))[0]
    tol = 2e-5 + R.tolerance(8, np.abs(ref).max())                           # ceil(24 / 16)^3 windows per voxel
    mask = vol != vol.min()                                                  # stride 16 covers all 56 voxels of an axis; the minimum is background
    assert mask.mean() > 0.99
    assert np.abs(got.cpu().numpy().astype(np.float64) - ref)[mask].max() <= tol


# ---- end to end: VolumeInference with a sampler that returns its first draw ---------------------------------------------------------------
SEED_E = 11


def first_draw(x, noise):
    return noise(x.shape)


def device_field(shape, sample):
    """The device's own normals of the whole [D,H,W] field (draw 0), assembled from 4^3 windows on the lattice of multiples of 4."""
    from diffusioniqt_amd import ops
    g = [s // 4 for s in shape]
    org = np.array([(4 * a, 4 * b, 4 * c) for a in range(g[0]) for b in range(g[1]) for c in range(g[2])], dtype=np.int32)
    w = ops.anchored_noise(org, 1, 4, *shape, SEED_E, draw=0, sample=sample).cpu().numpy()
    return w.reshape(g[0], g[1], g[2], 4, 4, 4).transpose(0, 3, 1, 4, 2, 5).reshape(shape)


@pytest.fixture(scope="module")
def shared():
    """The shared volume of the blend tests on the device; per sample 0 / 1 the float64 normals of its field and the device's own fp32
    field; per stride the voxels the crop-and-overwrite stitching writes, the voxels a kept window covers (both without the
    background) and the windows per voxel (read only)."""
    from diffusioniqt_amd.inference import crop_margins
    vol = R.shared_volume()
    f64 = [A.normals(A.field(vol.shape, 1, SEED_E, 0, s))[0] for s in (0, 1)]
    f32 = [device_field(vol.shape, s) for s in (0, 1)]
    masks = {}
    for stride in (8, 5):
        ref = R.reference(vol, R.shared_cfg(stride), lambda x: x, blend='constant')
        org, _ = R.origins_of(vol.shape, 16, stride)
        kept = org[[np.count_nonzero(vol[i:i + 16, j:j + 16, k:k + 16]) / 16.0 ** 3 >= 0.05 for i, j, k in org]]
        written = np.zeros(vol.shape, dtype=bool)
        for (i, j, k), m in zip(kept, crop_margins(kept, vol.shape, 16, stride)):
            written[i + m[0]:i + 16 - m[1], j + m[2]:j + 16 - m[3], k + m[4]:k + 16 - m[5]] = True
        masks[stride] = written & ~ref['background'], ref['covered'] & ~ref['background'], ref['windows_per_voxel']
        assert masks[stride][0].any() and masks[stride][1].any()
    return torch.from_numpy(vol).to(DEV), f64, f32, masks


def test_device_field_is_the_reference_field(shared):
    _, f64, f32, _ = shared
    for a, b in zip(f64, f32):
        assert np.abs(a - b).max() <= 2e-5


@pytest.mark.parametrize('stride', [8, 5])
def test_volume_inference_stitches_the_field_itself(shared, stride):
    from diffusioniqt_amd.inference import VolumeInference
    vol, f64, f32, masks = shared
    written, covered, n = masks[stride]
    got = VolumeInference(R.shared_cfg(stride), first_draw, noise='anchored', seed=SEED_E)(vol).cpu().numpy()
    # crop-and-overwrite: whichever window wrote a voxel last, it wrote the field's value there, bit for bit
    assert np.array_equal(got[written], f32[0][written])
    for blend in ('constant', 'gaussian'):
        b = VolumeInference(R.shared_cfg(stride), first_draw, blend=blend, noise='anchored', seed=SEED_E)(vol).cpu().numpy()
        tol = R.tolerance(n, np.abs(f32[0][covered]).max())                   # a weighted mean of equal numbers is that number
        err = np.abs(b.astype(np.float64) - f32[0].astype(np.float64))[covered].max()
        print(f"stride {stride}, blend {blend}: max |blend - field| = {err:.3e} (tolerance {tol:.3e})")
        assert err <= tol


def test_volume_inference_does_not_depend_on_the_batch_size(shared):
    from diffusioniqt_amd.inference import VolumeInference
    vol = shared[0]
    for blend in (None, 'gaussian'):
        a = VolumeInference(R.shared_cfg(5, batch_size=7), first_draw, blend=blend, noise='anchored', seed=SEED_E)(vol)
        b = VolumeInference(R.shared_cfg(5, batch_size=3), first_draw, blend=blend, noise='anchored', seed=SEED_E)(vol)
        assert torch.equal(a, b), blend
    c = VolumeInference(R.shared_cfg(5, batch_size=3), first_draw, blend='gaussian', noise='anchored', seed=SEED_E + 1)(vol)
    assert not torch.equal(b, c)                                               # another seed is another field


def test_volume_inference_samples_are_the_fields_of_their_index(shared):
    """samples = 2: the blended mean is (f0 + f1) / 2 and the unbiased deviation |f0 - f1| / sqrt(2) -- which pins the two samples to the
    fields of sample 0 and sample 1.  Each blended sample is within ``tolerance`` of its field; the deviation map is allowed twice that
    (volume_blend_reference.tolerance)."""
    from diffusioniqt_amd.inference import VolumeInference
    vol, f64, f32, masks = shared
    _, covered, n = masks[8]
    inf = VolumeInference(R.shared_cfg(8), first_draw, blend='constant', samples=2, noise='anchored', seed=SEED_E)
    mean, std = (t.cpu().numpy().astype(np.float64) for t in inf(vol, return_std=True))
    assert (std[covered] > 0).mean() > 0.99
    f0, f1 = (f.astype(np.float64) for f in f32)
    tol = R.tolerance(n, max(np.abs(f0[covered]).max(), np.abs(f1[covered]).max()))
    assert np.abs(mean - 0.5 * (f0 + f1))[covered].max() <= tol
    assert np.abs(std - np.abs(f0 - f1) / np.sqrt(2.0))[covered].max() <= 2 * tol


def test_volume_inference_rank_shards_see_one_field(shared):
    """``patch_slice``: the windows of two ranks, merged, are the single-rank result -- anchoring makes rank sharding noise-consistent."""
    from diffusioniqt_amd.inference import VolumeInference
    vol = shared[0]
    inf = VolumeInference(R.shared_cfg(16), first_draw, noise='anchored', seed=SEED_E)      # stride = patch: every voxel has one owner
    full, a, b = inf(vol), inf(vol, patch_slice=(0, 2)), inf(vol, patch_slice=(1, 2))
    fill = float((np.float32(0.) - np.float32(300.0)) / np.float32(200.0))
    assert not torch.equal(a, full) and not torch.equal(b, full)
    assert torch.equal(torch.where(a != fill, a, b), full)
