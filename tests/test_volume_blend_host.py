"""Blend modes of the whole-volume inference, the part that needs no GPU: the taps, the float64 specification itself
(tests/volume_blend_reference.py), argument validation before any device use, and the error codes of ``diqt_volume_blend``."""
import numpy as np
import pytest
import torch

from tests import volume_blend_reference as R


@pytest.mark.parametrize("P", [16, 24, 31, 32])
def test_blend_taps(P):
    from diffusioniqt_amd.inference import blend_taps
    t = blend_taps(P, 'gaussian', 0.125)
    assert t.dtype == np.float32 and t.shape == (P,)
    assert np.array_equal(t, t[::-1])
    assert t.max() == np.float32(1.0) and (t > 0).all()
    assert np.array_equal(t.astype(np.float64), R.taps_of(P, 'gaussian', 0.125))
    i = np.arange(P, dtype=np.float64)
    want = np.exp(-(i - (P - 1) / 2.0) ** 2 / (2.0 * (0.125 * P) ** 2))
    assert np.abs(t - want / want.max()).max() <= 2.0 ** -24
    c = blend_taps(P, 'constant')
    assert c.dtype == np.float32 and np.array_equal(c, np.ones(P, dtype=np.float32))
    with pytest.raises(ValueError):
        blend_taps(P, 'hann')


@pytest.mark.parametrize("stride,candidates,kept,uncovered", [(8, 48, 36, 22400), (5, 150, 120, 17604)])
def test_reference_constant_sampler_is_reproduced(stride, candidates, kept, uncovered):
    """A partition of unity: whatever the weights, blending windows that all hold 0.75 gives 0.75."""
    vol = R.shared_volume()
    const = lambda x: np.full_like(x, 0.75)
    for kind in ('constant', 'gaussian'):
        ref = R.reference(vol, R.shared_cfg(stride), const, blend=kind)
        assert (ref['candidates'], ref['kept']) == (candidates, kept)
        assert int((~ref['covered']).sum()) == uncovered and vol.size == 63360
        assert ref['windows_per_voxel'] == -(-16 // stride) ** 3
        inner = ref['covered'] & ~ref['background']
        assert inner.any() and ref['background'].any()
        if kind == 'constant':
            assert (ref['mean'][inner] == 0.75).all()
        else:
            assert np.abs(ref['mean'][inner] - 0.75).max() <= 1e-12
        assert (ref['mean'][~ref['covered'] & ~ref['background']] == np.float64(ref['fill'])).all()
        assert (ref['mean'][ref['background']] == np.float64(ref['min_val'])).all()
        assert not ref['std'].any()


def test_reference_block_split_matches_oracle():
    from oracle import iqt_oracle as O
    x = np.random.default_rng(0).standard_normal((1, 1, 24, 24, 24)).astype(np.float32)
    sub = R.split_block(x, 8)
    assert np.array_equal(sub, O.convert_volume_to_subvolume(torch.from_numpy(x), (27, 1, 8, 8, 8)).numpy())
    assert np.array_equal(R.merge_block(sub, 24), x)
    assert np.array_equal(O.merge_sub_volumes(torch.from_numpy(sub), (1, 1, 24, 24, 24)).numpy(), x)


def test_reference_sampler_sees_order_and_sample():
    vol = R.shared_volume()
    ref = R.reference(vol, R.shared_cfg(8), R.make_sampler(3), samples=3, blend='gaussian')
    inner = ref['covered'] & ~ref['background']
    assert (ref['std'][inner] > 0).any() and not ref['std'][~inner].any()
    a = R.reference(vol, R.shared_cfg(8, batch_size=1), R.make_window_sampler(2), samples=2)
    b = R.reference(vol, R.shared_cfg(8, batch_size=7), R.make_window_sampler(2), samples=2)
    assert np.array_equal(a['mean'], b['mean']) and np.array_equal(a['std'], b['std'])
    c = R.reference(vol, R.shared_cfg(8, batch_size=1), R.make_sampler(2), samples=2)
    assert not np.array_equal(a['mean'], c['mean'])


def test_validation_raises_before_any_device_use():
    from diffusioniqt_amd.inference import VolumeInference

    def never(x):
        raise AssertionError("the sampler must not run")
    cfg = R.shared_cfg(8)
    with pytest.raises(ValueError, match="blend"):
        VolumeInference(cfg, never, blend='hann')
    with pytest.raises(ValueError, match="samples"):
        VolumeInference(cfg, never, blend='gaussian', samples=0)
    with pytest.raises(ValueError, match="blend"):
        VolumeInference(cfg, never, samples=2)
    cpu_vol = torch.from_numpy(R.shared_volume())                       # a CPU tensor: any device use would raise RuntimeError
    with pytest.raises(NotImplementedError, match="whole volumes"):
        VolumeInference(cfg, never, blend='gaussian')(cpu_vol, patch_slice=(0, 2))
    with pytest.raises(ValueError, match="return_std"):
        VolumeInference(cfg, never)(cpu_vol, return_std=True)
    with pytest.raises(ValueError, match="return_std"):
        VolumeInference(cfg, never, blend='constant')(cpu_vol, return_std=True)
    inf = VolumeInference(cfg, never)                                   # the defaults are today's path
    assert inf.blend is None and inf.samples == 1


def test_volume_blend_bad_arguments_return_error_codes():
    from diffusioniqt_amd import _lib
    lib = _lib.load()
    shape = (1, 4, 40, 36, 44, 16, 8, 4, 3, 4)                          # S, N, D, H, W, P, stride, G0, G1, G2
    tail = (300.0, 200.0, -1.5, -1.5, None)
    assert lib.diqt_volume_blend(None, None, None, None, None, None, *shape, *tail) == -2          # DIQT_E_ALIGN
    assert b"null pointer" in lib.diqt_last_error()
    p = 256                                                             # any non-null address: the checks below return before a launch

    def rc(S=1, N=4, D=40, H=36, W=44, P=16, stride=8, G=(4, 3, 4), std_out=None):
        return lib.diqt_volume_blend(p, p, p, None, p, std_out, S, N, D, H, W, P, stride, *G, *tail)
    assert rc(P=37) == -1 and b"shape" in lib.diqt_last_error()         # DIQT_E_SHAPE: P > min(D, H, W)
    assert rc(stride=0) == -1
    assert rc(S=0) == -1
    assert rc(G=(4, 3, 3)) == -1 and b"lattice" in lib.diqt_last_error()
    assert rc(stride=5, G=(4, 3, 4)) == -1
    assert rc(S=1, std_out=p) == -1 and b"2 samples" in lib.diqt_last_error()
    with pytest.raises(RuntimeError, match="volume_blend"):
        _lib.call("diqt_volume_blend", None, None, None, None, None, None, *shape, *tail)
