"""MI355X checks of the device MS-SSIM (``diqt_msssim3d`` -> ``ops.msssim3d`` -> ``metrics.MSSIM`` ->
``inference.evaluate_volume``) against the float64 restatement of torchmetrics 0.9.0 in tests/msssim_reference.py.

Inputs are generated from formulas (tests/msssim_reference.py); every factor of the reference's product is asserted to be
>= 0.3 on the reference side, so a comparison never degenerates into NaN == NaN.  Tolerances: per-scale ssim / cs absolute 1e-5
(what ``diqt_ssim3d`` is held to), range relative 1e-6 (the pooling rounds in fp32), the product by first-order propagation of
the per-term tolerance plus 2e-7 for the fp32 result's own rounding."""
import math

import numpy as np
import pytest
import torch

from oracle import iqt_data_oracle as DO
from tests import msssim_reference as R

pytestmark = pytest.mark.gpu

BIG = (176, 192, 208)
TERM_FLOOR = 0.3


def _f32(x):
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32))


def _case(name):
    """-> (pred, target) fp32 CPU tensors [B,1,D,H,W], number of scales"""
    if name == 'bias+texture':
        return _f32(R.minmax(R.bias_texture_pred(BIG)))[None, None], _f32(R.minmax(R.target_volume(BIG)))[None, None], 5
    if name == 'blur':
        return _f32(R.minmax(R.blur_pred(BIG)))[None, None], _f32(R.minmax(R.target_volume(BIG)))[None, None], 5
    if name == 'small raw':                                        # un-normalised, odd sizes, two volumes
        sh = (45, 52, 61)
        p = np.stack([R.noise_pred(sh, 3, 4), R.noise_pred(sh, 5, 6)])[:, None]
        t = np.stack([R.target_volume(sh, 3), R.target_volume(sh, 5)])[:, None]
        return _f32(p), _f32(t), 3
    if name == 'minimal':                                          # one surviving window at the last scale
        sh = (44, 44, 44)
        return _f32(R.noise_pred(sh))[None, None], _f32(R.target_volume(sh))[None, None], 3
    raise KeyError(name)


# the reference's own terms for the two 5-scale cases, three decimals (all ten distinct per case: a swapped cs / ssim, a wrong beta
# order or a range that is not refreshed per scale cannot hide); checked on the reference side so that the inputs stay what they are
QUOTED = {'bias+texture': ((.707, .730, .768, .790, .740), (.949, .936, .886, .813, .751), (1., .964, .913, .856, .701)),
          'blur': ((.415, .533, .767, .993, .996), (.952, .978, .992, .997, .996), None)}
_REF = {}


def _reference(name):
    if name not in _REF:
        p, t, scales = _case(name)
        value, rows = R.msssim(p, t, betas=R.BETAS[:scales])
        print(f'{name}: reference ms-ssim {value:.9f}')
        for s, r in enumerate(rows):
            print(f'   scale {s}: ssim {r[0]:.7f} cs {r[1]:.7f} range {r[2]:.6f}')
        assert min(R.terms_of(rows)) >= TERM_FLOOR, (name, rows)
        assert math.isfinite(value)
        if name in QUOTED:
            for col, want in enumerate(QUOTED[name]):
                if want is not None:
                    assert all(abs(r[col] - w) < 1.5e-3 for r, w in zip(rows, want)), (name, col, rows)
        _REF[name] = (p, t, scales, value, rows)
    return _REF[name]


@pytest.mark.parametrize('name', ['bias+texture', 'blur', 'small raw', 'minimal'])
def test_per_scale_terms_match_the_restatement(name):
    from diffusioniqt_amd import ops
    from diffusioniqt_amd.metrics import gaussian_taps
    p, t, scales, value, rows = _reference(name)
    betas = np.asarray(R.BETAS[:scales], dtype=np.float32)
    pd, td = p.cuda().reshape(-1, *p.shape[2:]), t.cuda().reshape(-1, *t.shape[2:])
    out = ops.msssim3d(pd, td, gaussian_taps(1.5), betas)
    assert out.is_cuda and tuple(out.shape) == (1 + 3 * scales,)
    got = out.cpu().double().numpy()
    for s, (ssim, cs, rng) in enumerate(rows):
        g = got[1 + 3 * s: 4 + 3 * s]
        print(f'{name} scale {s}: |ssim| {abs(g[0] - ssim):.2e} |cs| {abs(g[1] - cs):.2e} range rel {abs(g[2] - rng) / rng:.2e}')
    for s, (ssim, cs, rng) in enumerate(rows):
        g = got[1 + 3 * s: 4 + 3 * s]
        assert abs(g[0] - ssim) <= 1e-5, (name, s, 'ssim', g[0], ssim)
        assert abs(g[1] - cs) <= 1e-5, (name, s, 'cs', g[1], cs)
        assert abs(g[2] - rng) <= 1e-6 * rng, (name, s, 'range', g[2], rng)
    tol = R.product_tolerance(value, rows, R.BETAS[:scales])
    print(f'{name}: product {got[0]:.9f} vs {value:.9f} (tolerance {tol:.2e})')
    assert abs(got[0] - value) <= tol, (name, got[0], value, tol)


@pytest.mark.parametrize('name', ['bias+texture', 'blur'])
def test_MSSIM_matches_the_restatement(name):
    from diffusioniqt_amd.metrics import MSSIM
    p, t, scales, value, rows = _reference(name)
    tol = R.product_tolerance(value, rows)
    got = MSSIM(p.cuda(), t.cuda())
    assert got.is_cuda and got.ndim == 0
    print(f'{name}: MSSIM {float(got):.9f} vs {value:.9f} (tolerance {tol:.2e})')
    assert abs(float(got) - value) <= tol, (float(got), value, tol)
    cpu_in = MSSIM(p, t)                                          # CPU tensors in -> computed on the device, CPU scalar out
    assert not cpu_in.is_cuda and cpu_in.ndim == 0 and float(cpu_in) == float(got)


def test_MSSIM_properties():
    from diffusioniqt_amd.metrics import MSSIM
    p, t, _, _, _ = _reference('bias+texture')
    p, t = p.cuda(), t.cuda()
    assert abs(float(MSSIM(t, t)) - 1.0) <= 1e-6                  # identical volumes
    a, b = float(MSSIM(p, t)), float(MSSIM(t, p))
    assert abs(a - b) <= 1e-6                                     # symmetric
    assert math.isnan(float(MSSIM(1 - t, t)))                     # negative cs at the coarse scales, no clamp
    assert float(MSSIM(p, t)) == a                                # fixed-order reductions: the same bits run to run
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = MSSIM(p, t)
    side.synchronize()
    assert float(on_side) == a                                    # enqueued on the caller's stream, same bits


def test_small_volumes_are_refused():
    from diffusioniqt_amd import ops
    from diffusioniqt_amd.metrics import MSSIM, gaussian_taps
    z = torch.zeros(1, 1, 64, 64, 64, device='cuda')
    with pytest.raises(ValueError):
        MSSIM(z, z)
    v = torch.zeros(1, 43, 44, 44, device='cuda')
    with pytest.raises(RuntimeError, match='fewer than 11'):
        ops.msssim3d(v, v, gaussian_taps(1.5), np.asarray(R.BETAS[:3], dtype=np.float32))


@pytest.mark.parametrize('size', [256, 240])
def test_evaluate_volume_is_the_scripts_eval(size):
    from diffusioniqt_amd.inference import evaluate_volume
    shape = (size,) * 3
    gt, pred = R.target_volume(shape).astype(np.float32), R.noise_pred(shape).astype(np.float32)
    c = {256: 32, 240: 24}[size]
    gc, pc = gt[c:-c, c:-c, c:-c].astype(np.float64), pred[c:-c, c:-c, c:-c].astype(np.float64)
    value, rows = R.msssim(R.minmax(gc)[None, None], R.minmax(pc)[None, None])
    print(f'{size}^3: reference ms-ssim {value:.9f} terms {R.terms_of(rows)}')
    assert min(R.terms_of(rows)) >= TERM_FLOOR, rows
    want_psnr = float(DO.psnr(torch.as_tensor(gc)[None, None], torch.as_tensor(pc)[None, None]))
    tol = R.product_tolerance(value, rows)
    ssim, psnr = evaluate_volume(torch.as_tensor(gt).cuda(), torch.as_tensor(pred).cuda())      # what VolumeInference returns
    assert ssim.is_cuda and psnr.is_cuda and ssim.ndim == 0 and psnr.ndim == 0
    print(f'{size}^3: ssim {float(ssim):.9f} (tolerance {tol:.2e}) psnr {float(psnr):.6f} vs {want_psnr:.6f}')
    assert abs(float(ssim) - value) <= tol, (float(ssim), value, tol)
    assert abs(float(psnr) - want_psnr) < 1e-4 * abs(want_psnr)
    for a, b in ((gt, pred), (torch.as_tensor(gt), torch.as_tensor(pred))):                    # numpy arrays, CPU tensors
        s2, p2 = evaluate_volume(a, b)
        assert not s2.is_cuda and not p2.is_cuda
        assert float(s2) == float(ssim) and float(p2) == float(psnr)
