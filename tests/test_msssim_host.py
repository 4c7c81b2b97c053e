"""MS-SSIM without a GPU: the argument checks of ``metrics.MSSIM`` that come before any device work, the workspace query of
``diqt_msssim3d``, the float64 restatement (tests/msssim_reference.py) tied to the SSIM oracle the project already pins, and
the crop rule of ``inference.evaluate_volume``."""
import math

import numpy as np
import pytest
import torch

from oracle import iqt_data_oracle as DO
from tests import msssim_reference as R


def test_size_rule_and_rank_are_checked_on_the_host():
    from diffusioniqt_amd.metrics import MSSIM
    z = torch.zeros(1, 1, 64, 64, 64)
    with pytest.raises(ValueError):
        MSSIM(z, z)                                               # 64 // 16 = 4 <= 10
    with pytest.raises(ValueError):
        MSSIM(torch.zeros(1, 1, 192, 192), torch.zeros(1, 1, 192, 192))          # 4-D (2-D images): out of scope
    with pytest.raises(ValueError):
        MSSIM(torch.zeros(1, 1, 175, 192, 192), torch.zeros(1, 1, 175, 192, 192))   # D is held to the rule as well
    with pytest.raises(ValueError):
        MSSIM(torch.zeros(1, 1, 192, 192, 175), torch.zeros(1, 1, 192, 192, 175))


def test_compat_module_exports_the_device_msssim():
    import importlib.util
    import os
    from diffusioniqt_amd import metrics as M
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'compat', 'metrics.py')
    spec = importlib.util.spec_from_file_location('_compat_metrics_under_test', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.MSSIM is M.MSSIM
    assert M.MSSIM_BETAS == R.BETAS


def test_workspace_query():
    from diffusioniqt_amd import _lib
    q = lambda *a: _lib.query("diqt_msssim3d_workspace_bytes", *a)
    assert q(1, 192, 192, 192, 11, 5) > 0
    assert q(2, 45, 52, 61, 11, 3) > 0
    assert q(1, 44, 44, 44, 11, 3) > 0
    assert q(1, 175, 192, 192, 11, 5) == 0                        # 175 >> 4 = 10 < 11
    assert q(1, 192, 175, 192, 11, 5) == 0
    assert q(1, 192, 192, 175, 11, 5) == 0
    assert q(1, 43, 44, 44, 11, 3) == 0
    assert q(1, 192, 192, 192, 11, 0) == 0 and q(1, 192, 192, 192, 11, -1) == 0
    assert q(0, 192, 192, 192, 11, 5) == 0 and q(1, 192, 192, 192, 12, 5) == 0
    # the pooled pair of scale 1 and of scale 2 live in the workspace
    assert q(1, 192, 192, 192, 11, 5) >= 4 * 2 * (96 ** 3 + 48 ** 3)
    assert q(1, 192, 192, 192, 11, 1) < 4 * 96 ** 3


def test_restatement_equals_the_pinned_ssim_oracle_at_one_scale():
    gen = torch.Generator().manual_seed(24 + 19 + 13)
    t = torch.rand(1, 1, 24, 19, 13, generator=gen)
    p = (t + 0.1 * torch.randn(1, 1, 24, 19, 13, generator=gen)).clamp(0, 1)
    value, rows = R.msssim(p, t, betas=(1.0,), data_range=1.0)
    want = float(DO.ssim(p, t, data_range=1.0))
    assert abs(rows[0][0] - want) < 1e-6, (rows[0][0], want)
    assert abs(value - rows[0][0]) < 1e-12                         # one scale, beta 1: the product is ssim_0


def test_restatement_properties():
    shape = (176, 192, 208)
    x = R.minmax(R.target_volume(shape))[None, None]
    value, rows = R.msssim(x, x)
    assert abs(value - 1.0) < 1e-12
    value, rows = R.msssim(1 - x, x)
    assert math.isnan(value)
    assert all(r[1] < 0 for r in rows[2:])                         # cs_2 .. cs_4 are negative: no clamp, the power is NaN
    # pooling halves with floor, the range is refreshed per scale
    _, rows = R.msssim(x, x, betas=R.BETAS[:3])
    assert rows[0][2] == 1.0 and rows[1][2] < rows[0][2] and rows[2][2] < rows[1][2]


def test_eval_crop_rule():
    from diffusioniqt_amd.inference import eval_crop
    assert eval_crop(240) == 24 and eval_crop(256) == 32 and eval_crop(192) == 0
    assert eval_crop(241) == 0 and eval_crop(255) == 0 and eval_crop(0) == 0


def test_evaluate_volume_argument_checks_come_first():
    from diffusioniqt_amd.inference import evaluate_volume
    with pytest.raises(ValueError):
        evaluate_volume(np.zeros((8, 8, 8), np.float32), np.zeros((8, 8, 9), np.float32))
    with pytest.raises(ValueError):
        evaluate_volume(np.zeros((240, 240, 200), np.float32), np.zeros((240, 240, 200), np.float32))   # 200 - 48 = 152 // 16 = 9
