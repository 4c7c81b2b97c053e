"""bench.py's command line and its output dump, without a GPU: the plain / --full switch exists, and --dump-outputs writes float32
arrays within its 64 MB budget, sampling a larger output at the same seeded positions every time."""
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_help_lists_full_and_dump_outputs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "--full" in r.stdout and "--dump-outputs" in r.stdout


def test_write_outputs_float32_budget_and_fixed_sample(tmp_path):
    import bench
    big = torch.arange(10_000_000, dtype=torch.float64)
    arrays = {"img": torch.randn(2, 1, 4, 4, 4), "loss": torch.tensor([1.5]), "big": big}
    budget = 4 * 10**6
    bench.write_outputs(str(tmp_path / "a"), arrays, budget=budget)
    bench.write_outputs(str(tmp_path / "b"), arrays, budget=budget)
    total = 0
    for name in arrays:
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert a.dtype == np.float32 and np.array_equal(a, b)
        total += a.nbytes
    assert total <= budget
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "img.npy"), arrays["img"].numpy())
    s = np.load(tmp_path / "a" / "big.npy")
    assert s.ndim == 1 and 0 < s.size < big.numel() and np.all(np.diff(s) > 0)     # sorted, distinct positions of the original
