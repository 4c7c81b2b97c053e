"""The 16-bit conv dispatch on integer-valued data, bit for bit against float64: tests/conv_fuzz_worker_h.py runs the cases
tests/conv_fuzz_plan_h.py draws (tests/test_conv_fuzz_plan_h.py proves their coverage on the CPU) --

* family ``ops16``: ops.conv3d with autograd under fp16, bf16 and fp16 with the loss scaler's 16-bit backward: forward, dX (mode-1 packing
  on the 16-bit kernels), dW and db (conv_wgrad_h_kernel), and the fp32 fallbacks;
* family ``io16``: diqt_conv3d_fwd_h_io with 16-bit x / y, residual, statistics and the test switches (every kernel id of
  diqt_conv3d_fwd_h_kernel_id, conv_f9h_kernel's variants 1..5), diqt_conv3d_bwd_weight_h with 16-bit x / dY, and refusals.

Every comparison is torch.equal; the launches seen must be the ones the shape queries predicted.  The worker runs through
tests/test_gpu_conv_fuzz.py's run_worker, so a fault or timeout in either file stops both.

Measured on an MI355X host with 16 CPU threads, per seed (the pytest call: process start, plan, worker): ``ops16`` 5.0 / 4.6 / 4.8 s for
seeds 21 / 22 / 23 (118 cases and 1.5e10-1.6e10 multiply-adds of float64 reference each; the worker itself 3.0 s for seed 21, 2.0 s of it
the reference), ``io16`` 4.4 / 4.0 / 3.8 s for seeds 31 / 32 / 33 (128 cases, 1.4e10-1.7e10 multiply-adds; the worker 1.8 s for seed 31, 1.0 s
the reference).  Cases per target: ``pytest -s tests/test_conv_fuzz_plan_h.py`` prints the table (every reachable target >= 3 over the
three seeds of a family).
"""
import os

import pytest

from tests import conv_fuzz_plan_h as plan
from tests.test_gpu_conv_fuzz import run_worker


def _run(family, seed):
    env = {k: v for k, v in os.environ.items() if not k.startswith("DIQT_")}
    r = run_worker(family, seed, env, script="conv_fuzz_worker_h.py")
    assert r.returncode == 0 and "FUZZ_OK" in r.stdout, r.stdout[-8000:] + r.stderr[-2000:]
    n = sum(1 for line in r.stdout.splitlines() if line.startswith("case "))
    assert n == len(plan.cases(family, seed)), f"{n} case lines:\n" + r.stdout[-2000:]


@pytest.mark.gpu
@pytest.mark.parametrize("seed", plan.OPS16_SEEDS)
def test_integer_data_through_ops_conv3d_in_16_bit(seed):
    _run("ops16", seed)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", plan.IO16_SEEDS)
def test_integer_data_through_the_16_bit_entry_points(seed):
    _run("io16", seed)
