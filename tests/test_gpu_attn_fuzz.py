"""The fused multi-query attention across its whole dispatch, against float64: tests/attn_fuzz_worker.py runs the cases
tests/attn_fuzz_plan.py draws (tests/test_attn_fuzz_plan.py proves their coverage on the CPU from the launchers' own plan functions) --

* family ``fwd32``: diqt_mqa_attention_fwd, _fwd_lse and the in-place temporal entry _fwd_frames (bit-identical to _fwd on transposed copies);
* family ``bwd32``: diqt_mqa_attention_fwd_lse then diqt_mqa_attention_bwd: the one-pass short-sequence kernel, the dQ kernel and the dK/dV
  kernel with every KW, a sequence per wave, VALU extra keys, the XCD remap, only extra keys, a null bias without a table, and refusals;
* family ``fwd16``: diqt_cast_to_h + diqt_mqa_attention_fwd_h in fp16 and bf16, on both sides of the 4-wave threshold.

Outputs and the workspace sit in guarded, NaN-prefilled buffers; the launches seen must be the ones the route queries predicted; every case
runs twice, bit-identical.  The worker runs through tests/test_gpu_conv_fuzz.py's run_worker, so a fault or timeout in any fuzz file stops
the others on that card.

Measured on an MI355X host with 16 CPU threads, per seed (the pytest call: process start, plan, worker): ``bwd32`` 4.8 / 5.1 / 5.2 s for
seeds 51 / 52 / 53 (121 cases and 2.9e9-3.1e9 multiply-adds of float64 reference each; the worker itself 2.7-2.9 s, 1.0 s of it the
reference), ``fwd32`` 2.4 / 2.7 / 2.7 s for seeds 41 / 42 / 43 (93 cases, 1.2e9-1.5e9 multiply-adds; the worker 0.6-0.7 s, 0.1-0.2 s the
reference), ``fwd16`` 2.6 / 2.4 / 2.6 s for seeds 61 / 62 / 63 (74 cases, 1.7e9-2.2e9 multiply-adds; the worker 0.4-0.5 s, 0.1 s the reference).
Largest errors seen, relative to max|ref|: out 3.4e-6, lse 8.0e-7, dq 3.8e-6, dkv 4.8e-6, drel 9.7e-6, dnull 8.6e-6 (fp32); 0.49 ulp (16 bit).
Cases per target: ``pytest -s tests/test_attn_fuzz_plan.py`` prints the tables (every reachable target >= 3 over the three seeds of a family).
"""
import os

import pytest

from tests import attn_fuzz_plan as plan
from tests.test_gpu_conv_fuzz import run_worker


def _run(family, seed):
    env = {k: v for k, v in os.environ.items() if not k.startswith("DIQT_")}
    r = run_worker(family, seed, env, script="attn_fuzz_worker.py")
    assert r.returncode == 0 and "FUZZ_OK" in r.stdout, r.stdout[-8000:] + r.stderr[-2000:]
    n = sum(1 for line in r.stdout.splitlines() if line.startswith("case "))
    assert n == len(plan.cases(family, seed)), f"{n} case lines:\n" + r.stdout[-2000:]


@pytest.mark.gpu
@pytest.mark.parametrize("seed", plan.SEEDS["fwd32"])
def test_fp32_forwards_and_the_frames_entry(seed):
    _run("fwd32", seed)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", plan.SEEDS["bwd32"])
def test_backward_across_its_dispatch(seed):
    _run("bwd32", seed)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", plan.SEEDS["fwd16"])
def test_16_bit_forward(seed):
    _run("fwd16", seed)
