"""The normalisation and soft-max launchers of csrc/elementwise.hip across their dispatch, against float64: tests/norm_fuzz_worker.py runs
the cases tests/norm_fuzz_plan.py draws (tests/test_norm_fuzz_plan.py proves their coverage on the CPU from the launchers' own route queries) --

* family ``gn32``: the GroupNorm statistics, coefficient, apply and backward entries in fp32 (both colreduce paths, 1 / 2-255 / 256 workgroups,
  the empty trailing workgroups at 16385 rows, both apply kernels, every activation, producer partials with 1 to 2048 blocks);
* family ``gn16``: diqt_gn_act_fwd_h and diqt_gn_act_bwd_h with every compile-time type triple and two run-time ones;
* family ``softmax``: diqt_softmax_fwd then diqt_softmax_bwd on both sides of every threshold of diqt_softmax_route;
* family ``rows``: channel LayerNorm forward / backward, l2norm over strided rows, the attention soft-max and both of its backwards.

Outputs and workspaces sit in guarded, NaN-prefilled buffers; the launches seen must be the ones the route queries predicted; every case
runs twice, bit-identical (drel / dnull of the atomic attention soft-max backward by tolerance only).  The worker runs through
tests/test_gpu_conv_fuzz.py's run_worker, so a fault or timeout in any fuzz file stops the others on that card.

Measured on an MI355X host with 16 CPU threads, per seed (the pytest call: process start, plan, worker), next to the attention fuzz in the
same session (its slowest seed: ``bwd32`` 5.06 s): ``softmax`` 3.9 / 4.2 / 4.1 s for seeds 91 / 92 / 93 (71 cases, 2.9e7-3.2e7 reference
elements, the worker itself 1.5-1.8 s), ``gn32`` 3.7 / 2.9 / 3.2 s for seeds 71 / 72 / 73 (140 cases, 1.7e7-2.0e7 elements, the worker
0.9-1.6 s), ``gn16`` 2.6 / 2.9 / 2.5 s for seeds 81 / 82 / 83 (54 cases, the worker 0.5-0.7 s), ``rows`` 2.2 / 2.3 / 2.3 s for seeds
101 / 102 / 103 (124 cases, the worker 0.4-0.6 s).
Largest errors seen, relative to max|ref| (per row / column where the worker judges so): GroupNorm y 3.6e-7, coef 9.8e-8, dx 1.9e-6, dgamma
7.1e-6, dbeta 7.6e-7, dscale 4.2e-6, dshift 7.0e-7; soft-max y 3.3e-6, dx 2.4e-7; LayerNorm y 2.2e-7, mean 5.1e-7, rstd 1.1e-7, dx 1.3e-7,
dg 3.3e-7, db 2.5e-6; l2norm 3.1e-6; attention soft-max p 2.6e-7, dsim 2.5e-7, drel 1.5e-7 (table) / 5.5e-7 (atomics), dnull 4.8e-7 / 6.8e-7.
Statistics against the bound derived from the reduction's shape (worker docstring), largest share of the bound used, mean / rstd:
randn 0.10 / 0.28, offset 0.33 / 0.46 (the constructed 16385-row offset cases included: the E[x^2] - m^2 form of gn_stats_final_kernel
holds the bound with room to spare, no kernel change), tiny 0.04 / 0.48, wide 0.07 / 0.24, const 0.15 / 0.46.
Found by this fuzz and fixed: a 16-bit x or dy behind the scalar path of colreduce_kernel (C > 1024) was indexed as fp32 -- an illegal
address at (2, 831, 1028) with an fp16 dy (plan: "16-bit behind the scalar reduce").
Cases per target: ``pytest -s tests/test_norm_fuzz_plan.py`` prints the tables (every reachable target >= 3 over the three seeds of a family).
"""
import os

import pytest

from tests import norm_fuzz_plan as plan
from tests import test_gpu_conv_fuzz as conv_fuzz
from tests.test_gpu_conv_fuzz import run_worker


def _run(family, seed):
    env = {k: v for k, v in os.environ.items() if not k.startswith("DIQT_")}
    r = run_worker(family, seed, env, script="norm_fuzz_worker.py")
    if "illegal memory access" in r.stdout + r.stderr:          # HIP reported a fault and Python turned it into an ordinary exit status
        conv_fuzz._card_faulted.append(f"{family} seed {seed}: illegal memory access")
    assert r.returncode == 0 and "FUZZ_OK" in r.stdout, r.stdout[-8000:] + r.stderr[-2000:]
    n = sum(1 for line in r.stdout.splitlines() if line.startswith("case "))
    assert n == len(plan.cases(family, seed)), f"{n} case lines:\n" + r.stdout[-2000:]


@pytest.mark.gpu
@pytest.mark.parametrize("seed", plan.SEEDS["gn32"])
def test_groupnorm_fp32_entries(seed):
    _run("gn32", seed)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", plan.SEEDS["gn16"])
def test_groupnorm_16_bit_entries(seed):
    _run("gn16", seed)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", plan.SEEDS["softmax"])
def test_softmax_forward_and_backward(seed):
    _run("softmax", seed)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", plan.SEEDS["rows"])
def test_layernorm_l2norm_and_attention_softmax(seed):
    _run("rows", seed)
