"""Random shapes through ops.conv3d -- forward, input gradient, weight and bias gradient -- against float64 convs on the host, run by
tests/conv_fuzz_worker.py on the cases tests/conv_fuzz_plan.py draws (tests/test_conv_fuzz_plan.py proves their coverage on the CPU):

* family ``f9small``: every conv_fwd9_kernel variant on small shapes (DIQT_CONV_F9=2 makes it take launches of any tile count: ragged
  extents in all three axes, single-tile launches, ragged channel blocks, causal temporal padding, split-K);
* family ``default``: the whole dispatch in the configuration users and bench.py run (no DIQT_* variable), with shapes on and next to the
  planners' thresholds; the worker also checks that the launches it saw are the ones the shape queries predicted.

Measured on an MI355X host with 16 CPU threads: 8.5-9.6 s per ``default`` seed (132 cases, 3.8e10-4.5e10 multiply-adds; the worker
itself 6.4-7.6 s, of which 4.7-5.6 s are the float64 reference: 0.12-0.14 s per 1e9 multiply-adds), 3.2-3.7 s per ``f9small`` seed (the
worker 1.2-1.3 s, 0.9 s of it the reference).  Largest errors seen, relative to max|ref|: y 1.4e-6, dX 3.2e-6, dW 1.5e-6, db 8.2e-6.
"""
import os
import subprocess
import sys

import pytest

from tests import conv_fuzz_plan as plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAULT_STATUS = (124, 134, 137, 139, -6, -11)
_card_faulted = []      # a worker ended by a signal or the timeout: nothing more of this file starts on that card


def run_worker(family, seed, env, script="conv_fuzz_worker.py"):
    """Runs tests/<script> <family> <seed> in a process of its own (tests/test_gpu_conv_fuzz_h.py runs its worker through here too: a
    fault or timeout in either file stops both)."""
    if _card_faulted:
        pytest.skip("an earlier fuzz worker met a GPU fault or hang (%s): not starting more work on that card" % _card_faulted[0])
    cmd = [sys.executable, os.path.join(ROOT, "tests", script), family, str(seed)]
    try:
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    except subprocess.TimeoutExpired as e:
        _card_faulted.append(f"{family} seed {seed}: timeout")
        out = e.stdout.decode(errors="replace") if isinstance(e.stdout, bytes) else (e.stdout or "")
        pytest.fail("the fuzz worker hung; its last lines:\n" + out[-3000:])
    if r.returncode < 0 or r.returncode in FAULT_STATUS:
        _card_faulted.append(f"{family} seed {seed}: status {r.returncode}")
        pytest.fail(f"the fuzz worker ended with status {r.returncode} (GPU fault or abort); its last lines:\n" + r.stdout[-3000:] + r.stderr[-2000:])
    return r


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1, 2])
def test_random_shapes_on_the_one_wave_per_simd_conv(seed):
    env = dict(os.environ, DIQT_CONV_F9="2")
    r = run_worker("f9small", seed, env)
    assert r.returncode == 0 and "FUZZ_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    assert r.stdout.count("kid=4") >= 20, "most cases should have run on conv_fwd9_kernel:\n" + r.stdout[-2000:]


@pytest.mark.gpu
@pytest.mark.parametrize("seed", plan.DEFAULT_SEEDS)
def test_random_shapes_across_the_conv_dispatch(seed):
    env = {k: v for k, v in os.environ.items() if not k.startswith("DIQT_")}
    r = run_worker("default", seed, env)
    assert r.returncode == 0 and "FUZZ_OK" in r.stdout, r.stdout[-6000:] + r.stderr[-2000:]
    n = sum(1 for line in r.stdout.splitlines() if line.startswith("case "))
    assert n == len(plan.cases("default", seed)), f"{n} case lines:\n" + r.stdout[-2000:]
