"""Scheduling of the Winograd F(2,3) tile of conv_fwd9_kernel (variant 7): cases in which a change to the order of its DMA issues,
waits, fragment reads or to its epilogue could go wrong and which tests/test_gpu_conv_f9w.py does not reach (tests/f9w_sched_worker.py
lists them).  Per case: the route, the error against a float64 host convolution (the bound of tests/test_gpu_conv_f9w.py for this
tile), the epilogue statistics, and bit-identity of output and statistics to the digests in tests/golden/f9w_sched_digests.json
(recorded with `f9w_sched_worker.py <group> --record` on the commit whose results the kernel has to keep)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import f9w_sched_worker as worker  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    with open(worker.GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def main_runs():
    from diffusioniqt_amd import _lib
    _lib.load()
    return {case[0]: worker.evaluate(case, want) for case, want in worker.MAIN}


@pytest.fixture(scope="module")
def ragged_runs():
    # the planner reads DIQT_CONV_F9 once per process: the ragged case needs a process of its own
    env = dict(os.environ, DIQT_CONV_F9="2")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "f9w_sched_worker.py"), "ragged"], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("F9WS_RESULT ")]
    assert line, r.stdout[-3000:]
    return json.loads(line[-1][len("F9WS_RESULT "):])


def check(name, want_stats, v, golden):
    print(f"{name}: {v}")
    assert v["taken"], f"{name}: gn_conv3d returned None"
    assert v["variant"] == 7, f"{name}: the launch ran variant {v['variant']}"
    assert v["err"] <= 2e-5, f"{name}: max error {v['err']:.3e} vs float64"
    if want_stats:
        assert v["stats"] is not None, f"{name}: no statistics emitted"
        assert v["stats"] <= 1e-4 and v["sumsq"] <= 1e-4, f"{name}: column sums {v['stats']:.3e} / sums of squares {v['sumsq']:.3e}"
    else:
        assert v["stats_sha"] is None, f"{name}: a split-K launch emits no statistics of its own"
    assert v["y_sha"] == golden[name]["y_sha256"], f"{name}: output bits differ from the recorded ones"
    assert v["stats_sha"] == golden[name]["stats_sha256"], f"{name}: statistics bits differ from the recorded ones"


@pytest.mark.gpu
@pytest.mark.parametrize("name,want_stats", [(c[0], w) for c, w in worker.MAIN])
def test_winograd_schedule_cases(main_runs, golden, name, want_stats):
    check(name, want_stats, main_runs[name], golden)


@pytest.mark.gpu
@pytest.mark.parametrize("name,want_stats", [(c[0], w) for c, w in worker.RAGGED])
def test_winograd_schedule_ragged_cases(ragged_runs, golden, name, want_stats):
    check(name, want_stats, ragged_runs[name], golden)
