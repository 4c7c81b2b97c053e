"""The three-product split route (conv_split16.hip) keeps its bits: y and the statistics partials of the cases of
tools/make_golden_split16_bits.py hash to the digests recorded in tests/golden/split16_bits.json on the commit named there, and two
launches agree with each other.  The kernel's schedule may change (weight ring, waits, tile boundary); its arithmetic may not.

The cases walk what such a change touches: three tiles per workgroup with one chunk (the weight ring wraps inside and across tiles)
under the four residual x statistics instantiations, workgroups with three and with two tiles, two and three chunks, a Cout padded
to 64 with a ragged last D tile.  On a mismatch the message gives max |y - float64 ref| / max |ref| on the first and last batch entry:
about 3e-7 is a rounding change, a stale weight panel or a missed wait reads orders of magnitude above that."""
import json
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_golden_split16_bits as G  # noqa: E402

with open(G.GOLDEN) as _f:
    GOLD = json.load(_f)


def float64_error(name, host, y):
    case = G.CASES[name][0]
    x, w, b, r, gamma, beta, ss = host
    B, Cin, pad = case[1], case[3], case[5]
    idx = [0, B - 1]
    h = x[idx].double()
    if case[7]:
        h = F.group_norm(h, 8, gamma.double(), beta.double(), eps=1e-5)
        if ss is not None:
            s = ss[idx].double()
            h = h * (s[:, :Cin, None, None, None] + 1.0) + s[:, Cin:, None, None, None]
        h = F.mish(h)
    ref = F.conv3d(h, w.double(), b.double(), padding=pad)
    if r is not None:
        ref = ref + r[idx].double()
    got = y.cpu().permute(0, 4, 1, 2, 3).double()[idx]
    return (got - ref).abs().max().item() / max(ref.abs().max().item(), 1e-30)


def test_golden_names_every_case():
    assert set(GOLD["cases"]) == set(G.CASES) and GOLD["commit"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(G.CASES))
def test_split16_bits(name):
    from diffusioniqt_amd import _lib
    _lib.load()
    assert _lib.query("diqt_conv3d_fwd_split16_supported", *G.geometry(name)) == 1, "the route's planner refuses this geometry"
    host = G.host_inputs(name)
    try:
        (y, st), (y2, st2) = G.run_case(name, host)
    except RuntimeError as e:            # a HIP error: nothing more is started on the device in this session
        pytest.exit(f"{name}: {e}", returncode=3)
    assert torch.equal(y, y2), "two launches differ in y"
    assert st is None or torch.equal(st, st2), "two launches differ in the statistics partials"
    got, want = G.digests(y, st), GOLD["cases"][name]
    if got != want:
        err = float64_error(name, host, y)
        pytest.fail(f"{name}: bits differ from commit {GOLD['commit']} (y {'same' if got['y'] == want['y'] else 'DIFFERS'}, statistics "
                    f"{'same' if got['stats'] == want['stats'] else 'DIFFER'}); max |y - float64 ref| / max |ref| = {err:.3e}")
