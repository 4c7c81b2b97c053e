"""The conv3d weight-gradient dispatch as the shape queries report it, on the CPU: frozen answers of every query over a fixed list of
geometries, and the properties that tie them to the one decision behind the launch (``convw_route``, read through
``diqt_conv3d_bwd_weight_route``).

The list: the 10 936 geometries of ``test_conv_fwd_route_host.geometries()``, then (1,7,7) and (5,5,5) filters with 'same' padding and
the causal (3,1,1) filter (pad (2,0,0), extra pad (-2,0,0)) over B in 1, 2, cube edges 6, 8, 12, 16, Cin in 3, 8, 20, 32 and Cout in
1, 7, 24, 40, then (1,256,8,8) 32->32 3x3x3 (conv_wgrad3_kernel refuses D > 255) and 4100 flattened rows 128->64 1x1x1 (rows that are no
multiple of 64).  Every 1x1x1 filter of the list has zero padding.  A row holds the geometry and the answers of
``diqt_conv3d_bwd_weight_kernel_id``, ``_workspace_bytes``, ``_h_workspace_bytes`` and ``_h_supported`` for flags 0, 2, 4 and 6.  The
weight-gradient planners read no environment variable: one process records them.

tests/golden/conv_wgrad_queries.json holds, per filter, the row count, the count per kernel id and the SHA-256 of the canonical JSON of
the rows.  It was recorded from commit 411bfd2, the last one with three copies of the dispatch rules in conv_mfma.hip (the launch, the
workspace query and the kernel-id query), and is what folding them into one route had to keep: it is not to be regenerated from later
code.  The recorder (``rows``) calls only ``_lib.query`` on symbols that commit exports, so this file's ``record`` mode runs on either
tree: ``python tests/test_conv_wgrad_route_host.py record [DIR]`` prints the summary and, given DIR (or with DIQT_CONV_QUERIES_DUMP=DIR
under pytest), writes one row per line to DIR/wgrad.json for diffing."""
import collections
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)

import pytest

from diffusioniqt_amd import _lib
from tests import test_conv_fwd_route_host as fwd_host

GOLDEN = os.path.join(ROOT, "tests", "golden", "conv_wgrad_queries.json")
H_FLAGS = (0, 2, 4, 6)       # bits of diqt_conv3d_bwd_weight_h's `bf16` argument: 2: 16-bit x, 4: 16-bit dY
ID0_PATHS, KERNEL_PATHS = (0, 1, 2), {3: 3, 4: 2, 5: 1}          # diqt_conv3d_bwd_weight_route, field 1 -> field 0
# 1x1x1 filters with one output channel and a padded output: the launch has no column sum for them (it needs the flattened rows)
PADDED_ONE_CHANNEL = [(1, 8, 8, 8, 32, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0), (2, 6, 9, 12, 20, 1, 1, 1, 1, 0, 1, 1, 0, 0, 0),
                      (1, 16, 16, 16, 64, 1, 1, 1, 1, 0, 0, 0, 1, 0, 0)]


def geometries():
    geos = list(fwd_host.geometries())
    for k, pad, epad in (((1, 7, 7), (0, 3, 3), (0, 0, 0)), ((5, 5, 5), (2, 2, 2), (0, 0, 0)), ((3, 1, 1), (2, 0, 0), (-2, 0, 0))):
        for B in (1, 2):
            for A in (6, 8, 12, 16):
                for Cin in (3, 8, 20, 32):
                    for Cout in (1, 7, 24, 40):
                        geos.append((B, A, A, A, Cin, Cout, *k, *pad, *epad))
    geos.append((1, 256, 8, 8, 32, 32, 3, 3, 3, 1, 1, 1, 0, 0, 0))
    geos.append((1, 1, 1, 4100, 128, 64, 1, 1, 1, 0, 0, 0, 0, 0, 0))
    return list(dict.fromkeys(geos))


COLUMNS = ("kernel_id", "ws", "ws_h", "h_supported_0", "h_supported_2", "h_supported_4", "h_supported_6")


def rows(geos):
    """[geometry + answers], the answers in the order of COLUMNS"""
    q = _lib.query
    return [[*g, q("diqt_conv3d_bwd_weight_kernel_id", *g), q("diqt_conv3d_bwd_weight_workspace_bytes", *g),
             q("diqt_conv3d_bwd_weight_h_workspace_bytes", *g), *(q("diqt_conv3d_bwd_weight_h_supported", *g, f) for f in H_FLAGS)] for g in geos]


def summary(table):
    by_filter = collections.defaultdict(list)
    for r in table:
        by_filter["%dx%dx%d" % tuple(r[6:9])].append(r)
    return {f: {"rows": len(rs), "kernel_ids": dict(sorted(collections.Counter(str(r[15]) for r in rs).items())),
                "sha256": hashlib.sha256(json.dumps(rs, separators=(",", ":")).encode()).hexdigest()}
            for f, rs in sorted(by_filter.items())}


def record(where=None):
    table = rows(geometries())
    if where:
        fwd_host.dump("wgrad", table, where)
    return summary(table)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def geos():
    return geometries()


def test_the_list_is_the_recorded_one(golden, geos):
    inherited = fwd_host.geometries()
    assert len(inherited) == 10936 and geos[:10936] == inherited and len(geos) == 10936 + 3 * 2 * 4 * 4 * 4 + 2
    assert sum(v["rows"] for v in golden.values()) == len(geos)
    assert not [g for g in geos if g[6:9] == (1, 1, 1) and any(g[9:])]                  # the padded 1x1x1 shapes are pinned below
    ids = collections.Counter()
    for v in golden.values():
        ids.update(v["kernel_ids"])
    assert set(ids) == {"0", "1", "2", "3"}, ids


def test_query_answers_are_the_recorded_ones(golden):
    got = record(os.environ.get("DIQT_CONV_QUERIES_DUMP"))
    for f in sorted(set(got) | set(golden)):
        print(f, got.get(f, {}).get("kernel_ids"))
        assert got.get(f) == golden.get(f), "filter %s: run `python tests/test_conv_wgrad_route_host.py record DIR` here and on commit " \
                                            "411bfd2 and diff DIR/wgrad.json" % f


# ---- the route behind the launch ---------------------------------------------------------------------------------------------------
def route(g, aligned=1, want_bias=0):
    """(kernel id, path, split-K shares, bias rides on the kernel, workspace bytes used, return code) of diqt_conv3d_bwd_weight_route"""
    return tuple(_lib.query("diqt_conv3d_bwd_weight_route", *g, aligned, want_bias, field) for field in range(6))


def check_route(g):
    kid = _lib.query("diqt_conv3d_bwd_weight_kernel_id", *g)
    ws = _lib.query("diqt_conv3d_bwd_weight_workspace_bytes", *g)
    assert kid == route(g)[0], g
    for want_bias in (0, 1):
        al, un = route(g, 1, want_bias), route(g, 0, want_bias)
        for r in (al, un):
            assert r[4] <= ws, (g, want_bias, r, ws)
            assert r[2] <= 1 or r[4] > 0, (g, want_bias, r)
            assert (r[1] in ID0_PATHS) == (r[0] == 0), (g, want_bias, r)
            assert (r[5] == 0) == (r[1] >= 0) and (r[0] == 0 or r[1] < 0 or KERNEL_PATHS[r[1]] == r[0]), (g, want_bias, r)     # -1: refused
            assert not r[3] or (want_bias and r[0] in (2, 3)), (g, want_bias, r)
        assert un[0] != 3 and (un == al or al[0] == 3), (g, want_bias, al, un)
        assert al[:3] == route(g, 1, 1 - want_bias)[:3], (g, want_bias)              # a bias wish moves no launch to another kernel
    assert _lib.query("diqt_conv3d_bwd_weight_route", *g, 1, 0, 6) == -1             # unknown field


def test_the_queries_are_the_route_of_their_ask(geos):
    for g in geos:
        check_route(g)


def test_a_bad_shape_is_refused_by_every_query():
    g = (1, 0, 8, 8, 32, 32, 3, 3, 3, 1, 1, 1, 0, 0, 0)
    assert _lib.query("diqt_conv3d_bwd_weight_kernel_id", *g) == -1 and _lib.query("diqt_conv3d_bwd_weight_workspace_bytes", *g) == 0
    r = route(g)
    assert r[:2] == (-1, -1) and r[4] == 0 and r[5] == -1, r                           # DIQT_E_SHAPE, as the launch returns


@pytest.mark.parametrize("g", PADDED_ONE_CHANNEL)
def test_padded_one_channel_1x1x1_filters_run_a_conv_kernel(g):
    """``diqt_conv3d_bwd_weight_kernel_id`` used to answer 0 ("GEMM / column-sum path") for every 1x1x1 filter with one output
    channel.  The launch takes the weighted column sum only where the output rows are the input rows (no padding); a padded one falls
    through im2col (1x1x1: not taken) and the 1x1x1 GEMM (padding: not taken) to the conv kernels.  The query is now the launch's route,
    so these shapes (not in the frozen list) answer the id of that kernel."""
    r = route(g)
    assert r[0] in (1, 2, 3) and r[0] == _lib.query("diqt_conv3d_bwd_weight_kernel_id", *g), r
    assert r[1] == {3: 3, 2: 4, 1: 5}[r[0]] and r[5] == 0, r
    check_route(g)
    if g == PADDED_ONE_CHANNEL[0]:
        assert r[0] == 2, r                                          # conv_bwd_weight2_kernel: Cout = 1 is no shape of conv_wgrad3_kernel
    flat = (*g[:9], 0, 0, 0, 0, 0, 0)
    assert route(flat)[:2] == (0, 0) and _lib.query("diqt_conv3d_bwd_weight_kernel_id", *flat) == 0      # un-padded: the column sum


if __name__ == "__main__":
    if sys.argv[1] == "record":                  # as tests/golden/conv_wgrad_queries.json holds it
        print(json.dumps(record(sys.argv[2] if len(sys.argv) > 2 else None), indent=1, sort_keys=True))
