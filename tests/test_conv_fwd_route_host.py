"""The fp32 conv3d forward dispatch as the shape queries report it, on the CPU: frozen answers of every query over a fixed list of
geometries, and the properties that tie them to the one decision behind the launch (``convf_route``, read through
``diqt_conv3d_fwd_route``).

The list: every forward and every backward-data geometry of ``plan.cases("default", 11|12|13)`` and ``plan.cases("f9small", 1|2)``, then
a sweep of filters (3,3,3) / (1,3,3) / (3,1,1) with 'same' padding and (1,1,1) over B in 1, 2, 8, 27, cube edges 4..48, Cin 1..512 and
Cout 1..256 -- 10 936 geometries.  A row holds, per geometry, the answers of ``diqt_conv3d_fwd_kernel_id``, ``_fwd9_variant``,
``_stats_blocks`` / ``_pk``, ``_neighbours_stats_blocks`` (where the geometry is a sub-volume batch), ``_workspace_bytes`` / ``_pk``,
``_gn_supported`` / ``_pk`` for Mish, SiLU and GELU and ``_gnbwd_blocks`` with the fusion switch off and on; the ``_pk`` forms for a
buffer that holds the direct pack and for one that holds the Winograd panels behind it.  The planners read DIQT_CONV_F9 / DIQT_CONV_F9W
once per process, so the rows are recorded in four CPU-only processes: no variable set, DIQT_CONV_F9=2, DIQT_CONV_F9=0, DIQT_CONV_F9W=0.

tests/golden/conv_fwd_queries.json holds, per (environment, filter), the row count, the count per kernel id and the SHA-256 of the
canonical JSON of the rows (the rows themselves are about 0.6 MB per environment).  It was recorded from commit beeb12e, the last one
before the six copies of the dispatch rules in conv_mfma.hip became one route, and is what that refactor had to keep: it is not to be
regenerated from later code.  The recorder (``rows``) calls only ``_lib.query`` on symbols that commit exports, so this file's
``record`` mode runs on either tree: ``python tests/test_conv_fwd_route_host.py record [DIR]`` prints the summary and, given DIR (or
with DIQT_CONV_QUERIES_DUMP=DIR under pytest), writes one row per line to DIR/<environment>.json for diffing."""
import collections
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)

import pytest

from diffusioniqt_amd import _lib
from tests import conv_fuzz_plan as plan

GOLDEN = os.path.join(ROOT, "tests", "golden", "conv_fwd_queries.json")
ENVS = {"default": {}, "DIQT_CONV_F9=2": {"DIQT_CONV_F9": "2"}, "DIQT_CONV_F9=0": {"DIQT_CONV_F9": "0"}, "DIQT_CONV_F9W=0": {"DIQT_CONV_F9W": "0"}}
ACTS = (1, 2, 3)             # DIQT_ACT_MISH, _SILU, _GELU
# the shapes of the latent refusal: GroupNorm-apply supported, conv_fwd9 split-K, and statistics rows granted to the plain launch
PINNED = [(2, 16, 16, 16, 32, 256, 1, 3, 3, 0, 1, 1, 0, 0, 0), (8, 16, 16, 16, 32, 64, 1, 3, 3, 0, 1, 1, 0, 0, 0),
          (1, 32, 32, 32, 32, 16, 1, 3, 3, 0, 1, 1, 0, 0, 0)]


def geometries():
    geos = []
    for family, seeds in (("default", plan.DEFAULT_SEEDS), ("f9small", plan.F9SMALL_SEEDS)):
        for seed in seeds:
            for case in plan.cases(family, seed):
                B, D, H, W, Cin, Cout, k, pad, epad, res, grads = case
                Do, Ho, Wo = plan.out_extent(case)
                geos.append((B, D, H, W, Cin, Cout, *k, *pad, *epad))
                geos.append((B, Do, Ho, Wo, Cout, Cin, *k, *(kk - 1 - p for kk, p in zip(k, pad)), *(-e for e in epad)))
    for k in ((3, 3, 3), (1, 3, 3), (3, 1, 1), (1, 1, 1)):
        for B in (1, 2, 8, 27):
            for A in (4, 8, 12, 16, 24, 32, 48):
                for Cin in (1, 2, 3, 4, 8, 16, 32, 48, 64, 128, 192, 256, 512):
                    for Cout in (1, 2, 16, 32, 64, 128, 256):
                        geos.append((B, A, A, A, Cin, Cout, *k, *(kk // 2 for kk in k), 0, 0, 0))
    return list(dict.fromkeys(geos))              # each geometry once, in order of first appearance


def packed_lengths(geo):
    """(direct pack, direct pack + Winograd panels) of the filter a launch of this geometry reads"""
    Cin, Cout, k = geo[4], geo[5], geo[6:9]
    n = _lib.query("diqt_conv_packed_elems", Cout, Cin, *k)
    return n, n + _lib.query("diqt_conv_packed_wino_elems", Cout, Cin, *k)


COLUMNS = ("kernel_id", "variant", "variant_w", "stats", "stats_pk", "stats_pk_w", "neighbours_stats", "ws", "ws_pk", "ws_pk_w",
           "gn_mish", "gn_silu", "gn_gelu", "gn_pk_mish", "gn_pk_silu", "gn_pk_gelu", "gn_pk_w_mish", "gn_pk_w_silu", "gn_pk_w_gelu",
           "gnbwd_off", "gnbwd_on")


def rows(geos):
    """[geometry + answers], the answers in the order of COLUMNS"""
    q = _lib.query
    was = q("diqt_set_gnbwd_fuse", 0)
    gnbwd = []
    for on in (0, 1):
        q("diqt_set_gnbwd_fuse", on)
        gnbwd.append([q("diqt_conv3d_fwd_gnbwd_blocks", *g) for g in geos])
    q("diqt_set_gnbwd_fuse", was)
    out = []
    for i, g in enumerate(geos):
        B, D, H, W, Cin, Cout, kd, kh, kw, pd, ph, pw, epd, eph, epw = g
        nd, nw = packed_lengths(g)
        f = round(B ** (1 / 3))
        sub_volumes = f ** 3 == B and D == H == W and kd == kh == kw and kd % 2 == 1 and (pd, ph, pw) == (kd // 2,) * 3 and (epd, eph, epw) == (0, 0, 0)
        out.append([*g, q("diqt_conv3d_fwd_kernel_id", *g), q("diqt_conv3d_fwd9_variant", *g, nd), q("diqt_conv3d_fwd9_variant", *g, nw),
                    q("diqt_conv3d_fwd_stats_blocks", *g), q("diqt_conv3d_fwd_stats_blocks_pk", *g, nd), q("diqt_conv3d_fwd_stats_blocks_pk", *g, nw),
                    q("diqt_conv3d_fwd_neighbours_stats_blocks", f, D, Cin, Cout, kd) if sub_volumes else None,
                    q("diqt_conv3d_fwd_workspace_bytes", *g), q("diqt_conv3d_fwd_workspace_bytes_pk", *g, nd), q("diqt_conv3d_fwd_workspace_bytes_pk", *g, nw),
                    *(q("diqt_conv3d_fwd_gn_supported", *g, a) for a in ACTS), *(q("diqt_conv3d_fwd_gn_supported_pk", *g, a, nd) for a in ACTS),
                    *(q("diqt_conv3d_fwd_gn_supported_pk", *g, a, nw) for a in ACTS), gnbwd[0][i], gnbwd[1][i]])
    return out


def summary(table):
    by_filter = collections.defaultdict(list)
    for r in table:
        by_filter["%dx%dx%d" % tuple(r[6:9])].append(r)
    return {f: {"rows": len(rs), "kernel_ids": dict(sorted(collections.Counter(str(r[15]) for r in rs).items())),
                "sha256": hashlib.sha256(json.dumps(rs, separators=(",", ":")).encode()).hexdigest()}
            for f, rs in sorted(by_filter.items())}


def dump(name, table, where):
    os.makedirs(where, exist_ok=True)
    path = os.path.join(where, name.replace("=", "_") + ".json")
    with open(path, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r, separators=(",", ":")) for r in table) + "\n]\n")
    return path


def record(name, where=None):
    """The summary of environment ``name``, from a process of its own (the planners read their variables once)."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("DIQT_")}
    env.update(ENVS[name], HIP_VISIBLE_DEVICES="", **({"DIQT_LIB": os.environ["DIQT_LIB"]} if "DIQT_LIB" in os.environ else {}))
    cmd = [sys.executable, os.path.abspath(__file__), "rows", name] + ([where] if where else [])
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return json.loads(r.stdout.splitlines()[-1])


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def geos():
    return geometries()


def test_the_list_is_the_recorded_one(golden, geos):
    assert len(geos) == 10936 and set(golden) == set(ENVS)
    for name in ENVS:
        assert sum(v["rows"] for v in golden[name].values()) == len(geos)


@pytest.mark.parametrize("name", list(ENVS))
def test_query_answers_are_the_recorded_ones(name, golden):
    where = os.environ.get("DIQT_CONV_QUERIES_DUMP")
    got = record(name, where)
    for f in sorted(set(got) | set(golden[name])):
        print(name, f, got.get(f, {}).get("kernel_ids"))
        assert got.get(f) == golden[name].get(f), "%s, filter %s: run `python tests/test_conv_fwd_route_host.py record DIR` here and on " \
                                                  "commit beeb12e and diff DIR/%s.json" % (name, f, name.replace("=", "_"))


# ---- the route behind the launch (this process: whatever DIQT_CONV_F9 / DIQT_CONV_F9W it was started with) -------------------------
def route(g, npk, has_workspace=1, has_stats=0, sub_f=0, gn_act=0):
    """(kernel, ksplit, variant, statistics rows, workspace bytes) of diqt_conv3d_fwd_route"""
    return tuple(_lib.query("diqt_conv3d_fwd_route", *g, npk, has_workspace, has_stats, sub_f, gn_act, field) for field in range(5))


def test_kernel_id_and_variant_are_the_route_of_their_ask(geos):
    for g in geos:
        nd, nw = packed_lengths(g)
        kid = _lib.query("diqt_conv3d_fwd_kernel_id", *g)
        assert kid == route(g, nd)[0], g
        for npk in (nd, nw):
            r = route(g, npk)
            assert _lib.query("diqt_conv3d_fwd9_variant", *g, npk) == (r[2] if kid == 4 else -1), (g, npk)
            assert (r[0] == 4) == (r[2] >= 0), (g, npk, r)
        assert _lib.query("diqt_conv3d_fwd_route", *g, nd, 1, 0, 0, 0, 5) == -1           # unknown field


def check_statistics(g):
    for npk in packed_lengths(g):
        rows_pk = _lib.query("diqt_conv3d_fwd_stats_blocks_pk", *g, npk)
        ws_pk = _lib.query("diqt_conv3d_fwd_workspace_bytes_pk", *g, npk)
        for has_workspace in (0, 1):
            r = route(g, npk, has_workspace, 1)
            assert r[3] == rows_pk, (g, npk, r)
            assert r[3] == 0 or r[1] == 1, (g, npk, r)
            assert r[1] == 1 or ws_pk >= r[4] > 0, (g, npk, r)
            assert has_workspace or r[1] == 1, (g, npk, r)
        r = route(g, npk)
        assert r[1] == 1 or ws_pk >= r[4] > 0, (g, npk, r)
        for act in ACTS:
            if not _lib.query("diqt_conv3d_fwd_gn_supported_pk", *g, act, npk):
                continue
            r = route(g, npk, 1, 1, 0, act)
            assert r[0] == 4 and r[2] == route(g, npk)[2], (g, npk, act, r)             # the launch the plain ask plans, with the prologue
            assert r[3] == (rows_pk if r[1] == 1 else 0), (g, npk, act, r)              # statistics only from an un-split launch
            assert r[1] == 1 or ws_pk >= r[4] > 0, (g, npk, act, r)


def test_statistics_are_granted_to_unsplit_launches_only(geos):
    for g in geos:
        check_statistics(g)


@pytest.mark.parametrize("g", PINNED)
def test_groupnorm_apply_on_a_split_launch_is_granted_no_statistics(g):
    """Per-frame convs of a 32-channel pseudo-3D level: the plain launch with statistics runs un-split (rows granted), the
    GroupNorm-apply launch stays on conv_fwd9_kernel's split-K form and gets none (it used to be handed the plain launch's rows and
    refuse them)."""
    assert not [k for k in os.environ if k in ("DIQT_CONV_F9", "DIQT_CONV_F9W")]
    nd, nw = packed_lengths(g)
    assert nd == nw                                                  # (1,3,3): no Winograd panels
    assert _lib.query("diqt_conv3d_fwd_gn_supported_pk", *g, 2, nw) == 1 and _lib.query("diqt_conv3d_fwd_workspace_bytes_pk", *g, nw) > 0
    assert _lib.query("diqt_conv3d_fwd_stats_blocks_pk", *g, nw) > 0
    r = route(g, nw, 1, 1, 0, 2)
    assert r[0] == 4 and r[1] > 1 and r[3] == 0 and r[4] > 0, r
    plain = route(g, nw, 1, 1)
    assert plain[1] == 1 and plain[3] == _lib.query("diqt_conv3d_fwd_stats_blocks_pk", *g, nw), plain
    check_statistics(g)
    if g == PINNED[0]:
        assert r[1:3] == (2, 4) and plain[3] == 32, (r, plain)


def test_neighbour_launches_never_take_conv_fwd9(geos):
    for g in geos:
        B, D, H, W, Cin, Cout, kd, kh, kw, pd, ph, pw = g[:12]
        f = round(B ** (1 / 3))
        if not (f ** 3 == B and D == H == W and kd == kh == kw and kd % 2 == 1 and (pd, ph, pw) == (kd // 2,) * 3 and g[12:] == (0, 0, 0)):
            continue
        nd = packed_lengths(g)[0]
        r = route(g, nd, 1, 1, f)
        assert r[0] != 4 and r[3] == _lib.query("diqt_conv3d_fwd_neighbours_stats_blocks", f, D, Cin, Cout, kd), (g, r)


if __name__ == "__main__":
    if sys.argv[1] == "rows":                    # one environment, in this process: the summary as the last line
        table = rows(geometries())
        if len(sys.argv) > 3:
            dump(sys.argv[2], table, sys.argv[3])
        print(json.dumps(summary(table), sort_keys=True))
    elif sys.argv[1] == "record":                # all four, as tests/golden/conv_fwd_queries.json holds them
        print(json.dumps({name: record(name, sys.argv[2] if len(sys.argv) > 2 else None) for name in ENVS}, indent=1, sort_keys=True))
