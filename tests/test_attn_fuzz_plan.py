"""Which kernels and branches the fused-attention fuzz reaches, proved on the CPU from the library's own plan functions
(diqt_mqa_attention_bwd_route, diqt_mqa_attention_fwd_h_route): ``pytest -s`` prints the cases-per-target tables."""
import collections

import pytest

from diffusioniqt_amd import _lib
from tests import attn_fuzz_plan as plan


@pytest.fixture(scope="module")
def all_cases():
    _lib.load()
    return {fam: [c for seed in plan.SEEDS[fam] for c in plan.cases(fam, seed)] for fam in plan.SEEDS}


def bwd_targets(c):
    r = plan.route_bwd(c)
    t = ["path " + plan.PATHS[r["path"]]]
    if r["path"] == 0:
        return t
    nobias = "null bias without a table" if c.null and not c.rel else "table without a null bias" if c.rel and not c.null else None
    if nobias:
        t.append("%s, %s" % (plan.PATHS[r["path"]], nobias))
    if r["path"] == 1:
        t.append("seq nwg %s 256" % ("<" if r["nwg"] < 256 else "="))
        t.append("seq relLds %s" % ("zero" if r["relLds"] == 0 else "non-zero"))
        return t
    t += ["KW %d" % r["KW"], "EV " + ("zero" if r["EV"] == 0 else "non-zero"), "remap " + ("on" if r["remap"] else "off"),
          "perWave " + ("on" if r["perWave"] else "off"), "key-tile workgroups " + ("1" if r["nkt"] == 1 else "> 1")]
    if c.rel:
        # (h <= 64 and at most 1536 entries by the entry point's refusals: the dK/dV kernel never gathers the table from global memory)
        assert r["relLds"] == (2 * c.ns - 1) * c.h, (c, r)
        t.append("table of the dK/dV kernel in LDS")
    if plan.residue(c):
        t.append("one-hot soft-max (residue)")
    if c.ns == 0:
        t.append("no self keys (Mt %s)" % ("= 0" if r["EV"] == c.E else "> 0"))
    if c.E == 0:
        t.append("no extra key")
    if c.ns != c.n:
        t.append("n_self != n")
    if r["EV"] > 1:
        t.append("several VALU extra keys")
    return t


BWD_REACHABLE = ["path refused", "path seq", "path two-kernel", "KW 0", "KW 1", "KW 2", "KW 4", "EV zero", "EV non-zero", "remap on", "remap off",
                 "perWave on", "perWave off", "key-tile workgroups 1", "key-tile workgroups > 1", "seq nwg < 256", "seq nwg = 256",
                 "seq relLds zero", "seq relLds non-zero", "seq, null bias without a table", "seq, table without a null bias",
                 "two-kernel, null bias without a table", "two-kernel, table without a null bias", "table of the dK/dV kernel in LDS",
                 "no self keys (Mt = 0)", "no self keys (Mt > 0)", "no extra key", "n_self != n", "several VALU extra keys", "one-hot soft-max (residue)"]


def fwd16_targets(c):
    r = plan.route_fwd16(c)
    return ["%d waves" % r["waves"], "HASREL " + ("on" if r["hasrel"] else "off"), "%s round_out %d" % ("bf16" if c.bf16 else "fp16", c.round_out),
            "query workgroups " + ("1" if c.n * c.h <= r["rows"] else "> 1"), "key tiles " + ("1" if plan.keys(c) <= 64 else "> 1"),
            "data " + c.data] + (["n_self != n"] if c.ns != c.n else []) + (["null bias without a table"] if c.null and not c.rel else [])


FWD16_REACHABLE = ["4 waves", "8 waves", "HASREL on", "HASREL off", "fp16 round_out 0", "fp16 round_out 1", "bf16 round_out 0", "bf16 round_out 1",
                   "query workgroups 1", "query workgroups > 1", "key tiles 1", "key tiles > 1", "n_self != n", "null bias without a table"] + \
                  ["data " + d for d in plan.DATA]


def fwd32_targets(c):
    t = ["entry " + c.entry, "data " + c.data, "query workgroups " + ("1" if c.n * c.h <= 128 else "> 1"),
         "VALU null key " + ("on" if c.E == 1 else "off"), "key tiles " + ("<= 1" if plan.keys(c) - (c.E == 1) <= 32 else "> 1")]
    if c.entry == "fwd":
        t.append("HASREL " + ("on" if c.rel else "off"))
    if c.entry == "frames":
        t.append("frames " + ("with" if c.rel else "without") + " a table")
        t.append("frames " + ("causal" if c.causal else "not causal"))
        t.append("frames P " + ("= 1" if c.P == 1 else "> 1"))
    if c.ns != c.n:
        t.append("n_self != n" if c.ns else "no self keys")
    if c.null and not c.rel:
        t.append("null bias without a table")
    return t


FWD32_REACHABLE = ["entry fwd", "entry lse", "entry frames", "query workgroups 1", "query workgroups > 1", "VALU null key on", "VALU null key off",
                   "key tiles <= 1", "key tiles > 1", "HASREL on", "HASREL off", "frames with a table", "frames without a table", "frames causal",
                   "frames not causal", "frames P = 1", "frames P > 1", "n_self != n", "no self keys", "null bias without a table"] + \
                  ["data " + d for d in plan.DATA]


@pytest.mark.parametrize("family,targets,reachable", [("bwd32", bwd_targets, BWD_REACHABLE), ("fwd16", fwd16_targets, FWD16_REACHABLE),
                                                      ("fwd32", fwd32_targets, FWD32_REACHABLE)])
def test_every_reachable_target_is_hit_three_times(all_cases, family, targets, reachable):
    count = collections.Counter(t for c in all_cases[family] for t in targets(c))
    print("\n%s: %d cases over seeds %s" % (family, len(all_cases[family]), plan.SEEDS[family]))
    for t in sorted(set(count) | set(reachable)):
        print("  %-50s %4d" % (t, count[t]))
    assert not [t for t in reachable if count[t] < 3], {t: count[t] for t in reachable if count[t] < 3}


def _groups(family, seed):
    g = collections.defaultdict(dict)
    for label, c in plan.labelled(family, seed).items():
        if ": " in label:
            name, side = label.split(": ", 1)
            g[name][side] = c
    return g


# group -> (plan field, {side: value})
BWD_SIDES = {
    "seq G": ("path", {"511": 2, "512": 1}), "seq n": ("path", {"32": 1, "33": 2}), "seq h": ("path", {"3": 2, "4": 1}),
    "seq n_extra": ("path", {"1": 1, "2": 2}), "seq LDS": ("path", {"n 24": 1, "n 32": 2}),
    "perWave G": ("perWave", {"2047": 0, "2048": 1}), "perWave Mt": ("perWave", {"32": 1, "33": 0}),
    "KW G 2": ("KW", {"Mt 32": 1, "Mt 33": 1, "Mt 64": 1, "Mt 65": 1}), "KW G 16": ("KW", {"Mt 32": 1, "Mt 33": 1, "Mt 64": 1, "Mt 65": 1}),
    "KW G 300": ("KW", {"Mt 32": 1, "Mt 33": 1, "Mt 64": 1, "Mt 65": 2}), "KW G 600": ("KW", {"Mt 32": 1, "Mt 33": 2, "Mt 64": 2, "Mt 65": 4}),
    "EV count": ("EV", {"8 of 8": 8, "9": 0}), "EV tiles": ("EV", {"3 extra keys, 2 tiles": 0, "3 extra keys, 3 tiles": 3}),
    "remap": ("remap", {"G 8": 1, "G 9": 0, "G 16": 1}), "refusal": ("path", {"n 96": 2, "n 100": 0, "h 16, n 50": 0, "h 64": 2, "h 128": 0}),
    "residue, one-hot": ("path", {"one token, two keys": 2, "five sequences with a table": 2, "forty tokens, two key tiles": 2}),
    "residue, single key": ("perWave", {"a sequence per wave": 1, "sixteen heads": 0}),
}


@pytest.mark.parametrize("seed", plan.SEEDS["bwd32"])
def test_constructed_backward_pairs_land_on_their_sides(seed):
    _lib.load()
    groups = _groups("bwd32", seed)
    assert set(groups) == set(BWD_SIDES), set(groups) ^ set(BWD_SIDES)
    for name, (field, sides) in BWD_SIDES.items():
        got = {side: plan.route_bwd(c)[field] for side, c in groups[name].items()}
        assert got == sides, (name, field, got)
    for side, c in groups["remap"].items():
        r = plan.route_bwd(c)
        assert r["path"] == 2 and r["nkt"] >= 3 and not r["perWave"], (side, r)
    for side, c in groups["refusal"].items():
        r = plan.route_bwd(c)
        assert (r["err"] != 0) == (r["path"] == 0), r
    # (the KW groups stay off the seq path, the perWave ones too)
    for name in ("KW G 2", "KW G 16", "KW G 300", "KW G 600", "perWave G", "perWave Mt", "EV count", "EV tiles"):
        assert all(plan.route_bwd(c)["path"] == 2 for c in groups[name].values()), name
    lab = plan.labelled("bwd32", seed)
    r = plan.route_bwd(lab["perWave, VALU null key, h 3"])
    assert (r["path"], r["KW"], r["perWave"], r["EV"], r["nkt"]) == (2, 0, 1, 1, 1), r
    r = plan.route_bwd(lab["n_self 0, one extra key"])
    assert (r["path"], r["EV"], r["nkt"]) == (2, 1, 1), r


@pytest.mark.parametrize("seed", plan.SEEDS["fwd16"])
def test_constructed_16_bit_pairs_land_on_their_sides(seed):
    _lib.load()
    lab = plan.labelled("fwd16", seed)
    waves = lambda k: plan.route_fwd16(lab[k])["waves"]
    assert waves("four waves: n h 4095") == 8 and waves("four waves: n h 4096") == 4
    assert lab["four waves: n h 4095"].n * lab["four waves: n h 4095"].h == 4095 and lab["four waves: n h 4096"].n * lab["four waves: n h 4096"].h == 4096
    assert waves("n h 4096 with a table") == 8 and waves("n h 4096 at d 32") == 8 and waves("four waves, ragged last workgroup") == 4
    assert plan.route_fwd16(lab["four waves: n h 4096"])["rows"] == 128 and plan.route_fwd16(lab["four waves: n h 4095"])["rows"] == 256
    assert (plan.keys(lab["tile keys: 64"]), plan.keys(lab["tile keys: 65"])) == (64, 65)
    assert (lab["query rows: 256"].n * lab["query rows: 256"].h, lab["query rows: 257"].n * lab["query rows: 257"].h) == (256, 257)


@pytest.mark.parametrize("seed", plan.SEEDS["fwd32"])
def test_constructed_forward_pairs_land_on_their_sides(seed):
    lab = plan.labelled("fwd32", seed)
    rows = lambda k: lab[k].n * lab[k].h
    assert (rows("query rows: 128"), rows("query rows: 129")) == (128, 129)
    assert (plan.keys(lab["tile keys: 32"]), plan.keys(lab["tile keys: 33"])) == (32, 33) and lab["tile keys: 32"].E != 1
    a, b = lab["tile keys behind a VALU null key: 32"], lab["tile keys behind a VALU null key: 33"]
    assert (a.E, a.ns, b.E, b.ns) == (1, 32, 1, 33)
    c = lab["causal row 0 sees one key"]
    assert c.causal and c.E == 0
    assert 32 % lab["h 5 does not divide 32"].h != 0


def test_fused_ok_agrees_with_the_route_query(all_cases):
    refused = 0
    for c in all_cases["bwd32"]:
        r = plan.route_bwd(c)
        assert plan.fused_ok(c) == (r["path"] != 0), (c, r)
        refused += r["path"] == 0
    assert refused >= 3
    # what the Attention module asks before it chooses the fused path, at shapes next to every refusal of the plan function
    from diffusioniqt_amd import ops
    for G, n, h, d, has_rel in ((1, 96, 8, 64, 1), (1, 100, 8, 64, 1), (1, 100, 8, 64, 0), (65535, 4, 2, 32, 1), (65536, 4, 2, 32, 1), (2, 8, 2, 48, 0),
                                (2, 8, 2, 128, 1), (1, 769, 1, 32, 1), (1, 768, 1, 32, 1), (2, 4, 64, 32, 1), (2, 4, 65, 32, 1), (2, 4, 65, 32, 0)):
        path = _lib.query("diqt_mqa_attention_bwd_route", G, n, h, d, 1, n, has_rel, has_rel, 0)
        assert bool(ops.mqa_attention_fused_ok(G, n, h, d, n, bool(has_rel))) == (path != 0), (G, n, h, d, has_rel, path)


def test_the_seq_kernel_leaves_tensors_of_2_gib_to_the_two_kernel_path():
    """mqa_seq_bwd_kernel addresses `out` through a buffer resource of G n h d 4 bytes < 2^31: (8192, 32, 32, 64) is exactly 2^31 -- a shape
    no GPU test can afford -- and must take the two-kernel path; half of it takes the seq kernel."""
    _lib.load()
    q = lambda G, f: _lib.query("diqt_mqa_attention_bwd_route", G, 32, 32, 64, 1, 32, 0, 1, f)
    assert q(8192, 0) == 2 and q(8192, 4) == 1          # two-kernel, a sequence per wave
    assert q(4096, 0) == 1 and q(8191, 0) == 1
    # with a table the LDS bound refuses h = 32 first; the byte bound must hold there too
    assert _lib.query("diqt_mqa_attention_bwd_route", 8192, 16, 32, 64, 1, 16, 1, 1, 0) == 2


def test_budgets(all_cases):
    for fam, seeds in plan.SEEDS.items():
        assert len(seeds) == 3
        for seed in seeds:
            cs = plan.cases(fam, seed)
            total = sum(plan.ref_macs(c) for c in cs)
            print("%s seed %d: %d cases, %.3g multiply-adds of float64 reference" % (fam, seed, len(cs), total))
            assert total <= plan.MAX_MACS_SEED, (fam, seed, total)
            for c in cs:
                assert plan.ref_macs(c) <= plan.MAX_MACS_CASE, (c, plan.ref_macs(c))
                assert plan.largest_tensor_bytes(c) <= plan.MAX_TENSOR_BYTES, c
                if c.entry == "bwd" and plan.route_bwd(c)["path"]:
                    nws = _lib.query("diqt_mqa_attention_bwd_workspace_bytes", c.G, c.n, c.h, c.d, c.E, c.ns, int(c.rel))
                    assert 0 < nws <= plan.MAX_TENSOR_BYTES, (c, nws)
            assert cs == plan.cases(fam, seed), "the generator is not a function of the seed"


def test_workspace_rows_cover_the_seq_kernel(all_cases):
    """"nwg * 4 <= rows": the one-pass kernel writes 4 rows of bias-gradient partials per workgroup into the workspace sized for the
    two-kernel path (rows = 4 x the dQ grid)"""
    n = 0
    for c in all_cases["bwd32"]:
        r = plan.route_bwd(c)
        if r["path"] != 1:
            continue
        rows = r["rows"]
        tbl = (2 * c.ns - 1) * c.h if c.rel else 0
        assert r["nwg"] * 4 <= rows
        assert _lib.query("diqt_mqa_attention_bwd_workspace_bytes", c.G, c.n, c.h, c.d, c.E, c.ns, int(c.rel)) == 4 * (c.G * c.n * c.h + rows * tbl + rows * 32)
        n += 1
    assert n >= 3


def test_a_refused_route_query_leaves_the_last_error_alone():
    lib = _lib.load()
    assert lib.diqt_act_fwd(None, None, 16, 1, None) == -2
    before = lib.diqt_last_error()
    assert lib.diqt_mqa_attention_bwd_route(1, 100, 8, 64, 1, 100, 1, 1, 1) == -3 and lib.diqt_mqa_attention_bwd_route(2, 4, 128, 32, 1, 4, 0, 1, 0) == 0
    assert lib.diqt_last_error() == before and b"null pointer" in before
