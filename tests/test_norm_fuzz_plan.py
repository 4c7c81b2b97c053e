"""Which kernels and branches the normalisation / soft-max fuzz reaches, proved on the CPU from the library's own route queries
(diqt_softmax_route, diqt_colreduce_route, diqt_gn_apply_route, diqt_attn_softmax_bwd_workspace_bytes): ``pytest -s`` prints the
cases-per-target tables."""
import collections

import pytest

from diffusioniqt_amd import _lib
from tests import norm_fuzz_plan as plan


@pytest.fixture(scope="module")
def all_cases():
    _lib.load()
    return {fam: [c for seed in plan.SEEDS[fam] for c in plan.cases(fam, seed)] for fam in plan.SEEDS}


def _colreduce_targets(c):
    r = plan.colreduce_of(c)
    if r is None or plan.expect(c)[0]:
        return []
    t = ["colreduce " + ("channel quads" if r["vec"] else "scalar"), "nblk " + ("1" if r["nblk"] == 1 else "256" if r["nblk"] == 256 else "2 to 255")]
    return t + (["empty trailing workgroups"] if r["empty"] else [])


def gn_targets(c):
    err, _ = plan.expect(c)
    t = ["entry " + c.entry, "data " + c.data]
    if err:
        return t + ["refusal: %s, code %d" % (c.entry, err)]
    t += _colreduce_targets(c)
    if c.entry in ("fwd", "fwd_h") + plan.GN_BWD:
        t.append("apply " + ("vectorised" if plan.apply_route(c)["vec"] else "scalar"))
        t.append("act %d %s" % (c.act, "fwd" if c.entry.startswith("fwd") else "bwd"))
    if c.entry not in ("stats", "stats_fp"):
        t.append("scale / shift " + {0: "absent", c.C: "in two tensors", 2 * c.C: "in halves of a [B, 2C] row"}[c.cs])
        t.append("gamma / beta " + ("present" if c.gb else "absent"))
    if c.nblk:
        t.append("partials nblk %d" % c.nblk)
    if c.entry in plan.GN_BWD:
        t.append("dx_add " + ("given" if c.add else "null"))
        t += ["null " + {"g": "dgamma", "b": "dbeta", "s": "dscale / dshift"}[n] for n in c.null if n != "s" or c.cs]
    if c.C % 4 == 0 and (c.C // c.G) % 4:
        t.append("a channel quad spans groups")
    t.append("G " + ("1" if c.G == 1 else "C" if c.G == c.C else "between"))
    if c.mis and not err:
        t.append("misaligned %s runs" % c.mis)
    if c.entry == "fwd_h":
        t.append("fwd_h %s x_half %d" % ("bf16" if c.bf16 else "fp16", c.x_half))
    if c.entry == "bwd_h" and (c.xt or c.dyt) and not c.nblk and not plan.colreduce_of(c)["vec"]:
        t.append("16-bit x or dy behind the scalar colreduce")
    if c.entry == "bwd_h":
        t.append("bwd_h types (%d, %d, %d)%s" % (c.xt, c.dxt, c.dyt, " compile-time" if (c.xt, c.dxt, c.dyt) in plan.TRIPLES_CT else ""))
    return t


_COL = ["colreduce channel quads", "colreduce scalar", "nblk 1", "nblk 2 to 255", "nblk 256", "empty trailing workgroups"]
GN32_REACHABLE = (["entry " + e for e in ("stats", "stats_coef", "stats_fp", "coef_fp", "coef", "fwd", "bwd", "bwd_fp", "bwd_ex")] +
                  ["data " + d for d in plan.DATA["gn32"] + ("const",)] + _COL + ["apply vectorised", "apply scalar"] +
                  ["act %d %s" % (a, w) for a in plan.ACTS for w in ("fwd", "bwd")] +
                  ["scale / shift absent", "scale / shift in two tensors", "scale / shift in halves of a [B, 2C] row", "gamma / beta present", "gamma / beta absent"] +
                  ["partials nblk %d" % n for n in (1, 7, 64, 65, 256, 2048)] + ["dx_add given", "dx_add null", "null dgamma", "null dbeta", "null dscale / dshift",
                   "a channel quad spans groups", "G 1", "G C", "G between", "misaligned x runs", "misaligned y runs", "misaligned dx runs", "misaligned add runs",
                   "misaligned dy runs", "refusal: stats, code -2", "refusal: stats_coef, code -2", "refusal: bwd, code -2", "refusal: bwd_ex, code -2"])
GN16_REACHABLE = (["entry fwd_h", "entry bwd_h"] + ["data " + d for d in plan.DATA["gn16"]] + _COL + ["apply vectorised", "apply scalar"] +
                  ["fwd_h %s x_half %d" % (t, x) for t in ("fp16", "bf16") for x in (0, 1)] +
                  ["bwd_h types (%d, %d, %d) compile-time" % t for t in plan.TRIPLES_CT] + ["bwd_h types (%d, %d, %d)" % t for t in plan.TRIPLES_RT] +
                  ["refusal: fwd_h, code -3", "refusal: bwd_h, code -3", "16-bit x or dy behind the scalar colreduce", "dx_add given", "dx_add null", "a channel quad spans groups"])


def softmax_targets(c):
    err, _ = plan.expect(c)
    if err:
        return ["refusal: scale 0 in the backward"]
    if c.outer == 0:
        return ["outer 0"]
    return ["forward " + plan.SOFTMAX_ROUTES[plan.softmax_route(c, 0)], "backward " + plan.SOFTMAX_ROUTES[plan.softmax_route(c, 1)], "data " + c.data,
            "scale %g" % c.scale] + (["long row with a tail (n % 1024)"] if plan.softmax_route(c, 0) == 0 and c.n % 1024 else []) + \
           (["wave per row with a tail (n % 64)"] if plan.softmax_route(c, 0) == 1 and c.n % 64 else []) + \
           (["column workgroup with a ragged last sweep"] if plan.softmax_route(c, 0) == 2 and c.n % (1024 // c.inner) else [])


SOFTMAX_REACHABLE = (["forward " + v for v in plan.SOFTMAX_ROUTES.values()] + ["backward " + plan.SOFTMAX_ROUTES[r] for r in (0, 1, 3)] +
                     ["data " + d for d in plan.DATA["softmax"]] + ["scale 1", "scale 0.25", "scale -0.5", "outer 0", "refusal: scale 0 in the backward",
                      "long row with a tail (n % 1024)", "wave per row with a tail (n % 64)", "column workgroup with a ragged last sweep"])


def rows_targets(c):
    err, _ = plan.expect(c)
    t = ["entry " + c.entry, "data " + c.data]
    if err:
        return t + ["refusal: %s%s, code %d" % (c.entry, ", misaligned " + c.mis if getattr(c, "mis", "") else "", err)]
    if c.entry == "ln_fwd":
        t += ["ln_fwd bias %d" % c.bias, "ln_fwd residual %d" % c.res, "ln_fwd statistics %d" % c.stats, "C " + ("<= 64" if c.C <= 64 else "> 64")]
    if c.entry == "ln_bwd":
        t += _colreduce_targets(c) + ["ln_bwd dx_add %d" % c.add, "ln_bwd " + ("dx only" if not c.dg else "dg and db" if c.db else "dg only")]
        if c.mis:
            t.append("ln_bwd misaligned %s runs" % c.mis)
    if c.entry == "l2":
        t += ["l2 d %s 16" % ("<" if c.d < 16 else "=" if c.d == 16 else ">"), "l2 rows %% 16 %s" % ("= 0" if c.rows % 16 == 0 else "!= 0"),
              "l2 strides " + ("packed" if c.xs == c.ys == c.dxs == c.d else "all different" if len({c.xs, c.ys, c.dxs}) == 3 else "padded")]
        t += ["l2 zero row"] if c.zero else []
        t += ["l2 without inv"] if not c.inv else []
    if c.entry in ("asm_fwd", "asm_bwd"):
        M = c.E + c.ns
        t += ["%s M %s 64" % (c.entry, "<" if M < 64 else "=" if M == 64 else ">"), "%s h %d" % (c.entry, c.h), "%s n_extra %s" % (c.entry, c.E if c.E < 2 else "> 1"),
              "%s rel %d null %d causal %d" % (c.entry, c.rel, c.null, c.causal)]
    if c.entry == "asm_bwd":
        t.append("asm_bwd " + ("table" if plan.asm_table(c) else "atomics" if (c.rel or c.null) else "no bias gradient"))
        t.append("asm_bwd through " + ("_ws" if c.ws else "the plain entry"))
    return t


ROWS_REACHABLE = (["entry " + e for e in ("ln_fwd", "ln_bwd", "l2", "asm_fwd", "asm_bwd")] + ["data " + d for d in plan.DATA["rows"]] + _COL +
                  ["ln_fwd %s %d" % (w, v) for w in ("bias", "residual", "statistics") for v in (0, 1)] + ["C <= 64", "C > 64", "ln_bwd dx_add 0", "ln_bwd dx_add 1",
                   "ln_bwd dx only", "ln_bwd dg only", "ln_bwd dg and db", "ln_bwd misaligned dy runs", "refusal: ln_bwd, misaligned ws, code -2",
                   "refusal: ln_bwd, misaligned dy, code -2", "refusal: asm_fwd, code -1", "refusal: asm_bwd, code -1", "l2 d < 16", "l2 d = 16", "l2 d > 16",
                   "l2 rows % 16 = 0", "l2 rows % 16 != 0", "l2 strides packed", "l2 strides all different", "l2 zero row", "l2 without inv",
                   "asm_bwd table", "asm_bwd atomics", "asm_bwd no bias gradient", "asm_bwd through _ws", "asm_bwd through the plain entry"] +
                  ["%s M %s 64" % (e, s) for e in ("asm_fwd", "asm_bwd") for s in "<=>"] + ["%s h %d" % (e, h) for e in ("asm_fwd", "asm_bwd") for h in (1, 3, 8)] +
                  ["%s n_extra %s" % (e, v) for e in ("asm_fwd", "asm_bwd") for v in ("0", "1", "> 1")] +
                  ["%s rel %d null %d causal %d" % (e, *b) for e in ("asm_fwd", "asm_bwd") for b in ((1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 0, 0), (1, 0, 1), (0, 1, 1))])


@pytest.mark.parametrize("family,targets,reachable", [("gn32", gn_targets, GN32_REACHABLE), ("gn16", gn_targets, GN16_REACHABLE),
                                                      ("softmax", softmax_targets, SOFTMAX_REACHABLE), ("rows", rows_targets, ROWS_REACHABLE)])
def test_every_reachable_target_is_hit_three_times(all_cases, family, targets, reachable):
    count = collections.Counter(t for c in all_cases[family] for t in targets(c))
    print("\n%s: %d cases over seeds %s" % (family, len(all_cases[family]), plan.SEEDS[family]))
    for t in sorted(set(count) | set(reachable)):
        print("  %-60s %4d" % (t, count[t]))
    assert not [t for t in reachable if count[t] < 3], {t: count[t] for t in reachable if count[t] < 3}


def _groups(family, seed):
    g = collections.defaultdict(dict)
    for label, c in plan.labelled(family, seed).items():
        if ": " in label:
            name, side = label.split(": ", 1)
            g[name][side] = c
    return g


@pytest.mark.parametrize("seed", plan.SEEDS["gn32"])
def test_constructed_groupnorm_pairs_land_on_their_sides(seed):
    _lib.load()
    g = _groups("gn32", seed)
    nblk = {side: plan.colreduce_of(c)["nblk"] for side, c in g["nblk"].items()}
    assert nblk == {"rows 1": 1, "rows 63": 1, "rows 64": 1, "rows 127": 1, "rows 128": 2, "rows 831": 12, "rows 4159": 64, "rows 16383": 255,
                    "rows 16384": 256, "rows 16385": 256}, nblk
    assert {s: plan.colreduce_of(c)["rows_per"] for s, c in g["nblk"].items() if s in ("rows 16384", "rows 16385")} == {"rows 16384": 64, "rows 16385": 65}
    assert {s: plan.colreduce_of(c)["empty"] for s, c in g["empty tail"].items()} == {"rows 16384": False, "rows 16385": True}
    # with 16385 rows the workgroups 253 to 255 start past the last row
    r = plan.colreduce_of(g["empty tail"]["rows 16385"])
    assert [b for b in range(r["nblk"]) if b * r["rows_per"] >= 16385] == [253, 254, 255]
    assert {s: plan.colreduce_of(c)["vec"] for s, c in g["colreduce path"].items()} == {
        "C 4, stats": 1, "C 4, bwd": 1, "C 6, stats": 0, "C 6, bwd": 0, "C 1024, stats": 1, "C 1024, bwd": 1, "C 1028, stats": 0, "C 1028, bwd": 0}
    # C = 1028: a scalar reduce in front of a vectorised apply on a grid that is a multiple of 257; C = 192: a multiple of 3
    a = plan.apply_route(g["colreduce path"]["C 1028, bwd"])
    assert a["vec"] == 1 and a["grid"] % 257 == 0 and plan.apply_route(plan.gn("fwd", B=3, rows=216, C=192, G=8))["grid"] % 3 == 0
    assert {s: plan.col_route(64, int(s.split()[1].rstrip(",")))["rpar"] for s in ("C 4,", "C 12,", "C 192,", "C 260,", "C 1024,")} == {
        "C 4,": 256, "C 12,": 85, "C 192,": 5, "C 260,": 3, "C 1024,": 1}
    lab = plan.labelled("gn32", seed)
    assert plan.apply_route(lab["aligned x: fwd"])["vec"] == 1 and plan.apply_route(lab["misaligned x: fwd"])["vec"] == 0
    assert plan.expect(lab["misaligned x: stats, C 6"])[0] == 0 and plan.expect(lab["misaligned x: stats, C 64 (refusal)"])[0] == plan.E_ALIGN
    assert plan.expect(lab["misaligned x: bwd, C 64 (refusal)"])[0] == plan.E_ALIGN and plan.expect(lab["misaligned dx: bwd, C 1028"])[0] == 0
    assert plan.expect(lab["misaligned dx_add: bwd_ex, partials"])[0] == 0 and plan.expect(lab["misaligned dy: bwd, C 6"])[0] == 0
    for c in g["quad straddles two groups"].values():
        assert c.C % 4 == 0 and (c.C // c.G) % 4 != 0
    for c in g["residue"].values():
        assert plan.residue(c)


@pytest.mark.parametrize("seed", plan.SEEDS["softmax"])
def test_constructed_softmax_pairs_land_on_their_sides(seed):
    _lib.load()
    g = _groups("softmax", seed)
    routes = lambda name: {side: (plan.softmax_route(c, 0), plan.softmax_route(c, 1)) for side, c in g[name].items()}
    assert routes("long row n") == {"4095": (1, 1), "4096": (0, 0)}
    assert routes("long row outer") == {"1024": (0, 0), "1025": (1, 1)}
    assert routes("column workgroup n") == {"63": (3, 3), "64": (2, 3)}
    assert routes("column workgroup inner") == {"64": (2, 3), "96": (3, 3), "1024": (2, 3), "2048": (3, 3)}
    assert routes("column workgroup outer") == {"65535": (2, 3), "65536": (3, 3)}
    big = g["column workgroup outer"]["65536"]
    assert plan.largest_tensor_bytes(big) == 32 << 20


@pytest.mark.parametrize("seed", plan.SEEDS["rows"])
def test_constructed_row_pairs_land_on_their_sides(seed):
    _lib.load()
    g = _groups("rows", seed)
    assert {s: plan.asm_table(c) for s, c in g["table"].items()} == {"n_self 192": True, "n_self 193": False}
    assert all(c.h == 8 and c.rel for c in g["table"].values())
    codes = {s: plan.expect(c)[0] for s, c in g["ln_bwd alignment"].items()}
    assert codes == {"aligned": 0, "misaligned workspace (refusal)": plan.E_ALIGN, "misaligned dy, C 64 (refusal)": plan.E_ALIGN,
                     "misaligned dy, C 64, no db": 0, "misaligned dy, C 63": 0, "misaligned dy, C 1100": 0}, codes
    assert plan.colreduce_of(g["ln_bwd empty tail"]["rows 16385"])["empty"]
    assert all(plan.expect(c)[0] == plan.E_SHAPE for c in g["refusal"].values()) and len(g["refusal"]) == 3


@pytest.mark.parametrize("seed", plan.SEEDS["gn16"])
def test_constructed_16_bit_cases(seed):
    _lib.load()
    lab = plan.labelled("gn16", seed)
    assert plan.expect(lab["refusal: fwd_h C 6"])[0] == plan.E_UNSUPPORTED and plan.expect(lab["refusal: bwd_h C 6"])[0] == plan.E_UNSUPPORTED
    assert plan.expect(lab["fp32 through bwd_h, C 6"])[0] == 0
    assert plan.colreduce_of(lab["bwd_h at 16385 rows"])["empty"]
    for k, c in lab.items():
        if k.startswith("16-bit behind the scalar reduce"):
            assert plan.colreduce_of(c)["vec"] == 0 and plan.apply_route(c)["vec"] == 1 and plan.expect(c)[0] == 0 and (c.xt or c.dyt)


REFUSABLE = {"gn32": ("stats", "stats_coef", "bwd", "bwd_ex"), "gn16": ("fwd_h", "bwd_h"), "softmax": ("softmax",), "rows": ("ln_bwd", "asm_fwd", "asm_bwd")}


def test_budgets(all_cases):
    for fam, seeds in plan.SEEDS.items():
        assert len(seeds) == 3
        for seed in seeds:
            cs = plan.cases(fam, seed)
            total = sum(plan.ref_elems(c) for c in cs)
            refused = [c for c in cs if plan.expect(c)[0]]
            print("%s seed %d: %d cases, %d refusals, %.3g reference elements" % (fam, seed, len(cs), len(refused), total))
            assert total <= plan.MAX_ELEMS_SEED, (fam, seed, total)
            for c in cs:
                assert plan.ref_elems(c) <= plan.MAX_ELEMS_CASE, (c, plan.ref_elems(c))
                assert plan.largest_tensor_bytes(c) <= plan.MAX_TENSOR_BYTES, c
                assert set(plan.expect(c)[1]) <= set(plan.TAGS)
            assert cs == plan.cases(fam, seed), "the generator is not a function of the seed"
        fam_cases = all_cases[fam]
        refused = [c for c in fam_cases if plan.expect(c)[0]]
        assert len(refused) <= 0.1 * len(fam_cases), (fam, len(refused), len(fam_cases))
        assert {c.entry for c in refused} >= set(REFUSABLE[fam]), (fam, {c.entry for c in refused})


def test_misalignment_only_where_the_launcher_reads_it(all_cases):
    """a tensor goes in 4 bytes off only where vec_ok or an aligned16 requirement looks at it: x, y of the forward apply; x, dy, dx, dx_add of
    the GroupNorm backwards; x of the statistics; the workspace and dy of the LayerNorm backward"""
    reads = {"fwd": {"x", "y"}, "stats": {"x"}, "stats_coef": {"x"}, "bwd": {"x", "dy", "dx"}, "bwd_ex": {"x", "dy", "dx", "add"}, "ln_bwd": {"ws", "dy"}}
    n = 0
    for cs in all_cases.values():
        for c in cs:
            mis = getattr(c, "mis", "")
            if mis:
                assert mis in reads.get(c.entry, ()), c
                n += 1
    assert n >= 3


def test_a_route_query_leaves_the_last_error_alone():
    lib = _lib.load()
    assert lib.diqt_act_fwd(None, None, 16, 1, None) == -2
    before = lib.diqt_last_error()
    assert lib.diqt_softmax_route(3, 0, 1, 0) == -1 and lib.diqt_colreduce_route(0, 4, 0) == -1 and lib.diqt_gn_apply_route(1, 1, 4, 1, 7) == -1
    assert lib.diqt_last_error() == before and b"null pointer" in before
