"""Case generator, router and float64 reference of the fused multi-query attention fuzz (tests/attn_fuzz_worker.py runs the cases on the
GPU, tests/test_attn_fuzz_plan.py proves on the CPU which kernels and branches they reach).  Needs no GPU: the routes come from the
library's own shape queries diqt_mqa_attention_bwd_route / diqt_mqa_attention_fwd_h_route -- the plan functions the launchers themselves
call -- never from a restatement here.

Families (three seeds each):

* ``fwd32``: diqt_mqa_attention_fwd (entry "fwd"), diqt_mqa_attention_fwd_lse ("lse") and diqt_mqa_attention_fwd_frames ("frames": a case
  carries G = B * P sequences of n = F frames behind one null key).
* ``bwd32``: diqt_mqa_attention_fwd_lse then diqt_mqa_attention_bwd.  One constructed pair per threshold of attn_bwd_plan, at the smallest
  shape that flips it; about one case in twenty is a refusal.  The seq kernel's bound ``G n h d 4 < 2^31`` needs multi-GiB tensors: it is
  covered on the CPU only (test_attn_fuzz_plan.py asks the query at (8192, 32, 32, 64) with a table: two-kernel path).
* ``fwd16``: diqt_cast_to_h + diqt_mqa_attention_fwd_h, fp16 and bf16, round_out 0 and 1.

A case with ``rep`` > 1 holds G / rep distinct sequences ``rep`` times: the kernels see G sequences (what their dispatch depends on), the
float64 reference is evaluated for the distinct ones only.  Repeat r holds them rolled by r places (``tile``), so a kernel that reads or
writes sequence g +- k G / rep instead of g meets other data.  That is how the G >= 512 thresholds stay inside the budget.

Data classes, drawn per case: "randn"; "peaked" (q x 8: scores of standard deviation ~8); "late" / "first" (component 0 of every query
lifted by 4 and one key -- in the last key tile / the first key -- lifted there so that its score stands ln(M - 1) + 4 above the rest: it
takes ~98 % of the probability, and the online soft-max rescales by e^-(ln(M - 1) + 4) at the last tile / never again after the first).
The height follows from the conditioning of the backward: dS = P (dP - delta) cancels to 1 - p_max of its operands, so the fp32 rounding
of dP and delta = rowsum(dO . O) reaches dq, dk and the bias gradients amplified by 1 / (1 - p_max); at 2 % that is 50 x 2^-24 ~ 3e-6,
inside the project's 1e-4.  A fifth class, "onehot" (the last key 12 above the rest whatever M: 1 - p_max ~ 1e-5), and cases with a single
key in total (p = 1: every gradient through the soft-max is exactly zero) are not drawn but constructed, labelled ``residue``: there the
kernels return the rounding residue of dP - delta, which the relative rule cannot judge (max|ref| is itself a residue, or zero), and
the worker judges dq, dk, drel and dnull by the rule PLUS a ceiling derived from the number formats (attn_fuzz_worker.residue_ceiling);
out, lse, dv, the guards, the launches and the two-run identity are judged as everywhere.

Budgets (test_attn_fuzz_plan.py checks them): float64 reference work ``G/rep n h M d`` multiply-adds per einsum x 2 einsums (forward) or
6 (forward and autograd), <= 3e8 per case and <= 4e9 per seed; no tensor above 64 MiB.
"""
import collections
import math
import random

import torch

from diffusioniqt_amd import _lib, ops

MAX_MACS_CASE = 3e8
MAX_MACS_SEED = 4e9
MAX_TENSOR_BYTES = 64 << 20
SEEDS = {"fwd32": (41, 42, 43), "bwd32": (51, 52, 53), "fwd16": (61, 62, 63)}
DATA = ("randn", "peaked", "late", "first")

# entry: "fwd" | "lse" | "frames" (fwd32), "bwd" (bwd32), "h" (fwd16).  E = n_extra, ns = n_self.  frames: P pixels, G = B * P, E = 1, ns = n = F.
Case = collections.namedtuple("Case", "entry G n h d E ns rel null causal data rep P bf16 round_out")

BWD_FIELDS = ("path", "err", "nwg", "KW", "perWave", "EV", "nkt", "relLds", "remap", "dkvGy", "rows")
PATHS = {0: "refused", 1: "seq", 2: "two-kernel"}
BWD_TAGS = ("mqa_attention_bwd(seq)", "mqa_attention_bwd(seq, bias reduce)", "mqa_attention_bwd(dq)", "mqa_attention_bwd(bias reduce)",
            "mqa_attention_bwd(dkv)")


def case(entry, G, n, h, d, E=1, ns=None, rel=False, null=False, causal=False, data="randn", rep=1, P=0, bf16=0, round_out=1):
    c = Case(entry, G, n, h, d, E, n if ns is None else ns, bool(rel), bool(null), bool(causal), data, rep, P, bf16, round_out)
    assert c.G % c.rep == 0 and (c.ns == c.n or not (c.rel or c.causal)) and (c.E >= 1 or not c.null) and c.E + c.ns > 0, c
    return c


def keys(c):
    return c.E + c.ns


def ref_macs(c):
    """multiply-adds of the float64 reference: two einsums, and four more for their autograd"""
    return (c.G // c.rep) * c.n * c.h * keys(c) * c.d * (6 if c.entry == "bwd" else 2)


def largest_tensor_bytes(c):
    return 4 * c.G * max(c.n * c.h * c.d, keys(c) * 2 * c.d)


def route_bwd(c):
    """attn_bwd_plan's answer for the case, by field name"""
    args = (c.G, c.n, c.h, c.d, c.E, c.ns, int(c.rel), int(c.null))
    return {f: _lib.query("diqt_mqa_attention_bwd_route", *args, i) for i, f in enumerate(BWD_FIELDS)}


def bwd_tags(r, c):
    """{census tag: launches} of one diqt_mqa_attention_bwd call"""
    bias = c.rel or c.null
    if r["path"] == 1:
        return {"mqa_attention_bwd(seq)": 1, **({"mqa_attention_bwd(seq, bias reduce)": 1} if bias else {})}
    if r["path"] == 2:
        return {"mqa_attention_bwd(dq)": 1, "mqa_attention_bwd(dkv)": 1, **({"mqa_attention_bwd(bias reduce)": 1} if bias else {})}
    return {}


def route_fwd16(c):
    q = lambda f: _lib.query("diqt_mqa_attention_fwd_h_route", c.n, c.h, c.d, int(c.rel), f)
    return {"waves": q(0), "rows": q(1), "hasrel": q(2)}


def fused_ok(c):
    return bool(ops.mqa_attention_fused_ok(c.G, c.n, c.h, c.d, c.ns, c.rel))


def describe(c):
    if c.entry == "bwd":
        r = route_bwd(c)
        if r["path"] != 2:
            return PATHS[r["path"]] + (" nwg=%d" % r["nwg"] if r["path"] else " err=%d" % r["err"])
        return "two-kernel KW=%d EV=%d nkt=%d relLds=%d remap=%d" % (r["KW"], r["EV"], r["nkt"], r["relLds"], r["remap"])
    if c.entry == "h":
        return "%d waves" % route_fwd16(c)["waves"]
    return c.entry


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference: Attention.forward's products (imagen_video.py:483-520) on whatever dtype the operands carry (float64 in the tests)
# ---------------------------------------------------------------------------------------------------------------------------------
def mqa_scores(q, kv, rel, nb, n, h, d, E, causal, scale, n_self=None):
    """sim[G, n, h, E + n_self]: scale q k^T, the T5-style relative bias on the self keys (needs n_self == n), null_bias on the last extra
    key, -inf on causally masked keys.  ``scale`` None: q carries it already."""
    ns = n if n_self is None else n_self
    G = q.shape[0]
    sim = torch.einsum('gihd,gjd->gihj', q.reshape(G, n, h, d), kv[..., :d])
    if scale is not None:
        sim = sim * scale
    parts = [sim[..., :E], sim[..., E:]]
    if nb is not None:
        parts[0] = torch.cat((sim[..., :E - 1], sim[..., E - 1:E] + nb[None, None, :, None]), dim=-1)
    if rel is not None:
        i = torch.arange(n)[:, None]; j = torch.arange(n)[None, :]
        parts[1] = parts[1] + rel[(i - j + n - 1)].permute(0, 2, 1)[None]                   # [1, n, h, n] indexed (i, hh, j)
    sim = torch.cat(parts, dim=-1)
    if causal:
        i = torch.arange(n)[:, None]; j = torch.arange(n)[None, :]
        mask = torch.cat((torch.zeros(n, E, dtype=torch.bool), j > i), dim=1)[None, :, None, :]
        sim = sim.masked_fill(mask, float('-inf'))
    return sim


def mqa_ref(q, kv, rel, nb, n, h, d, E, causal, scale, n_self=None, with_lse=False):
    """out[G, n, h d] (and the row log-sum-exp [G, n h]); autograd gives the gradients when the operands are leaves that require grad"""
    sim = mqa_scores(q, kv, rel, nb, n, h, d, E, causal, scale, n_self)
    out = torch.einsum('gihj,gjd->gihd', sim.softmax(dim=-1), kv[..., d:]).reshape(q.shape[0], n, h * d)
    return (out, torch.logsumexp(sim, dim=-1).reshape(q.shape[0], n * h)) if with_lse else out


def inputs(c, gen):
    """fp32 host tensors of the G / rep distinct sequences: q [Gu, n, h d], kv [Gu, E + ns, 2 d], rel, null_bias, dout"""
    Gu, M, d = c.G // c.rep, keys(c), c.d
    q = torch.randn(Gu, c.n, c.h * d, generator=gen)
    kv = torch.randn(Gu, M, 2 * d, generator=gen)
    rel = torch.randn(2 * c.n - 1, c.h, generator=gen) if c.rel else None
    nb = torch.randn(c.h, generator=gen) if c.null else None
    up = torch.randn(Gu, c.n, c.h * d, generator=gen)
    if c.entry == "frames":
        kv[:, 0] = kv[0, 0].clone()         # the one learned null row in front of every sequence
    if c.data == "peaked":
        q = q * 8.0
    elif c.data == "onehot":
        q.view(Gu, c.n, c.h, d)[..., 0] += 4.0
        kv[:, M - 1, 0] = 12.0 * d ** 0.5 / 4.0
    elif c.data in ("late", "first"):
        jstar = M - 1 - int(torch.randint(0, min(M, 8), (1,), generator=gen)) if c.data == "late" else 0
        q.view(Gu, c.n, c.h, d)[..., 0] += 4.0
        kv[:, jstar, 0] = (math.log(max(M - 1, 1)) + 4.0) * d ** 0.5 / 4.0
    return q, kv, rel, nb, up


def tile(t, rep):
    """[Gu, ...] -> [rep Gu, ...]: repeat r is the block rolled by r places along the sequence axis"""
    return t if rep == 1 else torch.cat([t.roll(-r, 0) for r in range(rep)], dim=0)


def residue(c):
    """a constructed case whose soft-max is one-hot: see the module docstring"""
    return c.entry == "bwd" and (c.data == "onehot" or keys(c) == 1)


# ---------------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------------
def fixed_bwd32(rnd):
    """{label: case}; a label "<name>: <side>" belongs to the pair / group <name> (test_attn_fuzz_plan.py checks the sides)"""
    b = lambda *a, **k: case("bwd", *a, **k)
    coin = lambda: rnd.random() < 0.5
    bias = lambda: dict(zip(("rel", "null", "causal"), rnd.choice([(0, 0, 0), (1, 1, 1), (1, 1, 0), (0, 1, 0), (1, 0, 1), (0, 0, 1)])))
    dat = lambda: rnd.choice(DATA)
    f = {}
    # the one-pass short-sequence kernel: n_extra == 1, n <= 32, 32 % h == 0, G >= 512, LDS <= 160 KiB
    f["seq G: 511"] = b(511, 8, 2, 32, **bias(), data=dat())
    f["seq G: 512"] = b(512, 8, 2, 32, **bias(), data=dat())
    f["seq n: 32"] = b(512, 32, 2, 32, **bias(), data=dat(), rep=4)
    f["seq n: 33"] = b(512, 33, 2, 32, **bias(), data=dat(), rep=4)
    f["seq h: 3"] = b(512, 8, 3, 32, **bias(), data=dat())
    f["seq h: 4"] = b(512, 8, 4, 32, **bias(), data=dat())
    f["seq n_extra: 1"] = b(512, 8, 2, 32, E=1, **bias(), data=dat())
    f["seq n_extra: 2"] = b(512, 8, 2, 32, E=2, **bias(), data=dat())
    f["seq LDS: n 24"] = b(512, 24, 16, 64, rel=True, null=coin(), causal=coin(), rep=16)
    f["seq LDS: n 32"] = b(512, 32, 16, 64, rel=True, null=coin(), causal=coin(), rep=16)
    f["seq, 256 workgroups walk 1030 sequences"] = b(1030, 5, 2, 32, **bias(), data=dat())
    f["seq, 256 workgroups walk 2300 sequences"] = b(2300, 7, 4, 64, **bias(), data=dat(), rep=4)
    f["seq no bias"] = b(516, 20, 4, 64, data=dat(), rep=4)
    f["seq null bias without a table"] = b(514, 7, 2, 32, null=True, causal=coin(), data=dat())
    f["seq table without a null bias"] = b(513, 9, 8, 32, rel=True, causal=coin(), data=dat())
    # a sequence per wave of the dK/dV kernel: Mt <= 32 and G >= 2048 (off the seq path: no extra key, two, or heads that do not divide 32)
    f["perWave G: 2047"] = b(2047, 5, 2, 32, E=0, causal=coin(), data=dat())
    f["perWave G: 2048"] = b(2048, 5, 2, 32, E=0, causal=coin(), data=dat())
    f["perWave, two extra keys through the tile"] = b(2051, 5, 1, 32, E=2, **bias(), data=dat())
    f["perWave, VALU null key, h 3"] = b(2050, 6, 3, 32, E=1, **bias(), data=dat())
    f["perWave Mt: 32"] = b(2048, 32, 1, 32, E=0, data=dat(), rep=8)
    f["perWave Mt: 33"] = b(2048, 33, 1, 32, E=0, data=dat(), rep=8)
    # KW from Mt (32 | 33 | 64 | 65) and the loop that halves it while (key-tile workgroups) x G < 512
    for G, E, rep in ((2, 1, 1), (16, 1, 1), (600, 0, 8), (300, 1, 4)):
        for Mt in (32, 33, 64, 65):
            f["KW G %d: Mt %d" % (G, Mt)] = b(G, Mt, 2, 32, E=E, **(bias() if E else {"causal": coin()}), data=dat(), rep=rep)
    # extra keys on the VALU: n_extra == 1, or n_extra <= 8 and n_extra <= ceil(n_self / 32)
    f["EV count: 8 of 8"] = b(2, 256, 1, 32, E=8, **bias(), data=dat())
    f["EV count: 9"] = b(2, 288, 1, 32, E=9, **bias(), data=dat())
    f["EV tiles: 3 extra keys, 2 tiles"] = b(2, 64, 2, 32, E=3, **bias(), data=dat())
    f["EV tiles: 3 extra keys, 3 tiles"] = b(2, 65, 2, 32, E=3, **bias(), data=dat())
    # only extra keys
    f["n_self 0, one extra key"] = b(3, 7, 3, 32, E=1, ns=0, null=coin(), data=dat())
    f["n_self 0, five extra keys"] = b(3, 40, 4, 64, E=5, ns=0, null=coin(), data=dat())
    f["n_self 0, one extra key, a sequence per wave"] = b(2049, 3, 2, 32, E=1, ns=0, null=True)
    f["n_self != n"] = b(5, 20, 3, 32, E=2, ns=45, null=coin(), data=dat())
    f["no extra key"] = b(4, 37, 5, 64, E=0, rel=coin(), causal=coin(), data=dat())
    # the XCD remap of the dK/dV kernel: grid.y % 8 == 0, three key-tile workgroups per batch entry
    for G in (8, 9, 16):
        f["remap: G %d" % G] = b(G, 70, 2, 32, E=1, **bias(), data=dat())
    # null bias without a table: the dK/dV kernel reads it from global memory
    f["null bias without a table, two key tiles"] = b(3, 50, 3, 64, E=2, null=True, causal=coin(), data=dat())
    f["null bias without a table, VALU extra keys"] = b(2, 70, 5, 32, E=3, null=True, data=dat())
    # the table must fit the dQ kernel's LDS budget: (2 n - 1) h <= 1536
    f["refusal: n 96"] = b(1, 96, 8, 32, rel=True, null=coin(), causal=coin(), data=dat())
    f["refusal: n 100"] = b(1, 100, 8, 32, rel=True, null=coin(), causal=coin(), data=dat())
    f["refusal: h 16, n 50"] = b(2, 50, 16, 64, rel=True, null=True)
    # found by this fuzz: the bias reduce keeps 256 h floats in LDS without raising the 64-KiB default, so 128 heads with a null bias failed
    # at its launch, after the dQ kernel had run; the entry point now refuses more than 64 heads and ops.mqa_attention_fused_ok agrees
    f["refusal: h 64"] = b(2, 4, 64, 32, rel=True, null=True, causal=coin(), data=dat())
    f["refusal: h 128"] = b(2, 4, 128, 32, rel=True, null=True)
    # found by this fuzz: a one-token, two-key case with the key 12 above the rest showed dq off by 2.9e-3 of its maximum (fp32 PyTorch autograd
    # on the CPU: 5.5e-4; fp32 PyTorch of the kernel's formula with delta = rowsum(dO . O): 9.0e-3), and single-key cases ~1e-5 where the
    # reference is exactly zero: rounding residue of dP - delta, judged with residue_ceiling
    f["residue, one-hot: one token, two keys"] = b(1, 1, 4, 64, E=1, ns=1, data="onehot")
    f["residue, one-hot: five sequences with a table"] = b(5, 1, 4, 64, E=1, ns=1, rel=True, data="onehot")
    f["residue, one-hot: forty tokens, two key tiles"] = b(3, 40, 4, 32, E=1, rel=True, null=True, causal=coin(), data="onehot")
    f["residue, single key: a sequence per wave"] = b(2051, 1, 3, 64, E=0, ns=1, rel=True, data="first")
    f["residue, single key: sixteen heads"] = b(8, 1, 16, 64, E=0, ns=1, rel=True, data="peaked")
    return f


def fixed_fwd32(rnd):
    coin = lambda: rnd.random() < 0.5
    dat = lambda: rnd.choice(DATA)
    ent = lambda: rnd.choice(["fwd", "lse"])
    f = {}
    f["query rows: 128"] = case(ent(), 2, 32, 4, 64, rel=coin(), null=coin(), causal=coin(), data=dat())
    f["query rows: 129"] = case(ent(), 2, 43, 3, 64, rel=coin(), null=coin(), causal=coin(), data=dat())
    f["tile keys: 32"] = case(ent(), 3, 30, 2, 32, E=2, rel=coin(), null=coin(), data=dat())
    f["tile keys: 33"] = case(ent(), 3, 31, 2, 32, E=2, rel=coin(), null=coin(), data=dat())
    f["tile keys behind a VALU null key: 32"] = case(ent(), 3, 32, 2, 32, E=1, rel=coin(), null=coin(), data=dat())
    f["tile keys behind a VALU null key: 33"] = case(ent(), 3, 33, 2, 32, E=1, rel=coin(), null=coin(), data=dat())
    f["causal row 0 sees one key"] = case(ent(), 2, 40, 3, 32, E=0, rel=coin(), causal=True, data=dat())
    f["one token, one key"] = case(ent(), 2, 1, 5, 64, E=0)
    f["h 5 does not divide 32"] = case(ent(), 2, 27, 5, 64, rel=True, null=True, causal=coin(), data=dat())
    f["n_self 0, one extra key"] = case(ent(), 3, 9, 3, 32, E=1, ns=0, null=coin())
    f["n_self 0, five extra keys"] = case(ent(), 2, 50, 4, 64, E=5, ns=0, null=coin(), data=dat())
    f["n_self != n"] = case(ent(), 3, 20, 3, 32, E=2, ns=77, null=coin(), data=dat())
    f["null bias without a table (fwd)"] = case("fwd", 2, 70, 4, 64, E=3, null=True, causal=coin(), data=dat())
    f["null bias without a table (lse)"] = case("lse", 2, 33, 8, 32, E=1, null=True, data=dat())
    f["table without a null bias"] = case(ent(), 2, 33, 2, 64, E=1, rel=True, causal=coin(), data=dat())
    for i, (B, F, P) in enumerate(((1, 7, 33), (2, 32, 7), (1, 33, 5), (7, 64, 3), (33, 1, 2), (1, 64, 1), (2, 5, 64), (1, 32, 32))):
        f["frames B %d F %d P %d" % (B, F, P)] = case("frames", B * P, F, rnd.choice([1, 2, 3, 8]), rnd.choice([32, 64]), P=P, rel=i % 2 == 0,
                                                      null=i % 4 < 2, causal=i % 3 == 0, data=dat())
    return f


def fixed_fwd16(rnd):
    coin = lambda: rnd.random() < 0.5
    dat = lambda: rnd.choice(DATA)
    hp = lambda: dict(bf16=rnd.randint(0, 1), round_out=rnd.randint(0, 1))
    f = {}
    # (n_self != n keeps the reference of the long-sequence cases inside the budget: the threshold looks at the query rows only)
    f["four waves: n h 4095"] = case("h", 1, 1365, 3, 64, E=rnd.choice([0, 1, 5]), ns=rnd.choice([64, 200]), data=dat(), **hp())
    f["four waves: n h 4096"] = case("h", 1, 512, 8, 64, E=rnd.choice([0, 1, 5]), causal=coin(), data=dat(), **hp())
    f["four waves, n h 4096, few keys"] = case("h", 2, 1024, 4, 64, E=1, ns=rnd.choice([63, 64, 130]), null=coin(), data=dat(), **hp())
    f["n h 4096 with a table"] = case("h", 1, 512, 8, 64, rel=True, null=coin(), causal=coin(), data=dat(), **hp())
    f["n h 4096 at d 32"] = case("h", 1, 512, 8, 32, causal=coin(), data=dat(), **hp())
    f["four waves, ragged last workgroup"] = case("h", 2, 1030, 4, 64, E=2, ns=70, null=coin(), data=dat(), **hp())
    f["tile keys: 64"] = case("h", 3, 63, 2, 32, E=1, rel=coin(), null=coin(), causal=coin(), data=dat(), **hp())
    f["tile keys: 65"] = case("h", 3, 64, 2, 32, E=1, rel=coin(), null=coin(), causal=coin(), data=dat(), **hp())
    f["query rows: 256"] = case("h", 2, 64, 4, 64, rel=coin(), null=coin(), causal=coin(), data=dat(), **hp())
    f["query rows: 257"] = case("h", 2, 257, 1, 64, rel=coin(), null=coin(), causal=coin(), data=dat(), **hp())
    f["n_self 0, one extra key"] = case("h", 3, 9, 3, 32, E=1, ns=0, null=coin(), **hp())
    f["n_self != n"] = case("h", 3, 20, 3, 64, E=2, ns=130, null=coin(), data=dat(), **hp())
    f["null bias without a table"] = case("h", 2, 70, 4, 64, E=3, null=True, causal=coin(), data=dat(), **hp())
    f["causal row 0 sees one key"] = case("h", 2, 40, 3, 32, E=0, causal=True, data=dat(), **hp())
    return f


_NS = [1, 1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129]


def _draw(rnd, entry):
    d, h = rnd.choice([32, 64]), rnd.choice([1, 2, 3, 4, 5, 8, 16])
    n = rnd.choice(_NS) if rnd.random() < 0.5 else rnd.randint(1, 300)
    E = rnd.randint(0, 9) if rnd.random() < 0.6 else 1
    rel, null, causal = rnd.random() < 0.4, rnd.random() < 0.5, rnd.random() < 0.4
    ns = n
    if not (rel or causal) and rnd.random() < 0.35:
        ns = 0 if rnd.random() < 0.3 else rnd.randint(1, 300)
    if E == 0:
        null = False
        if ns == 0:
            ns = n
    G = rnd.choice([1, 1, 2, 3, 5, 8, 9, 16, 24, 40])
    if entry == "bwd" and n <= 40 and rnd.random() < 0.5:          # many short sequences: the seq kernel, a sequence per wave
        G = rnd.choice([300, 512, 515, 700, 2048, 2051, 2300])
    data = rnd.choice(DATA)
    hp = dict(bf16=rnd.randint(0, 1), round_out=rnd.randint(0, 1)) if entry == "h" else {}
    return case(entry, G, n, h, d, E=E, ns=ns, rel=rel, null=null, causal=causal, data=data, **hp)


def _draw_frames(rnd):
    B, F = rnd.choice([1, 7, 32, 33, 64]), rnd.choice([1, 7, 32, 33, 64])
    P = rnd.choice([1, 3, 5, 7, 11, 30, 33, 64])
    return case("frames", B * P, F, rnd.choice([1, 2, 3, 4, 5, 8, 16]), rnd.choice([32, 64]), P=P, rel=rnd.random() < 0.5, null=rnd.random() < 0.5,
                causal=rnd.random() < 0.5, data=rnd.choice(DATA))


def _fits(c, budget):
    return ref_macs(c) <= min(MAX_MACS_CASE, budget) and largest_tensor_bytes(c) <= MAX_TENSOR_BYTES


N_RANDOM = {"fwd32": 70, "bwd32": 60, "fwd16": 60}


def cases(family, seed):
    rnd = random.Random(seed)
    fixed = {"fwd32": fixed_fwd32, "bwd32": fixed_bwd32, "fwd16": fixed_fwd16}[family](rnd)
    out = list(fixed.values())
    budget = MAX_MACS_SEED - sum(ref_macs(c) for c in out)
    left = N_RANDOM[family]
    while left > 0:
        if family == "fwd32":
            c = _draw_frames(rnd) if rnd.random() < 0.3 else _draw(rnd, rnd.choice(["fwd", "lse"]))
        else:
            c = _draw(rnd, "bwd" if family == "bwd32" else "h")
        if not _fits(c, budget / left) or (family == "bwd32" and keys(c) == 1):
            continue
        out.append(c)
        budget -= ref_macs(c)
        left -= 1
    return out


def labelled(family, seed):
    return {"fwd32": fixed_fwd32, "bwd32": fixed_bwd32, "fwd16": fixed_fwd16}[family](random.Random(seed))
