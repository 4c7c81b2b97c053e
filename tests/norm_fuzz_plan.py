"""Case generator, router and float64 references of the normalisation / soft-max fuzz (tests/norm_fuzz_worker.py runs the cases on the GPU
through the C entry points of csrc/elementwise.hip, tests/test_norm_fuzz_plan.py proves on the CPU which kernels and branches they reach).
Needs no GPU: every route comes from the shape queries the launchers themselves call (diqt_softmax_route, diqt_colreduce_route,
diqt_gn_apply_route, diqt_attn_softmax_bwd_workspace_bytes), never from a restatement here.

Families (three seeds each; a case is ``Case(entry, data, kv)``, its parameters readable as attributes):

* ``gn32``: "stats" diqt_groupnorm_stats, "stats_coef" diqt_groupnorm_stats_coef, "stats_fp" diqt_groupnorm_stats_from_partials, "coef_fp"
  diqt_gn_coef_from_partials, "coef" diqt_gn_coef, "fwd" diqt_gn_act_fwd, "bwd" diqt_gn_act_bwd, "bwd_fp" diqt_gn_act_bwd_from_partials,
  "bwd_ex" diqt_gn_act_bwd_ex (``nblk`` > 0: with partials; ``add``: with dx_add).
* ``gn16``: "fwd_h" diqt_gn_act_fwd_h (``bf16``, ``x_half``), "bwd_h" diqt_gn_act_bwd_h (``xt``, ``dxt``, ``dyt``: 0 fp32, 1 fp16, 2 bf16).
  16-bit inputs are fp32 draws rounded to the type; the reference uses the rounded values.
* ``softmax``: "softmax" diqt_softmax_fwd then diqt_softmax_bwd on [outer][n][inner].
* ``rows``: "ln_fwd" diqt_chan_layernorm_fwd_res, "ln_bwd" diqt_chan_layernorm_bwd_ex, "l2" diqt_l2norm_rows_fwd then _bwd, "asm_fwd"
  diqt_attn_softmax_fwd, "asm_bwd" diqt_attn_softmax_bwd_ws (``ws`` 1) or diqt_attn_softmax_bwd (``ws`` 0).

The entries that apply statistics (fwd, bwd*, coef, ln_bwd) receive mean and rstd computed in float64 and rounded to fp32, so their
verdict does not depend on the statistics kernels; the partials of the ``*_fp`` entries are float64 block sums rounded to fp32.

Data classes.  gn32 / gn16: "randn"; "offset" (every group's mean four of its standard deviations from zero: E[x^2] - m^2 cancels to 1/17);
"tiny" (values ~1e-3: eps = 1e-5 carries the variance); "wide" (standard deviation 30 -- x itself for the statistics entries, gamma x 30 for
the entries that apply given statistics, because the normalisation would undo a wide x: Mish and SiLU then saturate on both sides);
"const" (group (0, 0) constant: variance exactly 0, rstd = eps^-1/2) is never drawn but constructed and labelled ``residue``: A x + Bc then
cancels two products 316 times larger than their difference, and the worker adds the ceiling ``residue_ceiling`` to the project's rule.
The backwards never see a group of fewer than four values (``gn`` adds rows): with one value the variance is exactly 0, with two or three
the projection leaves the exact dx (nearly) zero, and the kernels return the residue r u |A dz|.  Under ReLU, dy is zero wherever z lies within rounding of the jump of the derivative (gn_inputs).
softmax: "randn"; "wide" (x 30: most exponentials underflow); "peaked" (one entry 40 above the rest); "masked" (up to half the entries
-inf, never a whole row); "flat" (constant rows).  rows: "randn", "offset" (x + 4), "wide" (x 30; the attention soft-max backward, whose
exact result would be a rounding residue on one-hot rows, keeps standard normal scores).

``mis``: the named tensor is handed over 4 bytes off a 16-byte boundary -- only on entries whose launcher reads that tensor's alignment
(vec_ok, or an aligned16 requirement); ``expect`` then says whether the scalar kernels run or the call is refused.

Budgets (test_norm_fuzz_plan.py checks them): no tensor above 64 MiB, at most 2e7 reference elements per case and 4e8 per seed; refusals at
most 10 % of a family's cases and at least one per refusable entry.
"""
import collections
import random

import torch

from diffusioniqt_amd import _lib

MAX_ELEMS_CASE = 2e7
MAX_ELEMS_SEED = 4e8
MAX_TENSOR_BYTES = 64 << 20
SEEDS = {"gn32": (71, 72, 73), "gn16": (81, 82, 83), "softmax": (91, 92, 93), "rows": (101, 102, 103)}
DATA = {"gn32": ("randn", "offset", "tiny", "wide"), "gn16": ("randn", "offset", "wide"), "softmax": ("randn", "wide", "peaked", "masked", "flat"),
        "rows": ("randn", "offset", "wide")}
ACTS = (0, 1, 2, 3, 4, 5)                      # none, Mish, SiLU, GELU, ReLU, sigmoid (include/diqt.h)
E_SHAPE, E_ALIGN, E_UNSUPPORTED = -1, -2, -3
EPS = 1e-5
HDT = {1: torch.float16, 2: torch.bfloat16}
GN_STATS, GN_BWD = ("stats", "stats_coef"), ("bwd", "bwd_fp", "bwd_ex", "bwd_h")
# the (x, dx, dy) types gn_act_bwd_impl instantiates at compile time, and two that fall to the run-time kernel
TRIPLES_CT = ((0, 0, 1), (0, 0, 2), (1, 1, 1), (2, 2, 2), (1, 1, 0), (2, 2, 0))
TRIPLES_RT = ((0, 1, 0), (1, 1, 2))
SOFTMAX_ROUTES = {0: "long row", 1: "wave per row", 2: "column workgroup", 3: "thread per column"}


class Case(collections.namedtuple("Case", "entry data kv")):
    __slots__ = ()

    def __getattr__(self, k):
        for a, b in self.kv:
            if a == k:
                return b
        raise AttributeError(k)


def _case(entry, data, defaults, kw):
    assert not set(kw) - set(defaults), set(kw) - set(defaults)
    return Case(entry, data, tuple(sorted({**defaults, **kw}.items())))


_GN = dict(B=2, rows=64, C=64, G=8, cs=0, gb=1, act=1, nblk=0, add=0, null="", mis="", xt=0, dxt=0, dyt=0, bf16=0, x_half=0)


def gn(entry, data="randn", **kw):
    c = _case(entry, data, _GN, kw)
    if entry not in ("stats", "stats_coef", "stats_fp", "coef_fp") and c.rows * (c.C // c.G) == 1 and data != "const":
        # one value per group: variance exactly 0, the residue class -- constructed on purpose only ("const"); two rows instead
        return gn(entry, data, **{**kw, "rows": 2})
    if entry in GN_BWD and c.rows * (c.C // c.G) < 4:
        # ... and with two or three values per group the projection leaves dx (nearly) nothing but that residue: four at least
        return gn(entry, data, **{**kw, "rows": -(-4 // (c.C // c.G))})
    assert not c.add or entry in ("bwd_ex", "bwd_h"), c
    assert c.C % c.G == 0 and c.cs in (0, c.C, 2 * c.C) and (c.nblk > 0) == (entry in ("stats_fp", "coef_fp", "bwd_fp") or (entry in ("bwd_ex", "bwd_h") and c.nblk > 0)), c
    return c


def softmax(outer, n, inner, scale=1.0, data="randn", refuse=0):
    return _case("softmax", data, dict(outer=0, n=1, inner=1, scale=1.0, refuse=0), dict(outer=outer, n=n, inner=inner, scale=scale, refuse=refuse))


def ln(entry, rows, C, data="randn", **kw):
    return _case(entry, data, dict(rows=1, C=1, bias=1, res=0, stats=1, add=0, dg=1, db=1, mis=""), dict(rows=rows, C=C, **kw))


def l2(rows, d, xs=None, ys=None, dxs=None, inv=1, zero=0, data="randn"):
    return _case("l2", data, dict(rows=1, d=1, xs=1, ys=1, dxs=1, inv=1, zero=0),
                 dict(rows=rows, d=d, xs=xs or d, ys=ys or d, dxs=dxs or d, inv=inv, zero=zero))


def asm(entry, G, n, h, E=1, ns=None, rel=0, null=0, causal=0, ws=1, data="randn"):
    return _case(entry, data, dict(G=1, n=1, h=1, E=1, ns=1, rel=0, null=0, causal=0, ws=1),
                 dict(G=G, n=n, h=h, E=E, ns=n if ns is None else ns, rel=int(rel), null=int(null), causal=int(causal), ws=ws))


# ---------------------------------------------------------------------------------------------------------------------------------
# routes: the launchers' own answers
# ---------------------------------------------------------------------------------------------------------------------------------
def col_route(rows, C):
    r = {f: _lib.query("diqt_colreduce_route", rows, C, i) for i, f in enumerate(("nblk", "rows_per", "vec", "rpar"))}
    r["empty"] = (r["nblk"] - 1) * r["rows_per"] >= rows          # the last workgroup starts at or past `rows`
    # the longest fp32 addition chain behind one partial: rows a thread adds up, plus the row groups a workgroup combines through LDS
    r["chain"] = -(-r["rows_per"] // r["rpar"]) + r["rpar"] if r["vec"] else r["rows_per"]
    return r


def apply_route(c):
    aligned = int(not (getattr(c, "mis", "") and c.mis in ("x", "y", "dy", "dx", "add")))
    return {"vec": _lib.query("diqt_gn_apply_route", c.B, c.rows, c.C, aligned, 0), "grid": _lib.query("diqt_gn_apply_route", c.B, c.rows, c.C, aligned, 1)}


def softmax_route(c, backward):
    return _lib.query("diqt_softmax_route", c.outer, c.n, c.inner, int(backward))


def asm_table(c):
    """the deterministic LDS-table kernel (True) or the global-atomics kernel of the relative-bias gradient"""
    return bool(c.ws and (c.rel or c.null) and _lib.query("diqt_attn_softmax_bwd_workspace_bytes", c.G, c.n, c.h, c.E, c.ns) > 0)


def colreduce_of(c):
    """the colreduce_kernel route of the case, or None where the entry launches none"""
    if c.entry in GN_STATS or (c.entry in GN_BWD and c.nblk == 0):
        return col_route(c.rows, c.C)
    if c.entry == "ln_bwd" and c.dg:
        return col_route(c.rows, c.C)
    return None


def expect(c):
    """(error code, {census tag: launches}) of one call of the case's entry (the two calls of "softmax" and "l2" together)"""
    e = c.entry
    if e in GN_STATS:
        if c.mis == "x" and c.C % 4 == 0:
            return E_ALIGN, {}
        tag = "groupnorm_" + e
        return 0, {tag + "/reduce": 1, tag + "/final": 1}
    if e in ("stats_fp", "coef_fp", "coef"):
        return 0, {{"stats_fp": "groupnorm_stats_from_partials", "coef_fp": "gn_coef_from_partials", "coef": "gn_coef"}[e]: 1}
    if e == "fwd":
        return 0, {"gn_act_fwd": 1}
    if e == "fwd_h":
        return (0, {"gn_act_fwd_h": 1}) if apply_route(c)["vec"] else (E_UNSUPPORTED, {})
    if e in GN_BWD:
        vec = apply_route(c)["vec"]
        if not vec and (c.xt or c.dxt or c.dyt):
            return E_UNSUPPORTED, {}
        if not c.nblk and not vec and col_route(c.rows, c.C)["vec"]:
            return E_ALIGN, {}
        return 0, {**({} if c.nblk else {"gn_act_bwd/reduce": 1}), "gn_act_bwd/sum": 1, "gn_act_bwd/final": 1, "gn_act_bwd/dx": 1}
    if e == "softmax":
        if c.refuse:
            return E_SHAPE, {"softmax_fwd": 1}
        return 0, ({"softmax_fwd": 1, "softmax_bwd": 1} if c.outer else {})
    if e == "ln_fwd":
        return 0, {"chan_layernorm_fwd": 1}
    if e == "ln_bwd":
        if c.dg and (c.mis == "ws" or (c.mis == "dy" and c.db and col_route(c.rows, c.C)["vec"])):
            return E_ALIGN, {}
        t = {"chan_layernorm_bwd/dx": 1}
        if c.dg:
            t.update({"chan_layernorm_bwd/dg": 1, "chan_layernorm_bwd/dg-final": 1})
            if c.db:
                t.update({"chan_layernorm_bwd/db": 1, "chan_layernorm_bwd/db-final": 1})
        return 0, t
    if e == "l2":
        return 0, {"l2norm_rows_fwd": 1, **({"l2norm_rows_bwd": 1} if c.inv else {})}
    if e == "asm_fwd":
        bad = ((c.causal or c.rel) and c.ns != c.n) or (c.null and c.E < 1)
        return (E_SHAPE, {}) if bad else (0, {"attn_softmax_fwd": 1})
    if e == "asm_bwd":
        if (c.rel and c.ns != c.n) or (c.null and c.E < 1):
            return E_SHAPE, {}
        return 0, ({"attn_softmax_bwd(table)": 1, "attn_softmax_bwd(reduce)": 1} if asm_table(c) else {"attn_softmax_bwd": 1})
    raise ValueError(e)


TAGS = ("groupnorm_stats/reduce", "groupnorm_stats/final", "groupnorm_stats_coef/reduce", "groupnorm_stats_coef/final",
        "groupnorm_stats_from_partials", "gn_coef_from_partials", "gn_coef", "gn_act_fwd", "gn_act_fwd_h", "gn_act_bwd/reduce", "gn_act_bwd/sum",
        "gn_act_bwd/final", "gn_act_bwd/dx", "softmax_fwd", "softmax_bwd", "chan_layernorm_fwd", "chan_layernorm_bwd/dx", "chan_layernorm_bwd/dg",
        "chan_layernorm_bwd/dg-final", "chan_layernorm_bwd/db", "chan_layernorm_bwd/db-final", "l2norm_rows_fwd", "l2norm_rows_bwd",
        "attn_softmax_fwd", "attn_softmax_bwd(table)", "attn_softmax_bwd(reduce)", "attn_softmax_bwd")


def ref_elems(c):
    """elements the float64 reference walks (the largest tensor of the case)"""
    e = c.entry
    if e in ("coef", "coef_fp", "stats_fp", "bwd_fp"):
        part = c.B * max(c.nblk, 1) * 2 * c.C
        return max(part, c.B * c.rows * c.C if e == "bwd_fp" else 0)
    if e in _GN_ENTRIES:
        return c.B * c.rows * c.C
    if e == "softmax":
        return c.outer * c.n * c.inner
    if e in ("ln_fwd", "ln_bwd"):
        return c.rows * c.C
    if e == "l2":
        return c.rows * max(c.xs, c.ys, c.dxs)
    return c.G * c.n * c.h * (c.E + c.ns)


def largest_tensor_bytes(c):
    if c.entry in _GN_ENTRIES:
        return 4 * max(c.B * c.rows * c.C if c.entry not in ("coef", "coef_fp", "stats_fp") else 0, c.B * max(c.nblk, 1) * 2 * c.C,
                       _lib.query("diqt_reduce_workspace_bytes", c.B, c.C) // 4)
    return 4 * ref_elems(c)


_GN_ENTRIES = ("stats", "stats_coef", "stats_fp", "coef_fp", "coef", "fwd", "bwd", "bwd_fp", "bwd_ex", "fwd_h", "bwd_h")


def residue(c):
    return c.data == "const"


def describe(c):
    err, tags = expect(c)
    if err:
        return "refused %d" % err
    r = colreduce_of(c)
    s = []
    if r:
        s.append("colreduce %s nblk=%d rows_per=%d%s" % ("vec" if r["vec"] else "scalar", r["nblk"], r["rows_per"], " empty-tail" if r["empty"] else ""))
    if c.entry in ("fwd", "fwd_h") + GN_BWD:
        a = apply_route(c)
        s.append("apply %s grid=%d" % ("vec" if a["vec"] else "scalar", a["grid"]))
    if c.entry == "softmax":
        s.append("fwd %s, bwd %s" % (SOFTMAX_ROUTES[softmax_route(c, 0)], SOFTMAX_ROUTES[softmax_route(c, 1)]))
    if c.entry == "asm_bwd":
        s.append("table" if asm_table(c) else "atomics")
    return ", ".join(s) or c.entry


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs (fp32 host tensors) and float64 references
# ---------------------------------------------------------------------------------------------------------------------------------
def act_ref(z, act):
    F = torch.nn.functional
    return {0: lambda t: t, 1: F.mish, 2: F.silu, 3: F.gelu, 4: F.relu, 5: torch.sigmoid}[act](z)


def act_grad_ref(z, act):
    if not act:
        return torch.ones_like(z)
    z = z.detach().clone().requires_grad_()
    act_ref(z, act).sum().backward()
    return z.grad


def _round(t, ty):
    return t.to(HDT[ty]).float() if ty else t


def gn_inputs(c, gen):
    B, rows, C, G = c.B, c.rows, c.C, c.G
    Cg = C // G
    r = lambda *s: torch.randn(*s, generator=gen)
    applies = c.entry not in ("stats", "stats_coef", "stats_fp", "coef_fp")
    x = r(B, rows, C)
    if c.data == "offset":
        s = 0.5 + 1.5 * torch.rand(B, 1, G, generator=gen)
        sign = torch.where(torch.rand(B, 1, G, generator=gen) < 0.5, -1.0, 1.0)
        x = (x.view(B, rows, G, Cg) * s[..., None] + (4.0 * s * sign)[..., None]).reshape(B, rows, C)
    elif c.data == "tiny":
        x = x * 1e-3
    elif c.data == "wide" and not applies:
        x = x * 30.0
    elif c.data == "const":
        x.view(B, rows, G, Cg)[0, :, 0, :] = 1.7
    x = _round(x, c.xt if c.entry == "bwd_h" else (2 if c.bf16 else 1) if (c.entry == "fwd_h" and c.x_half) else 0)
    d = {"x": x}
    if c.gb:
        d["gamma"] = (1.0 + 0.3 * r(C)) * (30.0 if c.data == "wide" and applies else 1.0)
        d["beta"] = 0.3 * r(C)
    if c.cs:
        d["emb"] = 0.3 * r(B, 2 * C)          # scale = emb[:, :C], shift = emb[:, C:] (cs == C: two tensors of their own)
    if c.entry in GN_BWD:
        d["dy"] = _round(r(B, rows, C), c.dyt)
        if c.act == 4:
            # ReLU's derivative jumps at z = 0: where the exact z lies within 64 u (|A x| + |Bc| + 1) of it -- eight times what fp32 can
            # misplace it by -- the upstream gradient is zero, so both values of the derivative give the same dz
            m, _, rs, _, _ = gn_stats_ref(x, G)
            A, Bc = gn_coef_ref(c, d, m.float(), rs.float())
            Ax = A[:, None] * x.double()
            d["dy"] = d["dy"].masked_fill((Ax + Bc[:, None]).abs() <= 64 * 2.0 ** -24 * (Ax.abs() + Bc[:, None].abs() + 1.0), 0.0)
        if c.add:
            d["add"] = r(B, rows, C)
    return d


def gn_stats_ref(x, G, eps=EPS):
    """float64 (mean, var, rstd, E|x|, E[x^2]) per (b, g) of x [B, rows, C]"""
    B, rows, C = x.shape
    xg = x.double().view(B, rows, G, C // G).permute(0, 2, 1, 3).reshape(B, G, -1)
    m = xg.mean(-1)
    var = ((xg - m[..., None]) ** 2).mean(-1)
    return m, var, (var + eps).rsqrt(), xg.abs().mean(-1), (xg * xg).mean(-1)


def gn_terms(c, d, mean, rstd):
    """float64 per-(b, c) factors: mean, rstd expanded to channels, gamma, beta, 1 + scale, shift"""
    B, C, G = c.B, c.C, c.G
    ex = lambda t: t.double().repeat_interleave(C // G, dim=1)
    ga = d["gamma"].double()[None] if c.gb else torch.ones(1, C, dtype=torch.float64)
    be = d["beta"].double()[None] if c.gb else torch.zeros(1, C, dtype=torch.float64)
    sc = 1.0 + d["emb"].double()[:, :C] if c.cs else torch.ones(B, C, dtype=torch.float64)
    sf = d["emb"].double()[:, C:] if c.cs else torch.zeros(B, C, dtype=torch.float64)
    return ex(mean), ex(rstd), ga, be, sc, sf


def gn_coef_ref(c, d, mean, rstd):
    m, r, ga, be, sc, sf = gn_terms(c, d, mean, rstd)
    return torch.stack((r * ga * sc, (be - m * r * ga) * sc + sf))          # [2, B, C]


def gn_fwd_ref(c, d, mean, rstd):
    m, r, ga, be, sc, sf = gn_terms(c, d, mean, rstd)
    xhat = (d["x"].double() - m[:, None]) * r[:, None]
    return act_ref((xhat * ga[:, None] + be[:, None]) * sc[:, None] + sf[:, None], c.act)


def gn_bwd_sums(c, d, mean, rstd):
    """(dz, xhat, S1 = sum_rows dz, S2 = sum_rows dz xhat) in float64"""
    m, r, ga, be, sc, sf = gn_terms(c, d, mean, rstd)
    xhat = (d["x"].double() - m[:, None]) * r[:, None]
    z = (xhat * ga[:, None] + be[:, None]) * sc[:, None] + sf[:, None]
    dz = d["dy"].double() * act_grad_ref(z, c.act)
    return dz, xhat, dz.sum(1), (dz * xhat).sum(1)


def gn_bwd_ref(c, d, mean, rstd):
    m, r, ga, be, sc, sf = gn_terms(c, d, mean, rstd)
    dz, xhat, S1, S2 = gn_bwd_sums(c, d, mean, rstd)
    B, C, G = c.B, c.C, c.G
    count = c.rows * (C // G)
    grp = lambda t: (t.view(B, G, C // G).sum(-1) / count).repeat_interleave(C // G, dim=1)
    m1, m2 = grp(ga * sc * S1), grp(ga * sc * S2)
    dx = r[:, None] * (ga[:, None] * sc[:, None] * dz - m1[:, None] - xhat * m2[:, None])
    if c.add:
        dx = dx + d["add"].double()
    return {"dx": dx, "dgamma": (sc * S2).sum(0), "dbeta": (sc * S1).sum(0), "dscale": ga * S2 + be * S1, "dshift": S1}


def block_sums(a, b, nblk):
    """partial[B][nblk][2][C]: float64 sums of a and b [B, rows, C] over nblk row blocks of ceil(rows / nblk) rows, rounded to fp32"""
    B, rows, C = a.shape
    per = -(-rows // nblk)
    out = torch.zeros(B, nblk, 2, C, dtype=torch.float64)
    for k in range(min(nblk, -(-rows // per))):
        out[:, k, 0] = a[:, k * per:(k + 1) * per].sum(1)
        out[:, k, 1] = b[:, k * per:(k + 1) * per].sum(1)
    return out.float()


def softmax_inputs(c, gen):
    shape = (c.outer, c.n, c.inner)
    x = torch.randn(*shape, generator=gen)
    if c.data == "wide":
        x = x * 30.0
    elif c.data == "peaked":
        j = torch.randint(0, c.n, (c.outer, 1, c.inner), generator=gen)
        x.scatter_(1, j, x.gather(1, j) + 40.0)
    elif c.data == "masked":
        keep = torch.randint(0, c.n, (c.outer, 1, c.inner), generator=gen)
        drop = torch.rand(*shape, generator=gen) < 0.5 * torch.rand(c.outer, 1, c.inner, generator=gen)
        drop.scatter_(1, keep, False)
        x = x.masked_fill(drop, float("-inf"))
    elif c.data == "flat":
        x = torch.randn(c.outer, 1, c.inner, generator=gen).expand(*shape).contiguous()
    return {"x": x, "dy": torch.randn(*shape, generator=gen)}


def softmax_ref(c, d):
    y = torch.softmax(d["x"].double(), dim=1) * c.scale
    y32 = y.float()                                                    # what the backward is given
    yd, dy = y32.double(), d["dy"].double()
    return {"y": y, "y32": y32, "dx": yd * (dy - (yd * dy).sum(1, keepdim=True) / c.scale)}


def ln_inputs(c, gen):
    r = lambda *s: torch.randn(*s, generator=gen)
    x = r(c.rows, c.C)
    if c.data == "offset":
        x = x + 4.0
    elif c.data == "wide":
        x = x * 30.0
    d = {"x": x, "g": 1.0 + 0.3 * r(c.C)}
    if c.entry == "ln_fwd":
        if c.bias:
            d["b"] = 0.3 * r(c.C)
        if c.res:
            d["res"] = r(c.rows, c.C)
    else:
        d["dy"] = r(c.rows, c.C)
        if c.add:
            d["add"] = r(c.rows, c.C)
    return d


def ln_stats_ref(x, eps=EPS):
    x = x.double()
    m = x.mean(1)
    return m, (((x - m[:, None]) ** 2).mean(1) + eps).rsqrt()


def ln_fwd_ref(c, d):
    m, rs = ln_stats_ref(d["x"])
    y = (d["x"].double() - m[:, None]) * rs[:, None] * d["g"].double()
    if c.bias:
        y = y + d["b"].double()
    if c.res:
        y = y + d["res"].double()
    return {"y": y, "mean": m, "rstd": rs}


def ln_bwd_ref(c, d, mean, rstd):
    x, dy, g = d["x"].double(), d["dy"].double(), d["g"].double()
    xh = (x - mean.double()[:, None]) * rstd.double()[:, None]
    dxh = dy * g
    dx = rstd.double()[:, None] * (dxh - dxh.mean(1, keepdim=True) - xh * (dxh * xh).mean(1, keepdim=True))
    if c.add:
        dx = dx + d["add"].double()
    return {"dx": dx, "dg": (dy * xh).sum(0), "db": dy.sum(0)}


def l2_inputs(c, gen):
    x = torch.randn(c.rows, c.xs, generator=gen)
    if c.zero:
        x[c.rows // 2] = 0.0
    return {"x": x, "dy": torch.randn(c.rows, c.ys, generator=gen)}


def l2_ref(c, d):
    x = d["x"].double()[:, :c.d]
    inv = 1.0 / x.norm(dim=1).clamp_min(1e-12)
    y = x * inv[:, None]
    y32, inv32 = y.float(), inv.float()                                # what the backward is given
    yd, dy = y32.double(), d["dy"].double()[:, :c.d]
    return {"y": y, "inv": inv, "y32": y32, "inv32": inv32, "dx": (dy - yd * (yd * dy).sum(1, keepdim=True)) * inv32.double()[:, None]}


def asm_inputs(c, gen):
    M = c.E + c.ns
    sim = torch.randn(c.G, c.n, c.h, M, generator=gen) * (30.0 if c.data == "wide" and c.entry == "asm_fwd" else 1.0)
    d = {"sim": sim, "dp": torch.randn(c.G, c.n, c.h, M, generator=gen)}
    if c.rel:
        d["rel"] = torch.randn(2 * c.ns - 1, c.h, generator=gen)
    if c.null:
        d["null"] = torch.randn(c.h, generator=gen)
    return d


def asm_ref(c, d):
    """p [G, n, h, M], and for the backward dsim, drel [(2 ns - 1), h], dnull [h] from the fp32-rounded p"""
    n, h, E, ns = c.n, c.h, c.E, c.ns
    s = d["sim"].double().clone()
    i, j = torch.arange(n)[:, None], torch.arange(ns)[None, :]
    if c.null:
        s[..., E - 1] += d["null"].double()
    if c.rel:
        s[..., E:] += d["rel"].double()[i - j + ns - 1].permute(0, 2, 1)[None]          # [1, n, h, ns]
    if c.causal:
        s[..., E:] = s[..., E:].masked_fill((j > i)[None, :, None, :], float("-inf"))
    p = torch.softmax(s, dim=-1)
    out = {"p": p, "p32": p.float()}
    if c.entry == "asm_bwd":
        pd, dp = out["p32"].double(), d["dp"].double()
        ds = pd * (dp - (pd * dp).sum(-1, keepdim=True))
        out["dsim"] = ds
        if c.rel:
            live = ds[..., E:].masked_fill((j > i)[None, :, None, :], 0.0) if c.causal else ds[..., E:]
            drel = torch.zeros(2 * ns - 1, h, dtype=torch.float64)
            drel.index_put_(((i - j + ns - 1)[:, None, :].expand(n, h, ns), torch.arange(h)[None, :, None].expand(n, h, ns)), live.sum(0), accumulate=True)
            out["drel"] = drel
        if c.null:
            out["dnull"] = ds[..., E - 1].sum((0, 1))
    return out


def inputs(c, gen):
    if c.entry in _GN_ENTRIES:
        return gn_inputs(c, gen)
    return {"softmax": softmax_inputs, "ln_fwd": ln_inputs, "ln_bwd": ln_inputs, "l2": l2_inputs, "asm_fwd": asm_inputs, "asm_bwd": asm_inputs}[c.entry](c, gen)


# ---------------------------------------------------------------------------------------------------------------------------------
# cases: {label: case}; a label "<name>: <side>" belongs to the pair / group <name> (test_norm_fuzz_plan.py checks the sides)
# ---------------------------------------------------------------------------------------------------------------------------------
def _g_straddle(C):
    """a group count whose width C / G is no multiple of 4, so that a channel quad spans two groups (None if C has none)"""
    for G in (4, 2, 3, 5, 13, 32, 64, 512):
        if C % G == 0 and (C // G) % 4 and C // G > 1 and C % 4 == 0:
            return G
    return None


def _cond(rnd, C):
    return dict(cs=rnd.choice([0, C, 2 * C]), gb=int(rnd.random() < 0.8))


def fixed_gn32(rnd):
    f = {}
    dat = lambda: rnd.choice(DATA["gn32"])
    act = lambda: rnd.choice(ACTS)
    st = lambda: rnd.choice(GN_STATS)
    bw = lambda: rnd.choice(["bwd", "bwd_ex"])
    # red_nblk = rows / 64 clamped to 1 .. 256; rows per workgroup = ceil(rows / nblk)
    for rows in (1, 63, 64, 127, 128, 831, 4159, 16383, 16384, 16385):
        C = rnd.choice([4, 12, 64]) if rows > 4159 else rnd.choice([4, 6, 12, 64, 192, 260])
        f["nblk: rows %d" % rows] = gn(st(), dat(), B=rnd.choice([1, 2]), rows=rows, C=C, G=rnd.choice([1, C]), **_cond(rnd, C))
    f["empty tail: rows 16384"] = gn("bwd", dat(), B=1, rows=16384, C=12, G=4, act=act(), **_cond(rnd, 12))
    f["empty tail: rows 16385"] = gn("bwd", dat(), B=1, rows=16385, C=12, G=4, act=act(), **_cond(rnd, 12))
    f["offset at 16385 rows, stats"] = gn("stats", "offset", B=2, rows=16385, C=64, G=8)
    f["offset at 16385 rows, stats_coef"] = gn("stats_coef", "offset", B=1, rows=16385, C=4, G=1, cs=8)
    f["offset at 16385 rows, scalar reduce"] = gn("stats", "offset", B=1, rows=16385, C=6, G=2)
    # the channel-quad path of colreduce_kernel: C % 4 == 0 and C <= 1024
    for C in (4, 6, 1024, 1028):
        f["colreduce path: C %d, stats" % C] = gn(st(), dat(), B=rnd.choice([1, 3]), rows=rnd.choice([63, 127, 831]), C=C, G=rnd.choice([1, 2, C]), **_cond(rnd, C))
        e = bw()
        f["colreduce path: C %d, bwd" % C] = gn(e, dat(), B=rnd.choice([2, 5]), rows=rnd.choice([64, 128, 831]), C=C, G=rnd.choice([1, 2, C]), act=act(),
                                               add=int(e == "bwd_ex") * rnd.randint(0, 1), **_cond(rnd, C))
    # every C of the issue through the apply kernels, G = 1, C and a width a channel quad straddles
    for C in (4, 6, 12, 64, 192, 260, 1024, 1028):
        for G in sorted({1, C, _g_straddle(C) or 2}):
            e = rnd.choice(["fwd", "bwd", "bwd_ex", "stats_coef"])
            f["C %d G %d" % (C, G)] = gn(e, dat(), B=rnd.choice([1, 2, 3, 5]), rows=rnd.choice([1, 63, 64, 127, 128, 831]), C=C, G=G, act=act(),
                                         add=int(e == "bwd_ex"), **_cond(rnd, C))
    f["quad straddles two groups: fwd"] = gn("fwd", dat(), B=3, rows=127, C=12, G=4, act=act(), cs=24)
    f["quad straddles two groups: bwd"] = gn("bwd", dat(), B=3, rows=127, C=12, G=4, act=act(), cs=24)
    # every activation, forward and backward
    for a in ACTS:
        f["act %d fwd" % a] = gn("fwd", rnd.choice(["randn", "wide"]), B=2, rows=rnd.choice([63, 216]), C=rnd.choice([12, 64, 6]), G=2, act=a)
        f["act %d bwd" % a] = gn(bw(), rnd.choice(["randn", "wide"]), B=2, rows=rnd.choice([63, 216]), C=rnd.choice([12, 64, 6]), G=2, act=a)
    # each optional output null in turn; no scale / shift; no gamma / beta
    for null in ("g", "b", "gb"):
        f["null outputs: " + null] = gn(bw(), dat(), B=2, rows=100, C=rnd.choice([6, 64]), G=2, act=act(), null=null)
    f["null outputs: scale and shift gradients"] = gn("bwd", dat(), B=2, rows=100, C=64, G=2, act=act(), cs=128, null="s")
    f["no gamma, no scale"] = gn("fwd", dat(), B=2, rows=65, C=64, G=4, act=act(), cs=0, gb=0)
    f["no gamma, scale in halves"] = gn("bwd", dat(), B=3, rows=65, C=64, G=4, act=act(), cs=128, gb=0)
    # the entries that take a producer's partials: the 512-thread stride of the finaliser, the 64-lane stride of sum_partials_kernel
    for i, nblk in enumerate((1, 7, 64, 65, 256, 2048)):
        C = (64, 12, 6, 192, 64, 4)[(i + rnd.randint(0, 5)) % 6]
        G = rnd.choice([1, C, 2])
        rows = rnd.choice([nblk, 3 * nblk + 1, max(nblk // 2, 1)])
        f["partials: stats_fp nblk %d" % nblk] = gn("stats_fp", dat(), B=rnd.choice([1, 2]), rows=rows, C=C, G=G, nblk=nblk)
        f["partials: coef_fp nblk %d" % nblk] = gn("coef_fp", dat(), B=rnd.choice([1, 3]), rows=rows, C=C, G=G, nblk=nblk, **_cond(rnd, C))
        f["partials: bwd_fp nblk %d" % nblk] = gn("bwd_fp", dat(), B=2, rows=min(rows, 600), C=C, G=G, nblk=nblk, act=act(), **_cond(rnd, C))
        f["partials: bwd_ex nblk %d" % nblk] = gn("bwd_ex", dat(), B=2, rows=min(rows, 600), C=C, G=G, nblk=nblk, act=act(), add=i % 2, **_cond(rnd, C))
    for i in range(3):
        C = (64, 6, 192)[i]
        f["coef %d" % i] = gn("coef", dat(), B=(1, 3, 5)[i], rows=1, C=C, G=(8, 1, 192)[i], **_cond(rnd, C))
    # alignment, only where the launcher reads it: the apply takes the scalar kernel, the reductions refuse
    f["aligned x: fwd"] = gn("fwd", dat(), B=2, rows=65, C=64, G=4, act=act(), cs=128)
    f["misaligned x: fwd"] = gn("fwd", dat(), B=2, rows=65, C=64, G=4, act=act(), cs=128, mis="x")
    f["misaligned y: fwd"] = gn("fwd", dat(), B=1, rows=130, C=12, G=4, act=act(), mis="y")
    f["misaligned x: stats, C 6"] = gn("stats", dat(), B=2, rows=65, C=6, G=2, mis="x")
    f["misaligned x: stats, C 64 (refusal)"] = gn("stats", dat(), B=2, rows=65, C=64, G=2, mis="x")
    f["misaligned x: stats_coef, C 64 (refusal)"] = gn("stats_coef", dat(), B=1, rows=65, C=64, G=2, cs=64, mis="x")
    f["misaligned dy: bwd_ex, C 64 (refusal)"] = gn("bwd_ex", dat(), B=2, rows=65, C=64, G=2, act=act(), add=1, mis="dy")
    f["misaligned x: bwd, C 64 (refusal)"] = gn("bwd", dat(), B=2, rows=65, C=64, G=2, act=act(), mis="x")
    f["misaligned dx: bwd, C 1028"] = gn("bwd", dat(), B=2, rows=65, C=1028, G=2, act=act(), mis="dx")
    f["misaligned dx_add: bwd_ex, partials"] = gn("bwd_ex", dat(), B=2, rows=65, C=64, G=2, act=act(), add=1, nblk=3, mis="add")
    f["misaligned dy: bwd, C 6"] = gn("bwd", dat(), B=2, rows=65, C=6, G=3, act=act(), mis="dy")
    # variance exactly zero (residue)
    f["residue: stats"] = gn("stats", "const", B=2, rows=216, C=64, G=8)
    f["residue: stats_coef, scalar reduce"] = gn("stats_coef", "const", B=2, rows=831, C=6, G=3, cs=12)
    f["residue: stats_fp"] = gn("stats_fp", "const", B=2, rows=200, C=12, G=4, nblk=7)
    f["residue: fwd"] = gn("fwd", "const", B=2, rows=216, C=64, G=8, act=1, cs=128)
    f["residue: fwd, scalar apply"] = gn("fwd", "const", B=2, rows=100, C=6, G=3, act=2)
    return f


def fixed_gn16(rnd):
    f = {}
    dat = lambda: rnd.choice(DATA["gn16"])
    act = lambda: rnd.choice(ACTS)
    shape = lambda: dict(B=rnd.choice([1, 2, 3, 5]), rows=rnd.choice([1, 63, 64, 127, 128, 831]), **rnd.choice([dict(C=4, G=1), dict(C=12, G=4), dict(C=64, G=8),
                         dict(C=192, G=192), dict(C=260, G=5), dict(C=1024, G=1), dict(C=1028, G=2)]))
    for bf16 in (0, 1):
        for xh in (0, 1):
            for i in range(2):
                s = shape()
                f["fwd_h bf16 %d x_half %d, %d" % (bf16, xh, i)] = gn("fwd_h", dat(), act=act(), bf16=bf16, x_half=xh, **s, **_cond(rnd, s["C"]))
    for t in TRIPLES_CT + TRIPLES_RT + ((0, 0, 0),):
        for i in range(2):
            s = shape()
            f["bwd_h types %d %d %d, %d" % (*t, i)] = gn("bwd_h", dat(), act=act(), xt=t[0], dxt=t[1], dyt=t[2], add=rnd.randint(0, 1),
                                                        nblk=rnd.choice([0, 0, 5]), **s, **_cond(rnd, s["C"]))
    f["bwd_h at 16385 rows"] = gn("bwd_h", dat(), B=1, rows=16385, C=64, G=8, act=1, xt=1, dxt=1, dyt=1)
    f["bwd_h straddling quads"] = gn("bwd_h", dat(), B=3, rows=127, C=12, G=4, act=1, xt=2, dxt=2, dyt=2, cs=24)
    # found by this fuzz: with C > 1024 colreduce_kernel takes its scalar path, and GnBwdF::scalar indexed a 16-bit x or dy as fp32 -- twice
    # the tensor's bytes, an illegal address at (2, 831, 1028) with an fp16 dy; it now loads by type (ld1_any)
    f["16-bit behind the scalar reduce: fp16 dy"] = gn("bwd_h", dat(), B=2, rows=831, C=1028, G=2, act=0, add=1, xt=0, dxt=0, dyt=1)
    f["16-bit behind the scalar reduce: bf16 x and dy"] = gn("bwd_h", dat(), B=1, rows=127, C=1028, G=4, act=act(), xt=2, dxt=2, dyt=2, cs=2056)
    f["16-bit behind the scalar reduce: fp16 x, fp32 dy"] = gn("bwd_h", dat(), B=3, rows=65, C=2048, G=8, act=act(), xt=1, dxt=1, dyt=0)
    f["refusal: fwd_h C 6"] = gn("fwd_h", B=2, rows=64, C=6, G=2, bf16=rnd.randint(0, 1))
    f["refusal: bwd_h C 6"] = gn("bwd_h", B=2, rows=64, C=6, G=2, xt=1, dxt=1, dyt=1)
    f["fp32 through bwd_h, C 6"] = gn("bwd_h", B=2, rows=64, C=6, G=2)
    return f


def fixed_softmax(rnd):
    f = {}
    dat = lambda: rnd.choice(DATA["softmax"])
    sc = lambda: rnd.choice([1.0, 0.25, -0.5])
    f["long row n: 4095"] = softmax(3, 4095, 1, sc(), dat())
    f["long row n: 4096"] = softmax(3, 4096, 1, sc(), dat())
    f["long row outer: 1024"] = softmax(1024, 4096, 1, sc(), dat())
    f["long row outer: 1025"] = softmax(1025, 4096, 1, sc(), dat())
    f["column workgroup n: 63"] = softmax(3, 63, 64, sc(), dat())
    f["column workgroup n: 64"] = softmax(3, 64, 64, sc(), dat())
    f["column workgroup inner: 64"] = softmax(5, 65, 64, sc(), dat())
    f["column workgroup inner: 96"] = softmax(5, 65, 96, sc(), dat())
    f["column workgroup inner: 1024"] = softmax(2, 65, 1024, sc(), dat())
    f["column workgroup inner: 2048"] = softmax(2, 65, 2048, sc(), dat())
    f["column workgroup outer: 65535"] = softmax(65535, 64, 2, sc(), dat())
    f["column workgroup outer: 65536"] = softmax(65536, 64, 2, sc(), dat())
    for n in (1, 63, 65, 1023, 1025, 4097, 5000):
        f["tail n %d, rows" % n] = softmax(rnd.choice([1, 3, 7]), n, 1, sc(), dat())
        f["tail n %d, columns" % n] = softmax(rnd.choice([1, 3]), n, rnd.choice([2, 3, 64]), sc(), dat())
    f["long row, one row of 5000, flat"] = softmax(1, 5000, 1, 1.0, "flat")
    f["long row, flat 4096"] = softmax(2, 4096, 1, 1.0, "flat")
    f["long row, one row of 4096"] = softmax(1, 4096, 1, sc(), dat())
    f["outer 0"] = softmax(0, 5, 3)
    f["refusal: scale 0"] = softmax(2, 9, 3, 0.0, refuse=1)
    for d_ in DATA["softmax"]:
        f["%s through the column workgroup" % d_] = softmax(2, 200, rnd.choice([2, 64, 1024]), sc(), d_)
        f["%s through the long row" % d_] = softmax(2, rnd.choice([4096, 4100, 6000]), 1, sc(), d_)
    return f


def fixed_rows(rnd):
    f = {}
    dat = lambda: rnd.choice(DATA["rows"])
    coin = lambda: rnd.randint(0, 1)
    for i, C in enumerate((1, 24, 63, 64, 65, 1024, 1100)):
        rows = (1, 3, 5, 4099, 3, 5, 1)[(i + rnd.randint(0, 6)) % 7]
        f["ln_fwd C %d" % C] = ln("ln_fwd", rows, C, dat(), bias=coin(), res=coin(), stats=coin())
        f["ln_bwd C %d" % C] = ln("ln_bwd", rows, C, dat(), add=coin(), db=coin())
    for rows in (1, 3, 5, 4099):
        f["ln_fwd rows %d" % rows] = ln("ln_fwd", rows, rnd.choice([24, 64, 65]), dat(), bias=coin(), res=coin(), stats=coin())
        f["ln_bwd rows %d" % rows] = ln("ln_bwd", rows, rnd.choice([24, 64, 65]), dat(), add=coin(), db=coin())
    for b, r_, s in ((0, 0, 0), (1, 1, 1), (0, 1, 0), (1, 0, 0)):
        f["ln_fwd bias %d res %d stats %d" % (b, r_, s)] = ln("ln_fwd", 70, 48, dat(), bias=b, res=r_, stats=s)
    f["ln_bwd dx only"] = ln("ln_bwd", 70, 48, dat(), dg=0, db=0)
    f["ln_bwd dg only, dx_add"] = ln("ln_bwd", 130, 48, dat(), add=1, db=0)
    f["ln_bwd dg and db"] = ln("ln_bwd", 130, 65, dat(), add=0, db=1)
    f["ln_bwd empty tail: rows 16385"] = ln("ln_bwd", 16385, 24, dat(), db=1)
    # the alignment requirements of diqt_chan_layernorm_bwd_ex: the workspace always, dy where IdentF loads it 16 bytes per lane
    f["ln_bwd alignment: aligned"] = ln("ln_bwd", 70, 64, dat(), db=1)
    f["ln_bwd alignment: misaligned workspace (refusal)"] = ln("ln_bwd", 70, 64, dat(), db=coin(), mis="ws")
    f["ln_bwd alignment: misaligned dy, C 64 (refusal)"] = ln("ln_bwd", 70, 64, dat(), db=1, mis="dy")
    f["ln_bwd alignment: misaligned dy, C 64, no db"] = ln("ln_bwd", 70, 64, dat(), db=0, mis="dy")
    f["ln_bwd alignment: misaligned dy, C 63"] = ln("ln_bwd", 70, 63, dat(), db=1, mis="dy")
    f["ln_bwd alignment: misaligned dy, C 1100"] = ln("ln_bwd", 9, 1100, dat(), db=1, mis="dy")
    # l2norm: 16 lanes per row, rows a multiple of 16 per sweep
    for i, d in enumerate((1, 15, 16, 17, 64, 100)):
        rows = (1, 15, 16, 17, 4099, 17)[(i + rnd.randint(0, 5)) % 6]
        f["l2 d %d" % d] = l2(rows, d, d + rnd.choice([0, 3]), d + rnd.choice([0, 5]), d + rnd.choice([0, 2]), zero=coin())
    for rows in (1, 15, 16, 17, 4099):
        d = rnd.choice([15, 16, 17, 64])
        f["l2 rows %d" % rows] = l2(rows, d, d + 1, d + 4, d + 2, zero=int(rows > 1))
    f["l2 without inv"] = l2(33, 20, 20, 23, 20, inv=0, zero=1)
    f["l2 packed"] = l2(100, 64, zero=1)
    # attention soft-max: one wave per row of M = n_extra + n_self keys
    for i, M in enumerate((1, 63, 64, 65, 129)):
        for h in (1, 3, 8):
            E = (0, 1, 5)[(i + h) % 3]
            if M - E < 1:
                E = 0
            ns = M - E
            own = rnd.random() < 0.6          # n_self == n: causal / table allowed
            rel, causal, null = (coin(), coin(), coin() if E else 0) if own else (0, 0, coin() if E else 0)
            n = ns if own else rnd.choice([3, 40])
            e = rnd.choice(["asm_fwd", "asm_bwd"])
            f["%s M %d h %d" % (e, M, h)] = asm(e, rnd.choice([1, 2, 5]), n, h, E, ns, rel, null, causal, ws=coin(), data=dat())
    for rel, null, causal in ((1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 0, 0), (1, 0, 1), (0, 1, 1)):
        f["asm_fwd rel %d null %d causal %d" % (rel, null, causal)] = asm("asm_fwd", 2, 37, 3, 2, None, rel, null, causal, data=dat())
        f["asm_bwd_ws rel %d null %d causal %d" % (rel, null, causal)] = asm("asm_bwd", 2, 37, 3, 2, None, rel, null, causal, ws=1, data=dat())
        f["asm_bwd rel %d null %d causal %d" % (rel, null, causal)] = asm("asm_bwd", 2, 37, 3, 2, None, rel, null, causal, ws=0, data=dat())
    f["table: n_self 192"] = asm("asm_bwd", 1, 192, 8, 1, None, 1, 1, coin(), ws=1, data=dat())
    f["table: n_self 193"] = asm("asm_bwd", 1, 193, 8, 1, None, 1, 1, coin(), ws=1, data=dat())
    f["table, many rows per wave"] = asm("asm_bwd", 40, 30, 8, 1, None, 1, 1, 1, ws=1, data=dat())
    f["refusal: asm_fwd causal with n_self != n"] = asm("asm_fwd", 2, 5, 3, 1, 9, 0, 0, 1)
    f["refusal: asm_fwd null bias without a null key"] = asm("asm_fwd", 2, 5, 3, 0, None, 0, 1, 0)
    f["refusal: asm_bwd table gradient with n_self != n"] = asm("asm_bwd", 2, 9, 3, 1, 5, 1, 0, 0, ws=coin())
    return f


FIXED = {"gn32": fixed_gn32, "gn16": fixed_gn16, "softmax": fixed_softmax, "rows": fixed_rows}
N_RANDOM = {"gn32": 30, "gn16": 20, "softmax": 30, "rows": 30}


def _draw(rnd, family):
    if family == "gn32":
        C = rnd.choice([4, 6, 12, 64, 192, 260])
        e = rnd.choice(["stats", "stats_coef", "stats_fp", "coef_fp", "coef", "fwd", "bwd", "bwd_fp", "bwd_ex"])
        nblk = rnd.choice([1, 7, 64, 65]) if e.endswith("_fp") or (e == "bwd_ex" and rnd.random() < 0.5) else 0
        return gn(e, rnd.choice(DATA["gn32"]), B=rnd.choice([1, 2, 3, 5]), rows=rnd.choice([1, 63, 64, 127, 128, 831, rnd.randint(1, 900)]), C=C,
                  G=rnd.choice([1, C, _g_straddle(C) or 2]), act=rnd.choice(ACTS), nblk=nblk, add=int(e == "bwd_ex" and rnd.random() < 0.5),
                  null="" if not e.startswith("bwd") else rnd.choice(["", "", "g", "b", "s"]), **_cond(rnd, C))
    if family == "gn16":
        C, G = rnd.choice([(4, 1), (12, 4), (64, 8), (192, 192), (260, 5)])
        t = rnd.choice(TRIPLES_CT + TRIPLES_RT)
        shape = dict(B=rnd.choice([1, 2, 3, 5]), rows=rnd.choice([1, 63, 64, 127, 128, 831, rnd.randint(1, 900)]), C=C, G=G, act=rnd.choice(ACTS))
        if rnd.random() < 0.3:
            return gn("fwd_h", rnd.choice(DATA["gn16"]), bf16=rnd.randint(0, 1), x_half=rnd.randint(0, 1), **shape, **_cond(rnd, C))
        return gn("bwd_h", rnd.choice(DATA["gn16"]), xt=t[0], dxt=t[1], dyt=t[2], add=rnd.randint(0, 1), nblk=rnd.choice([0, 0, 7]), **shape, **_cond(rnd, C))
    if family == "softmax":
        inner = rnd.choice([1, 1, 2, 3, 64, 96, 1024, 2048])
        n = rnd.choice([1, 63, 64, 65, 1023, 1025, 4096, 4097, 5000, rnd.randint(1, 300)])
        return softmax(rnd.choice([1, 3, rnd.randint(1, 40)]), n, inner, rnd.choice([1.0, 0.25, -0.5]), rnd.choice(DATA["softmax"]))
    e = rnd.choice(["ln_fwd", "ln_bwd", "l2", "asm_fwd", "asm_bwd"])
    dat = rnd.choice(DATA["rows"])
    if e in ("ln_fwd", "ln_bwd"):
        kw = dict(bias=rnd.randint(0, 1), res=rnd.randint(0, 1), stats=rnd.randint(0, 1)) if e == "ln_fwd" else dict(add=rnd.randint(0, 1), db=rnd.randint(0, 1))
        return ln(e, rnd.choice([1, 3, 5, 300, rnd.randint(1, 200)]), rnd.choice([1, 24, 63, 64, 65, 1024, 1100]), dat, **kw)
    if e == "l2":
        d = rnd.choice([1, 15, 16, 17, 64, 100])
        return l2(rnd.choice([1, 15, 16, 17, 300]), d, d + rnd.randint(0, 3), d + rnd.randint(0, 3), d + rnd.randint(0, 3), zero=rnd.randint(0, 1))
    ns, h, E = rnd.choice([1, 31, 63, 64, 65, 100]), rnd.choice([1, 3, 8]), rnd.choice([0, 1, 5])
    own = rnd.random() < 0.6
    return asm(e, rnd.choice([1, 2, 5]), ns if own else rnd.randint(1, 50), h, E, ns, own and rnd.randint(0, 1), E > 0 and rnd.randint(0, 1),
               own and rnd.randint(0, 1), ws=rnd.randint(0, 1), data=dat)


def cases(family, seed):
    rnd = random.Random(seed)
    out = list(FIXED[family](rnd).values())
    budget = MAX_ELEMS_SEED / 8 - sum(ref_elems(c) for c in out)
    left = N_RANDOM[family]
    while left > 0:
        c = _draw(rnd, family)
        if ref_elems(c) > min(2e6, max(budget, 0) / left + 1e5) or largest_tensor_bytes(c) > MAX_TENSOR_BYTES:
            continue
        out.append(c)
        budget -= ref_elems(c)
        left -= 1
    return out


def labelled(family, seed):
    return FIXED[family](random.Random(seed))
