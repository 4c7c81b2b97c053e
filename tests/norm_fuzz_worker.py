"""Worker of tests/test_gpu_norm_fuzz.py: ``python tests/norm_fuzz_worker.py <family> <seed> [--reference-only]`` runs the cases
tests/norm_fuzz_plan.py draws for (family, seed) through the C entry points of csrc/elementwise.hip (``_lib.call``, no ops layer in
between) and compares every result with the float64 formulas of the plan.

* Every output and workspace is a view inside a larger buffer (attn_fuzz_worker.Guarded's layout: payload 0xFF bytes -- a NaN in fp32, fp16
  and bf16 --, guards 0xA5), 16-byte aligned unless the case asks for 4 bytes off.  After the call the guards must be untouched and no output
  may hold a NaN.  Accumulating outputs (drel / dnull of the atomic diqt_attn_softmax_bwd) are zero-prefilled instead.
* A refusal must return the planned error code, launch nothing and leave its outputs untouched; otherwise the launches the census saw must be
  those plan.expect derived from the route queries.  Every case runs twice, bit-identically -- except drel / dnull of the atomic kernel.
* fp32 outputs: the project's rule (tests/test_gpu_kernels.py) against float64, ``max err <= tol * max|ref|`` with tol 2e-5 for forwards and
  1e-4 for gradients, without an absolute floor.  Soft-max forwards (diqt_softmax_fwd, diqt_attn_softmax_fwd) and both l2norm passes (a zero
  row has inv = 1e12) are held to it per row / column: ``max|ref|`` of that row.
* 16-bit outputs: ``|got - ref| <= half a 16-bit ulp at |ref| + t, plus t``, t the fp32 tolerance above.
* Statistics (diqt_groupnorm_stats, _stats_coef, and with d = 1 the *_from_partials entries, whose partials are block sums rounded once):
  with u = 2^-24 and d the longest fp32 addition chain behind one partial (plan.col_route: rows per thread plus row groups per workgroup),
  ``|mean - m| <= (d + 2) u E|x|``, and rstd must lie between the values that ``var -+ (d + 2) u (E[x^2] + 2 m^2)`` give through
  (var + eps)^-1/2 (2 u for its own rounding).  The largest observed ratio to these bounds is printed per data class (for rstd: the used
  share of the interval between the exact value and the nearer end).  The coefficients of
  _stats_coef / _coef_from_partials are judged against float64 of the statistics the same call returned.
* Residue ceilings, added to the rule where the exact result is a cancellation the rule cannot scale (derived from the number formats, not
  from what the kernels return): ``residue_ceiling`` for the constructed zero-variance GroupNorm applies; ``softmax_bwd_ceiling`` for the
  soft-max backward on "peaked" and "wide" rows, where y is nearly one-hot and dx = y (dy - sum(y dy)) is the rounding residue of the sum.

``--reference-only`` runs everything but the GPU calls (inputs, references, budgets) on the CPU.  One process per (family, seed): a fault or
hang ends at the caller's timeout.
"""
import os
import re
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from diffusioniqt_amd import _lib
from tests import norm_fuzz_plan as plan
from tests import attn_fuzz_worker as attn

DEV = "cuda"
GUARD = attn.GUARD
TOL_FWD, TOL_GRAD = 2e-5, 1e-4
U = 2.0 ** -24
TAGS = sorted(plan.TAGS, key=len, reverse=True)


class Guarded(attn.Guarded):
    """attn_fuzz_worker.Guarded with two more choices: ``shift`` bytes off the 16-byte boundary, and a zero-prefilled payload"""

    def __init__(self, shape, dtype=torch.float32, k=0, nbytes=None, shift=0, zero=False):
        self.off = GUARD + 16 * (1 + k % 5) + shift
        self.n = nbytes if nbytes is not None else torch.Size(shape).numel() * torch.empty((), dtype=dtype).element_size()
        self.raw = torch.full((self.off + self.n + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
        pay = self.raw[self.off:self.off + self.n]
        pay.fill_(0 if zero else 0xFF)
        self.t = pay.view(dtype).view(shape) if nbytes is None else pay
        assert self.t.data_ptr() % 16 == shift


def observed(cen):
    """{tag: launches} with exact tags (diqt_census_count matches substrings), and nothing this worker does not know"""
    exact = {}
    for t in TAGS:
        exact[t] = cen.count(t) - sum(n for u, n in exact.items() if t in u)
    assert cen.count(None) == sum(exact.values()), "a launch tag this worker does not know"
    return {t: n for t, n in exact.items() if n}


def invoke(name, *args):
    """the entry's return code, through _lib.call"""
    try:
        _lib.call(name, *args)
        return 0
    except RuntimeError as e:
        return int(re.search(r"failed \((-?\d+)\)", str(e)).group(1))


def stream():
    return torch.cuda.current_stream().cuda_stream


def dev(t, mis=False, dtype=None):
    """the host tensor on the device, contiguous; mis: 4 bytes off a 16-byte boundary (fp32 only)"""
    if t is None:
        return None
    t = t.contiguous() if dtype is None else t.to(dtype).contiguous()
    if not mis:
        return t.to(DEV)
    assert t.dtype == torch.float32
    buf = torch.empty(t.numel() + 4, dtype=torch.float32, device=DEV)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def ulp16(a, ty):
    """the spacing of fp16 (ty 1) / bf16 (ty 2) numbers at magnitude a (float64 tensor)"""
    mant, emin = (10, -14) if ty == 1 else (7, -126)
    e = torch.floor(torch.log2(a.clamp_min(2.0 ** emin))).clamp_min(emin)
    return torch.pow(2.0, e - mant)


class Check:
    def __init__(self, stats, data):
        self.why, self.stats, self.data = [], stats, data

    def note(self, what, v):
        key = (self.data, what)
        self.stats[key] = max(self.stats.get(key, 0.0), float(v))

    def close(self, got, ref, tol, what, ceiling=None, ty=0, axis=None):
        """max|got - ref| <= tol max|ref| (+ an elementwise ceiling); axis: per slice along that axis; ty: a 16-bit output"""
        got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
        assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
        if ref.numel() == 0:
            return
        err = (got - ref).abs()
        scale = ref.abs().amax(axis, keepdim=True) if axis is not None else ref.abs().max()
        bound = tol * scale + (ceiling if ceiling is not None else 0.0)
        if ty:
            bound = bound + 0.5 * ulp16(ref.abs() + bound, ty)
        bound = bound + torch.zeros_like(err)
        if ceiling is None and not ty:
            self.note(what, (err / (scale + torch.zeros_like(err)).clamp_min(1e-300)).max())
        bad = ~(err <= bound)
        if bool(bad.any()):
            i = int((err - bound).argmax())
            self.why.append("%s: |err| %.3e > bound %.3e at flat index %d (max|ref| %.3e, tol %.0e%s%s)" % (
                what, err.flatten()[i], bound.flatten()[i], i, ref.abs().max(), tol, ", + ceiling" if ceiling is not None else "",
                ", + half a 16-bit ulp" if ty else ""))

    def guards(self, bufs, cols=None):
        for name, b in bufs.items():
            if b is None:
                continue
            if not b.guards_intact():
                self.why.append("%s written outside its buffer" % name)
            elif b.t.dtype.is_floating_point:
                t = b.t
                if cols and name in cols:          # rows wider than their payload: the gap stays as prefilled
                    if not bool(torch.isnan(t[:, cols[name]:]).all()):
                        self.why.append("%s written between its rows" % name)
                    t = t[:, :cols[name]]
                if bool(torch.isnan(t).any()):
                    self.why.append("%s has elements nobody wrote" % name)


def twice(c, k, ck, setup, loose=(), cols=None, stay=()):
    """setup(k) -> ({name: Guarded}, call); runs it twice under the census and applies the checks every case shares.  Returns the first
    run's buffers (None after a planned refusal).  loose: outputs exempt from bit identity; stay: outputs a planned partial refusal leaves."""
    err, tags = plan.expect(c)
    runs = []
    for rep in range(2):
        bufs, call = setup(k + 3 * rep)
        torch.cuda.synchronize()
        with _lib.census() as cen:
            rc = call()
            torch.cuda.synchronize()
        runs.append((rc, bufs, observed(cen)))
    for rc, bufs, seen in runs:
        if rc != err:
            ck.why.append("returned %d, planned %d" % (rc, err))
        if seen != tags:
            ck.why.append("launches %s, planned %s" % (seen, tags))
        if err:
            for name, b in bufs.items():
                if b is not None and (not stay or name in stay) and not b.untouched():
                    ck.why.append("a refusal wrote " + name)
        if not err or stay:
            ck.guards({n: b for n, b in bufs.items() if not (err and n in stay)}, cols)
    if err or runs[0][0] or runs[1][0]:
        return None
    for name, b in runs[0][1].items():
        o = runs[1][1][name]
        if b is not None and name not in loose and name != "workspace" and not torch.equal(b.raw[b.off:b.off + b.n], o.raw[o.off:o.off + o.n]):
            ck.why.append(name + " differs between two runs")
    return runs[0][1]


# ---------------------------------------------------------------------------------------------------------------------------------
# GroupNorm
# ---------------------------------------------------------------------------------------------------------------------------------
def cond_ptrs(c, d, emb=None):
    """(gamma, beta, scale, shift, cond_stride) device pointers: scale / shift halves of one [B, 2C] row, or two tensors"""
    ga, be = (dev(d["gamma"]), dev(d["beta"])) if c.gb else (None, None)
    if not c.cs:
        return ga, be, None, None, c.C, ()
    if c.cs == 2 * c.C:
        e = dev(d["emb"])
        return ga, be, e[:, :c.C], e[:, c.C:], c.cs, (e,)
    sc, sf = dev(d["emb"][:, :c.C]), dev(d["emb"][:, c.C:])
    return ga, be, sc, sf, c.cs, (sc, sf)


def stat_bounds(ck, c, x, G, chain, mean, rstd):
    m, var, r, eabs, ex2 = plan.gn_stats_ref(x, G)
    bm, bv = (chain + 2) * U * eabs, (chain + 2) * U * (ex2 + 2 * m * m)
    gm, gr = mean.double().cpu().view_as(m), rstd.double().cpu().view_as(m)
    em = (gm - m).abs()
    lo, hi = (var + bv + plan.EPS).rsqrt() * (1 - 2 * U), ((var - bv).clamp_min(0) + plan.EPS).rsqrt() * (1 + 2 * U)
    ck.note("mean error / bound", (em / bm.clamp_min(1e-300)).max() if bool((bm > 0).all()) else 0.0)
    # how much of the interval [lo, hi] around the exact rstd the result used up
    ck.note("rstd error / bound", torch.maximum((gr - r) / (hi - r), (r - gr) / (r - lo)).max())
    if not bool((em <= bm).all()):
        ck.why.append("mean: error %.3e over its bound %.3e (chain %d)" % (em.max(), bm.flatten()[int(em.argmax())], chain))
    if not bool(((gr >= lo) & (gr <= hi)).all()):
        i = int(torch.maximum(lo - gr, gr - hi).argmax())
        ck.why.append("rstd %.9g outside [%.9g, %.9g] (exact %.9g, chain %d)" % (gr.flatten()[i], lo.flatten()[i], hi.flatten()[i], r.flatten()[i], chain))


def residue_ceiling(c, d, mean, rstd):
    """z = A x + Bc with A = r ga (1 + sc) and Bc = (be - m r ga) (1 + sc) + sf: five fp32 roundings of products of size |A x| (A itself two,
    A x one, m r ga two) and the addition: at most 8 u max|A| max|x| on z, and every activation here is 1.1-Lipschitz at most"""
    A = plan.gn_coef_ref(c, d, mean, rstd)[0]
    return 1.1 * 8 * U * A.abs().max().item() * d["x"].abs().max().item()


def check_gn(c, k, ck, d, ref_only):
    B, rows, C, G = c.B, c.rows, c.C, c.G
    e = c.entry
    x = d["x"]
    m64, var64, r64, _, _ = plan.gn_stats_ref(x, G)
    mean32, rstd32 = m64.float(), r64.float()
    st = stream() if not ref_only else None
    nws = _lib.query("diqt_reduce_workspace_bytes", B, C)
    bf = 2 if c.bf16 else 1
    # references first: every plan error shows without a GPU
    if e in ("stats_fp", "coef_fp"):
        parts = plan.block_sums(x.double(), x.double() ** 2, c.nblk)
    if e in ("bwd_fp", "bwd_ex", "bwd_h") and c.nblk:
        dz, xhat, _, _ = plan.gn_bwd_sums(c, d, mean32, rstd32)
        parts = plan.block_sums(dz, dz * xhat, c.nblk)
    ref = {}
    if e == "coef":
        ref["coef"] = plan.gn_coef_ref(c, d, mean32, rstd32)
    elif e in ("fwd", "fwd_h"):
        ref["y"] = plan.gn_fwd_ref(c, d, mean32, rstd32)
    elif e in plan.GN_BWD:
        ref = plan.gn_bwd_ref(c, d, mean32, rstd32)
    for name, t in ref.items():
        if not bool(torch.isfinite(t).all()):
            ck.why.append("plan error: the reference's %s is not finite" % name)
    if ref_only:
        return "-"

    if e in ("stats", "stats_coef", "stats_fp", "coef_fp"):
        def setup(k):
            bufs = {"mean": Guarded((B * G,), k=k), "rstd": Guarded((B * G,), k=k + 1)}
            ga, be, sc, sf, cs, keep = cond_ptrs(c, d)
            if e in ("stats_coef", "coef_fp"):
                bufs["coef"] = Guarded((2, B, C), k=k + 2)
            if e in ("stats", "stats_coef"):
                bufs["workspace"] = Guarded(None, k=k + 3, nbytes=nws)
                xd = dev(x, c.mis == "x")
                if e == "stats":
                    return bufs, lambda: invoke("diqt_groupnorm_stats", xd, bufs["mean"].t, bufs["rstd"].t, bufs["workspace"].t, nws, B, rows, C, G, plan.EPS, st)
                return bufs, lambda: (keep, invoke("diqt_groupnorm_stats_coef", xd, ga, be, sc, sf, cs, bufs["mean"].t, bufs["rstd"].t, bufs["coef"].t,
                                                   bufs["workspace"].t, nws, B, rows, C, G, plan.EPS, st))[1]
            pd = dev(parts)
            if e == "stats_fp":
                return bufs, lambda: invoke("diqt_groupnorm_stats_from_partials", pd, bufs["mean"].t, bufs["rstd"].t, B, c.nblk, rows, C, G, plan.EPS, st)
            return bufs, lambda: (keep, invoke("diqt_gn_coef_from_partials", pd, c.nblk, rows, ga, be, sc, sf, cs, bufs["mean"].t, bufs["rstd"].t,
                                               bufs["coef"].t, B, C, G, plan.EPS, st))[1]
        out = twice(c, k, ck, setup)
        if out:
            chain = plan.col_route(rows, C)["chain"] if e in ("stats", "stats_coef") else 1
            stat_bounds(ck, c, x, G, chain, out["mean"].t, out["rstd"].t)
            if "coef" in out:
                own = plan.gn_coef_ref(c, d, out["mean"].t.double().cpu().view(B, G), out["rstd"].t.double().cpu().view(B, G))
                ck.close(out["coef"].t, own, TOL_FWD, "coef")
        return plan.describe(c)

    if e == "coef":
        def setup(k):
            bufs = {"coef": Guarded((2, B, C), k=k)}
            ga, be, sc, sf, cs, keep = cond_ptrs(c, d)
            md, rd = dev(mean32), dev(rstd32)
            return bufs, lambda: (keep, invoke("diqt_gn_coef", md, rd, ga, be, sc, sf, cs, bufs["coef"].t, B, C, G, st))[1]
        out = twice(c, k, ck, setup)
        if out:
            ck.close(out["coef"].t, ref["coef"], TOL_FWD, "coef")
        return plan.describe(c)

    if e in ("fwd", "fwd_h"):
        oty = bf if e == "fwd_h" else 0

        def setup(k):
            bufs = {"y": Guarded((B, rows, C), dtype=plan.HDT[oty] if oty else torch.float32, k=k, shift=4 if c.mis == "y" else 0)}
            ga, be, sc, sf, cs, keep = cond_ptrs(c, d)
            md, rd = dev(mean32), dev(rstd32)
            if e == "fwd":
                xd = dev(x, c.mis == "x")
                return bufs, lambda: (keep, invoke("diqt_gn_act_fwd", xd, md, rd, ga, be, sc, sf, cs, bufs["y"].t, B, rows, C, G, c.act, st))[1]
            xd = dev(x, dtype=plan.HDT[bf] if c.x_half else None)
            return bufs, lambda: (keep, invoke("diqt_gn_act_fwd_h", xd, md, rd, ga, be, sc, sf, cs, bufs["y"].t, B, rows, C, G, c.act, c.bf16, c.x_half, st))[1]
        out = twice(c, k, ck, setup)
        if out:
            ck.close(out["y"].t, ref["y"], TOL_FWD, "y" + ("" if not oty else ", fp16" if oty == 1 else ", bf16"),
                     residue_ceiling(c, d, mean32, rstd32) if plan.residue(c) else None, ty=oty)
        return plan.describe(c)

    # the backwards
    want = {"dgamma": "g" not in c.null, "dbeta": "b" not in c.null, "dscale": bool(c.cs) and "s" not in c.null, "dshift": bool(c.cs) and "s" not in c.null}

    def setup(k):
        bufs = {"dx": Guarded((B, rows, C), dtype=plan.HDT[c.dxt] if c.dxt else torch.float32, k=k, shift=4 if c.mis == "dx" else 0),
                "dgamma": Guarded((C,), k=k + 1) if want["dgamma"] else None, "dbeta": Guarded((C,), k=k + 2) if want["dbeta"] else None,
                "workspace": Guarded(None, k=k + 3, nbytes=nws)}
        ga, be, sc, sf, cs, keep = cond_ptrs(c, d)
        dsc = dsf = None
        if want["dscale"]:
            if c.cs == 2 * C:
                bufs["dscale|dshift"] = Guarded((B, 2 * C), k=k + 4)
                dsc, dsf = bufs["dscale|dshift"].t[:, :C], bufs["dscale|dshift"].t[:, C:]
            else:
                bufs["dscale"], bufs["dshift"] = Guarded((B, C), k=k + 4), Guarded((B, C), k=k)
                dsc, dsf = bufs["dscale"].t, bufs["dshift"].t
        md, rd = dev(mean32), dev(rstd32)
        xd = dev(x, c.mis == "x", plan.HDT[c.xt] if c.xt else None)
        dyd = dev(d["dy"], c.mis == "dy", plan.HDT[c.dyt] if c.dyt else None)
        add = dev(d["add"], c.mis == "add") if c.add else None
        pd = dev(parts) if c.nblk else None
        dg, db = (bufs[n].t if bufs[n] else None for n in ("dgamma", "dbeta"))
        tail = (bufs["workspace"].t, nws, B, rows, C, G, c.act)
        if e == "bwd":
            fn = lambda: invoke("diqt_gn_act_bwd", xd, dyd, md, rd, ga, be, sc, sf, cs, bufs["dx"].t, dg, db, dsc, dsf, *tail, st)
        elif e == "bwd_fp":
            fn = lambda: invoke("diqt_gn_act_bwd_from_partials", xd, dyd, pd, c.nblk, md, rd, ga, be, sc, sf, cs, bufs["dx"].t, dg, db, dsc, dsf, *tail, st)
        elif e == "bwd_ex":
            fn = lambda: invoke("diqt_gn_act_bwd_ex", xd, dyd, pd, c.nblk, add, md, rd, ga, be, sc, sf, cs, bufs["dx"].t, dg, db, dsc, dsf, *tail, st)
        else:
            fn = lambda: invoke("diqt_gn_act_bwd_h", xd, dyd, pd, c.nblk, add, md, rd, ga, be, sc, sf, cs, bufs["dx"].t, dg, db, dsc, dsf, *tail,
                                c.xt, c.dxt, c.dyt, st)
        return bufs, lambda: (keep, fn())[1]
    out = twice(c, k, ck, setup)
    if out:
        ck.close(out["dx"].t, ref["dx"], TOL_GRAD, "dx" + ("" if not c.dxt else ", fp16" if c.dxt == 1 else ", bf16"), ty=c.dxt)
        for name in ("dgamma", "dbeta"):
            if want[name]:
                ck.close(out[name].t, ref[name], TOL_GRAD, name)
        if want["dscale"]:
            both = out["dscale|dshift"].t if c.cs == 2 * C else torch.cat((out["dscale"].t, out["dshift"].t), dim=1)
            ck.close(both[:, :C], ref["dscale"], TOL_GRAD, "dscale")
            ck.close(both[:, C:], ref["dshift"], TOL_GRAD, "dshift")
    return plan.describe(c)


# ---------------------------------------------------------------------------------------------------------------------------------
# soft-max over the middle axis
# ---------------------------------------------------------------------------------------------------------------------------------
def softmax_bwd_ceiling(y, dy, n, scale):
    """dx_i = y_i (dy_i - s), s = sum_j y_j dy_j / scale summed in fp32: s is wrong by at most (n + 2) u sum|y dy| / |scale|, the difference
    and the product add 2 u (|dy_i| + |s|); all of it times |y_i|.  Where y is nearly one-hot the exact dx is that residue or less."""
    yd, dd = y.double(), dy.double()
    t = (yd * dd).abs().sum(1, keepdim=True) / abs(scale)
    return yd.abs() * ((n + 2) * U * t + 2 * U * (dd.abs() + t))


def check_softmax(c, k, ck, d, ref_only):
    ref = plan.softmax_ref(c, d) if not c.refuse else None
    if ref_only:
        return "-"
    st = stream()
    shape = (max(c.outer, 1), c.n, c.inner)          # outer 0: one slice that must stay untouched
    xd = dev(d["x"]) if c.outer else torch.zeros(shape, device=DEV)
    dyd = dev(d["dy"]) if c.outer else torch.zeros(shape, device=DEV)
    y32 = dev(ref["y32"]) if ref is not None and c.outer else torch.zeros(shape, device=DEV)

    def setup(k):
        bufs = {"y": Guarded(shape, k=k), "dx": Guarded(shape, k=k + 1)}

        def call():
            rc = invoke("diqt_softmax_fwd", xd, bufs["y"].t, c.outer, c.n, c.inner, c.scale, st)
            return rc or invoke("diqt_softmax_bwd", y32, dyd, bufs["dx"].t, c.outer, c.n, c.inner, c.scale, st)
        return bufs, call
    if c.outer == 0:
        err, tags = plan.expect(c)
        for rep in range(2):
            bufs, call = setup(k + rep)
            with _lib.census() as cen:
                rc = call()
                torch.cuda.synchronize()
            if rc != 0 or observed(cen) or not bufs["y"].untouched() or not bufs["dx"].untouched():
                ck.why.append("outer 0: returned %d, launched %s or wrote something" % (rc, observed(cen)))
        return "nothing to do"
    out = twice(c, k, ck, setup, stay=("dx",) if c.refuse else ())
    if out:
        ck.close(out["y"].t, ref["y"], TOL_FWD, "y, per column", axis=1)
        ceil = softmax_bwd_ceiling(ref["y32"], d["dy"], c.n, c.scale) if c.data in ("peaked", "wide") else None
        ck.close(out["dx"].t, ref["dx"], TOL_GRAD, "dx", ceil)
    return plan.describe(c)


# ---------------------------------------------------------------------------------------------------------------------------------
# rows: channel LayerNorm, l2norm, attention soft-max
# ---------------------------------------------------------------------------------------------------------------------------------
def check_ln(c, k, ck, d, ref_only):
    rows, C = c.rows, c.C
    if c.entry == "ln_fwd":
        ref = plan.ln_fwd_ref(c, d)
    else:
        m64, r64 = plan.ln_stats_ref(d["x"])
        mean32, rstd32 = m64.float(), r64.float()
        ref = plan.ln_bwd_ref(c, d, mean32, rstd32)
    if ref_only:
        return "-"
    st = stream()
    if c.entry == "ln_fwd":
        def setup(k):
            bufs = {"y": Guarded((rows, C), k=k), "mean": Guarded((rows,), k=k + 1) if c.stats else None, "rstd": Guarded((rows,), k=k + 2) if c.stats else None}
            xd, gd, bd, rd = dev(d["x"]), dev(d["g"]), dev(d.get("b")), dev(d.get("res"))
            return bufs, lambda: invoke("diqt_chan_layernorm_fwd_res", xd, gd, bd, rd, bufs["y"].t, bufs["mean"].t if c.stats else None,
                                        bufs["rstd"].t if c.stats else None, rows, C, plan.EPS, st)
        out = twice(c, k, ck, setup)
        if out:
            ck.close(out["y"].t, ref["y"], TOL_FWD, "LayerNorm y")
            if c.stats:
                ck.close(out["mean"].t, ref["mean"], TOL_FWD, "LayerNorm mean")
                ck.close(out["rstd"].t, ref["rstd"], TOL_FWD, "LayerNorm rstd")
        return plan.describe(c)
    nws = _lib.query("diqt_reduce_workspace_bytes", 1, C)

    def setup(k):
        bufs = {"dx": Guarded((rows, C), k=k), "dg": Guarded((C,), k=k + 1) if c.dg else None, "db": Guarded((C,), k=k + 2) if c.dg and c.db else None,
                "workspace": Guarded(None, k=k + 3, nbytes=nws, shift=4 if c.mis == "ws" else 0)}
        xd, dyd, gd, ad = dev(d["x"]), dev(d["dy"], c.mis == "dy"), dev(d["g"]), dev(d.get("add"))
        md, rd = dev(mean32), dev(rstd32)
        return bufs, lambda: invoke("diqt_chan_layernorm_bwd_ex", xd, dyd, ad, gd, md, rd, bufs["dx"].t, bufs["dg"].t if bufs["dg"] else None,
                                    bufs["db"].t if bufs["db"] else None, bufs["workspace"].t, nws, rows, C, st)
    out = twice(c, k, ck, setup)
    if out:
        ck.close(out["dx"].t, ref["dx"], TOL_GRAD, "LayerNorm dx")
        for name in ("dg", "db"):
            if out[name] is not None:
                ck.close(out[name].t, ref[name], TOL_GRAD, "LayerNorm " + name)
    return plan.describe(c)


def check_l2(c, k, ck, d, ref_only):
    ref = plan.l2_ref(c, d)
    if ref_only:
        return "-"
    st = stream()
    rows, dd = c.rows, c.d
    y32 = torch.zeros(rows, c.ys)
    y32[:, :dd] = ref["y32"]
    xd, dyd, yd, ivd = dev(d["x"]), dev(d["dy"]), dev(y32), dev(ref["inv32"])

    def setup(k):
        bufs = {"y": Guarded((rows, c.ys), k=k), "inv": Guarded((rows,), k=k + 1) if c.inv else None, "dx": Guarded((rows, c.dxs), k=k + 2) if c.inv else None}

        def call():
            rc = invoke("diqt_l2norm_rows_fwd", xd, bufs["y"].t, bufs["inv"].t if c.inv else None, rows, dd, c.xs, c.ys, st)
            return rc or (invoke("diqt_l2norm_rows_bwd", yd, dyd, ivd, bufs["dx"].t, rows, dd, c.ys, c.dxs, st) if c.inv else 0)
        return bufs, call
    out = twice(c, k, ck, setup, cols={"y": dd, "dx": dd})
    if out:
        ck.close(out["y"].t[:, :dd], ref["y"], TOL_FWD, "l2norm y, per row", axis=1)
        if c.inv:
            ck.close(out["inv"].t[:, None], ref["inv"][:, None], TOL_FWD, "l2norm inv, per row", axis=1)
            ck.close(out["dx"].t[:, :dd], ref["dx"], TOL_GRAD, "l2norm dx, per row", axis=1)
    return plan.describe(c)


def check_asm(c, k, ck, d, ref_only):
    err, _ = plan.expect(c)
    ref = plan.asm_ref(c, d) if not err else None
    if ref_only:
        return "-"
    st = stream()
    G, n, h, E, ns, M = c.G, c.n, c.h, c.E, c.ns, c.E + c.ns
    reld, nulld = dev(d.get("rel")), dev(d.get("null"))
    if c.entry == "asm_fwd":
        simd = dev(d["sim"])

        def setup(k):
            bufs = {"p": Guarded((G, n, h, M), k=k)}
            return bufs, lambda: invoke("diqt_attn_softmax_fwd", simd, reld, nulld, bufs["p"].t, G, n, h, E, ns, c.causal, st)
        out = twice(c, k, ck, setup)
        if out:
            ck.close(out["p"].t, ref["p"], TOL_FWD, "attention p, per row", axis=3)
        return plan.describe(c)
    table = plan.asm_table(c)
    nws = _lib.query("diqt_attn_softmax_bwd_workspace_bytes", G, n, h, E, ns) if c.ws else 0
    pd = dev(ref["p32"]) if ref else torch.zeros(G, n, h, M, device=DEV)
    dpd = dev(d["dp"])

    def setup(k):
        acc = not table and not err          # the atomic kernel accumulates: zero-prefilled
        bufs = {"dsim": Guarded((G, n, h, M), k=k), "drel": Guarded((2 * ns - 1, h), k=k + 1, zero=acc) if c.rel else None,
                "dnull": Guarded((h,), k=k + 2, zero=acc) if c.null else None, "workspace": Guarded(None, k=k + 3, nbytes=nws) if nws else None}
        dr, dn = (bufs[x].t if bufs[x] else None for x in ("drel", "dnull"))
        if c.ws:
            return bufs, lambda: invoke("diqt_attn_softmax_bwd_ws", pd, dpd, bufs["dsim"].t, dr, dn, bufs["workspace"].t if nws else None, nws,
                                        G, n, h, E, ns, c.causal, st)
        return bufs, lambda: invoke("diqt_attn_softmax_bwd", pd, dpd, bufs["dsim"].t, dr, dn, G, n, h, E, ns, c.causal, st)
    out = twice(c, k, ck, setup, loose=() if table else ("drel", "dnull"))
    if out:
        ck.close(out["dsim"].t, ref["dsim"], TOL_GRAD, "attention dsim")
        for name in ("drel", "dnull"):
            if out[name] is not None:
                ck.close(out[name].t, ref[name], TOL_GRAD, "attention %s (%s)" % (name, "table" if table else "atomics"))
    return plan.describe(c)


RUN = {**{e: check_gn for e in plan._GN_ENTRIES}, "softmax": check_softmax, "ln_fwd": check_ln, "ln_bwd": check_ln, "l2": check_l2,
       "asm_fwd": check_asm, "asm_bwd": check_asm}


def main(family, seed, ref_only):
    _lib.load()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    cases = plan.cases(family, seed)
    total = sum(plan.ref_elems(c) for c in cases)
    assert total <= plan.MAX_ELEMS_SEED, "budget: %.3g reference elements" % total
    bad, t0, stats = 0, time.time(), {}
    for i, c in enumerate(cases):
        assert plan.ref_elems(c) <= plan.MAX_ELEMS_CASE and plan.largest_tensor_bytes(c) <= plan.MAX_TENSOR_BYTES, c
        gen = torch.Generator().manual_seed(1000 * seed + i)
        d = plan.inputs(c, gen)
        ck = Check(stats, c.data)
        ran = RUN[c.entry](c, i, ck, d, ref_only)
        bad += 1 if ck.why else 0
        print("case %3d %s data=%s %s plan[%s] %s" % (i, c.entry, c.data, " ".join("%s=%s" % kv for kv in c.kv if kv[1] not in ("", 0) or kv[0] in ("outer", "E")),
                                                       ran, "ok" if not ck.why else "FAIL: " + "; ".join(dict.fromkeys(ck.why))), flush=True)
    if stats:
        print("largest error / max|ref| (or ratio to the statistics bound): " + ", ".join("%s %s %.2e" % (d_, w, v) for (d_, w), v in sorted(stats.items())), flush=True)
    print("time: %.1f s, %.3g reference elements, %d threads" % (time.time() - t0, total, torch.get_num_threads()), flush=True)
    print("FUZZ_OK" if bad == 0 else "FUZZ_FAILED %d" % bad, flush=True)
    return 0 if bad == 0 else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], int(sys.argv[2]), "--reference-only" in sys.argv[3:]))
