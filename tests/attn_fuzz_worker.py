"""Worker of tests/test_gpu_attn_fuzz.py: ``python tests/attn_fuzz_worker.py <family> <seed> [--reference-only]`` runs the cases
tests/attn_fuzz_plan.py draws for (family, seed) through the C entry points of the fused multi-query attention (``_lib.call``, no ops
layer in between) and compares every result with the float64 formula of plan.mqa_ref and its autograd.

* Every output and the backward's workspace is a view at a 16-byte-aligned offset inside a larger buffer: the payload prefilled with 0xFF
  bytes (a NaN in fp32, fp16 and bf16), the guard regions around it with 0xA5.  After the call the guards must be untouched and no output
  may hold a NaN (a row the kernel forgot).  The workspace view has exactly diqt_mqa_attention_bwd_workspace_bytes bytes.
* fp32 tolerances, the project's own (tests/test_gpu_kernels.py), through its ``close`` rule ``err <= tol * max|ref| + 1e-6``: 3e-5 for out
  and lse (against float64 logsumexp), 1e-4 for dq, dkv, drel, dnull -- for every data class.
* 16-bit: the model and bound of test_fused_attention_low_precision -- float64 attention of the operands as the kernel rounds them (scaled
  q, k, v to 16 bit), ``err <= 2.5 ulp * max|ref|``, with round_out 0 and 1 alike; the 16-bit copy of kv must equal torch's rounding.
* ``frames``: torch.equal to diqt_mqa_attention_fwd on the (b p) f (h d) transposed copies with the null row concatenated in front, and
  within the fp32 tolerance of float64.
* The launches the census saw must be exactly those of the route (plan.bwd_tags; one mqa_attention_fwd_h and one cast_to_h), every case runs
  twice with bit-identical outputs, and a refusal must return an error, launch nothing and leave its prefilled outputs untouched.
* Every tenth case of ``bwd32`` also goes through ops.mqa_attention with autograd: the same bits, gradients exactly for the inputs given.

``--reference-only`` runs everything but the GPU calls, and additionally evaluates the same formula and its autograd in plain fp32 PyTorch
on the CPU; the largest error of that evaluation against float64, per data class and output, relative to max|ref|, is printed at the end.
Rule for a data class whose legitimate fp32 rounding exceeds the project's tolerance: its bound becomes 4 x that error (the 4 allows for
a different summation order).  No class needs it.  Measured over the three seeds of ``bwd32`` (largest per output over the classes): out
3.3e-6 (peaked), lse 7.1e-7 (late), dq 1.2e-5 (late), dkv 2.9e-6 (peaked), drel 2.3e-6 (peaked), dnull 3.3e-5 (first); over ``fwd32``:
out 3.2e-6 (peaked), lse 5.7e-7 (first).  The constructed ``residue`` cases (one-hot soft-max: see the plan) are judged by that rule plus
residue_ceiling below and stay out of these figures.

One process per (family, seed): a fault or hang ends at the caller's timeout.
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from diffusioniqt_amd import ops, _lib
from tests import attn_fuzz_plan as plan

DEV = "cuda"
GUARD = 4096
TOL_OUT, TOL_GRAD = 3e-5, 1e-4
DT = {0: torch.float16, 1: torch.bfloat16}
ULP = {0: 2.0 ** -10, 1: 2.0 ** -7}
FWD_TAGS = ("mqa_attention_fwd", "mqa_attention_fwd_lse", "mqa_attention_fwd_frames", "mqa_attention_fwd_h", "cast_to_h")
ALL_TAGS = sorted(FWD_TAGS + plan.BWD_TAGS, key=len, reverse=True)


class Guarded:
    """A tensor at a 16-byte-aligned offset inside a larger buffer: payload 0xFF bytes (NaN), guards 0xA5."""

    def __init__(self, shape, dtype=torch.float32, k=0, nbytes=None):
        self.off = GUARD + 16 * (1 + k % 5)
        self.n = nbytes if nbytes is not None else torch.Size(shape).numel() * torch.empty((), dtype=dtype).element_size()
        self.raw = torch.full((self.off + self.n + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
        pay = self.raw[self.off:self.off + self.n]
        pay.fill_(0xFF)
        self.t = pay.view(dtype).view(shape) if nbytes is None else pay
        assert self.t.data_ptr() % 16 == 0

    def guards_intact(self):
        return bool((self.raw[:self.off] == 0xA5).all()) and bool((self.raw[self.off + self.n:] == 0xA5).all())

    def untouched(self):
        return self.guards_intact() and bool((self.raw[self.off:self.off + self.n] == 0xFF).all())


def observed(cen):
    """{tag: launches} with exact tags -- diqt_census_count matches substrings -- and nothing this worker does not know"""
    exact = {}
    for t in ALL_TAGS:
        exact[t] = cen.count(t) - sum(n for u, n in exact.items() if t in u)
    assert cen.count(None) == sum(exact.values()), "a launch tag this worker does not know"
    return {t: n for t, n in exact.items() if n}


def rel_err(got, ref):
    """(error, max|ref|) in float64"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    return (got - ref).abs().max().item(), ref.abs().max().item()


class Check:
    def __init__(self, stats, data):
        self.why, self.stats, self.data = [], stats, data

    def close(self, got, ref, tol, what, rep=1, ceiling=None):
        if got.shape != ref.shape and rep > 1:
            ref = plan.tile(ref, rep)
        err, scale = rel_err(got, ref)
        if ceiling is None:
            key = (self.data, what)
            self.stats[key] = max(self.stats.get(key, 0.0), err / max(scale, 1e-30))
        if not err <= tol * scale + 1e-6 + (ceiling or 0.0):
            self.why.append("%s: max err %.3e vs scale %.3e (bound %.1e%s)" % (what, err, scale, tol, " + %.1e" % ceiling if ceiling else ""))

    def guards(self, bufs, what):
        for name, b in bufs.items():
            if b is None:
                continue
            if not b.guards_intact():
                self.why.append("%s: %s written outside its buffer" % (what, name))
            elif b.t.dtype.is_floating_point and bool(torch.isnan(b.t).any()):
                self.why.append("%s: %s has rows nobody wrote" % (what, name))


def dev(t, rep=1):
    if t is None:
        return None
    return plan.tile(t, rep).contiguous().to(DEV)


def stream():
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------------------------------------------------------------------------
def reference(c, q, kv, rel, nb, up, dtype=torch.float64):
    """{"out", "lse"} and, for a backward case, {"dq", "dkv", "drel", "dnull"} (table gradients of all G sequences) in ``dtype``"""
    grad = c.entry == "bwd"
    leaf = lambda t: t.to(dtype).requires_grad_(grad) if t is not None else None
    qr, kvr, relr, nbr = leaf(q), leaf(kv), leaf(rel), leaf(nb)
    out, lse = plan.mqa_ref(qr, kvr, relr, nbr, c.n, c.h, c.d, c.E, c.causal, c.d ** -0.5, n_self=c.ns, with_lse=True)
    r = {"out": out.detach(), "lse": lse.detach()}
    if grad:
        out.backward(up.to(dtype))
        r.update(dq=qr.grad, dkv=kvr.grad, drel=relr.grad * c.rep if c.rel else None, dnull=nbr.grad * c.rep if c.null else None)
    return r


def residue_ceiling(c, q, kv, up):
    """Absolute allowances for the gradients of a ``residue`` case (plan.residue), on top of the relative rule.  dP[row, j] = dO . v_j and
    delta[row] = dO . O are fp32 sums of d products, each wrong by at most d u sum_i |dO_i| max_j |v_j,i| =: d u A (u = 2^-24); O is itself
    a rounded convex combination of M value rows (M + 4 more u).  So dP - delta carries at most e = (2 d + M + 4) u A, doubled for the
    rounding of P = exp(S - lse), while its exact value is (1 - p_max) small: dS = P (dP - delta) is wrong by up to e_s = 2 e per row.
    From there, with sum_j p_j = 1: |dq| <= scale e_s max|k|, |dk| <= scale n h e_s max|q|, and an entry of drel or dnull sums one dS of
    at most G n rows.  A ceiling, not an estimate: the errors seen are 100 x smaller, but nothing tighter can be derived without a model of
    the summation order, and the exact gradients are of the same size or zero."""
    Gu, d, M = q.shape[0], c.d, plan.keys(c)
    A = (up.double().reshape(Gu, c.n * c.h, d).abs() * kv.double()[..., d:].abs().amax(1)[:, None, :]).sum(-1).max().item()
    e_s = 2.0 * (2 * d + M + 4) * 2.0 ** -24 * A
    scale = d ** -0.5
    return {"dq": scale * e_s * kv[..., :d].abs().max().item(), "dk": scale * c.n * c.h * e_s * q.abs().max().item(),
            "drel": c.G * c.n * e_s, "dnull": c.G * c.n * e_s}


def fp32_formula_error(c, ref, q, kv, rel, nb, up, fp32_stats):
    r32 = reference(c, q, kv, rel, nb, up, dtype=torch.float32)
    for name, t in r32.items():
        if t is not None:
            err, scale = rel_err(t, ref[name])
            key = (c.data, name)
            fp32_stats[key] = max(fp32_stats.get(key, 0.0), err / max(scale, 1e-30))


def run_fwd32(c, k, q, kv, rel, nb):
    """one call of the case's entry point -> (outputs by name, guarded buffers, launches)"""
    G, hd, scale = c.G, c.h * c.d, c.d ** -0.5
    qd, kvd, reld, nbd = dev(q, c.rep), dev(kv, c.rep), dev(rel), dev(nb)
    bufs = {"out": Guarded((G, c.n, hd), k=k), "lse": Guarded((G, c.n * c.h), k=k + 1) if c.entry == "lse" else None}
    with _lib.census() as cen:
        if c.entry == "frames":
            B, F, P = G // c.P, c.n, c.P
            qf = qd.view(B, P, F, hd).permute(0, 2, 1, 3).contiguous()
            kvf = kvd[:, 1:].reshape(B, P, F, 2 * c.d).permute(0, 2, 1, 3).contiguous()
            nullkv = kvd[0, 0].clone()
            bufs["out"] = Guarded((B, F, P, hd), k=k)
            _lib.call("diqt_mqa_attention_fwd_frames", qf, kvf, nullkv, reld, nbd, bufs["out"].t, B, F, P, c.h, c.d, int(c.causal), scale, stream())
        elif c.entry == "lse":
            _lib.call("diqt_mqa_attention_fwd_lse", qd, kvd, reld, nbd, bufs["out"].t, bufs["lse"].t, G, c.n, c.h, c.d, c.E, c.ns, int(c.causal),
                      scale, stream())
        else:
            _lib.call("diqt_mqa_attention_fwd", qd, kvd, reld, nbd, bufs["out"].t, G, c.n, c.h, c.d, c.E, c.ns, int(c.causal), scale, stream())
        torch.cuda.synchronize()
    tags = observed(cen)
    res = {"out": bufs["out"].t, "lse": bufs["lse"].t if bufs["lse"] else None}
    if c.entry == "frames":
        res["out"] = res["out"].permute(0, 2, 1, 3).reshape(G, c.n, hd)
        twin = Guarded((G, c.n, hd), k=k + 2)
        _lib.call("diqt_mqa_attention_fwd", qd, kvd, reld, nbd, twin.t, G, c.n, c.h, c.d, 1, c.n, int(c.causal), scale, stream())
        torch.cuda.synchronize()
        bufs["out of the transposed copies"] = twin
        res["twin"] = twin.t
    return res, bufs, tags


def check_fwd32(c, k, ck, ref, q, kv, rel, nb):
    runs = [run_fwd32(c, k + 3 * i, q, kv, rel, nb) for i in range(2)]
    tag = {"fwd": "mqa_attention_fwd", "lse": "mqa_attention_fwd_lse", "frames": "mqa_attention_fwd_frames"}[c.entry]
    for res, bufs, tags in runs:
        ck.guards(bufs, c.entry)
        if tags != {tag: 1}:
            ck.why.append("launches %s" % tags)
    res = runs[0][0]
    ck.close(res["out"], ref["out"], TOL_OUT, "out", c.rep)
    if c.entry == "lse":
        ck.close(res["lse"], ref["lse"], TOL_OUT, "lse", c.rep)
    if c.entry == "frames" and not torch.equal(res["out"], res["twin"]):
        ck.why.append("frames differs from diqt_mqa_attention_fwd on transposed copies (max |diff| %g)" % (res["out"] - res["twin"]).abs().max().item())
    for name in res:
        if res[name] is not None and not torch.equal(res[name], runs[1][0][name]):
            ck.why.append(name + " differs between two runs")
    return "+".join(sorted(runs[0][2]))


def run_bwd32(c, k, rt, dv):
    """forward with lse, then the backward, through guarded buffers -> (error text or None, outputs, buffers, launches of the backward)"""
    G, hd, M, scale = c.G, c.h * c.d, plan.keys(c), c.d ** -0.5
    qd, kvd, reld, nbd, upd = dv
    fw = {"out": Guarded((G, c.n, hd), k=k), "lse": Guarded((G, c.n * c.h), k=k + 1)}
    _lib.call("diqt_mqa_attention_fwd_lse", qd, kvd, reld, nbd, fw["out"].t, fw["lse"].t, G, c.n, c.h, c.d, c.E, c.ns, int(c.causal), scale, stream())
    nws = _lib.query("diqt_mqa_attention_bwd_workspace_bytes", G, c.n, c.h, c.d, c.E, c.ns, int(c.rel))
    bw = {"dq": Guarded((G, c.n, hd), k=k + 2), "dkv": Guarded((G, M, 2 * c.d), k=k + 3),
          "drel": Guarded((2 * c.ns - 1, c.h), k=k + 4) if c.rel else None, "dnull": Guarded((c.h,), k=k) if c.null else None,
          "workspace": Guarded(None, k=k + 1, nbytes=nws)}
    err = None
    torch.cuda.synchronize()
    with _lib.census() as cen:
        try:
            _lib.call("diqt_mqa_attention_bwd", qd, kvd, reld, nbd, fw["out"].t, upd, fw["lse"].t, bw["dq"].t, bw["dkv"].t,
                      bw["drel"].t if c.rel else None, bw["dnull"].t if c.null else None, bw["workspace"].t, nws, G, c.n, c.h, c.d, c.E, c.ns,
                      int(c.causal), scale, stream())
        except RuntimeError as e:
            err = str(e)
        torch.cuda.synchronize()
    tags = observed(cen)
    return err, {**{n: b.t for n, b in fw.items()}, **{n: (b.t if b else None) for n, b in bw.items() if n != "workspace"}}, {**fw, **bw}, tags


def check_bwd32(c, k, ck, ref, q, kv, rel, nb, up, with_ops):
    rt = plan.route_bwd(c)
    dv = (dev(q, c.rep), dev(kv, c.rep), dev(rel), dev(nb), dev(up, c.rep))
    runs = [run_bwd32(c, k + 2 * i, rt, dv) for i in range(2)]
    for err, res, bufs, tags in runs:
        ck.guards({n: bufs[n] for n in ("out", "lse")}, "forward")
        if rt["path"] == 0:
            if err is None:
                ck.why.append("a refusal was taken")
            if tags:
                ck.why.append("a refusal launched %s" % tags)
            for n in ("dq", "dkv", "drel", "dnull", "workspace"):
                if bufs[n] is not None and not bufs[n].untouched():
                    ck.why.append("a refusal wrote " + n)
            continue
        if err is not None:
            ck.why.append("refused: " + err)
            continue
        ck.guards({n: b for n, b in bufs.items() if n != "workspace"}, "backward")
        if not bufs["workspace"].guards_intact():
            ck.why.append("backward: written outside the workspace")
        if tags != plan.bwd_tags(rt, c):
            ck.why.append("launches %s, planned %s" % (tags, plan.bwd_tags(rt, c)))
    res = runs[0][1]
    ck.close(res["out"], ref["out"], TOL_OUT, "out", c.rep)
    ck.close(res["lse"], ref["lse"], TOL_OUT, "lse", c.rep)
    if rt["path"] and runs[0][0] is None and runs[1][0] is None:
        ceil = residue_ceiling(c, q, kv, up) if plan.residue(c) else {}
        for name in ("dq", "drel", "dnull"):
            if ref[name] is not None:
                ck.close(res[name], ref[name], TOL_GRAD, name, c.rep if name == "dq" else 1, ceil.get(name))
        if ceil:        # dv = P^T dO does not pass through dP - delta: the relative rule alone
            dkv_ref = plan.tile(ref["dkv"], c.rep)
            ck.close(res["dkv"][..., :c.d], dkv_ref[..., :c.d], TOL_GRAD, "dk", 1, ceil["dk"])
            ck.close(res["dkv"][..., c.d:], dkv_ref[..., c.d:], TOL_GRAD, "dv")
        else:
            ck.close(res["dkv"], ref["dkv"], TOL_GRAD, "dkv", c.rep)
        for name, t in res.items():
            if t is not None and not torch.equal(t, runs[1][1][name]):
                ck.why.append(name + " differs between two runs")
        if with_ops:
            leaf = lambda t: t.clone().requires_grad_() if t is not None else None
            qa, kva, rela, nba = leaf(dv[0]), leaf(dv[1]), leaf(dv[2]), leaf(dv[3])
            out = ops.mqa_attention(qa, kva, rela, nba, c.n, c.h, c.d, c.E, c.ns, c.causal, c.d ** -0.5)
            out.backward(dv[4])
            torch.cuda.synchronize()
            for name, got in (("out", out.detach()), ("dq", qa.grad), ("dkv", kva.grad), ("drel", rela.grad if c.rel else None),
                              ("dnull", nba.grad if c.null else None)):
                if (got is None) != (res[name] is None) or (got is not None and not torch.equal(got, res[name])):
                    ck.why.append("ops.mqa_attention: %s differs from the direct call" % name)
    return "+".join(sorted(runs[0][3])) or "refused"


def reference_fwd16(c, q, kv, rel, nb):
    dt = DT[c.bf16]
    qd = (q * c.d ** -0.5).to(dt).double()
    dbl = lambda t: t.double() if t is not None else None
    return {"out": plan.mqa_ref(qd, kv.to(dt).double(), dbl(rel), dbl(nb), c.n, c.h, c.d, c.E, c.causal, None, n_self=c.ns)}


def run_fwd16(c, k, q, kv, rel, nb):
    G, hd, M, scale = c.G, c.h * c.d, plan.keys(c), c.d ** -0.5
    qd, kvd, reld, nbd = dev(q, c.rep), dev(kv, c.rep), dev(rel), dev(nb)
    bufs = {"kv_h": Guarded((G, M, 2 * c.d), dtype=torch.int16, k=k), "out": Guarded((G, c.n, hd), k=k + 1)}
    with _lib.census() as cen:
        _lib.call("diqt_cast_to_h", kvd, bufs["kv_h"].t, kvd.numel(), c.bf16, stream())
        _lib.call("diqt_mqa_attention_fwd_h", qd, bufs["kv_h"].t, reld, nbd, bufs["out"].t, G, c.n, c.h, c.d, c.E, c.ns, int(c.causal), scale,
                  c.bf16, c.round_out, stream())
        torch.cuda.synchronize()
    return {"kv_h": bufs["kv_h"].t, "out": bufs["out"].t}, bufs, observed(cen), kvd


def check_fwd16(c, k, ck, ref, q, kv, rel, nb):
    dt = DT[c.bf16]
    runs = [run_fwd16(c, k + 2 * i, q, kv, rel, nb) for i in range(2)]
    for res, bufs, tags, kvd in runs:
        ck.guards(bufs, "fwd_h")
        if tags != {"cast_to_h": 1, "mqa_attention_fwd_h": 1}:
            ck.why.append("launches %s" % tags)
        if not torch.equal(res["kv_h"], kvd.to(dt).view(torch.int16)):
            ck.why.append("cast_to_h differs from torch's rounding")
    out = runs[0][0]["out"]
    err, scale = rel_err(out, plan.tile(ref["out"], c.rep))
    key = (c.data, "out, %s, in ulp" % ("bf16" if c.bf16 else "fp16"))
    ck.stats[key] = max(ck.stats.get(key, 0.0), err / max(scale, 1e-30) / ULP[c.bf16])
    if not err <= 2.5 * ULP[c.bf16] * scale:
        ck.why.append("out: max err %.3e vs scale %.3e (%.2f ulp, bound 2.5)" % (err, scale, err / scale / ULP[c.bf16]))
    if c.round_out and not torch.equal(out, out.to(dt).float()):
        ck.why.append("round_out = 1 left values that are not %s numbers" % dt)
    for name in ("kv_h", "out"):
        if not torch.equal(runs[0][0][name], runs[1][0][name]):
            ck.why.append(name + " differs between two runs")
    return "+".join(sorted(runs[0][2]))


def main(family, seed, ref_only):
    _lib.load()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    cases = plan.cases(family, seed)
    total = sum(plan.ref_macs(c) for c in cases)
    assert total <= plan.MAX_MACS_SEED, "budget: %.3g multiply-adds" % total
    bad, t_ref, t0 = 0, 0.0, time.time()
    stats, fp32_stats = {}, {}
    for i, c in enumerate(cases):
        assert plan.ref_macs(c) <= plan.MAX_MACS_CASE and plan.largest_tensor_bytes(c) <= plan.MAX_TENSOR_BYTES, c
        gen = torch.Generator().manual_seed(1000 * seed + i)
        q, kv, rel, nb, up = plan.inputs(c, gen)
        refused = c.entry == "bwd" and plan.route_bwd(c)["path"] == 0
        tr = time.time()
        ref = reference_fwd16(c, q, kv, rel, nb) if c.entry == "h" else reference(c._replace(entry="lse") if refused else c, q, kv, rel, nb, up)
        for name in ("dq", "dkv", "drel", "dnull"):
            ref.setdefault(name, None)
        t_ref += time.time() - tr
        ck = Check(stats, c.data)
        for name, t in ref.items():
            if t is not None and not bool(torch.isfinite(t).all()):
                ck.why.append("plan error: the reference's %s is not finite" % name)
        if ref_only:
            ran = "-"
            if c.entry != "h" and not refused and not plan.residue(c):
                fp32_formula_error(c, ref, q, kv, rel, nb, up, fp32_stats)
        elif c.entry == "h":
            ran = check_fwd16(c, i, ck, ref, q, kv, rel, nb)
        elif c.entry == "bwd":
            ran = check_bwd32(c, i, ck, ref, q, kv, rel, nb, up, with_ops=i % 10 == 0)
        else:
            ran = check_fwd32(c, i, ck, ref, q, kv, rel, nb)
        bad += 1 if ck.why else 0
        extra = (" P=%d" % c.P if c.entry == "frames" else "") + (" %s round_out=%d" % ("bf16" if c.bf16 else "fp16", c.round_out) if c.entry == "h" else "")
        print(f"case {i:3d} {c.entry} G={c.G} n={c.n} h={c.h} d={c.d} n_extra={c.E} n_self={c.ns} rel={int(c.rel)} null={int(c.null)} "
              f"causal={int(c.causal)} data={c.data} rep={c.rep}{extra} plan[{plan.describe(c)}] ran[{ran}] "
              f"{'ok' if not ck.why else 'FAIL: ' + '; '.join(dict.fromkeys(ck.why))}", flush=True)
    for title, table in (("largest error / max|ref|", stats), ("fp32 PyTorch formula on the CPU against float64, error / max|ref|", fp32_stats)):
        if table:
            print(title + ": " + ", ".join("%s %s %.2e" % (d, w, v) for (d, w), v in sorted(table.items())), flush=True)
    print(f"time: {time.time() - t0:.1f} s, of which float64 reference {t_ref:.1f} s, {total:.3g} multiply-adds, {torch.get_num_threads()} threads",
          flush=True)
    print("FUZZ_OK" if bad == 0 else f"FUZZ_FAILED {bad}", flush=True)
    return 0 if bad == 0 else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], int(sys.argv[2]), "--reference-only" in sys.argv[3:]))
