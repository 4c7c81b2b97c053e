"""Worker of tests/test_gpu_conv_fuzz_h.py: ``python tests/conv_fuzz_worker_h.py <family> <seed> [--reference-only]`` runs the cases
tests/conv_fuzz_plan_h.py draws for (family, seed) through the 16-bit conv dispatch on integer-valued data and compares every result with
``torch.equal`` against a float64 conv of the explicitly padded input (and its autograd), rounded ONCE to the operand type where the
planned route says a 16-bit kernel ran (y before the fp32 residual is added, dX of a mode-1 launch) and not rounded where it says fp32; dW
and db are never rounded.  Every case runs twice (bit-identical), and the launches the census saw -- and the conv_f9h_kernel variant --
must be the planned ones.  A refusal must return an error, launch nothing and leave its prefilled output untouched.

Statistics cases: the partials, summed over the blocks in float64, must equal the column sums and sums of squares of the stored y exactly;
that needs sum(y^2) < 2^24 per (batch entry, channel), which is checked on the reference -- a case outside it is a plan error.

``--reference-only`` runs everything but the GPU calls (references, the statistics bound, budgets): the plan can be checked without a GPU.
One process per (family, seed): a fault or hang ends at the caller's timeout.
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from diffusioniqt_amd import ops, _lib
from tests import conv_fuzz_plan as base
from tests import conv_fuzz_plan_h as plan

DEV = "cuda"
DT = {0: torch.float16, 1: torch.bfloat16}
ALL_TAGS = sorted(set(base.FWD_TAGS + base.WG_TAGS + base.FOREIGN_TAGS), key=len, reverse=True)
SENTINEL = 7.0


def cl(t):      # NCDHW host -> NDHWC device
    return t.permute(0, 2, 3, 4, 1).contiguous().to(DEV)


def cf(t):      # NDHWC device -> NCDHW host, float64
    return t.detach().cpu().permute(0, 4, 1, 2, 3).double()


def once(t, dt):
    """float64 integers (< 2^24: exact in fp32) rounded once to the operand type"""
    return t.float().to(dt).double()


def observed(c):
    """Exact launch counts per known tag, split into (forward-type, weight-gradient) -- diqt_census_count matches substrings."""
    exact = {}
    for t in ALL_TAGS:
        exact[t] = c.count(t) - sum(n for u, n in exact.items() if t in u)
    for stem in ("conv3d_fwd", "conv3d_bwd_weight", "conv_reduce_dw", "colsum"):
        assert c.count(stem) == sum(n for u, n in exact.items() if stem in u), "a launch tag this worker does not know: " + stem
    assert not exact["conv3d_fwd_gn(split-K reduce)"]
    fwd = {t: n for t, n in exact.items() if n and (t in base.FWD_TAGS or t in plan.H_FWD_TAGS)}
    wg = {t: (1 if t == "weighted_colsum" else n) for t, n in exact.items() if n and (t in base.WG_TAGS or t in plan.H_WG_TAGS)}
    return fwd, wg


def ints(g, lo, hi, shape):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def reference(c, x, w, b, r, dy, want_x, want_w):
    """float64: (y before the residual, dX, dW, db)"""
    xr = x.clone().requires_grad_(want_x)
    wr = w.clone().requires_grad_(want_w)
    xp = F.pad(xr, (c.pad[2], c.pad[2] + c.epad[2], c.pad[1], c.pad[1] + c.epad[1], c.pad[0], c.pad[0] + c.epad[0]))
    y = F.conv3d(xp, wr, b)
    if want_x or want_w:
        y.backward(dy)
    return y.detach(), xr.grad, wr.grad, (dy.sum(dim=(0, 2, 3, 4)) if dy is not None else None)


# ---------------------------------------------------------------------------------------------------------------------------------
def run_ops16(c, x, w, b, r, dy):
    xd = cl(x.float()).requires_grad_("x" in c.grads)
    wd = w.float().to(DEV).requires_grad_("w" in c.grads)
    bd = b.float().to(DEV).requires_grad_("w" in c.grads) if c.bias else None
    rd = cl(r.float()).requires_grad_() if c.res else None
    dyd = cl(dy.float())
    _lib.query("diqt_get_last_conv_f9h_variant")
    with _lib.census() as cen:
        with ops.low_precision("bf16" if c.prec == "bf16" else "fp16"):
            y = ops.conv3d(xd, wd, bd, c.pad, residual=rd, extra_pad=c.epad)
        torch.cuda.synchronize()
    fwd_obs, wg0 = observed(cen)
    assert not wg0, wg0
    with _lib.census() as cen:
        y.backward(dyd)
        torch.cuda.synchronize()
    bwd_obs, wg_obs = observed(cen)
    return {"y": y.detach(), "dx": xd.grad, "dw": wd.grad, "db": bd.grad if c.bias else None, "dr": rd.grad if c.res else None, "dy": dyd,
            "fwd_obs": fwd_obs, "bwd_obs": bwd_obs, "wg_obs": wg_obs, "f9h": _lib.query("diqt_get_last_conv_f9h_variant")}


def check_ops16(c, rt, g, ref_only):
    why = []
    Do, Ho, Wo = plan.out_extent(c)
    dt = DT[plan.LP[c.prec]]
    x = ints(g, -3, 3, (c.B, c.Cin, c.D, c.H, c.W))
    w = ints(g, -2, 2, (c.Cout, c.Cin, *c.k))
    b = ints(g, -4, 4, (c.Cout,)) if c.bias else None
    r = ints(g, -5, 5, (c.B, c.Cout, Do, Ho, Wo)) if c.res else None
    dy = ints(g, -2, 2, (c.B, c.Cout, Do, Ho, Wo))
    tr = time.time()
    y, dx, dw, db = reference(c, x, w, b, r, dy, "x" in c.grads, "w" in c.grads)
    assert y.abs().max().item() <= 62212 and (dx is None or dx.abs().max().item() <= 65504)
    if rt["fwd"]["half"]:
        y = once(y, dt)
    if c.res:
        y = y + r
    if dx is not None and rt["bwd_data"]["half"]:
        dx = once(dx, dt)
    t_ref = time.time() - tr
    if ref_only:
        return why, "-", t_ref
    prev = ops.FP16_BACKWARD
    ops.FP16_BACKWARD = c.prec == "fp16s"
    try:
        o, o2 = run_ops16(c, x, w, b, r, dy), run_ops16(c, x, w, b, r, dy)
    finally:
        ops.FP16_BACKWARD = prev
    if not torch.equal(cf(o["y"]), y):
        why.append("y (max |diff| %g)" % (cf(o["y"]) - y).abs().max().item())
    if "x" in c.grads:
        if not torch.equal(cf(o["dx"]), dx):
            why.append("dX (max |diff| %g)" % (cf(o["dx"]) - dx).abs().max().item())
    elif o["dx"] is not None:
        why.append("dX given to an input that does not require grad")
    if "w" in c.grads:
        if not torch.equal(o["dw"].cpu().double(), dw):
            why.append("dW (max |diff| %g)" % (o["dw"].cpu().double() - dw).abs().max().item())
        if c.bias and not torch.equal(o["db"].cpu().double(), db):
            why.append("db")
    elif o["dw"] is not None or o["db"] is not None:
        why.append("dW / db given to parameters that do not require grad")
    if c.res and not torch.equal(o["dr"], o["dy"]):
        why.append("d residual != dY")
    for name in ("y", "dx", "dw", "db"):
        if (o[name] is None) != (o2[name] is None) or (o[name] is not None and not torch.equal(o[name], o2[name])):
            why.append(name + " differs between two runs")
    for run in (o, o2):
        if run["fwd_obs"] not in plan.fwd_tags(rt["fwd"]):
            why.append("forward route")
        if rt["bwd_data"] is None:
            if run["bwd_obs"]:
                why.append("backward-data ran without need")
        elif run["bwd_obs"] not in plan.fwd_tags(rt["bwd_data"]):
            why.append("backward-data route")
        if run["wg_obs"] != (plan.wgrad_tags(rt["wgrad"], c.bias) if rt["wgrad"] else {}):
            why.append("weight-gradient route")
        if run["f9h"] != -1:
            why.append("conv_f9h_kernel ran behind ops.conv3d")
    obs = "fwd=%s bwd=%s wg=%s" % ("+".join(sorted(o["fwd_obs"])), "+".join(sorted(o["bwd_obs"])) or "-", "+".join(sorted(o["wg_obs"])) or "-")
    return why, obs, t_ref


# ---------------------------------------------------------------------------------------------------------------------------------
def census_total(cen):
    return sum(cen.count(s) for s in ("conv3d_fwd", "conv3d_bwd_weight", "conv_reduce_dw"))


def run_io16_fwd(c, rt, x, packed, b, r, dt):
    """-> (error or None, y, stats, tags seen, f9h variant)"""
    Do, Ho, Wo = plan.out_extent(c)
    st = torch.cuda.current_stream().cuda_stream
    xd = cl(x.float())
    xd = xd.to(dt) if c.xh else xd
    y = torch.full((c.B, Do, Ho, Wo, c.Cout), SENTINEL, dtype=dt if c.yh else torch.float32, device=DEV)
    nblk = rt.get("stats_blocks", 0)
    # (a refusal gets room for the rows of any launch, so that a wrongly taken one stays inside the buffer and shows)
    sbuf = torch.full((c.B, nblk if rt["ok"] else plan.stats_rows_bound(c), 2, c.Cout), -1.0, device=DEV) if c.stats else None
    _lib.query("diqt_get_last_conv_f9h_variant")
    err = None
    with _lib.census() as cen:
        try:
            _lib.call("diqt_conv3d_fwd_h_io", xd, packed, b, r, y, *plan.geo_of(c), c.bf16, 1, c.xh, c.yh, sbuf, st)
        except RuntimeError as e:
            err = str(e)
        torch.cuda.synchronize()
    fwd_obs, wg_obs = observed(cen)
    assert not wg_obs, wg_obs
    return err, y, sbuf, fwd_obs, _lib.query("diqt_get_last_conv_f9h_variant")


def check_io16_fwd(c, rt, g, ref_only):
    why = []
    Do, Ho, Wo = plan.out_extent(c)
    dt = DT[c.bf16]
    a = 1 if c.stats else 3
    x = ints(g, -a, a, (c.B, c.Cin, c.D, c.H, c.W))
    w = ints(g, -1 if c.stats else -2, 1 if c.stats else 2, (c.Cout, c.Cin, *c.k))
    b = ints(g, -1 if c.stats else -4, 1 if c.stats else 4, (c.Cout,))
    r = ints(g, -5, 5, (c.B, c.Cout, Do, Ho, Wo)) if c.res else None
    tr = time.time()
    y = None
    if rt["ok"] or ref_only:
        y, _, _, _ = reference(c, x, w, b, r, None, False, False)
        y = once(y, dt)
        if c.res:
            y = y + r
        if c.stats and rt["ok"]:
            bound = (y * y).sum(dim=(2, 3, 4)).max().item() / 2.0 ** 24
            if not bound < 1.0:
                why.append("plan error: sum(y^2) / 2^24 = %.2f for a statistics case" % bound)
            if rt["stats_blocks"] <= 0:
                why.append("plan error: a statistics case whose launch emits none")
    t_ref = time.time() - tr
    if ref_only:
        return why, "-", t_ref
    st = torch.cuda.current_stream().cuda_stream
    packed = torch.empty(_lib.query("diqt_conv_packed_h_elems", c.Cout, c.Cin, *c.k), dtype=torch.int16, device=DEV)
    _lib.call("diqt_conv_pack_weight_h", w.float().to(DEV), packed, c.Cout, c.Cin, *c.k, 0, c.bf16, st)
    bd, rd = b.float().to(DEV), (cl(r.float()) if c.res else None)
    with plan.switches(c.f9mode, c.wgs):
        runs = [run_io16_fwd(c, rt, x, packed, bd, rd, dt) for _ in range(2)]
    for err, yd, sbuf, tags, var in runs:
        if not rt["ok"]:
            if err is None:
                why.append("a refusal was taken")
            if tags or var != -1:
                why.append("a refusal launched %s" % (tags or var))
            if not bool((yd.float() == SENTINEL).all()):
                why.append("a refusal wrote y")
            if sbuf is not None and not bool((sbuf == -1.0).all()):
                why.append("a refusal wrote statistics")
            continue
        if err is not None:
            why.append("refused: " + err)
            continue
        if tags != {plan.HID_TAG[rt["hid"]]: 1} or var != rt["variant"]:
            why.append("route")
        if not torch.equal(cf(yd.float()), y):
            why.append("y (max |diff| %g)" % (cf(yd.float()) - y).abs().max().item())
        if c.stats:
            stored = yd.double().reshape(c.B, -1, c.Cout).cpu()
            s = sbuf.double().sum(1).cpu()
            if not torch.equal(s[:, 0], stored.sum(1)):
                why.append("statistics: sums")
            if not torch.equal(s[:, 1], (stored * stored).sum(1)):
                why.append("statistics: sums of squares")
    if rt["ok"] and runs[0][0] is None and runs[1][0] is None:
        if not torch.equal(runs[0][1], runs[1][1]) or (c.stats and not torch.equal(runs[0][2], runs[1][2])):
            why.append("two runs differ")
    return why, "%s/v%d" % ("+".join(sorted(runs[0][3])) or "refused", runs[0][4]), t_ref


def check_io16_wgrad(c, rt, g, ref_only):
    why = []
    Do, Ho, Wo = plan.out_extent(c)
    dt = DT[c.bf16]
    x = ints(g, -3, 3, (c.B, c.Cin, c.D, c.H, c.W))
    dy = ints(g, -2, 2, (c.B, c.Cout, Do, Ho, Wo))
    tr = time.time()
    dw = db = None
    if rt["ok"] or ref_only:
        _, _, dw, db = reference(c, x, torch.zeros(c.Cout, c.Cin, *c.k, dtype=torch.float64), None, None, dy, False, True)
    t_ref = time.time() - tr
    if ref_only:
        return why, "-", t_ref
    st = torch.cuda.current_stream().cuda_stream
    xd, dyd = cl(x.float()), cl(dy.float())
    xd = xd.to(dt) if c.xh else xd
    dyd = dyd.to(dt) if c.yh else dyd
    nbytes = max(rt["nbytes"], 1 << 16)
    ws = torch.empty(nbytes // 4, device=DEV)
    outs = []
    for _ in range(2):
        dwd = torch.full((c.Cout, c.Cin, *c.k), SENTINEL, device=DEV)
        dbd = torch.full((c.Cout,), SENTINEL, device=DEV)
        err = None
        with _lib.census() as cen:
            try:
                _lib.call("diqt_conv3d_bwd_weight_h", xd, dyd, dwd, dbd, ws, nbytes, *plan.geo_of(c), c.bf16 | (2 if c.xh else 0) | (4 if c.yh else 0), st)
            except RuntimeError as e:
                err = str(e)
            torch.cuda.synchronize()
        fwd_obs, wg_obs = observed(cen)
        if not rt["ok"]:
            if err is None:
                why.append("a refusal was taken")
            if fwd_obs or wg_obs:
                why.append("a refusal launched %s" % (wg_obs or fwd_obs))
            if not bool((dwd == SENTINEL).all()) or not bool((dbd == SENTINEL).all()):
                why.append("a refusal wrote dW / db")
            continue
        if err is not None:
            why.append("refused: " + err)
            continue
        if fwd_obs or wg_obs != {t: 1 for t in plan.H_WG_TAGS}:
            why.append("route")
        if not torch.equal(dwd.cpu().double(), dw):
            why.append("dW (max |diff| %g)" % (dwd.cpu().double() - dw).abs().max().item())
        if not torch.equal(dbd.cpu().double(), db):
            why.append("db")
        outs.append((dwd, dbd))
    if len(outs) == 2 and not (torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])):
        why.append("two runs differ")
    return why, "wgrad_h" if rt["ok"] else "refused", t_ref


def main(family, seed, ref_only):
    _lib.load()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    cases = plan.cases(family, seed)
    total = sum(plan.ref_macs(c) for c in cases)
    assert total <= plan.MAX_MACS_SEED, "budget: %.3g multiply-adds" % total
    bad = 0
    t_ref = 0.0
    t0 = time.time()
    for i, c in enumerate(cases):
        g = torch.Generator().manual_seed(1000 * seed + i)
        if family == "ops16":
            rt = plan.route_ops16(c)
            why, obs, tr = check_ops16(c, rt, g, ref_only)
            planned = plan.describe_ops16(rt)
            what = f"{c.prec} bias={int(c.bias)} res={int(c.res)} grads={c.grads}"
        else:
            rt = plan.route_io16(c)
            why, obs, tr = (check_io16_wgrad if c.op == "wgrad" else check_io16_fwd)(c, rt, g, ref_only)
            planned = ("refused" if not rt["ok"] else "wgrad_h/ks%d" % rt["ksplit"] if c.op == "wgrad" else "h%d/v%d" % (rt["hid"], rt["variant"]))
            what = f"{c.op} {'bf16' if c.bf16 else 'fp16'} xh={c.xh} yh={c.yh} res={int(c.res)} stats={int(c.stats)} f9h_mode={c.f9mode} wgs={c.wgs}"
        t_ref += tr
        bad += 1 if why else 0
        print(f"case {i:3d} k={c.k} B={c.B} {c.D}x{c.H}x{c.W} {c.Cin}->{c.Cout} pad={c.pad} epad={c.epad} {what} plan[{planned}] ran[{obs}] "
              f"{'ok' if not why else 'FAIL: ' + '; '.join(dict.fromkeys(why))}", flush=True)
    print(f"time: {time.time() - t0:.1f} s, of which float64 reference {t_ref:.1f} s, {total:.3g} multiply-adds, {torch.get_num_threads()} threads",
          flush=True)
    print("FUZZ_OK" if bad == 0 else f"FUZZ_FAILED {bad}", flush=True)
    return 0 if bad == 0 else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], int(sys.argv[2]), "--reference-only" in sys.argv[3:]))
