"""Worker of tests/test_gpu_conv_fuzz.py: ``python tests/conv_fuzz_worker.py <family> <seed>`` runs the cases tests/conv_fuzz_plan.py
draws for (family, seed) through ops.conv3d -- forward, input gradient, weight and bias gradient -- against float64 convs on the host
(every element), twice for bit-for-bit run-to-run determinism, and compares the launches the library's census saw with the route the
plan predicted from the shape queries.  One process per (family, seed): a fault or hang ends at the caller's timeout.

Bounds: y and dX  max|got - ref| <= 2e-5 * max|ref| + 1e-6, dW and db the same with 5e-5 (tests/test_gpu_kernels.py: close() and the
module docstring); the f9small family keeps the 3e-5 forward and 1e-4 column-sum bounds it has always had.  The epilogue's per-tile sums
and sums of squares match those of the kernel's own y to 1e-5 * max.
"""
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from diffusioniqt_amd import ops, _lib
from tests import conv_fuzz_plan as plan

DEV = "cuda"


def cl(t):      # NCDHW host -> NDHWC device
    return t.permute(0, 2, 3, 4, 1).contiguous().to(DEV)


def cf(t):      # NDHWC device -> NCDHW host, float64
    return t.detach().cpu().permute(0, 4, 1, 2, 3).double()


def rel(got, ref):
    """(max|got - ref|, max|ref|)"""
    return (got.double() - ref).abs().max().item(), ref.abs().max().item()


def within(err_scale, tol):
    return err_scale[0] <= tol * err_scale[1] + 1e-6


def observed(c):
    """Exact launch counts per known tag (diqt_census_count matches substrings: a tag's count holds those of the longer tags around it)."""
    tags = sorted(set(plan.FWD_TAGS + plan.WG_TAGS + plan.FOREIGN_TAGS), key=len, reverse=True)
    exact = {}
    for t in tags:
        exact[t] = c.count(t) - sum(n for u, n in exact.items() if t in u)
    for stem in ("conv3d_fwd", "conv3d_bwd_weight", "conv_reduce_dw", "colsum"):
        assert c.count(stem) == sum(n for u, n in exact.items() if stem in u), "a launch tag this worker does not know: " + stem
    foreign = {t: n for t, n in exact.items() if n and t in plan.FOREIGN_TAGS}
    assert not foreign, f"launches outside the fp32 conv dispatch: {foreign}"
    fwd = {t: n for t, n in exact.items() if n and t in plan.FWD_TAGS}
    wg = {t: (1 if t == "weighted_colsum" else n) for t, n in exact.items() if n and t in plan.WG_TAGS}
    return fwd, wg


def run_gpu(case, x, w, b, r, dy):
    """One forward + backward; returns the results on the host and what ran."""
    B, D, H, W, Cin, Cout, k, pad, epad, res, grads = case
    xd = cl(x).requires_grad_("x" in grads)
    wd = w.to(DEV).requires_grad_("w" in grads)
    bd = b.to(DEV).requires_grad_("w" in grads)
    rd = cl(r).requires_grad_() if res else None
    dyd = cl(dy)
    _lib.query("diqt_get_last_conv_fwd9_variant")
    with _lib.census() as c:
        y = ops.conv3d(xd, wd, bd, pad, residual=rd, extra_pad=epad, want_stats=plan.want_stats(case))
        torch.cuda.synchronize()
    fwd_obs, wg0 = observed(c)
    assert not wg0, wg0
    fvar = _lib.query("diqt_get_last_conv_fwd9_variant")
    st = getattr(y, "_diqt_stats", None)
    with _lib.census() as c:
        y.backward(dyd)
        torch.cuda.synchronize()
    bwd_obs, wg_obs = observed(c)
    bvar = _lib.query("diqt_get_last_conv_fwd9_variant")
    return {"y": y.detach(), "dx": xd.grad, "dw": wd.grad, "db": bd.grad, "dr": rd.grad if res else None, "dy": dyd, "stats": st,
            "fwd_obs": fwd_obs, "fvar": fvar, "bwd_obs": bwd_obs, "bvar": bvar, "wg_obs": wg_obs}


def main(family, seed):
    _lib.load()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    f9small = family == "f9small"
    cases = plan.cases(family, seed)
    bad = 0
    t_ref = 0.0
    t0 = time.time()
    for i, case in enumerate(cases):
        B, D, H, W, Cin, Cout, k, pad, epad, res, grads = case
        T = k[0] * k[1] * k[2]
        Do, Ho, Wo = plan.out_extent(case)
        rt = plan.route(case)
        g = torch.Generator().manual_seed(1000 * seed + i)
        x = torch.randn(B, Cin, D, H, W, generator=g)
        w = torch.randn(Cout, Cin, *k, generator=g) / math.sqrt(Cin * T)
        b = torch.randn(Cout, generator=g)
        r = torch.randn(B, Cout, Do, Ho, Wo, generator=g) if res else None
        dy = torch.randn(B, Cout, Do, Ho, Wo, generator=g)
        # float64 reference: the explicitly padded input (low = pad, high = pad + extra_pad), every element, and its autograd
        tr = time.time()
        xr = x.double().requires_grad_("x" in grads)
        wr, br = w.double().requires_grad_("w" in grads), b.double().requires_grad_("w" in grads)
        xp = F.pad(xr, (pad[2], pad[2] + epad[2], pad[1], pad[1] + epad[1], pad[0], pad[0] + epad[0]))
        ref = F.conv3d(xp, wr, br)
        if res:
            ref = ref + r.double()
        ref.backward(dy.double())
        ref = ref.detach()
        t_ref += time.time() - tr

        why = []
        o = run_gpu(case, x, w, b, r, dy)
        e_y, e_dx, e_dw, e_db = rel(cf(o["y"]), ref), (0.0, 0.0), (0.0, 0.0), (0.0, 0.0)
        if not (e_y[0] / max(e_y[1], 1e-6) < 3e-5 if f9small else within(e_y, 2e-5)):
            why.append("y")
        if "x" in grads:
            e_dx = rel(cf(o["dx"]), xr.grad)
            if not within(e_dx, 2e-5):
                why.append("dX")
        elif o["dx"] is not None:
            why.append("dX given to an input that does not require grad")
        if "w" in grads:
            e_dw, e_db = rel(o["dw"].cpu(), wr.grad), rel(o["db"].cpu(), br.grad)
            if not within(e_dw, 5e-5):
                why.append("dW")
            if not within(e_db, 5e-5):
                why.append("db")
        elif o["dw"] is not None or o["db"] is not None:
            why.append("dW / db given to parameters that do not require grad")
        if res and not torch.equal(o["dr"], o["dy"]):
            why.append("d residual != dY")
        # statistics of the epilogue
        st = o["stats"]
        e_st = 0.0
        if (st is not None) != (plan.want_stats(case) and rt["fwd"]["stats_blocks"] > 0):
            why.append("statistics present = %s, diqt_conv3d_fwd_stats_blocks_pk = %d" % (st is not None, rt["fwd"]["stats_blocks"]))
        if st is not None:
            y64 = o["y"].double()
            if st.rows != Do * Ho * Wo or st.nblk != rt["fwd"]["stats_blocks"]:
                why.append("statistics rows / blocks")
            for j, own in ((0, y64.sum(dim=(1, 2, 3))), (1, (y64 * y64).sum(dim=(1, 2, 3)))):
                e = rel(st.partials[:, :, j, :].double().sum(1).cpu(), own.cpu())
                e_st = max(e_st, e[0] / max(e[1], 1e-30))
                if not within(e, 1e-5):
                    why.append("statistics[%d]" % j)
            if f9small:      # the bound this family has always held against the float64 column sums
                e = rel(st.partials[:, :, 0, :].double().sum(1).cpu(), ref.sum(dim=(2, 3, 4)))
                if not e[0] / max(e[1], 1e-6) < 1e-4:
                    why.append("column sums vs float64")
        # a second run on the same inputs: bit-identical
        o2 = run_gpu(case, x, w, b, r, dy)
        for name in ("y", "dx", "dw", "db"):
            if (o[name] is None) != (o2[name] is None) or (o[name] is not None and not torch.equal(o[name], o2[name])):
                why.append(name + " differs between two runs")
        # observed route = planned route
        obs = "fwd=%s/v%d bwd=%s/v%d wg=%s" % ("+".join(sorted(o["fwd_obs"])), o["fvar"], "+".join(sorted(o["bwd_obs"])) or "-", o["bvar"],
                                               "+".join(sorted(o["wg_obs"])) or "-")
        for run in (o, o2):
            if run["fwd_obs"] not in plan.fwd_tags(rt["fwd"]) or run["fvar"] != rt["fwd"]["variant"]:
                why.append("forward route")
            if rt["bwd_data"] is None:
                if run["bwd_obs"] or run["bvar"] != -1:
                    why.append("backward-data ran without need")
            elif run["bwd_obs"] not in plan.fwd_tags(rt["bwd_data"]) or run["bvar"] != rt["bwd_data"]["variant"]:
                why.append("backward-data route")
            if run["wg_obs"] != (plan.wgrad_tags(rt["wgrad"]) if rt["wgrad"] else {}):
                why.append("weight-gradient route")
        bad += 1 if why else 0
        kid = rt["fwd"]["kid"]
        print(f"case {i:2d} kid={kid} k={k} B={B} {D}x{H}x{W} {Cin}->{Cout} pad={pad} epad={epad} res={res} grads={grads} "
              f"plan[{plan.describe(rt)}] ran[{obs}] y={e_y[0] / max(e_y[1], 1e-30):.2e} dx={e_dx[0] / max(e_dx[1], 1e-30):.2e} "
              f"dw={e_dw[0] / max(e_dw[1], 1e-30):.2e} db={e_db[0] / max(e_db[1], 1e-30):.2e} stats={e_st:.2e} "
              f"{'ok' if not why else 'FAIL: ' + '; '.join(dict.fromkeys(why))}", flush=True)
    print(f"time: {time.time() - t0:.1f} s, of which float64 reference {t_ref:.1f} s, {torch.get_num_threads()} threads", flush=True)
    print("FUZZ_OK" if bad == 0 else f"FUZZ_FAILED {bad}", flush=True)
    return 0 if bad == 0 else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], int(sys.argv[2])))
