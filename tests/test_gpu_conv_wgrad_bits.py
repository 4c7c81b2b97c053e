"""The output BITS of ``diqt_conv3d_bwd_weight`` and ``diqt_conv3d_bwd_weight_h``, frozen, on the smallest shapes that reach each of
the launch's paths, and the refusals that return before any launch.

tests/golden/conv_wgrad_bits.json holds, per case, the SHA-256 of the bytes of ``dw`` and ``db`` of a call with a bias gradient and of
``dw`` of a call without one.  It was recorded on an MI355X from commit 411bfd2, the last one whose launch, workspace query and kernel-id
query each held a copy of the dispatch rules, and is what folding them into one route (``convw_route``) had to keep: it is not to be
regenerated from later code.  The weight gradient is deterministic (fixed-order slab sums), so digests are the freeze: no tolerance.
With ``DIQT_CONV_WGRAD_BITS_DUMP=<file>`` every case merges its digests into that JSON file instead of comparing them; the cases only
call entries that commit exports, so the recorder runs on either tree.

Inputs: ``np.random.default_rng(<case index>)`` standard normals cast to fp32 on the host (non-integer, so a change of summation order
changes bits); the calls go to the library directly with the workspace its query asks for, filled with NaN bit patterns (a launch that
read a share it had not written would show)."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from diffusioniqt_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_wgrad_bits.json")
K333, K133, K311, K111 = (3, 3, 3), (1, 3, 3), (3, 1, 1), (1, 1, 1)
COLSUM, IM2COL, PW, V3, V2, V1 = range(6)          # diqt_conv3d_bwd_weight_route, field 1


def _case(B, sp, Cin, Cout, k, causal=False):
    pad, epad = tuple(kk // 2 for kk in k), (0, 0, 0)
    if causal:
        pad, epad = (k[0] - 1, 0, 0), (-(k[0] - 1), 0, 0)
    return (B, *sp, Cin, Cout, *k, *pad, *epad)


# name -> (geometry, path of the launch, x at a 4-byte offset into its storage)
CASES = {
    "v3": (_case(2, (8, 10, 12), 16, 24, K333), V3, False),
    "v3, several tiles per workgroup": (_case(1, (16, 32, 36), 32, 32, K333), V3, False),
    "v3 causal": (_case(2, (40, 16, 18), 32, 48, K311, causal=True), V3, False),
    "v3 pointwise": (_case(2, (8, 8, 12), 48, 136, K111), V3, False),
    "v2, 3 taps": (_case(2, (9, 6, 7), 33, 7, K311), V2, False),
    "v2, 9 taps": (_case(2, (5, 12, 11), 12, 40, K133), V2, False),
    "v2, 27 taps": (_case(1, (7, 9, 10), 20, 22, K333), V2, False),
    "v2, 49 taps": (_case(2, (6, 8, 8), 8, 40, (1, 7, 7)), V2, False),
    "v1": (_case(1, (6, 12, 12), 20, 24, (5, 5, 5)), V1, False),
    "1x1x1 GEMM, dY first": (_case(2, (8, 16, 16), 62, 68, K111), PW, False),
    "1x1x1 GEMM, x first": (_case(2, (8, 16, 16), 68, 62, K111), PW, False),
    "im2col": (_case(2, (8, 16, 16), 3, 20, K333), IM2COL, False),
    "column sum": (_case(1, (16, 16, 16), 64, 1, K111), COLSUM, False),
    "unaligned fallback": (_case(2, (8, 10, 12), 16, 24, K333), V2, True),
}
KERNEL_IDS = {COLSUM: 0, IM2COL: 0, PW: 0, V3: 3, V2: 2, V1: 1}
# name -> (geometry, the `bf16` argument: 1 bf16 operands, 2: x holds 16-bit values, 4: dY holds 16-bit values)
H_CASES = {
    "h, flags 1": (_case(2, (8, 8, 8), 32, 32, K333), 1),
    "h, flags 1|2|4": (_case(2, (4, 8, 8), 32, 64, K133), 1 | 2 | 4),
}


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def out_extent(g):
    return tuple(g[1 + i] + 2 * g[9 + i] + g[12 + i] - g[6 + i] + 1 for i in range(3))


def tensors(name, g, offset=False, x16=False, dy16=False):
    """x [B,D,H,W,Cin] and dY [B,Do,Ho,Wo,Cout] on the device; ``offset``: x starts 4 bytes into its storage"""
    rng = np.random.default_rng((list(CASES) + list(H_CASES)).index(name))
    B, D, H, W, Cin, Cout = g[:6]
    x = rng.standard_normal((B, D, H, W, Cin)).astype(np.float32)
    dy = rng.standard_normal((B, *out_extent(g), Cout)).astype(np.float32)
    xd, dyd = torch.from_numpy(x).to(DEV), torch.from_numpy(dy).to(DEV)
    if offset:
        store = torch.empty(x.size + 1, dtype=torch.float32, device=DEV)
        store[1:] = xd.reshape(-1)
        xd = store[1:].view(x.shape)
        assert xd.data_ptr() % 16 == 4
    if x16:
        xd = xd.to(torch.bfloat16)
    if dy16:
        dyd = dyd.to(torch.bfloat16)
    return xd, dyd


def workspace(nbytes):
    assert nbytes > 0
    return torch.full(((nbytes + 3) // 4,), -1, dtype=torch.int32, device=DEV)          # 0xffffffff: NaN as fp32


def run(entry, ws_query, g, x, dy, *tail):
    """{"dw", "db", "dw_nobias"} digests of the two calls"""
    Cin, Cout, k = g[4], g[5], g[6:9]
    n = _lib.query(ws_query, *g)
    stream = torch.cuda.current_stream().cuda_stream
    out = {}
    for want_bias in (True, False):
        dw = torch.full((Cout, Cin, *k), float("nan"), dtype=torch.float32, device=DEV)
        db = torch.full((Cout,), float("nan"), dtype=torch.float32, device=DEV) if want_bias else None
        _lib.call(entry, x, dy, dw, db, workspace(n), n, *g, *tail, stream)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(dw).all()) and (db is None or bool(torch.isfinite(db).all())), (entry, g, want_bias)
        if want_bias:
            out["dw"], out["db"] = sha(dw), sha(db)
        else:
            out["dw_nobias"] = sha(dw)
    return out


def compare(name, got):
    where = os.environ.get("DIQT_CONV_WGRAD_BITS_DUMP")
    if where:
        table = {}
        if os.path.exists(where):
            with open(where) as f:
                table = json.load(f)
        table[name] = got
        with open(where, "w") as f:
            json.dump(table, f, indent=0, sort_keys=True)
        return
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert sorted(golden) == sorted(list(CASES) + list(H_CASES))
    bad = sorted(k for k in set(got) | set(golden[name]) if got.get(k) != golden[name].get(k))
    assert not bad, f"{name}: {bad} differ from the recorded bits"


@pytest.mark.parametrize("name", list(CASES))
def test_fp32_output_bits_are_the_recorded_ones(name):
    g, path, offset = CASES[name]
    x, dy = tensors(name, g, offset)
    assert offset or _lib.query("diqt_conv3d_bwd_weight_kernel_id", *g) == KERNEL_IDS[path], name
    if "diqt_conv3d_bwd_weight_route" in _lib.PROTOTYPES:            # (the recorder also runs on the commit before the route)
        for want_bias in (0, 1):
            assert _lib.query("diqt_conv3d_bwd_weight_route", *g, int(not offset), want_bias, 1) == path, (name, want_bias)
    got = run("diqt_conv3d_bwd_weight", "diqt_conv3d_bwd_weight_workspace_bytes", g, x, dy)
    assert got["dw"] == got["dw_nobias"], name                       # the bias gradient does not move the weight gradient's sums
    compare(name, got)


@pytest.mark.parametrize("name", list(H_CASES))
def test_16_bit_output_bits_are_the_recorded_ones(name):
    g, flags = H_CASES[name]
    assert _lib.query("diqt_conv3d_bwd_weight_h_supported", *g, flags & 6) == 1, name
    x, dy = tensors(name, g, x16=bool(flags & 2), dy16=bool(flags & 4))
    got = run("diqt_conv3d_bwd_weight_h", "diqt_conv3d_bwd_weight_h_workspace_bytes", g, x, dy, flags)
    assert got["dw"] == got["dw_nobias"], name
    compare(name, got)


def test_the_cases_differ():
    with open(GOLDEN) as f:
        golden = json.load(f)
    digests = [v for c in golden.values() for k, v in c.items() if k != "dw_nobias"]
    assert len(set(digests)) == len(digests) == 2 * (len(CASES) + len(H_CASES))


def test_refusals_return_before_any_launch():
    """A null pointer: DIQT_E_ALIGN (-2).  A workspace one byte short: DIQT_E_WORKSPACE (-5).  A workspace at a 4-byte offset:
    DIQT_E_ALIGN (-2).  Nothing is launched and nothing written."""
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    for name in ("v3", "v1", "1x1x1 GEMM, x first", "im2col", "column sum"):
        g = CASES[name][0]
        x, dy = tensors(name, g)
        n = _lib.query("diqt_conv3d_bwd_weight_workspace_bytes", *g)
        dw = torch.full((g[5], g[4], *g[6:9]), 7., dtype=torch.float32, device=DEV)
        db = torch.full((g[5],), 7., dtype=torch.float32, device=DEV)
        ws = workspace(n + 16)
        p = lambda t: None if t is None else t.data_ptr()
        with _lib.census() as c:
            for args in ((None, dy, dw, db, ws), (x, None, dw, db, ws), (x, dy, None, db, ws), (x, dy, dw, db, None)):
                assert lib.diqt_conv3d_bwd_weight(*(p(t) for t in args), n, *g, stream) == -2, (name, args)
                assert "null pointer" in _lib.last_error()
            assert lib.diqt_conv3d_bwd_weight(p(x), p(dy), p(dw), p(db), p(ws), n - 1, *g, stream) == -5, name
            assert "workspace %d < %d" % (n - 1, n) in _lib.last_error()
            assert lib.diqt_conv3d_bwd_weight(p(x), p(dy), p(dw), p(db), p(ws) + 4, n, *g, stream) == -2, name
            assert "16-byte aligned" in _lib.last_error()
            assert lib.diqt_conv3d_bwd_weight(p(x), p(dy), p(dw), p(db), p(ws) + 4, n - 1, *g, stream) == -5, name     # short before unaligned
        assert c.count() == 0, name
        torch.cuda.synchronize()
        assert bool((dw == 7.).all()) and bool((db == 7.).all()) and bool((ws == -1).all()), name
    g, flags = H_CASES["h, flags 1"]
    x, dy = tensors("h, flags 1", g)
    n = _lib.query("diqt_conv3d_bwd_weight_h_workspace_bytes", *g)
    dw = torch.full((g[5], g[4], *g[6:9]), 7., dtype=torch.float32, device=DEV)
    ws = workspace(n + 16)
    assert lib.diqt_conv3d_bwd_weight_h(None, dy.data_ptr(), dw.data_ptr(), None, ws.data_ptr(), n, *g, flags, stream) == -2
    assert lib.diqt_conv3d_bwd_weight_h(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), None, ws.data_ptr() + 4, n, *g, flags, stream) == -2
    assert lib.diqt_conv3d_bwd_weight_h(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), None, ws.data_ptr(), n - 1, *g, flags, stream) == -5
    torch.cuda.synchronize()
    assert bool((dw == 7.).all())
