"""The extended epilogues of the 1x1x1 conv (``diqt_conv1x1_fwd_ex``): Mish + depth-to-space, column-sum statistics, the gated residual.

Every output is compared bit for bit (``torch.equal``) with the launches it replaces (the conv un-split, see ``_conv_ref``); statistics
rows are compared with float64 column
sums at the bounds the other partial-sum tests use (1e-4 on the sums relative to their scale, 2e-5 on the GroupNorm they produce).
Outputs handed to the raw entry point are NaN-prefilled and have guard rows in front and behind: every element must be written, nothing
outside may be touched."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 256            # floats in front of and behind every raw output


def _guarded(n):
    buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float32, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def _guards_untouched(buf):
    return bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all())


def _conv_inputs(B, D, H, W, Cin, Cout, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, D, H, W, Cin, generator=g).to(DEV)
    w = (torch.randn(Cout, Cin, 1, 1, 1, generator=g) * Cin ** -0.5).to(DEV)
    b = torch.randn(Cout, generator=g).to(DEV)
    return x, w, b


def _conv_ref(x, w, b):
    """Today's conv1x1_fwd_kernel launch of this conv, un-split: ``ops.conv3d`` always brings the split-K workspace, and at these small
    shapes its route then slices K over workgroups -- another summation order than the kernel whose epilogue is extended here.  Where
    the route does not split, ``ops.conv3d`` is this very launch (asserted)."""
    from diffusioniqt_amd import ops, _lib
    B, D, H, W, Cin = x.shape
    Cout = w.shape[0]
    geo = (B, D, H, W, Cin, Cout, 1, 1, 1, 0, 0, 0, 0, 0, 0)
    packed = ops._packed(w, 0)
    assert _lib.query("diqt_conv3d_fwd_route", *geo, packed.numel(), 0, 0, 0, 0, 0) == 2         # conv1x1_fwd_kernel
    y = torch.empty(B, D, H, W, Cout, device=DEV)
    _lib.call("diqt_conv3d_fwd", x, packed, b, None, y, *geo, ops._stream())
    if _lib.query("diqt_conv3d_fwd_route", *geo, packed.numel(), 1, 0, 0, 0, 1) == 1 and not (Cin == 64 and Cout >= 256):
        assert torch.equal(y, ops.conv3d(x, w, b))
    return y


def _check_sums(stats, y, rows, what):
    """[B][nblk][2][C] partial rows against float64 column sums of y[B][rows][C]"""
    B, C = y.shape[0], y.shape[-1]
    assert not torch.isnan(stats).any(), f"{what}: a statistics element was not written"
    got = stats.double().sum(1)
    flat = y.double().reshape(B, rows, C)
    for k, ref in ((0, flat.sum(1)), (1, (flat * flat).sum(1))):
        err = (got[:, k] - ref).abs().max().item()
        scale = ref.abs().max().item()
        print(f"{what}: {'sum' if k == 0 else 'sum of squares'} max err {err:.3e} of scale {scale:.3e}")
        assert err <= 1e-4 * scale, (what, k, err, scale)


def _check_groupnorm(y, groups=8):
    """the GroupNorm that consumes the rows against the one that reduces the tensor itself"""
    from diffusioniqt_amd import ops, _lib
    C = y.shape[-1]
    gamma, beta = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
    plain = y.clone()
    with torch.no_grad():
        with _lib.census() as c:
            z1 = ops.groupnorm_act(y, gamma, beta, None, groups, ops.ACT_MISH, 1e-5)
            assert c.count("groupnorm_stats_from_partials") == 1
        z0 = ops.groupnorm_act(plain, gamma, beta, None, groups, ops.ACT_MISH, 1e-5)
    err, scale = (z1 - z0).abs().max().item(), z0.abs().max().item()
    print(f"GroupNorm from the rows: max err {err:.3e} of scale {scale:.3e}")
    assert err <= 2e-5 * scale, (err, scale)


# (B, D, H, W, Cin, C', statistics): one tile per sample; two co tiles per q and two row tiles per sample; ragged row tile and ragged
# K chunk (no statistics: 105 rows per sample)
SHUFFLE_CASES = [(2, 4, 8, 4, 32, 64, True), (2, 4, 8, 8, 64, 128, True), (1, 3, 5, 7, 36, 64, False)]


@pytest.mark.parametrize("B,D,H,W,Cin,Cp,stats", SHUFFLE_CASES)
def test_conv_mish_shuffle_equals_the_three_launches(B, D, H, W, Cin, Cp, stats):
    from diffusioniqt_amd import ops, _lib
    Cout = 8 * Cp
    x, w, b = _conv_inputs(B, D, H, W, Cin, Cout, 100 + Cin)
    with torch.no_grad():
        ref = ops.depth_to_space(ops.activation(_conv_ref(x, w, b), ops.ACT_MISH))
        with _lib.census() as c:
            y = ops.conv1x1_act_shuffle(x, w, b, ops.ACT_MISH, want_stats=stats)
            assert c.count("conv1x1_fwd_ex(mish + d2s") == 1 and c.count("depth_to_space2") == 0 and c.count("act_fwd") == 0
        assert y is not None and torch.equal(y, ref)
        # the raw entry point on a NaN-prefilled output with guard rows
        assert _lib.query("diqt_conv1x1_fwd_ex_supported", B, D, H, W, Cin, Cout, ops.ACT_MISH, 1, int(stats), 0) == 1
        nblk = _lib.query("diqt_conv1x1_fwd_ex_stats_blocks", B, D, H, W, Cin, Cout, ops.ACT_MISH, 1, 0)
        assert nblk == (D * H * W // 128 * 8 if stats else 0)
        packed, bpk = ops._packed_d2s(w, b)
        ybuf, yv = _guarded(ref.numel())
        sbuf, sv = _guarded(B * nblk * 2 * Cp) if stats else (None, None)
        _lib.call("diqt_conv1x1_fwd_ex", x, packed, bpk, None, None, yv, sv, B, D, H, W, Cin, Cout, ops.ACT_MISH, 1, ops._stream())
        assert torch.equal(yv.view_as(ref), ref) and _guards_untouched(ybuf)
        if stats:
            assert _guards_untouched(sbuf)
            st = y._diqt_stats
            assert st.nblk == nblk and st.rows == 8 * D * H * W and torch.equal(st.partials.reshape(-1), sv)
            _check_sums(st.partials, ref, 8 * D * H * W, f"mish + d2s C'={Cp}")
            _check_groupnorm(y)
        else:
            assert getattr(y, "_diqt_stats", None) is None


def test_shapes_the_query_refuses_fall_back():
    """64 rows per sample with statistics, and C' = 24: the query answers 0, the ops function returns None and the caller's separate
    launches run; the raw entry point refuses the launch instead of running it."""
    from diffusioniqt_amd import ops, _lib
    from diffusioniqt_amd.imagen_pytorch3D import PixelShuffleUpsample
    M = ops.ACT_MISH
    assert _lib.query("diqt_conv1x1_fwd_ex_stats_blocks", 2, 4, 4, 4, 32, 512, M, 1, 0) == 0
    assert _lib.query("diqt_conv1x1_fwd_ex_supported", 2, 4, 4, 4, 32, 512, M, 1, 1, 0) == 0
    assert _lib.query("diqt_conv1x1_fwd_ex_supported", 2, 4, 4, 4, 32, 512, M, 1, 0, 0) == 1        # without statistics: taken
    assert _lib.query("diqt_conv1x1_fwd_ex_stats_blocks", 2, 4, 4, 4, 32, 64, 0, 0, 0) == 0
    assert _lib.query("diqt_conv1x1_fwd_ex_stats_blocks", 2, 4, 4, 4, 128, 64, 0, 0, 1) == 0
    assert _lib.query("diqt_conv1x1_fwd_ex_supported", 2, 4, 8, 4, 32, 8 * 24, M, 1, 0, 0) == 0
    x, w, b = _conv_inputs(2, 4, 4, 4, 32, 64, 5)
    with torch.no_grad():
        assert ops.conv1x1_stats(x, w, b) is None
        # 64 rows per sample, statistics wanted: the launch without them runs, and says so
        x5, w5, b5 = _conv_inputs(2, 4, 4, 4, 32, 512, 6)
        y = ops.conv1x1_act_shuffle(x5, w5, b5, M, want_stats=True)
        assert y is not None and getattr(y, "_diqt_stats", None) is None
        assert torch.equal(y, ops.depth_to_space(ops.activation(_conv_ref(x5, w5, b5), M)))
        # C' = 24: the up-sampler module keeps its three launches
        up = PixelShuffleUpsample(32, 24).to(DEV)
        xu = torch.randn(2, 4, 8, 4, 32, device=DEV)
        assert ops.conv1x1_act_shuffle(xu, up.net[0].weight, up.net[0].bias, M) is None
        with _lib.census() as c:
            yu = up(xu)
            assert c.count("conv1x1_fwd_ex") == 0 and c.count("depth_to_space2") == 1 and c.count("act_fwd") == 1
        assert yu.shape == (2, 8, 16, 8, 24)
        ybuf, yv = _guarded(2 * 64 * 64)
        sbuf, sv = _guarded(2 * 2 * 64)
        with pytest.raises(Exception):
            _lib.call("diqt_conv1x1_fwd_ex", x, ops._packed(w, 0), b, None, None, yv, sv, 2, 4, 4, 4, 32, 64, 0, 0, ops._stream())
        assert torch.isnan(ybuf).all() and torch.isnan(sbuf).all()


@pytest.mark.parametrize("B,D,H,W,Cin,Cout", [(2, 4, 8, 4, 512, 64), (2, 4, 8, 8, 36, 40)])
def test_conv_with_statistics_rows(B, D, H, W, Cin, Cout):
    """the plain 1x1 conv with the statistics epilogue (the form a down-sampling projection would take); the second case has a ragged
    K chunk and a ragged 64-channel tile"""
    from diffusioniqt_amd import ops, _lib
    x, w, b = _conv_inputs(B, D, H, W, Cin, Cout, 300 + Cin)
    with torch.no_grad():
        ref = _conv_ref(x, w, b)
        y = ops.conv1x1_stats(x, w, b)
        assert y is not None and torch.equal(y, ref)
        nblk = D * H * W // 128
        assert y._diqt_stats.nblk == nblk == _lib.query("diqt_conv1x1_fwd_ex_stats_blocks", B, D, H, W, Cin, Cout, 0, 0, 0)
        ybuf, yv = _guarded(ref.numel())
        sbuf, sv = _guarded(B * nblk * 2 * Cout)
        _lib.call("diqt_conv1x1_fwd_ex", x, ops._packed(w, 0), b, None, None, yv, sv, B, D, H, W, Cin, Cout, 0, 0, ops._stream())
        assert torch.equal(yv.view_as(ref), ref) and _guards_untouched(ybuf) and _guards_untouched(sbuf)
        assert torch.equal(sv, y._diqt_stats.partials.reshape(-1))
        _check_sums(y._diqt_stats.partials, ref, D * H * W, f"conv + stats {Cin}->{Cout}")
        _check_groupnorm(y)


@pytest.mark.parametrize("B,D,H,W,Cin,Cout", [(2, 4, 8, 4, 128, 64), (2, 4, 4, 8, 512, 256)])
def test_gated_residual_equals_res_conv_plus_se_gate_residual(B, D, H, W, Cin, Cout):
    from diffusioniqt_amd import ops, _lib
    x, w, b = _conv_inputs(B, D, H, W, Cin, Cout, 200 + Cin)
    g = torch.Generator().manual_seed(7 * Cout)
    # h as the block's second conv leaves it: a 3x3x3 conv output that carries its column sums
    hin = torch.randn(B, D, H, W, Cout, generator=g).to(DEV)
    w3 = (torch.randn(Cout, Cout, 3, 3, 3, generator=g) * (27 * Cout) ** -0.5).to(DEV)
    w1 = (torch.randn(Cout // 16, Cout, generator=g) * Cout ** -0.5).to(DEV)
    w2 = (torch.randn(Cout, Cout // 16, generator=g) * 0.5).to(DEV)
    with torch.no_grad():
        h = ops.conv3d(hin, w3, None, (1, 1, 1), want_stats=True)
        pre = getattr(h, "_diqt_stats", None)
        if pre is None:                  # a split-K launch grants no rows: hand the tail the sums a statistics conv would have written
            ident = torch.eye(Cout, device=DEV).reshape(Cout, Cout, 1, 1, 1).contiguous()
            hs = ops.conv1x1_stats(h, ident, None)
            assert hs is not None and torch.equal(hs, h)
            h._diqt_stats = pre = hs._diqt_stats
        ref = ops.se_gate_residual(h, w1, w2, _conv_ref(x, w, b))
        with _lib.census() as c:
            y = ops.se_conv1x1_residual(h, w1, w2, x, w, b)
            assert c.count("conv1x1_fwd_ex(gated residual") == 1 and c.count("se_pool_mlp_fwd") == 1
            assert c.count("gate_residual_fwd") == 0 and c.count("conv3d_fwd") == 0
        assert y is not None and torch.equal(y, ref)
        rows = D * H * W
        nblk = _lib.query("diqt_conv1x1_fwd_ex_stats_blocks", B, D, H, W, Cin, Cout, 0, 0, 1)
        assert nblk == rows // 128 == y._diqt_stats.nblk
        # raw launch, NaN-prefilled with guard rows, with the gate the two-launch form computes
        pooled, hidden, gate = torch.empty(B, Cout, device=DEV), torch.empty(B, Cout // 16, device=DEV), torch.empty(B, Cout, device=DEV)
        _lib.call("diqt_se_pool_mlp_fwd", pre.partials, pre.nblk, rows, pooled, w1, w2, hidden, gate, B, Cout, Cout // 16, ops._stream())
        ybuf, yv = _guarded(ref.numel())
        sbuf, sv = _guarded(B * nblk * 2 * Cout)
        _lib.call("diqt_conv1x1_fwd_ex", x, ops._packed(w, 0), b, h, gate, yv, sv, B, D, H, W, Cin, Cout, 0, 0, ops._stream())
        assert torch.equal(yv.view_as(ref), ref) and _guards_untouched(ybuf) and _guards_untouched(sbuf)
        assert torch.equal(sv, y._diqt_stats.partials.reshape(-1))
        _check_sums(y._diqt_stats.partials, ref, rows, f"gated residual {Cin}->{Cout}")
        _check_groupnorm(y)
