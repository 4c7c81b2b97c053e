"""Autograd operators of the hot path, each a thin ``torch.autograd.Function`` over libdiqt_hip.so.

PyTorch supplies device memory, streams and the autograd tape; all arithmetic runs in the HIP kernels
of ``csrc/``.  Activations are fp32 channels-last: ``x[B, D, H, W, C]`` (or ``[rows, C]``).
There is no CPU fallback: a non-CUDA tensor raises.
"""
import contextlib
import os

import torch
from torch.autograd import Function

from . import _lib

ACT_NONE, ACT_MISH, ACT_SILU, ACT_GELU, ACT_RELU, ACT_SIGMOID = range(6)

_WEIGHT_EPOCH = 0     # bumped by the fused optimiser (it writes parameters through raw pointers)


def bump_weight_epoch():
    global _WEIGHT_EPOCH
    _WEIGHT_EPOCH += 1
    if _LIVE_GRAPHS > 0:          # every captured graph froze the old weights' packed copies: stale from here on (graphs.drop_all)
        from . import graphs
        graphs.drop_all()


# A captured hipGraph (graphs.py) holds raw device addresses of everything its launches read: besides the tensors of its private pool
# also what the host side had cached BEFORE the capture (packed weights, position-bias tables, the scratch arena).  When such a cache
# replaces its tensor while a graph is alive the old one is parked here instead of being freed, until the last graph is gone.
_GRAPH_PINS = []
_LIVE_GRAPHS = 0


_CAPTURE_CLOCK = 0      # number of graph captures begun so far


def capture_begins():
    """graphs.py, right before a capture: tensors the host caches created up to here may be addressed by the new graph."""
    global _CAPTURE_CLOCK
    _CAPTURE_CLOCK += 1


def born(t):
    """Stamps a tensor a host-side cache is about to keep with the capture clock (see ``retire``)."""
    if t is not None:
        t._diqt_born = _CAPTURE_CLOCK
    return t


def retire(*tensors):
    """A host-side cache is dropping these device tensors: keep them alive while any captured graph may still address them.  A tensor
    created after the newest capture began (``born``) is addressed by no graph -- or lives in that graph's own pool -- and is not pinned:
    with a captured TRAINING step alive for the whole run, every validation / sampling pass in between re-packs the weights, and those
    copies must not pile up."""
    if _LIVE_GRAPHS > 0:
        _GRAPH_PINS.extend(t for t in tensors if t is not None and getattr(t, "_diqt_born", -1) < _CAPTURE_CLOCK)


def graphs_alive(delta):
    """graphs.py: ``delta`` graphs were captured (+) or dropped (-)."""
    global _LIVE_GRAPHS
    _LIVE_GRAPHS = max(_LIVE_GRAPHS + delta, 0)
    if _LIVE_GRAPHS == 0:
        _GRAPH_PINS.clear()


def set_gnbwd_fuse(on: bool) -> bool:
    """Switches the GroupNorm-backward reduction between its own pass (False, the default) and the epilogue of the conv's
    backward-data launch (True; ``diqt_conv3d_fwd_gnbwd``).  Returns the previous setting.  Both are product paths and the parity
    suite runs whole-network gradients in each."""
    return bool(_lib.query("diqt_set_gnbwd_fuse", int(bool(on))))


@contextlib.contextmanager
def gnbwd_fuse(on: bool):
    prev = set_gnbwd_fuse(on)
    try:
        yield
    finally:
        set_gnbwd_fuse(prev)


# --------------------------------------------------------------------------------------------
# mixed precision: the reference's fp16 switch is torch.autocast (ImagenTrainer(fp16=True) -> Accelerator(mixed_precision='fp16'),
# trainer.py:293-311; `torch.autocast` around ElucidatedImagen.sample).  Under autocast -- or inside
# ``low_precision('fp16' | 'bf16')`` -- conv3d / linear FORWARDS run on the fp16 / bf16 MFMA kernel (fp32 accumulate, result
# rounded once to the operand type like an fp16 output tensor); everything autocast keeps in fp32 (GroupNorm, soft-max, losses,
# the sampler arithmetic) is untouched, and so are attention products and backward passes (fp32 here: more precise than the
# reference, never less).  Activations stay fp32 in HBM; the cast happens inside the kernel while the halo tile is staged.
# --------------------------------------------------------------------------------------------
_LP_FORCED = None      # None: follow torch.autocast; 'off' | 'fp16' | 'bf16'


class low_precision:
    """Context manager forcing the conv/linear compute type: 'fp16', 'bf16' or 'off' (fp32 even under torch.autocast)."""

    def __init__(self, mode):
        assert mode in ('off', 'fp16', 'bf16'), mode
        self.mode = mode

    def __enter__(self):
        global _LP_FORCED
        self.prev, _LP_FORCED = _LP_FORCED, self.mode
        return self

    def __exit__(self, *exc):
        global _LP_FORCED
        _LP_FORCED = self.prev
        return False


def lp_mode():
    """None (fp32), 0 (fp16 operands) or 1 (bf16 operands) for the conv/linear forward launched now."""
    if _LP_FORCED is not None:
        return {'off': None, 'fp16': 0, 'bf16': 1}[_LP_FORCED]
    if torch.is_autocast_enabled('cuda'):
        dt = torch.get_autocast_dtype('cuda')
        return 0 if dt == torch.float16 else (1 if dt == torch.bfloat16 else None)
    return None


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _chk(*ts):
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError("diffusioniqt_amd ops run only on MI355X (HIP) tensors; got a CPU tensor. "
                               "There is no CPU fallback — use oracle/ for CPU checks.")
        if t.dtype != torch.float32:
            raise RuntimeError(f"diffusioniqt_amd ops are fp32; got {t.dtype}")
        if not t.is_contiguous():
            raise RuntimeError("diffusioniqt_amd ops need contiguous tensors")


class KernelTimer:
    """Optional HIP-event timing of the dominant kernel (conv3d fwd/bwd-data launches) for bench.py's roofline:
    events are recorded on the stream the kernel is launched on (torch's current stream)."""
    def __init__(self):
        self.records = []      # (start_event, end_event, flops, tag, shape)
        self.enabled = False

    def reset(self):
        self.records = []

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for s, e, flops, tag, _ in self.records:
            ms, fl, n = out.get(tag, (0.0, 0.0, 0))
            out[tag] = (ms + s.elapsed_time(e), fl + flops, n + 1)
        return out

    def by_shape(self):
        """{(tag, shape): (ms, flops, launches)} -- tools/shape_profile.py"""
        torch.cuda.synchronize()
        out = {}
        for s, e, flops, tag, shape in self.records:
            ms, fl, n = out.get((tag, shape), (0.0, 0.0, 0))
            out[(tag, shape)] = (ms + s.elapsed_time(e), fl + flops, n + 1)
        return out


TIMER = KernelTimer()

_WS = {}


def _workspace(nbytes, device):
    """Grow-only scratch arena per device; kernels using it are ordered by the stream."""
    key = device.index
    ws = _WS.get(key)
    if ws is None or ws.numel() < nbytes:
        retire(ws)                                        # a captured graph may hold the old arena's address
        ws = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
        _WS[key] = ws
    return ws


def _reduce_ws(B, C, device):
    n = _lib.query("diqt_reduce_workspace_bytes", B, C)
    return _workspace(n, device), n


# --------------------------------------------------------------------------------------------
# convolution / linear
# --------------------------------------------------------------------------------------------
def _packed_len(shape, mode):
    """(direct, Winograd) floats of ``_packed(weight, mode)``: forward packs of 3x3x3 filters carry the Winograd panels of
    conv_fwd9_kernel's F(2,3) tile behind the direct ones (pack mode 2), which the ``*_pk`` entry points see from the length."""
    Cout, Cin, kd, kh, kw = shape
    eff = (Cout, Cin) if mode == 0 else (Cin, Cout)
    n = _lib.query("diqt_conv_packed_elems", eff[0], eff[1], kd, kh, kw)
    return n, (_lib.query("diqt_conv_packed_wino_elems", Cout, Cin, kd, kh, kw) if mode == 0 else 0)


def _packed(weight5, mode):
    """Packed copy of an OIDHW weight for the MFMA kernel, cached on the tensor until it changes."""
    owner = weight5._base if weight5._base is not None else weight5   # views (nn.Linear) share the cache
    cache = getattr(owner, "_diqt_pack", None)
    if cache is None:
        cache = {}
        try:
            owner._diqt_pack = cache
        except Exception:
            pass
    key = (mode, weight5.data_ptr(), weight5._version, _WEIGHT_EPOCH)
    hit = cache.get(mode)
    if hit is not None and hit[0] == key:
        return hit[1]
    Cout, Cin, kd, kh, kw = weight5.shape
    n, nw = _packed_len(weight5.shape, mode)
    packed = torch.empty(n + nw, dtype=torch.float32, device=weight5.device)
    _lib.call("diqt_conv_pack_weight", weight5.detach(), packed, Cout, Cin, kd, kh, kw, 2 if nw else mode, _stream())
    if hit is not None:
        retire(hit[1])
    cache[mode] = (key, born(packed))
    return packed


def _packed_h(weight5, bf16, mode=0):
    """16-bit packed copy of an OIDHW weight for the fp16 / bf16 MFMA kernel, cached like ``_packed`` (mode 1: backward-data)."""
    owner = weight5._base if weight5._base is not None else weight5
    cache = getattr(owner, "_diqt_pack", None)
    if cache is None:
        cache = {}
        try:
            owner._diqt_pack = cache
        except Exception:
            pass
    slot = ('h', bf16, mode)
    key = (slot, weight5.data_ptr(), weight5._version, _WEIGHT_EPOCH)
    hit = cache.get(slot)
    if hit is not None and hit[0] == key:
        return hit[1]
    Cout, Cin, kd, kh, kw = weight5.shape
    eff = (Cout, Cin) if mode == 0 else (Cin, Cout)
    n = _lib.query("diqt_conv_packed_h_elems", eff[0], eff[1], kd, kh, kw)
    packed = torch.empty(n, dtype=torch.int16, device=weight5.device)
    _lib.call("diqt_conv_pack_weight_h", weight5.detach(), packed, Cout, Cin, kd, kh, kw, mode, bf16, _stream())
    if hit is not None:
        retire(hit[1])
    cache[slot] = (key, born(packed), weight5.detach())   # (a graph-free alias of) the weight: repack_cached_h re-derives the copy from it
    return packed


SPLIT16 = True        # False: ``split16=True`` requests are ignored (A/B timing and tests; the launches then take the default route)


def _packed_split16(weight5):
    """Head / scaled-tail fp16 pack of an OIDHW weight for the three-product split route (``diqt_conv_pack_weight_split16``), cached
    like ``_packed``.  None: the layer is refused -- a weight with |w| >= 65504, decided once per weight version at pack time and cached
    with the pack -- or a pack would have to be made (and its verdict read back) during a graph capture."""
    owner = weight5._base if weight5._base is not None else weight5
    cache = getattr(owner, "_diqt_pack", None)
    if cache is None:
        cache = {}
        try:
            owner._diqt_pack = cache
        except Exception:
            pass
    slot = 's16'
    key = (slot, weight5.data_ptr(), weight5._version, _WEIGHT_EPOCH)
    hit = cache.get(slot)
    if hit is not None and hit[0] == key:
        return hit[1]
    if torch.cuda.is_current_stream_capturing():
        return None
    Cout, Cin, kd, kh, kw = weight5.shape
    n = _lib.query("diqt_conv_packed_split16_elems", Cout, Cin, kd, kh, kw)
    packed = torch.empty(n, dtype=torch.int16, device=weight5.device)
    refused = torch.empty(1, dtype=torch.int32, device=weight5.device)
    _lib.call("diqt_conv_pack_weight_split16", weight5.detach(), packed, refused, Cout, Cin, kd, kh, kw, _stream())
    if hit is not None:
        retire(hit[1])
    packed = None if int(refused.item()) else born(packed)
    cache[slot] = (key, packed)
    return packed


def _split16_plan(geo, act, split16):
    """Which plan of the split route takes the launch: "" (the 256-voxel tiles, ``split16=True``), "_fill" (``split16="fill"``: the fill
    plan is asked first -- smaller tiles where the 256-voxel ones leave CUs idle -- then the other), "_pair" (``split16="pair"``: the
    pair plan is asked first -- the tap-paired 16x16x32 body where the 256-voxel tile fills the chip -- then what "fill" answers),
    None: none of them, or switched off.  The value is the suffix of the entry points' names."""
    if not split16 or not SPLIT16:
        return None
    if split16 == "pair" and _lib.query("diqt_conv3d_fwd_gn_split16_pair_supported", *geo, act):
        return "_pair"
    if split16 in ("fill", "pair") and _lib.query("diqt_conv3d_fwd_gn_split16_fill_supported", *geo, act):
        return "_fill"
    return "" if _lib.query("diqt_conv3d_fwd_gn_split16_supported", *geo, act) else None


def _conv_fwd_split16(x5, weight, bias, residual, pad, epad, want_stats, coef=None, act=0, split16=True):
    """fp32 3x3x3 forward on the fp16 matrix pipe by the three-product split (conv_split16.hip): the pass that splits x (with
    ``coef``: and applies act(A x + Bc), the GroupNorm-apply of ``gn_conv3d``), then ``conv_f9h_kernel``'s split build.  None when the
    request is switched off (``SPLIT16``), the shape is not granted or the weight is refused; y carries ``_diqt_stats`` when asked.
    ``split16``: True, "fill" or "pair" (``_split16_plan``)."""
    B, D, H, W, Cin = x5.shape
    Cout, _, kd, kh, kw = weight.shape
    geo = (B, D, H, W, Cin, Cout, kd, kh, kw, *pad, *epad)
    plan = _split16_plan(geo, act, split16)
    if plan is None:
        return None
    packed = _packed_split16(weight)
    if packed is None:
        return None
    Do, Ho, Wo = D + 2 * pad[0] + epad[0] - kd + 1, H + 2 * pad[1] + epad[1] - kh + 1, W + 2 * pad[2] + epad[2] - kw + 1
    y = torch.empty((B, Do, Ho, Wo, Cout), dtype=torch.float32, device=x5.device)
    x16 = torch.empty((B, D, H, W, 2 * Cin), dtype=torch.float16, device=x5.device)
    if TIMER.enabled:
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
    stats = None
    if want_stats:
        nblk = _lib.query(f"diqt_conv3d_fwd_split16{plan}_stats_blocks", *geo)
        stats = torch.empty((B, nblk, 2, Cout), dtype=torch.float32, device=x5.device)
        y._diqt_stats = ColStats(stats, nblk, Do * Ho * Wo)
    if coef is None:
        _lib.call(f"diqt_conv3d_fwd_split16{plan}", x5, x16, packed, bias, residual, y, stats, *geo, _stream())
    else:
        _lib.call(f"diqt_conv3d_fwd_gn_split16{plan}", x5, x16, packed, bias, residual, y, stats, coef, act, *geo, _stream())
    if TIMER.enabled:
        e.record()
        TIMER.records.append((s, e, 2.0 * B * Do * Ho * Wo * Cout * Cin * kd * kh * kw, "conv_f9h_kernel_split16", geo[:9]))
    return y


def repack_cached_h(module, bf16):
    """Re-derives every cached 16-bit packed copy (``_packed_h``) of ``module``'s weights for operand type ``bf16`` in ONE launch per 64
    weights (``diqt_conv_pack_weight_h_multi``) into fresh tensors keyed on the current weight epoch.  graphs.TrainStepGraphs calls it as the
    first thing inside the capture of a training micro-step: a replay then refreshes all packed weights with one or two launches instead
    of one per conv and direction (86 for the C2 U-Net).  Returns the number of copies re-derived."""
    rows = []
    for p in module.parameters():
        cache = getattr(p, "_diqt_pack", None)
        if not cache or not p.is_cuda:
            continue
        for slot, ent in list(cache.items()):
            if not (isinstance(slot, tuple) and slot[0] == 'h' and slot[1] == bf16 and len(ent) == 3):
                continue
            w5 = ent[2]
            if w5.data_ptr() != ent[0][1] or not w5.is_contiguous() or w5.dtype != torch.float32:
                continue                                  # the parameter moved: the lazy path repacks it
            mode = slot[2]
            packed = torch.empty(ent[1].numel(), dtype=torch.int16, device=w5.device)
            Cout, Cin, kd, kh, kw = w5.shape
            rows.append((w5.data_ptr(), packed.data_ptr(), Cout, Cin, kd, kh, kw, mode))
            retire(ent[1])
            cache[slot] = ((slot, w5.data_ptr(), w5._version, _WEIGHT_EPOCH), born(packed), w5)
    if rows:
        _lib.call("diqt_conv_pack_weight_h_multi", torch.tensor(rows, dtype=torch.int64), len(rows), int(bf16), _stream())
    return len(rows)


def _conv_fwd_half(x5, weight, bias, residual, pad, epad, bf16, mode=0, x_half=False, y_half=False, stats_out=None):
    """fp16 / bf16-operand forward (mode 0) or backward-data (mode 1: x5 is dY, pad / epad already transformed) through
    diqt_conv3d_fwd_h, or None when the low-precision kernel does not take this shape.  x_half / y_half: the tensor at that end holds
    16-bit values of the operand type (diqt_conv3d_fwd_h_io; the caller has asked conv_half_io16_ok)."""
    B, D, H, W, Cin = x5.shape
    kd, kh, kw = weight.shape[2:]
    Cout = weight.shape[0] if mode == 0 else weight.shape[1]
    geo = (B, D, H, W, Cin, Cout, kd, kh, kw, *pad, *epad)
    hdt = torch.bfloat16 if bf16 else torch.float16
    ex, ey = (2 if x_half else 4), (2 if y_half else 4)
    Bc = B                      # batch entries per launch: the kernel addresses a tensor through one buffer descriptor (< 1 GiB of fp32)
    io16 = x_half or y_half
    while not io16 and not _lib.query("diqt_conv3d_fwd_h_supported", Bc, *geo[1:]):
        if Bc % 2 or max(x5[:Bc].numel(), Bc * D * H * W * Cout) * 4 < (1 << 30):
            return None
        Bc //= 2
    assert not io16 or (Bc == B and x5.dtype == (hdt if x_half else torch.float32))
    Do, Ho, Wo = D + 2 * pad[0] + epad[0] - kd + 1, H + 2 * pad[1] + epad[1] - kh + 1, W + 2 * pad[2] + epad[2] - kw + 1
    y = torch.empty((B, Do, Ho, Wo, Cout), dtype=hdt if y_half else torch.float32, device=x5.device)
    if TIMER.enabled:
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
    packed = _packed_h(weight, bf16, mode)
    if io16:
        stats = None
        if stats_out is not None:
            nblk = _lib.query("diqt_conv3d_fwd_h_stats_blocks", *geo, int(x_half), int(y_half))
            if nblk > 0:                     # per-(tile, wave) column sums of y for the consumer's GroupNorm
                stats = torch.empty((B, nblk, 2, Cout), dtype=torch.float32, device=x5.device)
                stats_out.append(ColStats(stats, nblk, Do * Ho * Wo))
        _lib.call("diqt_conv3d_fwd_h_io", x5, packed, bias, residual, y, *geo, bf16, 1, int(x_half), int(y_half), stats, _stream())
    else:
        for b0 in range(0, B, Bc):
            _lib.call("diqt_conv3d_fwd_h", x5[b0:b0 + Bc], packed, bias, residual[b0:b0 + Bc] if residual is not None else None,
                      y[b0:b0 + Bc], Bc, *geo[1:], bf16, 1, _stream())
    if TIMER.enabled:
        e.record()
        # rocprofv3's name of the kernel that ran: launches of >= 2 x 256 units take the persistent form
        last = _lib.last_launch()
        tag = ("conv_f9h_kernel" if "v9h" in last else "conv_pw_h_kernel" if "gemm" in last
               else "conv_fwd_hp_kernel" if "persistent" in last else "conv_fwd_h_kernel")
        TIMER.records.append((s, e, 2.0 * B * Do * Ho * Wo * Cout * Cin * kd * kh * kw, tag, (B, D, H, W, Cin, Cout, kd, kh, kw)))
    return y


def _groupnorm_act_h(x, gamma, beta, ss, groups, act, eps, lp):
    """act(GN(x) * (scale + 1) + shift) stored in the operand type of the 16-bit conv that consumes it (sampling path under autocast).
    x: fp32, or the 16-bit output of a conv of this path (conv_pair_nograd_h(out_half=True): it carries its GroupNorm statistics)."""
    B, C = x.shape[0], x.shape[-1]
    rows = x.numel() // (B * C)
    mean = torch.empty(B * groups, dtype=torch.float32, device=x.device)
    rstd = torch.empty_like(mean)
    s = _stream()
    pre = getattr(x, "_diqt_stats", None)
    x_half = x.dtype != torch.float32
    if pre is not None and pre.rows == rows and pre.partials.shape == (B, pre.nblk, 2, C):
        _lib.call("diqt_groupnorm_stats_from_partials", pre.partials, mean, rstd, B, pre.nblk, rows, C, groups, float(eps), s)
    elif x_half:
        raise RuntimeError("a 16-bit block output must carry the GroupNorm statistics of the conv that wrote it")
    else:
        ws, n = _reduce_ws(B, C, x.device)
        _lib.call("diqt_groupnorm_stats", x, mean, rstd, ws, n, B, rows, C, groups, float(eps), s)
    scale = shift = None
    cs = 0
    if isinstance(ss, SSView):
        assert ss.width == 2 * C and ss.base.shape[0] == B
        scale, cs = ss.base.data_ptr() + 4 * ss.off, ss.base.shape[1]
        shift = scale + 4 * C
    elif ss is not None:
        assert ss.shape == (B, 2 * C) and ss.stride(1) == 1 and ss.is_cuda and ss.dtype == torch.float32
        scale, shift, cs = ss.data_ptr(), ss.data_ptr() + 4 * C, ss.stride(0)
    y = torch.empty(x.shape, dtype=torch.bfloat16 if lp == 1 else torch.float16, device=x.device)
    _lib.call("diqt_gn_act_fwd_h", x, mean, rstd, gamma, beta, scale, shift, cs, y, B, rows, C, groups, act, lp, int(x_half), s)
    return y


def gn_conv3d_h(x, gamma, beta, scale_shift, groups, act, eps, weight, bias, padding, residual=None, want_stats=False, out_half=False):
    """Sampling path under autocast: ``conv3d(act(GN(x) * (scale + 1) + shift))`` with the GroupNorm-apply pass writing the conv's input in
    the operand type and the conv on the LDS-DMA 16-bit kernel (``conv_f9h_kernel``: the 3x3x3 Blocks of Family A, imagen_pytorch3D.py:535-566).
    x: fp32, or the 16-bit output of such a conv (``out_half``: it carries its GroupNorm statistics).  ``out_half``: y only feeds the next
    Block's GroupNorm (ResnetBlock: block1 -> block2) -- stored in the operand type, the values autocast's conv output tensor holds anyway.
    None when not under autocast or the shape is not taken by a 16-bit-input kernel."""
    lp = lp_mode()
    if lp is None or torch.is_grad_enabled() or x.dim() != 5:
        return None
    B, D, H, W, C = x.shape
    Cout, Cin, kd, kh, kw = weight.shape
    padding = tuple(int(p) for p in ((padding,) * 3 if isinstance(padding, int) else padding))
    x_is_half = x.dtype != torch.float32
    yh = bool(out_half and want_stats and residual is None)
    geo = (B, D, H, W, C, Cout, kd, kh, kw, *padding, 0, 0, 0)
    ok = Cin == C and C % groups == 0 and C % 4 == 0 and _lib.query("diqt_conv3d_fwd_h_io16_supported", *geo, 1, int(yh))
    if ok and yh:
        ok = _lib.query("diqt_conv3d_fwd_h_stats_blocks", *geo, 1, 1) > 0
    if not ok:
        if x_is_half:
            raise RuntimeError("gn_conv3d_h: a 16-bit block output reached a conv that does not take 16-bit input")
        return None
    _chk(None if x_is_half else x, gamma, beta, weight, bias, residual, scale_shift.base if isinstance(scale_shift, SSView) else None)
    xin = _groupnorm_act_h(x, gamma, beta, scale_shift, groups, act, eps, lp)
    holder = [] if want_stats else None
    y = _conv_fwd_half(xin, weight, bias, residual, padding, (0, 0, 0), lp, x_half=True, y_half=yh, stats_out=holder)
    if holder:
        y._diqt_stats = holder[0]
    assert not yh or holder
    return y


def conv_half_out_ok(shape5, weight, padding):
    """May a Block hand its conv output on in the operand type?  (the NEXT Block's conv has to take a 16-bit input of that shape)"""
    if lp_mode() is None or torch.is_grad_enabled():
        return False
    B, D, H, W, C = shape5
    Cout, Cin, kd, kh, kw = weight.shape
    padding = tuple(int(p) for p in ((padding,) * 3 if isinstance(padding, int) else padding))
    return bool(Cin == C and _lib.query("diqt_conv3d_fwd_h_io16_supported", B, D, H, W, C, Cout, kd, kh, kw, *padding, 0, 0, 0, 1, 0))


def conv_pair_nograd_h(x, w1, b1, pad1, w2, b2, pad2, epad2, residual=None, gn=None, want_stats=False, out_half=False):
    """Two convs in a row on the sampling path under autocast -- the per-frame and the temporal conv of a pseudo-3D block -- with
    the tensor between them in the operand type (it holds exactly the values the fp32 tensor would: the first conv's result is rounded
    to that type either way).  ``gn`` = (gamma, beta, scale_shift, groups, act, eps): x is the raw input of the block's GroupNorm, whose
    apply pass then writes the first conv's input in the operand type as well.  None when not under autocast or a shape is not taken
    by the persistent 16-bit kernel."""
    lp = lp_mode()
    if lp is None or torch.is_grad_enabled():
        return None
    x_is_half = x.dtype != torch.float32                  # the 16-bit output of the previous block's pair (out_half)
    assert not x_is_half or gn is not None
    _chk(None if x_is_half else x, w1, b1, w2, b2, residual)
    B, D, H, W, Cin = x.shape
    Cm, C2 = w1.shape[0], w2.shape[0]
    k1, k2 = tuple(w1.shape[2:]), tuple(w2.shape[2:])
    D1, H1, W1 = D + 2 * pad1[0] - k1[0] + 1, H + 2 * pad1[1] - k1[1] + 1, W + 2 * pad1[2] - k1[2] + 1
    xh = gn is not None
    if xh and (Cin % 4 != 0 or Cin % gn[3] != 0):
        return None
    if not (_lib.query("diqt_conv3d_fwd_h_io16_supported", B, D, H, W, Cin, Cm, *k1, *pad1, 0, 0, 0, int(xh), 1)
            and _lib.query("diqt_conv3d_fwd_h_io16_supported", B, D1, H1, W1, Cm, C2, *k2, *pad2, *epad2, 1, 0)):
        return None
    xin = x
    if xh:
        gamma, beta, ss, groups, act, eps = gn
        _chk(gamma, beta, ss.base if isinstance(ss, SSView) else None)
        xin = _groupnorm_act_h(x, gamma, beta, ss, groups, act, eps, lp)
    mid = _conv_fwd_half(xin, w1, b1, None, pad1, (0, 0, 0), lp, x_half=xh, y_half=True)
    # out_half: the pair's output only feeds the next block's GroupNorm (ResnetBlock: block1 -> block2) -- it is stored in the operand type
    # too (no residual, so it holds fp16-exact values) PROVIDED the statistics that GroupNorm needs come along
    out_half = bool(out_half and want_stats and residual is None
                    and _lib.query("diqt_conv3d_fwd_h_io16_supported", B, D1, H1, W1, Cm, C2, *k2, *pad2, *epad2, 1, 1)
                    and _lib.query("diqt_conv3d_fwd_h_stats_blocks", B, D1, H1, W1, Cm, C2, *k2, *pad2, *epad2, 1, 1) > 0)
    holder = [] if want_stats else None
    y = _conv_fwd_half(mid, w2, b2, residual, pad2, epad2, lp, x_half=True, y_half=out_half, stats_out=holder)
    if holder:
        y._diqt_stats = holder[0]           # consumed by the next GroupNorm on this exact tensor
    assert not out_half or holder
    return y


def _conv_fwd_smallcout(x5, weight, bias, residual, pad, epad):
    """Forward of a conv with one or two output channels through diqt_conv3d_fwd_smallcout (exact fp32), or None."""
    B, D, H, W, Cin = x5.shape
    Cout, _, kd, kh, kw = weight.shape
    geo = (B, D, H, W, Cin, Cout, kd, kh, kw, *pad, *epad)
    if not _lib.query("diqt_conv3d_fwd_smallcout_supported", *geo):
        return None
    Do, Ho, Wo = D + 2 * pad[0] + epad[0] - kd + 1, H + 2 * pad[1] + epad[1] - kh + 1, W + 2 * pad[2] + epad[2] - kw + 1
    y = torch.empty((B, Do, Ho, Wo, Cout), dtype=torch.float32, device=x5.device)
    if TIMER.enabled:
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
    _lib.call("diqt_conv3d_fwd_smallcout", x5, weight.detach().contiguous(), bias, residual, y, *geo, _stream())
    if TIMER.enabled:
        e.record()
        TIMER.records.append((s, e, 2.0 * B * Do * Ho * Wo * Cout * Cin * kd * kh * kw, "conv_smallcout_kernel",
                              (B, D, H, W, Cin, Cout, kd, kh, kw)))
    return y


class ColStats:
    """Per-tile column sums (sum, sum of squares) of a conv output, written by the conv epilogue: [B, nblk, 2, C].
    Attached to the output tensor as ``_diqt_stats`` for the consumer's GroupNorm statistics / SE pooling."""
    __slots__ = ("partials", "nblk", "rows")

    def __init__(self, partials, nblk, rows):
        self.partials, self.nblk, self.rows = partials, nblk, rows


def _conv_fwd_raw(x5, packed, bias, residual, Cout, k, pad, epad=(0, 0, 0), stats_out=None):
    B, D, H, W, Cin = x5.shape
    kd, kh, kw = k
    pd, ph, pw = pad
    epd, eph, epw = epad
    Do, Ho, Wo = D + 2 * pd + epd - kd + 1, H + 2 * ph + eph - kh + 1, W + 2 * pw + epw - kw + 1
    y = torch.empty((B, Do, Ho, Wo, Cout), dtype=torch.float32, device=x5.device)
    if TIMER.enabled:
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
    npk = packed.numel()
    n = _lib.query("diqt_conv3d_fwd_workspace_bytes_pk", B, D, H, W, Cin, Cout, kd, kh, kw, pd, ph, pw, epd, eph, epw, npk)
    ws = _workspace(n, x5.device) if n else None
    stats = None
    if stats_out is not None:
        nblk = _lib.query("diqt_conv3d_fwd_stats_blocks_pk", B, D, H, W, Cin, Cout, kd, kh, kw, pd, ph, pw, epd, eph, epw, npk)
        if nblk > 0:
            stats = torch.empty((B, nblk, 2, Cout), dtype=torch.float32, device=x5.device)
            stats_out.append(ColStats(stats, nblk, Do * Ho * Wo))
    _lib.call("diqt_conv3d_fwd_pk", x5, packed, npk, bias, residual, y, stats, ws, n, B, D, H, W, Cin, Cout, kd, kh, kw, pd, ph, pw,
              epd, eph, epw, _stream())
    if TIMER.enabled:
        e.record()
        # the tag names the kernel the C side dispatched to (the launch's own decision for what it was given), so that bench.py's
        # per-kernel numbers line up with rocprofv3's; a split-K launch's interval includes the slab sum
        taps = kd * kh * kw
        kid = _lib.query("diqt_conv3d_fwd_route", B, D, H, W, Cin, Cout, kd, kh, kw, pd, ph, pw, epd, eph, epw, npk, int(ws is not None),
                         int(stats is not None), 0, 0, 0)
        tag = ("conv_fwd_kernel", "conv_fwd_smallcin_kernel", "conv1x1_fwd_kernel", "conv_fwd8_kernel", "conv_fwd9_kernel")[kid]
        TIMER.records.append((s, e, 2.0 * B * Do * Ho * Wo * Cout * Cin * taps, tag, (B, D, H, W, Cin, Cout, kd, kh, kw)))
    return y


def _conv_bwd_weight_raw(x, dy, dw, db, geo, h_flags=None):
    """dW (and db unless None) of a conv from x and dY, on the fp32 entry or (``h_flags``: its ``bf16`` argument) on the 16-bit one: the
    workspace the entry's query asks for, the call and the timer record.  False: the 16-bit entry does not take the shape, nothing ran."""
    half = h_flags is not None
    n = _lib.query("diqt_conv3d_bwd_weight_h_workspace_bytes" if half else "diqt_conv3d_bwd_weight_workspace_bytes", *geo)
    if half and not n:
        return False
    ws = _workspace(n, x.device)
    if TIMER.enabled:
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
    if half:
        _lib.call("diqt_conv3d_bwd_weight_h", x, dy, dw, db, ws, n, *geo, h_flags, _stream())
    else:
        _lib.call("diqt_conv3d_bwd_weight", x, dy, dw, db, ws, n, *geo, _stream())
    if TIMER.enabled:
        e.record()
        # tagged with rocprofv3's name of the kernel the entry dispatches to; the interval also holds the fixed-order split-K slab sum
        # that finishes the gradient
        tag = "conv_wgrad_h_kernel" if half else ("conv_bwd_weight_gemm", "conv_bwd_weight_kernel", "conv_bwd_weight2_kernel",
                                                  "conv_wgrad3_kernel")[max(_lib.query("diqt_conv3d_bwd_weight_kernel_id", *geo), 0)]
        B, Cin, Cout, kd, kh, kw = geo[0], *geo[4:9]
        Do, Ho, Wo = dy.shape[1:4]
        TIMER.records.append((s, e, 2.0 * B * Do * Ho * Wo * Cout * Cin * kd * kh * kw, tag, tuple(geo[:9])))
    return True


class GnCtx:
    """What the backward-data pass of a conv needs to know about the fused GroupNorm + activation that produced its input."""
    __slots__ = ("x", "mean", "rstd", "gamma", "beta", "ss", "groups", "act")

    def __init__(self, x, mean, rstd, gamma, beta, ss, groups, act):
        self.x, self.mean, self.rstd, self.gamma, self.beta, self.ss, self.groups, self.act = x, mean, rstd, gamma, beta, ss, groups, act


def _conv_bwd_data_gn(dy, packed, Cout, k, pad, epad, gn):
    """dX of a conv whose input was act(GN(gn.x)): the conv_fwd9_kernel launch that computes dX also reduces the GroupNorm backward's
    per-channel sums in its epilogue; they travel to _GnActFn.backward on the gradient tensor (``_diqt_gnbwd``).  None: not this shape."""
    B, D, H, W, Cin = dy.shape
    kd, kh, kw = k
    geo = (B, D, H, W, Cin, Cout, kd, kh, kw, *pad, *epad)
    if gn.act not in (ACT_MISH, ACT_SILU) or tuple(gn.x.shape[-1:]) != (Cout,):
        return None
    nblk = _lib.query("diqt_conv3d_fwd_gnbwd_blocks", *geo)
    Do, Ho, Wo = D + 2 * pad[0] + epad[0] - kd + 1, H + 2 * pad[1] + epad[1] - kh + 1, W + 2 * pad[2] + epad[2] - kw + 1
    if nblk <= 0 or tuple(gn.x.shape) != (B, Do, Ho, Wo, Cout) or Cout % gn.groups != 0:
        return None
    dx = torch.empty((B, Do, Ho, Wo, Cout), dtype=torch.float32, device=dy.device)
    partials = torch.empty((B, nblk, 2, Cout), dtype=torch.float32, device=dy.device)
    scale = shift = None
    cs = 0
    if gn.ss is not None:
        scale, shift, cs = gn.ss.data_ptr(), gn.ss.data_ptr() + 4 * Cout, gn.ss.stride(0)
    if TIMER.enabled:
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
    _lib.call("diqt_conv3d_fwd_gnbwd", dy, packed, dx, partials, gn.x, gn.mean, gn.rstd, gn.gamma, gn.beta, scale, shift, cs, gn.groups,
              gn.act, *geo, _stream())
    if TIMER.enabled:
        e.record()
        TIMER.records.append((s, e, 2.0 * B * Do * Ho * Wo * Cout * Cin * kd * kh * kw, "conv_fwd9_kernel", geo[:9]))
    dx._diqt_gnbwd = (partials, nblk, dx._version, dx.data_ptr())
    return dx


class _Conv3dFn(Function):
    @staticmethod
    def forward(ctx, x, weight, bias, pad, residual, epad=(0, 0, 0), stats_out=None, gnctx=None):
        _chk(x, weight, bias, residual)
        ctx.gnctx = gnctx           # x = act(GN(.)): the backward-data pass can do the GroupNorm backward's reduction in its epilogue
        Cout, Cin, kd, kh, kw = weight.shape
        assert x.dim() == 5 and x.shape[-1] == Cin, f"conv3d: x {tuple(x.shape)} vs weight {tuple(weight.shape)}"
        lp = lp_mode()
        y = None
        if Cout <= 2 and stats_out is None:
            y = _conv_fwd_smallcout(x, weight, bias, residual, pad, epad)      # dim -> image channel: one pass over x on the vector ALU
            if y is not None:
                lp = None
        if y is None and lp is not None:
            y = _conv_fwd_half(x, weight, bias, residual, pad, epad, lp)
        if y is None:
            y = _conv_fwd_raw(x, _packed(weight, 0), bias, residual, Cout, (kd, kh, kw), pad, epad, stats_out)
        ctx.save_for_backward(x, weight)
        ctx.pad = pad
        ctx.epad = epad
        ctx.lp = lp                 # backward runs outside the autocast region: remember the forward's compute type
        ctx.has_bias = bias is not None
        ctx.has_res = residual is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        dy = dy.contiguous()
        Cout, Cin, kd, kh, kw = weight.shape
        pd, ph, pw = ctx.pad
        epd, eph, epw = ctx.epad
        B, D, H, W, _ = x.shape
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            # dX = conv(dY, flipped W): low pad' = k-1-pad_lo, high pad' = k-1-pad_hi  ->  epad' = -epad
            bpad, bepad = (kd - 1 - pd, kh - 1 - ph, kw - 1 - pw), (-epd, -eph, -epw)
            # bf16 training: backward-data on the bf16 MFMA kernel too (the reference's autocast backward runs in the forward's
            # type).  fp16 gradients would need the GradScaler the reference pairs with fp16; they stay on the fp32 kernel.
            lpb = _lp_backward(ctx.lp)
            dx = _conv_fwd_half(dy, weight, None, None, bpad, bepad, lpb, mode=1) if lpb is not None else None
            gn = ctx.gnctx
            if dx is None and gn is not None:
                dx = _conv_bwd_data_gn(dy, _packed(weight, 1), Cin, (kd, kh, kw), bpad, bepad, gn)
            if dx is None:
                dx = _conv_fwd_raw(dy, _packed(weight, 1), None, None, Cin, (kd, kh, kw), bpad, bepad)
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            dw = torch.empty_like(weight)
            db = torch.empty(Cout, dtype=torch.float32, device=x.device) if ctx.has_bias else None
            lpb = _lp_backward(ctx.lp)
            geo = (B, D, H, W, Cin, Cout, kd, kh, kw, pd, ph, pw, epd, eph, epw)
            # bf16 training: the weight gradient on the bf16 MFMA too (x and dY rounded to bf16 while staged, fp32 accumulation; the
            # reference's autocast backward runs in the forward's type); other shapes stay on the fp32 kernel
            if lpb is None or not _conv_bwd_weight_raw(x, dy, dw, db, geo, lpb):
                _conv_bwd_weight_raw(x, dy, dw, db, geo)
        return dx, dw, db, None, (dy if ctx.has_res else None), None, None, None


def conv3d(x, weight, bias=None, padding=(0, 0, 0), residual=None, extra_pad=(0, 0, 0), want_stats=False, split16=False):
    """Stride-1 conv on channels-last x[B,D,H,W,Cin] with an OIDHW weight (MFMA implicit GEMM).
    Filters whose halo tile cannot fit the 160 KiB LDS (e.g. 15^3 cross-embed taps) take the direct kernel.
    ``split16`` (no autograd, no autocast): ask for the three-product split on the fp16 matrix pipe (``_conv_fwd_split16``); a launch
    it does not grant takes the default route.  ``split16="fill"`` asks its fill plan first, ``split16="pair"`` its pair plan and then the
    fill plan (``_split16_plan``)."""
    if isinstance(padding, int):
        padding = (padding,) * 3
    padding = tuple(int(p) for p in padding)
    extra_pad = tuple(int(p) for p in extra_pad)
    if split16 and SPLIT16 and not torch.is_grad_enabled() and lp_mode() is None and x.dim() == 5 and x.shape[-1] == weight.shape[1]:
        _chk(x, weight, bias, residual)
        y = _conv_fwd_split16(x, weight, bias, residual, padding, extra_pad, want_stats, split16=split16)
        if y is not None:
            return y
    _, D, H, W, _ = x.shape
    kd, kh, kw = weight.shape[2:]
    if _lib.query("diqt_conv3d_lds_bytes", D, H, W, kd, kh, kw, *padding, *extra_pad) > 160 * 1024:
        y = _ConvDirectFn.apply(x, weight, bias, (1, 1, 1), padding, 1, extra_pad)
        return y if residual is None else add(y, residual)
    gnctx = getattr(x, "_diqt_gnctx", None) if torch.is_grad_enabled() else None
    if not want_stats:
        return _Conv3dFn.apply(x, weight, bias, padding, residual, extra_pad, None, gnctx)
    holder = []
    y = _Conv3dFn.apply(x, weight, bias, padding, residual, extra_pad, holder, gnctx)
    if holder:
        y._diqt_stats = holder[0]           # consumed by groupnorm_act / se_gate_residual on this exact tensor
    return y


def _packed_d2s(weight5, bias):
    """(packed weights, packed bias) of a 1x1x1 conv whose output goes through depth-to-space by 2, in the column order (q, c') of the
    deep channel 8 c' + q that ``diqt_conv1x1_fwd_ex`` wants; cached on the weight like ``_packed`` until either tensor changes."""
    owner = weight5._base if weight5._base is not None else weight5
    cache = getattr(owner, "_diqt_pack", None)
    if cache is None:
        cache = {}
        try:
            owner._diqt_pack = cache
        except Exception:
            pass
    key = ("d2s", weight5.data_ptr(), weight5._version, _WEIGHT_EPOCH) + \
        ((bias.data_ptr(), bias._version) if bias is not None else (0, -1))
    hit = cache.get("d2s")
    if hit is not None and hit[0] == key:
        return hit[1], hit[2]
    Cout, Cin = weight5.shape[:2]
    packed = torch.empty(_lib.query("diqt_conv_packed_elems", Cout, Cin, 1, 1, 1), dtype=torch.float32, device=weight5.device)
    bpk = torch.empty(Cout, dtype=torch.float32, device=weight5.device) if bias is not None else None
    _lib.call("diqt_conv1x1_pack_d2s", weight5.detach(), bias.detach() if bias is not None else None, packed, bpk, Cout, Cin, _stream())
    if hit is not None:
        retire(hit[1], hit[2])
    cache["d2s"] = (key, born(packed), born(bpk) if bpk is not None else None)
    return packed, bpk


def _conv1x1_ex_ok(x, weight, *more):
    if torch.is_grad_enabled() or lp_mode() is not None or x.dim() != 5 or x.dtype != torch.float32 or not x.is_cuda:
        return False
    if tuple(weight.shape[2:]) != (1, 1, 1) or weight.shape[1] != x.shape[-1] or weight.dtype != torch.float32:
        return False
    return all(t is None or (t.dtype == torch.float32 and t.is_cuda) for t in more)


def conv1x1_act_shuffle(x, weight, bias, act=ACT_MISH, want_stats=False):
    """Sampling path (no autograd, fp32): depth_to_space(act(conv1x1(x))) -- the pixel-shuffle up-sampler -- as ONE launch: the conv's
    epilogue applies the activation and stores each 64-channel tile straight into its fine voxels.  Bit-identical to
    ``conv3d`` -> ``activation`` -> ``depth_to_space``.  ``want_stats``: the launch also writes the column sums of its output
    (``_diqt_stats``) where the shape allows.  Returns None when the shape is not taken (the caller keeps the three launches)."""
    if not _conv1x1_ex_ok(x, weight, bias):
        return None
    B, D, H, W, Cin = x.shape
    Cout = weight.shape[0]
    if not _lib.query("diqt_conv1x1_fwd_ex_supported", B, D, H, W, Cin, Cout, act, 1, 0, 0):
        return None
    x = x.contiguous()
    _chk(x, weight, bias)
    packed, bpk = _packed_d2s(weight, bias)
    y = torch.empty((B, 2 * D, 2 * H, 2 * W, Cout // 8), dtype=torch.float32, device=x.device)
    stats = None
    nblk = _lib.query("diqt_conv1x1_fwd_ex_stats_blocks", B, D, H, W, Cin, Cout, act, 1, 0) if want_stats else 0
    if nblk > 0:
        stats = torch.empty((B, nblk, 2, Cout // 8), dtype=torch.float32, device=x.device)
        y._diqt_stats = ColStats(stats, nblk, 8 * D * H * W)
    _lib.call("diqt_conv1x1_fwd_ex", x, packed, bpk, None, None, y, stats, B, D, H, W, Cin, Cout, act, 1, _stream())
    return y


def conv1x1_stats(x, weight, bias):
    """Sampling path: conv1x1(x) whose epilogue also writes the column sums of its output (``_diqt_stats``) for the GroupNorm that
    consumes it.  Returns None when the shape is not taken (rows per batch entry that are no multiple of 128, ...)."""
    if not _conv1x1_ex_ok(x, weight, bias):
        return None
    B, D, H, W, Cin = x.shape
    Cout = weight.shape[0]
    nblk = _lib.query("diqt_conv1x1_fwd_ex_stats_blocks", B, D, H, W, Cin, Cout, 0, 0, 0)
    if nblk <= 0:
        return None
    x = x.contiguous()
    _chk(x, weight, bias)
    y = torch.empty((B, D, H, W, Cout), dtype=torch.float32, device=x.device)
    stats = torch.empty((B, nblk, 2, Cout), dtype=torch.float32, device=x.device)
    _lib.call("diqt_conv1x1_fwd_ex", x, _packed(weight, 0), bias, None, None, y, stats, B, D, H, W, Cin, Cout, 0, 0, _stream())
    y._diqt_stats = ColStats(stats, nblk, D * H * W)
    return y


def se_conv1x1_residual(h, w1, w2, x, weight, bias):
    """Sampling path: h * sigmoid(relu(mean(h) w1^T) w2^T) + conv1x1(x) -- the tail of a ResnetBlock with an SE block and a 1x1
    ``res_conv`` -- in two launches: the gate from the column sums h carries (the first launch of ``se_gate_residual``), then the conv,
    whose epilogue applies the gate to h, adds, and writes the block output with its column sums (``_diqt_stats``): the residual branch
    is never written to memory and read back.  Bit-identical to ``conv3d`` + ``se_gate_residual``.  None: shape not taken."""
    pre = getattr(h, "_diqt_stats", None)
    if pre is None or h.dim() != 5 or not _conv1x1_ex_ok(x, weight, bias, h, w1, w2):
        return None
    B, D, H, W, Cin = x.shape
    C = weight.shape[0]
    rows = D * H * W
    if tuple(h.shape) != (B, D, H, W, C) or pre.rows != rows or pre.partials.shape != (B, pre.nblk, 2, C):
        return None
    if not (256 % min(C, 256) == 0 and (C <= 256 or C % 256 == 0)):        # the one-launch pool + MLP of _SEResidualFn
        return None
    nblk = _lib.query("diqt_conv1x1_fwd_ex_stats_blocks", B, D, H, W, Cin, C, 0, 0, 1)
    if nblk <= 0:
        return None
    x = x.contiguous()
    _chk(x, weight, bias, h, w1, w2)
    dev, s = x.device, _stream()
    Cr = w1.shape[0]
    pooled = torch.empty((B, C), dtype=torch.float32, device=dev)
    hidden = torch.empty((B, Cr), dtype=torch.float32, device=dev)
    gate = torch.empty((B, C), dtype=torch.float32, device=dev)
    _lib.call("diqt_se_pool_mlp_fwd", pre.partials, pre.nblk, rows, pooled, w1, w2, hidden, gate, B, C, Cr, s)
    y = torch.empty((B, D, H, W, C), dtype=torch.float32, device=dev)
    stats = torch.empty((B, nblk, 2, C), dtype=torch.float32, device=dev)
    _lib.call("diqt_conv1x1_fwd_ex", x, _packed(weight, 0), bias, h, gate, y, stats, B, D, H, W, Cin, C, 0, 0, s)
    y._diqt_stats = ColStats(stats, nblk, rows)
    return y


def conv3d_neighbours(x, weight, bias, f, residual=None, want_stats=False):
    """Inference-only 'same' conv over the f^3 sub-volume batch x[f^3, A, A, A, Cin] of one merged volume whose halo voxels come
    from the NEIGHBOUR sub-volumes (zero only outside the merged volume) -- the reference's ``boundary_pad`` + unpadded Conv3d
    (imagen_pytorch3D.py:37-46, 550-566) without the merge / pad / split copies.  No autograd: training keeps the copy path."""
    _chk(x, weight, bias, residual)
    assert not torch.is_grad_enabled() or not (x.requires_grad or weight.requires_grad), 'conv3d_neighbours is the sampling path'
    B, A, A2, A3, Cin = x.shape
    Cout, Cin2, k, k2, k3 = weight.shape
    assert B == f ** 3 and A == A2 == A3 and Cin == Cin2 and k == k2 == k3 and k % 2 == 1, (tuple(x.shape), tuple(weight.shape), f)
    if lp_mode() is not None:          # mixed precision: the 16-bit kernel has no neighbour tables -- materialise the copies
        return None
    p = k // 2
    geo = (B, A, A, A, Cin, Cout, k, k, k, p, p, p, 0, 0, 0)
    y = torch.empty((B, A, A, A, Cout), dtype=torch.float32, device=x.device)
    n = _lib.query("diqt_conv3d_fwd_workspace_bytes", *geo)
    ws = _workspace(n, x.device) if n else None
    stats = None
    if want_stats:
        nblk = _lib.query("diqt_conv3d_fwd_neighbours_stats_blocks", f, A, Cin, Cout, k)
        if nblk > 0:
            stats = torch.empty((B, nblk, 2, Cout), dtype=torch.float32, device=x.device)
            y._diqt_stats = ColStats(stats, nblk, A * A * A)
    _lib.call("diqt_conv3d_fwd_neighbours", x, _packed(weight, 0), bias, residual, y, stats, ws, n, f, A, Cin, Cout, k, _stream())
    return y


class _LinearSmallFn(Function):
    """nn.Linear over <= 64 rows (time-conditioning MLPs): one wave per output column, no MFMA pipeline fill."""
    @staticmethod
    def forward(ctx, x2, weight, bias):
        _chk(x2, weight, bias)
        M, K = x2.shape
        N = weight.shape[0]
        y = torch.empty((M, N), dtype=torch.float32, device=x2.device)
        _lib.call("diqt_linear_small_fwd", x2, weight, bias, y, M, K, N, _stream())
        ctx.save_for_backward(x2, weight)
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x2, weight = ctx.saved_tensors
        dy = dy.contiguous()
        M, K = x2.shape
        N = weight.shape[0]
        need_dx, need_dw = ctx.needs_input_grad[0], ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2])
        dx = torch.empty_like(x2) if need_dx else None
        dw = torch.empty_like(weight) if need_dw else None
        db = torch.empty(N, dtype=torch.float32, device=x2.device) if (need_dw and ctx.has_bias) else None
        n = _lib.query("diqt_linear_small_workspace_bytes", M, K, N)
        ws = _workspace(n, x2.device)
        _lib.call("diqt_linear_small_bwd", x2, weight, dy, dx, dw, db, ws, n, M, K, N, _stream())
        return dx, dw, db


class _BatchedLinearSmallFn(Function):
    """y_i = a W_i^T + b_i for n Linear layers that share the input a[M <= 64, K] (the time MLPs of a U-Net's ResnetBlocks,
    imagen_pytorch3D.py:586-589 / imagen_video.py:716-719) as ONE launch over the concatenated weights, with autograd: the outputs are
    column blocks of one [M, sum N_i] buffer, their gradients are written by the consumers (GroupNorm backward) into the same blocks of
    one shared gradient buffer, and backward is one dx / dW / db launch set instead of three per layer plus a sum of n gradients of a."""
    @staticmethod
    def forward(ctx, a, wcat, bcat, gradbuf, sizes, *params):
        _chk(a, wcat, bcat)
        M, K = a.shape
        N = wcat.shape[0]
        out = torch.empty((M, N), dtype=torch.float32, device=a.device)
        _lib.call("diqt_linear_small_fwd", a, wcat, bcat, out, M, K, N, _stream())
        ctx.save_for_backward(a, wcat)
        ctx.gradbuf, ctx.sizes, ctx.has_bias = gradbuf, sizes, [b is not None for b in params[1::2]]
        ctx.set_materialize_grads(False)
        offs, o = [], 0
        for n in sizes:
            offs.append(o)
            o += n
        ctx.offs = offs
        return tuple(out[:, o:o + n] for o, n in zip(offs, sizes))

    @staticmethod
    def backward(ctx, *grads):
        a, wcat = ctx.saved_tensors
        M, K = a.shape
        N = wcat.shape[0]
        buf = ctx.gradbuf
        used = [g is not None for g in grads]     # a layer whose output nobody consumed (mid_block) keeps grad None, like unbatched
        for g, o, n in zip(grads, ctx.offs, ctx.sizes):
            dst = buf[:, o:o + n]
            if g is None:
                dst.zero_()
            elif g.data_ptr() != dst.data_ptr() or g.stride() != dst.stride():
                dst.copy_(g)                    # a consumer that did not write in place (not the fused GroupNorm backward)
        dx = torch.empty_like(a) if ctx.needs_input_grad[0] else None
        dw = torch.empty_like(wcat)
        db = torch.empty(N, dtype=torch.float32, device=a.device)
        n = _lib.query("diqt_linear_small_workspace_bytes", M, K, N)
        ws = _workspace(n, a.device)
        _lib.call("diqt_linear_small_bwd", a, wcat, buf, dx, dw, db, ws, n, M, K, N, _stream())
        pg = []
        for o, nn_, hb, u in zip(ctx.offs, ctx.sizes, ctx.has_bias, used):
            pg.append(dw[o:o + nn_] if u else None)
            pg.append(db[o:o + nn_] if (hb and u) else None)
        return (dx, None, None, None, None, *pg)


def batched_linear_small(a, wcat, bcat, linears):
    """One launch for ``[l(a) for l in linears]`` (wcat / bcat: their concatenated weights / biases, rebuilt by the caller when a
    parameter changes).  Returns the outputs as [M, N_i] column blocks; each carries ``_diqt_gradview``, its block of the shared
    gradient buffer (ops.groupnorm_act's backward writes d scale/shift there)."""
    sizes = tuple(l.weight.shape[0] for l in linears)
    gradbuf = torch.empty((a.shape[0], wcat.shape[0]), dtype=torch.float32, device=a.device)
    params = []
    for l in linears:
        params += [l.weight, l.bias]
    outs = _BatchedLinearSmallFn.apply(a.contiguous(), wcat, bcat, gradbuf, sizes, *params)
    o = 0
    for t, n in zip(outs, sizes):
        t._diqt_gradview = gradbuf[:, o:o + n]
        o += n
    return outs


def linear(x, weight, bias=None):
    """x[..., Cin] @ weight[Cout, Cin]^T + bias: skinny kernel for <= 64 rows, otherwise the MFMA kernel (1x1x1 conv)."""
    Cout, Cin = weight.shape
    lead = x.shape[:-1]
    rows = x.numel() // Cin
    if 0 < rows <= 64:
        return _LinearSmallFn.apply(x.reshape(rows, Cin).contiguous(), weight.contiguous(), bias).reshape(*lead, Cout)
    y = _Conv3dFn.apply(x.reshape(1, 1, 1, -1, Cin), weight.view(Cout, Cin, 1, 1, 1), bias, (0, 0, 0), None, (0, 0, 0))
    return y.reshape(*lead, Cout)


class _ConvDirectFn(Function):
    @staticmethod
    def forward(ctx, x, weight, bias, stride, pad, groups, epad=(0, 0, 0)):
        _chk(x, weight, bias)
        B, D, H, W, Cin = x.shape
        Cout, _, kd, kh, kw = weight.shape
        sd, sh, sw = stride
        pd, ph, pw = pad
        epd, eph, epw = epad
        Do, Ho, Wo = (D + 2 * pd + epd - kd) // sd + 1, (H + 2 * ph + eph - kh) // sh + 1, (W + 2 * pw + epw - kw) // sw + 1
        y = torch.empty((B, Do, Ho, Wo, Cout), dtype=torch.float32, device=x.device)
        ctx.geom = (B, D, H, W, Cin, Cout, groups, kd, kh, kw, sd, sh, sw, pd, ph, pw, epd, eph, epw)
        _lib.call("diqt_conv3d_direct_fwd", x, weight, bias, y, *ctx.geom, _stream())
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        dy = dy.contiguous()
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            _lib.call("diqt_conv3d_direct_bwd_data", dy, weight, dx, *ctx.geom, _stream())
        if ctx.needs_input_grad[1]:
            dw = torch.empty_like(weight)
            db = torch.empty(weight.shape[0], dtype=torch.float32, device=x.device) if ctx.has_bias else None
            nws = _lib.query("diqt_conv3d_direct_bwd_weight_workspace_bytes", *ctx.geom)
            ws = _workspace(nws, x.device) if nws else None
            _lib.call("diqt_conv3d_direct_bwd_weight_ws", x, dy, dw, db, ws, nws, *ctx.geom, _stream())
        return dx, dw, db, None, None, None, None


def conv3d_direct(x, weight, bias=None, stride=(1, 1, 1), padding=(0, 0, 0), groups=1, extra_pad=(0, 0, 0)):
    t3 = lambda v: (v,) * 3 if isinstance(v, int) else tuple(v)
    return _ConvDirectFn.apply(x, weight, bias, t3(stride), t3(padding), int(groups), t3(extra_pad))


class _DwConvTemporalFn(Function):
    """Depthwise (3,1,1) temporal conv + bias (+ residual) on channels-last x[B,F,H,W,C] (the TemporalPEG of the pseudo-3D U-Net)."""
    @staticmethod
    def forward(ctx, x, weight, bias, left, res, res_is_x=False):
        """res_is_x: the residual IS the input (`conv(x) + x`, the TemporalPEG): one autograd input, and the backward-data launch adds
        dy to its own result -- otherwise autograd sums the two gradients of x in a separate pass."""
        if res_is_x:
            res = x
        _chk(x, weight, bias, res)
        B, F, H, W, C = x.shape
        kt = weight.shape[2]
        w2 = weight.reshape(C, kt).contiguous()
        y = torch.empty_like(x)
        _lib.call("diqt_dwconv_temporal_fwd", x, w2, bias, res, y, B, F, H * W, C, kt, int(left), 0, _stream())
        ctx.save_for_backward(x, w2)
        ctx.cfg = (B, F, H * W, C, kt, int(left), bias is not None, res is not None and not res_is_x, tuple(weight.shape))
        ctx.res_is_x = res_is_x
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w2 = ctx.saved_tensors
        B, F, P, C, kt, left, has_bias, has_res, wshape = ctx.cfg
        dy = dy.contiguous()
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            _lib.call("diqt_dwconv_temporal_fwd", dy, w2, None, dy if ctx.res_is_x else None, dx, B, F, P, C, kt, kt - 1 - left, 1, _stream())
        if ctx.needs_input_grad[1]:
            n = _lib.query("diqt_dwconv_temporal_bwd_weight_workspace_bytes", B, F, P, C, kt)
            ws = _workspace(n, x.device)
            dwb = torch.empty((kt + 1, C), dtype=torch.float32, device=x.device)
            _lib.call("diqt_dwconv_temporal_bwd_weight", x, dy, dwb, ws, n, B, F, P, C, kt, left, _stream())
            dw = dwb[:kt].t().reshape(wshape)
            db = dwb[kt].clone() if has_bias else None
        return dx, dw, db, None, (dy if has_res else None), None


def dwconv_temporal_ok(x, weight, groups, stride=(1, 1, 1)):
    C = x.shape[-1]
    return (x.dim() == 5 and tuple(weight.shape) == (C, 1, 3, 1, 1) and groups == C and tuple(stride) == (1, 1, 1)
            and C % 4 == 0 and 256 % (C // 4) == 0)


def dwconv_temporal(x, weight, bias, left, residual=None):
    """nn.Conv3d(C, C, (3,1,1), groups=C) on frames padded with ``left`` zero frames in front (2: causal, 1: symmetric), + residual."""
    if residual is x:
        return _DwConvTemporalFn.apply(x.contiguous(), weight, bias, int(left), None, True)
    return _DwConvTemporalFn.apply(x.contiguous(), weight, bias, int(left), residual.contiguous() if residual is not None else None)


# --------------------------------------------------------------------------------------------
# GroupNorm + scale/shift + activation
# --------------------------------------------------------------------------------------------
class SSView:
    """Columns [off, off + width) of a batched time-MLP output ``base`` [B, sum of widths]: the (scale | shift) embedding of one
    ResnetBlock when all blocks' time MLPs ran as ONE launch (sampling path)."""
    __slots__ = ("base", "off", "width")

    def __init__(self, base, off, width):
        self.base, self.off, self.width = base, off, width


class _GnActFn(Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, ss, groups, act, eps, pre=None, gn_out=None, tap=False, ss_grad=None):
        """tap=True: also returns x itself as a second output.  The caller routes x's OTHER consumer (the residual branch of a
        ResnetBlock) through that alias, so autograd sees one consumer of x and hands the branch's gradient to backward(), where it is
        added inside the dx kernel instead of by a separate elementwise pass."""
        _chk(x, gamma, beta, ss.base if isinstance(ss, SSView) else None)
        if ss is not None and not isinstance(ss, SSView):          # [B, 2C] rows, possibly a column block of a wider buffer
            assert ss.is_cuda and ss.dtype == torch.float32 and ss.dim() == 2 and ss.stride(1) == 1, "scale/shift rows must be fp32 HIP tensors"
        ctx.tap = tap
        ctx.set_materialize_grads(False)
        B, C = x.shape[0], x.shape[-1]
        rows = x.numel() // (B * C)
        mean = torch.empty(B * groups, dtype=torch.float32, device=x.device)
        rstd = torch.empty_like(mean)
        s = _stream()
        if pre is not None and pre.rows == rows and pre.partials.shape == (B, pre.nblk, 2, C):
            # the producing conv's epilogue already summed x and x^2 per tile: no pass over x for the statistics
            _lib.call("diqt_groupnorm_stats_from_partials", pre.partials, mean, rstd, B, pre.nblk, rows, C, groups, float(eps), s)
        else:
            ws, n = _reduce_ws(B, C, x.device)
            _lib.call("diqt_groupnorm_stats", x, mean, rstd, ws, n, B, rows, C, groups, float(eps), s)
        y = torch.empty_like(x)
        scale = shift = None
        cs = 0
        if isinstance(ss, SSView):
            # one row block of a batched time-MLP output [B, sum 2C_i] (sampling path, no autograd): columns off .. off + 2C
            assert ss.width == 2 * C and ss.base.shape[0] == B and not torch.is_grad_enabled()
            scale, cs = ss.base.data_ptr() + 4 * ss.off, ss.base.shape[1]
            shift = scale + 4 * C
            _lib.call("diqt_gn_act_fwd", x, mean, rstd, gamma, beta, scale, shift, cs, y, B, rows, C, groups, act, s)
            return y
        if ss is not None:
            assert ss.shape == (B, 2 * C) and ss.stride(1) == 1, f"scale/shift embedding must be [B, 2C] rows, got {tuple(ss.shape)}"
            scale, shift, cs = ss.data_ptr(), ss.data_ptr() + 4 * C, ss.stride(0)
        _lib.call("diqt_gn_act_fwd", x, mean, rstd, gamma, beta, scale, shift, cs, y, B, rows, C, groups, act, s)
        # a column block of the batched time-MLP output (batched_time_mlps): its gradient is written straight into the block's place in
        # the shared gradient buffer
        ctx.ss_grad = ss_grad
        ctx.save_for_backward(x, gamma, beta, ss, mean, rstd)
        ctx.cfg = (B, rows, C, groups, act)
        if gn_out is not None and x.dim() == 5:
            gn_out.append(GnCtx(x, mean, rstd, gamma, beta, ss, groups, act))
        return (y, x) if tap else y

    @staticmethod
    def backward(ctx, dy, dtap=None):
        x, gamma, beta, ss, mean, rstd = ctx.saved_tensors
        B, rows, C, groups, act = ctx.cfg
        if dy is None:                      # only the alias was used downstream
            return dtap, None, None, None, None, None, None, None, None, None, None
        if dtap is not None:
            dtap = dtap.contiguous()
        # partial sums from the producer of dy -- valid only for the very tensor they were computed for (autograd adds other
        # branches' gradients in place: the version counter tells)
        pre = getattr(dy, "_diqt_gnbwd", None)
        if pre is not None and (pre[2] != dy._version or pre[3] != dy.data_ptr() or not dy.is_contiguous()):
            pre = None
        dy = dy.contiguous()
        dx = torch.empty_like(x)
        dgamma = torch.empty_like(gamma) if gamma is not None else None
        dbeta = torch.empty_like(beta) if beta is not None else None
        scale = shift = dscale = dshift = None
        dss = None
        cs = 0
        if ss is not None:
            cs = ss.stride(0)
            dss = ctx.ss_grad if ctx.ss_grad is not None else torch.empty_strided(ss.shape, ss.stride(), dtype=ss.dtype, device=ss.device)
            assert dss.stride() == ss.stride()
            scale, shift = ss.data_ptr(), ss.data_ptr() + 4 * C
            dscale, dshift = dss.data_ptr(), dss.data_ptr() + 4 * C
        ws, n = _reduce_ws(B, C, x.device)
        # pre: the conv behind this GroupNorm reduced (sum dz, sum dz xhat) in the epilogue of its backward-data pass; dtap: the
        # gradient of x's other consumer, added in the dx pass
        part, nblk = (pre[0], pre[1]) if pre is not None and pre[0].shape == (B, pre[1], 2, C) else (None, 0)
        _lib.call("diqt_gn_act_bwd_ex", x, dy, part, nblk, dtap, mean, rstd, gamma, beta, scale, shift, cs, dx, dgamma, dbeta,
                  dscale, dshift, ws, n, B, rows, C, groups, act, _stream())
        return dx, dgamma, dbeta, dss, None, None, None, None, None, None, None


# fp16 training with a loss scaler (ImagenTrainer(fp16=True): the reference pairs fp16 autocast with torch's GradScaler, trainer.py:293-311,
# 364): the trainer sets this while its scaler is active, and the backward kernels of fp16-forward convs then run on the fp16 MFMA too
# (dY carries the loss scale, which is what keeps fp16 gradients out of the denormals).  Without a scaler fp16 backward stays in fp32.
FP16_BACKWARD = False


def _lp_backward(lp):
    """The 16-bit type of a conv's backward kernels: bf16 always follows the forward; fp16 only under a loss scaler; else None (fp32)."""
    return lp if lp == 1 or (lp == 0 and FP16_BACKWARD) else None


_NO_TRAIN_FUSE = os.environ.get("DIQT_NO_TRAIN_FUSE") == "1"      # A/B switch: bf16 training Blocks as two autograd nodes
_NO_TRAIN_HALF = os.environ.get("DIQT_NO_TRAIN_HALF") == "1"      # A/B switch: fp32 tensor (and gradient) between block1 and block2


class _GnActConvHFn(Function):
    """Training under ``ImagenTrainer(precision='bf16')`` -- or ``fp16=True`` with its loss scaler -- (trainer.py:293-311):
    ``conv3d(act(GN(x) * (scale + 1) + shift))`` as ONE autograd node whose intermediate -- the conv's input -- exists only in the 16-bit
    operand type: the GroupNorm-apply pass writes it so (the bits autocast's cast of the fp32 tensor produces), the forward conv reads it
    through ``conv_f9h_kernel`` (LDS-DMA, 16-bit x) and the weight gradient reads the same tensor (``diqt_conv3d_bwd_weight_h``, bit 1).
    ``out_half``: the conv's OUTPUT is an autograd tensor of that type too (a ResnetBlock's block1 -> block2: a conv result autocast rounds
    anyway); the node that consumes it (x of a 16-bit type, statistics from the column sums) hands back a 16-bit gradient
    (``diqt_gn_act_bwd_h``), which this node's backward-data runs through ``conv_f9h_kernel`` and its weight gradient reads as it is (bit 2)
    -- the same bits the fp32 tensors round to inside those kernels.  Bit-identical to the two-node path (``_GnActFn`` + ``_Conv3dFn``)."""
    @staticmethod
    def forward(ctx, x, gamma, beta, ss, groups, act, eps, pre, weight, bias, pad, residual, stats_out, tap, ss_grad, out_half):
        x_half = x.dtype != torch.float32
        _chk(None if x_half else x, gamma, beta, weight, bias, residual)
        if ss is not None:
            assert ss.is_cuda and ss.dtype == torch.float32 and ss.dim() == 2 and ss.stride(1) == 1, "scale/shift rows must be fp32 HIP tensors"
        assert not (x_half and tap), "the alias output routes an fp32 input's second consumer"
        ctx.tap = tap
        ctx.set_materialize_grads(False)
        B, C = x.shape[0], x.shape[-1]
        rows = x.numel() // (B * C)
        mean = torch.empty(B * groups, dtype=torch.float32, device=x.device)
        rstd = torch.empty_like(mean)
        s = _stream()
        if pre is not None and pre.rows == rows and pre.partials.shape == (B, pre.nblk, 2, C):
            _lib.call("diqt_groupnorm_stats_from_partials", pre.partials, mean, rstd, B, pre.nblk, rows, C, groups, float(eps), s)
        else:
            assert not x_half, "a 16-bit block output must carry the GroupNorm statistics of the conv that wrote it"
            ws, n = _reduce_ws(B, C, x.device)
            _lib.call("diqt_groupnorm_stats", x, mean, rstd, ws, n, B, rows, C, groups, float(eps), s)
        scale = shift = None
        cs = 0
        if ss is not None:
            assert ss.shape == (B, 2 * C), f"scale/shift embedding must be [B, 2C] rows, got {tuple(ss.shape)}"
            scale, shift, cs = ss.data_ptr(), ss.data_ptr() + 4 * C, ss.stride(0)
        lp = lp_mode()                                       # 1: bf16, 0: fp16 (under a loss scaler)
        hdt = torch.bfloat16 if lp == 1 else torch.float16
        assert not x_half or x.dtype == hdt
        y16 = torch.empty(x.shape, dtype=hdt, device=x.device)
        _lib.call("diqt_gn_act_fwd_h", x, mean, rstd, gamma, beta, scale, shift, cs, y16, B, rows, C, groups, act, lp, int(x_half), s)
        y = _conv_fwd_half(y16, weight, bias, residual, pad, (0, 0, 0), lp, x_half=True, y_half=bool(out_half), stats_out=stats_out)
        ctx.lp = lp
        ctx.ss_grad = ss_grad
        ctx.save_for_backward(x, gamma, beta, ss, mean, rstd, y16, weight)
        ctx.cfg = (B, rows, C, groups, act, pad, bias is not None, residual is not None, x_half, bool(out_half))
        return (y, x) if tap else y

    @staticmethod
    def backward(ctx, dy, dtap=None):
        x, gamma, beta, ss, mean, rstd, y16, weight = ctx.saved_tensors
        B, rows, C, groups, act, pad, has_bias, has_res, x_half, y_half = ctx.cfg
        none = (None,) * 16
        if dy is None:                      # only the alias was used downstream
            return (dtap,) + none[1:]
        dy = dy.contiguous()
        assert (dy.dtype != torch.float32) == y_half
        Cout, Cin, kd, kh, kw = weight.shape
        D, H, W = x.shape[1:4]
        pd, ph, pw = pad
        bpad = (kd - 1 - pd, kh - 1 - ph, kw - 1 - pw)
        # ---- conv: dX on the 16-bit MFMA kernel (flipped weights; conv_f9h_kernel when dY is 16-bit), dW / db with the 16-bit activation ----
        # the gradient w.r.t. the activated tensor only feeds the GroupNorm backward's two passes: in the operand type when the 16-bit
        # kernel writes it (what autocast's conv backward returns anyway) -- half the bytes written here and read twice there
        dact_half = bool(y_half and not _NO_TRAIN_HALF and Cin % 8 == 0
                         and _lib.query("diqt_conv3d_fwd_h_io16_supported", B, D, H, W, Cout, Cin, kd, kh, kw, *bpad, 0, 0, 0, 1, 1))
        dact = _conv_fwd_half(dy, weight, None, None, bpad, (0, 0, 0), ctx.lp, mode=1, x_half=y_half, y_half=dact_half)
        if dact is None:
            assert not y_half
            dact = _conv_fwd_raw(dy, _packed(weight, 1), None, None, Cin, (kd, kh, kw), bpad, (0, 0, 0))
        dw = torch.empty_like(weight)
        db = torch.empty(Cout, dtype=torch.float32, device=x.device) if has_bias else None
        geo = (B, D, H, W, Cin, Cout, kd, kh, kw, pd, ph, pw, 0, 0, 0)
        took = _conv_bwd_weight_raw(y16, dy, dw, db, geo, ctx.lp | 2 | (4 if y_half else 0))      # bit 1: x is 16-bit, bit 2: dY is 16-bit
        assert took
        # ---- GroupNorm + activation backward (as _GnActFn.backward; a 16-bit x gets a 16-bit gradient) ----
        if dtap is not None:
            dtap = dtap.contiguous()
        dx = torch.empty_like(x)
        dgamma = torch.empty_like(gamma) if gamma is not None else None
        dbeta = torch.empty_like(beta) if beta is not None else None
        scale = shift = dscale = dshift = None
        dss = None
        cs = 0
        if ss is not None:
            cs = ss.stride(0)
            dss = ctx.ss_grad if ctx.ss_grad is not None else torch.empty_strided(ss.shape, ss.stride(), dtype=ss.dtype, device=ss.device)
            assert dss.stride() == ss.stride()
            scale, shift = ss.data_ptr(), ss.data_ptr() + 4 * C
            dscale, dshift = dss.data_ptr(), dss.data_ptr() + 4 * C
        ws, n = _reduce_ws(B, C, x.device)
        if x_half or dact_half:
            ty = 2 if ctx.lp == 1 else 1
            xt = ty if x_half else 0
            _lib.call("diqt_gn_act_bwd_h", x, dact, None, 0, dtap, mean, rstd, gamma, beta, scale, shift, cs, dx, dgamma, dbeta,
                      dscale, dshift, ws, n, B, rows, C, groups, act, xt, xt, ty if dact_half else 0, _stream())
        else:
            _lib.call("diqt_gn_act_bwd_ex", x, dact, None, 0, dtap, mean, rstd, gamma, beta, scale, shift, cs, dx, dgamma, dbeta,
                      dscale, dshift, ws, n, B, rows, C, groups, act, _stream())
        return dx, dgamma, dbeta, dss, None, None, None, None, dw, db, None, (dy if has_res else None), None, None, None, None


def _train_h_geo_ok(B, D, H, W, Cin, Cout, k, padding, groups):
    """Is a 'same' conv of this shape taken by the one-node low-precision training Block (16-bit-x forward kernel + 16-bit weight gradient)?"""
    kd, kh, kw = k
    geo = (B, D, H, W, Cin, Cout, kd, kh, kw, *padding, 0, 0, 0)
    if Cin % groups != 0 or Cin % 8 != 0 or not _lib.query("diqt_conv3d_fwd_h_io16_supported", *geo, 1, 0):
        return False
    if _lib.query("diqt_conv3d_bwd_weight_h_workspace_bytes", *geo) == 0:
        return False
    return D + 2 * padding[0] - kd + 1 == D and H + 2 * padding[1] - kh + 1 == H and W + 2 * padding[2] - kw + 1 == W


def train_half_out_ok(shape5, w_next, padding_next, groups_next):
    """May a Block of a low-precision TRAINING step hand its conv output on in the operand type?  (the next Block has to take it: see
    ``gn_conv3d_train_h``)"""
    if _lp_backward(lp_mode()) is None or not torch.is_grad_enabled() or _NO_TRAIN_FUSE or _NO_TRAIN_HALF:
        return False
    B, D, H, W, C = shape5
    Cout, Cin, kd, kh, kw = w_next.shape
    padding_next = tuple(int(p) for p in ((padding_next,) * 3 if isinstance(padding_next, int) else padding_next))
    return Cin == C and _train_h_geo_ok(B, D, H, W, C, Cout, (kd, kh, kw), padding_next, groups_next)


def gn_conv3d_train_h(x, gamma, beta, scale_shift, groups, act, eps, weight, bias, padding, residual=None, want_stats=False, tap=False,
                      out_half=False):
    """``Block.forward`` of a low-precision training step as one autograd node (``_GnActConvHFn``); ``tap`` as in ``groupnorm_act``;
    ``out_half``: the output may leave in the operand type (it only feeds the next Block's GroupNorm).  None when not in such a step or
    the shape is not taken by the 16-bit-input kernels (the caller then runs ``groupnorm_act`` + ``conv3d``)."""
    x_half = x.dtype != torch.float32
    if _lp_backward(lp_mode()) is None or not torch.is_grad_enabled() or x.dim() != 5 or isinstance(scale_shift, SSView) or _NO_TRAIN_FUSE:
        assert not x_half
        return None
    B, D, H, W, C = x.shape
    Cout, Cin, kd, kh, kw = weight.shape
    padding = tuple(int(p) for p in ((padding,) * 3 if isinstance(padding, int) else padding))
    if Cin != C or not _train_h_geo_ok(B, D, H, W, C, Cout, (kd, kh, kw), padding, groups):
        if x_half:
            raise RuntimeError("gn_conv3d_train_h: a 16-bit block output reached a conv that does not take 16-bit input")
        return None
    geo = (B, D, H, W, C, Cout, kd, kh, kw, *padding, 0, 0, 0)
    bpad = (kd - 1 - padding[0], kh - 1 - padding[1], kw - 1 - padding[2])
    # a 16-bit output: statistics rows for its consumer, and this node's backward-data (a conv Cout -> Cin over the 16-bit gradient)
    yh = bool(out_half and want_stats and residual is None
              and _lib.query("diqt_conv3d_fwd_h_io16_supported", *geo, 1, 1)
              and _lib.query("diqt_conv3d_fwd_h_stats_blocks", *geo, 1, 1) > 0
              and _lib.query("diqt_conv3d_fwd_h_io16_supported", B, D, H, W, Cout, C, kd, kh, kw, *bpad, 0, 0, 0, 1, 0)
              and Cout % 8 == 0)
    use_tap = tap and x.requires_grad
    ss_grad = getattr(scale_shift, "_diqt_gradview", None)
    if scale_shift is not None and ss_grad is None and not scale_shift.is_contiguous():
        scale_shift = scale_shift.contiguous()
    holder = [] if want_stats else None
    out = _GnActConvHFn.apply(x, gamma, beta, scale_shift, groups, act, eps, getattr(x, "_diqt_stats", None), weight, bias, padding, residual,
                              holder, use_tap, ss_grad, yh)
    y, alias = out if use_tap else (out, x)
    if holder:
        y._diqt_stats = holder[0]
    assert not yh or holder
    return (y, alias) if tap else y


def groupnorm_act(x, gamma, beta, scale_shift=None, groups=8, act=ACT_MISH, eps=1e-5, tap=False):
    """act(GN(x) * (scale+1) + shift) with scale_shift = one [B, 2C] embedding (scale first).
    ``tap=True`` returns ``(y, x_alias)``: route x's other consumer through ``x_alias`` (see _GnActFn.forward)."""
    if not torch.is_grad_enabled() or isinstance(scale_shift, SSView):
        y = _GnActFn.apply(x, gamma, beta, scale_shift, groups, act, eps, getattr(x, "_diqt_stats", None))
        return (y, x) if tap else y
    holder = []
    use_tap = tap and x.requires_grad
    ss_grad = getattr(scale_shift, "_diqt_gradview", None)     # a block of the batched time-MLP output: its place in the shared gradient buffer
    if scale_shift is not None and ss_grad is None and not scale_shift.is_contiguous():
        scale_shift = scale_shift.contiguous()
    out = _GnActFn.apply(x, gamma, beta, scale_shift, groups, act, eps, getattr(x, "_diqt_stats", None), holder, use_tap, ss_grad)
    y, alias = out if use_tap else (out, x)
    if holder:
        y._diqt_gnctx = holder[0]           # read by conv3d on this exact tensor (Block: GN -> act -> conv)
    return (y, alias) if tap else y


def gn_conv3d(x, gamma, beta, scale_shift, groups, act, eps, weight, bias, padding, residual=None, extra_pad=(0, 0, 0), want_stats=False,
              split16=False):
    """Sampling path (no autograd, fp32): conv3d(act(GN(x) * (scale + 1) + shift)) as ONE conv launch -- the GroupNorm statistics
    (from the producer's column sums when x carries them) are folded into per-(batch, channel) coefficients by one tiny launch and
    ``conv_fwd9_kernel`` applies them to its input tiles while staging them (``diqt_conv3d_fwd_gn``).  Returns None when the shape is
    not taken (the caller then runs ``groupnorm_act`` + ``conv3d``).  ``split16``: ask for the three-product split on the fp16 matrix
    pipe instead -- the same coefficients, applied by the pass that splits x (``_conv_fwd_split16``); a launch it does not grant takes
    the route above; ``split16="fill"`` asks the route's fill plan first, ``split16="pair"`` its pair plan and then the fill plan
    (``_split16_plan``)."""
    if torch.is_grad_enabled() or lp_mode() is not None or x.dim() != 5:
        return None
    B, D, H, W, C = x.shape
    Cout, Cin, kd, kh, kw = weight.shape
    padding = tuple(int(p) for p in ((padding,) * 3 if isinstance(padding, int) else padding))
    extra_pad = tuple(int(p) for p in extra_pad)
    geo = (B, D, H, W, C, Cout, kd, kh, kw, *padding, *extra_pad)
    npk = sum(_packed_len(weight.shape, 0))
    # (the split route has its own planner: it also takes activations and shapes the GroupNorm-apply build of conv_fwd9_kernel does not)
    use_split = _split16_plan(geo, act, split16) is not None
    default_ok = bool(_lib.query("diqt_conv3d_fwd_gn_supported_pk", *geo, act, npk))
    if Cin != C or C % groups != 0 or not (use_split or default_ok):
        return None
    _chk(x, gamma, beta, weight, bias, residual, scale_shift.base if isinstance(scale_shift, SSView) else None)
    rows = D * H * W
    dev = x.device
    s = _stream()
    mean = torch.empty(B * groups, dtype=torch.float32, device=dev)
    rstd = torch.empty_like(mean)
    coef = torch.empty(2 * B * C, dtype=torch.float32, device=dev)
    scale = shift = None
    cs = 0
    if isinstance(scale_shift, SSView):
        assert scale_shift.width == 2 * C and scale_shift.base.shape[0] == B
        scale, cs = scale_shift.base.data_ptr() + 4 * scale_shift.off, scale_shift.base.shape[1]
        shift = scale + 4 * C
    elif scale_shift is not None:
        assert scale_shift.shape == (B, 2 * C) and scale_shift.stride(1) == 1 and scale_shift.is_cuda and scale_shift.dtype == torch.float32
        scale, shift, cs = scale_shift.data_ptr(), scale_shift.data_ptr() + 4 * C, scale_shift.stride(0)
    pre = getattr(x, "_diqt_stats", None)
    if pre is not None and pre.rows == rows and pre.partials.shape == (B, pre.nblk, 2, C):
        _lib.call("diqt_gn_coef_from_partials", pre.partials, pre.nblk, rows, gamma, beta, scale, shift, cs, mean, rstd, coef, B, C, groups,
                  float(eps), s)
    else:
        ws, n = _reduce_ws(B, C, dev)
        _lib.call("diqt_groupnorm_stats_coef", x, gamma, beta, scale, shift, cs, mean, rstd, coef, ws, n, B, rows, C, groups, float(eps), s)
    if use_split:
        y = _conv_fwd_split16(x, weight, bias, residual, padding, extra_pad, want_stats, coef, act, split16)
        if y is not None:
            return y
    if not default_ok:
        return None
    Do, Ho, Wo = D + 2 * padding[0] + extra_pad[0] - kd + 1, H + 2 * padding[1] + extra_pad[1] - kh + 1, W + 2 * padding[2] + extra_pad[2] - kw + 1
    y = torch.empty((B, Do, Ho, Wo, Cout), dtype=torch.float32, device=dev)
    if TIMER.enabled:
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
    n = _lib.query("diqt_conv3d_fwd_workspace_bytes_pk", *geo, npk)
    ws = _workspace(n, dev) if n else None
    stats = None
    if want_stats:
        # the rows this launch is granted (field 3 of its route): none where conv_fwd9_kernel splits K -- the consumer's GroupNorm then
        # reduces y itself (diqt_groupnorm_stats_coef)
        nblk = _lib.query("diqt_conv3d_fwd_route", *geo, npk, int(ws is not None), 1, 0, act, 3)
        if nblk > 0:
            stats = torch.empty((B, nblk, 2, Cout), dtype=torch.float32, device=dev)
            y._diqt_stats = ColStats(stats, nblk, Do * Ho * Wo)
    packed = _packed(weight, 0)
    assert packed.numel() == npk
    _lib.call("diqt_conv3d_fwd_gn_pk", x, packed, npk, bias, residual, y, stats, ws, n, coef, act, *geo, s)
    if TIMER.enabled:
        ev1.record()
        TIMER.records.append((ev0, ev1, 2.0 * B * Do * Ho * Wo * Cout * C * kd * kh * kw, "conv_fwd9_kernel", geo[:9]))
    return y


class _ActFn(Function):
    @staticmethod
    def forward(ctx, x, act):
        _chk(x)
        y = torch.empty_like(x)
        _lib.call("diqt_act_fwd", x, y, x.numel(), act, _stream())
        ctx.save_for_backward(x)
        ctx.act = act
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        dx = torch.empty_like(x)
        _lib.call("diqt_act_bwd", x, dy.contiguous(), dx, x.numel(), ctx.act, _stream())
        return dx, None


def activation(x, act):
    return _ActFn.apply(x.contiguous(), act)


def mish(x):
    return activation(x, ACT_MISH)


class _ChanLayerNormFn(Function):
    @staticmethod
    def forward(ctx, x, g, b, eps, res=None, tap=False):
        """tap: as _GnActFn.forward -- x comes back as a second output for its other consumer (the `+ x` of the block)."""
        _chk(x, g, b, res)
        ctx.tap = tap
        ctx.set_materialize_grads(False)
        C = x.shape[-1]
        rows = x.numel() // C
        y = torch.empty_like(x)
        mean = torch.empty(rows, dtype=torch.float32, device=x.device)
        rstd = torch.empty_like(mean)
        _lib.call("diqt_chan_layernorm_fwd_res", x, g, b, res, y, mean, rstd, rows, C, float(eps), _stream())
        ctx.save_for_backward(x, g, mean, rstd)
        ctx.has_bias = b is not None
        ctx.has_res = res is not None
        return (y, x) if tap else y

    @staticmethod
    def backward(ctx, dy, dtap=None):
        x, g, mean, rstd = ctx.saved_tensors
        if dy is None:
            return dtap, None, None, None, None, None
        C = x.shape[-1]
        rows = x.numel() // C
        dx = torch.empty_like(x)
        dg = torch.empty_like(g)
        db = torch.empty_like(g) if ctx.has_bias else None
        ws, n = _reduce_ws(1, C, x.device)
        dy = dy.contiguous()
        if db is not None and C % 4 == 0 and dy.data_ptr() % 16:
            dy = dy.clone()          # a contiguous view at an odd offset: the bias-gradient reduction loads dy 16 bytes per lane
        if dtap is not None:
            dtap = dtap.contiguous()
        _lib.call("diqt_chan_layernorm_bwd_ex", x, dy, dtap, g, mean, rstd, dx, dg, db, ws, n, rows, C, _stream())
        return dx, dg, db, None, (dy if ctx.has_res else None), None


def chan_layernorm(x, g, eps=1e-5, bias=None, residual=None, tap=False):
    """LayerNorm over the channel (last) axis; g (and the optional bias) are any tensors with C elements.  ``residual`` (same shape as
    x) is added to the result in the same pass.  ``tap=True`` returns ``(y, x_alias)`` (see _GnActFn.forward)."""
    if residual is not None:
        assert residual.shape == x.shape, (tuple(residual.shape), tuple(x.shape))
        residual = residual.contiguous()
    xc = x.contiguous()
    use_tap = tap and torch.is_grad_enabled() and xc.requires_grad
    out = _ChanLayerNormFn.apply(xc, g.reshape(-1), bias.reshape(-1) if bias is not None else None, eps, residual, use_tap)
    y, alias = out if use_tap else (out, x)
    y = y.view(x.shape)
    return (y, alias.view(x.shape)) if tap else y


# --------------------------------------------------------------------------------------------
# learned sinusoidal embedding
# --------------------------------------------------------------------------------------------
class _LearnedSinuFn(Function):
    @staticmethod
    def forward(ctx, t, w):
        _chk(t, w)
        B, half = t.shape[0], w.shape[0]
        out = torch.empty((B, 2 * half + 1), dtype=torch.float32, device=t.device)
        _lib.call("diqt_learned_sinu_fwd", t, w, out, B, half, _stream())
        ctx.save_for_backward(t, w)
        return out

    @staticmethod
    def backward(ctx, dout):
        t, w = ctx.saved_tensors
        dw = torch.empty_like(w)
        _lib.call("diqt_learned_sinu_bwd", t, w, dout.contiguous(), dw, t.shape[0], w.shape[0], _stream())
        return None, dw


def learned_sinusoidal(t, w):
    return _LearnedSinuFn.apply(t.contiguous(), w)


# --------------------------------------------------------------------------------------------
# squeeze-excite gate + residual (one autograd node for pool -> MLP -> h*gate + res)
# --------------------------------------------------------------------------------------------
class _SEResidualFn(Function):
    @staticmethod
    def forward(ctx, h, w1, w2, res, pre=None, stats_out=None):
        h_half = h.dtype != torch.float32      # block2's conv output in the operand type (autocast sampling / low-precision training)
        hty = 0 if not h_half else (2 if h.dtype == torch.bfloat16 else 1)
        _chk(None if h_half else h, w1, w2, res)
        B, C = h.shape[0], h.shape[-1]
        rows = h.numel() // (B * C)
        Cr = w1.shape[0]
        dev = h.device
        s = _stream()
        pooled = torch.empty((B, C), dtype=torch.float32, device=dev)
        hidden = torch.empty((B, Cr), dtype=torch.float32, device=dev)
        gate = torch.empty((B, C), dtype=torch.float32, device=dev)
        fused = 256 % min(C, 256) == 0 and (C <= 256 or C % 256 == 0)
        if fused and pre is not None and pre.rows == rows and pre.partials.shape == (B, pre.nblk, 2, C):
            # channel means from the producing conv's per-tile column sums + the two-layer gate MLP in ONE launch
            _lib.call("diqt_se_pool_mlp_fwd", pre.partials, pre.nblk, rows, pooled, w1, w2, hidden, gate, B, C, Cr, s)
        else:
            if pre is not None and pre.rows == rows and pre.partials.shape == (B, pre.nblk, 2, C):
                _lib.call("diqt_channel_mean_from_partials", pre.partials, pooled, B, pre.nblk, rows, C, s)
            else:
                assert not h_half, "a 16-bit conv output must carry its column sums (the SE squeeze reads them)"
                ws, n = _reduce_ws(B, C, dev)
                _lib.call("diqt_channel_mean", h, pooled, ws, n, B, rows, C, s)
            _lib.call("diqt_se_pool_mlp_fwd", None, 0, 0, pooled, w1, w2, hidden, gate, B, C, Cr, s)
        y = torch.empty(h.shape, dtype=torch.float32, device=dev)
        nblk = _lib.query("diqt_gate_residual_stats_blocks", rows, C) if stats_out is not None else 0
        if nblk > 0:
            # the block's output feeds the next block's first GroupNorm: its per-workgroup column sums ride along (no statistics pass)
            stats = torch.empty((B, nblk, 2, C), dtype=torch.float32, device=dev)
            if h_half:
                _lib.call("diqt_gate_residual_fwd_stats_h", h, gate, res, y, stats, B, rows, C, hty, s)
            else:
                _lib.call("diqt_gate_residual_fwd_stats", h, gate, res, y, stats, B, rows, C, s)
            stats_out.append(ColStats(stats, nblk, rows))
        elif h_half:
            _lib.call("diqt_gate_residual_fwd_h", h, gate, res, None, 0.0, y, B, rows, C, hty, 0, s)
        else:
            _lib.call("diqt_gate_residual_fwd", h, gate, res, None, 0.0, y, B, rows, C, s)
        ctx.save_for_backward(h, w1, w2, pooled, hidden, gate)
        ctx.has_res = res is not None
        ctx.hty = hty
        return y

    @staticmethod
    def backward(ctx, dy):
        h, w1, w2, pooled, hidden, gate = ctx.saved_tensors
        dy = dy.contiguous()
        B, C = h.shape[0], h.shape[-1]
        rows = h.numel() // (B * C)
        Cr = w1.shape[0]
        dev = h.device
        s = _stream()
        dgate = torch.empty_like(gate)
        ws, n = _reduce_ws(B, C, dev)
        if ctx.hty:
            _lib.call("diqt_gate_residual_bwd_h", h, dy, dgate, ws, n, B, rows, C, ctx.hty, s)
        else:
            _lib.call("diqt_gate_residual_bwd", h, dy, dgate, ws, n, B, rows, C, s)
        dpooled = torch.empty_like(pooled)
        dw1, dw2 = torch.empty_like(w1), torch.empty_like(w2)
        scratch = torch.empty(B * (C + Cr), dtype=torch.float32, device=dev)
        _lib.call("diqt_se_mlp_bwd", pooled, w1, w2, hidden, gate, dgate, dpooled, dw1, dw2, scratch, B, C, Cr, s)
        dh = torch.empty_like(h)                       # (a 16-bit h gets a 16-bit gradient: only 16-bit-operand conv kernels read it)
        if ctx.hty:
            _lib.call("diqt_gate_residual_fwd_h", dy, gate, None, dpooled, 1.0 / rows, dh, B, rows, C, 0, ctx.hty, s)
        else:
            _lib.call("diqt_gate_residual_fwd", dy, gate, None, dpooled, 1.0 / rows, dh, B, rows, C, s)
        return dh, dw1, dw2, (dy if ctx.has_res else None), None, None


def se_gate_residual(h, w1, w2, res=None):
    """h * sigmoid(relu(mean(h) w1^T) w2^T) + res."""
    holder = []
    y = _SEResidualFn.apply(h, w1, w2, res, getattr(h, "_diqt_stats", None), holder)
    if holder:
        y._diqt_stats = holder[0]           # consumed by groupnorm_act on this exact tensor
    return y


class _AddFn(Function):
    """a + b through the gate kernel with unit gates is wasteful; use axpby3 with unit coefficients."""
    @staticmethod
    def forward(ctx, a, b):
        _chk(a, b)
        out = torch.empty_like(a)
        one = _ones(1, a.device)
        _lib.call("diqt_axpby3", a.view(1, -1), b.view(1, -1), None, one, one, None, 0.0, 0.0, 0, out, 1, a.numel(),
                  _stream())
        return out

    @staticmethod
    def backward(ctx, d):
        return d, d


_ONES = {}


def _ones(n, device):
    key = (n, device.index)
    t = _ONES.get(key)
    if t is None:
        t = torch.ones(n, dtype=torch.float32, device=device)
        _ONES[key] = t
    return t


def add(a, b):
    return _AddFn.apply(a.contiguous(), b.contiguous())


# --------------------------------------------------------------------------------------------
# data movement
# --------------------------------------------------------------------------------------------
class _SpaceToDepthFn(Function):
    @staticmethod
    def forward(ctx, x):
        _chk(x)
        B, D2, H2, W2, C = x.shape
        y = torch.empty((B, D2 // 2, H2 // 2, W2 // 2, C * 8), dtype=torch.float32, device=x.device)
        _lib.call("diqt_space_to_depth2", x, y, B, D2 // 2, H2 // 2, W2 // 2, C, _stream())
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = dy.contiguous()
        B, D, H, W, C8 = dy.shape
        dx = torch.empty((B, 2 * D, 2 * H, 2 * W, C8 // 8), dtype=torch.float32, device=dy.device)
        _lib.call("diqt_depth_to_space2", dy, dx, B, D, H, W, C8 // 8, _stream())
        return dx


class _DepthToSpaceFn(Function):
    @staticmethod
    def forward(ctx, x):
        _chk(x)
        B, D, H, W, C8 = x.shape
        y = torch.empty((B, 2 * D, 2 * H, 2 * W, C8 // 8), dtype=torch.float32, device=x.device)
        _lib.call("diqt_depth_to_space2", x, y, B, D, H, W, C8 // 8, _stream())
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = dy.contiguous()
        B, D2, H2, W2, C = dy.shape
        dx = torch.empty((B, D2 // 2, H2 // 2, W2 // 2, C * 8), dtype=torch.float32, device=dy.device)
        _lib.call("diqt_space_to_depth2", dy, dx, B, D2 // 2, H2 // 2, W2 // 2, C, _stream())
        return dx


def space_to_depth(x):
    return _SpaceToDepthFn.apply(x)


def depth_to_space(x):
    return _DepthToSpaceFn.apply(x)


class _ConcatFn(Function):
    @staticmethod
    def forward(ctx, a, b, fa, fb):
        _chk(a, b)
        Ca, Cb = a.shape[-1], b.shape[-1]
        rows = a.numel() // Ca
        y = torch.empty((*a.shape[:-1], Ca + Cb), dtype=torch.float32, device=a.device)
        if fa == 1.0 and fb == 1.0 and (Ca % 4 or Cb % 4):
            _lib.call("diqt_concat_channels", a, Ca, b, Cb, y, rows, _stream())
        else:
            _lib.call("diqt_concat_channels_scaled", a, Ca, b, Cb, fa, fb, y, rows, _stream())
        ctx.shapes = (a.shape, b.shape)
        ctx.f = (fa, fb)
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = dy.contiguous()
        sa, sb = ctx.shapes
        da = torch.empty(sa, dtype=torch.float32, device=dy.device) if ctx.needs_input_grad[0] else None
        db = torch.empty(sb, dtype=torch.float32, device=dy.device) if ctx.needs_input_grad[1] else None
        if da is not None or db is not None:
            _lib.call("diqt_split_channels_scaled", dy, da, sa[-1], db, sb[-1], ctx.f[0], ctx.f[1], dy.numel() // dy.shape[-1], _stream())
        return da, db, None, None


def concat_channels(a, b, scale_a=1.0, scale_b=1.0, want_stats=False):
    """cat(scale_a * a, scale_b * b) over the last axis in one pass (the scaled skip connections).  ``want_stats`` (sampling path): the
    pass also writes the column sums of its output for the GroupNorm that consumes it (``_diqt_stats``), when the shape is taken."""
    if want_stats and not torch.is_grad_enabled() and a.dim() >= 3 and a.dtype == torch.float32 and b.dtype == torch.float32:
        a, b = a.contiguous(), b.contiguous()
        Ca, Cb, B = a.shape[-1], b.shape[-1], a.shape[0]
        rows = a.numel() // (B * Ca)
        nblk = _lib.query("diqt_concat_channels_stats_blocks", Ca, Cb, rows)
        if nblk > 0 and b.shape[:-1] == a.shape[:-1]:
            _chk(a, b)
            y = torch.empty((*a.shape[:-1], Ca + Cb), dtype=torch.float32, device=a.device)
            stats = torch.empty((B, nblk, 2, Ca + Cb), dtype=torch.float32, device=a.device)
            _lib.call("diqt_concat_channels_stats", a, Ca, b, Cb, float(scale_a), float(scale_b), y, B, rows, stats, _stream())
            y._diqt_stats = ColStats(stats, nblk, rows)
            return y
    return _ConcatFn.apply(a.contiguous(), b.contiguous(), float(scale_a), float(scale_b))


class _SplitFn(Function):
    @staticmethod
    def forward(ctx, x, ca):
        _chk(x)
        C = x.shape[-1]
        rows = x.numel() // C
        a = torch.empty((*x.shape[:-1], ca), dtype=torch.float32, device=x.device)
        b = torch.empty((*x.shape[:-1], C - ca), dtype=torch.float32, device=x.device)
        _lib.call("diqt_split_channels", x, a, ca, b, C - ca, rows, _stream())
        ctx.set_materialize_grads(False)
        ctx.cfg = (ca, C - ca, a.shape, b.shape)
        return a, b

    @staticmethod
    def backward(ctx, da, db):
        ca, cb, sa, sb = ctx.cfg
        ref = da if da is not None else db
        if ref is None:
            return None, None
        da = da.contiguous() if da is not None else torch.zeros(sa, dtype=torch.float32, device=ref.device)
        db = db.contiguous() if db is not None else torch.zeros(sb, dtype=torch.float32, device=ref.device)
        dx = torch.empty((*sa[:-1], ca + cb), dtype=torch.float32, device=ref.device)
        _lib.call("diqt_concat_channels", da, ca, db, cb, dx, da.numel() // ca, _stream())
        return dx, None


def split_channels(x, ca):
    """(x[..., :ca], x[..., ca:]) as two contiguous tensors (the inverse of ``concat_channels``)."""
    return _SplitFn.apply(x.contiguous(), int(ca))


class _SubvolumeFn(Function):
    """merged volume [1,S,S,S,C] -> sub-volume batch [f^3,A',A',A',C] (halo>0: zero-padded overlap)."""
    @staticmethod
    def forward(ctx, vol, f, A, halo):
        _chk(vol)
        C = vol.shape[-1]
        Ap = A + 2 * halo
        sub = torch.empty((f ** 3, Ap, Ap, Ap, C), dtype=torch.float32, device=vol.device)
        _lib.call("diqt_subvolume_gather", vol, sub, f, A, C, halo, _stream())
        ctx.cfg = (f, A, C, halo, vol.shape)
        return sub

    @staticmethod
    def backward(ctx, dsub):
        f, A, C, halo, shape = ctx.cfg
        dvol = torch.zeros(shape, dtype=torch.float32, device=dsub.device)
        _lib.call("diqt_subvolume_scatter", dsub.contiguous(), dvol, f, A, C, halo, 1 if halo > 0 else 0, _stream())
        return dvol, None, None, None


class _MergeFn(Function):
    @staticmethod
    def forward(ctx, sub, f):
        _chk(sub)
        n, A, _, _, C = sub.shape
        vol = torch.empty((1, f * A, f * A, f * A, C), dtype=torch.float32, device=sub.device)
        _lib.call("diqt_subvolume_scatter", sub, vol, f, A, C, 0, 0, _stream())
        ctx.cfg = (f, A, C)
        return vol

    @staticmethod
    def backward(ctx, dvol):
        f, A, C = ctx.cfg
        dsub = torch.empty((f ** 3, A, A, A, C), dtype=torch.float32, device=dvol.device)
        _lib.call("diqt_subvolume_gather", dvol.contiguous(), dsub, f, A, C, 0, _stream())
        return dsub, None


class _TrilinearUpFn(Function):
    @staticmethod
    def forward(ctx, x, scale):
        _chk(x)
        B, D, H, W, C = x.shape
        y = torch.empty((B, D * scale, H * scale, W * scale, C), dtype=torch.float32, device=x.device)
        _lib.call("diqt_trilinear_up_fwd", x, y, B, D, H, W, C, scale, _stream())
        ctx.cfg = (B, D, H, W, C, scale)
        return y

    @staticmethod
    def backward(ctx, dy):
        B, D, H, W, C, scale = ctx.cfg
        dx = torch.zeros((B, D, H, W, C), dtype=torch.float32, device=dy.device)
        _lib.call("diqt_trilinear_up_bwd", dy.contiguous(), dx, B, D, H, W, C, scale, _stream())
        return dx, None


def trilinear_upsample(x, scale):
    """nn.Upsample(scale_factor=scale, mode='trilinear', align_corners=True) on channels-last x."""
    return _TrilinearUpFn.apply(x.contiguous(), int(scale))


def split_volume(vol, f, A, halo=0):
    return _SubvolumeFn.apply(vol.contiguous(), f, A, halo)


def merge_volume(sub, f):
    return _MergeFn.apply(sub.contiguous(), f)


# --------------------------------------------------------------------------------------------
# attention pieces
# --------------------------------------------------------------------------------------------
class _SoftmaxFn(Function):
    @staticmethod
    def forward(ctx, x, outer, n, inner, scale):
        _chk(x)
        y = torch.empty_like(x)
        _lib.call("diqt_softmax_fwd", x, y, outer, n, inner, float(scale), _stream())
        ctx.save_for_backward(y)
        ctx.cfg = (outer, n, inner, float(scale))
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        dx = torch.empty_like(y)
        _lib.call("diqt_softmax_bwd", y, dy.contiguous(), dx, *ctx.cfg, _stream())
        return dx, None, None, None, None


def softmax(x, dim, scale=1.0):
    """scale * softmax(x, dim) for a contiguous x."""
    x = x.contiguous()
    dim = dim % x.dim()
    outer = 1
    for s in x.shape[:dim]:
        outer *= s
    inner = 1
    for s in x.shape[dim + 1:]:
        inner *= s
    return _SoftmaxFn.apply(x, outer, x.shape[dim], inner, scale)


def _bgemm_strided(A, Bm, C, g, M, N, K, tA, tB, sA, lda, sB, ldb, sC, ldc, alpha, oA=0, oB=0, oC=0):
    nws = _lib.query("diqt_bgemm_workspace_bytes", g, M, N, K)
    ws = _workspace(nws, A.device) if nws else None
    _lib.call("diqt_bgemm_ws", A.data_ptr() + 4 * oA, Bm.data_ptr() + 4 * oB, C.data_ptr() + 4 * oC, ws, nws, g, M, N, K, int(tA),
              int(tB), sA, sB, sC, lda, ldb, ldc, float(alpha), 0.0, _stream())


class _BmmStridedFn(Function):
    """C[g] = alpha * op(A[g]) op(B[g]) with explicit batch strides / leading dimensions / element offsets, so attention
    heads (and the k|v halves of a fused projection) are addressed inside channels-last tensors without copies.
    spec = (g, M, N, K, tA, tB, sA, lda, sB, ldb, sC, ldc, alpha, out_shape[, offA, offB])."""
    @staticmethod
    def forward(ctx, A, Bm, spec):
        _chk(A, Bm)
        g, M, N, K, tA, tB, sA, lda, sB, ldb, sC, ldc, alpha, out_shape = spec[:14]
        oA, oB = (spec[14], spec[15]) if len(spec) > 14 else (0, 0)
        C = torch.empty(out_shape, dtype=torch.float32, device=A.device)
        _bgemm_strided(A, Bm, C, g, M, N, K, tA, tB, sA, lda, sB, ldb, sC, ldc, alpha, oA, oB)
        ctx.save_for_backward(A, Bm)
        ctx.spec = spec
        return C

    @staticmethod
    def backward(ctx, dC):
        A, Bm = ctx.saved_tensors
        spec = ctx.spec
        g, M, N, K, tA, tB, sA, lda, sB, ldb, sC, ldc, alpha, _ = spec[:14]
        oA, oB = (spec[14], spec[15]) if len(spec) > 14 else (0, 0)
        dC = dC.contiguous()
        dA = dB = None
        # operands addressed through offsets / interleaved strides cover only part of their tensor: zero-fill then
        partial_A = oA != 0 or len(spec) > 14
        if ctx.needs_input_grad[0]:
            dA = torch.zeros_like(A) if partial_A else torch.empty_like(A)
            if not tA:   # dA[M,K] = a * dC[M,N] op(B)^T
                _bgemm_strided(dC, Bm, dA, g, M, K, N, False, not tB, sC, ldc, sB, ldb, sA, lda, alpha, 0, oB, oA)
            else:        # A stored [K,M]: dA[K,M] = a * op(B)[K,N] dC^T[N,M]
                _bgemm_strided(Bm, dC, dA, g, K, M, N, tB, True, sB, ldb, sC, ldc, sA, lda, alpha, oB, 0, oA)
        if ctx.needs_input_grad[1]:
            dB = torch.zeros_like(Bm) if partial_A else torch.empty_like(Bm)
            if not tB:   # dB[K,N] = a * op(A)^T[K,M] dC[M,N]
                _bgemm_strided(A, dC, dB, g, K, N, M, not tA, False, sA, lda, sC, ldc, sB, ldb, alpha, oA, 0, oB)
            else:        # B stored [N,K]: dB[N,K] = a * dC^T[N,M] op(A)[M,K]
                _bgemm_strided(dC, A, dB, g, N, K, M, True, tA, sC, ldc, sA, lda, sB, ldb, alpha, 0, oA, oB)
        return dA, dB, None


def bmm_strided(A, Bm, spec):
    return _BmmStridedFn.apply(A.contiguous(), Bm.contiguous(), spec)


def _bgemm_raw(A, Bm, tA, tB, alpha=1.0):
    """A:[g,M,K] (or [g,K,M] if tA), B:[g,K,N] (or [g,N,K] if tB) -> [g,M,N]; contiguous inputs."""
    g = A.shape[0]
    M, K = (A.shape[2], A.shape[1]) if tA else (A.shape[1], A.shape[2])
    N = Bm.shape[1] if tB else Bm.shape[2]
    C = torch.empty((g, M, N), dtype=torch.float32, device=A.device)
    nws = _lib.query("diqt_bgemm_workspace_bytes", g, M, N, K)
    ws = _workspace(nws, A.device) if nws else None
    _lib.call("diqt_bgemm_ws", A, Bm, C, ws, nws, g, M, N, K, int(tA), int(tB), A.shape[1] * A.shape[2], Bm.shape[1] * Bm.shape[2],
              M * N, A.shape[2], Bm.shape[2], N, float(alpha), 0.0, _stream())
    return C


class _BmmFn(Function):
    @staticmethod
    def forward(ctx, A, Bm, tA, tB, alpha):
        _chk(A, Bm)
        ctx.save_for_backward(A, Bm)
        ctx.cfg = (tA, tB, alpha)
        return _bgemm_raw(A, Bm, tA, tB, alpha)

    @staticmethod
    def backward(ctx, dC):
        A, Bm = ctx.saved_tensors
        tA, tB, alpha = ctx.cfg
        dC = dC.contiguous()
        dA = dB = None
        # C = a * op(A) op(B)
        if ctx.needs_input_grad[0]:
            if not tA:   # dA = a * dC op(B)^T
                dA = _bgemm_raw(dC, Bm, False, not tB, alpha)
            else:        # dA^T = a*dC op(B)^T -> dA = a * op(B) dC^T
                dA = _bgemm_raw(Bm, dC, tB, True, alpha)
        if ctx.needs_input_grad[1]:
            if not tB:   # dB = a * op(A)^T dC
                dB = _bgemm_raw(A, dC, not tA, False, alpha)
            else:        # dB = a * dC^T op(A)
                dB = _bgemm_raw(dC, A, True, tA, alpha)
        return dA, dB, None, None, None


class _WeightedPoolFn(Function):
    """out[b, c] = sum_n w[b, n] x[b, n, c] (GlobalContext pooling): one column-reduction pass over x instead of a
    1-row GEMM with K = n; the gradients are two thin GEMMs (dw = x dout, dx = w (x) dout)."""
    @staticmethod
    def forward(ctx, w, x):
        _chk(w, x)
        B, n, C = x.shape
        out = torch.empty((B, C), dtype=torch.float32, device=x.device)
        ws, nws = _reduce_ws(B, C, x.device)
        _lib.call("diqt_weighted_colsum", x, w, out, ws, nws, B, n, C, _stream())
        ctx.save_for_backward(w, x)
        return out

    @staticmethod
    def backward(ctx, dout):
        w, x = ctx.saved_tensors
        B, n, C = x.shape
        dout = dout.contiguous()
        dw = dx = None
        if ctx.needs_input_grad[0]:
            dw = _bgemm_raw(x, dout.reshape(B, C, 1), False, False).reshape(B, n)
        if ctx.needs_input_grad[1]:
            dx = _bgemm_raw(w.reshape(B, n, 1), dout.reshape(B, 1, C), False, False)
        return dw, dx


def softmax_pool_nograd(x, w):
    """GlobalContext pooling in one pass (sampling path): x[B, n, C], w[C] -> pooled[B, C] = sum_n softmax_n(x . w)[n] x[n]; None when
    the shape is not taken or autograd is recording."""
    if torch.is_grad_enabled():
        return None
    B, n, C = x.shape
    if not _lib.query("diqt_softmax_pool_supported", B, n, C):
        return None
    x, w = x.contiguous(), w.contiguous()
    _chk(x, w)
    pooled = torch.empty((B, C), dtype=torch.float32, device=x.device)
    ws, nb = _reduce_ws(B, C, x.device)
    _lib.call("diqt_softmax_pool", x, w, pooled, ws, nb, B, n, C, _stream())
    return pooled


def weighted_pool(w, x):
    """w: [B, n] weights, x: [B, n, C] -> [B, C]"""
    return _WeightedPoolFn.apply(w.contiguous(), x.contiguous())


def bmm(A, Bm, transA=False, transB=False, alpha=1.0):
    return _BmmFn.apply(A.contiguous(), Bm.contiguous(), bool(transA), bool(transB), float(alpha))


class _ShuffleNdFn(Function):
    @staticmethod
    def forward(ctx, x, factors, to_space):
        _chk(x)
        sd, sh, sw = factors
        S = sd * sh * sw
        if to_space:
            B, D, H, W, CS = x.shape
            C = CS // S
            y = torch.empty((B, D * sd, H * sh, W * sw, C), dtype=torch.float32, device=x.device)
            _lib.call("diqt_depth_to_space_nd", x, y, B, D, H, W, C, sd, sh, sw, _stream())
        else:
            B, D2, H2, W2, C = x.shape
            D, H, W = D2 // sd, H2 // sh, W2 // sw
            y = torch.empty((B, D, H, W, C * S), dtype=torch.float32, device=x.device)
            _lib.call("diqt_space_to_depth_nd", x, y, B, D, H, W, C, sd, sh, sw, _stream())
        ctx.cfg = (factors, to_space)
        return y

    @staticmethod
    def backward(ctx, dy):
        factors, to_space = ctx.cfg
        return _ShuffleNdFn.apply(dy.contiguous(), factors, not to_space), None, None


def space_to_depth_nd(x, factors):
    """'b (d sd) (h sh) (w sw) c -> b d h w (c sd sh sw)' for factors in {1,2}."""
    return _ShuffleNdFn.apply(x.contiguous(), tuple(factors), False)


def depth_to_space_nd(x, factors):
    return _ShuffleNdFn.apply(x.contiguous(), tuple(factors), True)


class _TransposeMidFn(Function):
    @staticmethod
    def forward(ctx, x):
        _chk(x)
        A, M, N, C = x.shape
        y = torch.empty((A, N, M, C), dtype=torch.float32, device=x.device)
        _lib.call("diqt_transpose_mid", x, y, A, M, N, C, _stream())
        return y

    @staticmethod
    def backward(ctx, dy):
        return _TransposeMidFn.apply(dy.contiguous())


def transpose_mid(x):
    """[A, M, N, C] -> [A, N, M, C]."""
    return _TransposeMidFn.apply(x.contiguous())


class _NearestResizeFn(Function):
    @staticmethod
    def forward(ctx, x, size):
        _chk(x)
        B, D, H, W, C = x.shape
        Do, Ho, Wo = size
        y = torch.empty((B, Do, Ho, Wo, C), dtype=torch.float32, device=x.device)
        _lib.call("diqt_nearest_resize", x, y, B, D, H, W, C, Do, Ho, Wo, _stream())
        ctx.cfg = (B, D, H, W, C, Do, Ho, Wo)
        return y

    @staticmethod
    def backward(ctx, dy):
        B, D, H, W, C, Do, Ho, Wo = ctx.cfg
        dx = torch.empty((B, D, H, W, C), dtype=torch.float32, device=dy.device)
        _lib.call("diqt_nearest_resize_bwd", dy.contiguous(), dx, B, D, H, W, C, Do, Ho, Wo, _stream())       # whole-number up-scaling only
        return dx, None


def nearest_resize(x, size):
    """F.interpolate(mode='nearest') of a channels-last volume to (Do, Ho, Wo).  Differentiable for whole-number up-scaling factors
    (the feature maps of UpsampleCombiner); other sizes are data preparation only."""
    return _NearestResizeFn.apply(x.contiguous(), tuple(int(v) for v in size))


class _L2NormRowsFn(Function):
    """F.normalize(dim=-1) of the d-wide rows of x[..., stride] taken at column offset ``off`` (rows ``stride`` floats apart)."""
    @staticmethod
    def forward(ctx, x, off, d):
        _chk(x)
        stride = x.shape[-1]
        rows = x.numel() // stride
        y = torch.empty(x.shape[:-1] + (d,), dtype=torch.float32, device=x.device)
        inv = torch.empty(rows, dtype=torch.float32, device=x.device)
        _lib.call("diqt_l2norm_rows_fwd", x.data_ptr() + 4 * off, y, inv, rows, d, stride, d, _stream())
        ctx.save_for_backward(y, inv)
        ctx.cfg = (off, d, stride, rows, tuple(x.shape))
        return y

    @staticmethod
    def backward(ctx, dy):
        y, inv = ctx.saved_tensors
        off, d, stride, rows, shape = ctx.cfg
        dx = torch.zeros(shape, dtype=torch.float32, device=dy.device) if d != stride else torch.empty(shape, dtype=torch.float32, device=dy.device)
        _lib.call("diqt_l2norm_rows_bwd", y, dy.contiguous(), inv, dx.data_ptr() + 4 * off, rows, d, d, stride, _stream())
        return dx, None, None


def l2norm_rows(x, off=0, d=None):
    """l2-normalised copy of columns [off, off + d) of every row of x[..., C] (cosine-sim attention: q heads, the k half of k|v rows)."""
    d = x.shape[-1] if d is None else d
    return _L2NormRowsFn.apply(x.contiguous(), int(off), int(d))


class _AttnSoftmaxFn(Function):
    @staticmethod
    def forward(ctx, sim, rel, null_bias, n, h, n_extra, n_self, causal):
        _chk(sim, rel, null_bias)
        G = sim.numel() // (n * h * (n_extra + n_self))
        p = torch.empty_like(sim)
        _lib.call("diqt_attn_softmax_fwd", sim, rel, null_bias, p, G, n, h, n_extra, n_self, int(causal), _stream())
        ctx.save_for_backward(p)
        ctx.cfg = (G, n, h, n_extra, n_self, int(causal), rel is not None, null_bias is not None)
        ctx.shapes = (rel.shape if rel is not None else None, null_bias.shape if null_bias is not None else None)
        return p

    @staticmethod
    def backward(ctx, dp):
        (p,) = ctx.saved_tensors
        G, n, h, n_extra, n_self, causal, has_rel, has_null = ctx.cfg
        dsim = torch.empty_like(p)
        drel = torch.zeros(ctx.shapes[0], dtype=torch.float32, device=p.device) if has_rel else None
        dnull = torch.zeros(ctx.shapes[1], dtype=torch.float32, device=p.device) if has_null else None
        nws = _lib.query("diqt_attn_softmax_bwd_workspace_bytes", G, n, h, n_extra, n_self)
        ws = _workspace(nws, p.device) if nws else None
        _lib.call("diqt_attn_softmax_bwd_ws", p, dp.contiguous(), dsim, drel, dnull, ws, nws, G, n, h, n_extra, n_self, causal,
                  _stream())
        return dsim, drel, dnull, None, None, None, None, None


def mqa_attention_nograd(q, kv_ext, rel, null_bias, n, h, d, n_extra, n_self, causal, scale):
    """Fused multi-query attention forward (no autograd: sampling path).  q: [G, n, h*d]; kv_ext: [G, n_extra + n_self, 2d]."""
    _chk(q, kv_ext, rel, null_bias)
    G = q.shape[0]
    out = torch.empty((G, n, h * d), dtype=torch.float32, device=q.device)
    lp = lp_mode()
    if lp is not None:          # autocast: q k^T and p v on the fp16 / bf16 MFMA, soft-max statistics in fp32
        kv_h = torch.empty(kv_ext.shape, dtype=torch.int16, device=q.device)
        _lib.call("diqt_cast_to_h", kv_ext, kv_h, kv_ext.numel(), lp, _stream())
        _lib.call("diqt_mqa_attention_fwd_h", q, kv_h, rel, null_bias, out, G, n, h, d, n_extra, n_self, int(causal), float(scale),
                  lp, 1, _stream())
        return out
    _lib.call("diqt_mqa_attention_fwd", q, kv_ext, rel, null_bias, out, G, n, h, d, n_extra, n_self, int(causal), float(scale),
              _stream())
    return out


def mqa_attention_frames_nograd(q, kv, null_kv, rel, null_bias, h, d, causal, scale):
    """The temporal attention of the pseudo-3D U-Net in place (sampling path, fp32): q[B, F, P, h*d], kv[B, F, P, 2d] channels-last,
    sequences = (b, pixel), tokens = frames, ``null_kv``[2d] the extra key / value.  Returns out[B, F, P, h*d] -- no transposes, no
    concatenated copy of kv."""
    _chk(q, kv, null_kv, rel, null_bias)
    B, F, P, _ = q.shape
    out = torch.empty_like(q)
    _lib.call("diqt_mqa_attention_fwd_frames", q, kv, null_kv, rel, null_bias, out, B, F, P, h, d, int(causal), float(scale), _stream())
    return out


def temporal_attention_h_ok(B, F, P, C, h, d):
    return bool(_lib.query("diqt_temporal_attention_h_supported", B, F, P, C, h, d))


def pack_temporal_attention_h(to_q_w, to_kv_w, to_out_w, h, d, scale, lp):
    """16-bit operand copies of an Attention block's projections for diqt_temporal_attention_h: scale * to_q.weight [h d, C],
    to_kv.weight [2 d, C], and to_out.weight [C, h d] as [h][C][d] with a head's channels in the MFMA accumulator order."""
    dt = torch.bfloat16 if lp == 1 else torch.float16
    C = to_out_w.shape[0]
    wq = (to_q_w.detach().float() * scale).to(dt).contiguous()
    wkv = to_kv_w.detach().to(dt).contiguous()
    i = torch.arange(d, device=to_out_w.device)
    pos = 16 * (i >> 4) + 8 * ((i >> 2) & 1) + 4 * ((i >> 3) & 1) + (i & 3)
    wo = torch.empty((h, C, d), dtype=dt, device=to_out_w.device)
    wo[:, :, pos] = to_out_w.detach().reshape(C, h, d).permute(1, 0, 2).to(dt)
    return wq.view(torch.int16), wkv.view(torch.int16), wo.view(torch.int16)


def temporal_attention_h(x, norm_g, packed, out_g, null_kv, rel, null_bias, h, d, causal, eps, lp):
    """y = LayerNorm(Attention(LayerNorm(x)) W_o) + x over the frame axis of x[B, F, P, C], one kernel (sampling path, autocast)."""
    _chk(x, norm_g, out_g, null_kv, rel, null_bias)
    B, F, P, C = x.shape
    y = torch.empty_like(x)
    _lib.call("diqt_temporal_attention_h", x, norm_g, packed[0], packed[1], packed[2], out_g, null_kv, rel, null_bias, y, B, F, P, C,
              h, d, int(causal), float(eps), lp, 1, _stream())
    return y


class _MqaAttentionFn(Function):
    """Fused multi-query attention with autograd (training path): scores and probabilities never reach HBM, the backward
    recomputes them from the row log-sum-exp (diqt_mqa_attention_fwd_lse / diqt_mqa_attention_bwd)."""
    @staticmethod
    def forward(ctx, q, kv_ext, rel, null_bias, n, h, d, n_extra, n_self, causal, scale):
        _chk(q, kv_ext, rel, null_bias)
        G = q.shape[0]
        out = torch.empty((G, n, h * d), dtype=torch.float32, device=q.device)
        lse = torch.empty((G, n * h), dtype=torch.float32, device=q.device)
        _lib.call("diqt_mqa_attention_fwd_lse", q, kv_ext, rel, null_bias, out, lse, G, n, h, d, n_extra, n_self, int(causal),
                  float(scale), _stream())
        ctx.save_for_backward(q, kv_ext, rel, null_bias, out, lse)
        ctx.cfg = (G, n, h, d, n_extra, n_self, int(causal), float(scale))
        return out

    @staticmethod
    def backward(ctx, dout):
        q, kv_ext, rel, null_bias, out, lse = ctx.saved_tensors
        G, n, h, d, n_extra, n_self, causal, scale = ctx.cfg
        dout = dout.contiguous()
        dq = torch.empty_like(q)
        dkv = torch.empty_like(kv_ext)
        drel = torch.empty_like(rel) if rel is not None else None
        dnull = torch.empty_like(null_bias) if null_bias is not None else None
        nws = _lib.query("diqt_mqa_attention_bwd_workspace_bytes", G, n, h, d, n_extra, n_self, int(rel is not None))
        ws = _workspace(nws, q.device)
        _lib.call("diqt_mqa_attention_bwd", q, kv_ext, rel, null_bias, out, dout, lse, dq, dkv, drel, dnull, ws, nws, G, n, h, d,
                  n_extra, n_self, causal, scale, _stream())
        return dq, dkv, drel, dnull, None, None, None, None, None, None, None


def mqa_attention(q, kv_ext, rel, null_bias, n, h, d, n_extra, n_self, causal, scale):
    """Fused multi-query attention WITH autograd.  q: [G, n, h*d]; kv_ext: [G, n_extra + n_self, 2d]; rel: [2n-1, h] or None."""
    return _MqaAttentionFn.apply(q.contiguous(), kv_ext.contiguous(), rel.contiguous() if rel is not None else None,
                                 null_bias.contiguous() if null_bias is not None else None, n, h, d, n_extra, n_self, bool(causal),
                                 float(scale))


def mqa_attention_fused_ok(G, n, h, d, n_self, has_rel):
    """Shapes the fused training kernels take (otherwise: GEMM -> attn_softmax -> GEMM)."""
    return d in (32, 64) and G <= 65535 and h <= 64 and (not has_rel or 4 * (2 * n_self - 1) * h * 4 <= 24 * 1024)


def attn_softmax(sim, rel, null_bias, n, h, n_extra, n_self, causal):
    """softmax over keys of sim[G, n, h, n_extra + n_self] with T5-style relative bias table rel[2n-1, h] on the self
    keys, null_bias[h] on the null key (last extra key) and an optional causal mask (imagen_video.py:490-518)."""
    return _AttnSoftmaxFn.apply(sim.contiguous(), rel, null_bias, n, h, n_extra, n_self, bool(causal))


class _GateResidualFn(Function):
    """y = h * gate[b, c] + res  (GlobalContext gating + residual, imagen_video.py:768-770)."""
    @staticmethod
    def forward(ctx, h, gate, res):
        _chk(h, gate, res)
        B, C = h.shape[0], h.shape[-1]
        rows = h.numel() // (B * C)
        y = torch.empty_like(h)
        _lib.call("diqt_gate_residual_fwd", h, gate, res, None, 0.0, y, B, rows, C, _stream())
        ctx.save_for_backward(h, gate)
        ctx.has_res = res is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        h, gate = ctx.saved_tensors
        dy = dy.contiguous()
        B, C = h.shape[0], h.shape[-1]
        rows = h.numel() // (B * C)
        s = _stream()
        dgate = torch.empty_like(gate)
        ws, n = _reduce_ws(B, C, h.device)
        _lib.call("diqt_gate_residual_bwd", h, dy, dgate, ws, n, B, rows, C, s)
        dh = torch.empty_like(h)
        _lib.call("diqt_gate_residual_fwd", dy, gate, None, None, 0.0, dh, B, rows, C, s)
        return dh, dgate, (dy if ctx.has_res else None)


def gate_residual(h, gate, res=None):
    if not torch.is_grad_enabled() and res is not None:
        # sampling: a ResnetBlock's output usually feeds the next block's first GroupNorm -- its per-workgroup column sums ride along
        # (groupnorm_act / gn_conv3d read them from ``_diqt_stats``: no statistics pass over the tensor)
        h, gate = h.contiguous(), gate.contiguous()
        _chk(h, gate, res)
        B, C = h.shape[0], h.shape[-1]
        rows = h.numel() // (B * C)
        nblk = _lib.query("diqt_gate_residual_stats_blocks", rows, C)
        if nblk > 0:
            y = torch.empty_like(h)
            stats = torch.empty((B, nblk, 2, C), dtype=torch.float32, device=h.device)
            _lib.call("diqt_gate_residual_fwd_stats", h, gate, res, y, stats, B, rows, C, _stream())
            y._diqt_stats = ColStats(stats, nblk, rows)
            return y
    return _GateResidualFn.apply(h.contiguous(), gate.contiguous(), res)


class _ScaleFn(Function):
    @staticmethod
    def forward(ctx, x, alpha):
        _chk(x)
        out = torch.empty_like(x)
        c0 = torch.full((1,), float(alpha), dtype=torch.float32, device=x.device)
        _lib.call("diqt_axpby3", x, None, None, c0, None, None, 0.0, 0.0, 0, out, 1, x.numel(), _stream())
        ctx.alpha = float(alpha)
        return out

    @staticmethod
    def backward(ctx, d):
        return _ScaleFn.apply(d.contiguous(), ctx.alpha), None


def scale(x, alpha):
    return x if alpha == 1.0 else _ScaleFn.apply(x.contiguous(), alpha)


# --------------------------------------------------------------------------------------------
# diffusion math
# --------------------------------------------------------------------------------------------
def q_sample(x0, noise, alpha, sigma):
    """alpha[b]*x0 + sigma[b]*noise (no autograd: inputs are data)."""
    _chk(x0, noise, alpha, sigma)
    B = x0.shape[0]
    out = torch.empty_like(x0)
    _lib.call("diqt_q_sample", x0, noise, alpha, sigma, out, B, x0.numel() // B, _stream())
    return out


def ddpm_step(x_t, pred, noise, ca, cb, cn, lo, hi, clamp_mode):
    _chk(x_t, pred, noise, ca, cb, cn)
    B = x_t.shape[0]
    x_next, x0 = torch.empty_like(x_t), torch.empty_like(x_t)
    _lib.call("diqt_ddpm_step", x_t, pred, noise, ca, cb, cn, float(lo), float(hi), int(clamp_mode), x_next, x0, B,
              x_t.numel() // B, _stream())
    return x_next, x0


def abs_quantile(x, q):
    """torch.quantile(x.flatten(1).abs(), q, dim=-1) (linear interpolation) by radix select: [B] thresholds."""
    import numpy as np
    _chk(x)
    B = x.shape[0]
    per = x.numel() // B
    rank = np.float32(q) * np.float32(per - 1)             # the fp32 rank arithmetic of aten's quantile_compute
    k_lo = int(np.floor(rank))
    weight = float(np.float32(rank - np.float32(k_lo)))
    out = torch.empty(B, dtype=torch.float32, device=x.device)
    _lib.call("diqt_abs_quantile", x, out, B, per, k_lo, weight, _stream())
    return out


def dynamic_threshold(x0, s):
    """clamp(x0, -s[b], s[b]) / s[b]"""
    _chk(x0, s)
    B = x0.shape[0]
    out = torch.empty_like(x0)
    _lib.call("diqt_dynamic_threshold", x0, s, out, B, x0.numel() // B, _stream())
    return out


def mask_blend(x, y, mask):
    """mask ? y : x (mask: 0/1 float tensor of x's shape)"""
    _chk(x, y, mask)
    assert x.shape == y.shape == mask.shape
    out = torch.empty_like(x)
    _lib.call("diqt_mask_blend", x, y, mask, out, x.numel(), _stream())
    return out


def axpby3(a, b, c, c0, c1, c2, lo=0.0, hi=0.0, clamp_mode=0):
    _chk(a, b, c, c0, c1, c2)
    B = a.shape[0]
    out = torch.empty_like(a)
    _lib.call("diqt_axpby3", a, b, c, c0, c1, c2, float(lo), float(hi), int(clamp_mode), out, B, a.numel() // B,
              _stream())
    return out


class _MseClampFn(Function):
    @staticmethod
    def forward(ctx, pred, target, weight, lo, do_clamp, kind=0):
        _chk(pred, target, weight)
        B = pred.shape[0]
        per = pred.numel() // B
        partials = torch.empty(1024, dtype=torch.float32, device=pred.device)
        loss = torch.empty((), dtype=torch.float32, device=pred.device)
        clamped = torch.empty_like(pred)
        _lib.call("diqt_loss_clamp_fwd", pred, clamped, target, weight, float(lo), int(do_clamp), int(kind), partials, loss, B, per,
                  _stream())
        ctx.mark_non_differentiable(clamped)
        ctx.save_for_backward(clamped, target, weight)
        ctx.cfg = (float(lo), int(do_clamp), B, per, int(kind))
        return loss, clamped

    @staticmethod
    def backward(ctx, dloss, _dclamped):
        clamped, target, weight = ctx.saved_tensors
        lo, do_clamp, B, per, kind = ctx.cfg
        dpred = torch.empty_like(clamped)
        _lib.call("diqt_loss_clamp_bwd", clamped, target, weight, lo, do_clamp, kind, 1.0, dpred, B, per, _stream())
        return _ScaleByScalar.apply_raw(dpred, dloss), None, None, None, None, None


class _ScaleByScalar:
    @staticmethod
    def apply_raw(t, s):
        """t * s for a 0-dim device tensor s (chunk_frac scaling of the loss) — one axpby3 launch."""
        out = torch.empty_like(t)
        _lib.call("diqt_axpby3", t.view(1, -1), None, None, s.reshape(1).contiguous(), None, None, 0.0, 0.0, 0, out, 1,
                  t.numel(), _stream())
        return out


LOSS_KINDS = {'l2': 0, 'l1': 1, 'huber': 2}      # F.mse_loss / F.l1_loss / F.smooth_l1_loss (imagen_pytorch3D.py:1785-1790)


def mse_clamp(pred, target, lo=0.0, do_clamp=False, weight=None, kind='l2'):
    """mean(loss(clamp_min(pred, lo) - target) * weight[b]) with loss = square ('l2'), absolute value ('l1') or Huber with beta 1
    ('huber'); returns (loss, clamped_pred).  The reference clamps ``pred`` in place and returns it (imagen_pytorch3D.py:2361-2364);
    here the clamped values come back as a separate (non-differentiable) tensor — same numbers, no aliasing of an autograd view."""
    return _MseClampFn.apply(pred.contiguous(), target.contiguous(), weight, lo, do_clamp, LOSS_KINDS[kind])


# --------------------------------------------------------------------------------------------
# optimiser
# --------------------------------------------------------------------------------------------
def adam_step(param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, weight_decay, step, zero_grad=True, grad_scale=None):
    """Fused Adam over a flat arena.  ``grad_scale``: device scalar every gradient is multiplied with first (the clip coefficient of
    ``grad_norm_clip``)."""
    _chk(param, grad, exp_avg, exp_avg_sq)
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    if grad_scale is None:
        _lib.call("diqt_adam_step", param, grad, exp_avg, exp_avg_sq, param.numel(), float(lr), float(beta1), float(beta2),
                  float(eps), float(weight_decay), float(bc1), float(bc2), int(zero_grad), _stream())
    else:
        _chk(grad_scale)
        _lib.call("diqt_adam_step_scaled", param, grad, exp_avg, exp_avg_sq, param.numel(), float(lr), float(beta1), float(beta2),
                  float(eps), float(weight_decay), float(bc1), float(bc2), int(zero_grad), grad_scale, _stream())
    bump_weight_epoch()


def grad_norm_clip(grad_flat, max_norm):
    """torch.nn.utils.clip_grad_norm_ over a flat gradient arena WITHOUT touching it: returns a device tensor [total L2 norm,
    min(1, max_norm / (norm + 1e-6))]; the coefficient goes to ``adam_step(grad_scale=out[1:])``, which consumes the gradients."""
    _chk(grad_flat)
    nb = _lib.query("diqt_grad_norm_workspace_bytes")
    ws = _workspace(nb, grad_flat.device)
    out = torch.empty(2, dtype=torch.float32, device=grad_flat.device)
    _lib.call("diqt_grad_norm_clip", grad_flat, grad_flat.numel(), float(max_norm), ws, out, _stream())
    return out


def multi_accumulate(dst_flat, srcs, offsets):
    """dst_flat[off : off + t.numel()] += t for every (t, off): one launch for a whole micro-step's parameter gradients."""
    _chk(dst_flat, *srcs)
    if not srcs:
        return
    rows = []
    for t, off in zip(srcs, offsets):
        assert t.is_contiguous() and t.dtype == torch.float32
        rows.append((t.data_ptr(), int(off), t.numel()))
    # the table stays on the host and travels in the kernel arguments: no upload, and a captured micro-step replays the launch as it is
    table = torch.tensor(rows, dtype=torch.int64)
    _lib.call("diqt_multi_accumulate_host", dst_flat, table, len(rows), 16, _stream())   # same stream as the producers/allocator


def ema_lerp(ema, param, one_minus_decay):
    _chk(ema, param)
    _lib.call("diqt_ema_lerp", ema, param, ema.numel(), float(one_minus_decay), _stream())
    bump_weight_epoch()


# --------------------------------------------------------------------------------------------
# whole-volume inference (test_all.py:182-300)
# --------------------------------------------------------------------------------------------
def _chk_int(*ts):
    for t in ts:
        if not (t.is_cuda and t.dtype == torch.int32 and t.is_contiguous()):
            raise RuntimeError("index tables must be contiguous int32 HIP tensors")


def patch_gather(vol, idx, P, mean, std, want_patches=True, want_nonzero=False):
    """(patches [n,1,P,P,P] normalised, nonzero [n] int32) of the sliding-window origins ``idx`` [n,3] in a raw [D,H,W] volume."""
    _chk(vol)
    _chk_int(idx)
    D, H, W = vol.shape
    n = idx.shape[0]
    out = torch.empty((n, 1, P, P, P), dtype=torch.float32, device=vol.device) if want_patches else None
    nz = torch.empty(n, dtype=torch.int32, device=vol.device) if want_nonzero else None
    for lo in range(0, n, 65535):
        hi = min(n, lo + 65535)
        _lib.call("diqt_patch_gather", vol, idx[lo:hi], out[lo:hi] if out is not None else None,
                  nz[lo:hi] if nz is not None else None, hi - lo, D, H, W, P, float(mean), float(std), _stream())
    return out, nz


def patch_scatter(patches, idx, margins, pred, P):
    _chk(patches, pred)
    _chk_int(idx, margins)
    D, H, W = pred.shape
    _lib.call("diqt_patch_scatter", patches, idx, margins, pred, idx.shape[0], D, H, W, P, _stream())


def background_reset(pred, vol, mean, std, min_val):
    _chk(pred, vol)
    _lib.call("diqt_background_reset", pred, vol, pred.numel(), float(mean), float(std), float(min_val), _stream())


def min_value(x):
    _chk(x)
    ws = torch.empty(1024, dtype=torch.float32, device=x.device)
    out = torch.empty(1, dtype=torch.float32, device=x.device)
    _lib.call("diqt_min_value", x, x.numel(), ws, out, _stream())
    return out


def volume_blend(patches, slot, taps, vol, mean, std, min_val, fill, stride, want_std):
    """Weighted overlap blending of ``patches`` [S,N,P,P,P] (S samples of the N kept windows, candidate order) into the [D,H,W] grid of
    the raw volume ``vol``: ``slot`` [G0,G1,G2] int32 is a window's row in ``patches`` (-1: not kept) on the origin lattice
    ``g * stride``, ``taps`` [P] the 1-D window on the device.  Returns ``(mean, std | None)``: the per-voxel mean over the samples of
    the blended value and, with ``want_std`` (S >= 2), its unbiased standard deviation; uncovered voxels hold ``fill``, background
    voxels (normalised ``vol`` equal to ``min_val``) ``min_val``, both with deviation 0.  One launch, bit-reproducible."""
    _chk(patches, taps, vol)
    _chk_int(slot)
    if not (patches.is_contiguous() and taps.is_contiguous() and vol.is_contiguous()):
        raise RuntimeError("volume_blend: tensors must be contiguous")
    if patches.ndim != 5 or slot.ndim != 3 or vol.ndim != 3 or taps.ndim != 1:
        raise ValueError("volume_blend: expected patches [S,N,P,P,P], slot [G0,G1,G2], taps [P] and vol [D,H,W]")
    S, N, P = patches.shape[:3]
    if tuple(patches.shape[2:]) != (P, P, P) or taps.shape[0] != P:
        raise ValueError(f"volume_blend: patches {tuple(patches.shape)} / taps {tuple(taps.shape)} are not cubic windows of one size")
    if slot.numel() and int(slot.max()) >= N:                     # the kernel indexes `patches` by it
        raise ValueError(f"volume_blend: slot names window {int(slot.max())} of {N}")
    D, H, W = vol.shape
    out = torch.empty((D, H, W), dtype=torch.float32, device=vol.device)
    dev = torch.empty_like(out) if want_std else None
    _lib.call("diqt_volume_blend", patches if N else None, slot, taps, vol, out, dev, S, N, D, H, W, P, int(stride), *slot.shape,
              float(mean), float(std), float(min_val), float(fill), _stream())
    return out, dev


def anchored_noise(origins, C, P, D, H, W, seed, draw=0, sample=0, raw=False, device=None):
    """Volume-anchored noise for the windows ``origins`` [B,3] (HOST integers: (z, y, x) of each window's first voxel) of edge P in a
    C-channel [D,H,W] volume: fp32 normals [B,C,P,P,P], or with ``raw`` the two Philox4x32-10 words per voxel, int32 [B,C,P,P,P,2].
    The value at a voxel depends on (seed, channel, global position, draw, sample) alone -- include/diqt.h, diqt_anchored_noise -- so
    windows that overlap agree on the overlap bit for bit.  The origins are checked here, on the host, before anything is launched."""
    import numpy as np
    if torch.is_tensor(origins):
        origins = origins.detach().cpu().numpy()
    org = np.asarray(origins)
    if org.ndim != 2 or org.shape[1] != 3 or org.shape[0] < 1 or not np.issubdtype(org.dtype, np.integer):
        raise ValueError(f"anchored_noise: origins must be an integer [B,3] array with B >= 1, got {org.dtype} {tuple(org.shape)}")
    C, P, D, H, W = int(C), int(P), int(D), int(H), int(W)
    if min(C, P, D, H, W) < 1:
        raise ValueError(f"anchored_noise: C, P and the volume shape must be positive, got C {C}, P {P}, volume {(D, H, W)}")
    org = org.astype(np.int64)
    if (org < 0).any() or (org + P > np.array([D, H, W], dtype=np.int64)).any():
        bad = org[((org < 0) | (org + P > np.array([D, H, W], dtype=np.int64))).any(axis=1)][0]
        raise ValueError(f"anchored_noise: the window of edge {P} at {tuple(int(v) for v in bad)} leaves the volume {(D, H, W)}")
    seed, draw, sample = int(seed), int(draw), int(sample)
    if not (0 <= seed < 2 ** 64 and 0 <= draw < 2 ** 32 and 0 <= sample < 2 ** 32):
        raise ValueError(f"anchored_noise: seed must fit 64 bits, draw and sample 32 bits (unsigned), got {seed}, {draw}, {sample}")
    if not torch.cuda.is_available():
        raise RuntimeError("diffusioniqt_amd.ops.anchored_noise runs on the MI355X only (no CPU fallback)")
    device = torch.device('cuda' if device is None else device)
    B = org.shape[0]
    idx = torch.from_numpy(np.ascontiguousarray(org.astype(np.int32))).to(device)
    shape = (B, C, P, P, P)
    with torch.cuda.device(idx.device):
        out = torch.empty(shape + (2,), dtype=torch.int32, device=device) if raw else torch.empty(shape, dtype=torch.float32, device=device)
        _lib.call("diqt_anchored_noise", idx, B, C, P, D, H, W, seed, draw, sample, int(bool(raw)), out, _stream())
    return out


def _noise_key(who, seed, draw, sample):
    seed, draw, sample = int(seed), int(draw), int(sample)
    if not (0 <= seed < 2 ** 64 and 0 <= draw < 2 ** 32 and 0 <= sample < 2 ** 32):
        raise ValueError(f"{who}: seed must fit 64 bits, draw and sample 32 bits (unsigned), got {seed}, {draw}, {sample}")
    return seed, draw, sample


def _joint_lattice(who, slot, shape, P, stride):
    """The host-side shape rules shared by the two joint-sampling launches (the entry checks the lattice again)."""
    _chk_int(slot)
    if slot.ndim != 3 or len(shape) != 3:
        raise ValueError(f"{who}: expected slot [G0,G1,G2] and a [D,H,W] volume")
    stride = int(stride)
    if stride < 1 or P < 1 or any(P > s for s in shape):
        raise ValueError(f"{who}: windows of edge {P} with stride {stride} do not fit the volume {tuple(shape)}")
    if tuple(slot.shape) != tuple(len(range(0, s - P + 1, stride)) for s in shape):
        raise ValueError(f"{who}: slot {tuple(slot.shape)} is not the origin lattice of {tuple(shape)}, P {P}, stride {stride}")
    return stride


def _joint_windows(who, y, slot, taps, x_t, clamp_mode, stride):
    """The host checks shared by the joint step launches; returns (N, P, stride)."""
    _chk(y, taps, x_t)
    if y.ndim != 4 or x_t.ndim != 3 or taps.ndim != 1:
        raise ValueError(f"{who}: expected y [N,P,P,P], slot [G0,G1,G2], taps [P] and x_t [D,H,W]")
    if not (y.is_contiguous() and taps.is_contiguous() and x_t.is_contiguous()):
        raise RuntimeError(f"{who}: tensors must be contiguous")
    N, P = y.shape[:2]
    if tuple(y.shape[1:]) != (P, P, P) or taps.shape[0] != P:
        raise ValueError(f"{who}: y {tuple(y.shape)} / taps {tuple(taps.shape)} are not cubic windows of one size")
    stride = _joint_lattice(who, slot, x_t.shape, P, stride)
    if int(clamp_mode) not in (0, 1):
        raise ValueError(f"{who}: clamp_mode must be 0 (min) or 1 (box), got {clamp_mode!r}")
    return N, P, stride


def _joint_slots(who, slot, N):
    if slot.numel() and int(slot.max()) >= N:                     # the kernel indexes `y` by it
        raise ValueError(f"{who}: slot names window {int(slot.max())} of {N}")


def _joint_initial(who, entry, head, floats, shape, need, seed, draw, sample, device, draws=1, more_draws=()):
    """The initial state of a joint chain, one path for its makers: a new fp32 [D,H,W] = ``shape`` volume on ``device``, filled by
    the window-less launch of ``entry`` -- ``head(out)`` are its arguments before the shape, ``floats`` its coefficients; the lattice and
    the clamp are zeros.  ``need``: how the shape error begins; ``draws``: how many consecutive draws the launch reads; ``more_draws``:
    the further draw indices of an entry that takes some between ``draw`` and ``sample``."""
    shape = tuple(int(s) for s in shape)
    if len(shape) != 3 or min(shape) < 1:
        raise ValueError(f"{who}: {need} a positive (D, H, W), got {shape!r}")
    seed, draw, sample = _noise_key(who, seed, draw, sample)
    if draw + draws > 2 ** 32:
        raise ValueError(f"{who}: draw + 1 must fit 32 bits (unsigned), got draw {draw}")
    if not torch.cuda.is_available():
        raise RuntimeError(f"diffusioniqt_amd.ops.{who} runs on the MI355X only (no CPU fallback)")
    device = torch.device('cuda' if device is None else device)
    with torch.cuda.device(device):
        out = torch.empty(shape, dtype=torch.float32, device=device)
        _lib.call(entry, *head(out), *shape, 0, 0, 0, 0, 0, *(float(v) for v in floats), 0, seed, draw, *more_draws, sample, _stream())
    return out


def _joint_volumes(who, x_t, x0_prev, out, x0_out, need_x0=True):
    """``(out, x0_out)`` as a joint step launch takes them: new tensors like ``x_t`` where None (``x0_out`` only with ``need_x0``), after
    the check that they and ``x0_prev`` are contiguous fp32 device tensors of x_t's shape."""
    if out is None:
        out = torch.empty_like(x_t)
    if x0_out is None and need_x0:
        x0_out = torch.empty_like(x_t)
    for t, name in ((x0_prev, 'x0_prev'), (out, 'out'), (x0_out, 'x0_out')):
        if t is not None:
            _chk(t)
            if t.shape != x_t.shape or not t.is_contiguous():
                raise ValueError(f"{who}: {name} must be a contiguous tensor of x_t's shape")
    return out, x0_out


def volume_joint_init(shape, seed, sample=0, draw=0, device=None):
    """The initial state of a joint chain: fp32 [D,H,W], the volume-anchored normal of ``draw`` (channel 0) at every voxel -- the
    ``x_t == NULL`` launch of ``diqt_volume_joint_step``, bit for bit what ``anchored_noise`` hands to a window there."""
    return _joint_initial("volume_joint_init", "diqt_volume_joint_step", lambda out: (None, None, None, None, out, None, 0),
                          (0.0, 0.0, 0.0, 0.0, 0.0), shape, "shape must be", seed, draw, sample, device)


def volume_joint_step(y, slot, taps, x_t, kx, k0, kn, lo, hi, clamp_mode, stride, seed, draw, sample=0, out=None, x0_out=None):
    """One reverse step of the joint chain of a whole volume (include/diqt.h, diqt_volume_joint_step): ``y`` [N,P,P,P] are the kept
    windows' x0 predictions of this step in candidate order, ``slot`` / ``taps`` / ``stride`` as in ``volume_blend``, ``x_t`` [D,H,W] the
    state.  Per covered voxel x0 = the weighted mean of the clamped predictions (``clamp_mode`` 0: max(y, lo); 1: clip(y, lo, hi)) and
    x_next = kx x_t + k0 x0 + kn n with n the volume-anchored normal of (seed, draw, sample); uncovered voxels keep ``x_t``.  ``out``:
    where x_next goes (``x_t`` itself for an in-place step; None: a new tensor); ``x0_out`` (optional [D,H,W]) receives the fused x0
    (0 where uncovered).  Returns ``out``.  One launch, bit-reproducible."""
    N, P, stride = _joint_windows("volume_joint_step", y, slot, taps, x_t, clamp_mode, stride)
    seed, draw, sample = _noise_key("volume_joint_step", seed, draw, sample)
    _joint_slots("volume_joint_step", slot, N)
    out, x0_out = _joint_volumes("volume_joint_step", x_t, None, out, x0_out, need_x0=False)
    _lib.call("diqt_volume_joint_step", y if N else None, slot, taps, x_t, out, x0_out, N, *x_t.shape, P, stride, *slot.shape,
              float(kx), float(k0), float(kn), float(lo), float(hi), int(clamp_mode), seed, draw, sample, _stream())
    return out


def volume_joint_multistep(y, slot, taps, x_t, x0_prev, kx, k0, kp, lo, hi, clamp_mode, stride, out=None, x0_out=None):
    """One step of a second-order multistep chain on the joint state (include/diqt.h, diqt_volume_joint_multistep): ``volume_joint_step``
    with the previous step's fused x0 ``x0_prev`` [D,H,W] (None: zeros, the first step) as the third operand instead of a normal,
    x_next = kx x_t + k0 x0 + kp x0_prev on covered voxels; uncovered voxels keep ``x_t``.  ``out`` / ``x0_out``: where x_next and the
    fused x0 (0 where uncovered) go -- ``x_t`` and ``x0_prev`` themselves for an in-place step, None: new tensors.  Returns
    ``(out, x0_out)``.  One launch, bit-reproducible."""
    N, P, stride = _joint_windows("volume_joint_multistep", y, slot, taps, x_t, clamp_mode, stride)
    _joint_slots("volume_joint_multistep", slot, N)
    out, x0_out = _joint_volumes("volume_joint_multistep", x_t, x0_prev, out, x0_out)
    _lib.call("diqt_volume_joint_multistep", y if N else None, slot, taps, x_t, x0_prev, out, x0_out, N, *x_t.shape, P, stride,
              *slot.shape, float(kx), float(k0), float(kp), float(lo), float(hi), int(clamp_mode), _stream())
    return out, x0_out


def multistep_sde_step(x, x0, x0_prev, noise, kx, k0, kp, kn, out=None):
    """One step of DPM-Solver++ 2M in sigma space on a window batch (include/diqt.h, diqt_multistep_sde_step): ``x`` / ``x0`` [B, ...]
    the state and this step's (clamped or thresholded) prediction, ``x0_prev`` the previous step's and ``noise`` the step's normals (each
    may be None: zeros, not read), ``kx`` / ``k0`` / ``kp`` / ``kn`` device [B], one coefficient row per sample.
    x_next = kx x + k0 x0 + kp x0_prev (+ kn noise where kn != 0).  ``out``: where x_next goes (``x`` itself for an in-place step;
    None: a new tensor).  Returns ``out``.  One launch."""
    _chk(x, x0, x0_prev, noise, kx, k0, kp, kn, out)
    if x.ndim < 2 or x.numel() == 0:
        raise ValueError(f"multistep_sde_step: x must be a non-empty [B, ...] tensor, got {tuple(x.shape)}")
    B = x.shape[0]
    if B > 65535:
        raise ValueError(f"multistep_sde_step: at most 65535 samples per launch, got {B}")
    if out is None:
        out = torch.empty_like(x)
    for t, name in ((x0, 'x0'), (x0_prev, 'x0_prev'), (noise, 'noise'), (out, 'out')):
        if t is not None and t.shape != x.shape:
            raise ValueError(f"multistep_sde_step: {name} must have x's shape {tuple(x.shape)}, got {tuple(t.shape)}")
    for t, name in ((kx, 'kx'), (k0, 'k0'), (kp, 'kp'), (kn, 'kn')):
        if tuple(t.shape) != (B,):
            raise ValueError(f"multistep_sde_step: {name} must be a [B] = [{B}] tensor, got {tuple(t.shape)}")
    _lib.call("diqt_multistep_sde_step", x, x0, x0_prev, noise, kx, k0, kp, kn, out, B, x.numel() // B, _stream())
    return out


def volume_joint_multistep_sde(y, slot, taps, x_t, x0_prev, kx, k0, kp, kn, lo, hi, clamp_mode, stride, seed, draw, sample=0, out=None,
                               x0_out=None, shape=None, device=None):
    """One step of the sigma-space DPM-Solver++ 2M chain on the joint state (include/diqt.h, diqt_volume_joint_multistep_sde):
    ``volume_joint_multistep`` plus ``kn n`` with n the volume-anchored normal of (seed, draw, sample), added last and only when
    ``kn != 0`` -- with ``kn == 0`` the bits of ``volume_joint_multistep``.  ``x_t = None`` is the initial state: returns
    ``(kn n(draw), None)`` on a new [D,H,W] = ``shape`` volume (``y``, ``slot``, ``taps`` and the other coefficients are not looked at);
    otherwise ``out`` / ``x0_out`` are where x_next and the fused x0 (0 where uncovered) go -- ``x_t`` and ``x0_prev`` themselves for an
    in-place step, None: new tensors -- and ``(out, x0_out)`` is returned.  One launch, bit-reproducible."""
    seed, draw, sample = _noise_key("volume_joint_multistep_sde", seed, draw, sample)
    if x_t is None:
        return _joint_initial("volume_joint_multistep_sde", "diqt_volume_joint_multistep_sde",
                              lambda out: (None, None, None, None, None, out, None, 0), (0.0, 0.0, 0.0, kn, 0.0, 0.0), shape or (),
                              "the initial state needs shape =", seed, draw, sample, device), None
    N, P, stride = _joint_windows("volume_joint_multistep_sde", y, slot, taps, x_t, clamp_mode, stride)
    _joint_slots("volume_joint_multistep_sde", slot, N)
    out, x0_out = _joint_volumes("volume_joint_multistep_sde", x_t, x0_prev, out, x0_out)
    _lib.call("diqt_volume_joint_multistep_sde", y if N else None, slot, taps, x_t, x0_prev, out, x0_out, N, *x_t.shape, P, stride,
              *slot.shape, float(kx), float(k0), float(kp), float(kn), float(lo), float(hi), int(clamp_mode), seed, draw, sample,
              _stream())
    return out, x0_out


def consistency_cell(who, cell, weight=1.0, extents=()):
    """The host rules of the data-consistency arguments (``ValueError`` naming "consistency"; nothing touches the device): ``cell`` =
    (fz, fy, fx) integers >= 1 with 2 <= fz fy fx <= 64, ``weight`` a number in (0, 1] (0 is refused: it would differ from "off" in the
    sign of a zero), and every (size, axis) of ``extents`` a multiple of that axis' factor.  Returns ``(cell, weight)`` as ints / float."""
    import numbers
    ok = isinstance(cell, (tuple, list)) and len(cell) == 3 and all(
        not isinstance(f, bool) and isinstance(f, numbers.Integral) and f >= 1 for f in cell)
    if not ok or not 2 <= cell[0] * cell[1] * cell[2] <= 64:
        raise ValueError(f"{who}: the consistency cell must be (fz, fy, fx), integers >= 1 with 2 <= fz fy fx <= 64, got {cell!r}")
    if isinstance(weight, bool) or not isinstance(weight, (int, float)) or not 0. < weight <= 1.:
        raise ValueError(f"{who}: the consistency weight must be a number in (0, 1], got {weight!r}")
    cell = tuple(int(f) for f in cell)
    for size, axis in extents:
        if int(size) % cell[axis]:
            raise ValueError(f"{who}: the consistency cell {cell} does not divide the size {int(size)} of axis {axis}")
    return cell, float(weight)


def cell_profile(cell, profile):
    """The host table of a slice profile for the ``consistency_profile`` modes (``ValueError`` naming "consistency"; nothing touches
    the device).  ``profile`` = (pz, py, px): three sequences of finite numbers >= 0 of lengths fz, fy, fx, each with a positive sum
    -- the separable weight of a voxel under its cell's measurement, zeros for a slice gap.  Returns a contiguous fp32 host tensor
    [2, n], n = fz fy fx, in lexicographic (z, y, x) order: row 0 the weights u = pz_i py_j px_k / (sum pz sum py sum px) (so sum u = 1
    and the measurement of a cell is u . x), row 1 the gains g = u / sum u^2 of the projection x0' = x0 + w g (y - u . x0).  float64
    arithmetic, every entry rounded once to fp32; the uniform profile gives u = 1 / n and g = 1.  Move it to the device once per
    chain."""
    import math
    import numbers
    who = "cell_profile"
    cell, _ = consistency_cell(who, cell)
    if not isinstance(profile, (tuple, list)) or len(profile) != 3:
        raise ValueError(f"{who}: the consistency profile must be (pz, py, px), three sequences of weights, got {type(profile).__name__}")
    axes = []
    for axis, (p, f) in enumerate(zip(profile, cell)):
        if not isinstance(p, (tuple, list)) or len(p) != f:
            raise ValueError(f"{who}: axis {axis} of the consistency profile must be a sequence of {f} numbers (the cell is {cell})")
        if not all(not isinstance(v, bool) and isinstance(v, numbers.Real) and math.isfinite(v) and v >= 0 for v in p):
            raise ValueError(f"{who}: the weights of the consistency profile must be finite numbers >= 0, got {p!r} on axis {axis}")
        p = [float(v) for v in p]
        total = 0.0
        for v in p:
            total += v
        if not (total > 0.0 and math.isfinite(total)):
            raise ValueError(f"{who}: axis {axis} of the consistency profile must have a positive finite sum, got {p!r}")
        axes.append((p, total))
    (pz, sz), (py, sy), (px, sx) = axes
    den = sz * sy * sx
    u = [a * b * c / den for a in pz for b in py for c in px]
    sq = 0.0
    for v in u:
        sq += v * v
    if not (sq > 0.0 and math.isfinite(sq)):
        raise ValueError(f"{who}: the consistency profile {profile!r} has no usable norm (sum u^2 = {sq!r})")
    table = torch.tensor([u, [v / sq for v in u]], dtype=torch.float64).to(torch.float32).contiguous()
    if not bool(torch.isfinite(table).all()):
        raise ValueError(f"{who}: the consistency profile {profile!r} does not fit fp32")
    return table


def _cell_table(who, table, cell, like):
    """The check of a ``cell_profile`` table handed to a kernel: fp32 [2, n], contiguous, on ``like``'s device."""
    n = cell[0] * cell[1] * cell[2]
    if not torch.is_tensor(table) or table.dtype != torch.float32 or tuple(table.shape) != (2, n) or not table.is_contiguous():
        raise ValueError(f"{who}: the consistency profile table must be a contiguous fp32 [2, {n}] tensor (ops.cell_profile), got "
                         f"{(table.dtype, tuple(table.shape)) if torch.is_tensor(table) else type(table).__name__}")
    if table.device != like.device:
        raise ValueError(f"{who}: the consistency profile table is on {table.device}, the data on {like.device}")
    _chk(table)


def cell_mean(vol, cell):
    """The block average of a [D,H,W] volume over cells of ``cell`` = (fz, fy, fx) voxels (include/diqt.h, diqt_cell_mean): fp32
    [D/fz, H/fy, W/fx], each value the cell's sum in (z, y, x) order divided by n -- the measurement operator of the ``consistency``
    modes, e.g. to simulate a thick-slice acquisition.  One launch."""
    _chk(vol)
    if vol.ndim != 3 or not vol.is_contiguous() or vol.numel() == 0:
        raise ValueError(f"cell_mean: vol must be a non-empty contiguous [D,H,W] tensor, got {tuple(vol.shape)}")
    cell, _ = consistency_cell("cell_mean", cell, 1.0, [(s, a) for a, s in enumerate(vol.shape)])
    out = torch.empty(tuple(s // f for s, f in zip(vol.shape, cell)), dtype=torch.float32, device=vol.device)
    _lib.call("diqt_cell_mean", vol, out, *vol.shape, *cell, _stream())
    return out


def cell_measure(vol, cell, table):
    """The measurement of a [D,H,W] volume under a slice profile (include/diqt.h, diqt_cell_wmean): fp32 [D/fz, H/fy, W/fx], each
    value u . x over its cell with u = ``table[0]`` (``cell_profile``, on ``vol``'s device), the sum fused-multiply-added in (z, y, x)
    order -- the measurement operator of the ``consistency_profile`` modes, e.g. to simulate a thick-slice acquisition with a slice
    profile and gaps.  One launch."""
    _chk(vol)
    if vol.ndim != 3 or not vol.is_contiguous() or vol.numel() == 0:
        raise ValueError(f"cell_measure: vol must be a non-empty contiguous [D,H,W] tensor, got {tuple(vol.shape)}")
    cell, _ = consistency_cell("cell_measure", cell, 1.0, [(s, a) for a, s in enumerate(vol.shape)])
    _cell_table("cell_measure", table, cell, vol)
    out = torch.empty(tuple(s // f for s, f in zip(vol.shape, cell)), dtype=torch.float32, device=vol.device)
    _lib.call("diqt_cell_wmean", vol, table, out, *vol.shape, *cell, _stream())
    return out


def cell_replicate(meas, cell):
    """A measurement [D/fz, H/fy, W/fx] replicated onto the high-res grid [D,H,W] (every voxel holds its cell's value): what the
    ``consistency`` kernels read as ``meas_up``.  ``repeat_interleave`` on the three axes; no kernel of this library."""
    if not torch.is_tensor(meas) or meas.ndim != 3 or not meas.is_floating_point():
        raise ValueError(f"cell_replicate: the consistency measurement must be a float [D/fz, H/fy, W/fx] tensor, got "
                         f"{tuple(meas.shape) if torch.is_tensor(meas) else type(meas).__name__}")
    cell, _ = consistency_cell("cell_replicate", cell)
    out = meas.float()
    for axis, f in enumerate(cell):
        out = out.repeat_interleave(f, dim=axis)
    return out.contiguous()


def _project(who, entry, x0, meas, name, cell, weight, clamp, out, own, noise=None, out_noise=None, shaped=False):
    """The one body of the projection launches on a window batch: the [B,C,P,P,P] cube check, ``out`` (and, for a launch that is
    ``shaped`` -- it also reduces the step's normals ``noise`` -- ``out_noise``) allocated where None, the shape, contiguity and
    aliasing checks, the cell against the cube and the decoding of ``clamp``.  ``meas`` is the measurement operand, ``name`` what its
    wrapper calls it; ``own(cell, weight, P)`` runs the wrapper's own checks and returns its ``(pointers, scalars)``, the operands
    of ``entry`` between the measurement and ``out`` and between the cell and the clamp."""
    _chk(x0, meas, noise, out, out_noise)
    if x0.ndim != 5 or x0.numel() == 0 or len(set(x0.shape[2:])) != 1:
        raise ValueError(f"{who}: x0 must be a non-empty [B,C,P,P,P] tensor of cubes, got {tuple(x0.shape)}")
    if out is None:
        out = torch.empty_like(x0)
    if shaped and out_noise is None:
        out_noise = torch.empty_like(x0)
    operands = ((meas, name), (noise, 'noise'), (out, 'out'), (out_noise, 'out_noise')) if shaped else ((meas, name), (out, 'out'))
    for t, label in operands:
        if t.shape != x0.shape:
            raise ValueError(f"{who}: {label} must have x0's shape {tuple(x0.shape)}, got {tuple(t.shape)}")
    if not (x0.is_contiguous() and all(t.is_contiguous() for t, _ in operands)):
        raise RuntimeError(f"{who}: tensors must be contiguous")
    if shaped and (out_noise.data_ptr() in (x0.data_ptr(), out.data_ptr(), meas.data_ptr()) or
                   out.data_ptr() in (noise.data_ptr(), meas.data_ptr())):
        raise ValueError(f"{who}: out may alias only x0, out_noise only noise")
    P = x0.shape[2]
    cell, weight = consistency_cell(who, cell, weight, [(P, a) for a in range(3)])
    pointers, scalars = own(cell, weight, P)
    lo, hi, mode = (0., 0., 2) if clamp is None else clamp                # the entry's third mode: no clamp
    if clamp is not None and int(mode) not in (0, 1):
        raise ValueError(f"{who}: clamp mode must be 0 (min) or 1 (box), got {mode!r}")
    _lib.call(entry, x0, meas, *pointers, out, *((out_noise,) if shaped else ()), x0.shape[0] * x0.shape[1], P, *cell, *scalars,
              float(lo), float(hi), int(mode), _stream())
    return (out, out_noise) if shaped else out


def _joint_form(who, form, noisy=False):
    """``form`` of a consistent joint step as an int: 0, 1 or 2, and not 1 for a launch that shapes the step's normals."""
    form = int(form)
    if noisy and form not in (0, 2):
        raise ValueError(f"{who}: form must be 0 (first order) or 2 (multistep with noise), got {form!r}")
    if form not in (0, 1, 2):
        raise ValueError(f"{who}: form must be 0 (first order), 1 (multistep) or 2 (multistep with noise), got {form!r}")
    return form


def _joint_consistent(who, entry, y, slot, taps, x_t, x0_prev, meas_up, cell, weight, form, coefs, lo, hi, clamp_mode, stride, seed, draw,
                      sample, out, x0_out, own):
    """The one body of the consistent joint steps, after ``_joint_form``: the window, noise-key and slot checks, the cell against the
    volume, ``meas_up`` (None: the launch reads none) and the ``out`` / ``x0_out`` volumes.  ``own(cell, weight, P)`` runs the
    wrapper's own checks and returns its ``(pointers, scalars)``: the operands of ``entry`` between ``x0_prev`` and ``out`` and between
    the cell and the coefficients ``coefs`` = (kx, k0, kp, kn).  Returns ``(out, x0_out)``."""
    N, P, stride = _joint_windows(who, y, slot, taps, x_t, clamp_mode, stride)
    seed, draw, sample = _noise_key(who, seed, draw, sample)
    _joint_slots(who, slot, N)
    cell, weight = consistency_cell(who, cell, weight, [(s, a) for a, s in enumerate(x_t.shape)])
    if meas_up is not None:
        _chk(meas_up)
        if meas_up.shape != x_t.shape or not meas_up.is_contiguous():
            raise ValueError(f"{who}: meas_up must be a contiguous tensor of x_t's shape")
    pointers, scalars = own(cell, weight, P)
    out, x0_out = _joint_volumes(who, x_t, None if form == 0 else x0_prev, out, x0_out)
    _lib.call(entry, y if N else None, slot, taps, x_t, None if form == 0 else x0_prev, *pointers, out, x0_out, form, N, *x_t.shape, P,
              stride, *slot.shape, *cell, *scalars, *(float(k) for k in coefs), float(lo), float(hi), int(clamp_mode), seed, draw, sample,
              _stream())
    return out, x0_out


def cell_project(x0, meas_up, cell, weight=1.0, clamp=None, out=None):
    """The data-consistency projection of a window batch (include/diqt.h, diqt_cell_project): ``x0`` / ``meas_up`` [B,C,P,P,P] the
    prediction and the replicated measurement in the same space, ``cell`` = (fz, fy, fx), ``clamp`` = (lo, hi, mode) with
    ``ddpm_step``'s meaning (None: no clamp).  a = clamp(x0); per cell m = the mean of a; out = a + weight (meas_up - m).  ``out``:
    where it goes (``x0`` itself for an in-place projection; None: a new tensor).  Returns ``out``.  One launch."""
    return _project("cell_project", "diqt_cell_project", x0, meas_up, 'meas_up', cell, weight, clamp, out, lambda cell, w, P: ((), (w,)))


def cell_project_profile(x0, meas_up, cell, table, weight=1.0, clamp=None, out=None):
    """``cell_project`` for a measurement with a slice profile (include/diqt.h, diqt_cell_project_profile): ``table`` [2, n] =
    ``cell_profile``'s weights u and gains g, on ``x0``'s device.  a = clamp(x0); per cell m = u . a; out = a + weight g (meas_up - m):
    at weight 1 the weighted cell means land on the measurement, and a voxel in a gap (u = 0) is never moved.  Everything else --
    shapes, ``clamp``, ``out`` -- as there.  Returns ``out``.  One launch."""
    def own(cell, w, P):
        _cell_table("cell_project_profile", table, cell, x0)
        return (table,), (w,)
    return _project("cell_project_profile", "diqt_cell_project_profile", x0, meas_up, 'meas_up', cell, weight, clamp, out, own)


def volume_joint_consistent_step(y, slot, taps, x_t, x0_prev, meas_up, cell, weight, form, kx, k0, kp, kn, lo, hi, clamp_mode, stride,
                                 seed=0, draw=0, sample=0, out=None, x0_out=None):
    """One step of a joint chain with the data-consistency projection between the fuse and the update (include/diqt.h,
    diqt_volume_joint_consistent_step).  ``form`` 0 / 1 / 2: the update of ``volume_joint_step`` (``x0_prev`` and ``kp`` are not looked
    at) / ``volume_joint_multistep`` (``kn`` and the noise key are not) / ``volume_joint_multistep_sde``.  ``meas_up`` [D,H,W]: the
    replicated measurement in state space; ``cell`` = (fz, fy, fx) must divide the volume, ``weight`` in (0, 1].  Every cell whose
    voxels are all covered has the mean of its fused x0 moved onto the measurement (by ``weight`` of the way) before the update; a
    cell with an uncovered voxel steps as in the plain launch.  ``out`` / ``x0_out``: where x_next and the corrected x0 (0 where
    uncovered) go -- ``x_t`` and ``x0_prev`` themselves for an in-place step, None: new tensors.  Returns ``(out, x0_out)``.  One launch,
    bit-reproducible."""
    who = "volume_joint_consistent_step"
    return _joint_consistent(who, "diqt_volume_joint_consistent_step", y, slot, taps, x_t, x0_prev, meas_up, cell, weight,
                             _joint_form(who, form), (kx, k0, kp, kn), lo, hi, clamp_mode, stride, seed, draw, sample, out, x0_out,
                             lambda cell, w, P: ((meas_up,), (w,)))


def volume_joint_consistent_profile_step(y, slot, taps, x_t, x0_prev, meas_up, cell, table, weight, form, kx, k0, kp, kn, lo, hi,
                                         clamp_mode, stride, seed=0, draw=0, sample=0, out=None, x0_out=None):
    """``volume_joint_consistent_step`` for a measurement with a slice profile (include/diqt.h,
    diqt_volume_joint_consistent_profile_step): ``table`` [2, n] = ``cell_profile``'s weights and gains, on ``x_t``'s device.  Every
    cell whose voxels are ALL covered -- whatever their weights -- has the weighted mean u . x0 of its fused x0 moved onto the
    measurement (by ``weight`` of the way, each voxel by its gain) before the update; everything else as there.  Returns
    ``(out, x0_out)``.  One launch, bit-reproducible."""
    who = "volume_joint_consistent_profile_step"

    def own(cell, w, P):
        _cell_table(who, table, cell, x_t)
        return (meas_up, table), (w,)
    return _joint_consistent(who, "diqt_volume_joint_consistent_profile_step", y, slot, taps, x_t, x0_prev, meas_up, cell, weight,
                             _joint_form(who, form), (kx, k0, kp, kn), lo, hi, clamp_mode, stride, seed, draw, sample, out, x0_out, own)


class SlabTable:
    """What ``slab_profile`` returns: ``cell`` = (fz, fy, fx), ``reach`` = r and ``jmax``, the run positions the table holds;
    ``table`` the flat fp32 tensor the kernels read (include/diqt.h: u_z [fz + 2r], u_yx [fy fx], g_yx [fy fx], e, m [jmax],
    ip [jmax]); ``d``, ``e``, ``q`` the float64 numbers it was made from and ``cond`` = (d + 2e) / (d - 2e), which bounds the condition
    number of every run.  ``to(device)`` gives the same object around the moved tensor (once per chain or volume)."""

    def __init__(self, cell, reach, jmax, table, d, e, q):
        self.cell, self.reach, self.jmax, self.table, self.d, self.e, self.q = cell, reach, jmax, table, d, e, q
        self.cond = (d + 2 * e) / (d - 2 * e)

    def to(self, device):
        return SlabTable(self.cell, self.reach, self.jmax, self.table.to(device), self.d, self.e, self.q)

    def part(self, name):
        """The host copy of one member of the flat table: 'uz', 'uyx', 'gyx', 'e', 'm' or 'ip'."""
        L, n, J = self.cell[0] + 2 * self.reach, self.cell[1] * self.cell[2], self.jmax
        lo, hi = {'uz': (0, L), 'uyx': (L, L + n), 'gyx': (L + n, L + 2 * n), 'e': (L + 2 * n, L + 2 * n + 1),
                  'm': (L + 2 * n + 1, L + 2 * n + 1 + J), 'ip': (L + 2 * n + 1 + J, L + 2 * n + 1 + 2 * J)}[name]
        return self.table[lo:hi].cpu()

    def __repr__(self):
        return f"SlabTable(cell={self.cell}, reach={self.reach}, jmax={self.jmax}, cond<={self.cond:.3g})"


def slab_profile(cell, profile, jmax=64):
    """The host table of overlapping slice profiles for the ``consistency_slab`` modes (``ValueError`` naming "consistency"; nothing
    touches the device).  ``profile`` = (pz, py, px): ``pz`` of length L = fz + 2r with reach r >= 1 and 2r <= fz (the profile of a
    slice along z, r voxels into each neighbouring cell), ``py`` / ``px`` of lengths fy / fx (the in-plane profile inside the cell, as
    in ``cell_profile``); all finite and >= 0, every axis with a positive sum.  ``jmax``: the run positions to tabulate, at least the
    number of slices of the largest domain the table will serve (a cube's P / fz, a volume's D / fz).  With u_z = pz / sum pz,
    u_yx = py (x) px / (sum py sum px), q = sum u_yx^2, d = sum u_z^2 and e = sum_{i < 2r} u_z[i] u_z[i + fz]: the table holds u_z, u_yx,
    g_yx = u_yx / q, e and for j < jmax the pivots pi_0 = d, pi_j = d - e^2 / pi_{j-1} as m_j = e / pi_{j-1} (m_0 = 0) and
    ip_j = 1 / pi_j.  float64 arithmetic, every entry rounded once to fp32.  A profile with d - 2e < d / 64 is refused: the rule bounds
    the condition number of any run by 128, well inside what the fp32 solve resolves.  Returns a ``SlabTable``."""
    import math
    import numbers
    who = "slab_profile"
    cell, _ = consistency_cell(who, cell)
    if isinstance(jmax, bool) or not isinstance(jmax, numbers.Integral) or not 1 <= jmax <= 65535:
        raise ValueError(f"{who}: the consistency_slab table needs 1 <= jmax <= 65535 run positions, got {jmax!r}")
    if not isinstance(profile, (tuple, list)) or len(profile) != 3:
        raise ValueError(f"{who}: the consistency_slab profile must be (pz, py, px), three sequences of weights, got "
                         f"{type(profile).__name__}")
    if not all(isinstance(p, (tuple, list)) for p in profile):
        raise ValueError(f"{who}: every axis of the consistency_slab profile must be a sequence of numbers")
    extra = len(profile[0]) - cell[0]
    if extra < 2 or extra % 2 or extra > cell[0]:
        raise ValueError(f"{who}: pz of the consistency_slab profile must have fz + 2r = {cell[0]} + 2r entries with reach r >= 1 and "
                         f"2r <= fz (a slice overlaps its two neighbours only), got {len(profile[0])}")
    r = extra // 2
    axes = []
    for axis, (p, f) in enumerate(zip(profile, (cell[0] + 2 * r, cell[1], cell[2]))):
        if len(p) != f:
            raise ValueError(f"{who}: axis {axis} of the consistency_slab profile must be a sequence of {f} numbers (the cell is {cell})")
        if not all(not isinstance(v, bool) and isinstance(v, numbers.Real) and math.isfinite(v) and v >= 0 for v in p):
            raise ValueError(f"{who}: the weights of the consistency_slab profile must be finite numbers >= 0, got {p!r} on axis {axis}")
        p = [float(v) for v in p]
        total = 0.0
        for v in p:
            total += v
        if not (total > 0.0 and math.isfinite(total)):
            raise ValueError(f"{who}: axis {axis} of the consistency_slab profile must have a positive finite sum, got {p!r}")
        axes.append((p, total))
    (pz, sz), (py, sy), (px, sx) = axes
    uz = [v / sz for v in pz]
    uyx = [a * b / (sy * sx) for a in py for b in px]
    q = d = e = 0.0
    for v in uyx:
        q += v * v
    for v in uz:
        d += v * v
    for i in range(2 * r):
        e += uz[i] * uz[i + cell[0]]
    if not (q > 0.0 and d > 0.0 and math.isfinite(q) and math.isfinite(d)):
        raise ValueError(f"{who}: the consistency_slab profile {profile!r} has no usable norm (q = {q!r}, d = {d!r})")
    if d - 2 * e < d / 64:
        raise ValueError(f"{who}: the consistency_slab profile is too flat across the slice border: d - 2e = {d - 2 * e!r} is below "
                         f"d / 64 = {d / 64!r} (d = sum u_z^2, e the overlap product), so neighbouring slices are nearly dependent")
    m, ip, pivot = [], [], d
    for j in range(int(jmax)):
        if j:
            m.append(e / pivot)
            pivot = d - e * e / pivot
        else:
            m.append(0.0)
        ip.append(1.0 / pivot)
    table = torch.tensor(uz + uyx + [v / q for v in uyx] + [e] + m + ip, dtype=torch.float64).to(torch.float32).contiguous()
    if not bool(torch.isfinite(table).all()):
        raise ValueError(f"{who}: the consistency_slab profile {profile!r} does not fit fp32")
    return SlabTable(cell, r, int(jmax), table, d, e, q)


def slab_lds(cell, edge):
    """The bytes of LDS ``slab_project`` plans for cubes of edge ``edge``: one float per slice for each of the 256 threads of a block.
    The entry refuses a plan above 65536 with DIQT_E_SHAPE."""
    return 4 * 256 * (int(edge) // cell[0])


def slab_plan(who, cell, edge):
    """``ValueError`` naming "consistency_slab" for cubes whose ``slab_project`` launch plans more than 64 KiB of LDS."""
    need = slab_lds(cell, edge)
    if need > 65536:
        raise ValueError(f"{who}: consistency_slab with the cell {tuple(cell)} on cubes of edge {edge} plans {need} bytes of LDS "
                         f"({int(edge) // cell[0]} slices for each of 256 columns), above the 65536 a launch may have")


def _slab_table(who, table, cell, like, slices):
    """The check of a ``slab_profile`` table handed to a kernel: a ``SlabTable`` of this cell with at least ``slices`` run positions,
    its tensor on ``like``'s device.  Returns the cell as the table has it."""
    if not isinstance(table, SlabTable):
        raise ValueError(f"{who}: the consistency_slab table must be what ops.slab_profile returns, got {type(table).__name__}")
    if tuple(cell) != table.cell:
        raise ValueError(f"{who}: the consistency_slab table was made for the cell {table.cell}, not {tuple(cell)}")
    if table.jmax < slices:
        raise ValueError(f"{who}: the consistency_slab table holds {table.jmax} run positions, the domain has {slices} slices "
                         f"(ops.slab_profile(..., jmax=))")
    if table.table.device != like.device:
        raise ValueError(f"{who}: the consistency_slab table is on {table.table.device}, the data on {like.device}")
    _chk(table.table)
    return table.cell


def slab_measure(vol, cell, table):
    """The measurement of a [D,H,W] volume under overlapping slice profiles (include/diqt.h, diqt_slab_measure): fp32
    [D/fz, H/fy, W/fx], slice s of a column the u_z-weighted sum of the in-plane weighted means of planes s fz - r .. s fz + fz + r - 1;
    a slice that leaves the volume takes the truncated sum.  ``table``: ``slab_profile``'s, on ``vol``'s device.  It simulates the
    acquisition of the ``consistency_slab`` modes; once per volume.  One launch."""
    who = "slab_measure"
    _chk(vol)
    if vol.ndim != 3 or not vol.is_contiguous() or vol.numel() == 0:
        raise ValueError(f"{who}: vol must be a non-empty contiguous [D,H,W] tensor, got {tuple(vol.shape)}")
    cell, _ = consistency_cell(who, cell, 1.0, [(s, a) for a, s in enumerate(vol.shape)])
    _slab_table(who, table, cell, vol, 1)
    out = torch.empty(tuple(s // f for s, f in zip(vol.shape, cell)), dtype=torch.float32, device=vol.device)
    _lib.call("diqt_slab_measure", vol, table.table, out, *vol.shape, *cell, table.reach, table.jmax, _stream())
    return out


def slab_project(x0, meas_up, cell, table, weight=1.0, clamp=None, out=None):
    """``cell_project_profile`` for overlapping slice profiles (include/diqt.h, diqt_slab_project): ``table`` = ``slab_profile``'s, on
    ``x0``'s device, with jmax >= P / fz.  a = clamp(x0); the domain is each cube, whose slices 1 .. P/fz - 2 are the active rows (the
    first and last leave the cube and are never enforced); out = a + weight A_act^T (A_act A_act^T)^-1 (y_act - A_act a) by one
    tridiagonal solve per column, y_s read from ``meas_up`` at the first voxel of slice s' cell.  A voxel under no active row keeps
    a.  Shapes, ``clamp`` and ``out`` as there.  Returns ``out``.  One launch."""
    def own(cell, w, P):
        _slab_table("slab_project", table, cell, x0, P // cell[0])
        slab_plan("slab_project", cell, P)
        return (table.table,), (table.reach, table.jmax, w)
    return _project("slab_project", "diqt_slab_project", x0, meas_up, 'meas_up', cell, weight, clamp, out, own)


def slab_workspace(shape, cell, device):
    """``(workspace, coef)`` of the joint slab launches for a [D,H,W] volume: fp32 device tensors of (2 D + D/fz) (H/fy) (W/fx) floats
    and [D/fz, H/fy, W/fx]; allocate them once per volume."""
    D, H, W = (int(s) for s in shape)
    rows = (D // cell[0], H // cell[1], W // cell[2])
    return (torch.empty((2 * D + rows[0]) * rows[1] * rows[2], dtype=torch.float32, device=device),
            torch.empty(rows, dtype=torch.float32, device=device))


def _slab_joint(who, x_like, cell, table, workspace, coef):
    """The host checks the two joint slab launches share; returns the cell."""
    cell, _ = consistency_cell(who, cell, 1.0, [(s, a) for a, s in enumerate(x_like.shape)])
    _slab_table(who, table, cell, x_like, x_like.shape[0] // cell[0])
    _chk(workspace, coef)
    rows = tuple(s // f for s, f in zip(x_like.shape, cell))
    need = (2 * x_like.shape[0] + rows[0]) * rows[1] * rows[2]
    if workspace.ndim != 1 or workspace.numel() < need or tuple(coef.shape) != rows:
        raise ValueError(f"{who}: the consistency_slab workspace must hold {need} floats and coef be {rows} (ops.slab_workspace), got "
                         f"{tuple(workspace.shape)} and {tuple(coef.shape)}")
    return cell


def volume_joint_slab_coeffs(y, slot, taps, meas_up, cell, table, workspace, coef, lo, hi, clamp_mode, stride):
    """The first two of the three launches of a joint step under ``consistency_slab`` (include/diqt.h,
    diqt_volume_joint_slab_coeffs): the windows ``y`` are fused as in ``volume_joint_step`` into one weighted plane value per
    (z, cy, cx), then every column (cy, cx) solves its runs of active rows along the whole depth; the coefficients c go into
    ``coef`` [D/fz, H/fy, W/fx], the run positions stay in ``workspace`` for ``volume_joint_consistent_slab_step``.  ``meas_up``
    [D,H,W]: the replicated measurement in state space.  Returns ``coef``."""
    who = "volume_joint_slab_coeffs"
    N, P, stride = _joint_windows(who, y, slot, taps, meas_up, clamp_mode, stride)
    _joint_slots(who, slot, N)
    cell = _slab_joint(who, meas_up, cell, table, workspace, coef)
    _lib.call("diqt_volume_joint_slab_coeffs", y if N else None, slot, taps, meas_up, table.table, workspace, workspace.numel(), coef, N,
              *meas_up.shape, P, stride, *slot.shape, *cell, table.reach, table.jmax, float(lo), float(hi), int(clamp_mode), _stream())
    return coef


def volume_joint_consistent_slab_step(y, slot, taps, x_t, x0_prev, cell, table, workspace, coef, weight, form, kx, k0, kp, kn, lo, hi,
                                      clamp_mode, stride, seed=0, draw=0, sample=0, out=None, x0_out=None):
    """The third launch (include/diqt.h, diqt_volume_joint_consistent_slab_step): ``volume_joint_consistent_step``'s three update forms
    with the slab correction of every voxel between the fuse and the update, ``workspace`` / ``coef`` as
    ``volume_joint_slab_coeffs`` left them for the same ``y``.  A covered voxel under no active row steps with its plain x0.
    ``out`` / ``x0_out`` as there.  Returns ``(out, x0_out)``.  One launch, bit-reproducible."""
    who = "volume_joint_consistent_slab_step"

    def own(cell, w, P):
        _slab_joint(who, x_t, cell, table, workspace, coef)
        return (table.table, coef, workspace, workspace.numel()), (table.reach, table.jmax, w)
    return _joint_consistent(who, "diqt_volume_joint_consistent_slab_step", y, slot, taps, x_t, x0_prev, None, cell, weight,
                             _joint_form(who, form), (kx, k0, kp, kn), lo, hi, clamp_mode, stride, seed, draw, sample, out, x0_out, own)


class BandTable:
    """What ``band_table`` returns: ``shape`` = (Nz, Ny, Nx) the periodic domain, ``cell`` = (fz, fy, fx), ``offset`` = the three
    offsets in voxels; ``axes``: per axis a dict of ``N``, ``n`` = N / f, ``f``, ``delta``, ``active``, ``kept`` (the kept k >= 1),
    ``h`` (the normalised weights, h[0] = 1), the fp32 host tensors ``d``, ``a``, ``g`` [N] and the float64 values ``d64``, ``a64``,
    ``g64`` they were rounded from; ``active``: the mask of the axes that
    have a pass (1 = z, 2 = y, 4 = x); ``table``: the flat fp32 tensor the kernels read (include/diqt.h: d, a, g of z, then y, then
    x); ``gain`` = the product over the active axes of sum_m |d[m]| on the fp32 values, the factor of the rounding bounds.
    ``to(device)`` gives the same object around the moved tensor (once per chain or volume)."""

    def __init__(self, shape, cell, offset, axes, table):
        self.shape, self.cell, self.offset, self.axes, self.table = shape, cell, offset, axes, table
        self.active = sum(1 << i for i, ax in enumerate(axes) if ax['active'])
        self.gain = 1.0
        for ax in axes:
            if ax['active']:
                self.gain *= float(ax['d'].double().abs().sum())

    def to(self, device):
        return BandTable(self.shape, self.cell, self.offset, self.axes, self.table.to(device))

    def __repr__(self):
        return f"BandTable(shape={self.shape}, cell={self.cell}, kept={[len(ax['kept']) for ax in self.axes]}, gain={self.gain:.3g})"


BAND_MAX_N = 512                                                 # csrc/datapath.hip: BAND_MAX_N


def band_table(shape, cell, band=None, offset=None):
    """The host tables of a k-space band limit for the ``consistency_band`` modes (``ValueError`` naming "consistency_band"; nothing
    touches the device).  ``shape`` = (Nz, Ny, Nx): the periodic domain, a cube of a sampler or a whole volume; ``cell`` = (fz, fy, fx)
    divides it, n = N / f per axis.  ``band`` = (hz, hy, hx), or None for three times None; per axis None or a sequence of weights for
    the frequencies k = 0 .. len - 1, the band symmetric in +-k: finite and >= 0, h[0] > 0 (the weights are divided by it),
    len <= kappa + 1 with kappa = (n - 1) // 2 (the measurement grid holds nothing beyond), a zero drops its frequency, and a positive
    weight below max(h) / 64 is refused (the back-projection would amplify by more than 64 on that axis).  None is the full band, ones
    up to kappa -- on an even n the unpaired Nyquist bin is NOT part of the band -- except on an axis with f = 1, which is then the
    identity and has no pass.  ``offset`` = (dz, dy, dx) in high-res voxels (None: zeros; 'centre': (f - 1) / 2 per axis): where in
    its cell a low-res sample sits.  With K the kept k >= 1, in float64, every entry rounded once to fp32:
        d[m] = (1 + 2 sum_K cos(2 pi k m / N)) / N, for m <= N / 2 and mirrored (symmetric to the bit): P[i, j] = d[(i - j) mod N];
        a[m] = (1 + 2 sum_K h_k cos(2 pi k (m + delta) / N)) / N: A[s, j] = a[(s f - j) mod N], rows sum to 1;
        g[m] = (1 + 2 sum_K cos(2 pi k (m + delta) / N) / h_k) / n: A+[j, s] = g[(s f - j) mod N].
    Returns a ``BandTable``."""
    import math
    import numbers
    who = "band_table"
    real = lambda v: not isinstance(v, bool) and isinstance(v, numbers.Real) and math.isfinite(v)
    if (not isinstance(shape, (tuple, list, torch.Size)) or len(shape) != 3 or
            not all(not isinstance(s, bool) and isinstance(s, numbers.Integral) and s >= 1 for s in shape)):
        raise ValueError(f"{who}: the consistency_band domain must be (Nz, Ny, Nx), three integers >= 1, got {shape!r}")
    shape = tuple(int(s) for s in shape)
    try:
        cell, _ = consistency_cell(who, cell, 1.0, [(s, a) for a, s in enumerate(shape)])
    except ValueError as err:
        raise ValueError(f"{err} (consistency_band)") from None
    if band is None:
        band = (None, None, None)
    if not isinstance(band, (tuple, list)) or len(band) != 3:
        raise ValueError(f"{who}: consistency_band must be (hz, hy, hx), per axis None or a sequence of k-space weights, got {band!r}")
    if offset is None:
        offset = (0.0, 0.0, 0.0)
    elif isinstance(offset, str) and offset == 'centre':
        offset = tuple((f - 1) / 2 for f in cell)
    if not isinstance(offset, (tuple, list)) or len(offset) != 3 or not all(real(v) for v in offset):
        raise ValueError(f"{who}: the offset of consistency_band must be three finite numbers (high-res voxels) or 'centre', got {offset!r}")
    offset = tuple(float(v) for v in offset)
    axes = []
    for axis, (N, f, h, delta) in enumerate(zip(shape, cell, band, offset)):
        n = N // f
        kappa = (n - 1) // 2
        if h is not None and (torch.is_tensor(h) or type(h).__module__ == 'numpy'):
            h = h.tolist()
        if h is None and f == 1:
            if delta != 0.0:
                raise ValueError(f"{who}: axis {axis} of consistency_band is the identity (f = 1, full band) and takes no offset, got "
                                 f"{delta!r}")
            one = torch.zeros(N, dtype=torch.float32)
            one[0] = 1.0
            axes.append(dict(N=N, n=n, f=f, delta=0.0, active=False, kept=tuple(range(1, N // 2 + 1)), h=None, d=one, a=one, g=one,
                             d64=one.double(), a64=one.double(), g64=one.double()))
            continue
        if h is None:
            h = [1.0] * (kappa + 1)
        if not isinstance(h, (tuple, list)) or len(h) < 1 or not all(real(v) and v >= 0 for v in h):
            raise ValueError(f"{who}: axis {axis} of consistency_band must be None or a sequence of finite weights >= 0 for "
                             f"k = 0 .. len - 1, got {h!r}")
        if not h[0] > 0:
            raise ValueError(f"{who}: axis {axis} of consistency_band must keep the mean: h[0] > 0, got {h[0]!r}")
        if len(h) > kappa + 1:
            raise ValueError(f"{who}: axis {axis} of consistency_band has {len(h)} weights, the measurement grid of n = {n} samples "
                             f"holds the frequencies k <= kappa = {kappa} only (at most {kappa + 1} weights)")
        h = [float(v) / float(h[0]) for v in h]
        top = max(h)
        if any(0 < v < top / 64 for v in h):
            raise ValueError(f"{who}: axis {axis} of consistency_band has a positive weight below max(h) / 64 = {top / 64!r}: the "
                             f"back-projection would amplify that frequency by more than 64 (drop it with a zero instead), got {h!r}")
        kept = tuple(k for k in range(1, len(h)) if h[k] > 0)
        w = 2.0 * math.pi / N
        d = [0.0] * N
        for m in range(N // 2 + 1):
            s = 1.0
            for k in kept:
                s += 2.0 * math.cos(w * ((k * m) % N))
            d[m] = d[(N - m) % N] = s / N
        a, g = [], []
        for m in range(N):
            sa = sg = 1.0
            for k in kept:
                c = math.cos(w * (((k * m) % N) + k * delta))
                sa += 2.0 * h[k] * c
                sg += 2.0 * c / h[k]
            a.append(sa / N)
            g.append(sg / n)
        d64, a64, g64 = (torch.tensor(v, dtype=torch.float64) for v in (d, a, g))
        axes.append(dict(N=N, n=n, f=f, delta=delta, active=True, kept=kept, h=tuple(h), d=d64.to(torch.float32), a=a64.to(torch.float32),
                         g=g64.to(torch.float32), d64=d64, a64=a64, g64=g64))
    table = torch.cat([t for ax in axes for t in (ax['d'], ax['a'], ax['g'])]).contiguous()
    return BandTable(shape, cell, offset, axes, table)


def band_lds(N):
    """The bytes of LDS one band pass plans on an axis of ``N`` voxels: the padded doubled table and a 64 x 65 panel."""
    return 4 * (2 * int(N) + 128 + 64 * 65)


def band_plan(who, shape):
    """``ValueError`` naming "consistency_band" for a domain with an axis above 512 voxels or a pass that plans more than 64 KiB of LDS;
    before anything touches the device."""
    for axis, N in enumerate(shape):
        if int(N) > BAND_MAX_N:
            raise ValueError(f"{who}: consistency_band takes at most {BAND_MAX_N} voxels per axis, axis {axis} of {tuple(shape)} has {int(N)}")
        if band_lds(N) > 65536:
            raise ValueError(f"{who}: consistency_band on axis {axis} of {tuple(shape)} plans {band_lds(N)} bytes of LDS, above the 65536 "
                             f"a launch may have")


def band_workspace(shape, device):
    """The workspace of the joint band launches for a [D,H,W] volume: a fp32 device tensor [5, D, H, W] -- the fused prediction a, the
    covered flags, the residual r, c = P r and the buffer of ``band_apply``; allocate it once per volume."""
    return torch.empty((5, *(int(s) for s in shape)), dtype=torch.float32, device=device)


def _band_table(who, table, shape, like, cell=None):
    """The check of a ``band_table`` table handed to a kernel: a ``BandTable`` of this domain (and cell), its tensor on ``like``'s
    device, and the domain inside ``band_plan``."""
    if not isinstance(table, BandTable):
        raise ValueError(f"{who}: the consistency_band table must be what ops.band_table returns, got {type(table).__name__}")
    if tuple(shape) != table.shape:
        raise ValueError(f"{who}: the consistency_band table was made for the domain {table.shape}, not {tuple(shape)}")
    if cell is not None and tuple(cell) != table.cell:
        raise ValueError(f"{who}: the consistency_band table was made for the cell {table.cell}, not {tuple(cell)}")
    band_plan(who, shape)
    if table.table.device != like.device:
        raise ValueError(f"{who}: the consistency_band table is on {table.table.device}, the data on {like.device}")
    _chk(table.table)


def _band_rect(who, entry, src, table, low, workspace):
    """``band_measure`` / ``band_backproject``: ``src`` is the [D,H,W] volume or (``low``) its measurement."""
    _chk(src, workspace)
    _band_table(who, table, getattr(table, 'shape', ()), src)
    rows = tuple(s // f for s, f in zip(table.shape, table.cell))
    want = rows if low else table.shape
    if src.ndim != 3 or not src.is_contiguous() or tuple(src.shape) != want:
        raise ValueError(f"{who}: expected a contiguous {want} tensor for the consistency_band domain {table.shape} and cell {table.cell}, "
                         f"got {tuple(src.shape)}")
    need = 2 * table.shape[0] * table.shape[1] * table.shape[2]
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.float32, device=src.device)
    if not workspace.is_contiguous() or workspace.numel() < need:
        raise ValueError(f"{who}: the consistency_band workspace must be a contiguous fp32 tensor of twice the volume, {need} floats")
    out = torch.empty(table.shape if low else rows, dtype=torch.float32, device=src.device)
    _lib.call(entry, src, table.table, out, workspace, workspace.numel(), *table.shape, *table.cell, table.active, _stream())
    return out


def band_measure(vol, table, workspace=None):
    """The measurement of a [D,H,W] volume under a k-space band limit (include/diqt.h, diqt_band_measure): fp32 [D/fz, H/fy, W/fx] =
    A vol, the periodic low-pass of ``table`` (``band_table`` for this volume's shape, on its device) sampled on the low-res grid.  It
    simulates the acquisition of the ``consistency_band`` modes; once per volume.  ``workspace``: fp32, twice the volume (None: made
    here).  One launch per active axis."""
    return _band_rect("band_measure", "diqt_band_measure", vol, table, False, workspace)


def band_backproject(y, table, workspace=None):
    """t = A+ y on the high-res grid (include/diqt.h, diqt_band_backproject): ``y`` [D/fz, H/fy, W/fx] a measurement, fp32 [D,H,W] the
    band-limited volume whose measurement it is -- what the ``consistency_band`` projections read as their target.  Once per volume;
    ``table`` and ``workspace`` as in ``band_measure``."""
    return _band_rect("band_backproject", "diqt_band_backproject", y, table, True, workspace)


def band_project(x0, target, cell, table, weight=1.0, clamp=None, out=None, workspace=None):
    """``cell_project_profile`` for a k-space band limit (include/diqt.h, diqt_band_project): ``target`` [B,C,P,P,P] = t = A+ y of every
    cube, ``table`` = ``band_table((P, P, P), cell, ...)`` on ``x0``'s device.  a = clamp(x0); out = a + weight P (t - a) with P the
    band's projector on the periodic cube: at weight 1 the measurement of out is y.  ``workspace``: fp32, two batches of cubes (None:
    made here).  Shapes, ``clamp`` and ``out`` as there.  Returns ``out``.  One launch per active axis (one more with a single axis)."""
    who = "band_project"
    ws = []

    def own(cell, w, P):
        _band_table(who, table, (P, P, P), x0, cell)
        space = torch.empty(2 * x0.numel(), dtype=torch.float32, device=x0.device) if workspace is None else workspace
        _chk(space)
        if space.dtype != torch.float32 or not space.is_contiguous() or space.numel() < 2 * x0.numel():
            raise ValueError(f"{who}: the consistency_band workspace must be a contiguous fp32 tensor of two cube batches, "
                             f"{2 * x0.numel()} floats")
        ws.append(space)
        return (table.table, space), (space.numel(), table.active, w)
    return _project(who, "diqt_band_project", x0, target, 'target', cell, weight, clamp, out, own)


def _band_joint(who, x_like, table, workspace):
    """The host checks the joint band launches share."""
    _band_table(who, table, tuple(x_like.shape), x_like)
    _chk(workspace)
    if tuple(workspace.shape) != (5, *x_like.shape) or not workspace.is_contiguous():
        raise ValueError(f"{who}: the consistency_band workspace must be a contiguous fp32 {(5, *x_like.shape)} tensor "
                         f"(ops.band_workspace), got {tuple(workspace.shape)}")


def volume_joint_band_residual(y, slot, taps, target, table, workspace, lo, hi, clamp_mode, stride):
    """The first of the three calls of a joint step under ``consistency_band`` (include/diqt.h, diqt_volume_joint_band_residual): the
    windows ``y`` are fused as in ``volume_joint_step``; ``workspace[0]`` receives the fused clamped prediction a (0 where no kept
    window covers), ``workspace[1]`` the covered flags and ``workspace[2]`` the residual ``target`` - a, 0 where uncovered -- there the
    measurement is believed, so only a fully covered volume is made exactly consistent.  ``target`` [D,H,W]: t = A+ y in state space.
    Returns ``workspace``.  One launch."""
    who = "volume_joint_band_residual"
    N, P, stride = _joint_windows(who, y, slot, taps, target, clamp_mode, stride)
    _joint_slots(who, slot, N)
    _band_joint(who, target, table, workspace)
    _lib.call("diqt_volume_joint_band_residual", y if N else None, slot, taps, target, workspace[0], workspace[1], workspace[2], N,
              *target.shape, P, stride, *slot.shape, float(lo), float(hi), int(clamp_mode), _stream())
    return workspace


def band_apply(x, table, out, workspace):
    """``out`` = P ``x``: the band's projector over a [D,H,W] volume (include/diqt.h, diqt_band_apply), through ``out`` and
    ``workspace`` (a volume each; the three are different tensors).  The second call of a joint step: ``band_apply(ws[2], table, ws[3],
    ws[4])``.  Returns ``out``.  One launch per active axis."""
    who = "band_apply"
    _chk(x, out, workspace)
    _band_table(who, table, tuple(x.shape), x)
    for t, name in ((x, 'x'), (out, 'out'), (workspace, 'workspace')):
        if t.shape != x.shape or not t.is_contiguous():
            raise ValueError(f"{who}: {name} must be a contiguous fp32 tensor of the domain {table.shape}, got {tuple(t.shape)}")
    if len({x.data_ptr(), out.data_ptr(), workspace.data_ptr()}) != 3:
        raise ValueError(f"{who}: x, out and the workspace must be three different volumes")
    _lib.call("diqt_band_apply", x, table.table, out, workspace, workspace.numel(), *x.shape, table.active, _stream())
    return out


def volume_joint_consistent_band_step(y, slot, taps, x_t, x0_prev, cell, table, workspace, weight, form, kx, k0, kp, kn, lo, hi,
                                      clamp_mode, stride, seed=0, draw=0, sample=0, out=None, x0_out=None):
    """The third call (include/diqt.h, diqt_volume_joint_consistent_band_step): ``volume_joint_consistent_step``'s three update forms on
    x0' = a + weight c, with a and the flags as ``volume_joint_band_residual`` left them in ``workspace`` for the same ``y`` and
    c = ``workspace[3]`` from ``band_apply``; the windows are not walked again.  An uncovered voxel keeps ``x_t``.  ``out`` / ``x0_out``
    as there.  Returns ``(out, x0_out)``.  One launch, bit-reproducible."""
    who = "volume_joint_consistent_band_step"

    def own(cell, w, P):
        _band_joint(who, x_t, table, workspace)
        if tuple(cell) != table.cell:
            raise ValueError(f"{who}: the consistency_band table was made for the cell {table.cell}, not {tuple(cell)}")
        return (workspace[0], workspace[1], workspace[3]), (w,)
    return _joint_consistent(who, "diqt_volume_joint_consistent_band_step", y, slot, taps, x_t, x0_prev, None, cell, weight,
                             _joint_form(who, form), (kx, k0, kp, kn), lo, hi, clamp_mode, stride, seed, draw, sample, out, x0_out, own)


class TileOperator:
    """What ``tile_operator`` returns: ``cell`` = (fz, fy, fx); ``A`` [m, n] and ``pinv`` = A+ [n, m], float64 host tensors; ``table``
    the fp32 host [n, n] projector P = A+ A, symmetric to the bit, which the projecting kernels read; ``rank``; ``gain`` =
    max_q sum_r |P[q][r]| over the fp32 table (float), the factor of the rounding bounds; ``m`` and ``n``."""

    def __init__(self, cell, A, pinv, table, rank, gain):
        self.cell, self.A, self.pinv, self.table, self.rank, self.gain = cell, A, pinv, table, rank, gain
        self.m, self.n = A.shape

    def __repr__(self):
        return f"TileOperator(cell={self.cell}, m={self.m}, rank={self.rank}, gain={self.gain:.3g})"


def tile_projector(A):
    """float64 ``(A+, P, rank)`` of a finite [m, n] matrix by its SVD (host): a singular value counts as zero at or below
    1e-10 s_max; one in (1e-10, 1e-6) s_max leaves the rank ambiguous and is refused, as is rank 0 (``ValueError`` naming
    "consistency_operator").  P = A+ A symmetrised, (P + P^T) / 2: the orthogonal projector onto the row space of A."""
    who = "tile_operator (consistency_operator)"
    U, S, Vh = torch.linalg.svd(A, full_matrices=False)
    smax = float(S[0]) if S.numel() else 0.0
    if not smax > 0.0:
        raise ValueError(f"{who}: the operator has rank 0")
    rel = S / smax
    if bool(((rel > 1e-10) & (rel < 1e-6)).any()):
        raise ValueError(f"{who}: a singular value of {float(rel[(rel > 1e-10) & (rel < 1e-6)][0]):.3g} s_max leaves the rank "
                         f"ambiguous (zero is <= 1e-10 s_max, a real one >= 1e-6 s_max)")
    keep = rel > 1e-10
    pinv = (Vh[keep].T / S[keep]) @ U[:, keep].T
    proj = pinv @ A
    return pinv.contiguous(), (proj + proj.T) / 2, int(keep.sum())


def tile_operator(cell, A):
    """The host side of a tile-local linear measurement for the ``consistency_operator`` modes (``ValueError`` naming
    "consistency_operator"; nothing touches the device).  The volume splits into disjoint tiles of ``cell`` = (fz, fy, fx) voxels and
    every tile is measured by ``A``, array-like [m, n], finite, m >= 1, n = fz fy fx in 2 .. 64, its columns in lexicographic
    (z, y, x) order q = (i fy + j) fx + k.  float64: ``tile_projector``, then the fp32 table.  Refused besides: an operator blind to
    the tile mean, max |P 1 - 1| > 1e-9 -- with 1 in the row space, A+(a y + b A 1) = a t + b 1, so the back-projected measurement t
    passes through the z-score and the denoiser's affine ``state_space`` map as a plain volume (a pseudo-inverse of this size is
    accurate to about 1e-13; an operator that misses the constant misses it by O(1 / n) >= 1 / 64).  A single row with a slice
    profile is such an operator: that is ``consistency_profile``.  A ``TileOperator`` of the same cell is returned as it is."""
    who = "tile_operator (consistency_operator)"
    cell, _ = consistency_cell(who, cell)
    if isinstance(A, TileOperator):
        if A.cell != cell:
            raise ValueError(f"{who}: the operator was made for the cell {A.cell}, not {cell}")
        return A
    n = cell[0] * cell[1] * cell[2]
    try:
        A = torch.as_tensor(A, dtype=torch.float64).detach().cpu().contiguous()     # a list is read as float64, not through fp32
    except (TypeError, ValueError, RuntimeError):
        raise ValueError(f"{who}: the operator must be an [m, {n}] array of numbers, got {type(A).__name__}") from None
    if A.ndim != 2 or A.shape[0] < 1 or A.shape[1] != n:
        raise ValueError(f"{who}: the operator must be [m, {n}] with m >= 1 (the cell {cell} has n = {n} voxels), got {tuple(A.shape)}")
    if not bool(torch.isfinite(A).all()):
        raise ValueError(f"{who}: the operator must be finite")
    pinv, proj, rank = tile_projector(A)
    miss = float((proj.sum(1) - 1.0).abs().max())
    if miss > 1e-9:
        raise ValueError(f"{who}: the operator is blind to the tile mean (max |P 1 - 1| = {miss:.3g}): the constant must lie in its "
                         f"row space; a single row with a slice profile is consistency_profile, not an operator")
    table = proj.to(torch.float32).contiguous()
    return TileOperator(cell, A, pinv, table, rank, float(table.double().abs().sum(1).max()))


def stack_operator(cell, axes):
    """The ``tile_operator`` of orthogonal thick-slice stacks: for each axis of ``axes`` (distinct values of 0, 1, 2, in that order)
    one row per line of the tile along that axis -- the lines in lexicographic order of their other two coordinates -- with weight
    1 / f_axis on the line's voxels: a stack with thick slices along that axis and full resolution in plane."""
    who = "stack_operator (consistency_operator)"
    cell, _ = consistency_cell(who, cell)
    if not isinstance(axes, (tuple, list)) or not axes or len(set(axes)) != len(axes) or any(
            isinstance(a, bool) or a not in (0, 1, 2) for a in axes):
        raise ValueError(f"{who}: axes must be distinct values of 0, 1, 2, got {axes!r}")
    n = cell[0] * cell[1] * cell[2]
    q = torch.arange(n).reshape(cell)
    rows = []
    for a in axes:
        for line in q.movedim(a, -1).reshape(-1, cell[a]):
            r = torch.zeros(n, dtype=torch.float64)
            r[line] = 1.0 / cell[a]
            rows.append(r)
    return tile_operator(cell, torch.stack(rows))


def stack_rows(stacks, cell, axes):
    """The stack volumes a user has as the [m, D/fz, H/fy, W/fx] measurement of ``stack_operator(cell, axes)``: ``stacks[i]`` is the
    volume of ``axes[i]``, [D,H,W] with that axis divided by its factor ([D/fz, H, W] for axis 0, ...).  A pure reshape and
    permute."""
    who = "stack_rows (consistency_operator)"
    cell, _ = consistency_cell(who, cell)
    if not isinstance(stacks, (tuple, list)) or not isinstance(axes, (tuple, list)) or len(stacks) != len(axes) or not stacks or any(
            isinstance(a, bool) or a not in (0, 1, 2) for a in axes) or not all(torch.is_tensor(v) and v.ndim == 3 for v in stacks):
        raise ValueError(f"{who}: one [.,.,.] tensor per axis of {axes!r} (values of 0, 1, 2)")
    full = tuple(s * (cell[b] if b == axes[0] else 1) for b, s in enumerate(stacks[0].shape))      # the volume the stacks were cut from
    out = []
    for vol, a in zip(stacks, axes):
        want = tuple(s // cell[a] if b == a else s for b, s in enumerate(full))
        if any(s % f for s, f in zip(full, cell)) or tuple(vol.shape) != want:
            raise ValueError(f"{who}: the stack of axis {a} must be {want} (the volume {full}, the cell {cell}), got {tuple(vol.shape)}")
        # [D/fz, i, H/fy, j, W/fx, k] with the stack's own axis of length 1, then the in-tile coordinates in front
        dims = [d for s, f in zip(full, cell) for d in (s // f, f)]
        dims[2 * a + 1] = 1
        out.append(vol.reshape(dims).permute(1, 3, 5, 0, 2, 4).reshape(-1, *dims[0::2]))
    return torch.cat(out).contiguous()


def _tile_volume(who, vol, operator):
    _chk(vol)
    if not isinstance(operator, TileOperator):
        raise ValueError(f"{who}: operator must be what ops.tile_operator returns (consistency_operator), got {type(operator).__name__}")
    return operator.cell


def tile_measure(vol, operator):
    """The measurement of a [D,H,W] volume under a tile operator (include/diqt.h, diqt_tile_measure): fp32 [m, D/fz, H/fy, W/fx],
    row r of A applied to every tile, the sum fused-multiply-added in (z, y, x) order with A rounded to fp32 -- it simulates the
    acquisition.  One launch."""
    who = "tile_measure"
    cell = _tile_volume(who, vol, operator)
    if vol.ndim != 3 or not vol.is_contiguous() or vol.numel() == 0:
        raise ValueError(f"{who}: vol must be a non-empty contiguous [D,H,W] tensor, got {tuple(vol.shape)}")
    consistency_cell(who, cell, 1.0, [(s, a) for a, s in enumerate(vol.shape)])
    out = torch.empty((operator.m, *(s // f for s, f in zip(vol.shape, cell))), dtype=torch.float32, device=vol.device)
    _lib.call("diqt_tile_measure", vol, operator.A.to(vol.device, torch.float32).contiguous(), out, operator.m, *vol.shape, *cell, _stream())
    return out


def tile_backproject(y, operator):
    """t = A+ y on the high-res grid (include/diqt.h, diqt_tile_backproject): ``y`` fp32 [m, D/fz, H/fy, W/fx] as ``tile_measure``
    or ``stack_rows`` lay it out, the result fp32 [D,H,W] -- what the ``consistency_operator`` kernels read where the replicated
    measurement stood.  A+ rounded to fp32, the sum fused-multiply-added in row order.  One launch."""
    who = "tile_backproject"
    cell = _tile_volume(who, y, operator)
    if y.ndim != 4 or y.shape[0] != operator.m or not y.is_contiguous() or y.numel() == 0:
        raise ValueError(f"{who}: y must be a non-empty contiguous [{operator.m}, D/fz, H/fy, W/fx] tensor (consistency_operator: one "
                         f"value per row of the operator and tile), got {tuple(y.shape)}")
    shape = tuple(s * f for s, f in zip(y.shape[1:], cell))
    out = torch.empty(shape, dtype=torch.float32, device=y.device)
    _lib.call("diqt_tile_backproject", y, operator.pinv.to(y.device, torch.float32).contiguous(), out, operator.m, *shape, *cell, _stream())
    return out


def _tile_table(who, table, cell, like):
    """The check of a ``tile_operator`` table handed to a kernel: fp32 [n, n], contiguous, on ``like``'s device."""
    n = cell[0] * cell[1] * cell[2]
    if not torch.is_tensor(table) or table.dtype != torch.float32 or tuple(table.shape) != (n, n) or not table.is_contiguous():
        raise ValueError(f"{who}: the consistency_operator table must be a contiguous fp32 [{n}, {n}] tensor (ops.tile_operator), got "
                         f"{(table.dtype, tuple(table.shape)) if torch.is_tensor(table) else type(table).__name__}")
    if table.device != like.device:
        raise ValueError(f"{who}: the consistency_operator table is on {table.device}, the data on {like.device}")
    _chk(table)


def tile_project(x0, target, cell, table, weight=1.0, clamp=None, out=None):
    """``cell_project`` for a tile operator (include/diqt.h, diqt_tile_project): ``target`` [B,C,P,P,P] = windows of the
    back-projected measurement t = A+ y, ``table`` [n, n] = ``tile_operator``'s P, on ``x0``'s device.  a = clamp(x0); per tile
    out = a + weight (t - P a): at weight 1, P out = t, and A out = y for a y in the range of A.  Everything else -- shapes,
    ``clamp``, ``out`` -- as there.  Returns ``out``.  One launch."""
    def own(cell, w, P):
        _tile_table("tile_project", table, cell, x0)
        return (table,), (w,)
    return _project("tile_project", "diqt_tile_project", x0, target, 'target', cell, weight, clamp, out, own)


def volume_joint_consistent_tile_step(y, slot, taps, x_t, x0_prev, meas_up, cell, table, weight, form, kx, k0, kp, kn, lo, hi,
                                      clamp_mode, stride, seed=0, draw=0, sample=0, out=None, x0_out=None):
    """``volume_joint_consistent_step`` for a tile operator (include/diqt.h, diqt_volume_joint_consistent_tile_step): ``meas_up``
    [D,H,W] = the back-projected measurement t in state space, ``table`` [n, n] = ``tile_operator``'s P, on ``x_t``'s device.  Every
    tile whose voxels are ALL covered has its fused x0 moved to x0 + ``weight`` (t - P x0) before the update; everything else as
    there.  Returns ``(out, x0_out)``.  One launch, bit-reproducible."""
    who = "volume_joint_consistent_tile_step"

    def own(cell, w, P):
        _tile_table(who, table, cell, x_t)
        return (meas_up, table), (w,)
    return _joint_consistent(who, "diqt_volume_joint_consistent_tile_step", y, slot, taps, x_t, x0_prev, meas_up, cell, weight,
                             _joint_form(who, form), (kx, k0, kp, kn), lo, hi, clamp_mode, stride, seed, draw, sample, out, x0_out, own)


def consistency_noise_sigma(who, sigma_y, has_consistency=True, stochastic=True):
    """The host rules of ``consistency_noise=`` (``ValueError`` naming "consistency_noise"; nothing touches the device): it rides on
    ``consistency``, is a finite number > 0 (0 would leave the last step's 0 / 0 undefined; "off" is None) and needs a chain with a
    stochastic row -- a deterministic sampler gets weight 0 on every step.  Returns it as a float."""
    import math
    import numbers
    if not has_consistency:
        raise ValueError(f"{who}: consistency_noise needs consistency=(measurement, cell)")
    if isinstance(sigma_y, bool) or not isinstance(sigma_y, numbers.Real) or not math.isfinite(sigma_y) or not sigma_y > 0:
        raise ValueError(f"{who}: consistency_noise must be a finite number > 0, the standard deviation of the measurement's noise "
                         f"(None: a noise-free measurement), got {sigma_y!r}")
    if not stochastic:
        raise ValueError(f"{who}: consistency_noise needs a sampler with fresh noise per step (ddpm, ddim or dpmpp2m with eta > 0): a "
                         f"deterministic chain would never project; use a constant consistency_weight < 1 there")
    return float(sigma_y)


def cell_norm(cell, table=None):
    """s = |u|_2, the one non-zero singular value of the cell measurement A (A A^T = s^2 I), as a float (float64 arithmetic):
    1 / sqrt(n) for the plain mean, sqrt(sum u^2) over the fp32 weights of a ``cell_profile`` table summed in float64."""
    import math
    cell, _ = consistency_cell("cell_norm", cell)
    n = cell[0] * cell[1] * cell[2]
    if table is None:
        return 1.0 / math.sqrt(n)
    if not torch.is_tensor(table) or table.dtype != torch.float32 or tuple(table.shape) != (2, n):
        raise ValueError(f"cell_norm: the consistency profile table must be an fp32 [2, {n}] tensor (ops.cell_profile)")
    sq = 0.0
    for v in table[0].tolist():                          # fp32 values, widened exactly
        sq += v * v
    return math.sqrt(sq)


def consistency_noise_schedule(rows, s, sigma_y, weight):
    """The per-step weights and noise reductions of noise-aware data consistency (DDNM+, Wang et al. 2023, 3.3) for a chain
    x_next = kx x + k0 x0' + kp x0'_prev + kn eps: float64 [T, 2] = (w_i, shrink_i).  ``rows`` [T, 4] = (kx, k0, kp, kn) per step
    (first-order tables pass kp = 0), ``s`` = ``cell_norm``, ``sigma_y`` the standard deviation of the measurement's noise in the units
    the chain projects in, ``weight`` the cap (``consistency_weight``).  With w_{-1} = 0, per row: kn == 0 gives w_i = 0 (a plain step);
    otherwise b = kn s / sigma_y, w_i = min(weight, max(0, (b - kp w_{i-1}) / k0)), a_i = k0 w_i + kp w_{i-1},
    rho_i = sqrt(max(0, 1 - (a_i / b)^2)), shrink_i = 1 - rho_i: in the range of A the measurement noise the step carries,
    (a_i sigma_y / s)^2, plus the fresh noise left there, (rho_i kn)^2, is kn^2.  A row with kn != 0 and k0 <= 0 is a ``ValueError``.
    Pure host arithmetic in float64."""
    import math
    rows = [[float(v) for v in r] for r in (rows.tolist() if torch.is_tensor(rows) else rows)]
    if any(len(r) != 4 for r in rows):
        raise ValueError("consistency_noise_schedule: rows must be [T, 4] = (kx, k0, kp, kn)")
    s, sigma_y, weight = float(s), float(sigma_y), float(weight)
    out = torch.zeros(len(rows), 2, dtype=torch.float64)
    w_prev = 0.0
    for i, (kx, k0, kp, kn) in enumerate(rows):
        w_i = shrink = 0.0
        if kn != 0.0:
            if not k0 > 0.0:
                raise ValueError(f"consistency_noise_schedule: consistency_noise needs k0 > 0 on a stochastic row, row {i} has {k0!r}")
            b = kn * s / sigma_y
            w_i = min(weight, max(0.0, (b - kp * w_prev) / k0))
            a = k0 * w_i + kp * w_prev
            shrink = 1.0 - math.sqrt(max(0.0, 1.0 - (a / b) ** 2))
        out[i, 0], out[i, 1] = w_i, shrink
        w_prev = w_i
    return out


def consistency_noise_dispatch(schedule):
    """A schedule as the chains dispatch on it: the (w_i, shrink_i) rounded to fp32, as Python floats."""
    return [tuple(r) for r in schedule.to(torch.float32).tolist()]


def cell_project_noise(x0, meas_up, noise, cell, weight, shrink, table=None, clamp=None, out=None, out_noise=None):
    """One step's projection of noise-aware data consistency (include/diqt.h, diqt_cell_project_noise): ``cell_project`` (``table``
    None) or ``cell_project_profile`` of ``x0`` with ``weight`` and ``clamp``, and the step's normals ``noise`` -- a tensor of
    ``x0``'s shape -- reduced in the range of A, noise' = noise - shrink g (u . noise) per cell, which is the same projection of
    ``noise`` onto a zero measurement with ``shrink`` and no clamp, bit for bit.  ``weight`` and ``shrink`` in (0, 1].  ``out`` /
    ``out_noise``: where x0' and noise' go (``x0`` / ``noise`` themselves for in place; None: new tensors -- a caller's noise tensor is
    never modified unless it is handed in as ``out_noise``).  Returns ``(x0', noise')``.  One launch."""
    who = "cell_project_noise"
    if isinstance(shrink, bool) or not isinstance(shrink, (int, float)) or not 0. < shrink <= 1.:
        raise ValueError(f"{who}: the consistency_noise shrink must be a number in (0, 1], got {shrink!r}")

    def own(cell, w, P):
        if table is not None:
            _cell_table(who, table, cell, x0)
        return (noise, table), (w, float(shrink))
    return _project(who, "diqt_cell_project_noise", x0, meas_up, 'meas_up', cell, weight, clamp, out, own, noise, out_noise, shaped=True)


def volume_joint_consistent_noise_step(y, slot, taps, x_t, x0_prev, meas_up, cell, table, weight, shrink, form, kx, k0, kp, kn, lo, hi,
                                       clamp_mode, stride, seed=0, draw=0, sample=0, out=None, x0_out=None):
    """``volume_joint_consistent_step`` (``table`` None) or ``volume_joint_consistent_profile_step`` with the step's normal shaped as
    in ``cell_project_noise`` before it enters the update (include/diqt.h, diqt_volume_joint_consistent_noise_step): in every cell
    whose voxels are ALL covered, eps' = eps - ``shrink`` g (u . eps); a cell with an uncovered voxel keeps its plain x0 and its plain
    normals.  ``form`` 0 or 2 with ``kn != 0`` and ``shrink`` in (0, 1] only.  The normals are the plain launch's (same key, same draw
    number).  Returns ``(out, x0_out)``.  One launch, bit-reproducible."""
    who = "volume_joint_consistent_noise_step"
    form = _joint_form(who, form, noisy=True)
    if float(kn) == 0.0:
        raise ValueError(f"{who}: kn == 0: a step without a normal has no consistency_noise shaping")
    if isinstance(shrink, bool) or not isinstance(shrink, (int, float)) or not 0. < shrink <= 1.:
        raise ValueError(f"{who}: the consistency_noise shrink must be a number in (0, 1], got {shrink!r}")

    def own(cell, w, P):
        if table is not None:
            _cell_table(who, table, cell, x_t)
        return (meas_up, table), (w, float(shrink))
    return _joint_consistent(who, "diqt_volume_joint_consistent_noise_step", y, slot, taps, x_t, x0_prev, meas_up, cell, weight, form,
                             (kx, k0, kp, kn), lo, hi, clamp_mode, stride, seed, draw, sample, out, x0_out, own)


class TileNoiseOperator(TileOperator):
    """What ``tile_noise_operator`` returns: a ``TileOperator`` (so ``tile_measure`` and ``tile_backproject`` take it) whose ``A`` is
    the matrix as given -- ``tile_measure`` still simulates the acquisition -- and whose ``pinv`` is the EFFECTIVE pseudo-inverse
    A_w+ diag(omega) [n, m] of the whitened operator A_w = diag(omega) A, omega_r = sigma_min / sigma_r.  ``table`` (P = A_w+ A_w),
    ``rank`` and ``gain`` as there.  Float64 host tensors besides: ``singular`` [rank], the non-zero singular values of A_w,
    ``basis`` [rank, n], its right singular vectors as rows, ``weights`` [m] = omega and ``row_noise`` [m] = sigma."""

    def __init__(self, cell, A, pinv, table, rank, gain, singular, basis, weights, row_noise):
        super().__init__(cell, A, pinv, table, rank, gain)
        self.singular, self.basis, self.weights, self.row_noise = singular, basis, weights, row_noise

    def __repr__(self):
        return f"TileNoiseOperator(cell={self.cell}, m={self.m}, rank={self.rank}, gain={self.gain:.3g})"


def tile_noise_operator(cell, A, row_noise):
    """The host side of ``consistency_row_noise=`` (DDNM+ for a tile operator; ``ValueError`` naming "consistency_row_noise"; nothing
    touches the device).  ``A`` as ``tile_operator`` takes it (a ``TileOperator`` gives its ``A``); ``row_noise`` the standard
    deviation of the noise of each row of A: one finite number > 0, or a sequence of m of them (stacks: one value per stack, repeated
    over its rows).  Whitening is unit-free: omega_r = sigma_min / sigma_r in (0, 1], A_w = diag(omega) A, and in float64 the SVD
    A_w = U S V^T under ``tile_projector``'s zero and ambiguity thresholds.  t = (A_w+ diag omega) y is what ``tile_backproject``
    makes of the raw y with the object returned; P = A_w+ A_w projects onto the row space of A as before, so the "blind to the tile
    mean" refusal is ``tile_operator``'s.  With one number omega = 1 and everything is ``tile_operator``'s.  A
    ``TileNoiseOperator`` given deviations proportional to its own (the same noise in other units: a z-score, a ``state_space``
    slope) keeps its decomposition to the bit and takes the new values as ``row_noise``; otherwise it gives its matrix."""
    import math
    import numbers
    who = "tile_noise_operator (consistency_row_noise)"
    try:
        base = tile_operator(cell, A)
        if isinstance(A, TileNoiseOperator):                              # its pinv is an effective one: start again from the matrix
            base = tile_operator(cell, A.A)
    except ValueError as err:
        raise ValueError(f"{err} (consistency_row_noise rides on consistency_operator)") from None
    m = base.m

    def number(v):
        return not isinstance(v, bool) and isinstance(v, numbers.Real) and math.isfinite(v) and v > 0

    if torch.is_tensor(row_noise) or type(row_noise).__module__ == 'numpy':
        row_noise = row_noise.tolist()
    if isinstance(row_noise, (tuple, list)):
        if len(row_noise) != m or not all(number(v) for v in row_noise):
            raise ValueError(f"{who}: consistency_row_noise must be one finite number > 0 or {m} of them, one per row of the operator, "
                             f"got {row_noise!r}")
        sigma = [float(v) for v in row_noise]
    elif number(row_noise):
        sigma = [float(row_noise)] * m
    else:
        raise ValueError(f"{who}: consistency_row_noise must be one finite number > 0 or a sequence of {m} of them, the standard "
                         f"deviation of the noise of each row of the operator, got {row_noise!r}")
    sigma = torch.tensor(sigma, dtype=torch.float64)
    if isinstance(A, TileNoiseOperator):
        ratio = sigma / A.row_noise
        if bool(((ratio - ratio[0]).abs() <= 1e-12 * ratio[0]).all()):    # a change of units: whitening is unit-free
            return TileNoiseOperator(A.cell, A.A, A.pinv, A.table, A.rank, A.gain, A.singular, A.basis, A.weights, sigma)
    omega = sigma.min() / sigma
    Aw = omega[:, None] * base.A
    try:
        pinv_w, proj, rank = tile_projector(Aw)
    except ValueError as err:
        raise ValueError(f"{err} (after whitening by consistency_row_noise)") from None
    _, S, Vh = torch.linalg.svd(Aw, full_matrices=False)
    keep = S / S[0] > 1e-10
    table = proj.to(torch.float32).contiguous()
    return TileNoiseOperator(base.cell, base.A, (pinv_w * omega[None, :]).contiguous(), table, rank,
                             float(table.double().abs().sum(1).max()), S[keep].contiguous(), Vh[keep].contiguous(), omega, sigma)


def _tile_noise_op(who, operator):
    if not isinstance(operator, TileNoiseOperator):
        raise ValueError(f"{who}: operator must be what ops.tile_noise_operator returns (consistency_row_noise), got "
                         f"{type(operator).__name__}")


def tile_noise_schedule(operator, rows, sigma, weight):
    """The per-step, per-direction weights and noise reductions of ``consistency_row_noise``: float64 [T, rank, 2] =
    (lambda_ij, shrink_ij).  Along the right singular vector v_j of the whitened operator the noise of t has the deviation
    sigma_min / s_j, so direction j takes the scalar recursion as it is: ``consistency_noise_schedule(rows, s_j, sigma, weight)``,
    history term, cap and the zero on rows with kn = 0 included.  ``sigma`` = sigma_min, the smallest row deviation, in the units the
    chain projects in.  Null-space directions are not listed: their lambda and shrink are 0."""
    who = "tile_noise_schedule"
    _tile_noise_op(who, operator)
    return torch.stack([consistency_noise_schedule(rows, float(s), sigma, weight) for s in operator.singular.tolist()], dim=1)


def tile_noise_tables(operator, schedule):
    """The tables the ``consistency_row_noise`` launches read, and how each step dispatches: ``(tables, kinds)``.  ``tables`` is the
    fp32 host tensor [T, 2, n, n] = (M_i, G_i), M_i = V diag(lambda_i) V^T and G_i = V diag(shrink_i) V^T formed in float64,
    symmetrised as (X + X^T) / 2 and rounded once to fp32 -- lambda is continuous in s, so the result does not depend on the basis the
    SVD picked inside a repeated singular value.  ``kinds[i]`` = (kind, w), on the fp32 values of the schedule: ``('plain', 0.)`` when
    every lambda is 0 (the family's plain step, no projection), ``('tile', w)`` when every shrink is 0 and every lambda equals w (the
    constant-weight tile launch with P), else ``('noise', 0.)`` (the launches that read the tables)."""
    who = "tile_noise_tables"
    _tile_noise_op(who, operator)
    if not torch.is_tensor(schedule) or schedule.ndim != 3 or tuple(schedule.shape[1:]) != (operator.rank, 2):
        raise ValueError(f"{who}: the consistency_row_noise schedule must be [T, {operator.rank}, 2] (ops.tile_noise_schedule)")
    schedule = schedule.double()
    V = operator.basis.T                                                        # [n, rank]
    tables = torch.einsum('qj,tjc,rj->tcqr', V, schedule, V)
    tables = ((tables + tables.transpose(2, 3)) / 2).to(torch.float32).contiguous()
    kinds = []
    for step in schedule.to(torch.float32):                               # [rank, 2] of one step, as the device will see them
        lam, shrink = step[:, 0].tolist(), step[:, 1].tolist()
        if all(v == 0. for v in lam):
            kinds.append(('plain', 0.))
        elif all(v == 0. for v in shrink) and all(v == lam[0] for v in lam):
            kinds.append(('tile', lam[0]))
        else:
            kinds.append(('noise', 0.))
    return tables, kinds


def tile_noise_lds(cell, P, edge=None):
    """The bytes of LDS a ``consistency_row_noise`` launch plans for ``cell``: the fused joint launch (``edge`` None; ``P`` taps,
    four box arrays, 2 n^2 table floats) or the per-window launch on cubes of edge ``edge`` (three box arrays clipped to the cube).
    The entries refuse a plan above 65536 with DIQT_E_SHAPE."""
    fz, fy, fx = cell
    by, bx = fy * -(-4 // (fz * fy)), fx * -(-64 // fx)
    n = fz * fy * fx
    if edge is None:
        return 4 * (int(P) + 4 * fz * by * bx + 2 * n * n)
    return 4 * (3 * fz * min(by, edge) * min(bx, edge) + 2 * n * n)


def tile_noise_plan(who, cell, P, edge=None):
    """``ValueError`` naming "consistency_row_noise" for a cell whose launch plan exceeds 64 KiB of LDS (``tile_noise_lds``)."""
    need = tile_noise_lds(cell, P, edge)
    if need > 65536:
        raise ValueError(f"{who}: consistency_row_noise with the cell {tuple(cell)} plans {need} bytes of LDS (the box arrays and two "
                         f"{cell[0] * cell[1] * cell[2]}^2 tables), above the 65536 a launch may have")


def _tile_noise_tables(who, tables, cell, like, device=True):
    """The check of one step's ``tile_noise_tables`` handed to a kernel: fp32 [2, n, n], contiguous, on ``like``'s device
    (``device`` False: the shape rules only)."""
    n = cell[0] * cell[1] * cell[2]
    if not torch.is_tensor(tables) or tables.dtype != torch.float32 or tuple(tables.shape) != (2, n, n) or not tables.is_contiguous():
        raise ValueError(f"{who}: the consistency_row_noise tables of a step must be a contiguous fp32 [2, {n}, {n}] tensor "
                         f"(ops.tile_noise_tables), got "
                         f"{(tables.dtype, tuple(tables.shape)) if torch.is_tensor(tables) else type(tables).__name__}")
    if tables.device != like.device:
        raise ValueError(f"{who}: the consistency_row_noise tables are on {tables.device}, the data on {like.device}")
    if device:
        _chk(tables)


def tile_project_noise(x0, target, noise, cell, tables_i, clamp=None, out=None, out_noise=None):
    """One step's projection of ``consistency_row_noise`` (include/diqt.h, diqt_tile_project_noise): ``target`` [B,C,P,P,P] = windows
    of t, ``noise`` the step's normals, a tensor of ``x0``'s shape, ``tables_i`` [2, n, n] = (M_i, G_i) of this step on ``x0``'s
    device.  a = clamp(x0); per tile x0' = a + M_i (t - a) and noise' = noise - G_i noise (never clamped).  ``out`` / ``out_noise``:
    where they go (``x0`` / ``noise`` themselves for in place; None: new tensors -- a caller's noise tensor is never modified unless
    it is handed in as ``out_noise``).  Returns ``(x0', noise')``.  One launch."""
    who = "tile_project_noise"
    if torch.is_tensor(x0) and x0.ndim == 5:                              # the cell's and the tables' own rules first: they need no device
        _tile_noise_tables(who, tables_i, consistency_cell(who, cell, 1.0, [(x0.shape[2], a) for a in range(3)])[0], x0, device=False)

    def own(cell, w, P):
        _tile_noise_tables(who, tables_i, cell, x0)
        tile_noise_plan(who, cell, 0, P)
        return (noise, tables_i), ()
    return _project(who, "diqt_tile_project_noise", x0, target, 'target', cell, 1.0, clamp, out, own, noise, out_noise, shaped=True)


def volume_joint_consistent_tile_noise_step(y, slot, taps, x_t, x0_prev, meas_up, cell, tables_i, form, kx, k0, kp, kn, lo, hi,
                                            clamp_mode, stride, seed=0, draw=0, sample=0, out=None, x0_out=None):
    """``volume_joint_consistent_tile_step`` for ``consistency_row_noise`` (include/diqt.h,
    diqt_volume_joint_consistent_tile_noise_step): ``meas_up`` [D,H,W] = t in state space, ``tables_i`` [2, n, n] = (M_i, G_i) of this
    step on ``x_t``'s device.  Every tile whose voxels are ALL covered has its fused x0 moved to x0 + M_i (t - x0) and its normals to
    eps - G_i eps before the update; a tile with an uncovered voxel keeps both.  ``form`` 0 or 2 with ``kn != 0`` only.  The normals
    are the plain launch's (same key, same draw number).  Returns ``(out, x0_out)``.  One launch, bit-reproducible."""
    who = "volume_joint_consistent_tile_noise_step"
    form = _joint_form(who, form, noisy=True)
    if float(kn) == 0.0:
        raise ValueError(f"{who}: kn == 0: a step without a normal has no consistency_row_noise shaping")

    def own(cell, w, P):
        _tile_noise_tables(who, tables_i, cell, x_t)
        tile_noise_plan(who, cell, P)
        return (meas_up, tables_i), ()
    return _joint_consistent(who, "diqt_volume_joint_consistent_tile_noise_step", y, slot, taps, x_t, x0_prev, meas_up, cell, 1.0, form,
                             (kx, k0, kp, kn), lo, hi, clamp_mode, stride, seed, draw, sample, out, x0_out, own)


def volume_joint_heun_init(shape, sigma0, kc, seed, draw=0, sample=0, device=None):
    """The first ``images_hat`` of a joint Heun chain (phase 0 of ``diqt_volume_joint_heun``): fp32 [D,H,W],
    ``(sigma0 n(draw)) + kc n(draw + 1)`` with n the volume-anchored normals of channel 0 -- the initial image as
    ``ElucidatedImagen.one_unet_sample`` stores it, then the churn of step 0."""
    return _joint_initial("volume_joint_heun_init", "diqt_volume_joint_heun", lambda out: (None, None, None, out, None, None, 0, 0),
                          (sigma0, 0.0, 0.0, 0.0, kc, 0.0, 0.0), shape, "shape must be", seed, draw, sample, device, draws=2)


def volume_joint_heun(y, slot, taps, xh, xn, x0, phase, coefs, kc, lo, hi, clamp_mode, stride, seed=0, draw=0, sample=0):
    """The predictor (``phase`` 1) or the corrector with the next churn (``phase`` 2) of the stochastic Heun sampler on the joint state
    of a whole volume (include/diqt.h, diqt_volume_joint_heun), IN PLACE on the three [D,H,W] volumes ``xh`` (images_hat), ``xn``
    (images_next) and ``x0`` (the fused prediction).  ``y`` / ``slot`` / ``taps`` / ``stride`` / the clamp as in ``volume_joint_step``.
    Phase 1, ``coefs = (a, b)``: x0 = the weighted mean of the clamped predictions, xn = a xh + b x0.  Phase 2, ``coefs = (a, b, c, d)``:
    x = (a xh + b x0 + c xn) + d x0b with x0b the weighted mean, then xh = x + kc n with n the volume-anchored normal of (seed, draw,
    sample) (xh = x when ``kc`` is 0) and x0 = x0b.  Uncovered voxels: phase 1 copies xh to xn, phase 2 leaves xh; both write x0 = 0.
    Returns ``(xh, xn, x0)``.  One launch, bit-reproducible."""
    phase = int(phase)
    if phase not in (1, 2):
        raise ValueError(f"volume_joint_heun: phase must be 1 (predictor) or 2 (corrector), got {phase!r}; phase 0 is volume_joint_heun_init")
    N, P, stride = _joint_windows("volume_joint_heun", y, slot, taps, xh, clamp_mode, stride)
    seed, draw, sample = _noise_key("volume_joint_heun", seed, draw, sample)
    _joint_slots("volume_joint_heun", slot, N)
    coefs = tuple(float(v) for v in coefs)
    if len(coefs) != 2 * phase:
        raise ValueError(f"volume_joint_heun: phase {phase} takes {2 * phase} coefficients, got {len(coefs)}")
    for t, name in ((xn, 'xn'), (x0, 'x0')):
        _chk(t)
        if t.shape != xh.shape or not t.is_contiguous():
            raise ValueError(f"volume_joint_heun: {name} must be a contiguous tensor of xh's shape")
    if len({xh.data_ptr(), xn.data_ptr(), x0.data_ptr()}) != 3:
        raise ValueError("volume_joint_heun: xh, xn and x0 are three different volumes")
    _lib.call("diqt_volume_joint_heun", y if N else None, slot, taps, xh, xn, x0, phase, N, *xh.shape, P, stride, *slot.shape,
              *(coefs + (0.0, 0.0))[:4], float(kc) if phase == 2 else 0.0, float(lo), float(hi), int(clamp_mode), seed, draw, sample,
              _stream())
    return xh, xn, x0


JOINT_HEUN_MODES = {'cell': 0, 'profile': 1, 'tile': 2}          # ``mode`` of diqt_volume_joint_consistent_heun


def volume_joint_consistent_heun_lds(cell, P, mode):
    """The bytes of LDS ``volume_joint_consistent_heun`` plans: ``P`` taps, the two box arrays of ``cell`` and the mode's table
    (2 n floats of a profile, n^2 of a tile operator).  The entry refuses a plan above 65536 with DIQT_E_SHAPE."""
    fz, fy, fx = cell
    by, bx = fy * -(-4 // (fz * fy)), fx * -(-64 // fx)
    n = fz * fy * fx
    return 4 * (int(P) + 2 * fz * by * bx + {'cell': 0, 'profile': 2 * n, 'tile': n * n}[mode])


def volume_joint_consistent_heun(y, slot, taps, xh, xn, x0, meas_up, cell, table, weight, phase, coefs, kc, lo, hi, clamp_mode, stride,
                                 seed=0, draw=0, sample=0, mode='cell'):
    """``volume_joint_heun`` with the data-consistency projection between the fuse and the update (include/diqt.h,
    diqt_volume_joint_consistent_heun), IN PLACE on ``xh``, ``xn`` and ``x0`` as there.  ``mode`` ``'cell'`` (``table`` None),
    ``'profile'`` (``table`` [2, n] = ``cell_profile``'s) or ``'tile'`` (``table`` [n, n] = ``tile_operator``'s P and ``meas_up`` =
    t); ``meas_up`` [D,H,W] in state space, ``cell`` = (fz, fy, fx) dividing the volume, ``weight`` in (0, 1].  Every cell whose voxels
    are all covered has this phase's fused prediction replaced by x0 + weight A+(y - A x0) before the update -- phase 1: x0 = x0', xn
    = a xh + b x0'; phase 2: x = (a xh + b x0 + c xn) + d x0b', xh = x + kc n, x0 = x0b' -- a cell with an uncovered voxel and the
    uncovered voxels are the plain launch's.  ``phase``, ``coefs``, ``kc``, the clamp and the noise key as in ``volume_joint_heun``.
    Returns ``(xh, xn, x0)``.  One launch, bit-reproducible."""
    who = "volume_joint_consistent_heun"
    phase = int(phase)
    if phase not in (1, 2):
        raise ValueError(f"{who}: phase must be 1 (predictor) or 2 (corrector), got {phase!r}; phase 0 is volume_joint_heun_init")
    if mode not in JOINT_HEUN_MODES:
        raise ValueError(f"{who}: mode must be 'cell', 'profile' or 'tile', got {mode!r}")
    N, P, stride = _joint_windows(who, y, slot, taps, xh, clamp_mode, stride)
    seed, draw, sample = _noise_key(who, seed, draw, sample)
    _joint_slots(who, slot, N)
    cell, weight = consistency_cell(who, cell, weight, [(s, a) for a, s in enumerate(xh.shape)])
    coefs = tuple(float(v) for v in coefs)
    if len(coefs) != 2 * phase:
        raise ValueError(f"{who}: phase {phase} takes {2 * phase} coefficients, got {len(coefs)}")
    for t, name in ((xn, 'xn'), (x0, 'x0'), (meas_up, 'meas_up')):
        _chk(t)
        if t.shape != xh.shape or not t.is_contiguous():
            raise ValueError(f"{who}: {name} must be a contiguous tensor of xh's shape")
    if len({xh.data_ptr(), xn.data_ptr(), x0.data_ptr(), meas_up.data_ptr()}) != 4:
        raise ValueError(f"{who}: xh, xn, x0 and meas_up are four different volumes")
    if mode == 'cell':
        if table is not None:
            raise ValueError(f"{who}: mode 'cell' takes no table")
    else:
        (_cell_table if mode == 'profile' else _tile_table)(who, table, cell, xh)
    need = volume_joint_consistent_heun_lds(cell, P, mode)
    if need > 65536:
        raise ValueError(f"{who}: the consistency cell {cell} with windows of edge {P} plans {need} bytes of LDS (the taps, two box "
                         f"arrays and the table), above the 65536 a launch may have")
    _lib.call("diqt_volume_joint_consistent_heun", y if N else None, slot, taps, xh, xn, x0, meas_up, table, phase, JOINT_HEUN_MODES[mode],
              N, *xh.shape, P, stride, *slot.shape, *cell, weight, *(coefs + (0.0, 0.0))[:4], float(kc) if phase == 2 else 0.0, float(lo),
              float(hi), int(clamp_mode), seed, draw, sample, _stream())
    return xh, xn, x0


def _chk_mask(who, mask, like):
    if not mask.is_cuda:
        raise RuntimeError(f"diffusioniqt_amd.ops.{who} runs on the MI355X only (no CPU fallback); the mask is a CPU tensor")
    if mask.dtype not in (torch.uint8, torch.bool) or tuple(mask.shape) != tuple(like.shape) or not mask.is_contiguous():
        raise ValueError(f"{who}: mask must be a contiguous uint8 or bool tensor of shape {tuple(like.shape)}, got {mask.dtype} "
                         f"{tuple(mask.shape)}")


def edm_inpaint_churn(x, renoise, known, mask, eps, kr, kc, out=None):
    """One pass boundary of the EDM inpainting loop on a window batch (include/diqt.h, diqt_edm_inpaint_churn): ``x`` [B, ...] the state,
    ``renoise`` the re-noise normals of the pass that just ended (None: no re-noise, ``kr`` may be None too), ``known`` the known image in
    state space, ``mask`` one byte per element (uint8 or bool; non-zero: known), ``eps`` the churn normals, ``kr`` / ``kc`` device [B].
    out = sel(mask, known, x + kr renoise) + kc eps with the roundings of the two ``axpby3`` calls it replaces.  ``out``: where it goes
    (``x`` itself for an in-place pass; None: a new tensor).  Returns ``out``.  One launch."""
    _chk(x, renoise, known, eps, kr, kc, out)
    if x.ndim < 2 or x.numel() == 0:
        raise ValueError(f"edm_inpaint_churn: x must be a non-empty [B, ...] tensor, got {tuple(x.shape)}")
    B = x.shape[0]
    if B > 65535:
        raise ValueError(f"edm_inpaint_churn: at most 65535 samples per launch, got {B}")
    if out is None:
        out = torch.empty_like(x)
    for t, name in ((renoise, 'renoise'), (known, 'known'), (eps, 'eps'), (out, 'out')):
        if t is not None and t.shape != x.shape:
            raise ValueError(f"edm_inpaint_churn: {name} must have x's shape {tuple(x.shape)}, got {tuple(t.shape)}")
    _chk_mask("edm_inpaint_churn", mask, x)
    if renoise is not None and kr is None:
        raise ValueError("edm_inpaint_churn: a re-noise needs its coefficients kr")
    for t, name in ((kr, 'kr'), (kc, 'kc')):
        if t is not None and tuple(t.shape) != (B,):
            raise ValueError(f"edm_inpaint_churn: {name} must be a [B] = [{B}] tensor, got {tuple(t.shape)}")
    _lib.call("diqt_edm_inpaint_churn", x, renoise, known, mask, eps, kr, kc, out, B, x.numel() // B, _stream())
    return out


def _joint_known(who, known, mask, shape):
    _chk(known)
    if tuple(known.shape) != tuple(shape):
        raise ValueError(f"{who}: known must be a [D,H,W] = {tuple(shape)} volume, got {tuple(known.shape)}")
    _chk_mask(who, mask, known)


def volume_joint_heun_inpaint_init(known, mask, sigma0, kc, seed, draw=0, sample=0):
    """The first ``images_hat`` of a joint Heun chain that inpaints (phase 0 of ``diqt_volume_joint_heun_inpaint``): a new fp32 [D,H,W]
    volume, ``sel(mask, known, sigma0 n(draw)) + kc n(draw + 1)`` -- ``volume_joint_heun_init`` with the known volume (in state space,
    fp32 [D,H,W]) pasted under ``mask`` (uint8 or bool [D,H,W]) before the churn of step 0."""
    _joint_known("volume_joint_heun_inpaint_init", known, mask, known.shape)      # the mask against known; the shape itself below
    return _joint_initial("volume_joint_heun_inpaint_init", "diqt_volume_joint_heun_inpaint",
                          lambda out: (None, None, None, out, None, None, known, mask, 0, 0), (sigma0, 0.0, 0.0, 0.0, 0.0, kc, 0.0, 0.0),
                          known.shape, "known must be", seed, draw, sample, known.device, draws=2, more_draws=(0,))


def volume_joint_heun_inpaint(y, slot, taps, xh, xn, x0, known, mask, phase, coefs, kr, kc, lo, hi, clamp_mode, stride, seed=0, draw=0,
                              draw_r=0, sample=0):
    """The corrector (``phase`` 2) or the re-churn (``phase`` 3) of a joint Heun chain that inpaints (include/diqt.h,
    diqt_volume_joint_heun_inpaint), IN PLACE on ``xh`` and ``x0``; the predictor is ``volume_joint_heun(phase=1)``.  ``known`` fp32
    [D,H,W] in state space, ``mask`` uint8 or bool [D,H,W].  Phase 2, ``coefs = (a, b, c, d)``: ``volume_joint_heun``'s corrector up to
    x, then x += kr n(draw_r) where ``kr != 0`` (the re-noise of a pass that is not the last of its step), then
    xh = sel(mask, known, x) + kc n(draw) and x0 = the fused prediction.  Phase 3 (``y`` / ``slot`` / ``taps`` may be None, ``coefs``
    empty): xh = sel(mask, known, xn) + kc n(draw) at every voxel -- the further passes of the step that ends at sigma 0.
    Returns ``(xh, xn, x0)``.  One launch, bit-reproducible."""
    who = "volume_joint_heun_inpaint"
    phase = int(phase)
    if phase not in (2, 3):
        raise ValueError(f"{who}: phase must be 2 (corrector) or 3 (re-churn), got {phase!r}; phase 0 is volume_joint_heun_inpaint_init "
                         f"and the predictor volume_joint_heun(phase=1)")
    seed, draw, sample = _noise_key(who, seed, draw, sample)
    draw_r = _noise_key(who, seed, draw_r, sample)[1]
    coefs = tuple(float(v) for v in coefs)
    if len(coefs) != (4 if phase == 2 else 0):
        raise ValueError(f"{who}: phase {phase} takes {4 if phase == 2 else 0} coefficients, got {len(coefs)}")
    _chk(xh)
    if xh.ndim != 3:
        raise ValueError(f"{who}: xh must be a [D,H,W] volume")
    for t, name in ((xn, 'xn'), (x0, 'x0')):
        _chk(t)
        if t.shape != xh.shape or not t.is_contiguous():
            raise ValueError(f"{who}: {name} must be a contiguous tensor of xh's shape")
    if len({xh.data_ptr(), xn.data_ptr(), x0.data_ptr()}) != 3:
        raise ValueError(f"{who}: xh, xn and x0 are three different volumes")
    _joint_known(who, known, mask, xh.shape)
    if phase == 3:
        _lib.call("diqt_volume_joint_heun_inpaint", None, None, None, xh, xn, x0, known, mask, 3, 0, *xh.shape, 0, 0, 0, 0, 0, 0.0, 0.0,
                  0.0, 0.0, 0.0, float(kc), 0.0, 0.0, 0, seed, draw, 0, sample, _stream())
        return xh, xn, x0
    N, P, stride = _joint_windows(who, y, slot, taps, xh, clamp_mode, stride)
    _joint_slots(who, slot, N)
    _lib.call("diqt_volume_joint_heun_inpaint", y if N else None, slot, taps, xh, xn, x0, known, mask, 2, N, *xh.shape, P, stride,
              *slot.shape, *coefs, float(kr), float(kc), float(lo), float(hi), int(clamp_mode), seed, draw, draw_r, sample, _stream())
    return xh, xn, x0


def ddpm_inpaint_paste(x, renoise, known, mask, qnoise, kr0, kr1, al, sg, out=None):
    """One pass boundary of the DDPM inpainting loop on a window batch (include/diqt.h, diqt_ddpm_inpaint_paste): ``x`` [B, ...] the
    state, ``renoise`` the re-noise normals of the pass that just ended (None: no re-noise, ``kr0`` / ``kr1`` may be None too), ``known``
    the known image in state space, ``mask`` one byte per element (uint8 or bool; non-zero: known), ``qnoise`` the normals of the known
    image's forward sample, ``kr0`` / ``kr1`` / ``al`` / ``sg`` device [B].  out = sel(mask, al known + sg qnoise, kr0 x + kr1 renoise)
    with the roundings of the ``axpby3``, ``q_sample`` and ``mask_blend`` calls it replaces.  ``out``: where it goes (``x`` itself for an
    in-place pass; None: a new tensor).  Returns ``out``.  One launch."""
    who = "ddpm_inpaint_paste"
    _chk(x, renoise, known, qnoise, kr0, kr1, al, sg, out)
    if x.ndim < 2 or x.numel() == 0:
        raise ValueError(f"{who}: x must be a non-empty [B, ...] tensor, got {tuple(x.shape)}")
    B = x.shape[0]
    if B > 65535:
        raise ValueError(f"{who}: at most 65535 samples per launch, got {B}")
    if out is None:
        out = torch.empty_like(x)
    for t, name in ((renoise, 'renoise'), (known, 'known'), (qnoise, 'qnoise'), (out, 'out')):
        if t is not None and t.shape != x.shape:
            raise ValueError(f"{who}: {name} must have x's shape {tuple(x.shape)}, got {tuple(t.shape)}")
    _chk_mask(who, mask, x)
    if renoise is not None and (kr0 is None or kr1 is None):
        raise ValueError(f"{who}: a re-noise needs its coefficients kr0 and kr1")
    for t, name in ((kr0, 'kr0'), (kr1, 'kr1'), (al, 'al'), (sg, 'sg')):
        if t is not None and tuple(t.shape) != (B,):
            raise ValueError(f"{who}: {name} must be a [B] = [{B}] tensor, got {tuple(t.shape)}")
    _lib.call("diqt_ddpm_inpaint_paste", x, renoise, known, mask, qnoise, kr0, kr1, al, sg, out, B, x.numel() // B, _stream())
    return out


def volume_joint_step_inpaint_init(known, mask, al, sg, seed, draw=0, draw_q=1, sample=0):
    """The first state of a joint first-order chain that inpaints (phase 0 of ``diqt_volume_joint_step_inpaint``): a new fp32 [D,H,W]
    volume, ``sel(mask, al known + sg n(draw_q), n(draw))`` -- ``volume_joint_init`` under the first paste of the known volume (in state
    space, fp32 [D,H,W]; ``mask`` uint8 or bool [D,H,W])."""
    who = "volume_joint_step_inpaint_init"
    _joint_known(who, known, mask, known.shape)              # the mask against known; the shape itself below
    draw_q = _noise_key(who, seed, draw_q, sample)[1]
    return _joint_initial(who, "diqt_volume_joint_step_inpaint", lambda out: (None, None, None, out, None, known, mask, 0, 0, 0),
                          (0.0, 0.0, 0.0, 0.0, 0.0, al, sg, 0.0, 0.0), known.shape, "known must be", seed, draw, sample, known.device,
                          more_draws=(0, draw_q))


def volume_joint_step_inpaint(y, slot, taps, x, known, mask, flags, kx, k0, kn, kr, q, lo, hi, clamp_mode, stride, seed, draw, draw_r=0,
                              draw_q=0, sample=0, x0_out=None):
    """One pass of a joint first-order chain that inpaints (include/diqt.h, diqt_volume_joint_step_inpaint, phase 1), IN PLACE on the
    state ``x`` [D,H,W]: ``volume_joint_step``'s u = kx x + k0 x0 + kn n(draw) on covered voxels; with ``flags`` bit 0
    u = kr[0] u + kr[1] n(draw_r), the re-noise that ends a pass; with bit 1 x = sel(mask, q[0] known + q[1] n(draw_q), u), the paste
    that begins the next pass (``q`` = the (alpha, sigma) of that pass's step), else x = u.  ``known`` fp32 [D,H,W] in state space,
    ``mask`` uint8 or bool [D,H,W]; ``x0_out`` (optional [D,H,W]) receives the fused x0 (0 where uncovered).  Uncovered voxels keep
    ``x``.  Returns ``x``.  One launch, bit-reproducible."""
    who = "volume_joint_step_inpaint"
    flags = int(flags)
    if flags not in (0, 1, 2, 3):
        raise ValueError(f"{who}: flags must be 0 .. 3 (bit 0: re-noise, bit 1: paste), got {flags!r}")
    N, P, stride = _joint_windows(who, y, slot, taps, x, clamp_mode, stride)
    seed, draw, sample = _noise_key(who, seed, draw, sample)
    draw_r, draw_q = (_noise_key(who, seed, d, sample)[1] for d in (draw_r, draw_q))
    _joint_slots(who, slot, N)
    _, x0_out = _joint_volumes(who, x, None, x, x0_out, need_x0=False)
    _joint_known(who, known, mask, x.shape)
    (kr0, kr1), (al, sg) = (float(v) for v in kr), (float(v) for v in q)
    _lib.call("diqt_volume_joint_step_inpaint", y if N else None, slot, taps, x, x0_out, known, mask, 1, flags, N, *x.shape, P, stride,
              *slot.shape, float(kx), float(k0), float(kn), kr0, kr1, al, sg, float(lo), float(hi), int(clamp_mode), seed, draw, draw_r,
              draw_q, sample, _stream())
    return x


def volume_joint_finish(x, slot, vol, P, stride, mean, std, min_val, fill, s, S, mean_io=None, m2_io=None, want_std=False):
    """The end of sample ``s`` of ``S`` joint chains (include/diqt.h, diqt_volume_joint_finish): the finished state ``x`` [D,H,W] with
    ``fill`` where no kept window of ``slot`` covers and ``min_val`` on the background of the raw ``vol`` enters the running Welford
    pair ``(mean_io, m2_io)`` (made here for sample 0, otherwise the pair the previous call returned; ``m2_io`` exists for S >= 2 only).
    Returns ``(mean_io, m2_io, std)`` with ``std`` the unbiased deviation map after the last sample when ``want_std``, else None."""
    _chk(x, vol)
    if x.ndim != 3 or x.shape != vol.shape or not (x.is_contiguous() and vol.is_contiguous()):
        raise ValueError("volume_joint_finish: x and vol must be contiguous [D,H,W] tensors of one shape")
    stride = _joint_lattice("volume_joint_finish", slot, x.shape, int(P), stride)
    s, S = int(s), int(S)
    if not 0 <= s < S:
        raise ValueError(f"volume_joint_finish: sample {s} of {S}")
    if want_std and S < 2:
        raise ValueError("volume_joint_finish: a deviation map needs at least 2 samples")
    if s == 0:
        mean_io = torch.empty_like(x)
        m2_io = torch.empty_like(x) if S > 1 else None
    else:
        if mean_io is None or m2_io is None:
            raise ValueError("volume_joint_finish: samples after the first continue the (mean_io, m2_io) pair of the previous call")
        _chk(mean_io, m2_io)
        if mean_io.shape != x.shape or m2_io.shape != x.shape or not (mean_io.is_contiguous() and m2_io.is_contiguous()):
            raise ValueError("volume_joint_finish: mean_io / m2_io must be contiguous tensors of x's shape")
    dev = torch.empty_like(x) if want_std and s == S - 1 else None
    _lib.call("diqt_volume_joint_finish", x, slot, vol, mean_io, m2_io, dev, s, S, *x.shape, int(P), stride, *slot.shape, float(mean),
              float(std), float(min_val), float(fill), _stream())
    return mean_io, m2_io, dev


def patch_pair_crop(lr_vols, hr_vols, sel, P, mode, mean, std):
    """data.py:119-132: crop + normalise ``sel[n] = (volume, i0, j0, k0)`` patch pairs out of the HBM-resident [V,D,H,W]
    volume stacks in one launch.  Returns (lr [n,P,P,P], hr [n,P,P,P])."""
    _chk(lr_vols, hr_vols)
    V, D, H, W = lr_vols.shape
    n = sel.shape[0]
    lr = torch.empty(n, P, P, P, device=lr_vols.device, dtype=torch.float32)
    hr = torch.empty_like(lr)
    nws = _lib.query("diqt_patch_pair_crop_workspace_bytes", n, P) if mode == 1 else 0
    ws = _workspace(nws, lr_vols.device) if nws else None
    _lib.call("diqt_patch_pair_crop", lr_vols, hr_vols, sel, lr, hr, ws, nws, n, V, D, H, W, P, int(mode), float(mean), float(std),
              _stream())
    return lr, hr


def minmax(x):
    """Device [2] tensor {min, max} of x (no host sync)."""
    _chk(x)
    out = torch.empty(2, device=x.device, dtype=torch.float32)
    _lib.call("diqt_minmax", x, x.numel(), _workspace(8192, x.device), out, _stream())
    return out


def psnr(pred, target, stats=None, data_range=1.0):
    """Device [2] tensor {mse, PSNR}; ``stats`` = device [4] {pred min, max, target min, max} for min-max normalisation."""
    _chk(pred, target)
    out = torch.empty(2, device=pred.device, dtype=torch.float32)
    _lib.call("diqt_psnr", pred, target, pred.numel(), stats, float(data_range), _workspace(8192, pred.device), out, _stream())
    return out


def ssim3d(pred, target, taps, stats=None, data_range=1.0, k1=0.01, k2=0.03):
    """pred/target: contiguous [N, D, H, W]; taps: host float32 numpy array (odd length <= 11).  Device [1] tensor."""
    import ctypes
    _chk(pred, target)
    N, D, H, W = pred.shape
    K = int(taps.shape[0])
    nws = _lib.query("diqt_ssim3d_workspace_bytes", N, D, H, W, K)
    if nws == 0:
        raise RuntimeError(f"ssim3d: volume {D}x{H}x{W} smaller than the {K}-tap filter")
    out = torch.empty(1, device=pred.device, dtype=torch.float32)
    _lib.call("diqt_ssim3d", pred, target, N, D, H, W, taps.ctypes.data_as(ctypes.c_void_p), K, stats, float(data_range), float(k1),
              float(k2), _workspace(nws, pred.device), nws, out, _stream())
    return out


def msssim3d(pred, target, taps, betas, k1=0.01, k2=0.03):
    """pred/target: contiguous [N, D, H, W]; taps: host float32 numpy array (odd length <= 11); betas: one exponent per scale.
    Device [1 + 3 * scales] tensor {MS-SSIM, then per scale ssim_s, cs_s, range_s}; nothing is synchronised or copied back."""
    import ctypes
    import numpy as np
    _chk(pred, target)
    if pred.shape != target.shape:
        raise RuntimeError(f"msssim3d: shapes differ: {tuple(pred.shape)} vs {tuple(target.shape)}")
    N, D, H, W = pred.shape
    taps = np.ascontiguousarray(taps, dtype=np.float32)
    betas = np.ascontiguousarray(betas, dtype=np.float32)
    K, scales = int(taps.shape[0]), int(betas.shape[0])
    nws = _lib.query("diqt_msssim3d_workspace_bytes", N, D, H, W, K, scales)
    if nws == 0:
        raise RuntimeError(f"msssim3d: volume {D}x{H}x{W} leaves fewer than {K} voxels on an axis after {scales - 1} poolings "
                           f"(or scales = {scales} outside 1..16)")
    out = torch.empty(1 + 3 * scales, device=pred.device, dtype=torch.float32)
    _lib.call("diqt_msssim3d", pred, target, N, D, H, W, taps.ctypes.data_as(ctypes.c_void_p), K,
              betas.ctypes.data_as(ctypes.c_void_p), scales, float(k1), float(k2), _workspace(nws, pred.device), nws, out, _stream())
    return out
