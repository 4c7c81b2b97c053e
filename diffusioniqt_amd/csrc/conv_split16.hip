// fp32 3x3x3 forward convs on the fp16 matrix pipe by the three-product split (round 8):
//     xh = fp16(x)   xl = fp16((x - xh) 2^11)        wh = fp16(w)   wl = fp16((w - wh) 2^11)
//     x w ~= xh wh + 2^-11 (xh wl + xl wh)            (products exact, sums in fp32 inside the MFMA; the tail x tail term is dropped)
// Three `v_mfma_f32_32x32x16_f16` stand in for sixteen f32 MFMAs at the same K.  This file holds
//   * the weight pack: conv_pack_weight_h_kernel's order [chunk][tap][co pad 64][32], a chunk = 16 input channels as
//     [16 heads | 16 scaled tails]; a weight with |w| >= 65504 (or not finite) refuses the route for that layer (`refused`);
//   * the activation pass: optional GroupNorm-apply (the coefficients of diqt_gn_coef_from_partials / diqt_groupnorm_stats_coef) and
//     Mish / SiLU / GELU in fp32, then the split, written NDHWC with 2 C 16-bit channels, per voxel and group of 16 channels
//     [16 heads | 16 scaled tails] = 64 B: a halo row of conv_f9h_kernel's LDS image.  Heads are clamped to +-65504 and the tail is
//     taken from the clamped head (and clamped too): a value beyond the fp16 range loses accuracy, no inf or NaN is made;
//   * the split build of conv_f9h_kernel (256-voxel tiles, one workgroup per CU: three accumulator sets of NVB = 4 tiles -- head x
//     head of the even and of the odd taps, the cross terms -- and a 3-slot weight ring, 498-512 registers without scratch in its four
//     residual x statistics instantiations; at NVB = 8 the allocator spills) and the entry points.
#include "conv_f9h_kernel.h"
#include <atomic>

namespace diqt {

constexpr int S16_CG = 16;                     // fp32 channels per 32-wide chunk of 16-bit channels
constexpr float S16_MAX = 65504.f, S16_SCALE = 2048.f;

__device__ __forceinline__ float s16_clamp(float v) { return v > S16_MAX ? S16_MAX : (v < -S16_MAX ? -S16_MAX : v); }   // (a NaN stays one)

__device__ __forceinline__ void s16_split(float v, _Float16& head, _Float16& tail) {
    head = (_Float16)s16_clamp(v);
    tail = (_Float16)s16_clamp((v - (float)head) * S16_SCALE);
}

// packed[((chunk * T + tap) * CoutPad + o) * 32 + k]: k < 16 the head, k >= 16 the scaled tail of w[o][chunk * 16 + (k & 15)][tap]
__global__ __launch_bounds__(256) void conv_pack_weight_split16_kernel(const float* __restrict__ w, unsigned short* __restrict__ packed,
                                                                       int* __restrict__ refused, int Cout, int Cin, int T, int CoutPad,
                                                                       size_t total) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int k = (int)(i % h9::CK);
        size_t r = i / h9::CK;
        const int o = (int)(r % CoutPad);
        r /= CoutPad;
        const int tap = (int)(r % T);
        const int in = (int)(r / T) * S16_CG + (k & (S16_CG - 1));
        float v = 0.f;
        if (o < Cout && in < Cin) v = w[((size_t)o * Cin + in) * T + tap];
        if (!(fabsf(v) < S16_MAX)) *refused = 1;
        _Float16 head, tail;
        s16_split(v, head, tail);
        packed[i] = __builtin_bit_cast(unsigned short, k < S16_CG ? head : tail);
    }
}

// x: fp32 [B][rows][C]; y: 16-bit [B][rows][C / 16][16 heads | 16 tails]; coef (GN): [2][B][C] = A, then Bc: v = act(A x + Bc).
// A thread takes 8 consecutive channels of a voxel: 32 B in, 16 B of heads and 16 B of tails out.
template <bool GN>
__global__ __launch_bounds__(256) void split16_act_kernel(const float* __restrict__ x, const float* __restrict__ coef, int act,
                                                          unsigned short* __restrict__ y, int B, unsigned rows, int C, size_t total8) {
    typedef _Float16 h8 __attribute__((ext_vector_type(8)));
    const unsigned c8n = (unsigned)C / 8u;
    for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < total8; i += (size_t)gridDim.x * 256) {
        const unsigned c8 = (unsigned)(i % c8n);
        const size_t vox = i / c8n;
        const float4 lo = reinterpret_cast<const float4*>(x)[2 * i], hi = reinterpret_cast<const float4*>(x)[2 * i + 1];
        float v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        if (GN) {
            const size_t bc = (vox / rows) * (size_t)C + 8u * c8;
            const float4 a0 = *reinterpret_cast<const float4*>(coef + bc), a1 = *reinterpret_cast<const float4*>(coef + bc + 4);
            const float4 b0 = *reinterpret_cast<const float4*>(coef + (size_t)B * C + bc), b1 = *reinterpret_cast<const float4*>(coef + (size_t)B * C + bc + 4);
            const float A[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w}, Bc[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = act_fwd(fmaf(A[e], v[e], Bc[e]), act);
        }
        h8 head, tail;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            _Float16 h, t;
            s16_split(v[e], h, t);
            head[e] = h; tail[e] = t;
        }
        unsigned short* row = y + vox * (size_t)(2 * C) + (size_t)(c8 >> 1) * 32u + (c8 & 1u) * 8u;
        *reinterpret_cast<h8*>(row) = head;
        *reinterpret_cast<h8*>(row + S16_CG) = tail;
    }
}

namespace h9 {

int launch_split(const void* x, const unsigned short* wp, const float* bias, const float* residual, void* y, const H9Geom& g, size_t lds,
                 unsigned grid, void* stream) {
    if (g.variant == 6) return launch_split_cfg<H9S_333_256>(x, wp, bias, residual, y, g, lds, grid, stream);
    if (g.variant == 7 || g.variant == 8) return launch_split_b(x, wp, bias, residual, y, g, lds, grid, stream);
    if (g.variant == 9) return launch_split_c(x, wp, bias, residual, y, g, lds, grid, stream);
    set_error("conv3d_fwd_split16(v9h): no variant %d", g.variant);
    return DIQT_E_UNSUPPORTED;
}

}  // namespace h9
}  // namespace diqt

using namespace diqt;

extern "C" int diqt_set_conv_f9h_mode(int mode);

// The route's plan: conv_f9h_kernel's planner on the doubled channel count, its split tiles -- and only launches of at least 128
// (tile, 64-channel block) units, half the chip (tests lift that with diqt_set_conv_f9h_mode(2)): below, the Winograd tile of
// conv_fwd9_kernel with split-K keeps the launch, and tiny networks keep their kernels and their bits.
static bool split16_plan(H9Geom& g, size_t& lds, unsigned& grid, int B, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw, int pd,
                         int ph, int pw, int epd, int eph, int epw) {
    if (Cin <= 0 || Cin % S16_CG != 0 || Cin > (1 << 20)) return false;
    if (!f9h_plan(g, lds, grid, B, D, H, W, 2 * Cin, Cout, kd, kh, kw, pd, ph, pw, epd, eph, epw, false, true)) return false;
    if (diqt_set_conv_f9h_mode(-1) != 2 && (long long)g.MT * g.nNt < 128) return false;
    // (the activation pass addresses x and its split copy with 64-bit offsets; the kernel's descriptors are checked by the planner)
    return true;
}

// 0 (default): the fill plan chooses its tile; 6, 7, 8: it takes that variant's tile whatever the unit counts say -- honoured only
// under diqt_set_conv_f9h_mode(2), for tests that run every tile on one shape.  v >= 0 sets it, v < 0 only queries; returns the
// previous value.
static std::atomic<int> g_fill_tile{0};
extern "C" int diqt_set_conv_split16_fill_tile(int v) {
    if (v < 0) return g_fill_tile.load();
    return g_fill_tile.exchange(v == 6 || v == 7 || v == 8 ? v : 0);
}

// The fill plan (round 10): the same route for launches whose 256-voxel tiles leave CUs without a workgroup.  Candidates are the 256-,
// 128- and 64-voxel tiles in that order; a smaller tile is tried only when the larger gives fewer than 256 (tile, 64-channel block)
// units, the tiling taken must give at least 128, and the launch must hold at least 2^25 voxel x Cin x Cout products: below, the launch
// keeps its kernel (and the tiny networks of the parity and launch-trace suites their bits).  diqt_set_conv_f9h_mode(2) lifts both floors.
static bool split16_fill_plan(H9Geom& g, size_t& lds, unsigned& grid, int B, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw,
                              int pd, int ph, int pw, int epd, int eph, int epw) {
    if (Cin <= 0 || Cin % S16_CG != 0 || Cin > (1 << 20)) return false;
    const bool lifted = diqt_set_conv_f9h_mode(-1) == 2;
    const int forced = lifted ? g_fill_tile.load() : 0;
    bool have = false;
    for (int v = 6; v <= 8; ++v) {
        if (forced && v != forced) continue;
        H9Geom t; size_t l; unsigned gr;
        if (!f9h_plan(t, l, gr, B, D, H, W, 2 * Cin, Cout, kd, kh, kw, pd, ph, pw, epd, eph, epw, false, true, v)) continue;
        g = t; lds = l; grid = gr; have = true;
        if ((long long)t.MT * t.nNt >= 256) break;
    }
    if (!have) return false;
    if (!lifted) {
        if ((long long)g.MT * g.nNt < 128) return false;
        // sent back by measurement (round 10): 64-voxel tiles on less than the whole chip pay only up to Cin = 128.  Every workgroup pulls
        // its channel block's whole weight stream through L2 for 64 voxels, so the launch grows with Cin where the Winograd tile's
        // split-K spreads K over the chip: 256 -> 128 @ 8 x 8^3 (128 units) took 66.4 us against 61.3 us, 128 -> 128 39.9-41.3 against 43.7
        if (g.variant == 8 && (long long)g.MT * g.nNt < 256 && Cin > 128) return false;
        if ((unsigned long long)B * g.Do * g.Ho * g.Wo * (unsigned long long)Cin * (unsigned long long)Cout < (1ull << 25)) return false;
    }
    return true;
}

// The pair plan (round 11): the 256-voxel tile's launches on the tap-paired 16x16x32 body (variant 9: conv_split16_c.hip) -- the tiling,
// the statistics rows, x' and the packed weights of variant 6.  Granted where that tile fills the chip: at least 256 (tile, 64-channel
// block) units and 2^25 voxel x Cin x Cout products (diqt_set_conv_f9h_mode(2) lifts both floors).  In C2: 64 -> 64 and 128 -> 64 @
// 8 x 32^3, 128 -> 128 and 192 -> 128 @ 8 x 16^3.
static bool split16_pair_plan(H9Geom& g, size_t& lds, unsigned& grid, int B, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw,
                              int pd, int ph, int pw, int epd, int eph, int epw) {
    if (Cin <= 0 || Cin % S16_CG != 0 || Cin > (1 << 20)) return false;
    if (!f9h_plan(g, lds, grid, B, D, H, W, 2 * Cin, Cout, kd, kh, kw, pd, ph, pw, epd, eph, epw, false, true, 6)) return false;
    if (diqt_set_conv_f9h_mode(-1) != 2) {
        const long long units = (long long)g.MT * g.nNt;
        if (units < 256) return false;
        if ((unsigned long long)B * g.Do * g.Ho * g.Wo * (unsigned long long)Cin * (unsigned long long)Cout < (1ull << 25)) return false;
        // sent back by measurement (round 11): a workgroup whose walk is a single tile needs eight chunks to pay for the body's longer
        // prologue -- 64 -> 128 @ 8 x 16^3 (one tile of four chunks) took 54.9-55.8 us against 53.8-54.2 us on variant 6
        if (units <= (long long)grid && g.nChunks < 8) return false;
    }
    g.variant = 9;
    return true;
}

enum { S16_PLAN = 0, S16_FILL = 1, S16_PAIR = 2 };
static const char* const s16_suffix[3] = {"", "_fill", "_pair"};

static bool split16_any_plan(int plan, H9Geom& g, size_t& lds, unsigned& grid, int B, int D, int H, int W, int Cin, int Cout, int kd, int kh,
                             int kw, int pd, int ph, int pw, int epd, int eph, int epw) {
    if (plan == S16_PAIR) return split16_pair_plan(g, lds, grid, B, D, H, W, Cin, Cout, kd, kh, kw, pd, ph, pw, epd, eph, epw);
    return plan == S16_FILL ? split16_fill_plan(g, lds, grid, B, D, H, W, Cin, Cout, kd, kh, kw, pd, ph, pw, epd, eph, epw)
                            : split16_plan(g, lds, grid, B, D, H, W, Cin, Cout, kd, kh, kw, pd, ph, pw, epd, eph, epw);
}

static bool split16_act_ok(int act) { return act == 0 || act == DIQT_ACT_MISH || act == DIQT_ACT_SILU || act == DIQT_ACT_GELU; }

extern "C" size_t diqt_conv_packed_split16_elems(int Cout, int Cin, int kd, int kh, int kw) {
    if (Cout <= 0 || Cin <= 0 || kd <= 0 || kh <= 0 || kw <= 0) return 0;
    return (size_t)((Cin + S16_CG - 1) / S16_CG) * kd * kh * kw * ((Cout + 63) / 64 * 64) * h9::CK;
}

extern "C" int diqt_conv_pack_weight_split16(const float* w, void* packed, int* refused, int Cout, int Cin, int kd, int kh, int kw,
                                             void* stream) {
    DIQT_REQUIRE(w && packed && refused, DIQT_E_ALIGN, "conv_pack_weight_split16: null pointer");
    DIQT_REQUIRE(Cout > 0 && Cin > 0 && kd > 0 && kh > 0 && kw > 0, DIQT_E_SHAPE, "conv_pack_weight_split16: bad shape");
    const int T = kd * kh * kw, CoutPad = (Cout + 63) / 64 * 64;
    const size_t total = diqt_conv_packed_split16_elems(Cout, Cin, kd, kh, kw);
    hipError_t e = hipMemsetAsync(refused, 0, sizeof(int), (hipStream_t)stream);
    DIQT_REQUIRE(e == hipSuccess, DIQT_E_LAUNCH, "conv_pack_weight_split16: hipMemsetAsync: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(conv_pack_weight_split16_kernel, dim3(grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream, w,
                       static_cast<unsigned short*>(packed), refused, Cout, Cin, T, CoutPad, total);
    return check_launch("conv_pack_weight_split16");
}

extern "C" int diqt_conv3d_fwd_split16_supported(int B, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw, int pd, int ph, int pw,
                                                 int epd, int eph, int epw) {
    H9Geom g; size_t lds; unsigned grid;
    return split16_plan(g, lds, grid, B, D, H, W, Cin, Cout, kd, kh, kw, pd, ph, pw, epd, eph, epw) ? 1 : 0;
}

extern "C" int diqt_conv3d_fwd_gn_split16_supported(int B, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw, int pd, int ph,
                                                    int pw, int epd, int eph, int epw, int act) {
    return split16_act_ok(act) ? diqt_conv3d_fwd_split16_supported(B, D, H, W, Cin, Cout, kd, kh, kw, pd, ph, pw, epd, eph, epw) : 0;
}

// rows of column sums per batch entry a launch given `stats` writes ([B][rows][2][Cout]); 0: the route does not take the shape
extern "C" int diqt_conv3d_fwd_split16_stats_blocks(int B, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw, int pd, int ph,
                                                    int pw, int epd, int eph, int epw) {
    H9Geom g; size_t lds; unsigned grid;
    if (!split16_plan(g, lds, grid, B, D, H, W, Cin, Cout, kd, kh, kw, pd, ph, pw, epd, eph, epw)) return 0;
    return f9h_stats_blocks(g);
}

// the tile variant of that launch (6: H9S_333_256), -1: not taken
extern "C" int diqt_conv3d_fwd_split16_variant(int B, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw, int pd, int ph, int pw,
                                               int epd, int eph, int epw) {
    H9Geom g; size_t lds; unsigned grid;
    if (!split16_plan(g, lds, grid, B, D, H, W, Cin, Cout, kd, kh, kw, pd, ph, pw, epd, eph, epw)) return -1;
    return g.variant;
}

static int split16_run(const char* who, int plan, const float* x, void* x16, const void* packed, const float* bias, const float* residual, float* y,
                       float* stats, const float* coef, int act, int B, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw, int pd,
                       int ph, int pw, int epd, int eph, int epw, void* stream) {
    DIQT_REQUIRE(x && x16 && packed && y, DIQT_E_ALIGN, "%s: null pointer", who);
    DIQT_REQUIRE(aligned16(x) && aligned16(x16) && aligned16(packed) && aligned16(y) && (!residual || aligned16(residual)) &&
                 (!coef || aligned16(coef)), DIQT_E_ALIGN, "%s: tensors must be 16-byte aligned", who);
    DIQT_REQUIRE(split16_act_ok(act), DIQT_E_UNSUPPORTED, "%s: activation %d", who, act);
    H9Geom g; size_t lds; unsigned grid;
    DIQT_REQUIRE(split16_any_plan(plan, g, lds, grid, B, D, H, W, Cin, Cout, kd, kh, kw, pd, ph, pw, epd, eph, epw), DIQT_E_UNSUPPORTED,
                 "%s: shape not taken by the split route (diqt_conv3d_fwd_split16%s_supported == 0)", who, s16_suffix[plan]);
    const unsigned rows = (unsigned)D * H * W;
    const size_t total8 = (size_t)B * rows * (Cin / 8);
    if (coef)
        hipLaunchKernelGGL(split16_act_kernel<true>, dim3(grid_for(total8, 256)), dim3(256), 0, (hipStream_t)stream, x, coef, act,
                           static_cast<unsigned short*>(x16), B, rows, Cin, total8);
    else
        hipLaunchKernelGGL(split16_act_kernel<false>, dim3(grid_for(total8, 256)), dim3(256), 0, (hipStream_t)stream, x, coef, 0,
                           static_cast<unsigned short*>(x16), B, rows, Cin, total8);
    const int rc = check_launch("split16_act");
    if (rc != DIQT_OK) return rc;
    g.stats = stats;
    return f9h_launch_split(x16, static_cast<const unsigned short*>(packed), bias, residual, y, g, lds, grid, stream);
}

// y = conv3d(x) [+ residual]: x fp32 NDHWC, x16 a scratch of B D H W Cin * 4 bytes for the split copy, packed from
// diqt_conv_pack_weight_split16; stats: optional [B][diqt_conv3d_fwd_split16_stats_blocks][2][Cout]
extern "C" int diqt_conv3d_fwd_split16(const float* x, void* x16, const void* packed, const float* bias, const float* residual, float* y,
                                       float* stats, int B, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw, int pd, int ph,
                                       int pw, int epd, int eph, int epw, void* stream) {
    return split16_run("conv3d_fwd_split16", S16_PLAN, x, x16, packed, bias, residual, y, stats, nullptr, 0, B, D, H, W, Cin, Cout, kd, kh, kw, pd, ph, pw,
                       epd, eph, epw, stream);
}

// y = conv3d(act(A x + Bc)) [+ residual], coef = [2][B][Cin] (A, then Bc) as diqt_conv3d_fwd_gn takes them
extern "C" int diqt_conv3d_fwd_gn_split16(const float* x, void* x16, const void* packed, const float* bias, const float* residual, float* y,
                                          float* stats, const float* coef, int act, int B, int D, int H, int W, int Cin, int Cout, int kd,
                                          int kh, int kw, int pd, int ph, int pw, int epd, int eph, int epw, void* stream) {
    DIQT_REQUIRE(coef, DIQT_E_ALIGN, "conv3d_fwd_gn_split16: null coefficients");
    return split16_run("conv3d_fwd_gn_split16", S16_PLAN, x, x16, packed, bias, residual, y, stats, coef, act, B, D, H, W, Cin, Cout, kd, kh, kw, pd, ph, pw,
                       epd, eph, epw, stream);
}

// ---- the fill plan's queries and entry points: the arguments and meanings of their namesakes above, answered by split16_fill_plan ----
extern "C" int diqt_conv3d_fwd_split16_fill_supported(int B, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw, int pd, int ph,
                                                      int pw, int epd, int eph, int epw) {
    H9Geom g; size_t lds; unsigned grid;
    return split16_fill_plan(g, lds, grid, B, D, H, W, Cin, Cout, kd, kh, kw, pd, ph, pw, epd, eph, epw) ? 1 : 0;
}

extern "C" int diqt_conv3d_fwd_gn_split16_fill_supported(int B, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw, int pd, int ph,
                                                         int pw, int epd, int eph, int epw, int act) {
    return split16_act_ok(act) ? diqt_conv3d_fwd_split16_fill_supported(B, D, H, W, Cin, Cout, kd, kh, kw, pd, ph, pw, epd, eph, epw) : 0;
}

extern "C" int diqt_conv3d_fwd_split16_fill_stats_blocks(int B, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw, int pd, int ph,
                                                         int pw, int epd, int eph, int epw) {
    H9Geom g; size_t lds; unsigned grid;
    if (!split16_fill_plan(g, lds, grid, B, D, H, W, Cin, Cout, kd, kh, kw, pd, ph, pw, epd, eph, epw)) return 0;
    return f9h_stats_blocks(g);
}

// 6: H9S_333_256, 7: H9S_333_128, 8: H9S_333_64, -1: not taken
extern "C" int diqt_conv3d_fwd_split16_fill_variant(int B, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw, int pd, int ph,
                                                    int pw, int epd, int eph, int epw) {
    H9Geom g; size_t lds; unsigned grid;
    if (!split16_fill_plan(g, lds, grid, B, D, H, W, Cin, Cout, kd, kh, kw, pd, ph, pw, epd, eph, epw)) return -1;
    return g.variant;
}

extern "C" int diqt_conv3d_fwd_split16_fill(const float* x, void* x16, const void* packed, const float* bias, const float* residual, float* y,
                                            float* stats, int B, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw, int pd,
                                            int ph, int pw, int epd, int eph, int epw, void* stream) {
    return split16_run("conv3d_fwd_split16_fill", S16_FILL, x, x16, packed, bias, residual, y, stats, nullptr, 0, B, D, H, W, Cin, Cout, kd, kh, kw,
                       pd, ph, pw, epd, eph, epw, stream);
}

extern "C" int diqt_conv3d_fwd_gn_split16_fill(const float* x, void* x16, const void* packed, const float* bias, const float* residual,
                                               float* y, float* stats, const float* coef, int act, int B, int D, int H, int W, int Cin,
                                               int Cout, int kd, int kh, int kw, int pd, int ph, int pw, int epd, int eph, int epw,
                                               void* stream) {
    DIQT_REQUIRE(coef, DIQT_E_ALIGN, "conv3d_fwd_gn_split16_fill: null coefficients");
    return split16_run("conv3d_fwd_gn_split16_fill", S16_FILL, x, x16, packed, bias, residual, y, stats, coef, act, B, D, H, W, Cin, Cout, kd, kh,
                       kw, pd, ph, pw, epd, eph, epw, stream);
}

// ---- the pair plan's queries and entry points: the arguments and meanings of their namesakes above, answered by split16_pair_plan ----
extern "C" int diqt_conv3d_fwd_split16_pair_supported(int B, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw, int pd, int ph,
                                                      int pw, int epd, int eph, int epw) {
    H9Geom g; size_t lds; unsigned grid;
    return split16_pair_plan(g, lds, grid, B, D, H, W, Cin, Cout, kd, kh, kw, pd, ph, pw, epd, eph, epw) ? 1 : 0;
}

extern "C" int diqt_conv3d_fwd_gn_split16_pair_supported(int B, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw, int pd, int ph,
                                                         int pw, int epd, int eph, int epw, int act) {
    return split16_act_ok(act) ? diqt_conv3d_fwd_split16_pair_supported(B, D, H, W, Cin, Cout, kd, kh, kw, pd, ph, pw, epd, eph, epw) : 0;
}

// (variant 6's row layout)
extern "C" int diqt_conv3d_fwd_split16_pair_stats_blocks(int B, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw, int pd, int ph,
                                                         int pw, int epd, int eph, int epw) {
    H9Geom g; size_t lds; unsigned grid;
    if (!split16_pair_plan(g, lds, grid, B, D, H, W, Cin, Cout, kd, kh, kw, pd, ph, pw, epd, eph, epw)) return 0;
    return f9h_stats_blocks(g);
}

extern "C" int diqt_conv3d_fwd_split16_pair(const float* x, void* x16, const void* packed, const float* bias, const float* residual, float* y,
                                            float* stats, int B, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw, int pd,
                                            int ph, int pw, int epd, int eph, int epw, void* stream) {
    return split16_run("conv3d_fwd_split16_pair", S16_PAIR, x, x16, packed, bias, residual, y, stats, nullptr, 0, B, D, H, W, Cin, Cout, kd, kh,
                       kw, pd, ph, pw, epd, eph, epw, stream);
}

extern "C" int diqt_conv3d_fwd_gn_split16_pair(const float* x, void* x16, const void* packed, const float* bias, const float* residual,
                                               float* y, float* stats, const float* coef, int act, int B, int D, int H, int W, int Cin,
                                               int Cout, int kd, int kh, int kw, int pd, int ph, int pw, int epd, int eph, int epw,
                                               void* stream) {
    DIQT_REQUIRE(coef, DIQT_E_ALIGN, "conv3d_fwd_gn_split16_pair: null coefficients");
    return split16_run("conv3d_fwd_gn_split16_pair", S16_PAIR, x, x16, packed, bias, residual, y, stats, coef, act, B, D, H, W, Cin, Cout, kd,
                       kh, kw, pd, ph, pw, epd, eph, epw, stream);
}
