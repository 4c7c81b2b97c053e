// conv_f9p_kernel -- the three-product split build of conv_f9h_kernel on the 256-voxel tile with a TAP-PAIRED body on
// v_mfma_f32_16x16x32_f16 (round 11, variant 9; instantiated by conv_split16_c.hip).  conv_f9h_kernel.h has the scheme this kernel
// keeps unchanged: x' in HBM as [16 heads | 16 tails] per voxel and chunk, the halo LDS-DMA into a swizzled two-image ring, the
// persistent tile walk with one barrier per chunk, the staged bias, the four residual x statistics instantiations (RS), the packed
// weights of diqt_conv_pack_weight_split16, and the whole epilogue behind the accumulator -> scratch write.
// TWIN CODE: the halo DMA, the tile walk, the prologue and the epilogue below are copies of conv_f9h_kernel's SPLIT path (kept apart so
// that variants 0-8 compile to the instruction streams they had): a fix to either goes into both.
//
// Why another MFMA shape: in a power-limited MFMA loop the chip holds a higher clock on 16x16x32 than on 32x32x16 at equal cycles per
// FLOP (tools/probes/mfma_shape_probe.hip, profiles/r11_mfma_shape.md), and with K = 32 two taps go into one product, so the
// head x head chain of a block has as many sequential fp32 accumulations in ONE accumulator set as variant 6's even / odd pair of
// sets: the third set (64 registers) goes away.
//
// Arithmetic.  A pair step p (0..13) covers taps 2p and 2p+1: K index 0-15 = the chunk's 16 channels at tap 2p, 16-31 = at tap 2p+1.
// Per 16 co x 16 voxel block and step:  acc += WH XH,  acc1 += WL XH,  acc1 += WH XL;  the epilogue stores acc + 2^-11 acc1 + bias.
// Step 13 has no second tap: its upper-K weight lanes take an out-of-range buffer offset (zeros), its upper-K voxel lanes re-read tap
// 26's row (finite values of the true stencil: nothing from outside it can leak in).
//
// Operands.  A wave keeps its 128 voxels x 32 channels: 2 row blocks (16 channels) x 8 column blocks (16 voxels).  Lane l: m = l & 15,
// k-group kg = l >> 4 = octet (kg & 1) of tap 2p + (kg >> 1).
//   * weight fragment: row 16 rb + m of the existing pack at the lane's own tap (+ wStride for the upper groups) and octet, tails +32 B;
//   * voxel fragment: one ds_read_b128 at the lane's own voxel and its own tap.  The swizzle term of the address depends on the tap's
//     (ky, kx), so every (step, column-block parity, head / tail) has a per-lane address register: 56, set once per kernel and moved
//     with the image ring, four per step;
//   * a 4 x 8 block is two column blocks: rows {0, 2} (parity 0) and {1, 3} (parity 1) x 8 columns; columns m = 0-3 and 12-15 are the
//     first of the two rows, 4-11 the second (pair_col_voxel).  With the image's swizzle this is conflict-free for the four service
//     groups of ds_read_b128 at every step, both fragments and all column blocks (diqt_conv_split16_pair_lds_conflicts() == 1).
// The products are written instructions accumulating in place in AGPRs, one fragment read of the next step beside every three of them,
// the step's four weight loads and its halo pieces behind the MFMAs of groups of their own; a sched_barrier behind every group keeps
// that order.  (Left to the register allocator, 16x16 accumulators rotate through the body and pay v_accvgpr moves for it.)
#pragma once
#include "conv_f9h_kernel.h"

namespace diqt {
namespace h9 {

constexpr int PAIR_STEPS = 14;

// column m (0..15) of the column block with row parity h of a 4 x 8 block -> voxel (row j, column i)
__host__ __device__ constexpr int pair_col_j(int m, int h) { return h + 2 * (((m >> 2) ^ (m >> 3)) & 1); }
__host__ __device__ constexpr int pair_col_i(int m) { return 4 * (m >> 3) + (m & 3); }
// row of the epilogue's transpose scratch (conv_f9h_kernel's lane <-> voxel map of a block, inverted)
__host__ __device__ constexpr int pair_col_row(int m, int h) {
    const int t2 = ((m >> 2) ^ (m >> 3)) & 1, t1 = m >> 3;
    return (t2 << 4) | (t1 << 3) | ((h ^ t1 ^ t2) << 2) | (m & 3);
}
// the tap a lane's k-group reads at step p (voxel fragment; the weight fragment of step 13's upper groups is zero instead)
__host__ __device__ constexpr int pair_tap(int p, int kg) { return 2 * p + (kg >> 1) < 27 ? 2 * p + (kg >> 1) : 26; }
// LDS byte address (inside an image) of a voxel fragment: column m, octet ko of tap t, column block parity h, q = 0 heads / 1 tails, at
// the first block of voxel half wa (the image's swizzle: conv_f9h_kernel.h)
template <class C> __host__ __device__ constexpr int pair_lds_addr_t(int m, int ko, int t, int h, int q, int wa) {
    const int ky = (t / C::KW) % C::KH, kx = t % C::KW;
    const int j = pair_col_j(m, h), i = pair_col_i(m);
    const int gx = ((i + kx) >> 2) & 1, gy = ((j + ky) >> 1) & 1;
    return (C::blockrow(0) + (wa ? C::blockrow(C::NVB) : 0) + j * C::HWd + i + C::tapoff(t)) * ROWB + ((ko ^ gx) << 4) + ((q ^ gy) << 5);
}
// ... of lane l at step p
template <class C> __host__ __device__ constexpr int pair_lds_addr(int l, int p, int h, int q, int wa) {
    const int a0 = pair_lds_addr_t<C>(l & 15, (l >> 4) & 1, pair_tap(p, 0), h, q, wa), a1 = pair_lds_addr_t<C>(l & 15, (l >> 4) & 1, pair_tap(p, 2), h, q, wa);
    return (l >> 5) ? a1 : a0;
}
// the lanes ds_read_b128 serves together: service group s (0..3), member e (0..15)
__host__ __device__ constexpr int b128_group_lane(int s, int e) {
    const int in32 = (s & 1) ? (e < 8 ? 4 + e : (e < 12 ? 8 + e : 16 + e)) : (e < 4 ? e : (e < 8 ? 8 + e : 12 + e));
    return 32 * (s >> 1) + in32;
}
// worst number of distinct addresses on one 16-byte slot of the 64 banks over every service group, step, fragment and column block
template <class C> constexpr int pair_lds_conflicts() {
    int worst = 0;
    for (int wa = 0; wa < 2; ++wa)
        for (int p = 0; p < PAIR_STEPS; ++p)
            for (int cb = 0; cb < 2 * C::NVB; ++cb)
                for (int q = 0; q < 2; ++q)
                    for (int s = 0; s < 4; ++s) {
                        int addr[16] = {};
                        for (int e = 0; e < 16; ++e)
                            addr[e] = pair_lds_addr<C>(b128_group_lane(s, e), p, cb & 1, q, wa) + (C::blockrow(cb >> 1) - C::blockrow(0)) * ROWB;
                        for (int e = 0; e < 16; ++e) {
                            int n = 0;
                            for (int f = 0; f < 16; ++f) {
                                if (((addr[f] >> 4) & 15) != ((addr[e] >> 4) & 15)) continue;
                                bool seen = false;
                                for (int k = 0; k < f; ++k) seen = seen || addr[k] == addr[f];
                                if (!seen) ++n;
                            }
                            if (n > worst) worst = n;
                        }
                    }
    return worst;
}

// c (+)= a b on v_mfma_f32_16x16x32_f16, in place; Z: from a zero C operand (a tile's first products)
template <bool Z> __device__ __forceinline__ void mfma_pair(f32x4v& c, const u32x4& a, const u32x4& b) {
    if (Z) asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, 0" : "=a"(c) : "v"(a), "v"(b));
    else asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+a"(c) : "v"(a), "v"(b));
}

// PD: slots of the weight ring, one per pair step (4 x b128 per lane and slot); divides PAIR_STEPS
template <class C, int RS, int PD>
__global__ __launch_bounds__(256, 1) void conv_f9p_kernel(const void* __restrict__ xv, const unsigned short* __restrict__ wp,
                                                          const float* __restrict__ bias, const float* __restrict__ residual,
                                                          void* __restrict__ yv, H9Geom g) {
    constexpr int T = C::T, HB = C::HB, NPH = C::NPH, NVB = C::NVB, HH = C::HH, HWd = C::HWd, HV = C::HV, NIMG = C::NIMG;
    constexpr int NS = PAIR_STEPS, NCB = 2 * NVB;
    static_assert(T == 27 && NIMG == 2 && NVB == 4, "the pair body is written for the 3x3x3 filter on the 256-voxel tile");
    static_assert(NS % PD == 0 && PD >= 2, "the ring slot of a step is static");
    constexpr int NSP = NS - PD + 1;                  // steps of a chunk that issue halo pieces: all older than the last step's weight load
    static_assert(NSP >= 1, "halo pieces need a step to ride on");
    extern __shared__ __attribute__((aligned(1024))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int m = lane & 15, kg = lane >> 4;
    const int wa = wave >> 1, wb = wave & 1;            // voxel half, channel half of the tile
    const unsigned Gn = gridDim.x;
    const unsigned total = (unsigned)g.MT * g.nNt;
    unsigned L = xcd_remap(blockIdx.x, Gn);
    if (L >= total) return;
    DIQT_F9H_STAMP(0, 0, 7);                          // (stamps: a diagnostic build only, tools/probes/split_account_probe.hip -DPROBE_PAIR)
    const unsigned L0 = L;
    const int nMine = (int)((total - 1 - L) / Gn) + 1;
    const int n0 = (int)(L % g.nNt) * 64;
    const int nChunks = g.nChunks;

    const auto rs_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(xv), 0, (int)g.xBytes, 0x00020000);
    const auto rs_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned short*>(wp), 0, (int)g.wBytes, 0x00020000);
    const auto rs_y = __builtin_amdgcn_make_buffer_rsrc(yv, 0, (int)g.yBytes, 0x00020000);
    const auto rs_r = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(residual), 0, residual ? (int)g.rBytes : 0, 0x00020000);
    const unsigned ldsBase = (unsigned)(size_t)(lds_void*)smem;

    // ---- halo DMA pieces and the tile walk: conv_f9h_kernel's ----
    unsigned posH[NPH];
#pragma unroll
    for (int r = 0; r < NPH; ++r) {
        const int p = (wave + 4 * r) * 64 + lane;
        const int row = p >> 2;
        const int hx = row % HWd, hy = (row / HWd) % HH, hz = row / (HWd * HH);
        const int gsw = ((hx >> 2) & 1) | (((hy >> 1) & 1) << 1);
        posH[r] = (unsigned)hz | ((unsigned)hy << 10) | ((unsigned)(row < HV ? hx : 1023) << 20) | ((unsigned)((p & 3) ^ gsw) << 30);
    }
    const int Dm1 = g.D - 1, Hm1 = g.H - 1, Wm1 = g.W - 1;
    int tb, d0, h0, w0;
    int bz = 0, by = 0, bxx = 0;
    unsigned baseX = 0, deadX = OOB;
    auto tile_of = [&](unsigned Lt, int& b_, int& d_, int& h_, int& w_) __attribute__((always_inline)) {
        int mt = (int)(Lt / g.nNt);
        const int tx = mt % g.tilesW; mt /= g.tilesW;
        const int ty = mt % g.tilesH; mt /= g.tilesH;
        const int tz = mt % g.tilesD;
        b_ = mt / g.tilesD; d_ = tz * C::TD; h_ = ty * C::TH; w_ = tx * C::TW;
    };
    auto set_fetch = [&](int fit_) __attribute__((always_inline)) {
        const bool live = fit_ < nMine;
        int b_, d_, h_, w_;
        tile_of(live ? L0 + (unsigned)fit_ * Gn : L0, b_, d_, h_, w_);
        bz = d_ - g.pd; by = h_ - g.ph; bxx = w_ - g.pw;
        baseX = (unsigned)((((b_ * g.D + bz) * g.H + by) * g.W + bxx) * g.Cin) * 2u;
        deadX = live ? 0u : OOB;
    };
    const int HWs = g.W * g.Cin * 2, HHs = g.H * HWs, Cs = g.Cin * 2;
    auto dma_h = [&](int r, unsigned imgBase, int chunk) __attribute__((always_inline)) {     // r static
        const unsigned p = posH[r];
        const int hz = (int)(p & 1023u), hy = (int)((p >> 10) & 1023u), hx = (int)((p >> 20) & 1023u);
        const int iz = bz + hz, iy = by + hy, ix = bxx + hx;
        const unsigned mk = (unsigned)(iz | iy | ix) | (unsigned)((Dm1 - iz) | (Hm1 - iy) | (Wm1 - ix)) | deadX;
        const unsigned rel = (unsigned)(hz * HHs + hy * HWs + hx * Cs) + ((p >> 30) << 4);
        const unsigned voff = (baseX + rel + (unsigned)chunk * ROWB) | (mk & OOB);
        dma16(rs_x, imgBase + (unsigned)(wave + 4 * r) * 1024u, voff);
    };

    // ---- weight fragments: A operand, row = co (32 wb + 16 rb + m), the lane's own tap and octet; a slot is a pair step ----
    const unsigned wStride = (unsigned)g.CoutPad * ROWB;      // bytes between consecutive (chunk, tap) panels
    const unsigned wLane = (unsigned)((n0 + 32 * wb + m) * ROWB + (kg & 1) * 16) + (unsigned)(kg >> 1) * wStride;
    const unsigned wLane13 = (kg >> 1) ? OOB : wLane;         // step 13: no second tap, the upper k-groups read zeros
    const int WT = nChunks * T;
    u32x4 Wr[PD][2][2];                                       // [slot][row block][heads, tails]
    int wlin = 0;
    unsigned wsoff = 0;
    auto w_load = [&](int slot, bool last) __attribute__((always_inline)) {                    // slot, last (step 13 of its chunk) static
        const unsigned vo = last ? wLane13 : wLane;
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) {
            Wr[slot][rb][0] = __builtin_amdgcn_raw_buffer_load_b128(rs_w, vo + (unsigned)rb * 16u * ROWB, wsoff, 0);
            Wr[slot][rb][1] = __builtin_amdgcn_raw_buffer_load_b128(rs_w, vo + (unsigned)rb * 16u * ROWB + 32u, wsoff, 0);
        }
        wsoff += last ? wStride : 2u * wStride;
        wlin += last ? 1 : 2;
        if (wlin == WT) { wlin = 0; wsoff = 0; }
    };

    // ---- voxel fragments: B operand, column = this lane's voxel of a column block, K = its own tap and octet ----
    int xa[NS][2][2];                                         // [step][column block parity][heads, tails], image `img`
#pragma unroll
    for (int p = 0; p < NS; ++p)
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int q = 0; q < 2; ++q) xa[p][h][q] = pair_lds_addr<C>(lane, p, h, q, wa);

    const auto rs_b = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(bias), 0, bias ? g.Cout * 4 : 0, 0x00020000);
    f32x4v acc[2][NCB], acc1[2][NCB];                         // [row block][column block]: head x head, the cross terms (scaled by 2^11)

    // ---- prologue: the first unit's halo image, the first PD - 1 weight slots, the bias ----
    int fit = 0, fc = 0;
    set_fetch(0);
    auto advance_fetch = [&]() __attribute__((always_inline)) {
        if (++fc == nChunks) { fc = 0; ++fit; set_fetch(fit); }
    };
#pragma unroll
    for (int r = 0; r < NPH; ++r) dma_h(r, ldsBase, fc);
    advance_fetch();
#pragma unroll
    for (int s = 0; s < PD - 1; ++s) w_load(s, false);
    if (tid < 64)
        reinterpret_cast<float*>(smem + C::LDS_BYTES)[tid] =
            __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs_b, (unsigned)(n0 + tid) * 4u, 0, 0));
    __builtin_amdgcn_s_waitcnt(0x0f70);                    // vmcnt(0)
    __syncthreads();

    int img = 0, fimg = 1;
    tile_of(L, tb, d0, h0, w0);
    for (int it = 0; it < nMine; ++it) {
        // a unit = one chunk of a tile; the tile's first chunk is peeled: the first product of every accumulator takes a zero C operand
#pragma unroll
        for (int pass = 0; pass < 2; ++pass)
        for (int c = pass; c < (pass == 0 ? 1 : nChunks); ++c) {
            const bool FIRST = pass == 0;
            const unsigned fbase = ldsBase + (unsigned)fimg * HB;
            const int delta = (img ? -1 : 1) * HB;            // to the image the next chunk reads
            u32x4 Xh[2][NCB], Xl[2][NCB];
            auto rd = [&](int p, int cb, int q) __attribute__((always_inline)) {              // all static
                const u32x4 v = *reinterpret_cast<const u32x4*>(smem + xa[p][cb & 1][q] + (C::blockrow(cb >> 1) - C::blockrow(0)) * ROWB);
                if (q) Xl[p & 1][cb] = v; else Xh[p & 1][cb] = v;
            };
            DIQT_F9H_STAMP(it, c, 0);
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb) { rd(0, cb, 0); rd(0, cb, 1); }       // cold read of the chunk's first step (the barrier published the image)
#pragma unroll
            for (int p = 0; p < NS; ++p) {
                __builtin_amdgcn_sched_barrier(0);
                const int s = p % PD, cur = p & 1;
                const bool Z = FIRST && p == 0;
#pragma unroll
                for (int cb = 0; cb < NCB; ++cb) {
                    // three MFMAs and one fragment read of the next step per group; four MFMAs lie between the two sums into a cross block
                    if (p + 1 < NS) rd(p + 1, cb, 0);
                    if (Z) {
                        mfma_pair<true>(acc1[0][cb], Wr[s][0][1], Xh[cur][cb]);
                        mfma_pair<true>(acc1[1][cb], Wr[s][1][1], Xh[cur][cb]);
                        mfma_pair<true>(acc[0][cb], Wr[s][0][0], Xh[cur][cb]);
                    } else {
                        mfma_pair<false>(acc1[0][cb], Wr[s][0][1], Xh[cur][cb]);
                        mfma_pair<false>(acc1[1][cb], Wr[s][1][1], Xh[cur][cb]);
                        mfma_pair<false>(acc[0][cb], Wr[s][0][0], Xh[cur][cb]);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    if (p + 1 < NS) rd(p + 1, cb, 1);
                    if (Z) mfma_pair<true>(acc[1][cb], Wr[s][1][0], Xh[cur][cb]);
                    else mfma_pair<false>(acc[1][cb], Wr[s][1][0], Xh[cur][cb]);
                    mfma_pair<false>(acc1[0][cb], Wr[s][0][0], Xl[cur][cb]);
                    mfma_pair<false>(acc1[1][cb], Wr[s][1][0], Xl[cur][cb]);
                    // memory instructions ride behind the MFMAs of a group: the halo pieces of the next unit first (in program order in
                    // front of the weight slot PD - 1 steps ahead: loads retire in order, so the wait in front of the last step's weight
                    // fragment is what guarantees the next image before the chunk-end barrier), then the slot the previous step has left
                    if (cb == 1) {
#pragma unroll
                        for (int r = 0; r < NPH; ++r)
                            if (r * NSP / NPH == p) dma_h(r, fbase, fc);
                    }
                    if (cb == 3) w_load((p + PD - 1) % PD, (p + PD - 1) % NS == NS - 1);
                    // the next step's address registers move to the image of the next chunk behind their last read in this one (step 13:
                    // step 0's, read cold): two adds in a group instead of 56 at the chunk's end
                    if (cb >= NCB - 2) { const int pn = (p + 1) % NS; xa[pn][cb & 1][0] += delta; xa[pn][cb & 1][1] += delta; }
                    __builtin_amdgcn_sched_barrier(0);
                }
                if (p == PD - 2) { DIQT_F9H_STAMP(it, c, 1); }
            }
            DIQT_F9H_STAMP(it, c, 2);
            // End of the unit: the next unit's image is complete (see above); this wave's reads of image `img` have been consumed.
            asm volatile("s_barrier" ::: "memory");
            DIQT_F9H_STAMP(it, c, 3);
            advance_fetch();
            {
                fimg = img;
                img ^= 1;
            }
        }
        // ---- epilogue of the tile: conv_f9h_kernel's split form but for the accumulator -> scratch write.  Lane (m, kg) holds channels
        //      16 rb + 4 kg + e of voxel column m of column block cb = 2 vb + h: row pair_col_row(m, h) of block vb's [32 voxels][32 channels] ----
        asm volatile("s_nop 15\n\ts_nop 15");               // the last MFMAs' results, before VALU reads them
        {
            constexpr int SROW = 144;
            const bool hasRes = (RS & 1) != 0;
            const bool wantStats = (RS & 2) != 0;
            char* const scrb = smem + fimg * HB + wave * SCRW;
            const int piece = lane & 7, vl = lane >> 3;
            const int cop = n0 + 32 * wb + piece * 4;
            const bool cok = cop < g.Cout;
            const unsigned C4 = (unsigned)g.Cout * 4u;
            int rjk[4], rik[4];
            unsigned lo[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int vloc = 8 * k + vl, tqr = vloc >> 2;
                rjk[k] = 2 * (tqr >> 2) + ((tqr ^ (tqr >> 1) ^ (tqr >> 2)) & 1);
                rik[k] = 4 * (k & 1) + (vl & 3);
                lo[k] = cok ? (unsigned)(rjk[k] * g.Wo + rik[k]) * C4 + (unsigned)cop * 4u : OOB;
            }
            const unsigned tileOff = (unsigned)(((tb * g.Do + d0) * g.Ho + h0) * g.Wo + w0) * C4;
            auto offs = [&](int vb, unsigned (&vo)[4], unsigned& so) __attribute__((always_inline)) {
                const int id = wa * NVB + vb;
                const int bd = id / (C::NBH * C::NBW), bh = ((id / C::NBW) % C::NBH) * 4, bw = (id % C::NBW) * 8;
                so = tileOff + (unsigned)((bd * g.Ho + bh) * g.Wo + bw) * C4;
                const int hlim = d0 + bd < g.Do ? g.Ho - h0 - bh : 0, wlim = g.Wo - w0 - bw;
#pragma unroll
                for (int k = 0; k < 4; ++k) vo[k] = ((int)(rjk[k] < hlim) & (int)(rik[k] < wlim)) ? lo[k] : OOB;
            };
            float ssum[4], ssq[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) { ssum[e] = 0.f; ssq[e] = 0.f; }
            f32x4v b4[2];
#pragma unroll
            for (int rb = 0; rb < 2; ++rb)
                b4[rb] = *reinterpret_cast<const f32x4v*>(smem + C::LDS_BYTES + (32 * wb + 16 * rb + 4 * kg) * 4);
            const int srow0 = pair_col_row(m, 0) * SROW, srow1 = pair_col_row(m, 1) * SROW;
            unsigned vo[2][4], so[2];
            f32x4v rr[2][4];
            offs(0, vo[0], so[0]);
            if (hasRes) {
#pragma unroll
                for (int k = 0; k < 4; ++k) rr[0][k] = __builtin_bit_cast(f32x4v, __builtin_amdgcn_raw_buffer_load_b128(rs_r, vo[0][k], so[0], 0));
            }
            DIQT_F9H_STAMP(it, 0, 4);
#pragma unroll
            for (int vb = 0; vb < NVB; ++vb) {
                const int cur = vb & 1, nxt = cur ^ 1;
#pragma unroll
                for (int h = 0; h < 2; ++h)
#pragma unroll
                    for (int rb = 0; rb < 2; ++rb) {
                        f32x4v p;
#pragma unroll
                        for (int e = 0; e < 4; ++e) p[e] = fmaf(acc1[rb][2 * vb + h][e], 0x1p-11f, acc[rb][2 * vb + h][e]) + b4[rb][e];
                        *reinterpret_cast<f32x4v*>(scrb + (h ? srow1 : srow0) + 64 * rb + 16 * kg) = p;
                    }
                if (vb + 1 < NVB) {
                    offs(vb + 1, vo[nxt], so[nxt]);
                    if (hasRes) {
#pragma unroll
                        for (int k = 0; k < 4; ++k)
                            rr[nxt][k] = __builtin_bit_cast(f32x4v, __builtin_amdgcn_raw_buffer_load_b128(rs_r, vo[nxt][k], so[nxt], 0));
                    }
                }
                u32x4 d[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) d[k] = *reinterpret_cast<const u32x4*>(scrb + (8 * k + vl) * SROW + piece * 16);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (hasRes) {
                        f32x4v f = __builtin_bit_cast(f32x4v, d[k]);
#pragma unroll
                        for (int e = 0; e < 4; ++e) f[e] += rr[cur][k][e];
                        d[k] = __builtin_bit_cast(u32x4, f);
                    }
                    if (wantStats) {
                        const float okf = vo[cur][k] != OOB ? 1.f : 0.f;
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const unsigned wd = d[k][e];
                            const float v = __builtin_bit_cast(float, wd);
                            const float mv = okf * v;
                            ssum[e] += mv;
                            ssq[e] = fmaf(mv, v, ssq[e]);
                        }
                    }
                    __builtin_amdgcn_raw_buffer_store_b128(d[k], rs_y, vo[cur][k], so[cur], 0);
                }
            }
            DIQT_F9H_STAMP(it, 0, 5);
            if (wantStats) {
                const int tpb = g.tilesD * g.tilesH * g.tilesW, mtile = (int)(L / g.nNt);
                float* srow = g.stats + ((size_t)(mtile / tpb) * (2 * tpb) + (size_t)(mtile % tpb) * 2 + wa) * 2 * g.Cout;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
#pragma unroll
                    for (int o = 8; o < 64; o <<= 1) {
                        ssum[e] += __shfl_xor(ssum[e], o, 64);
                        ssq[e] += __shfl_xor(ssq[e], o, 64);
                    }
                }
                if (lane < 8 && cok) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) { srow[cop + e] = ssum[e]; srow[g.Cout + cop + e] = ssq[e]; }
                }
            }
        }
        asm volatile("s_barrier" ::: "memory");              // every wave's scratch reads are done (their stores have been issued)
        DIQT_F9H_STAMP(it, 0, 6);
        L += Gn;
        if (it + 1 < nMine) tile_of(L, tb, d0, h0, w0);
    }
    // the (dead) halo pieces issued during the last units write zeros into this workgroup's LDS: they have to land before it is released
    __builtin_amdgcn_s_waitcnt(0x0f70);                    // vmcnt(0)
    DIQT_F9H_STAMP(0, 0, 8);
}

}  // namespace h9
}  // namespace diqt
