// Probe: where does a wave of the split build of conv_f9h_kernel (conv_split16.hip, variant H9S_333_256) spend its cycles?
// A diagnostic build of conv_f9h_kernel.h with its DIQT_F9H_STAMP macro defined: every stamp is an `s_memtime` of the wave, written by
// lane 0 with an ordinary vector store into a buffer that nothing else reads (no output depends on it).  The library never has a stamp.
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -DPROBE_RS=2 tools/probes/split_account_probe.hip -o tools/probes/split_account_probe
//   tools/probes/split_account_probe            (both shapes: 64 -> 64 @ 8 x 32^3 and 128 -> 128 @ 8 x 16^3)
// PROBE_RS: the kernel's residual / statistics template argument (2 = statistics, no residual: the sampler's blocks); leave it undefined
// for a revision of the header whose kernel has no such parameter.  PROBE_HEADER: another revision's conv_f9h_kernel.h (with the stamp
// macro placed at the same points).  PROBE_PAIR: the tap-paired body instead (conv_f9p_kernel.h, variant 9, its 7-slot ring; needs PROBE_RS;
// its "first PD taps" span is its first six pair steps, its MFMA floor per chunk 14 x 48 x 16 = 10752).  PROBE_BIAS_WAIT: the s_waitcnt in front of stamp 4 (default lgkmcnt(0): the staged bias; 0x0070 =
// vmcnt(0) lgkmcnt(0) for a revision that loads the bias from global memory).
//
// Method (MI355X: the chip lowers its clock under load): random operands, at least 2 s of back-to-back launches, then the stamps of the
// LAST launch; medians over all waves of all workgroups.  In-kernel clock = d(s_memtime) / d(s_memrealtime) x 100 MHz over the kernel.
// Stamp points of unit (tile it, chunk c):  0 chunk start (before its first fragment read)   1 behind the first PD taps
//   2 behind the last tap (before the chunk-end barrier)   3 behind that barrier
// and per tile (c = 0):  4 bias values in registers   5 behind the last store instruction   6 behind the tile-end barrier;
// 7 = kernel entry, 8 = kernel exit (with s_memrealtime).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <random>
#include <stdio.h>
#include <stdlib.h>
#include <vector>

constexpr int P_MAXIT = 4, P_MAXC = 8, P_NPT = 8, P_HDR = 4;
constexpr int P_WAVE = P_HDR + P_MAXIT * P_MAXC * P_NPT;          // 64-bit slots per wave
__device__ unsigned long long* g_probe_buf;

#ifndef PROBE_BIAS_WAIT
#define PROBE_BIAS_WAIT 0xc07f
#endif

__device__ __forceinline__ void probe_stamp(int it, int c, int p) {
    __builtin_amdgcn_sched_barrier(0);
    if (p == 4) __builtin_amdgcn_s_waitcnt(PROBE_BIAS_WAIT);
    const unsigned long long t = __builtin_amdgcn_s_memtime();
    unsigned long long* w = g_probe_buf + (size_t)(blockIdx.x * 4 + (threadIdx.x >> 6)) * P_WAVE;
    if ((threadIdx.x & 63) == 0) {
        if (p >= 7) {
            w[(p - 7) * 2] = t;
            w[(p - 7) * 2 + 1] = __builtin_amdgcn_s_memrealtime();
        } else if (it < P_MAXIT && c < P_MAXC) {
            w[P_HDR + (it * P_MAXC + c) * P_NPT + p] = t;
        }
    }
    __builtin_amdgcn_sched_barrier(0);
}
#define DIQT_F9H_STAMP(it, c, point) probe_stamp((it), (c), (point))

#ifdef PROBE_HEADER
#include PROBE_HEADER
#else
#include "../../diffusioniqt_amd/csrc/conv_f9h_kernel.h"
#endif
#ifdef PROBE_PAIR
#include "../../diffusioniqt_amd/csrc/conv_f9p_kernel.h"
#endif

namespace diqt {                     // the two host hooks of common.h that live in lib.cpp
void set_error(const char*, ...) {}
void census_note(const char*) {}
}  // namespace diqt

using namespace diqt;
using Cf = h9::H9S_333_256;
#if defined(PROBE_PAIR)
static const auto kern = h9::conv_f9p_kernel<Cf, PROBE_RS, 7>;
constexpr int RSV = PROBE_RS;
constexpr size_t EXTRA_LDS = h9::BIASB;
#elif defined(PROBE_RS)
static const auto kern = h9::conv_f9h_kernel<Cf, false, false, true, PROBE_RS>;
constexpr int RSV = PROBE_RS;
constexpr size_t EXTRA_LDS = h9::BIASB;
#else
static const auto kern = h9::conv_f9h_kernel<Cf, false, false, true>;
constexpr int RSV = 2;
constexpr size_t EXTRA_LDS = 0;
#endif

#define CK(e) do { hipError_t e_ = (e); if (e_ != hipSuccess) { printf("%s: %s\n", #e, hipGetErrorString(e_)); exit(1); } } while (0)

static double med(std::vector<double>& v) {
    if (v.empty()) return 0.0;
    std::sort(v.begin(), v.end());
    return v[v.size() / 2];
}

static void run(int B, int S, int Cin, int Cout) {
    // the plan of f9h_plan(split) for a cubic volume, padding 1: Cin counts fp32 channels here, the kernel sees 2 Cin 16-bit channels
    H9Geom g{};
    g.B = B; g.D = g.H = g.W = S; g.Cin = 2 * Cin; g.Cout = Cout; g.Do = g.Ho = g.Wo = S; g.pd = g.ph = g.pw = 1;
    g.tilesD = (S + Cf::TD - 1) / Cf::TD; g.tilesH = (S + Cf::TH - 1) / Cf::TH; g.tilesW = (S + Cf::TW - 1) / Cf::TW;
    g.MT = B * g.tilesD * g.tilesH * g.tilesW; g.nNt = (Cout + 63) / 64; g.CoutPad = g.nNt * 64; g.nChunks = g.Cin / h9::CK; g.variant = 6;
    const size_t vox = (size_t)B * S * S * S;
    g.xBytes = (unsigned)(vox * g.Cin * 2); g.yBytes = g.rBytes = (unsigned)(vox * Cout * 4);
    g.wBytes = (unsigned)((size_t)g.nChunks * 27 * g.CoutPad * h9::CK * 2);
    const long long units = (long long)g.MT * g.nNt;
    unsigned grid = units > 256 ? 256u : (unsigned)units;
    if (units > 256) grid -= grid % (unsigned)g.nNt;
    const int tilesPerWg = (int)((units + grid - 1) / grid);
    const size_t lds = Cf::LDS_BYTES + EXTRA_LDS;

    std::mt19937 rng(1234);
    std::normal_distribution<float> nd(0.f, 1.f);
    std::vector<_Float16> hx(vox * g.Cin), hw((size_t)g.wBytes / 2);
    for (auto& v : hx) v = (_Float16)nd(rng);
    for (auto& v : hw) v = (_Float16)(nd(rng) * 0.02f);
    std::vector<float> hb(Cout);
    for (auto& v : hb) v = nd(rng) * 0.1f;
    void *x, *w, *y, *r = nullptr; float *bias, *stats = nullptr; unsigned long long* buf;
    CK(hipMalloc(&x, g.xBytes)); CK(hipMalloc(&w, g.wBytes)); CK(hipMalloc(&y, g.yBytes)); CK(hipMalloc(&bias, Cout * 4));
    CK(hipMemcpy(x, hx.data(), g.xBytes, hipMemcpyHostToDevice)); CK(hipMemcpy(w, hw.data(), g.wBytes, hipMemcpyHostToDevice));
    CK(hipMemcpy(bias, hb.data(), Cout * 4, hipMemcpyHostToDevice));
    if (RSV & 1) { CK(hipMalloc(&r, g.rBytes)); CK(hipMemset(r, 0, g.rBytes)); }
    if (RSV & 2) CK(hipMalloc(&stats, (size_t)B * g.tilesD * g.tilesH * g.tilesW * 2 * 2 * Cout * 4));
    g.stats = stats;
    const size_t nWaves = (size_t)grid * 4;
    CK(hipMalloc(&buf, nWaves * P_WAVE * 8)); CK(hipMemset(buf, 0, nWaves * P_WAVE * 8));
    CK(hipMemcpyToSymbol(HIP_SYMBOL(g_probe_buf), &buf, sizeof(buf)));
    CK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));

    auto launch = [&]() {
        hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, 0, (const void*)x, (const unsigned short*)w, (const float*)bias,
                           (const float*)r, y, g);
    };
    const auto t0 = std::chrono::steady_clock::now();
    long launches = 0;
    while (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() < 2.2) {     // >= 2 s of load before the sample
        for (int i = 0; i < 200; ++i) launch();
        CK(hipDeviceSynchronize());
        launches += 200;
    }
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    CK(hipEventRecord(e0));
    for (int i = 0; i < 200; ++i) launch();
    CK(hipEventRecord(e1)); CK(hipDeviceSynchronize());
    float ms = 0; CK(hipEventElapsedTime(&ms, e0, e1));
    std::vector<unsigned long long> h(nWaves * P_WAVE);
    CK(hipMemcpy(h.data(), buf, h.size() * 8, hipMemcpyDeviceToHost));

    const int nC = g.nChunks < P_MAXC ? g.nChunks : P_MAXC, nT = tilesPerWg < P_MAXIT ? tilesPerWg : P_MAXIT;
    auto S_ = [&](size_t wv, int it, int c, int p) { return (double)h[wv * P_WAVE + P_HDR + (it * P_MAXC + c) * P_NPT + p]; };
    std::vector<double> life, clk, pro, taps, bar, lastbar, toBias, toStore, toBar, toNext, bound, pdIn, pdFirst, pdTile;
    for (size_t wv = 0; wv < nWaves; ++wv) {
        const unsigned long long* q = &h[wv * P_WAVE];
        if (!q[0] || !q[2] || q[3] <= q[1]) continue;
        // tiles this workgroup really has (a stamp of a tile it does not own stays zero)
        int mine = 0;
        while (mine < nT && S_(wv, mine, 0, 0) > 0) ++mine;
        if (!mine) continue;
        life.push_back((double)(q[2] - q[0]));
        clk.push_back((double)(q[2] - q[0]) / (double)(q[3] - q[1]) * 100.0);
        pro.push_back(S_(wv, 0, 0, 0) - (double)q[0]);
        for (int it = 0; it < mine; ++it) {
            for (int c = 0; c < nC; ++c) {
                taps.push_back(S_(wv, it, c, 2) - S_(wv, it, c, 0));
                if (c + 1 < nC) bar.push_back(S_(wv, it, c, 3) - S_(wv, it, c, 2));
                const double pd = S_(wv, it, c, 1) - S_(wv, it, c, 0);
                if (c > 0) pdIn.push_back(pd);
                else if (it > 0) pdTile.push_back(pd);
                else pdFirst.push_back(pd);
            }
            lastbar.push_back(S_(wv, it, nC - 1, 3) - S_(wv, it, nC - 1, 2));
            toBias.push_back(S_(wv, it, 0, 4) - S_(wv, it, nC - 1, 3));
            toStore.push_back(S_(wv, it, 0, 5) - S_(wv, it, 0, 4));
            toBar.push_back(S_(wv, it, 0, 6) - S_(wv, it, 0, 5));
            if (it + 1 < mine) {
                toNext.push_back(S_(wv, it + 1, 0, 0) - S_(wv, it, 0, 6));
                bound.push_back(S_(wv, it + 1, 0, 0) - S_(wv, it, nC - 1, 2));
            }
        }
    }
#ifdef PROBE_PAIR
    const double mfma = 14.0 * 48 * 16.0;                 // MFMA cycles of a chunk: 14 pair steps x 48 MFMAs x 16 cycles
#else
    const double mfma = 3.0 * Cf::NVB * 27 * 32.0;       // MFMA cycles of a chunk: three products x NVB blocks x 27 taps x 32 cycles
#endif
    printf("== %d -> %d @ %d x %d^3: grid %u, %d tile(s) per workgroup, %d chunks; %.1f us per launch (200 launches after %ld), "
           "%zu waves sampled\n", Cin, Cout, B, S, grid, tilesPerWg, g.nChunks, ms * 1e3 / 200, launches, life.size());
    printf("   in-kernel clock %.0f MHz; wave life %.0f cycles (MFMA floor %.0f = %d units x %.0f)\n", med(clk), med(life),
           mfma * g.nChunks * tilesPerWg, g.nChunks * tilesPerWg, mfma);
    printf("   prologue to the first chunk start            %8.0f\n", med(pro));
    printf("   a chunk's taps (floor %.0f)                  %8.0f\n", mfma, med(taps));
    printf("   chunk-end barrier inside a tile              %8.0f\n", med(bar));
    printf("   tile boundary: last chunk's barrier          %8.0f\n", med(lastbar));
    printf("                  to the bias in registers      %8.0f\n", med(toBias));
    printf("                  to the last store issued      %8.0f\n", med(toStore));
    printf("                  statistics + tile-end barrier %8.0f\n", med(toBar));
    printf("                  to the next tile's chunk start%8.0f\n", med(toNext));
    printf("   = last MFMA of a tile to the next tile's chunk start %8.0f\n", med(bound));
    printf("   first PD taps: kernel start %.0f, inside a tile %.0f, behind a tile boundary %.0f (floor %.0f)\n", med(pdFirst), med(pdIn),
           med(pdTile), mfma / 27 * (g.nChunks ? 3 : 0));
    hipFree(x); hipFree(w); hipFree(y); hipFree(bias); hipFree(buf);
    if (r) hipFree(r);
    if (stats) hipFree(stats);
}

int main() {
    run(8, 32, 64, 64);
    run(8, 16, 128, 128);
    return 0;
}
