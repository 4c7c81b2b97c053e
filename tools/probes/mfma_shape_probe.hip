// Probe: does the chip run the split conv's products faster on v_mfma_f32_16x16x32_f16 than on v_mfma_f32_32x32x16_f16?
// Two kernels with the same FLOPs per tap, the same 32 channel x 128 voxel output tile per wave and the same three products of the split
// (acc += WH.XH, acc1 += WL.XH, acc1 += WH.XL), 256 threads, one workgroup per CU, one wave per SIMD, weights in registers, every voxel
// fragment re-read from a swizzled LDS image (16 consecutive lanes never share a 16-byte slot) that is staged once:
//   (a) per tap       8 ds_read_b128 + 12 v_mfma_f32_32x32x16_f16 on three accumulator sets of four 32x32 blocks (even taps, odd taps,
//       cross terms): the body of conv_f9h_kernel's split build on the 256-voxel tile;
//   (b) per tap pair 16 ds_read_b128 + 48 v_mfma_f32_16x16x32_f16 on two sets of sixteen 16x16 blocks, K 0-15 = tap 2p, K 16-31 = tap 2p+1.
// A "chunk" is 28 taps = 14 pairs in both.  No global traffic inside the loop; each lane stores one value to a buffer of its own at the end.
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/probes/mfma_shape_probe.hip -o tools/probes/mfma_shape_probe
//   tools/probes/mfma_shape_probe [chunks per launch, default 40]
//
// Method (MI355X: the chip lowers its clock under load): random fp16 operands; both kernels are first checked against a float64 sum on
// the host (two chunks); then three rounds of a, b: at least 2.2 s of back-to-back launches, then 1000 launches between two events.
// In-kernel clock = d(s_memtime) / d(s_memrealtime) x 100 MHz, stamped once around the loop by lane 0 of every wave (median over the
// waves of the last launch).  The stamps go to a buffer that nothing else reads.
// Verdict: (b) has to beat (a) by wall time by more than 3.7 % (the half-empty fourteenth pair step of a 27-tap chunk) plus three times
// the larger run-to-run spread of the two kernels.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <math.h>
#include <random>
#include <stdio.h>
#include <stdlib.h>
#include <vector>

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int TAPS = 28, PAIRS = TAPS / 2;
constexpr int TAP_VOX = 16;                        // a tap moves the window by 16 voxels: the swizzle term of a lane's address stays put
constexpr int WAVE_VOX = 128, WAVE_CO = 32;
constexpr int IMG_VOX = 2 * WAVE_VOX + TAP_VOX * (TAPS - 1);      // 688 rows of 64 B: [8 heads | 8 heads | 8 tails | 8 tails]
constexpr int IMG_PIECES = IMG_VOX * 4;
constexpr int WSLOTS = 8;                          // weight taps held in registers; tap t uses slot t & 7
constexpr size_t W_HALVES = (size_t)WSLOTS * 2 * WAVE_CO * 16;    // [slot][head, tail][co][16 channels]
constexpr int LDS_REQUEST = 96 * 1024;             // more than half a CU's LDS: one workgroup per CU

// 16-byte piece q (0, 1: head octets; 2, 3: tail octets) of voxel v in the image, in bytes.  Sixteen consecutive voxels at one q cover
// the sixteen 16-byte slots of a 256-byte LDS row once, from any first voxel.
__host__ __device__ constexpr unsigned img_addr(unsigned v, unsigned q) { return (v * 4u + (q ^ ((v >> 2) & 3u))) * 16u; }

__device__ __forceinline__ half8 lds_read(const char* lds, unsigned base, unsigned imm) {
    return *reinterpret_cast<const half8*>(lds + base + imm);
}

// The products as written instructions, accumulating in place in AGPRs: left to the register allocator, the 16x16 loop rotates its
// accumulators through the body and pays 88 v_accvgpr moves per chunk for it.  The reads stay C++ loads (the compiler counts them in
// lgkmcnt); a sched_barrier behind every group keeps the order written here.
__device__ __forceinline__ void mfma32(f32x16& c, const half8& a, const half8& b) {
    asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, %0" : "+a"(c) : "v"(a), "v"(b));
}
__device__ __forceinline__ void mfma16(f32x4& c, const half8& a, const half8& b) {
    asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+a"(c) : "v"(a), "v"(b));
}

struct Stamp { unsigned long long t, rt; };
__device__ __forceinline__ Stamp stamp() {
    __builtin_amdgcn_sched_barrier(0);
    Stamp s{__builtin_amdgcn_s_memtime(), __builtin_amdgcn_s_memrealtime()};
    __builtin_amdgcn_sched_barrier(0);
    return s;
}

__device__ __forceinline__ void stage(char* lds, const uint4* x) {
    for (int i = threadIdx.x; i < IMG_PIECES; i += 256)
        *reinterpret_cast<uint4*>(lds + img_addr(i >> 2, i & 3)) = x[i];
    __syncthreads();
}

__device__ __forceinline__ void finish(const Stamp& s0, const Stamp& s1, unsigned long long* stamps, float* out, float v) {
    out[blockIdx.x * 256 + threadIdx.x] = v;
    if ((threadIdx.x & 63) == 0) {
        unsigned long long* w = stamps + (size_t)(blockIdx.x * 4 + (threadIdx.x >> 6)) * 4;
        w[0] = s0.t; w[1] = s0.rt; w[2] = s1.t; w[3] = s1.rt;
    }
}

// `step` is zero at run time: it only keeps the fragment reads inside the chunk loop.
// `tile`: [4 waves][32 co][128 voxels] of workgroup 0, or null.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
void probe_32x32x16(const uint4* __restrict__ x, const half8* __restrict__ w, float* __restrict__ out, unsigned long long* stamps,
                    int chunks, unsigned step, float* __restrict__ tile) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    stage(lds, x);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const unsigned v0 = (wave & 1) * WAVE_VOX + r;
    unsigned aH = img_addr(v0, h), aL = img_addr(v0, 2 + h);      // blocks (+32 voxels) and taps (+16) leave the swizzle term alone
    half8 wH[WSLOTS], wL[WSLOTS];
#pragma unroll
    for (int s = 0; s < WSLOTS; ++s) {
        wH[s] = w[((s * 2 + 0) * WAVE_CO + r) * 2 + h];
        wL[s] = w[((s * 2 + 1) * WAVE_CO + r) * 2 + h];
    }
    f32x16 acc[4] = {}, acc2[4] = {}, acc1[4] = {};
    half8 xh[2][4], xl[2][4];
#pragma unroll
    for (int b = 0; b < 4; ++b) { xh[0][b] = lds_read(lds, aH, b * 32 * 64); xl[0][b] = lds_read(lds, aL, b * 32 * 64); }
    const Stamp s0 = stamp();
    for (int c = 0; c < chunks; ++c) {
        aH += step; aL += step;
#pragma unroll
        for (int t = 0; t < TAPS; ++t) {
            const int cur = t & 1, nxt = cur ^ 1, tn = (t + 1) % TAPS, s = t & (WSLOTS - 1);
#pragma unroll
            for (int g = 0; g < 4; ++g) {                         // two reads of the next tap beside every three MFMAs of this one
                xh[nxt][g] = lds_read(lds, aH, (g * 32 + tn * TAP_VOX) * 64);
                xl[nxt][g] = lds_read(lds, aL, (g * 32 + tn * TAP_VOX) * 64);
#pragma unroll
                for (int i = 3 * g; i < 3 * g + 3; ++i) {         // WH.XH of the four blocks, then WL.XH, then WH.XL
                    const int b = i & 3;
                    if (i < 4) mfma32(t & 1 ? acc2[b] : acc[b], wH[s], xh[cur][b]);
                    else if (i < 8) mfma32(acc1[b], wL[s], xh[cur][b]);
                    else mfma32(acc1[b], wH[s], xl[cur][b]);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
    asm volatile("s_nop 15\n\ts_nop 15");                         // the last MFMAs' results, before VALU reads them
    const Stamp s1 = stamp();
    float sum = 0.f;
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const float v = acc[b][i] + acc2[b][i] + acc1[b][i];
            sum += v;
            if (tile && blockIdx.x == 0) {
                const int co = (i & 3) + 8 * (i >> 2) + 4 * h;    // C/D map of the 32x32 shapes: column on the lane
                tile[(wave * WAVE_CO + co) * WAVE_VOX + b * 32 + r] = v;
            }
        }
    finish(s0, s1, stamps, out, sum);
}

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
void probe_16x16x32(const uint4* __restrict__ x, const half8* __restrict__ w, float* __restrict__ out, unsigned long long* stamps,
                    int chunks, unsigned step, float* __restrict__ tile) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    stage(lds, x);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m = lane & 15, kg = lane >> 4;
    // K index 8 kg + j: octet kg & 1 of tap 2p + (kg >> 1).  The lane's own tap goes into its base address.
    const unsigned v0 = (wave & 1) * WAVE_VOX + m + (kg >> 1) * TAP_VOX;
    unsigned aH = img_addr(v0, kg & 1), aL = img_addr(v0, 2 + (kg & 1));
    half8 wH[WSLOTS / 2][2], wL[WSLOTS / 2][2];                   // [pair slot][row block of 16 channels]
#pragma unroll
    for (int s = 0; s < WSLOTS / 2; ++s)
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) {
            const int slot = 2 * s + (kg >> 1), co = rb * 16 + m;
            wH[s][rb] = w[((slot * 2 + 0) * WAVE_CO + co) * 2 + (kg & 1)];
            wL[s][rb] = w[((slot * 2 + 1) * WAVE_CO + co) * 2 + (kg & 1)];
        }
    f32x4 acc[2][8] = {}, acc1[2][8] = {};
    half8 xh[2][8], xl[2][8];
#pragma unroll
    for (int cb = 0; cb < 8; ++cb) { xh[0][cb] = lds_read(lds, aH, cb * 16 * 64); xl[0][cb] = lds_read(lds, aL, cb * 16 * 64); }
    const Stamp s0 = stamp();
    for (int c = 0; c < chunks; ++c) {
        aH += step; aL += step;
#pragma unroll
        for (int p = 0; p < PAIRS; ++p) {
            const int cur = p & 1, nxt = cur ^ 1, pn = (p + 1) % PAIRS, s = p & (WSLOTS / 2 - 1);
#pragma unroll
            for (int cb = 0; cb < 8; ++cb) {                      // one read of the next pair beside every three MFMAs of this one
                xh[nxt][cb] = lds_read(lds, aH, (cb * 16 + 2 * pn * TAP_VOX) * 64);
                mfma16(acc1[0][cb], wL[s][0], xh[cur][cb]);       // four MFMAs between the two sums into one cross block
                mfma16(acc1[1][cb], wL[s][1], xh[cur][cb]);
                mfma16(acc[0][cb], wH[s][0], xh[cur][cb]);
                __builtin_amdgcn_sched_barrier(0);
                xl[nxt][cb] = lds_read(lds, aL, (cb * 16 + 2 * pn * TAP_VOX) * 64);
                mfma16(acc[1][cb], wH[s][1], xh[cur][cb]);
                mfma16(acc1[0][cb], wH[s][0], xl[cur][cb]);
                mfma16(acc1[1][cb], wH[s][1], xl[cur][cb]);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
    asm volatile("s_nop 15\n\ts_nop 15");                         // the last MFMAs' results, before VALU reads them
    const Stamp s1 = stamp();
    float sum = 0.f;
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int cb = 0; cb < 8; ++cb)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float v = acc[rb][cb][i] + acc1[rb][cb][i];
                sum += v;
                if (tile && blockIdx.x == 0)                      // C/D map of the 16x16 shapes: row 4 (lane >> 4) + i, column lane & 15
                    tile[(wave * WAVE_CO + rb * 16 + 4 * kg + i) * WAVE_VOX + cb * 16 + m] = v;
            }
    finish(s0, s1, stamps, out, sum);
}

#define CK(e) do { hipError_t e_ = (e); if (e_ != hipSuccess) { printf("%s: %s\n", #e, hipGetErrorString(e_)); exit(1); } } while (0)

using Kern = void (*)(const uint4*, const half8*, float*, unsigned long long*, int, unsigned, float*);

static double med(std::vector<double> v) {
    if (v.empty()) return 0.0;
    std::sort(v.begin(), v.end());
    return v[v.size() / 2];
}

int main(int argc, char** argv) {
    const int chunks = argc > 1 ? atoi(argv[1]) : 40;
    if (chunks < 1) { printf("chunks per launch must be positive\n"); return 2; }
    hipDeviceProp_t prop; CK(hipGetDeviceProperties(&prop, 0));
    const int grid = prop.multiProcessorCount;
    printf("%s, %d CUs: one workgroup of 256 threads per CU, %d chunks of %d taps per launch\n", prop.gcnArchName, grid, chunks, TAPS);

    std::mt19937 rng(1234);
    std::normal_distribution<float> nd(0.f, 1.f);
    std::vector<_Float16> hx((size_t)IMG_PIECES * 8), hw(W_HALVES);
    for (auto& v : hx) v = (_Float16)nd(rng);
    for (auto& v : hw) v = (_Float16)nd(rng);
    void *x, *w; float *out, *tile; unsigned long long* st;
    const size_t tileN = 4 * WAVE_CO * WAVE_VOX;
    CK(hipMalloc(&x, hx.size() * 2)); CK(hipMalloc(&w, hw.size() * 2)); CK(hipMalloc(&out, (size_t)grid * 256 * 4));
    CK(hipMalloc(&tile, tileN * 4)); CK(hipMalloc(&st, (size_t)grid * 4 * 4 * 8));
    CK(hipMemcpy(x, hx.data(), hx.size() * 2, hipMemcpyHostToDevice)); CK(hipMemcpy(w, hw.data(), hw.size() * 2, hipMemcpyHostToDevice));
    const Kern kern[2] = {probe_32x32x16, probe_16x16x32};
    const char* name[2] = {"(a) 32x32x16", "(b) 16x16x32"};
    for (int k = 0; k < 2; ++k)
        CK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern[k]), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_REQUEST));
    auto launch = [&](int k, int n, float* t) {
        hipLaunchKernelGGL(kern[k], dim3(grid), dim3(256), LDS_REQUEST, 0, (const uint4*)x, (const half8*)w, out, st, n, 0u, t);
    };

    // the sums both kernels have to give: two chunks, float64 on the host
    std::vector<double> ref(2 * WAVE_CO * WAVE_VOX, 0.0);
    auto X = [&](int v, int q, int j) { return (double)hx[((size_t)v * 4 + q) * 8 + j]; };
    auto W = [&](int s, int hl, int co, int ch) { return (double)hw[(((size_t)s * 2 + hl) * WAVE_CO + co) * 16 + ch]; };
    double refMax = 0.0;
    for (int half = 0; half < 2; ++half)
        for (int co = 0; co < WAVE_CO; ++co)
            for (int v = 0; v < WAVE_VOX; ++v) {
                double a = 0.0;
                for (int t = 0; t < TAPS; ++t)
                    for (int ch = 0; ch < 16; ++ch) {
                        const int vv = half * WAVE_VOX + v + t * TAP_VOX, s = t & (WSLOTS - 1);
                        const double xH = X(vv, ch >> 3, ch & 7), xL = X(vv, 2 + (ch >> 3), ch & 7);
                        a += W(s, 0, co, ch) * xH + W(s, 1, co, ch) * xH + W(s, 0, co, ch) * xL;
                    }
                ref[(half * WAVE_CO + co) * WAVE_VOX + v] = 2.0 * a;
                refMax = std::max(refMax, fabs(2.0 * a));
            }
    std::vector<float> ht(tileN);
    for (int k = 0; k < 2; ++k) {
        CK(hipMemset(tile, 0, tileN * 4));
        launch(k, 2, tile);
        CK(hipDeviceSynchronize());
        CK(hipMemcpy(ht.data(), tile, tileN * 4, hipMemcpyDeviceToHost));
        double err = 0.0;
        for (int wv = 0; wv < 4; ++wv)
            for (int i = 0; i < WAVE_CO * WAVE_VOX; ++i)
                err = std::max(err, fabs((double)ht[(size_t)wv * WAVE_CO * WAVE_VOX + i] - ref[(wv & 1) * WAVE_CO * WAVE_VOX + i]));
        printf("%s: max error %.3g of max |ref| %.3g\n", name[k], err, refMax);
        if (!(err <= 1e-5 * refMax)) { printf("wrong sums: no measurement\n"); return 1; }
    }

    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    double us[2][3], mhz[2][3], cyc[2][3];
    std::vector<unsigned long long> hs((size_t)grid * 4 * 4);
    for (int round = 0; round < 3; ++round)
        for (int k = 0; k < 2; ++k) {
            const auto t0 = std::chrono::steady_clock::now();
            long launches = 0;
            while (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() < 2.2) {
                for (int i = 0; i < 200; ++i) launch(k, chunks, nullptr);
                CK(hipDeviceSynchronize());
                launches += 200;
            }
            CK(hipEventRecord(e0));
            for (int i = 0; i < 1000; ++i) launch(k, chunks, nullptr);
            CK(hipEventRecord(e1)); CK(hipDeviceSynchronize());
            float ms = 0; CK(hipEventElapsedTime(&ms, e0, e1));
            CK(hipMemcpy(hs.data(), st, hs.size() * 8, hipMemcpyDeviceToHost));
            std::vector<double> clk, life;
            for (size_t wv = 0; wv < (size_t)grid * 4; ++wv) {
                const unsigned long long* q = &hs[wv * 4];
                if (q[3] <= q[1] || q[2] <= q[0]) continue;
                clk.push_back((double)(q[2] - q[0]) / (double)(q[3] - q[1]) * 100.0);
                life.push_back((double)(q[2] - q[0]));
            }
            us[k][round] = ms * 1e3 / 1000; mhz[k][round] = med(clk); cyc[k][round] = med(life) / ((double)chunks * TAPS);
            printf("round %d %s: %8.2f us per launch (1000 launches after %ld), in-kernel clock %.0f MHz, %.1f cycles per tap "
                   "(MFMA floor 384), %.0f TFLOP/s\n", round, name[k], us[k][round], launches, mhz[k][round], cyc[k][round],
                   2.0 * 12 * 32 * 32 * 16 * TAPS * chunks * 4.0 * grid / (us[k][round] * 1e-6) * 1e-12);
        }
    double m[2], spread[2];
    for (int k = 0; k < 2; ++k) {
        std::vector<double> v(us[k], us[k] + 3);
        m[k] = med(v);
        spread[k] = (*std::max_element(v.begin(), v.end()) - *std::min_element(v.begin(), v.end())) / m[k];
    }
    const double gain = m[0] / m[1] - 1.0, need = 0.037 + 3.0 * std::max(spread[0], spread[1]);
    printf("median wall: (a) %.2f us (spread %.2f %%), (b) %.2f us (spread %.2f %%); (a) / (b) - 1 = %+.2f %%, needed more than %.2f %%: %s\n",
           m[0], spread[0] * 100, m[1], spread[1] * 100, gain * 100, need * 100, gain > need ? "GO" : "NO-GO");
    CK(hipFree(x)); CK(hipFree(w)); CK(hipFree(out)); CK(hipFree(tile)); CK(hipFree(st));
    return 0;
}
