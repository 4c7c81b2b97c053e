// Training data path and validation metrics on the device:
//   * random-crop patch pairs out of HBM-resident volume pairs (data.py:50-137 supervisedIQT.__getitem__: the crop, the
//     z-score / min-max normalisation; the crop origins and the non-zero rejection are decided by the host from a
//     summed-area table, diffusioniqt_amd/data.py),
//   * PSNR / SSIM of valid_step (metrics.py:19-31 -> torchmetrics 0.9.0 peak_signal_noise_ratio and
//     StructuralSimilarityIndexMeasure on min-max normalised 5-D tensors),
//   * MS-SSIM of the evaluation script (metrics.py:32-34 MSSIM, called per volume at test_all.py:56-62 -> torchmetrics 0.9.0
//     MultiScaleStructuralSimilarityIndexMeasure): the SSIM tile kernel once per scale, which also pools the next scale,
//   * weighted overlap blending of the sliding windows of a whole volume with the per-voxel spread of several samples
//     (diffusioniqt_amd/inference.py, blend modes; in place of the crop-and-overwrite stitching of test_all.py:235-300),
//   * volume-anchored sampler noise: Philox4x32-10 keyed by the seed and counted by the voxel's position in the VOLUME, so overlapping
//     windows draw the same noise (diffusioniqt_amd/inference.py, noise='anchored'; in place of one torch.randn per window batch).
//   * lockstep joint sampling of the overlapping windows: one reverse step of the noisy state of the whole volume per launch -- the
//     blend walk over the windows' x0 predictions, the sampler step and the anchored noise fused (diffusioniqt_amd/inference.py,
//     joint=True), and the per-sample finish (fill, background reset, statistics over the samples),
//   * the sigma-space DPM-Solver++ 2M step of the EDM family (ElucidatedImagen(sampler='dpmpp2m'), ODE and SDE), per window batch and
//     on the joint state,
//   * data consistency between the fuse and the update of those chains: cell means, slice profiles, tile operators, overlapping slabs
//     and the k-space band limit, whose projector is three dense passes of real circulants along the axes (band_pass_kernel).
// All reductions are two-stage with a fixed order (bit-reproducible).
#include "common.h"

namespace diqt {
#define STREAM ((hipStream_t)stream)

struct MinMax { float lo, hi; };

__device__ __forceinline__ MinMax wg_minmax(float lo, float hi, MinMax* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, o, 64));
        hi = fmaxf(hi, __shfl_xor(hi, o, 64));
    }
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = MinMax{lo, hi};
    __syncthreads();
    MinMax r = sh[0];
    for (unsigned w = 1; w < blockDim.x / 64; ++w) { r.lo = fminf(r.lo, sh[w].lo); r.hi = fmaxf(r.hi, sh[w].hi); }
    __syncthreads();
    return r;
}

// sel[n] = {volume, i0, j0, k0}.  grid (nb, n, 2): z = 0 low-res, 1 high-res.
__global__ __launch_bounds__(256) void crop_minmax_kernel(const float* __restrict__ lr, const float* __restrict__ hr,
                                                          const int* __restrict__ sel, MinMax* __restrict__ part, int D, int H,
                                                          int W, int P) {
    __shared__ MinMax sh[4];
    const int n = blockIdx.y;
    const float* vol = (blockIdx.z ? hr : lr) + (size_t)sel[4 * n] * D * H * W;
    const int i0 = sel[4 * n + 1], j0 = sel[4 * n + 2], k0 = sel[4 * n + 3];
    const size_t per = (size_t)P * P * P;
    float lo = INFINITY, hi = -INFINITY;
    for (size_t e = blockIdx.x * (size_t)256 + threadIdx.x; e < per; e += (size_t)gridDim.x * 256) {
        const int k = (int)(e % P), j = (int)((e / P) % P), i = (int)(e / ((size_t)P * P));
        const float v = vol[((size_t)(i0 + i) * H + (j0 + j)) * W + (k0 + k)];
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
    }
    const MinMax r = wg_minmax(lo, hi, sh);
    if (threadIdx.x == 0) part[((size_t)blockIdx.z * gridDim.y + n) * gridDim.x + blockIdx.x] = r;
}
// mode 0: (v - mean) / std ; mode 1: 2 * ((v - min) / (max - min) - 0.5) with the patch's own min / max (data.py:82-86)
__global__ __launch_bounds__(256) void crop_apply_kernel(const float* __restrict__ lr, const float* __restrict__ hr,
                                                         const int* __restrict__ sel, const MinMax* __restrict__ part,
                                                         float* __restrict__ lr_out, float* __restrict__ hr_out, int D, int H, int W,
                                                         int P, int mode, float mean, float stdv) {
    const int n = blockIdx.y;
    const float* vol = (blockIdx.z ? hr : lr) + (size_t)sel[4 * n] * D * H * W;
    float* out = (blockIdx.z ? hr_out : lr_out) + (size_t)n * P * P * P;
    const int i0 = sel[4 * n + 1], j0 = sel[4 * n + 2], k0 = sel[4 * n + 3];
    const size_t per = (size_t)P * P * P;
    float lo = 0.f, range = 1.f;
    if (mode == 1) {
        const MinMax* pp = part + ((size_t)blockIdx.z * gridDim.y + n) * gridDim.x;
        float hi = -INFINITY;
        lo = INFINITY;
        for (unsigned b = 0; b < gridDim.x; ++b) { lo = fminf(lo, pp[b].lo); hi = fmaxf(hi, pp[b].hi); }
        range = hi - lo;
    }
    for (size_t e = blockIdx.x * (size_t)256 + threadIdx.x; e < per; e += (size_t)gridDim.x * 256) {
        const int k = (int)(e % P), j = (int)((e / P) % P), i = (int)(e / ((size_t)P * P));
        const float v = vol[((size_t)(i0 + i) * H + (j0 + j)) * W + (k0 + k)];
        out[e] = mode == 1 ? 2.f * ((v - lo) / range - 0.5f) : (v - mean) / stdv;
    }
}

// ---- global min / max -----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void minmax_stage1_kernel(const float* __restrict__ x, MinMax* __restrict__ part, size_t n) {
    __shared__ MinMax sh[4];
    float lo = INFINITY, hi = -INFINITY;
    for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const float v = x[i];
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
    }
    const MinMax r = wg_minmax(lo, hi, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = r;
}
__global__ __launch_bounds__(64) void minmax_stage2_kernel(const MinMax* __restrict__ part, int nb, float* __restrict__ out) {
    float lo = INFINITY, hi = -INFINITY;
    for (int i = threadIdx.x; i < nb; i += 64) { lo = fminf(lo, part[i].lo); hi = fmaxf(hi, part[i].hi); }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, o, 64));
        hi = fmaxf(hi, __shfl_xor(hi, o, 64));
    }
    if (threadIdx.x == 0) { out[0] = lo; out[1] = hi; }
}

// ---- PSNR: mean squared error of the (optionally min-max normalised) tensors -----------------------------------------
// stats = {pred min, pred max, target min, target max} on the device, or NULL for "compare as they are"
__global__ __launch_bounds__(256) void sqerr_stage1_kernel(const float* __restrict__ p, const float* __restrict__ t,
                                                           const float* __restrict__ stats, double* __restrict__ part, size_t n) {
    __shared__ double sh[4];
    float pl = 0.f, pr = 1.f, tl = 0.f, tr = 1.f;
    if (stats) { pl = stats[0]; pr = stats[1] - stats[0]; tl = stats[2]; tr = stats[3] - stats[2]; }
    double acc = 0.0;
    for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const float a = stats ? (p[i] - pl) / pr : p[i], b = stats ? (t[i] - tl) / tr : t[i];
        const float d = a - b;
        acc += (double)(d * d);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}
// out[0] = mse, out[1] = 10 log10(data_range^2 / mse)   (torchmetrics 0.9.0 functional/image/psnr.py: _psnr_compute, base 10)
__global__ __launch_bounds__(64) void psnr_stage2_kernel(const double* __restrict__ part, int nb, double count, float data_range,
                                                         float* __restrict__ out) {
    if (threadIdx.x) return;
    double s = 0.0;
    for (int i = 0; i < nb; ++i) s += part[i];
    const float mse = (float)(s / count);
    out[0] = mse;
    out[1] = (2.f * logf(data_range) - logf(mse)) * (10.f / logf(10.f));
}

// ---- SSIM ------------------------------------------------------------------------------------------------------------
// torchmetrics 0.9.0 functional/image/ssim.py _ssim_compute on 5-D input: reflect-pad by R = (K-1)/2, depthwise K^3 Gaussian
// filter of {p, t, p^2, t^2, p t}, SSIM map, crop R from every face, mean.  After the crop only windows that lie fully inside
// the un-padded volume survive, so the padding never contributes: the kernel evaluates the "valid" windows only.
constexpr int ST = 8;           // outputs per tile edge
constexpr int SK = 11;          // largest filter
constexpr int SI = ST + SK - 1; // input tile edge (18)
struct SsimTaps { float w[SK]; int K; };
// MS-SSIM only (torchmetrics 0.9.0 _multiscale_ssim_compute, one launch per scale): c1 / c2 come from range[0] on the device, the
// contrast-sensitivity sums go to part[gridDim.x + block], and when pool_p is set the tile also writes the 2x2x2 average pool of the
// raw voxels it OWNS (its 8^3 output corner; the last tile of an axis owns the rest, at most I voxels, all inside the tile it
// loaded) with their {p min, p max, t min, t max} to mm[4 * block] -- the next scale's input and data range.
struct MsScale { const float* range; float k1, k2; float* pool_p; float* pool_t; float* mm; };

template <bool MS>
__global__ __launch_bounds__(256) void ssim_tile_kernel(const float* __restrict__ p, const float* __restrict__ t,
                                                        const float* __restrict__ stats, double* __restrict__ part, int D, int H,
                                                        int W, int tilesD, int tilesH, int tilesW, SsimTaps taps, float c1,
                                                        float c2, MsScale ms) {
    extern __shared__ float lds[];
    const int K = taps.K, I = ST + K - 1;
    float* raw = lds;                                  // [2][I][I][I]
    float* f1 = raw + 2 * SI * SI * SI;                // [5][I][I][ST]   filtered along W
    float* f2 = f1 + 5 * SI * SI * ST;                 // [5][I][ST][ST]  filtered along H
    __shared__ double sh[4];
    const int Do = D - K + 1, Ho = H - K + 1, Wo = W - K + 1;
    unsigned b = blockIdx.x;
    const int tw = b % tilesW; b /= tilesW;
    const int th = b % tilesH; b /= tilesH;
    const int td = b % tilesD;
    const int vol = b / tilesD;
    const float* pv = p + (size_t)vol * D * H * W;
    const float* tv = t + (size_t)vol * D * H * W;
    float pl = 0.f, pr = 1.f, tl = 0.f, tr = 1.f;
    if (stats) { pl = stats[0]; pr = stats[1] - stats[0]; tl = stats[2]; tr = stats[3] - stats[2]; }
    const int d0 = td * ST, h0 = th * ST, w0 = tw * ST;
    if constexpr (MS) {
        const float r = ms.range[0];
        c1 = (ms.k1 * r) * (ms.k1 * r);
        c2 = (ms.k2 * r) * (ms.k2 * r);
    }
    for (int e = threadIdx.x; e < I * I * I; e += 256) {
        const int k = e % I, j = (e / I) % I, i = e / (I * I);
        const int di = min(d0 + i, D - 1), hj = min(h0 + j, H - 1), wk = min(w0 + k, W - 1);   // clamped reads feed masked outputs only
        const size_t off = ((size_t)di * H + hj) * W + wk;
        const float a = pv[off], c = tv[off];
        raw[(i * SI + j) * SI + k] = stats ? (a - pl) / pr : a;
        raw[SI * SI * SI + (i * SI + j) * SI + k] = stats ? (c - tl) / tr : c;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < I * I * ST; e += 256) {          // along W
        const int k = e % ST, j = (e / ST) % I, i = e / (ST * I);
        const float* rp = raw + (i * SI + j) * SI + k;
        const float* rt = rp + SI * SI * SI;
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f, s4 = 0.f;
        for (int q = 0; q < K; ++q) {
            const float w = taps.w[q], a = rp[q], c = rt[q];
            s0 = fmaf(w, a, s0); s1 = fmaf(w, c, s1); s2 = fmaf(w, a * a, s2); s3 = fmaf(w, c * c, s3); s4 = fmaf(w, a * c, s4);
        }
        float* o = f1 + (i * SI + j) * ST + k;
        o[0] = s0; o[SI * SI * ST] = s1; o[2 * SI * SI * ST] = s2; o[3 * SI * SI * ST] = s3; o[4 * SI * SI * ST] = s4;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < 5 * I * ST * ST; e += 256) {     // along H
        const int k = e % ST, j = (e / ST) % ST, i = (e / (ST * ST)) % I, f = e / (ST * ST * I);
        const float* r = f1 + f * SI * SI * ST + (i * SI + j) * ST + k;
        float s = 0.f;
        for (int q = 0; q < K; ++q) s = fmaf(taps.w[q], r[q * ST], s);
        f2[f * SI * ST * ST + (i * ST + j) * ST + k] = s;
    }
    __syncthreads();
    double acc = 0.0, acc_cs = 0.0;
    for (int e = threadIdx.x; e < ST * ST * ST; e += 256) {        // along D + the SSIM map
        const int k = e % ST, j = (e / ST) % ST, i = e / (ST * ST);
        if (d0 + i >= Do || h0 + j >= Ho || w0 + k >= Wo) continue;
        float m[5];
#pragma unroll
        for (int f = 0; f < 5; ++f) {
            const float* r = f2 + f * SI * ST * ST + (i * ST + j) * ST + k;
            float s = 0.f;
            for (int q = 0; q < K; ++q) s = fmaf(taps.w[q], r[q * ST * ST], s);
            m[f] = s;
        }
        const float mp2 = m[0] * m[0], mt2 = m[1] * m[1], mpt = m[0] * m[1];
        const float sp = m[2] - mp2, stt = m[3] - mt2, spt = m[4] - mpt;
        const float upper = 2.f * spt + c2, lower = sp + stt + c2;
        acc += (double)(((2.f * mpt + c1) * upper) / ((mp2 + mt2 + c1) * lower));
        if constexpr (MS) acc_cs += (double)(upper / lower);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
    if constexpr (MS) {
        __shared__ MinMax shm[4];
        __syncthreads();
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc_cs += __shfl_xor(acc_cs, o, 64);
        if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc_cs;
        __syncthreads();
        if (threadIdx.x == 0) part[gridDim.x + blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
        if (!ms.pool_p) return;
        const int D2 = D / 2, H2 = H / 2, W2 = W / 2;               // avg_pool3d(2): a trailing odd plane / row / column is dropped
        const int a0 = d0 / 2, b0 = h0 / 2, c0 = w0 / 2;
        const int na = (td == tilesD - 1 ? D2 : a0 + ST / 2) - a0, nb = (th == tilesH - 1 ? H2 : b0 + ST / 2) - b0,
                  nc = (tw == tilesW - 1 ? W2 : c0 + ST / 2) - c0;
        float plo = INFINITY, phi = -INFINITY, tlo = INFINITY, thi = -INFINITY;
        for (int e = threadIdx.x; e < na * nb * nc; e += 256) {
            const int c = e % nc, bb = (e / nc) % nb, a = e / (nc * nb);
            const float* rp = raw + (2 * a * SI + 2 * bb) * SI + 2 * c;
            const float* rt = rp + SI * SI * SI;
            const float vp = (((rp[0] + rp[1]) + (rp[SI] + rp[SI + 1])) +
                              ((rp[SI * SI] + rp[SI * SI + 1]) + (rp[SI * SI + SI] + rp[SI * SI + SI + 1]))) * 0.125f;
            const float vt = (((rt[0] + rt[1]) + (rt[SI] + rt[SI + 1])) +
                              ((rt[SI * SI] + rt[SI * SI + 1]) + (rt[SI * SI + SI] + rt[SI * SI + SI + 1]))) * 0.125f;
            const size_t off = (((size_t)vol * D2 + (a0 + a)) * H2 + (b0 + bb)) * W2 + (c0 + c);
            ms.pool_p[off] = vp;
            ms.pool_t[off] = vt;
            plo = fminf(plo, vp); phi = fmaxf(phi, vp);
            tlo = fminf(tlo, vt); thi = fmaxf(thi, vt);
        }
        const MinMax mp = wg_minmax(plo, phi, shm), mt = wg_minmax(tlo, thi, shm);
        if (threadIdx.x == 0) {
            float* o = ms.mm + 4 * (size_t)blockIdx.x;
            o[0] = mp.lo; o[1] = mp.hi; o[2] = mt.lo; o[3] = mt.hi;
        }
    }
}
__global__ __launch_bounds__(64) void mean_stage2_kernel(const double* __restrict__ part, int nb, double count, float* __restrict__ out) {
    if (threadIdx.x) return;
    double s = 0.0;
    for (int i = 0; i < nb; ++i) s += part[i];
    out[0] = (float)(s / count);
}

// ---- MS-SSIM: the small kernels between the per-scale tile launches ---------------------------------------------------------
constexpr int MS_MAX_SCALES = 16;      // every axis halves per scale: more scales than this need a volume no device holds
struct MsBetas { float b[MS_MAX_SCALES]; };

// range_0 = max(p.max - p.min, t.max - t.min) from the two minmax_stage1_kernel partial sets (nb each)
__global__ __launch_bounds__(64) void msssim_range0_kernel(const MinMax* __restrict__ part, int nb, float* __restrict__ range) {
    float r[2];
    for (int v = 0; v < 2; ++v) {
        float lo = INFINITY, hi = -INFINITY;
        for (int i = threadIdx.x; i < nb; i += 64) { lo = fminf(lo, part[v * nb + i].lo); hi = fmaxf(hi, part[v * nb + i].hi); }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            lo = fminf(lo, __shfl_xor(lo, o, 64));
            hi = fmaxf(hi, __shfl_xor(hi, o, 64));
        }
        r[v] = hi - lo;
    }
    if (threadIdx.x == 0) range[0] = fmaxf(r[0], r[1]);
}
// One workgroup per scale, fixed summation order: thread i adds partials i, i + 256, ...; then the xor tree; then the four waves.
// out[1 + 3 s ..] = {ssim_s, cs_s, range_s}; range[s + 1] for the next tile launch; the last scale forms
// out[0] = prod_j term_j ^ beta_j (term = cs below the last scale, ssim at it; no clamp: a negative term gives NaN, as torch.pow).
__global__ __launch_bounds__(256) void msssim_final_kernel(const double* __restrict__ part, const float* __restrict__ mm, int nb,
                                                           double count, float* __restrict__ range, float* __restrict__ out, int s,
                                                           int scales, MsBetas betas) {
    __shared__ double sh[2][4];
    __shared__ MinMax shm[4];
    const bool last = s + 1 == scales;
    double a = 0.0, c = 0.0;
    float plo = INFINITY, phi = -INFINITY, tlo = INFINITY, thi = -INFINITY;
    for (int i = threadIdx.x; i < nb; i += 256) {
        a += part[i];
        c += part[nb + i];
        if (!last) {
            const float* m = mm + 4 * (size_t)i;
            plo = fminf(plo, m[0]); phi = fmaxf(phi, m[1]);
            tlo = fminf(tlo, m[2]); thi = fmaxf(thi, m[3]);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_xor(a, o, 64);
        c += __shfl_xor(c, o, 64);
    }
    if ((threadIdx.x & 63) == 0) { sh[0][threadIdx.x >> 6] = a; sh[1][threadIdx.x >> 6] = c; }
    const MinMax mp = wg_minmax(plo, phi, shm), mt = wg_minmax(tlo, thi, shm);      // (its barriers publish sh too)
    if (threadIdx.x) return;
    const float ssim = (float)(((sh[0][0] + sh[0][1]) + (sh[0][2] + sh[0][3])) / count);
    const float cs = (float)(((sh[1][0] + sh[1][1]) + (sh[1][2] + sh[1][3])) / count);
    out[1 + 3 * s] = ssim;
    out[2 + 3 * s] = cs;
    out[3 + 3 * s] = range[s];
    if (!last) {
        range[s + 1] = fmaxf(mp.hi - mp.lo, mt.hi - mt.lo);
        return;
    }
    float prod = 1.f;
    for (int j = 0; j < scales; ++j) prod *= powf(j == s ? ssim : out[2 + 3 * j], betas.b[j]);
    out[0] = prod;
}

// ---- whole-volume inference: weighted overlap blending of the kept windows, with a per-voxel spread over S samples ----------
// Gather-side: one thread per OUTPUT voxel walks the windows that cover it in candidate order (g0, g1, g2 ascending on the origin
// lattice g * stride), so nothing is written twice, there is no atomic, and the sum order is a function of the voxel alone.
// patches[S][N][P][P][P]; slot[G0][G1][G2] = row of the window in `patches`, < 0 for a window that was not kept.  Per sample:
// b_s = sum(w y) / sum(w), w = (taps[i] taps[j]) taps[k] (the product accumulated with one fma per term); out_mean / out_std =
// Welford mean / unbiased deviation of b_s in sample order.  A voxel no kept window covers gets `fill`; a voxel whose normalised
// low-res value equals min_val gets min_val (background_reset_kernel's rule and expression), both with deviation 0.
// Block (64, 4): a wave owns 64 voxels of one row, so d, h and with them the g0 / g1 ranges, taps[i] taps[j] and the slot row are
// wave-uniform; only the g2 range is per lane (any stride, also one that does not divide P).  Lanes of one window read consecutive
// floats.  Every element of `patches` is read exactly once per launch.
// The window walk of one output voxel (d, h, x) over one sample's rows `ps`: num = sum(w c(y)), den = sum(w) over the covering kept
// windows in candidate order, with c the caller's clamp (the identity for the blend).  Shared by volume_blend_kernel and
// the joint kernels (joint_fuse), so they fuse windows with the same terms in the same order.
struct Cover { int lo0, hi0, lo1, hi1, lo2, hi2; };
// covering lattice indices of coordinate c: 0 <= g < G and 0 <= c - g * stride < P
__device__ __forceinline__ Cover covering(int d, int h, int x, int P, int stride, int G0, int G1, int G2) {
    return Cover{max(0, (d - P + stride) / stride), min(G0 - 1, d / stride), max(0, (h - P + stride) / stride), min(G1 - 1, h / stride),
                 max(0, (x - P + stride) / stride), min(G2 - 1, x / stride)};
}
struct NoClamp {
    __device__ __forceinline__ float operator()(float y) const { return y; }
};
template <class Clamp>
__device__ __forceinline__ void window_walk(const float* __restrict__ ps, const int* __restrict__ slot, const float* __restrict__ taps,
                                            const float* tp, int N, int P, int stride, int G1, int G2, int d, int h, int x,
                                            const Cover& cv, Clamp c, float& num, float& den) {
    const size_t per = (size_t)P * P * P;
    num = 0.f;
    den = 0.f;
    for (int g0 = cv.lo0; g0 <= cv.hi0; ++g0) {
        const int i = d - g0 * stride;
        const float wi = tp[i];
        for (int g1 = cv.lo1; g1 <= cv.hi1; ++g1) {
            const int j = h - g1 * stride;
            const float wij = wi * tp[j];
            const int* srow = slot + ((size_t)g0 * G1 + g1) * G2;
            const float* prow = ps + ((size_t)i * P + j) * P;
            // four windows per trip: their slot reads, then their patch reads, are independent loads in flight together (one
            // window per trip is a chain of two dependent loads, and the kernel ran at the memory latency).  A window that is
            // not kept (-1), or lies past hi2, reads taps[0] instead and enters with weight 0: adding +0 terms changes no bit.
            for (int g2 = cv.lo2; g2 <= cv.hi2; g2 += 4) {
                int n[4];
                float w[4], y[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int nn = srow[min(g2 + u, cv.hi2)];
                    n[u] = g2 + u <= cv.hi2 ? nn : -1;
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const bool ok = (unsigned)n[u] < (unsigned)N;
                    const int k = ok ? x - (g2 + u) * stride : 0;
                    const float yy = *(ok ? prow + (size_t)n[u] * per + k : taps);
                    w[u] = ok ? wij * tp[k] : 0.f;
                    y[u] = ok ? c(yy) : 0.f;
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    num = fmaf(w[u], y[u], num);
                    den += w[u];
                }
            }
        }
    }
}

// The output voxel of a thread of the (64, 4) block on the grid (ceil(W / 64), ceil(H / 4), D): x per lane, h and d wave-uniform, v its
// index in a [D][H][W] volume (= the Philox `lin` of channel 0), inside = false for the lanes and rows past the volume.
struct Voxel { int x, h, d; size_t v; bool inside; };
__device__ __forceinline__ Voxel block_voxel(int H, int W) {
    const int x = blockIdx.x * 64 + threadIdx.x;
    const int h = __builtin_amdgcn_readfirstlane(blockIdx.y * 4 + threadIdx.y), d = blockIdx.z;
    return Voxel{x, h, d, ((size_t)d * H + h) * W + x, h < H && x < W};
}
// The head of every kernel that walks windows: taps -> LDS tp[P] when this launch walks (`walks` is uniform over the launch; a launch
// that does not -- an initial state -- gets no LDS and reads no taps), a barrier BEFORE any thread may leave, then the thread's voxel.
__device__ __forceinline__ Voxel walk_prologue(float* tp, const float* __restrict__ taps, int P, bool walks, int H, int W) {
    if (walks) {
        for (int e = threadIdx.y * 64 + threadIdx.x; e < P; e += 256) tp[e] = taps[e];
        __syncthreads();
    }
    return block_voxel(H, W);
}

__global__ __launch_bounds__(256) void volume_blend_kernel(const float* __restrict__ patches, const int* __restrict__ slot,
                                                           const float* __restrict__ taps, const float* __restrict__ vol,
                                                           float* __restrict__ out_mean, float* __restrict__ out_std, int S, int N,
                                                           int D, int H, int W, int P, int stride, int G0, int G1, int G2, float mean,
                                                           float stdv, float min_val, float fill) {
    extern __shared__ float tp[];                      // [P]
    const Voxel p = walk_prologue(tp, taps, P, true, H, W);
    if (!p.inside) return;
    const int x = p.x, h = p.h, d = p.d;
    const size_t v = p.v;
    float om, os = 0.f;
    if (vol && (vol[v] - mean) / stdv == min_val) {
        om = min_val;
    } else {
        const Cover cv = covering(d, h, x, P, stride, G0, G1, G2);
        const size_t per = (size_t)P * P * P;
        float m = 0.f, m2 = 0.f, den = 0.f;
        for (int s = 0; s < S; ++s) {
            float num;                                  // den: the same terms in the same order for every s
            window_walk(patches + (size_t)s * N * per, slot, taps, tp, N, P, stride, G1, G2, d, h, x, cv, NoClamp{}, num, den);
            if (den == 0.f) break;
            const float b = num / den, delta = b - m;
            m += delta / (float)(s + 1);
            m2 = fmaf(delta, b - m, m2);
        }
        if (den == 0.f) {
            om = fill;
        } else {
            om = m;
            if (S > 1) os = sqrtf(m2 / (float)(S - 1));
        }
    }
    out_mean[v] = om;
    if (out_std) out_std[v] = os;
}

// ---- volume-anchored noise: a counter-based generator evaluated per output voxel ------------------------------------------------------
// The value at global voxel (z, y, x) of channel c, draw k, sample s is a pure function of (seed, c, z, y, x, k, s): Philox4x32-10
// (Salmon et al., SC'11; Random123's constants) with counter {lin & 0xffffffff, lin >> 32, draw, sample}, lin = ((c D + z) H + y) W + x in
// 64 bits, and key {seed & 0xffffffff, seed >> 32}.  Every window that covers a voxel therefore sees the same number, whatever the batch
// it came in.  ONE call per voxel, words r0 / r1 used and r2 / r3 dropped: sharing a call between four neighbours would tie the value to
// the window's alignment along x, and the whole launch is tens of microseconds beside a U-Net evaluation.
struct Philox { unsigned r0, r1; };
__device__ __forceinline__ Philox philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0, p1 = (unsigned long long)0xCD9E8D57u * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
        c1 = (unsigned)p1;
        c3 = (unsigned)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return Philox{c0, c1};
}
// Box-Muller on u1 = ((r0 >> 9) + 0.5) 2^-23 in (0, 1) and u2 = (r1 >> 8) 2^-24 in [0, 1), both exact in fp32, with the accurate
// logf / sqrtf / cospif.
__device__ __forceinline__ float philox_normal(Philox r) {
    const float u1 = ((float)(r.r0 >> 9) + 0.5f) * 1.1920928955078125e-7f;       // 2^-23
    const float u2 = (float)(r.r1 >> 8) * 5.9604644775390625e-8f;                // 2^-24
    return sqrtf(-2.f * logf(u1)) * cospif(2.f * u2);
}
// out[b][c][i][j][k] for the window origins[b] = {z0, y0, x0}; one thread per output voxel, consecutive lanes = consecutive k.
// RAW: the two words as they are (int32 pairs), otherwise philox_normal of them.
template <bool RAW>
__global__ __launch_bounds__(256) void anchored_noise_kernel(const int* __restrict__ origins, void* __restrict__ out, size_t total, int C,
                                                             int P, int D, int H, int W, unsigned k0, unsigned k1, unsigned draw,
                                                             unsigned sample) {
    const size_t per = (size_t)P * P * P;
    for (size_t e = blockIdx.x * (size_t)256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const size_t w = e / per;                              // b * C + c
        const unsigned v = (unsigned)(e - w * per), pp = (unsigned)P * P;
        const unsigned i = v / pp, j = (v - i * pp) / P, k = v - i * pp - j * P;
        const int b = (int)(w / C), c = (int)(w - (size_t)b * C);
        const int* o = origins + 3 * (size_t)b;
        const unsigned long long lin = (((unsigned long long)c * D + (unsigned)(o[0] + i)) * H + (unsigned)(o[1] + j)) * W + (unsigned)(o[2] + k);
        const Philox r = philox4x32_10((unsigned)lin, (unsigned)(lin >> 32), draw, sample, k0, k1);
        if constexpr (RAW) {
            static_cast<int2*>(out)[e] = make_int2((int)r.r0, (int)r.r1);
        } else {
            static_cast<float*>(out)[e] = philox_normal(r);
        }
    }
}

// ---- lockstep joint sampling of the overlapping windows: one noisy state for the whole volume ------------------------------------------
// One reverse step of the VOLUME (MultiDiffusion, Bar-Tal et al. 2023): y[N][P][P][P] holds the kept windows' x0 predictions of this
// step; per output voxel x0 = sum(w c(y)) / sum(w) over the covering kept windows -- volume_blend_kernel's walk for S = 1 with
// ddpm_step_kernel's clamp c on every term -- and x_next = kx x_t + k0 x0 + kn n with n the anchored normal of channel 0 at (seed, d, h,
// x, draw, sample), computed in the thread (no noise tensor, no blended x0 tensor, no separate step launch).  The multistep and Heun
// samplers put other updates behind the same fuse; volume_joint_linear_kernel and volume_joint_heun_kernel say which.
// ddpm_step_kernel's `ka * x_t + kb * x0 + kn * noise` as the compiler contracts it there: the x_t product is fused into the rounded
// x0 product, the rounded noise product is added last.  Spelled out (and kept from further contraction) because the same source
// expression contracted the other way round in this kernel, one ulp away from the independent-window chain.
__device__ __forceinline__ float sampler_update(float kx, float xt, float k0, float x0, float kn, float n) {
#pragma clang fp contract(off)
    const float b = k0 * x0, c = kn * n;
    return fmaf(kx, xt, b) + c;
}
struct StepClamp {
    float lo, hi;
    int mode;
    __device__ __forceinline__ float operator()(float y) const { return mode == 0 ? fmaxf(y, lo) : fminf(fmaxf(y, lo), hi); }
};
// The fuse of the joint kernels at voxel p, over the covering kept windows with c the step clamp: covered() says whether there is one,
// x0() = sum(w c(y)) / sum(w) is then the fused prediction.  The quotient is taken where the caller asks for it -- after it has issued
// its own loads, so that the division runs under their latency.
struct Fused {
    float num, den;
    __device__ __forceinline__ bool covered() const { return den != 0.f; }
    __device__ __forceinline__ float x0() const { return num / den; }
};
__device__ __forceinline__ Fused joint_fuse(const float* __restrict__ y, const int* __restrict__ slot, const float* __restrict__ taps,
                                            const float* tp, int N, int P, int stride, int G0, int G1, int G2, const Voxel& p,
                                            StepClamp c) {
    Fused f;
    window_walk(y, slot, taps, tp, N, P, stride, G1, G2, p.d, p.h, p.x, covering(p.d, p.h, p.x, P, stride, G0, G1, G2), c, f.num, f.den);
    return f;
}
// DPM-Solver++ 2M in sigma space (the EDM family; ElucidatedImagen.dpmpp2m_coefficients), ODE (kn == 0) and midpoint SDE (kn != 0):
// x_next = kx x + k0 D_i + kp D_{i-1} + kn n.  The first three terms are sampler_update's, in its order; the rounded kn n product is
// added last, and not at all when kn == 0 (no operand read, no Philox call).  ONE definition for the per-window step and the joint
// step, so at stride = patch the joint chain is the per-window loop bit for bit.
__device__ __forceinline__ float sampler_update_sde(float kx, float x, float k0, float d0, float kp, float dprev, float kn, float n) {
#pragma clang fp contract(off)
    float u = sampler_update(kx, x, k0, d0, kp, dprev);
    if (kn != 0.f) {
        const float c = kn * n;
        u = u + c;
    }
    return u;
}
// The per-window step: x / x0 / x0_prev / noise [B][per], one coefficient row per sample (device [B] each).  x0_prev == NULL and
// noise == NULL stand for zeros and are not read; noise is not read either for a sample whose kn is 0.  There is no clamp: x0 arrives
// clamped or thresholded.  x_next may alias x (every thread reads its own element, then writes it).  Block (64, 4) = 256 consecutive
// elements of sample blockIdx.y.
__global__ __launch_bounds__(256) void multistep_sde_step_kernel(const float* x, const float* __restrict__ x0,
                                                                 const float* __restrict__ x0_prev, const float* __restrict__ noise,
                                                                 const float* __restrict__ kx, const float* __restrict__ k0,
                                                                 const float* __restrict__ kp, const float* __restrict__ kn,
                                                                 float* x_next, size_t per) {
    const int b = blockIdx.y;
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.y * 64 + threadIdx.x;
    if (e >= per) return;
    const size_t v = (size_t)b * per + e;
    const float cn = noise ? kn[b] : 0.f;              // no noise: the term is dropped, as for kn == 0
    const float prev = x0_prev ? x0_prev[v] : 0.f;
    const float n = cn != 0.f ? noise[v] : 0.f;
    x_next[v] = sampler_update_sde(kx[b], x[v], k0[b], x0[v], kp[b], prev, cn, n);
}

// ONE kernel for the three linear updates of the joint state (diqt_volume_joint_step, _multistep and _multistep_sde): the fuse, then
// per covered voxel, with prev = x0_prev[v] (0 for x0_prev == NULL) and n the anchored normal of (seed, draw, sample) at the voxel,
// channel 0 (anchored_noise_kernel's Philox call and philox_normal; n = 0 and no call when kn == 0),
//   third_is_normal (the first-order step)   x_next = sampler_update(kx, xt, k0, x0, kn, n): the kn n product is added also when it is 0;
//   otherwise (the multistep forms)          x_next = sampler_update_sde(kx, xt, k0, x0, kp, prev, kn, n): the history term is
//                                            sampler_update's third operand and kn n a fourth term, added last and only when kn != 0.
// `third_is_normal` is uniform over the launch.  The identities the entries rely on, each exact in IEEE arithmetic:
//   * the 2M chain of the VP family (diqt_volume_joint_multistep) is the second form with kn = 0: nothing follows the history term;
//   * the second form with kp = 0 and no history is NOT the first: it is (u + +0) + kn n, and where u and kn n are both -0 that is +0
//     while the first form's u + kn n is -0 -- hence the flag, not a fold (tests/test_gpu_volume_joint_bits.py plants such voxels);
//   * x_t == NULL is the initial state, x_next = kn n(draw) at EVERY voxel as one rounded product -- sigma0 n as the per-window sampler
//     stores it; diqt_volume_joint_step asks for it with kn = 1, and 1 n is n bit for bit: anchored_noise_kernel's field.
// A voxel no kept window covers keeps x_t (nothing ever gathers it) and gets x0_out = 0.  x0_out == NULL (the first form only; the
// entries of the others require it): the fused x0 is not stored.  x_next may alias x_t and x0_out may alias x0_prev (no __restrict__
// on the four): every thread reads its own voxel of both, then writes it.  At stride = patch the first form is ddpm_step_kernel's
// chain and the second the per-window loop above, bit for bit.
__global__ __launch_bounds__(256) void volume_joint_linear_kernel(const float* __restrict__ y, const int* __restrict__ slot,
                                                                  const float* __restrict__ taps, const float* x_t,
                                                                  const float* x0_prev, float* x_next, float* x0_out, int N, int D,
                                                                  int H, int W, int P, int stride, int G0, int G1, int G2, float kx,
                                                                  float k0, float kp, float kn, float lo, float hi, int clamp_mode,
                                                                  int third_is_normal, unsigned key0, unsigned key1, unsigned draw,
                                                                  unsigned sample) {
    extern __shared__ float tp[];                      // [P]
    const Voxel p = walk_prologue(tp, taps, P, x_t != nullptr, H, W);
    if (!p.inside) return;
    const size_t v = p.v;
    const unsigned v0 = (unsigned)v, v1 = (unsigned)((unsigned long long)v >> 32);
    if (!x_t) {
        x_next[v] = kn * philox_normal(philox4x32_10(v0, v1, draw, sample, key0, key1));
        return;
    }
    const Fused f = joint_fuse(y, slot, taps, tp, N, P, stride, G0, G1, G2, p, StepClamp{lo, hi, clamp_mode});
    const float xt = x_t[v];
    if (!f.covered()) {
        x_next[v] = xt;
        if (x0_out) x0_out[v] = 0.f;
        return;
    }
    const float x0 = f.x0();
    const float prev = x0_prev ? x0_prev[v] : 0.f;
    float n = 0.f;
    if (kn != 0.f) n = philox_normal(philox4x32_10(v0, v1, draw, sample, key0, key1));
    const float r = third_is_normal ? sampler_update(kx, xt, k0, x0, kn, n) : sampler_update_sde(kx, xt, k0, x0, kp, prev, kn, n);
    // both stores after the last use of a load: a store counts in vmcnt on gfx950, so a wait for x_t behind a store waits for the store too
    if (x0_out) x0_out[v] = x0;
    x_next[v] = r;
}

// ---- data consistency (DDNM, Wang et al. 2023) for a block-average measurement -----------------------------------------------------------
// A cell is (fz, fy, fx) voxels, n = fz fy fx in 2 .. 64; the measurement is the cell mean A x, and it arrives replicated on the
// high-res grid (meas_up[v] = the measurement of v's cell).  The projection x0' = x0 + w A+(y - A x0) of the values a over one cell,
// ONE definition for the per-window kernel and the joint kernel (so at stride = patch the joint chain is the per-window loop bit for
// bit), fp32 and kept from contraction:
//   cell_mean    s = 0; s = s + a[v] over the cell's voxels in lexicographic (z, y, x) order; m = s / (float)n.  `a(i, j, k)` is the
//                value at offset (i, j, k) inside the cell;
//   cell_shift   a'[v] = fmaf(w, meas_up[v] - m, a[v]), w the consistency weight in (0, 1].
struct Cell { int fz, fy, fx; };
template <class Value>
__device__ __forceinline__ float cell_mean(Cell c, Value a) {
#pragma clang fp contract(off)
    float s = 0.f;
    for (int i = 0; i < c.fz; ++i)
        for (int j = 0; j < c.fy; ++j)
            for (int k = 0; k < c.fx; ++k) s = s + a(i, j, k);
    return s / (float)(c.fz * c.fy * c.fx);
}
__device__ __forceinline__ float cell_shift(float w, float meas, float m, float a) {
#pragma clang fp contract(off)
    const float r = meas - m;
    return fmaf(w, r, a);
}
// The same projection for a measurement with a slice profile (ops.cell_profile): y = sum u[q] x[q] over the cell, u >= 0 and sum u = 1,
// q the voxel's lexicographic (z, y, x) index inside its cell; the cells stay disjoint, so A A^T = |u|^2 I and A+ = A^T / |u|^2.  The
// table is [2][n]: u, then the gain g[q] = u[q] / sum u^2.  ONE definition again, fp32 and kept from contraction:
//   cell_wmean   s = 0; s = fmaf(u[q], a[q], s) over the cell's voxels in lexicographic order; m = s.  No division;
//   cell_wshift  t = w g[q], one rounded product; a'[v] = fmaf(t, meas_up[v] - m, a[v]).  A gap voxel (g = 0) keeps a[v]: the product
//                is a zero and a[v] + (+-0) is a[v] (only a[v] = -0 under a +0 product comes out as +0, as fmaf has it).
template <class Value>
__device__ __forceinline__ float cell_wmean(Cell c, const float* u, Value a) {
#pragma clang fp contract(off)
    float s = 0.f;
    int q = 0;
    for (int i = 0; i < c.fz; ++i)
        for (int j = 0; j < c.fy; ++j)
            for (int k = 0; k < c.fx; ++k, ++q) s = fmaf(u[q], a(i, j, k), s);
    return s;
}
__device__ __forceinline__ float cell_wshift(float w, float g, float meas, float m, float a) {
#pragma clang fp contract(off)
    const float t = w * g;
    const float r = meas - m;
    return fmaf(t, r, a);
}
// diqt_ddpm_step's clamp with a third mode: 2 = none (the value's own bits).
struct ProjectClamp {
    float lo, hi;
    int mode;
    __device__ __forceinline__ float operator()(float y) const { return mode == 2 ? y : StepClamp{lo, hi, mode}(y); }
};
// The operator A alone: out [D / fz][H / fy][W / fx] = cell_mean of x [D][H][W].  One thread per cell, consecutive lanes = consecutive
// cells along x.
__global__ __launch_bounds__(256) void cell_mean_kernel(const float* __restrict__ x, float* __restrict__ out, size_t cells, int H, int W,
                                                        Cell c) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= cells) return;
    const int cw = W / c.fx, ch = H / c.fy;
    const int cx = (int)(e % cw), cy = (int)((e / cw) % ch);
    const size_t cz = e / ((size_t)cw * ch);
    const float* base = x + ((cz * c.fz) * H + (size_t)cy * c.fy) * W + (size_t)cx * c.fx;
    out[e] = cell_mean(c, [&](int i, int j, int k) { return base[((size_t)i * H + j) * W + k]; });
}
// The per-window step: x0 / meas_up / out are `cubes` cubes of edge P; a = c(x0), then the projection.  One thread per cell: it reads
// its cell's n values twice (the sum, then the shift) and writes only them, so out may alias x0 (no __restrict__ on the two).
__global__ __launch_bounds__(256) void cell_project_kernel(const float* x0, const float* __restrict__ meas_up, float* out, size_t cells,
                                                           int P, Cell c, float w, ProjectClamp clamp) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= cells) return;
    const int cw = P / c.fx, ch = P / c.fy, cd = P / c.fz;
    const int cx = (int)(e % cw), cy = (int)((e / cw) % ch), cz = (int)((e / ((size_t)cw * ch)) % cd);
    const size_t cube = e / ((size_t)cw * ch * cd);
    const size_t base = ((cube * P + (size_t)cz * c.fz) * P + (size_t)cy * c.fy) * P + (size_t)cx * c.fx;
    auto at = [&](int i, int j, int k) { return base + ((size_t)i * P + j) * P + k; };
    const float m = cell_mean(c, [&](int i, int j, int k) { return clamp(x0[at(i, j, k)]); });
    for (int i = 0; i < c.fz; ++i)
        for (int j = 0; j < c.fy; ++j)
            for (int k = 0; k < c.fx; ++k) {
                const size_t v = at(i, j, k);
                out[v] = cell_shift(w, meas_up[v], m, clamp(x0[v]));
            }
}
// cell_mean_kernel with the slice profile: out = cell_wmean of x under table[0 .. n) (diqt_cell_wmean).  Every lane reads the same
// table entry at the same time.
__global__ __launch_bounds__(256) void cell_wmean_kernel(const float* __restrict__ x, const float* __restrict__ table,
                                                         float* __restrict__ out, size_t cells, int H, int W, Cell c) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= cells) return;
    const int cw = W / c.fx, ch = H / c.fy;
    const int cx = (int)(e % cw), cy = (int)((e / cw) % ch);
    const size_t cz = e / ((size_t)cw * ch);
    const float* base = x + ((cz * c.fz) * H + (size_t)cy * c.fy) * W + (size_t)cx * c.fx;
    out[e] = cell_wmean(c, table, [&](int i, int j, int k) { return base[((size_t)i * H + j) * W + k]; });
}
// cell_project_kernel with the slice profile (diqt_cell_project_profile): table [2][n] = u, then g.  The same thread-per-cell walk,
// so out may alias x0 here too.
__global__ __launch_bounds__(256) void cell_project_profile_kernel(const float* x0, const float* __restrict__ meas_up,
                                                                   const float* __restrict__ table, float* out, size_t cells, int P,
                                                                   Cell c, float w, ProjectClamp clamp) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= cells) return;
    const int cw = P / c.fx, ch = P / c.fy, cd = P / c.fz;
    const int cx = (int)(e % cw), cy = (int)((e / cw) % ch), cz = (int)((e / ((size_t)cw * ch)) % cd);
    const size_t cube = e / ((size_t)cw * ch * cd);
    const size_t base = ((cube * P + (size_t)cz * c.fz) * P + (size_t)cy * c.fy) * P + (size_t)cx * c.fx;
    auto at = [&](int i, int j, int k) { return base + ((size_t)i * P + j) * P + k; };
    const float m = cell_wmean(c, table, [&](int i, int j, int k) { return clamp(x0[at(i, j, k)]); });
    const float* g = table + c.fz * c.fy * c.fx;
    int q = 0;
    for (int i = 0; i < c.fz; ++i)
        for (int j = 0; j < c.fy; ++j)
            for (int k = 0; k < c.fx; ++k, ++q) {
                const size_t v = at(i, j, k);
                out[v] = cell_wshift(w, g[q], meas_up[v], m, clamp(x0[v]));
            }
}
// Noise-aware consistency (DDNM+, Wang et al. 2023, 3.3): the measurement carries noise of a known deviation, so a step projects with
// its own weight and takes its fresh normals REDUCED in the range of A: eps' = eps - shrink g (u . eps) per cell.  That is the
// projection above applied to the normals with a zero measurement -- m = cell_mean(eps), eps' = cell_shift(shrink, 0, m, eps), or
// cell_wmean / cell_wshift(shrink, g, 0, m, eps) -- so no new arithmetic is defined here.  The normals are never clamped.
// diqt_cell_project_noise: cell_project_kernel / cell_project_profile_kernel (PROFILE) and, in the same thread-per-cell walk, the
// shaping of `noise`, a tensor of x0's shape.  A thread reads and writes only its own cell of either pair, each value read before it is
// written, so out_x0 may alias x0 and out_noise may alias noise.
template <bool PROFILE>
__global__ __launch_bounds__(256) void cell_project_noise_kernel(const float* x0, const float* __restrict__ meas_up, const float* noise,
                                                                 const float* __restrict__ table, float* out_x0, float* out_noise,
                                                                 size_t cells, int P, Cell c, float w, float shrink,
                                                                 ProjectClamp clamp) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= cells) return;
    const int cw = P / c.fx, ch = P / c.fy, cd = P / c.fz;
    const int cx = (int)(e % cw), cy = (int)((e / cw) % ch), cz = (int)((e / ((size_t)cw * ch)) % cd);
    const size_t cube = e / ((size_t)cw * ch * cd);
    const size_t base = ((cube * P + (size_t)cz * c.fz) * P + (size_t)cy * c.fy) * P + (size_t)cx * c.fx;
    auto at = [&](int i, int j, int k) { return base + ((size_t)i * P + j) * P + k; };
    auto a = [&](int i, int j, int k) { return clamp(x0[at(i, j, k)]); };
    auto z = [&](int i, int j, int k) { return noise[at(i, j, k)]; };
    float m, mz;
    if constexpr (PROFILE) {
        m = cell_wmean(c, table, a);
        mz = cell_wmean(c, table, z);
    } else {
        m = cell_mean(c, a);
        mz = cell_mean(c, z);
    }
    int q = 0;
    for (int i = 0; i < c.fz; ++i)
        for (int j = 0; j < c.fy; ++j)
            for (int k = 0; k < c.fx; ++k, ++q) {
                const size_t v = at(i, j, k);
                if constexpr (PROFILE) {
                    const float g = table[c.fz * c.fy * c.fx + q];
                    out_x0[v] = cell_wshift(w, g, meas_up[v], m, clamp(x0[v]));
                    out_noise[v] = cell_wshift(shrink, g, 0.f, mz, noise[v]);
                } else {
                    out_x0[v] = cell_shift(w, meas_up[v], m, clamp(x0[v]));
                    out_noise[v] = cell_shift(shrink, 0.f, mz, noise[v]);
                }
            }
}
// volume_joint_linear_kernel with the projection between the fuse and the update (diqt_volume_joint_consistent_step): per voxel the
// fuse x0 = num / den exactly as there; a cell whose voxels are ALL covered takes x0' = cell_shift(w, meas_up, cell_mean(x0), x0) and
// each of its voxels the update with x0' in the place of x0; a cell with an uncovered voxel is left alone -- its covered voxels take
// the update with their plain x0, its uncovered ones keep x_t and get x0_out = 0.  The two update forms, the normals, the draw
// numbering and "no Philox call when kn == 0" are the linear kernel's; there is no initial state here and x0_out is required.
// Geometry: a block of (64, 4) threads owns a BOX of whole cells, (fz, cy fy, cx fx) voxels with cx = ceil(64 / fx) and
// cy = ceil(4 / (fz fy)) -- at least 256 voxels where the volume has them, at most 4096 -- on the grid (ceil(W / bx), ceil(H / by),
// D / fz); a thread takes the box's voxels e = t, t + 256, ... (x fastest: lanes read consecutive floats).  Pass 1 fuses every voxel of
// the box into LDS (x0s[e], and den[e] = 0 for an uncovered voxel or one past the volume); after a barrier pass 2 revisits the SAME
// voxels: the thread sums its voxel's cell out of LDS -- every voxel of a cell forms the same sum in the same order -- and updates it.
// A thread reads and writes only its own voxels of x_t / x0_prev / x_next / x0_out, each read before it is written, so x_next may alias
// x_t and x0_out may alias x0_prev; whole cells lie in one block, so there is no atomic and no waiting across blocks.  D, H and W are
// multiples of the cell, so a cell is inside the volume or outside it as a whole.
// PROFILE (diqt_volume_joint_consistent_profile_step): cell_wmean / cell_wshift in the place of cell_mean / cell_shift, the 2n floats
// of `table` copied into LDS behind dens in the prologue; a cell is still corrected only when ALL n of its voxels are covered, whatever
// their weights.  Nothing else differs, and the uniform instantiation never looks at `table`.
struct CellBox { int by, bx; };                        // the box is (fz, by, bx) voxels
__host__ __device__ __forceinline__ CellBox cell_box(Cell c) {
    const int zy = c.fz * c.fy;
    return CellBox{c.fy * ((4 + zy - 1) / zy), c.fx * ((64 + c.fx - 1) / c.fx)};
}
// NOISE (diqt_volume_joint_consistent_noise_step; forms 0 and 2 with kn != 0 only): the step's normals are shaped as in
// cell_project_noise_kernel.  Pass 1 draws a covered voxel's normal -- the Philox call of the update, moved, not a second one -- into a
// third LDS array ns[nb] behind the table; pass 2 reads it back, forms the cell's sum of ns in the order of the sum of x0s and, in a
// cell whose voxels are ALL covered, takes eps' = cell_shift(shrink, 0, m, eps) (PROFILE: cell_wshift with the voxel's gain).  A cell
// with an uncovered voxel keeps its plain x0 and its plain normals.  `shrink` is the LAST argument and the other instantiations never
// look at it, nor at ns: they are what they were.
template <bool PROFILE, bool NOISE>
__global__ __launch_bounds__(256) void volume_joint_consistent_kernel(const float* __restrict__ y, const int* __restrict__ slot,
                                                                      const float* __restrict__ taps, const float* x_t,
                                                                      const float* x0_prev, const float* __restrict__ meas_up,
                                                                      const float* __restrict__ table, float* x_next, float* x0_out,
                                                                      int N, int D, int H, int W, int P,
                                                                      int stride, int G0, int G1, int G2, Cell c, float w, float kx,
                                                                      float k0, float kp, float kn, float lo, float hi, int clamp_mode,
                                                                      int third_is_normal, unsigned key0, unsigned key1, unsigned draw,
                                                                      unsigned sample, float shrink) {
    extern __shared__ float tp[];                      // [P], then x0s [nb] and den [nb]; PROFILE: the table [2][n]; NOISE: ns [nb]
    const CellBox b = cell_box(c);
    const int nb = c.fz * b.by * b.bx, t = threadIdx.y * 64 + threadIdx.x;
    float* x0s = tp + P;
    float* dens = x0s + nb;
    float* tab = dens + nb;
    const int n = c.fz * c.fy * c.fx;
    float* ns = tab + (PROFILE ? 2 * n : 0);
    for (int e = t; e < P; e += 256) tp[e] = taps[e];
    if constexpr (PROFILE)
        for (int e = t; e < 2 * n; e += 256) tab[e] = table[e];
    __syncthreads();
    const int z0 = blockIdx.z * c.fz, y0 = blockIdx.y * b.by, xb = blockIdx.x * b.bx;
    for (int e = t; e < nb; e += 256) {
        const int lx = e % b.bx, ly = (e / b.bx) % b.by, lz = e / (b.bx * b.by);
        const Voxel p{xb + lx, y0 + ly, z0 + lz, 0, y0 + ly < H && xb + lx < W};
        Fused f{0.f, 0.f};
        if (p.inside) f = joint_fuse(y, slot, taps, tp, N, P, stride, G0, G1, G2, p, StepClamp{lo, hi, clamp_mode});
        x0s[e] = f.covered() ? f.x0() : 0.f;
        dens[e] = f.den;
        if constexpr (NOISE) {                         // covered implies inside: v is a voxel of the volume
            float z = 0.f;
            if (f.covered()) {
                const size_t v = ((size_t)p.d * H + p.h) * W + p.x;
                z = philox_normal(philox4x32_10((unsigned)v, (unsigned)((unsigned long long)v >> 32), draw, sample, key0, key1));
            }
            ns[e] = z;
        }
    }
    __syncthreads();
    for (int e = t; e < nb; e += 256) {
        const int lx = e % b.bx, ly = (e / b.bx) % b.by, lz = e / (b.bx * b.by);
        const int x = xb + lx, h = y0 + ly, d = z0 + lz;
        if (h >= H || x >= W) continue;
        const size_t v = ((size_t)d * H + h) * W + x;
        const float xt = x_t[v];
        if (dens[e] == 0.f) {
            x_next[v] = xt;
            x0_out[v] = 0.f;
            continue;
        }
        // the cell of this voxel inside the box: lz is its z offset (the box is one cell deep)
        const int cb = ((ly / c.fy) * c.fy) * b.bx + (lx / c.fx) * c.fx;
        bool all = true;
        auto value = [&](int i, int j, int k) {
            const int q = cb + (i * b.by + j) * b.bx + k;
            all = all && dens[q] != 0.f;
            return x0s[q];
        };
        auto normal = [&](int i, int j, int k) { return ns[cb + (i * b.by + j) * b.bx + k]; };
        float x0 = x0s[e];
        float eps = 0.f;
        if constexpr (NOISE) eps = ns[e];
        if constexpr (PROFILE) {
            const float m = cell_wmean(c, tab, value);
            // this voxel's index inside its cell
            const float g = tab[n + (lz * c.fy + ly % c.fy) * c.fx + lx % c.fx];
            if (all) x0 = cell_wshift(w, g, meas_up[v], m, x0);
            if constexpr (NOISE) {
                const float mz = cell_wmean(c, tab, normal);
                if (all) eps = cell_wshift(shrink, g, 0.f, mz, eps);
            }
        } else {
            const float m = cell_mean(c, value);
            if (all) x0 = cell_shift(w, meas_up[v], m, x0);
            if constexpr (NOISE) {
                const float mz = cell_mean(c, normal);
                if (all) eps = cell_shift(shrink, 0.f, mz, eps);
            }
        }
        const float prev = x0_prev ? x0_prev[v] : 0.f;
        if constexpr (!NOISE)
            if (kn != 0.f) eps = philox_normal(philox4x32_10((unsigned)v, (unsigned)((unsigned long long)v >> 32), draw, sample, key0, key1));
        const float r = third_is_normal ? sampler_update(kx, xt, k0, x0, kn, eps) : sampler_update_sde(kx, xt, k0, x0, kp, prev, kn, eps);
        x0_out[v] = x0;
        x_next[v] = r;
    }
}

// ---- data consistency for a tile-local linear operator (ops.tile_operator) ------------------------------------------------------------
// The volume splits into disjoint tiles of (fz, fy, fx) voxels and every tile is measured by the same m x n matrix A, m >= 1 rows of any
// rank -- orthogonal thick-slice stacks, a block-DCT low-pass, a partial-volume model.  The projection x0' = x0 + w A+(y - A x0) is
//     x0' = x0 + w (t - P x0),    t = A+ y on the high-res grid (where meas_up stood),    P = A+ A,
// P the n x n orthogonal projector onto the row space of A: symmetric to the bit (the host makes it so), at most 64 x 64 floats whatever
// m is.  ONE definition for the per-window kernel and the joint kernel, fp32 and kept from contraction; for a voxel with in-tile index
// q = (i fy + j) fx + k:
//   tile_apply   s = 0; s = fmaf(p[r stride], a[r], s) over the tile's voxels r in lexicographic (z, y, x) order;
//   then         a'[v] = cell_shift(w, t[v], s, a[v]) = fmaf(w, t[v] - s, a[v]).
// The projection reads p = P + q with stride n, that is P[r][q] and not P[q][r] (equal by symmetry): lanes that walk x inside a tile read
// consecutive LDS words, lanes of different tiles with equal q read ONE word (a broadcast), and the 64-word window [r n, r n + n) of a
// step meets a bank twice only when a 32-lane group holds both q and q + 32.  P[q][r] would put n words between neighbouring lanes.
// The operator itself (tile_measure_kernel) reads p = A + row n with stride 1.
template <class Value>
__device__ __forceinline__ float tile_apply(Cell c, const float* p, int stride, Value a) {
#pragma clang fp contract(off)
    float s = 0.f;
    int r = 0;
    for (int i = 0; i < c.fz; ++i)
        for (int j = 0; j < c.fy; ++j)
            for (int k = 0; k < c.fx; ++k, ++r) s = fmaf(p[r * stride], a(i, j, k), s);
    return s;
}
// A itself: out [m][D / fz][H / fy][W / fx], out[row][tile] = tile_apply of row `row` of A [m][n] on the tile of x [D][H][W].  One
// thread per output value, the tile index fastest.  Once per volume (to simulate an acquisition), not a step of a chain.
__global__ __launch_bounds__(256) void tile_measure_kernel(const float* __restrict__ x, const float* __restrict__ A,
                                                           float* __restrict__ out, size_t tiles, int m, int H, int W, Cell c) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= tiles * m) return;
    const size_t row = e / tiles, tile = e % tiles;
    const int cw = W / c.fx, ch = H / c.fy;
    const int cx = (int)(tile % cw), cy = (int)((tile / cw) % ch);
    const size_t cz = tile / ((size_t)cw * ch);
    const float* base = x + ((cz * c.fz) * H + (size_t)cy * c.fy) * W + (size_t)cx * c.fx;
    out[e] = tile_apply(c, A + row * (c.fz * c.fy * c.fx), 1, [&](int i, int j, int k) { return base[((size_t)i * H + j) * W + k]; });
}
// The back-projection t = A+ y: out [D][H][W], out[v] = sum over the rows of Ap[q][row] y[row][tile of v], Ap = A+ [n][m], the sum
// fused-multiply-added in row order.  One thread per voxel.  Once per volume too.
__global__ __launch_bounds__(256) void tile_backproject_kernel(const float* __restrict__ y, const float* __restrict__ Ap,
                                                               float* __restrict__ out, size_t total, size_t tiles, int m, int H, int W,
                                                               Cell c) {
#pragma clang fp contract(off)
    const size_t v = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= total) return;
    const int x = (int)(v % W), h = (int)((v / W) % H);
    const size_t d = v / ((size_t)W * H);
    const int q = ((int)(d % c.fz) * c.fy + h % c.fy) * c.fx + x % c.fx;
    const size_t tile = ((d / c.fz) * (H / c.fy) + h / c.fy) * (W / c.fx) + x / c.fx;
    float s = 0.f;
    for (int row = 0; row < m; ++row) s = fmaf(Ap[(size_t)q * m + row], y[row * tiles + tile], s);
    out[v] = s;
}
// The per-window step (diqt_tile_project): x0 / target / out are a [D][H][W] stack of cubes (D = cubes P, H = W = P; tiles never cross
// a cube since fz divides P); a = clamp(x0), then the projection.  One thread per cell would run n^2 serial FMAs; here a block of 256
// threads owns a BOX of whole tiles, `b` = cell_box clipped to the cube's edge, stages a into LDS (as [nb], then P [n][n]) and gives
// every voxel of the box a thread, as the joint kernel does.  A block reads its own voxels of x0 before the barrier and writes only
// them after it, so out may alias x0.  The grid is flat: box (bx, by, bz) = blockIdx.x split by gx and gy.
__global__ __launch_bounds__(256) void tile_project_kernel(const float* x0, const float* __restrict__ target,
                                                           const float* __restrict__ table, float* out, int H, int W, int gx, int gy,
                                                           Cell c, CellBox b, float w, ProjectClamp clamp) {
    extern __shared__ float as[];
    const int n = c.fz * c.fy * c.fx, nb = c.fz * b.by * b.bx, t = threadIdx.x;
    float* tab = as + nb;
    for (int e = t; e < n * n; e += 256) tab[e] = table[e];
    const int y0 = (int)((blockIdx.x / gx) % gy) * b.by, xb = (int)(blockIdx.x % gx) * b.bx;
    const size_t z0 = (size_t)(blockIdx.x / ((unsigned)gx * gy)) * c.fz;
    auto voxel = [&](int lx, int ly, int lz) { return ((z0 + lz) * H + (y0 + ly)) * W + (xb + lx); };
    for (int e = t; e < nb; e += 256) {
        const int lx = e % b.bx, ly = (e / b.bx) % b.by, lz = e / (b.bx * b.by);
        as[e] = y0 + ly < H && xb + lx < W ? clamp(x0[voxel(lx, ly, lz)]) : 0.f;
    }
    __syncthreads();
    for (int e = t; e < nb; e += 256) {
        const int lx = e % b.bx, ly = (e / b.bx) % b.by, lz = e / (b.bx * b.by);
        if (y0 + ly >= H || xb + lx >= W) continue;    // H and W are multiples of the tile: a tile is inside or outside as a whole
        const size_t v = voxel(lx, ly, lz);
        const int cb = ((ly / c.fy) * c.fy) * b.bx + (lx / c.fx) * c.fx;
        const int q = (lz * c.fy + ly % c.fy) * c.fx + lx % c.fx;
        const float s = tile_apply(c, tab + q, n, [&](int i, int j, int k) { return as[cb + (i * b.by + j) * b.bx + k]; });
        out[v] = cell_shift(w, target[v], s, as[e]);
    }
}
// volume_joint_consistent_kernel for a tile operator (diqt_volume_joint_consistent_tile_step): the same box, pass 1 as there (no
// NOISE), the n x n floats of `table` = P copied into LDS behind dens in the prologue; pass 2 forms tile_apply over the voxel's tile
// out of x0s in the place of cell_mean and shifts by meas_up = t.  The forms, the normals, the covered rule (ALL n voxels), the
// uncovered voxels and the aliasing are that kernel's.  `shrink` is not looked at (one launch helper serves both kernels).
__global__ __launch_bounds__(256) void volume_joint_consistent_tile_kernel(const float* __restrict__ y, const int* __restrict__ slot,
                                                                           const float* __restrict__ taps, const float* x_t,
                                                                           const float* x0_prev, const float* __restrict__ meas_up,
                                                                           const float* __restrict__ table, float* x_next, float* x0_out,
                                                                           int N, int D, int H, int W, int P, int stride, int G0, int G1,
                                                                           int G2, Cell c, float w, float kx, float k0, float kp, float kn,
                                                                           float lo, float hi, int clamp_mode, int third_is_normal,
                                                                           unsigned key0, unsigned key1, unsigned draw, unsigned sample,
                                                                           float shrink) {
    extern __shared__ float tp[];                      // [P], then x0s [nb] and den [nb], then the table [n][n]
    const CellBox b = cell_box(c);
    const int nb = c.fz * b.by * b.bx, t = threadIdx.y * 64 + threadIdx.x;
    float* x0s = tp + P;
    float* dens = x0s + nb;
    float* tab = dens + nb;
    const int n = c.fz * c.fy * c.fx;
    for (int e = t; e < P; e += 256) tp[e] = taps[e];
    for (int e = t; e < n * n; e += 256) tab[e] = table[e];
    __syncthreads();
    const int z0 = blockIdx.z * c.fz, y0 = blockIdx.y * b.by, xb = blockIdx.x * b.bx;
    for (int e = t; e < nb; e += 256) {
        const int lx = e % b.bx, ly = (e / b.bx) % b.by, lz = e / (b.bx * b.by);
        const Voxel p{xb + lx, y0 + ly, z0 + lz, 0, y0 + ly < H && xb + lx < W};
        Fused f{0.f, 0.f};
        if (p.inside) f = joint_fuse(y, slot, taps, tp, N, P, stride, G0, G1, G2, p, StepClamp{lo, hi, clamp_mode});
        x0s[e] = f.covered() ? f.x0() : 0.f;
        dens[e] = f.den;
    }
    __syncthreads();
    for (int e = t; e < nb; e += 256) {
        const int lx = e % b.bx, ly = (e / b.bx) % b.by, lz = e / (b.bx * b.by);
        const int x = xb + lx, h = y0 + ly, d = z0 + lz;
        if (h >= H || x >= W) continue;
        const size_t v = ((size_t)d * H + h) * W + x;
        const float xt = x_t[v];
        if (dens[e] == 0.f) {
            x_next[v] = xt;
            x0_out[v] = 0.f;
            continue;
        }
        const int cb = ((ly / c.fy) * c.fy) * b.bx + (lx / c.fx) * c.fx;
        const int q = (lz * c.fy + ly % c.fy) * c.fx + lx % c.fx;      // this voxel's index inside its tile
        bool all = true;
        const float s = tile_apply(c, tab + q, n, [&](int i, int j, int k) {
            const int u = cb + (i * b.by + j) * b.bx + k;
            all = all && dens[u] != 0.f;
            return x0s[u];
        });
        float x0 = x0s[e];
        if (all) x0 = cell_shift(w, meas_up[v], s, x0);
        const float prev = x0_prev ? x0_prev[v] : 0.f;
        float eps = 0.f;
        if (kn != 0.f) eps = philox_normal(philox4x32_10((unsigned)v, (unsigned)((unsigned long long)v >> 32), draw, sample, key0, key1));
        const float r = third_is_normal ? sampler_update(kx, xt, k0, x0, kn, eps) : sampler_update_sde(kx, xt, k0, x0, kp, prev, kn, eps);
        x0_out[v] = x0;
        x_next[v] = r;
    }
}
// ---- noise-aware consistency for a tile operator (DDNM+ per singular direction, ops.tile_noise_operator) --------------------------------
// Every row of A carries noise of its own deviation, so a step weighs every right singular direction v_j of the whitened operator on
// its own: `tables` is [2][n][n] = M, G of this step, M = V diag(lambda) V^T and G = V diag(shrink) V^T, both symmetric to the bit
// (ops.tile_noise_tables makes them on the host).  ONE definition for the two kernels below, fp32 and kept from contraction; for the
// voxel with in-tile index q, a = the tile's (clamped or fused) predictions, t = the back-projected measurement, eps = the normals:
//     d[r] = t[r] - a[r];   s = tile_apply(c, M + q, n, d);   a'[q] = a[q] + s;   g = tile_apply(c, G + q, n, eps);   eps'[q] = eps[q] - g.
// d is formed once per voxel and staged in LDS, so the two sums read LDS only: the tables as [r][q] (the pattern of tile_apply above),
// d and eps at one address per tile (a broadcast inside a tile).  The normals are never clamped.
// The per-window step (diqt_tile_project_noise): tile_project_kernel's box walk; LDS holds a [nb], d [nb], eps [nb], then M and G.
// A block reads only its own voxels of x0, target and noise, all before the barrier, and writes only them after it: out may alias x0
// and out_noise may alias noise.
__global__ __launch_bounds__(256) void tile_project_noise_kernel(const float* x0, const float* __restrict__ target, const float* noise,
                                                                 const float* __restrict__ tables, float* out, float* out_noise, int H,
                                                                 int W, int gx, int gy, Cell c, CellBox b, ProjectClamp clamp) {
#pragma clang fp contract(off)
    extern __shared__ float as[];
    const int n = c.fz * c.fy * c.fx, nb = c.fz * b.by * b.bx, t = threadIdx.x;
    float* ds = as + nb;
    float* zs = ds + nb;
    float* tab = zs + nb;
    for (int e = t; e < 2 * n * n; e += 256) tab[e] = tables[e];
    const int y0 = (int)((blockIdx.x / gx) % gy) * b.by, xb = (int)(blockIdx.x % gx) * b.bx;
    const size_t z0 = (size_t)(blockIdx.x / ((unsigned)gx * gy)) * c.fz;
    auto voxel = [&](int lx, int ly, int lz) { return ((z0 + lz) * H + (y0 + ly)) * W + (xb + lx); };
    for (int e = t; e < nb; e += 256) {
        const int lx = e % b.bx, ly = (e / b.bx) % b.by, lz = e / (b.bx * b.by);
        float a = 0.f, d = 0.f, z = 0.f;
        if (y0 + ly < H && xb + lx < W) {
            const size_t v = voxel(lx, ly, lz);
            a = clamp(x0[v]);
            d = target[v] - a;
            z = noise[v];
        }
        as[e] = a;
        ds[e] = d;
        zs[e] = z;
    }
    __syncthreads();
    for (int e = t; e < nb; e += 256) {
        const int lx = e % b.bx, ly = (e / b.bx) % b.by, lz = e / (b.bx * b.by);
        if (y0 + ly >= H || xb + lx >= W) continue;    // H and W are multiples of the tile: a tile is inside or outside as a whole
        const size_t v = voxel(lx, ly, lz);
        const int cb = ((ly / c.fy) * c.fy) * b.bx + (lx / c.fx) * c.fx;
        const int q = (lz * c.fy + ly % c.fy) * c.fx + lx % c.fx;
        const float s = tile_apply(c, tab + q, n, [&](int i, int j, int k) { return ds[cb + (i * b.by + j) * b.bx + k]; });
        const float g = tile_apply(c, tab + n * n + q, n, [&](int i, int j, int k) { return zs[cb + (i * b.by + j) * b.bx + k]; });
        out[v] = as[e] + s;
        out_noise[v] = zs[e] - g;
    }
}
// volume_joint_consistent_tile_kernel with that arithmetic (diqt_volume_joint_consistent_tile_noise_step; forms 0 and 2 with kn != 0
// only).  Pass 1 fuses each voxel as there and, for a covered one, reads t = meas_up[v] and draws the normal -- the Philox call of the
// update, moved, not a second one (the NOISE instantiations of volume_joint_consistent_kernel do the same) -- leaving x0, d, den and
// eps in LDS; the tables [2][n][n] ride behind them.  Pass 2 runs the two tile_apply sums; a tile whose voxels are ALL covered takes
// x0' and eps', a tile with an uncovered voxel keeps its plain x0 and its plain normals.  The forms, the uncovered voxels and the
// aliasing are that kernel's.  `w` and `shrink` are not looked at (one launch helper serves all these kernels).
__global__ __launch_bounds__(256) void volume_joint_consistent_tile_noise_kernel(
    const float* __restrict__ y, const int* __restrict__ slot, const float* __restrict__ taps, const float* x_t, const float* x0_prev,
    const float* __restrict__ meas_up, const float* __restrict__ tables, float* x_next, float* x0_out, int N, int D, int H, int W, int P,
    int stride, int G0, int G1, int G2, Cell c, float w, float kx, float k0, float kp, float kn, float lo, float hi, int clamp_mode,
    int third_is_normal, unsigned key0, unsigned key1, unsigned draw, unsigned sample, float shrink) {
#pragma clang fp contract(off)
    extern __shared__ float tp[];                      // [P], then x0s, ds, dens and ns [nb] each, then the tables [2][n][n]
    const CellBox b = cell_box(c);
    const int nb = c.fz * b.by * b.bx, t = threadIdx.y * 64 + threadIdx.x;
    float* x0s = tp + P;
    float* ds = x0s + nb;
    float* dens = ds + nb;
    float* ns = dens + nb;
    float* tab = ns + nb;
    const int n = c.fz * c.fy * c.fx;
    for (int e = t; e < P; e += 256) tp[e] = taps[e];
    for (int e = t; e < 2 * n * n; e += 256) tab[e] = tables[e];
    __syncthreads();
    const int z0 = blockIdx.z * c.fz, y0 = blockIdx.y * b.by, xb = blockIdx.x * b.bx;
    for (int e = t; e < nb; e += 256) {
        const int lx = e % b.bx, ly = (e / b.bx) % b.by, lz = e / (b.bx * b.by);
        const Voxel p{xb + lx, y0 + ly, z0 + lz, 0, y0 + ly < H && xb + lx < W};
        Fused f{0.f, 0.f};
        if (p.inside) f = joint_fuse(y, slot, taps, tp, N, P, stride, G0, G1, G2, p, StepClamp{lo, hi, clamp_mode});
        float x0 = 0.f, d = 0.f, z = 0.f;
        if (f.covered()) {                             // covered implies inside: v is a voxel of the volume
            const size_t v = ((size_t)p.d * H + p.h) * W + p.x;
            x0 = f.x0();
            d = meas_up[v] - x0;
            z = philox_normal(philox4x32_10((unsigned)v, (unsigned)((unsigned long long)v >> 32), draw, sample, key0, key1));
        }
        x0s[e] = x0;
        ds[e] = d;
        dens[e] = f.den;
        ns[e] = z;
    }
    __syncthreads();
    for (int e = t; e < nb; e += 256) {
        const int lx = e % b.bx, ly = (e / b.bx) % b.by, lz = e / (b.bx * b.by);
        const int x = xb + lx, h = y0 + ly, d = z0 + lz;
        if (h >= H || x >= W) continue;
        const size_t v = ((size_t)d * H + h) * W + x;
        const float xt = x_t[v];
        if (dens[e] == 0.f) {
            x_next[v] = xt;
            x0_out[v] = 0.f;
            continue;
        }
        const int cb = ((ly / c.fy) * c.fy) * b.bx + (lx / c.fx) * c.fx;
        const int q = (lz * c.fy + ly % c.fy) * c.fx + lx % c.fx;      // this voxel's index inside its tile
        bool all = true;
        const float s = tile_apply(c, tab + q, n, [&](int i, int j, int k) {
            const int u = cb + (i * b.by + j) * b.bx + k;
            all = all && dens[u] != 0.f;
            return ds[u];
        });
        const float g = tile_apply(c, tab + n * n + q, n, [&](int i, int j, int k) { return ns[cb + (i * b.by + j) * b.bx + k]; });
        float x0 = x0s[e], eps = ns[e];
        if (all) {
            x0 = x0 + s;
            eps = eps - g;
        }
        const float prev = x0_prev ? x0_prev[v] : 0.f;
        const float r = third_is_normal ? sampler_update(kx, xt, k0, x0, kn, eps) : sampler_update_sde(kx, xt, k0, x0, kp, prev, kn, eps);
        x0_out[v] = x0;
        x_next[v] = r;
    }
}

// ---- data consistency for OVERLAPPING slice profiles (the slab operator, ops.slab_profile) --------------------------------------------
// Slice s of column (cy, cx) measures y_s = sum_i u_z[i] (u_yx . x[s fz - r + i, cell]), i = 0 .. L - 1, L = fz + 2r, 1 <= r, 2r <= fz: a
// slice overlaps its two neighbours only, a voxel lies under at most two slices, and along z A A^T = q G with G Toeplitz tridiagonal
// (d = sum u_z^2, e = sum_{i < 2r} u_z[i] u_z[i + fz]) on every maximal run of consecutive ACTIVE rows -- rows whose whole support lies
// inside the domain and is covered.  The table is flat fp32: u_z [L], u_yx [fy fx], g_yx = u_yx / q [fy fx], e, then for run position
// j = 0 .. jmax - 1 the multipliers m_j = e / pi_{j-1} (m_0 = 0) and the inverse pivots ip_j = 1 / pi_j of the LDL^T sweep, made on the
// host: no kernel divides.  ONE definition for the per-window kernel and the joint kernels, fp32 and kept from contraction:
//   slab_plane     pm = 0; pm = fmaf(u_yx[q], a[q], pm) over the cell's fy fx voxels of one plane in (y, x) order;
//   the row        acc = 0; acc = fmaf(u_z[i], pm[s fz - r + i], acc) over ascending i; rho_s = y_s - acc;
//   slab_forward   zeta = rho at j = 0, else fmaf(-m_j, zeta_{s-1}, rho_s), over ascending s; a run restarts at j = 0;
//   slab_backward  c_s = fmaf(-e, c_{s+1}, zeta_s) * ip_j over descending s, c_{s+1} = 0 at the end of a run;
//   slab_shift     at depth z = k fz + o: t = 0; t = fmaf(u_z[.], c_s, t) over the active ones of s = k - 1 (o < r), k, k + 1
//                  (o >= fz - r) inside [0, S), ascending; a' = fmaf(w * g_yx[q], t, a), w * g_yx one rounded product.  A voxel under no
//                  active row keeps a's bits.
struct Slab { int fz, fy, fx, r, jmax; };
struct SlabTable { const float *uz, *uyx, *gyx, *m, *ip; };
__device__ __forceinline__ SlabTable slab_table(Slab s, const float* t) {
    const int L = s.fz + 2 * s.r, n = s.fy * s.fx;
    return SlabTable{t, t + L, t + L + n, t + L + 2 * n + 1, t + L + 2 * n + 1 + s.jmax};
}
__device__ __forceinline__ float slab_e(Slab s, const float* t) { return t[s.fz + 2 * s.r + 2 * s.fy * s.fx]; }
template <class Value>
__device__ __forceinline__ float slab_plane(Slab s, const float* uyx, Value a) {
#pragma clang fp contract(off)
    float pm = 0.f;
    int q = 0;
    for (int j = 0; j < s.fy; ++j)
        for (int k = 0; k < s.fx; ++k, ++q) pm = fmaf(uyx[q], a(j, k), pm);
    return pm;
}
__device__ __forceinline__ float slab_forward(float m, float zprev, float rho, int j) {
#pragma clang fp contract(off)
    return j == 0 ? rho : fmaf(-m, zprev, rho);
}
__device__ __forceinline__ float slab_backward(float e, float cnext, float zeta, float ip) {
#pragma clang fp contract(off)
    const float t = fmaf(-e, cnext, zeta);
    return t * ip;
}
// coef(s) is c_s and active(s) whether row s is active; both are asked only for 0 <= s < S.
template <class Coef, class Active>
__device__ __forceinline__ float slab_shift(Slab s, const float* uz, int S, int z, float w, float g, float a, Coef coef, Active active) {
#pragma clang fp contract(off)
    const int k = z / s.fz, o = z - k * s.fz;
    float t = 0.f;
    bool any = false;
    if (o < s.r && k >= 1 && active(k - 1)) {
        t = fmaf(uz[o + s.fz + s.r], coef(k - 1), t);
        any = true;
    }
    if (active(k)) {
        t = fmaf(uz[o + s.r], coef(k), t);
        any = true;
    }
    if (o >= s.fz - s.r && k + 1 < S && active(k + 1)) {
        t = fmaf(uz[o - s.fz + s.r], coef(k + 1), t);
        any = true;
    }
    if (!any) return a;
    const float wg = w * g;
    return fmaf(wg, t, a);
}
// The operator itself (diqt_slab_measure): out [D / fz][H / fy][W / fx]; a row that leaves the volume takes the truncated sum (the
// planes outside are skipped: they would add +0).  One thread per output, consecutive lanes = consecutive cells along x.
__global__ __launch_bounds__(256) void slab_measure_kernel(const float* __restrict__ x, const float* __restrict__ table,
                                                           float* __restrict__ out, size_t rows, int D, int H, int W, Slab sl) {
#pragma clang fp contract(off)
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= rows) return;
    const SlabTable tb = slab_table(sl, table);
    const int cw = W / sl.fx, ch = H / sl.fy;
    const int cx = (int)(e % cw), cy = (int)((e / cw) % ch), s = (int)(e / ((size_t)cw * ch));
    const int L = sl.fz + 2 * sl.r;
    float acc = 0.f;
    for (int i = 0; i < L; ++i) {
        const int z = s * sl.fz - sl.r + i;
        if (z < 0 || z >= D) continue;
        const float* base = x + ((size_t)z * H + (size_t)cy * sl.fy) * W + (size_t)cx * sl.fx;
        const float pm = slab_plane(sl, tb.uyx, [&](int j, int k) { return base[(size_t)j * W + k]; });
        acc = fmaf(tb.uz[i], pm, acc);
    }
    out[e] = acc;
}
// The per-window step (diqt_slab_project): `cubes` cubes of edge P, S = P / fz slices each; the domain is the cube, so rows 1 .. S - 2
// are active and form ONE run (j = s - 1); rows 0 and S - 1 leave the cube and are never enforced.  One thread owns one column
// (cube, cy, cx), consecutive lanes = consecutive cx.  It walks z once, adding every plane value to the (at most two) rows above it --
// ascending z is ascending i for each of them -- then sweeps forward and backward over its S floats of LDS (col[s * 256], one bank per
// lane), and walks z once more to write.  a = clamp(x0); every read of the column precedes its first write, so out may alias x0.
__global__ __launch_bounds__(256) void slab_project_kernel(const float* x0, const float* __restrict__ meas_up,
                                                           const float* __restrict__ table, float* out, size_t cols, int P, Slab sl,
                                                           float w, ProjectClamp clamp) {
#pragma clang fp contract(off)
    extern __shared__ float slab_lds[];                 // [S][256]
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= cols) return;
    const SlabTable tb = slab_table(sl, table);
    const float ee = slab_e(sl, table);
    const int S = P / sl.fz, cw = P / sl.fx, ch = P / sl.fy;
    const int cx = (int)(e % cw), cy = (int)((e / cw) % ch);
    const size_t cube = e / ((size_t)cw * ch);
    const size_t base = ((cube * P) * P + (size_t)cy * sl.fy) * P + (size_t)cx * sl.fx;
    auto at = [&](int z, int j, int k) { return base + ((size_t)z * P + j) * P + k; };
    float* col = slab_lds + threadIdx.x;
    for (int s = 0; s < S; ++s) col[s * 256] = 0.f;
    for (int z = 0; z < P; ++z) {
        const float pm = slab_plane(sl, tb.uyx, [&](int j, int k) { return clamp(x0[at(z, j, k)]); });
        const int k = z / sl.fz, o = z - k * sl.fz;
        if (o < sl.r && k >= 1) col[(k - 1) * 256] = fmaf(tb.uz[o + sl.fz + sl.r], pm, col[(k - 1) * 256]);
        col[k * 256] = fmaf(tb.uz[o + sl.r], pm, col[k * 256]);
        if (o >= sl.fz - sl.r && k + 1 < S) col[(k + 1) * 256] = fmaf(tb.uz[o - sl.fz + sl.r], pm, col[(k + 1) * 256]);
    }
    float run = 0.f;
    for (int s = 1; s <= S - 2; ++s) {
        const float rho = meas_up[at(s * sl.fz, 0, 0)] - col[s * 256];
        run = slab_forward(tb.m[s - 1], run, rho, s - 1);
        col[s * 256] = run;
    }
    run = 0.f;
    for (int s = S - 2; s >= 1; --s) {
        run = slab_backward(ee, run, col[s * 256], tb.ip[s - 1]);
        col[s * 256] = run;
    }
    auto coef = [&](int s) { return col[s * 256]; };
    auto active = [&](int s) { return s >= 1 && s <= S - 2; };
    for (int z = 0; z < P; ++z) {
        int q = 0;
        for (int j = 0; j < sl.fy; ++j)
            for (int k = 0; k < sl.fx; ++k, ++q) {
                const size_t v = at(z, j, k);
                out[v] = slab_shift(sl, tb.uz, S, z, w, tb.gyx[q], clamp(x0[v]), coef, active);
            }
    }
}
// The joint path needs a solve along the whole depth of the volume, so it is three launches per step where a box of cells takes one.
// FIRST (diqt_volume_joint_slab_coeffs): per (z, cy, cx) the fy fx voxels of the plane are fused as in the linear kernel (joint_fuse,
// the same StepClamp); pm = slab_plane of the fused x0 and covered = all of them have a window.  An uncovered plane stores pm = 0.
// A block owns one plane of volume_joint_consistent_kernel's box, (by, bx) voxels of whole in-plane cells: every voxel is fused by a
// thread of its own into LDS (lanes along x, so the windows' rows are read as in the other joint kernels), then one thread per cell
// forms the plane value from LDS.
__global__ __launch_bounds__(256) void volume_joint_slab_planes_kernel(const float* __restrict__ y, const int* __restrict__ slot,
                                                                       const float* __restrict__ taps, const float* __restrict__ table,
                                                                       float* __restrict__ pm_out, float* __restrict__ cov_out, int N,
                                                                       int D, int H, int W, int P, int stride, int G0, int G1, int G2,
                                                                       Slab sl, float lo, float hi, int clamp_mode) {
    extern __shared__ float tp[];                      // [P], then x0s [nb] and den [nb]
    const CellBox b = cell_box(Cell{1, sl.fy, sl.fx});
    const int nb = b.by * b.bx, t = threadIdx.y * 64 + threadIdx.x;
    float* x0s = tp + P;
    float* dens = x0s + nb;
    for (int e = t; e < P; e += 256) tp[e] = taps[e];
    __syncthreads();
    const int d = blockIdx.z, y0 = blockIdx.y * b.by, xb = blockIdx.x * b.bx;
    for (int e = t; e < nb; e += 256) {
        const int lx = e % b.bx, ly = e / b.bx;
        const Voxel p{xb + lx, y0 + ly, d, 0, y0 + ly < H && xb + lx < W};
        Fused f{0.f, 0.f};
        if (p.inside) f = joint_fuse(y, slot, taps, tp, N, P, stride, G0, G1, G2, p, StepClamp{lo, hi, clamp_mode});
        x0s[e] = f.covered() ? f.x0() : 0.f;
        dens[e] = f.den;
    }
    __syncthreads();
    const SlabTable tb = slab_table(sl, table);
    const int cw = W / sl.fx, ch = H / sl.fy, cbx = b.bx / sl.fx, cby = b.by / sl.fy;
    for (int e = t; e < cby * cbx; e += 256) {
        const int lx = e % cbx, ly = e / cbx;
        const int cx = xb / sl.fx + lx, cy = y0 / sl.fy + ly;
        if (cx >= cw || cy >= ch) continue;            // H and W are multiples of the cell: a cell is inside the volume as a whole
        bool all = true;
        const float pm = slab_plane(sl, tb.uyx, [&](int j, int k) {
            const int q = (ly * sl.fy + j) * b.bx + lx * sl.fx + k;
            all = all && dens[q] != 0.f;
            return x0s[q];
        });
        const size_t o = ((size_t)d * ch + cy) * cw + cx;
        pm_out[o] = all ? pm : 0.f;
        cov_out[o] = all ? 1.f : 0.f;
    }
}
// SECOND (the same entry): per column (cy, cx) the rows, the residuals and the two sweeps over the whole depth.  Row s is active when
// its support [s fz - r, s fz + fz + r) lies inside [0, D) and every plane of it is covered; a run restarts at j = 0 after an inactive
// row.  Block (64, 4): 64 columns, and the rows of a column are shared out over threadIdx.y for the part that is parallel -- the row
// sums and residuals, rho into `coef` and the activity into `act` -- then, after the barrier, the thread with threadIdx.y == 0 sweeps
// its column: up (zeta into `coef`, the run position j + 1 into `act`, 0 for an inactive row) and down (c into `coef`; inactive rows
// end with c = 0).  The sweeps read eight rows at a time ahead of the recurrence, whose steps do not depend on the loads.  What the
// sweeping thread reads was written by threads of its own block before the barrier; no other block touches the column.
// coef / act [D / fz][H / fy][W / fx]; y_s is read at voxel (s fz, cy fy, cx fx).
__global__ __launch_bounds__(256) void volume_joint_slab_solve_kernel(const float* __restrict__ pm, const float* __restrict__ cov,
                                                                      const float* __restrict__ meas_up, const float* __restrict__ table,
                                                                      float* coef, float* act, size_t cols, int D, int H, int W,
                                                                      Slab sl) {
#pragma clang fp contract(off)
    const size_t e = (size_t)blockIdx.x * 64 + threadIdx.x;
    const bool inside = e < cols;
    const SlabTable tb = slab_table(sl, table);
    const float ee = slab_e(sl, table);
    const int S = D / sl.fz, cw = W / sl.fx, L = sl.fz + 2 * sl.r;
    const int cx = inside ? (int)(e % cw) : 0, cy = inside ? (int)(e / cw) : 0;
    if (inside)
        for (int s = threadIdx.y; s < S; s += 4) {
            const int z0 = s * sl.fz - sl.r;
            bool on = z0 >= 0 && z0 + L <= D;
            float acc = 0.f;
            if (on)
                for (int i = 0; i < L; ++i) {
                    const size_t p = (size_t)(z0 + i) * cols + e;
                    on = on && cov[p] != 0.f;
                    acc = fmaf(tb.uz[i], pm[p], acc);
                }
            const float ys = meas_up[((size_t)(s * sl.fz) * H + (size_t)cy * sl.fy) * W + (size_t)cx * sl.fx];
            coef[(size_t)s * cols + e] = on ? ys - acc : 0.f;
            act[(size_t)s * cols + e] = on ? 1.f : 0.f;
        }
    __syncthreads();
    if (!inside || threadIdx.y != 0) return;
    int j = 0;
    float run = 0.f;
    for (int s0 = 0; s0 < S; s0 += 8) {
        float rho[8], on[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const size_t o = (size_t)min(s0 + u, S - 1) * cols + e;
            rho[u] = coef[o];
            on[u] = act[o];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            if (s0 + u >= S) break;
            const size_t o = (size_t)(s0 + u) * cols + e;
            if (on[u] != 0.f) {
                run = slab_forward(tb.m[j], run, rho[u], j);
                coef[o] = run;
                act[o] = (float)(j + 1);
                ++j;
            } else {
                j = 0;
            }
        }
    }
    run = 0.f;
    for (int s0 = S - 1; s0 >= 0; s0 -= 8) {
        float zeta[8], pos[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const size_t o = (size_t)max(s0 - u, 0) * cols + e;
            zeta[u] = coef[o];
            pos[u] = act[o];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            if (s0 - u < 0) break;
            const int at = (int)pos[u];
            if (at) {
                run = slab_backward(ee, run, zeta[u], tb.ip[at - 1]);
                coef[(size_t)(s0 - u) * cols + e] = run;
            } else {
                run = 0.f;
            }
        }
    }
}
// THIRD (diqt_volume_joint_consistent_slab_step): volume_joint_linear_kernel's three update forms with slab_shift between the fuse and
// the update, c and the activity read from the coefficient volumes of the second launch.  A covered voxel under no active row takes
// the update with its plain x0; an uncovered voxel keeps x_t and gets x0_out = 0; normals and draw numbering are the linear kernel's.
// Every thread reads only its own voxel of x_t / x0_prev, then writes it: x_next may alias x_t and x0_out may alias x0_prev.
__global__ __launch_bounds__(256) void volume_joint_slab_kernel(const float* __restrict__ y, const int* __restrict__ slot,
                                                                const float* __restrict__ taps, const float* x_t, const float* x0_prev,
                                                                const float* __restrict__ table, const float* __restrict__ coef,
                                                                const float* __restrict__ act, float* x_next, float* x0_out, int N, int D,
                                                                int H, int W, int P, int stride, int G0, int G1, int G2, Slab sl, float w,
                                                                float kx, float k0, float kp, float kn, float lo, float hi, int clamp_mode,
                                                                int third_is_normal, unsigned key0, unsigned key1, unsigned draw,
                                                                unsigned sample) {
    extern __shared__ float tp[];                      // [P]
    const Voxel p = walk_prologue(tp, taps, P, true, H, W);
    if (!p.inside) return;
    const size_t v = p.v;
    const unsigned v0 = (unsigned)v, v1 = (unsigned)((unsigned long long)v >> 32);
    const Fused f = joint_fuse(y, slot, taps, tp, N, P, stride, G0, G1, G2, p, StepClamp{lo, hi, clamp_mode});
    const float xt = x_t[v];
    if (!f.covered()) {
        x_next[v] = xt;
        x0_out[v] = 0.f;
        return;
    }
    const SlabTable tb = slab_table(sl, table);
    const int cw = W / sl.fx, ch = H / sl.fy, cy = p.h / sl.fy, cx = p.x / sl.fx;
    const size_t cols = (size_t)cw * ch, col = (size_t)cy * cw + cx;
    const float g = tb.gyx[(p.h - cy * sl.fy) * sl.fx + (p.x - cx * sl.fx)];
    const float x0 = slab_shift(sl, tb.uz, D / sl.fz, p.d, w, g, f.x0(), [&](int s) { return coef[(size_t)s * cols + col]; },
                                [&](int s) { return act[(size_t)s * cols + col] != 0.f; });
    const float prev = x0_prev ? x0_prev[v] : 0.f;
    float n = 0.f;
    if (kn != 0.f) n = philox_normal(philox4x32_10(v0, v1, draw, sample, key0, key1));
    const float r = third_is_normal ? sampler_update(kx, xt, k0, x0, kn, n) : sampler_update_sde(kx, xt, k0, x0, kp, prev, kn, n);
    x0_out[v] = x0;
    x_next[v] = r;
}

// ---- data consistency for a k-space band limit: the band operator (ops.band_table) ------------------------------------------------------
// The measurement keeps a box-shaped, symmetric band of the periodic domain's k-space, so A, A+ and the projector P = A+ A are Kronecker
// products over the three axes, and every factor is a real circulant: on an axis of N voxels with cell factor f and n = N / f,
//   projector        P[i][j]  = d[(i - j) mod N]          N x N
//   measurement      A[s][j]  = a[(s f - j) mod N]        n x N
//   back-projection  A+[j][s] = g[(s f - j) mod N]        N x n
// with d, a, g the fp32 tables of the axis (float64 closed forms rounded once, ops.band_table).  The flat table holds, for z, then y,
// then x, the three tables d, a, g of N floats each.  An axis that is the identity (f = 1, full band) is not `active`: its pass is
// skipped, its bits stay.  ONE arithmetic definition, fp32 and kept from contraction, for every pass:
//   out[i] = acc after  acc = 0;  acc = fmaf(T[idx(i, j)], v[j], acc) over ASCENDING j,
// idx(i, j) = (i si + j sj) mod N with (si, sj) = (1, -1) for d, (f, -1) for a and (-1, f) for g (there j runs over the n rows).
// The passes run z, y, x for P and A and x, y, z for A+ (the small axes first).
//
// band_pass_kernel: one pass along one axis of an array seen as [O][Nin][I] -> [O][Nout][I].  A column is one (o, k); a block of (64, 4)
// owns BAND_C = 64 columns, one per lane, and BAND_I = 4 BAND_R = 32 outputs, wave w the outputs i0 + w BAND_R .. + BAND_R - 1, so the
// table value of an FMA is uniform over a wave (an LDS broadcast) and every thread keeps BAND_R accumulators in registers.  The input
// line goes through LDS in panels of BAND_J = 64 values of j for the 64 columns, rows padded to 65 floats: loaded with the lanes along
// the columns (I > 1: the columns of one o are consecutive floats) or, LINES (I == 1, the x pass), with the lanes along j and stored
// transposed, so both the global read and the LDS accesses are conflict-free; LINES also stores its outputs through the same
// transpose.  The table sits doubled in LDS behind BAND_PAD floats of its own tail and before as many of its head:
// T2[BAND_PAD + k] = T[k mod N] for -BAND_PAD <= k < 2 N + BAND_PAD, so no pass takes a remainder in its loop.  SLIDE (the projector,
// si = 1, sj = -1): j is unrolled by BAND_R and the 2 BAND_R - 1 table values a block of j needs for the thread's BAND_R outputs
// sit in registers -- 15 table reads per 64 FMAs in place of 64; the rows of a panel past Nin hold zeros and the outputs past Nout
// read the padding, which changes no bit of what is stored (acc + T 0 = acc, and acc is never -0).  The other passes clamp the output
// index of the table read and stop at Nin.  Load(e) gives element e of the input array, Store(e, value) takes element e of the output.
constexpr int BAND_C = 64, BAND_R = 8, BAND_I = 4 * BAND_R, BAND_J = 64, BAND_PAD = 64, BAND_MAX_N = 512;
struct BandLoad {
    const float* __restrict__ x;
    __device__ __forceinline__ float operator()(size_t e) const { return x[e]; }
};
struct BandStore {
    float* __restrict__ out;
    __device__ __forceinline__ void operator()(size_t e, float v) const { out[e] = v; }
};
// The loader of a projection's first pass: the residual t - clamp(x0); the storer of its last: out = fmaf(w, c, clamp(x0)), which reads
// x0 at the element it writes and nowhere else (out may alias x0 once the pass itself reads the workspace).
struct BandResidualLoad {
    const float* __restrict__ t;
    const float* x0;
    ProjectClamp clamp;
    __device__ __forceinline__ float operator()(size_t e) const {
#pragma clang fp contract(off)
        return t[e] - clamp(x0[e]);
    }
};
struct BandShiftStore {
    const float* x0;
    float* out;
    float w;
    ProjectClamp clamp;
    __device__ __forceinline__ void operator()(size_t e, float c) const { out[e] = fmaf(w, c, clamp(x0[e])); }
};
template <bool LINES, bool SLIDE, class Load, class Store>
__global__ __launch_bounds__(256) void band_pass_kernel(const float* __restrict__ T, size_t C, int I, int Nin, int Nout, int N, int si,
                                                        int sj, Load load, Store store) {
    extern __shared__ float sh[];                      // T2 [2 N + 2 BAND_PAD], panel [BAND_J][BAND_C + 1]
    float* T2 = sh;
    float* panel = sh + 2 * N + 2 * BAND_PAD;
    constexpr int LD = BAND_C + 1;
    const int l = threadIdx.x, w = threadIdx.y;
    for (int e = w * 64 + l; e < 2 * N + 2 * BAND_PAD; e += 256) T2[e] = T[((e - BAND_PAD) % N + N) % N];
    const size_t c0 = (size_t)blockIdx.x * BAND_C, c = c0 + l;
    const int i0 = blockIdx.y * BAND_I + w * BAND_R;
    const bool cin = c < C;
    const size_t o = LINES ? c : c / (size_t)I, k = LINES ? 0 : c - o * (size_t)I;
    const size_t inbase = o * (size_t)Nin * I + k, outbase = o * (size_t)Nout * I + k;
    float acc[BAND_R];
    int ib[BAND_R];
#pragma unroll
    for (int r = 0; r < BAND_R; ++r) {
        acc[r] = 0.f;
        ib[r] = (SLIDE ? i0 + r : min(i0 + r, Nout - 1)) * si + N + BAND_PAD;
    }
    for (int j0 = 0; j0 < Nin; j0 += BAND_J) {
        __syncthreads();                               // the panel of the chunk before is read; the first: nothing
        if (LINES) {
            const int j = j0 + l;
            for (int cc = w; cc < BAND_C; cc += 4) {
                const size_t cl = c0 + cc;
                panel[l * LD + cc] = cl < C && j < Nin ? load(cl * (size_t)Nin + j) : 0.f;
            }
        } else {
            for (int jj = w; jj < BAND_J; jj += 4) {
                const int j = j0 + jj;
                panel[jj * LD + l] = cin && j < Nin ? load(inbase + (size_t)j * I) : 0.f;
            }
        }
        __syncthreads();                               // also: T2 is written
        const int jn = min(BAND_J, Nin - j0);
        if (SLIDE) {
            for (int jb = 0; jb < jn; jb += BAND_R) {
                float win[2 * BAND_R - 1];             // win[q] = T2[ib[0] - (j0 + jb) + q - (BAND_R - 1)]: offsets r - u of output r, step u
                const float* tw = T2 + ib[0] - (j0 + jb) - (BAND_R - 1);
#pragma unroll
                for (int q = 0; q < 2 * BAND_R - 1; ++q) win[q] = tw[q];
#pragma unroll
                for (int u = 0; u < BAND_R; ++u) {
                    const float v = panel[(jb + u) * LD + l];
#pragma unroll
                    for (int r = 0; r < BAND_R; ++r) acc[r] = fmaf(win[r - u + BAND_R - 1], v, acc[r]);
                }
            }
        } else {
            for (int jj = 0; jj < jn; ++jj) {
                const float v = panel[jj * LD + l];
                const int js = (j0 + jj) * sj;
#pragma unroll
                for (int r = 0; r < BAND_R; ++r) acc[r] = fmaf(T2[ib[r] + js], v, acc[r]);
            }
        }
    }
    if (LINES) {
        __syncthreads();
#pragma unroll
        for (int r = 0; r < BAND_R; ++r) panel[(w * BAND_R + r) * LD + l] = acc[r];
        __syncthreads();
        const int i = blockIdx.y * BAND_I + l;
        if (l < BAND_I && i < Nout)
            for (int cc = w; cc < BAND_C; cc += 4) {
                const size_t cl = c0 + cc;
                if (cl < C) store(cl * (size_t)Nout + i, panel[l * LD + cc]);
            }
    } else if (cin) {
#pragma unroll
        for (int r = 0; r < BAND_R; ++r)
            if (i0 + r < Nout) store(outbase + (size_t)(i0 + r) * I, acc[r]);
    }
}
// A projection with ONE active axis: its only pass reads x0 along whole lines, so it stores c in the workspace and this kernel forms
// out = fmaf(w, c, clamp(x0)) per element -- BandShiftStore's expression -- where out may alias x0.
__global__ __launch_bounds__(256) void band_shift_kernel(const float* x0, const float* __restrict__ c, float* out, size_t total, float w,
                                                         ProjectClamp clamp) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e < total) BandShiftStore{x0, out, w, clamp}(e, c[e]);
}
// FIRST launch of a joint step (diqt_volume_joint_band_residual): the fuse of volume_joint_linear_kernel at every voxel, then three
// volumes: a = the fused clamped prediction (0 where no kept window covers), the covered flag (1 / 0) and r = t - a (0 where
// uncovered: the measurement is believed where nothing was generated).
__global__ __launch_bounds__(256) void volume_joint_band_residual_kernel(const float* __restrict__ y, const int* __restrict__ slot,
                                                                         const float* __restrict__ taps, const float* __restrict__ t,
                                                                         float* __restrict__ a_out, float* __restrict__ cov_out,
                                                                         float* __restrict__ r_out, int N, int D, int H, int W, int P,
                                                                         int stride, int G0, int G1, int G2, float lo, float hi,
                                                                         int clamp_mode) {
#pragma clang fp contract(off)
    extern __shared__ float tp[];                      // [P]
    const Voxel p = walk_prologue(tp, taps, P, true, H, W);
    if (!p.inside) return;
    const Fused f = joint_fuse(y, slot, taps, tp, N, P, stride, G0, G1, G2, p, StepClamp{lo, hi, clamp_mode});
    const float tv = t[p.v];
    const bool cov = f.covered();
    const float a = cov ? f.x0() : 0.f;
    a_out[p.v] = a;
    cov_out[p.v] = cov ? 1.f : 0.f;
    r_out[p.v] = cov ? tv - a : 0.f;
}
// LAST launch of a joint step (diqt_volume_joint_consistent_band_step): volume_joint_linear_kernel's three update forms on
// x0' = fmaf(w, c, a), with a, the covered flag and c = P r read from the workspace -- the windows are not walked again.  An uncovered
// voxel keeps x_t and gets x0_out = 0; normals and draw numbering are the linear kernel's.  Every thread reads only its own voxel of
// x_t / x0_prev, then writes it: x_next may alias x_t and x0_out may alias x0_prev.
__global__ __launch_bounds__(256) void volume_joint_band_kernel(const float* x_t, const float* x0_prev, const float* __restrict__ a,
                                                                const float* __restrict__ cov, const float* __restrict__ c, float* x_next,
                                                                float* x0_out, int H, int W, float w, float kx, float k0, float kp,
                                                                float kn, int third_is_normal, unsigned key0, unsigned key1,
                                                                unsigned draw, unsigned sample) {
    const Voxel p = block_voxel(H, W);
    if (!p.inside) return;
    const size_t v = p.v;
    const unsigned v0 = (unsigned)v, v1 = (unsigned)((unsigned long long)v >> 32);
    const float xt = x_t[v];
    if (cov[v] == 0.f) {
        x_next[v] = xt;
        x0_out[v] = 0.f;
        return;
    }
    const float x0 = fmaf(w, c[v], a[v]);
    const float prev = x0_prev ? x0_prev[v] : 0.f;
    float n = 0.f;
    if (kn != 0.f) n = philox_normal(philox4x32_10(v0, v1, draw, sample, key0, key1));
    const float r = third_is_normal ? sampler_update(kx, xt, k0, x0, kn, n) : sampler_update_sde(kx, xt, k0, x0, kp, prev, kn, n);
    x0_out[v] = x0;
    x_next[v] = r;
}

// The stochastic Heun sampler of the EDM family (elucidated_imagen.py:382-532) on the same state: a churn, a predictor and a corrector
// per step, two U-Net evaluations, so the state is three volumes -- xh = images_hat, xn = images_next, x0 = the fused prediction (the
// one self-conditioning reads) -- and the launch takes a `phase`, uniform over the grid:
//   0 (no y)                       xh = (a n(draw)) + kc n(draw + 1): the initial image sigma0 n, rounded as the sampler stores it, then
//                                  the churn of step 0;
//   1 (after the stage-0 windows)  x0 = sum(w c(y)) / sum(w), xn = a xh + b x0: the Euler predictor, (a, b) = (1 + r, -r);
//   2 (after the stage-1 windows)  x0b = sum(w c(y)) / sum(w), t = a xh + b x0 + c xn, x = t + d x0b: the corrector, (a, b, c, d) =
//                                  (1 + r/2, -r/2, r2, -r2); then the next step's churn xh = x + kc n(draw) (no Philox call when
//                                  kc == 0) and x0 = x0b.
// A voxel no kept window covers: phase 1 writes xn = xh and x0 = 0, phase 2 leaves xh and writes x0 = 0 (nothing ever gathers it).
// The prologue, the fuse and the normals are the linear kernel's own.  Every thread reads only its own voxel of xh / xn / x0, then writes
// it: all three are updated in place (no __restrict__ on them).
// axpby3_kernel's `v = k0 a; v += k1 b; v += k2 c` as the compiler contracts it there: the first product is rounded, every later one
// is fused into the running sum.  Spelled out (and kept from further contraction) so that at stride = patch the joint chain is
// ElucidatedImagen.one_unet_sample's bit for bit.
__device__ __forceinline__ float axpby_update(float k0, float a, float k1, float b) {
#pragma clang fp contract(off)
    const float v = k0 * a;
    return fmaf(k1, b, v);
}
// The two updates of the inpainting loop around that sampler (RePaint; elucidated_imagen.py:473-530), with the roundings of the
// diqt_axpby3 calls they stand for -- ONE definition for the per-window pass and the joint pass:
//   inpaint_renoise   images + (sigma - sigma_next) n, the re-noise that ends a pass:   axpby3(x, n, 1, kr), 1 x is x bit for bit;
//   inpaint_churn     the known value under the mask, then the churn of the next pass:  axpby3(sel(m, known, t), eps, 1, kc).  The
//                     product is fused in also when kc == 0, as axpby3 does it (an unmasked -0 plus a +0 product is +0 there too).
__device__ __forceinline__ float inpaint_renoise(float x, float kr, float n) { return axpby_update(1.f, x, kr, n); }
__device__ __forceinline__ float inpaint_churn(bool m, float known, float t, float kc, float eps) {
    return axpby_update(1.f, m ? known : t, kc, eps);
}
// The per-window pass: x / renoise / known / eps / out [B][per], mask one byte per element, kr / kc device [B].  renoise == NULL: no
// re-noise (kr is not read).  out may alias x (every thread reads its own element, then writes it).  Block (64, 4) = 256 consecutive
// elements of sample blockIdx.y; the store follows the last use of a load.
__global__ __launch_bounds__(256) void edm_inpaint_churn_kernel(const float* x, const float* __restrict__ renoise,
                                                                const float* __restrict__ known,
                                                                const unsigned char* __restrict__ mask,
                                                                const float* __restrict__ eps, const float* __restrict__ kr,
                                                                const float* __restrict__ kc, float* out, size_t per) {
    const int b = blockIdx.y;
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.y * 64 + threadIdx.x;
    if (e >= per) return;
    const size_t v = (size_t)b * per + e;
    const bool m = mask[v] != 0;
    const float kn = known[v], ep = eps[v];
    float t = x[v];
    if (renoise) t = inpaint_renoise(t, kr[b], renoise[v]);
    out[v] = inpaint_churn(m, kn, t, kc[b], ep);
}
// The same loop around the ancestral sampler of the DDPM family (Imagen.p_sample_loop; the reference's imagen_pytorch3D.py:2116-2146),
// again ONE definition for the per-window pass and the joint pass:
//   ddpm_renoise   q_sample_from_to(img, t_next, t), the re-noise that ends a pass:  axpby3(img, n, renoise[i,0], renoise[i,1]);
//   ddpm_paste     q_sample(known, t) under the mask, t elsewhere: q_sample IS axpby3(known, nq, alpha, sigma), and mask_blend after it a
//                  pure selection -- an unmasked element keeps its bits (a -0 stays -0), there is no product to add.
__device__ __forceinline__ float ddpm_renoise(float x, float kr0, float kr1, float n) { return axpby_update(kr0, x, kr1, n); }
__device__ __forceinline__ float ddpm_paste(bool m, float known, float al, float sg, float nq, float t) {
    return m ? axpby_update(al, known, sg, nq) : t;
}
// The per-window pass boundary: x / renoise / known / qnoise / out [B][per], mask one byte per element, kr0 / kr1 / al / sg device
// [B].  renoise == NULL: no re-noise (kr0 / kr1 are not read).  out may alias x.  Geometry and the order of loads and the store as in
// edm_inpaint_churn_kernel.
__global__ __launch_bounds__(256) void ddpm_inpaint_paste_kernel(const float* x, const float* __restrict__ renoise,
                                                                 const float* __restrict__ known,
                                                                 const unsigned char* __restrict__ mask,
                                                                 const float* __restrict__ qnoise, const float* __restrict__ kr0,
                                                                 const float* __restrict__ kr1, const float* __restrict__ al,
                                                                 const float* __restrict__ sg, float* out, size_t per) {
    const int b = blockIdx.y;
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.y * 64 + threadIdx.x;
    if (e >= per) return;
    const size_t v = (size_t)b * per + e;
    const bool m = mask[v] != 0;
    const float kn = known[v], nq = qnoise[v];
    float t = x[v];
    if (renoise) t = ddpm_renoise(t, kr0[b], kr1[b], renoise[v]);
    out[v] = ddpm_paste(m, kn, al[b], sg[b], nq, t);
}
__global__ __launch_bounds__(256) void volume_joint_heun_kernel(const float* __restrict__ y, const int* __restrict__ slot,
                                                                const float* __restrict__ taps, float* xh, float* xn, float* x0v,
                                                                int phase, int N, int D, int H, int W, int P, int stride, int G0, int G1,
                                                                int G2, float a, float b, float c, float d, float kc, float lo, float hi,
                                                                int clamp_mode, unsigned key0, unsigned key1, unsigned draw,
                                                                unsigned sample) {
    extern __shared__ float tp[];                      // [P]
    const Voxel p = walk_prologue(tp, taps, P, phase != 0, H, W);
    if (!p.inside) return;
    const size_t v = p.v;
    const unsigned v0 = (unsigned)v, v1 = (unsigned)((unsigned long long)v >> 32);
    if (phase == 0) {
        float r = axpby_update(a, philox_normal(philox4x32_10(v0, v1, draw, sample, key0, key1)), 0.f, 0.f);
        if (kc != 0.f) r = fmaf(kc, philox_normal(philox4x32_10(v0, v1, draw + 1u, sample, key0, key1)), r);
        xh[v] = r;
        return;
    }
    const Fused f = joint_fuse(y, slot, taps, tp, N, P, stride, G0, G1, G2, p, StepClamp{lo, hi, clamp_mode});
    if (phase == 1) {
        const float h_ = xh[v];
        if (!f.covered()) {
            xn[v] = h_;
            x0v[v] = 0.f;
            return;
        }
        const float x0 = f.x0();
        x0v[v] = x0;
        xn[v] = axpby_update(a, h_, b, x0);
        return;
    }
    if (!f.covered()) {
        x0v[v] = 0.f;
        return;
    }
    const float x0b = f.x0();
    const float t = fmaf(c, xn[v], axpby_update(a, xh[v], b, x0v[v]));
    float r = fmaf(d, x0b, t);                         // axpby3(tmp, out2, 1, d): 1 * tmp is tmp
    if (kc != 0.f) r = fmaf(kc, philox_normal(philox4x32_10(v0, v1, draw, sample, key0, key1)), r);
    xh[v] = r;
    x0v[v] = x0b;
}
// Phases 1 and 2 of the kernel above with the data-consistency projection between the fuse and the update
// (diqt_volume_joint_consistent_heun): the box geometry and the two passes of volume_joint_consistent_kernel -- a (64, 4) block owns a
// box of whole cells (cell_box), pass 1 fuses every voxel of the box into LDS (x0s, dens), one barrier, pass 2 revisits the SAME voxels
// -- and the updates of that kernel's phases, with the projected prediction in the place of the fused one.  In a cell whose voxels are
// ALL covered the fused x0 becomes x0' = x0 + w A+(y - A x0) by the one definition of its MODE:
//   0 (uniform)  cell_mean / cell_shift;
//   1 (profile)  cell_wmean / cell_wshift, `table` [2][n] in LDS behind dens;
//   2 (tile)     tile_apply on P = `table` [n][n] (in LDS behind dens) read with stride n, then cell_shift by meas_up = t.
// A cell with an uncovered voxel is left alone: its covered voxels take the update with their plain x0.  Phase 1 stores x0v = x0' and
// xn = a xh + b x0'; phase 2 forms t = fma(c, xn, a xh + b x0v) and r = fma(d, x0b', t), churns r by kc n(draw) (no Philox call when
// kc == 0) and stores xh = r, x0v = x0b'.  An uncovered voxel: phase 1 writes xn = xh and x0v = 0, phase 2 leaves xh and writes
// x0v = 0.  `phase` is uniform over the launch; there is no phase 0 here (the initial state is the plain kernel's).  A thread reads and
// writes only its own voxels of xh / xn / x0v, each read before it is written, and whole cells lie in one block: all three are updated
// in place, without an atomic and without waiting across blocks.  At stride = patch the chain is one_unet_sample's Heun loop with the
// per-window projection launch after an evaluation, bit for bit.
template <int MODE>
__global__ __launch_bounds__(256) void volume_joint_consistent_heun_kernel(const float* __restrict__ y, const int* __restrict__ slot,
                                                                           const float* __restrict__ taps, float* xh, float* xn,
                                                                           float* x0v, const float* __restrict__ meas_up,
                                                                           const float* __restrict__ table, int phase, int N, int D,
                                                                           int H, int W, int P, int stride, int G0, int G1, int G2,
                                                                           Cell cell, float w, float a, float b, float c, float d,
                                                                           float kc, float lo, float hi, int clamp_mode, unsigned key0,
                                                                           unsigned key1, unsigned draw, unsigned sample) {
    extern __shared__ float tp[];                      // [P], then x0s [nb] and den [nb]; profile: the table [2][n]; tile: P [n][n]
    const CellBox box = cell_box(cell);
    const int nb = cell.fz * box.by * box.bx, t = threadIdx.y * 64 + threadIdx.x;
    float* x0s = tp + P;
    float* dens = x0s + nb;
    float* tab = dens + nb;
    const int n = cell.fz * cell.fy * cell.fx;
    for (int e = t; e < P; e += 256) tp[e] = taps[e];
    if constexpr (MODE != 0)
        for (int e = t; e < (MODE == 1 ? 2 * n : n * n); e += 256) tab[e] = table[e];
    __syncthreads();
    const int z0 = blockIdx.z * cell.fz, y0 = blockIdx.y * box.by, xb = blockIdx.x * box.bx;
    for (int e = t; e < nb; e += 256) {
        const int lx = e % box.bx, ly = (e / box.bx) % box.by, lz = e / (box.bx * box.by);
        const Voxel p{xb + lx, y0 + ly, z0 + lz, 0, y0 + ly < H && xb + lx < W};
        Fused f{0.f, 0.f};
        if (p.inside) f = joint_fuse(y, slot, taps, tp, N, P, stride, G0, G1, G2, p, StepClamp{lo, hi, clamp_mode});
        x0s[e] = f.covered() ? f.x0() : 0.f;
        dens[e] = f.den;
    }
    __syncthreads();
    for (int e = t; e < nb; e += 256) {
        const int lx = e % box.bx, ly = (e / box.bx) % box.by, lz = e / (box.bx * box.by);
        const int x = xb + lx, h = y0 + ly, dz = z0 + lz;
        if (h >= H || x >= W) continue;
        const size_t v = ((size_t)dz * H + h) * W + x;
        if (dens[e] == 0.f) {
            if (phase == 1) xn[v] = xh[v];
            x0v[v] = 0.f;
            continue;
        }
        // the cell of this voxel inside the box (the box is one cell deep) and the voxel's index inside its cell
        const int cb = ((ly / cell.fy) * cell.fy) * box.bx + (lx / cell.fx) * cell.fx;
        const int q = (lz * cell.fy + ly % cell.fy) * cell.fx + lx % cell.fx;
        bool all = true;
        auto value = [&](int i, int j, int k) {
            const int u = cb + (i * box.by + j) * box.bx + k;
            all = all && dens[u] != 0.f;
            return x0s[u];
        };
        float x0 = x0s[e];
        if constexpr (MODE == 0) {
            const float m = cell_mean(cell, value);
            if (all) x0 = cell_shift(w, meas_up[v], m, x0);
        } else if constexpr (MODE == 1) {
            const float m = cell_wmean(cell, tab, value);
            if (all) x0 = cell_wshift(w, tab[n + q], meas_up[v], m, x0);
        } else {
            const float s = tile_apply(cell, tab + q, n, value);
            if (all) x0 = cell_shift(w, meas_up[v], s, x0);
        }
        if (phase == 1) {
            const float h_ = xh[v];
            x0v[v] = x0;
            xn[v] = axpby_update(a, h_, b, x0);
            continue;
        }
        const float u = fmaf(c, xn[v], axpby_update(a, xh[v], b, x0v[v]));
        float r = fmaf(d, x0, u);                      // axpby3(tmp, out2, 1, d): 1 * tmp is tmp
        if (kc != 0.f)
            r = fmaf(kc, philox_normal(philox4x32_10((unsigned)v, (unsigned)((unsigned long long)v >> 32), draw, sample, key0, key1)), r);
        xh[v] = r;
        x0v[v] = x0;
    }
}
// The same chain with the inpainting loop on the joint state (diqt_volume_joint_heun_inpaint): known [D][H][W] in state space, mask one
// byte per voxel.  The predictor is phase 1 of the kernel above; the phases here, numbered as there, paste and churn with the helpers
// of the per-window pass:
//   0 (no y)                       xh = sel(m, known, a n(draw)) + kc n(draw + 1);
//   2 (after the stage-1 windows)  the corrector above up to x; where kr != 0, x = x + kr n(draw_r), the re-noise that ends a pass which
//                                  is not the last of its step; then xh = sel(m, known, x) + kc n(draw) and x0 = x0b;
//   3 (no y, no window walk)       xh = sel(m, known, xn) + kc n(draw): the further passes of the step that ends at sigma 0, which has no
//                                  corrector.  Every voxel: an uncovered one holds xn = xh since phase 1, and nothing gathers it.
// With kc == 0 the churn is the selection alone and there is no Philox call, as above.  A voxel no kept window covers: phase 2 leaves
// xh and writes x0 = 0.  xh and x0 are updated in place; the stores follow the last use of a load.
__global__ __launch_bounds__(256) void volume_joint_heun_inpaint_kernel(const float* __restrict__ y, const int* __restrict__ slot,
                                                                        const float* __restrict__ taps, float* xh, const float* xn,
                                                                        float* x0v, const float* __restrict__ known,
                                                                        const unsigned char* __restrict__ mask, int phase, int N, int D,
                                                                        int H, int W, int P, int stride, int G0, int G1, int G2, float a,
                                                                        float b, float c, float d, float kr, float kc, float lo,
                                                                        float hi, int clamp_mode, unsigned key0, unsigned key1,
                                                                        unsigned draw, unsigned draw_r, unsigned sample) {
    extern __shared__ float tp[];                      // [P]
    const Voxel p = walk_prologue(tp, taps, P, phase == 2, H, W);
    if (!p.inside) return;
    const size_t v = p.v;
    const unsigned v0 = (unsigned)v, v1 = (unsigned)((unsigned long long)v >> 32);
    if (phase != 2) {
        const bool m = mask[v] != 0;
        const float kn = known[v];
        unsigned dc = draw;
        float t;
        if (phase == 0) {
            t = axpby_update(a, philox_normal(philox4x32_10(v0, v1, draw, sample, key0, key1)), 0.f, 0.f);
            dc = draw + 1u;
        } else {
            t = xn[v];
        }
        xh[v] = kc != 0.f ? inpaint_churn(m, kn, t, kc, philox_normal(philox4x32_10(v0, v1, dc, sample, key0, key1))) : (m ? kn : t);
        return;
    }
    const Fused f = joint_fuse(y, slot, taps, tp, N, P, stride, G0, G1, G2, p, StepClamp{lo, hi, clamp_mode});
    if (!f.covered()) {
        x0v[v] = 0.f;
        return;
    }
    const float x0b = f.x0();
    const bool m = mask[v] != 0;
    const float kn = known[v];
    const float t = fmaf(c, xn[v], axpby_update(a, xh[v], b, x0v[v]));
    float r = fmaf(d, x0b, t);
    if (kr != 0.f) r = inpaint_renoise(r, kr, philox_normal(philox4x32_10(v0, v1, draw_r, sample, key0, key1)));
    r = kc != 0.f ? inpaint_churn(m, kn, r, kc, philox_normal(philox4x32_10(v0, v1, draw, sample, key0, key1))) : (m ? kn : r);
    xh[v] = r;
    x0v[v] = x0b;
}
// The inpainting loop of the DDPM family on the joint state (diqt_volume_joint_step_inpaint): the first-order step of
// volume_joint_linear_kernel with the pass boundary of ddpm_inpaint_paste_kernel behind it, x updated in place.  `phase` and `flags` are
// uniform over the launch:
//   phase 0 (no y, every voxel)   x = ddpm_paste(m, known, al, sg, n(draw_q), n(draw)): the initial image under the first paste;
//   phase 1 (after the windows)   x0 = sum(w c(y)) / sum(w); u = sampler_update(kx, x, k0, x0, kn, n(draw)) (the product added also when
//                                 it is 0, no Philox call when kn == 0); flags & 1: u = ddpm_renoise(u, kr0, kr1, n(draw_r)), the re-noise
//                                 that ends a pass; flags & 2: x = ddpm_paste(m, known, al, sg, n(draw_q), u), the paste that begins the
//                                 next pass with ITS step's (al, sg); else x = u.  x0_out (may be NULL) = x0.
// A masked voxel with a paste following stores a value that does not depend on u: it computes n(draw_q) alone -- no step, no other
// normal.  A voxel no kept window covers: phase 1 leaves x and writes x0_out = 0.  The stores follow the last use of a load.
__global__ __launch_bounds__(256) void volume_joint_step_inpaint_kernel(const float* __restrict__ y, const int* __restrict__ slot,
                                                                        const float* __restrict__ taps, float* x, float* x0_out,
                                                                        const float* __restrict__ known,
                                                                        const unsigned char* __restrict__ mask, int phase, int flags,
                                                                        int N, int D, int H, int W, int P, int stride, int G0, int G1,
                                                                        int G2, float kx, float k0, float kn, float kr0, float kr1,
                                                                        float al, float sg, float lo, float hi, int clamp_mode,
                                                                        unsigned key0, unsigned key1, unsigned draw, unsigned draw_r,
                                                                        unsigned draw_q, unsigned sample) {
    extern __shared__ float tp[];                      // [P]
    const Voxel p = walk_prologue(tp, taps, P, phase == 1, H, W);
    if (!p.inside) return;
    const size_t v = p.v;
    const unsigned v0 = (unsigned)v, v1 = (unsigned)((unsigned long long)v >> 32);
    if (phase == 0) {
        float r;
        if (mask[v] != 0) r = ddpm_paste(true, known[v], al, sg, philox_normal(philox4x32_10(v0, v1, draw_q, sample, key0, key1)), 0.f);
        else r = philox_normal(philox4x32_10(v0, v1, draw, sample, key0, key1));
        x[v] = r;
        return;
    }
    const Fused f = joint_fuse(y, slot, taps, tp, N, P, stride, G0, G1, G2, p, StepClamp{lo, hi, clamp_mode});
    if (!f.covered()) {
        if (x0_out) x0_out[v] = 0.f;
        return;
    }
    const bool pasted = (flags & 2) && mask[v] != 0;
    const float xt = x[v], kv = known[v];
    const float x0 = f.x0();
    float r;
    if (pasted) {
        r = ddpm_paste(true, kv, al, sg, philox_normal(philox4x32_10(v0, v1, draw_q, sample, key0, key1)), 0.f);
    } else {
        float n = 0.f;
        if (kn != 0.f) n = philox_normal(philox4x32_10(v0, v1, draw, sample, key0, key1));
        r = sampler_update(kx, xt, k0, x0, kn, n);
        if (flags & 1) r = ddpm_renoise(r, kr0, kr1, philox_normal(philox4x32_10(v0, v1, draw_r, sample, key0, key1)));
    }
    if (x0_out) x0_out[v] = x0;
    x[v] = r;
}

// The end of sample s of S: r = min_val on the background (background_reset_kernel's expression on the RAW vol), else x where a kept
// window covers the voxel, else fill; then volume_blend_kernel's Welford update of (mean_io, m2_io) with r, and after the last sample
// the unbiased deviation.  Sample 0 initialises the running pair (nothing is read from mean_io / m2_io then).
__global__ __launch_bounds__(256) void volume_joint_finish_kernel(const float* __restrict__ xs, const int* __restrict__ slot,
                                                                  const float* __restrict__ vol, float* __restrict__ mean_io,
                                                                  float* __restrict__ m2_io, float* __restrict__ out_std, int s, int S,
                                                                  int D, int H, int W, int P, int stride, int G0, int G1, int G2,
                                                                  float mean, float stdv, float min_val, float fill) {
    const Voxel p = block_voxel(H, W);
    if (!p.inside) return;
    const size_t v = p.v;
    float r;
    if (vol && (vol[v] - mean) / stdv == min_val) {
        r = min_val;
    } else {
        const Cover cv = covering(p.d, p.h, p.x, P, stride, G0, G1, G2);
        bool covered = false;
        for (int g0 = cv.lo0; g0 <= cv.hi0 && !covered; ++g0)
            for (int g1 = cv.lo1; g1 <= cv.hi1 && !covered; ++g1) {
                const int* srow = slot + ((size_t)g0 * G1 + g1) * G2;
                for (int g2 = cv.lo2; g2 <= cv.hi2 && !covered; ++g2) covered = srow[g2] >= 0;
            }
        r = covered ? xs[v] : fill;
    }
    float m = 0.f, m2 = 0.f;
    if (s > 0) {
        m = mean_io[v];
        if (m2_io) m2 = m2_io[v];
    }
    const float delta = r - m;
    m += delta / (float)(s + 1);
    m2 = fmaf(delta, r - m, m2);
    mean_io[v] = m;
    if (m2_io) m2_io[v] = m2;
    if (out_std && s == S - 1) out_std[v] = sqrtf(m2 / (float)(S - 1));
}
}  // namespace diqt

using namespace diqt;

static unsigned crop_blocks(int P) { return grid_for((size_t)P * P * P, 256, 64); }

extern "C" size_t diqt_patch_pair_crop_workspace_bytes(int n_patches, int P) {
    if (n_patches <= 0 || P <= 0) return 0;
    return (size_t)2 * n_patches * crop_blocks(P) * sizeof(MinMax);
}
extern "C" int diqt_patch_pair_crop(const float* lr_vols, const float* hr_vols, const int* sel, float* lr_out, float* hr_out,
                                    void* workspace, size_t workspace_bytes, int n_patches, int V, int D, int H, int W, int P,
                                    int mode, float mean, float stdv, void* stream) {
    DIQT_REQUIRE(lr_vols && hr_vols && sel && lr_out && hr_out, DIQT_E_ALIGN, "patch_pair_crop: null pointer");
    DIQT_REQUIRE(V > 0 && D > 0 && H > 0 && W > 0 && P > 0 && P <= D && P <= H && P <= W, DIQT_E_SHAPE, "patch_pair_crop: bad shape");
    DIQT_REQUIRE(mode == 0 || mode == 1, DIQT_E_UNSUPPORTED, "patch_pair_crop: mode %d (0 = z-score, 1 = min-max)", mode);
    DIQT_REQUIRE(mode == 1 || stdv != 0.f, DIQT_E_SHAPE, "patch_pair_crop: std == 0");
    if (n_patches <= 0) return DIQT_OK;
    DIQT_REQUIRE(n_patches <= 65535, DIQT_E_SHAPE, "patch_pair_crop: at most 65535 patches per call");
    const unsigned nb = crop_blocks(P);
    MinMax* part = static_cast<MinMax*>(workspace);
    if (mode == 1) {
        DIQT_REQUIRE(workspace && workspace_bytes >= diqt_patch_pair_crop_workspace_bytes(n_patches, P), DIQT_E_SHAPE,
                     "patch_pair_crop: workspace too small");
        hipLaunchKernelGGL(crop_minmax_kernel, dim3(nb, n_patches, 2), dim3(256), 0, STREAM, lr_vols, hr_vols, sel, part, D, H, W, P);
        int rc = check_launch("patch_pair_crop/minmax");
        if (rc) return rc;
    }
    hipLaunchKernelGGL(crop_apply_kernel, dim3(nb, n_patches, 2), dim3(256), 0, STREAM, lr_vols, hr_vols, sel, part, lr_out, hr_out, D, H,
                       W, P, mode, mean, stdv);
    return check_launch("patch_pair_crop");
}

extern "C" int diqt_minmax(const float* x, size_t n, void* workspace_8k, float* out2, void* stream) {
    DIQT_REQUIRE(x && workspace_8k && out2 && n > 0, DIQT_E_ALIGN, "minmax: null pointer / empty input");
    const unsigned nb = grid_for(n, 256, 1024);
    hipLaunchKernelGGL(minmax_stage1_kernel, dim3(nb), dim3(256), 0, STREAM, x, static_cast<MinMax*>(workspace_8k), n);
    int rc = check_launch("minmax/stage1");
    if (rc) return rc;
    hipLaunchKernelGGL(minmax_stage2_kernel, dim3(1), dim3(64), 0, STREAM, static_cast<const MinMax*>(workspace_8k), (int)nb, out2);
    return check_launch("minmax/stage2");
}

extern "C" int diqt_psnr(const float* pred, const float* target, size_t n, const float* stats4, float data_range, void* workspace_8k,
                         float* out2, void* stream) {
    DIQT_REQUIRE(pred && target && workspace_8k && out2 && n > 0, DIQT_E_ALIGN, "psnr: null pointer / empty input");
    DIQT_REQUIRE(data_range > 0.f, DIQT_E_SHAPE, "psnr: data_range must be positive");
    const unsigned nb = grid_for(n, 256, 1024);
    hipLaunchKernelGGL(sqerr_stage1_kernel, dim3(nb), dim3(256), 0, STREAM, pred, target, stats4, static_cast<double*>(workspace_8k), n);
    int rc = check_launch("psnr/stage1");
    if (rc) return rc;
    hipLaunchKernelGGL(psnr_stage2_kernel, dim3(1), dim3(64), 0, STREAM, static_cast<const double*>(workspace_8k), (int)nb, (double)n,
                       data_range, out2);
    return check_launch("psnr/stage2");
}

static void ssim_tiles(int N, int D, int H, int W, int K, int& tD, int& tH, int& tW, size_t& blocks) {
    tD = (D - K + 1 + ST - 1) / ST; tH = (H - K + 1 + ST - 1) / ST; tW = (W - K + 1 + ST - 1) / ST;
    blocks = (size_t)N * tD * tH * tW;
}
extern "C" size_t diqt_ssim3d_workspace_bytes(int N, int D, int H, int W, int K) {
    if (N <= 0 || K < 1 || K > SK || D < K || H < K || W < K) return 0;
    int a, b, c;
    size_t blocks;
    ssim_tiles(N, D, H, W, K, a, b, c, blocks);
    return blocks * sizeof(double);
}
extern "C" int diqt_ssim3d(const float* pred, const float* target, int N, int D, int H, int W, const float* taps, int K,
                           const float* stats4, float data_range, float k1, float k2, void* workspace, size_t workspace_bytes,
                           float* out, void* stream) {
    DIQT_REQUIRE(pred && target && taps && out, DIQT_E_ALIGN, "ssim3d: null pointer");
    DIQT_REQUIRE(K >= 1 && K <= SK && (K & 1), DIQT_E_UNSUPPORTED, "ssim3d: filter size %d (odd, <= %d)", K, SK);
    DIQT_REQUIRE(N > 0 && D >= K && H >= K && W >= K, DIQT_E_SHAPE, "ssim3d: volume smaller than the filter");
    int tD, tH, tW;
    size_t blocks;
    ssim_tiles(N, D, H, W, K, tD, tH, tW, blocks);
    DIQT_REQUIRE(blocks <= 0x7fffffffu, DIQT_E_SHAPE, "ssim3d: too many tiles");
    DIQT_REQUIRE(workspace && workspace_bytes >= blocks * sizeof(double), DIQT_E_SHAPE, "ssim3d: workspace too small");
    SsimTaps tp;
    for (int i = 0; i < SK; ++i) tp.w[i] = i < K ? taps[i] : 0.f;      // taps: HOST pointer
    tp.K = K;
    const float c1 = (k1 * data_range) * (k1 * data_range), c2 = (k2 * data_range) * (k2 * data_range);
    const size_t lds = (size_t)(2 * SI * SI * SI + 5 * SI * SI * ST + 5 * SI * ST * ST) * sizeof(float);
    static bool attr_set = false;
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(ssim_tile_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        DIQT_REQUIRE(e == hipSuccess, DIQT_E_LAUNCH, "ssim3d: LDS attribute: %s", hipGetErrorString(e));
        attr_set = true;
    }
    hipLaunchKernelGGL(ssim_tile_kernel<false>, dim3((unsigned)blocks), dim3(256), lds, STREAM, pred, target, stats4,
                       static_cast<double*>(workspace), D, H, W, tD, tH, tW, tp, c1, c2, MsScale{});
    int rc = check_launch("ssim3d/tiles");
    if (rc) return rc;
    const double count = (double)N * (D - K + 1) * (H - K + 1) * (W - K + 1);
    hipLaunchKernelGGL(mean_stage2_kernel, dim3(1), dim3(64), 0, STREAM, static_cast<const double*>(workspace), (int)blocks, count, out);
    return check_launch("ssim3d/mean");
}

// Workspace of diqt_msssim3d: {range[scales + 1] | range_0 min/max partials | part[2 * blocks_0] doubles | mm[4 * blocks_0] |
// pooled p, t of the odd scales | pooled p, t of the even scales} -- scale s + 1 is written while scale s is read, so two
// buffers alternate.
namespace {
struct MsLayout {
    size_t mm0, part, mm, pool[2], pool_elems[2], total, blocks0;
    bool ok;
};
constexpr unsigned MS_MM0_BLOCKS = 1024;
size_t ms_align(size_t n) { return (n + 255) & ~(size_t)255; }
MsLayout ms_layout(int N, int D, int H, int W, int K, int scales) {
    MsLayout L{};
    if (N <= 0 || K < 1 || K > SK || !(K & 1) || scales < 1 || scales > MS_MAX_SCALES || D <= 0 || H <= 0 || W <= 0) return L;
    if ((D >> (scales - 1)) < K || (H >> (scales - 1)) < K || (W >> (scales - 1)) < K) return L;
    int a, b, c;
    ssim_tiles(N, D, H, W, K, a, b, c, L.blocks0);
    if (L.blocks0 > 0x7fffffffu) return L;
    L.pool_elems[0] = scales > 1 ? (size_t)N * (D >> 1) * (H >> 1) * (W >> 1) : 0;      // scale 1 (largest of the odd scales)
    L.pool_elems[1] = scales > 2 ? (size_t)N * (D >> 2) * (H >> 2) * (W >> 2) : 0;      // scale 2
    L.mm0 = ms_align((MS_MAX_SCALES + 1) * sizeof(float));
    L.part = L.mm0 + ms_align(2 * MS_MM0_BLOCKS * sizeof(MinMax));
    L.mm = L.part + ms_align(2 * L.blocks0 * sizeof(double));
    L.pool[0] = L.mm + ms_align(4 * L.blocks0 * sizeof(float));
    L.pool[1] = L.pool[0] + ms_align(2 * L.pool_elems[0] * sizeof(float));
    L.total = L.pool[1] + ms_align(2 * L.pool_elems[1] * sizeof(float));
    L.ok = true;
    return L;
}
}  // namespace
extern "C" size_t diqt_msssim3d_workspace_bytes(int N, int D, int H, int W, int K, int scales) {
    const MsLayout L = ms_layout(N, D, H, W, K, scales);
    return L.ok ? L.total : 0;
}
extern "C" int diqt_msssim3d(const float* pred, const float* target, int N, int D, int H, int W, const float* taps, int K,
                             const float* betas, int scales, float k1, float k2, void* workspace, size_t workspace_bytes, float* out,
                             void* stream) {
    DIQT_REQUIRE(pred && target && taps && betas && out, DIQT_E_ALIGN, "msssim3d: null pointer");
    DIQT_REQUIRE(K >= 1 && K <= SK && (K & 1), DIQT_E_UNSUPPORTED, "msssim3d: filter size %d (odd, <= %d)", K, SK);
    DIQT_REQUIRE(scales >= 1 && scales <= MS_MAX_SCALES, DIQT_E_UNSUPPORTED, "msssim3d: %d scales (1 .. %d)", scales, MS_MAX_SCALES);
    const MsLayout L = ms_layout(N, D, H, W, K, scales);
    DIQT_REQUIRE(L.ok, DIQT_E_SHAPE, "msssim3d: %dx%dx%d leaves fewer than %d voxels on an axis at scale %d", D, H, W, K, scales - 1);
    DIQT_REQUIRE(workspace && workspace_bytes >= L.total, DIQT_E_SHAPE, "msssim3d: workspace too small");
    SsimTaps tp;
    for (int i = 0; i < SK; ++i) tp.w[i] = i < K ? taps[i] : 0.f;      // taps, betas: HOST pointers
    tp.K = K;
    MsBetas bt;
    for (int i = 0; i < MS_MAX_SCALES; ++i) bt.b[i] = i < scales ? betas[i] : 0.f;
    const size_t lds = (size_t)(2 * SI * SI * SI + 5 * SI * SI * ST + 5 * SI * ST * ST) * sizeof(float);
    static bool attr_set = false;
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(ssim_tile_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        DIQT_REQUIRE(e == hipSuccess, DIQT_E_LAUNCH, "msssim3d: LDS attribute: %s", hipGetErrorString(e));
        attr_set = true;
    }
    char* ws = static_cast<char*>(workspace);
    float* range = reinterpret_cast<float*>(ws);
    MinMax* mm0 = reinterpret_cast<MinMax*>(ws + L.mm0);
    double* part = reinterpret_cast<double*>(ws + L.part);
    float* mm = reinterpret_cast<float*>(ws + L.mm);
    // range_0: the two-stage min / max of diqt_minmax on each input, then one number
    const size_t n0 = (size_t)N * D * H * W;
    const unsigned nb0 = grid_for(n0, 256, MS_MM0_BLOCKS);
    hipLaunchKernelGGL(minmax_stage1_kernel, dim3(nb0), dim3(256), 0, STREAM, pred, mm0, n0);
    hipLaunchKernelGGL(minmax_stage1_kernel, dim3(nb0), dim3(256), 0, STREAM, target, mm0 + nb0, n0);
    hipLaunchKernelGGL(msssim_range0_kernel, dim3(1), dim3(64), 0, STREAM, mm0, (int)nb0, range);
    int rc = check_launch("msssim3d/range0");
    if (rc) return rc;
    const float *p = pred, *t = target;
    for (int s = 0; s < scales; ++s) {
        int tD, tH, tW;
        size_t blocks;
        ssim_tiles(N, D, H, W, K, tD, tH, tW, blocks);
        MsScale ms{range + s, k1, k2, nullptr, nullptr, mm};
        if (s + 1 < scales) {
            const int b = s & 1;                                       // scale s + 1 lives in pool[s & 1]
            ms.pool_p = reinterpret_cast<float*>(ws + L.pool[b]);
            ms.pool_t = ms.pool_p + (size_t)N * (D / 2) * (H / 2) * (W / 2);
        }
        hipLaunchKernelGGL(ssim_tile_kernel<true>, dim3((unsigned)blocks), dim3(256), lds, STREAM, p, t, (const float*)nullptr, part, D, H,
                           W, tD, tH, tW, tp, 0.f, 0.f, ms);
        rc = check_launch("msssim3d/tiles");
        if (rc) return rc;
        const double count = (double)N * (D - K + 1) * (H - K + 1) * (W - K + 1);
        hipLaunchKernelGGL(msssim_final_kernel, dim3(1), dim3(256), 0, STREAM, part, mm, (int)blocks, count, range, out, s, scales, bt);
        rc = check_launch("msssim3d/final");
        if (rc) return rc;
        p = ms.pool_p; t = ms.pool_t;
        D /= 2; H /= 2; W /= 2;
    }
    return DIQT_OK;
}

extern "C" int diqt_volume_blend(const float* patches, const int* slot, const float* taps, const float* vol, float* out_mean,
                                 float* out_std, int S, int N, int D, int H, int W, int P, int stride, int G0, int G1, int G2,
                                 float mean, float stdv, float min_val, float fill, void* stream) {
    DIQT_REQUIRE(slot && taps && out_mean && (patches || N == 0), DIQT_E_ALIGN, "volume_blend: null pointer");
    DIQT_REQUIRE(D > 0 && H > 0 && W > 0 && P > 0 && P <= D && P <= H && P <= W, DIQT_E_SHAPE, "volume_blend: bad shape");
    DIQT_REQUIRE(stride > 0 && S > 0 && N >= 0, DIQT_E_SHAPE, "volume_blend: stride %d, samples %d, windows %d", stride, S, N);
    DIQT_REQUIRE(G0 == (D - P) / stride + 1 && G1 == (H - P) / stride + 1 && G2 == (W - P) / stride + 1, DIQT_E_SHAPE,
                 "volume_blend: lattice %dx%dx%d does not match range(0, n - P + 1, stride) of %dx%dx%d, P %d, stride %d", G0, G1, G2, D,
                 H, W, P, stride);
    DIQT_REQUIRE(!(out_std && S == 1), DIQT_E_SHAPE, "volume_blend: a deviation map needs at least 2 samples");
    DIQT_REQUIRE(!vol || stdv != 0.f, DIQT_E_SHAPE, "volume_blend: std == 0");
    DIQT_REQUIRE(D <= 65535 && (H + 3) / 4 <= 65535, DIQT_E_SHAPE, "volume_blend: more than 65535 planes / row groups");
    hipLaunchKernelGGL(volume_blend_kernel, dim3((W + 63) / 64, (H + 3) / 4, D), dim3(64, 4), (size_t)P * sizeof(float), STREAM, patches,
                       slot, taps, vol, out_mean, out_std, S, N, D, H, W, P, stride, G0, G1, G2, mean, stdv, min_val, fill);
    return check_launch("volume_blend");
}

extern "C" int diqt_anchored_noise(const int* origins, int B, int C, int P, int D, int H, int W, unsigned long long seed, unsigned draw,
                                   unsigned sample, int raw, void* out, void* stream) {
    DIQT_REQUIRE(origins && out, DIQT_E_ALIGN, "anchored_noise: null pointer");
    DIQT_REQUIRE(B > 0 && C > 0 && P > 0 && D > 0 && H > 0 && W > 0 && P <= D && P <= H && P <= W, DIQT_E_SHAPE,
                 "anchored_noise: bad shape (B %d, C %d, P %d in %dx%dx%d)", B, C, P, D, H, W);
    DIQT_REQUIRE(P <= 1024, DIQT_E_SHAPE, "anchored_noise: windows of at most 1024^3 voxels");
    DIQT_REQUIRE(raw == 0 || raw == 1, DIQT_E_UNSUPPORTED, "anchored_noise: raw %d (0 = normals, 1 = the two Philox words)", raw);
    const size_t total = (size_t)B * C * P * P * P;
    const unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
    const unsigned nb = grid_for(total, 256);
    if (raw)
        hipLaunchKernelGGL(anchored_noise_kernel<true>, dim3(nb), dim3(256), 0, STREAM, origins, out, total, C, P, D, H, W, k0, k1, draw, sample);
    else
        hipLaunchKernelGGL(anchored_noise_kernel<false>, dim3(nb), dim3(256), 0, STREAM, origins, out, total, C, P, D, H, W, k0, k1, draw, sample);
    return check_launch("anchored_noise");
}

static int joint_lattice_ok(const char* who, int D, int H, int W, int P, int stride, int G0, int G1, int G2) {
    DIQT_REQUIRE(D > 0 && H > 0 && W > 0 && P > 0 && P <= D && P <= H && P <= W, DIQT_E_SHAPE, "%s: bad shape", who);
    DIQT_REQUIRE(stride > 0, DIQT_E_SHAPE, "%s: stride %d", who, stride);
    DIQT_REQUIRE(G0 == (D - P) / stride + 1 && G1 == (H - P) / stride + 1 && G2 == (W - P) / stride + 1, DIQT_E_SHAPE,
                 "%s: lattice %dx%dx%d does not match range(0, n - P + 1, stride) of %dx%dx%d, P %d, stride %d", who, G0, G1, G2, D, H, W,
                 P, stride);
    return DIQT_OK;
}

// What the four launches on the joint state share: the checks in the order every entry has made them -- the output volume, the shape,
// the grid limits, and for a launch that walks windows (an initial state looks at none of the window arguments) the window pointers
// (`window_ptrs`: the entry's own list), N, the lattice and the clamp mode -- then the grid of (64, 4) blocks and the LDS for the taps.
struct JointGrid { dim3 grid; size_t lds; };
static int joint_launch_plan(const char* who, const void* out, bool walks, bool window_ptrs, int N, int D, int H, int W, int P, int stride,
                             int G0, int G1, int G2, int clamp_mode, JointGrid& g) {
    DIQT_REQUIRE(out, DIQT_E_ALIGN, "%s: null pointer", who);
    DIQT_REQUIRE(D > 0 && H > 0 && W > 0, DIQT_E_SHAPE, "%s: bad shape", who);
    DIQT_REQUIRE(D <= 65535 && (H + 3) / 4 <= 65535, DIQT_E_SHAPE, "%s: more than 65535 planes / row groups", who);
    if (walks) {
        DIQT_REQUIRE(window_ptrs, DIQT_E_ALIGN, "%s: null pointer", who);
        DIQT_REQUIRE(N >= 0, DIQT_E_SHAPE, "%s: windows %d", who, N);
        int rc = joint_lattice_ok(who, D, H, W, P, stride, G0, G1, G2);
        if (rc) return rc;
        DIQT_REQUIRE(clamp_mode == 0 || clamp_mode == 1, DIQT_E_UNSUPPORTED, "%s: clamp_mode %d (0 = min, 1 = box)", who, clamp_mode);
    }
    g = JointGrid{dim3((W + 63) / 64, (H + 3) / 4, D), walks ? (size_t)P * sizeof(float) : 0};
    return DIQT_OK;
}
// volume_joint_linear_kernel behind its three entries; `third_is_normal` and the operands an entry does not have (x0_prev, kp, kn, the
// noise key) are the entry's to fill in.
static int joint_linear_launch(const char* who, bool window_ptrs, const float* y, const int* slot, const float* taps, const float* x_t,
                               const float* x0_prev, float* x_next, float* x0_out, int N, int D, int H, int W, int P, int stride, int G0,
                               int G1, int G2, float kx, float k0, float kp, float kn, float lo, float hi, int clamp_mode,
                               int third_is_normal, unsigned long long seed, unsigned draw, unsigned sample, void* stream) {
    JointGrid g;
    int rc = joint_launch_plan(who, x_next, x_t != nullptr, window_ptrs, N, D, H, W, P, stride, G0, G1, G2, clamp_mode, g);
    if (rc) return rc;
    hipLaunchKernelGGL(volume_joint_linear_kernel, g.grid, dim3(64, 4), g.lds, STREAM, y, slot, taps, x_t, x0_prev, x_next, x0_out, N, D,
                       H, W, P, stride, G0, G1, G2, kx, k0, kp, kn, lo, hi, clamp_mode, third_is_normal, (unsigned)seed,
                       (unsigned)(seed >> 32), draw, sample);
    return check_launch(who);
}

extern "C" int diqt_volume_joint_step(const float* y, const int* slot, const float* taps, const float* x_t, float* x_next, float* x0_out,
                                      int N, int D, int H, int W, int P, int stride, int G0, int G1, int G2, float kx, float k0, float kn,
                                      float lo, float hi, int clamp_mode, unsigned long long seed, unsigned draw, unsigned sample,
                                      void* stream) {
    // the initial state (x_t == NULL) is the plain normal: 1 n
    return joint_linear_launch("volume_joint_step", slot && taps && (y || N == 0), y, slot, taps, x_t, nullptr, x_next, x0_out, N, D, H, W,
                               P, stride, G0, G1, G2, kx, k0, 0.f, x_t ? kn : 1.f, lo, hi, clamp_mode, 1, seed, draw, sample, stream);
}

extern "C" int diqt_volume_joint_multistep(const float* y, const int* slot, const float* taps, const float* x_t, const float* x0_prev,
                                           float* x_next, float* x0_out, int N, int D, int H, int W, int P, int stride, int G0, int G1,
                                           int G2, float kx, float k0, float kp, float lo, float hi, int clamp_mode, void* stream) {
    // no initial state here, and every pointer is looked at before the shape
    DIQT_REQUIRE(x_t && x_next && x0_out && slot && taps && (y || N == 0), DIQT_E_ALIGN, "volume_joint_multistep: null pointer");
    return joint_linear_launch("volume_joint_multistep", true, y, slot, taps, x_t, x0_prev, x_next, x0_out, N, D, H, W, P, stride, G0, G1,
                               G2, kx, k0, kp, 0.f, lo, hi, clamp_mode, 0, 0, 0, 0, stream);
}

extern "C" int diqt_multistep_sde_step(const float* x, const float* x0, const float* x0_prev, const float* noise, const float* kx,
                                       const float* k0, const float* kp, const float* kn, float* x_next, int B, size_t per_batch,
                                       void* stream) {
    DIQT_REQUIRE(x && x0 && kx && k0 && kp && kn && x_next, DIQT_E_ALIGN, "multistep_sde_step: null pointer");
    DIQT_REQUIRE(B > 0 && per_batch > 0, DIQT_E_SHAPE, "multistep_sde_step: bad shape (B %d, per_batch %zu)", B, per_batch);
    DIQT_REQUIRE(B <= 65535 && (per_batch + 255) / 256 <= 0x7fffffffu, DIQT_E_SHAPE,
                 "multistep_sde_step: more than 65535 samples or 2^31 - 1 blocks per sample");
    hipLaunchKernelGGL(multistep_sde_step_kernel, dim3((unsigned)((per_batch + 255) / 256), B), dim3(64, 4), 0, STREAM, x, x0, x0_prev,
                       noise, kx, k0, kp, kn, x_next, per_batch);
    return check_launch("multistep_sde_step");
}

extern "C" int diqt_volume_joint_multistep_sde(const float* y, const int* slot, const float* taps, const float* x_t, const float* x0_prev,
                                               float* x_next, float* x0_out, int N, int D, int H, int W, int P, int stride, int G0,
                                               int G1, int G2, float kx, float k0, float kp, float kn, float lo, float hi,
                                               int clamp_mode, unsigned long long seed, unsigned draw, unsigned sample, void* stream) {
    return joint_linear_launch("volume_joint_multistep_sde", x0_out && slot && taps && (y || N == 0), y, slot, taps, x_t, x0_prev, x_next,
                               x0_out, N, D, H, W, P, stride, G0, G1, G2, kx, k0, kp, kn, lo, hi, clamp_mode, 0, seed, draw, sample, stream);
}

// The cell and the weight of the data-consistency entries: n = fz fy fx in 2 .. 64 and 0 < w <= 1, else DIQT_E_UNSUPPORTED.
static int cell_ok(const char* who, int fz, int fy, int fx, float w) {
    DIQT_REQUIRE(fz >= 1 && fy >= 1 && fx >= 1 && fz <= 64 && fy <= 64 && fx <= 64 && fz * fy * fx >= 2 && fz * fy * fx <= 64,
                 DIQT_E_UNSUPPORTED, "%s: cell %dx%dx%d (every factor >= 1, 2 <= fz fy fx <= 64)", who, fz, fy, fx);
    DIQT_REQUIRE(w > 0.f && w <= 1.f, DIQT_E_UNSUPPORTED, "%s: weight %g outside (0, 1]", who, (double)w);
    return DIQT_OK;
}

extern "C" int diqt_cell_mean(const float* x, float* out, int D, int H, int W, int fz, int fy, int fx, void* stream) {
    DIQT_REQUIRE(x && out, DIQT_E_ALIGN, "cell_mean: null pointer");
    int rc = cell_ok("cell_mean", fz, fy, fx, 1.f);
    if (rc) return rc;
    DIQT_REQUIRE(D > 0 && H > 0 && W > 0 && D % fz == 0 && H % fy == 0 && W % fx == 0, DIQT_E_SHAPE,
                 "cell_mean: the cell %dx%dx%d does not divide the volume %dx%dx%d", fz, fy, fx, D, H, W);
    const size_t cells = (size_t)(D / fz) * (H / fy) * (W / fx);
    DIQT_REQUIRE((cells + 255) / 256 <= 0x7fffffffu, DIQT_E_SHAPE, "cell_mean: more than 2^31 - 1 blocks");
    hipLaunchKernelGGL(cell_mean_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, STREAM, x, out, cells, H, W, Cell{fz, fy, fx});
    return check_launch("cell_mean");
}

extern "C" int diqt_cell_wmean(const float* x, const float* table, float* out, int D, int H, int W, int fz, int fy, int fx,
                               void* stream) {
    DIQT_REQUIRE(x && table && out, DIQT_E_ALIGN, "cell_wmean: null pointer");
    int rc = cell_ok("cell_wmean", fz, fy, fx, 1.f);
    if (rc) return rc;
    DIQT_REQUIRE(D > 0 && H > 0 && W > 0 && D % fz == 0 && H % fy == 0 && W % fx == 0, DIQT_E_SHAPE,
                 "cell_wmean: the cell %dx%dx%d does not divide the volume %dx%dx%d", fz, fy, fx, D, H, W);
    const size_t cells = (size_t)(D / fz) * (H / fy) * (W / fx);
    DIQT_REQUIRE((cells + 255) / 256 <= 0x7fffffffu, DIQT_E_SHAPE, "cell_wmean: more than 2^31 - 1 blocks");
    hipLaunchKernelGGL(cell_wmean_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, STREAM, x, table, out, cells, H, W,
                       Cell{fz, fy, fx});
    return check_launch("cell_wmean");
}

extern "C" int diqt_cell_project(const float* x0, const float* meas_up, float* out, size_t cubes, int P, int fz, int fy, int fx,
                                 float weight, float lo, float hi, int clamp_mode, void* stream) {
    DIQT_REQUIRE(x0 && meas_up && out, DIQT_E_ALIGN, "cell_project: null pointer");
    int rc = cell_ok("cell_project", fz, fy, fx, weight);
    if (rc) return rc;
    DIQT_REQUIRE(clamp_mode >= 0 && clamp_mode <= 2, DIQT_E_UNSUPPORTED, "cell_project: clamp_mode %d (0 = min, 1 = box, 2 = none)",
                 clamp_mode);
    DIQT_REQUIRE(cubes > 0 && P > 0 && P % fz == 0 && P % fy == 0 && P % fx == 0, DIQT_E_SHAPE,
                 "cell_project: the cell %dx%dx%d does not divide the %zu cubes of edge %d", fz, fy, fx, cubes, P);
    const size_t cells = cubes * (size_t)(P / fz) * (P / fy) * (P / fx);
    DIQT_REQUIRE((cells + 255) / 256 <= 0x7fffffffu, DIQT_E_SHAPE, "cell_project: more than 2^31 - 1 blocks");
    hipLaunchKernelGGL(cell_project_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, STREAM, x0, meas_up, out, cells, P,
                       Cell{fz, fy, fx}, weight, ProjectClamp{lo, hi, clamp_mode});
    return check_launch("cell_project");
}

extern "C" int diqt_cell_project_profile(const float* x0, const float* meas_up, const float* table, float* out, size_t cubes, int P,
                                         int fz, int fy, int fx, float weight, float lo, float hi, int clamp_mode, void* stream) {
    DIQT_REQUIRE(x0 && meas_up && table && out, DIQT_E_ALIGN, "cell_project_profile: null pointer");
    int rc = cell_ok("cell_project_profile", fz, fy, fx, weight);
    if (rc) return rc;
    DIQT_REQUIRE(clamp_mode >= 0 && clamp_mode <= 2, DIQT_E_UNSUPPORTED,
                 "cell_project_profile: clamp_mode %d (0 = min, 1 = box, 2 = none)", clamp_mode);
    DIQT_REQUIRE(cubes > 0 && P > 0 && P % fz == 0 && P % fy == 0 && P % fx == 0, DIQT_E_SHAPE,
                 "cell_project_profile: the cell %dx%dx%d does not divide the %zu cubes of edge %d", fz, fy, fx, cubes, P);
    const size_t cells = cubes * (size_t)(P / fz) * (P / fy) * (P / fx);
    DIQT_REQUIRE((cells + 255) / 256 <= 0x7fffffffu, DIQT_E_SHAPE, "cell_project_profile: more than 2^31 - 1 blocks");
    hipLaunchKernelGGL(cell_project_profile_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, STREAM, x0, meas_up, table, out,
                       cells, P, Cell{fz, fy, fx}, weight, ProjectClamp{lo, hi, clamp_mode});
    return check_launch("cell_project_profile");
}

extern "C" int diqt_cell_project_noise(const float* x0, const float* meas_up, const float* noise, const float* table, float* out_x0,
                                       float* out_noise, size_t cubes, int P, int fz, int fy, int fx, float weight, float shrink,
                                       float lo, float hi, int clamp_mode, void* stream) {
    DIQT_REQUIRE(x0 && meas_up && noise && out_x0 && out_noise, DIQT_E_ALIGN, "cell_project_noise: null pointer");
    int rc = cell_ok("cell_project_noise", fz, fy, fx, weight);
    if (rc) return rc;
    DIQT_REQUIRE(shrink > 0.f && shrink <= 1.f, DIQT_E_UNSUPPORTED, "cell_project_noise: shrink %g outside (0, 1]", (double)shrink);
    DIQT_REQUIRE(clamp_mode >= 0 && clamp_mode <= 2, DIQT_E_UNSUPPORTED, "cell_project_noise: clamp_mode %d (0 = min, 1 = box, 2 = none)",
                 clamp_mode);
    DIQT_REQUIRE(cubes > 0 && P > 0 && P % fz == 0 && P % fy == 0 && P % fx == 0, DIQT_E_SHAPE,
                 "cell_project_noise: the cell %dx%dx%d does not divide the %zu cubes of edge %d", fz, fy, fx, cubes, P);
    const size_t cells = cubes * (size_t)(P / fz) * (P / fy) * (P / fx);
    DIQT_REQUIRE((cells + 255) / 256 <= 0x7fffffffu, DIQT_E_SHAPE, "cell_project_noise: more than 2^31 - 1 blocks");
    const dim3 grid((unsigned)((cells + 255) / 256));
    if (table)
        hipLaunchKernelGGL(cell_project_noise_kernel<true>, grid, dim3(256), 0, STREAM, x0, meas_up, noise, table, out_x0, out_noise, cells,
                           P, Cell{fz, fy, fx}, weight, shrink, ProjectClamp{lo, hi, clamp_mode});
    else
        hipLaunchKernelGGL(cell_project_noise_kernel<false>, grid, dim3(256), 0, STREAM, x0, meas_up, noise, table, out_x0, out_noise, cells,
                           P, Cell{fz, fy, fx}, weight, shrink, ProjectClamp{lo, hi, clamp_mode});
    return check_launch("cell_project_noise");
}

// diqt_volume_joint_consistent_step and its profile twin: `table` == NULL is the uniform operator (the twin's entry refuses NULL).
// `shaped` is diqt_volume_joint_consistent_noise_step (which has checked `shrink`, the form and kn): the NOISE instantiations and
// their third LDS array; the other entries never look at `shrink`.
// `tile` is diqt_volume_joint_consistent_tile_step: `table` is the n x n projector of a tile operator and the kernel its own.
// `tile_noise` is diqt_volume_joint_consistent_tile_noise_step (which has checked the form and kn): `table` is [2][n][n] = M, G, the
// kernel has four box arrays and looks at neither `weight` nor `shrink`.
static int joint_consistent_launch(const char* who, const float* y, const int* slot, const float* taps, const float* x_t,
                                   const float* x0_prev, const float* meas_up, const float* table, float* x_next, float* x0_out,
                                   int form, int N, int D, int H, int W, int P, int stride, int G0, int G1, int G2, int fz, int fy,
                                   int fx, float weight, float kx, float k0, float kp, float kn, float lo, float hi, int clamp_mode,
                                   unsigned long long seed, unsigned draw, unsigned sample, void* stream, bool shaped = false,
                                   float shrink = 0.f, bool tile = false, bool tile_noise = false) {
    DIQT_REQUIRE(x_t && meas_up && x_next && x0_out && slot && taps && (y || N == 0), DIQT_E_ALIGN, "%s: null pointer", who);
    DIQT_REQUIRE(form >= 0 && form <= 2, DIQT_E_UNSUPPORTED, "%s: form %d (0 = first order, 1 = multistep, 2 = multistep with noise)", who,
                 form);
    int rc = cell_ok(who, fz, fy, fx, weight);
    if (rc) return rc;
    DIQT_REQUIRE(D > 0 && H > 0 && W > 0 && D % fz == 0 && H % fy == 0 && W % fx == 0, DIQT_E_SHAPE,
                 "%s: the cell %dx%dx%d does not divide the volume %dx%dx%d", who, fz, fy, fx, D, H, W);
    JointGrid g;                                       // the shape, lattice and clamp checks of the plain step; the grid is the boxes'
    rc = joint_launch_plan(who, x_next, true, true, N, D, H, W, P, stride, G0, G1, G2, clamp_mode, g);
    if (rc) return rc;
    const Cell c{fz, fy, fx};
    const CellBox b = cell_box(c);
    const size_t n = (size_t)fz * fy * fx;
    const size_t lds = ((size_t)P + (tile_noise ? 4 : shaped ? 3 : 2) * (size_t)fz * b.by * b.bx +
                        (tile_noise ? 2 * n * n : tile ? n * n : table ? 2 * n : 0)) * sizeof(float);
    DIQT_REQUIRE(lds <= 65536, DIQT_E_SHAPE, "%s: P %d needs %zu bytes of LDS", who, P, lds);
    DIQT_REQUIRE((H + b.by - 1) / b.by <= 65535, DIQT_E_SHAPE, "%s: more than 65535 rows of boxes", who);
    // first order: no history; multistep: no normal (and with it no key)
    const bool first = form == 0, noisy = form != 1;
    const dim3 grid((W + b.bx - 1) / b.bx, (H + b.by - 1) / b.by, D / fz);
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, dim3(64, 4), lds, STREAM, y, slot, taps, x_t, first ? nullptr : x0_prev, meas_up, table, x_next,
                           x0_out, N, D, H, W, P, stride, G0, G1, G2, c, weight, kx, k0, first ? 0.f : kp, noisy ? kn : 0.f, lo, hi,
                           clamp_mode, first ? 1 : 0, (unsigned)seed, (unsigned)(seed >> 32), draw, sample, shrink);
    };
    if (tile_noise)
        launch(volume_joint_consistent_tile_noise_kernel);
    else if (tile)
        launch(volume_joint_consistent_tile_kernel);
    else if (shaped)
        table ? launch(volume_joint_consistent_kernel<true, true>) : launch(volume_joint_consistent_kernel<false, true>);
    else
        table ? launch(volume_joint_consistent_kernel<true, false>) : launch(volume_joint_consistent_kernel<false, false>);
    return check_launch(who);
}

extern "C" int diqt_volume_joint_consistent_step(const float* y, const int* slot, const float* taps, const float* x_t,
                                                 const float* x0_prev, const float* meas_up, float* x_next, float* x0_out, int form,
                                                 int N, int D, int H, int W, int P, int stride, int G0, int G1, int G2, int fz, int fy,
                                                 int fx, float weight, float kx, float k0, float kp, float kn, float lo, float hi,
                                                 int clamp_mode, unsigned long long seed, unsigned draw, unsigned sample, void* stream) {
    return joint_consistent_launch("volume_joint_consistent_step", y, slot, taps, x_t, x0_prev, meas_up, nullptr, x_next, x0_out, form, N,
                                   D, H, W, P, stride, G0, G1, G2, fz, fy, fx, weight, kx, k0, kp, kn, lo, hi, clamp_mode, seed, draw,
                                   sample, stream);
}

extern "C" int diqt_volume_joint_consistent_profile_step(const float* y, const int* slot, const float* taps, const float* x_t,
                                                         const float* x0_prev, const float* meas_up, const float* table, float* x_next,
                                                         float* x0_out, int form, int N, int D, int H, int W, int P, int stride, int G0,
                                                         int G1, int G2, int fz, int fy, int fx, float weight, float kx, float k0,
                                                         float kp, float kn, float lo, float hi, int clamp_mode,
                                                         unsigned long long seed, unsigned draw, unsigned sample, void* stream) {
    DIQT_REQUIRE(table, DIQT_E_ALIGN, "volume_joint_consistent_profile_step: null pointer");
    return joint_consistent_launch("volume_joint_consistent_profile_step", y, slot, taps, x_t, x0_prev, meas_up, table, x_next, x0_out,
                                   form, N, D, H, W, P, stride, G0, G1, G2, fz, fy, fx, weight, kx, k0, kp, kn, lo, hi, clamp_mode, seed,
                                   draw, sample, stream);
}

extern "C" int diqt_volume_joint_consistent_noise_step(const float* y, const int* slot, const float* taps, const float* x_t,
                                                       const float* x0_prev, const float* meas_up, const float* table, float* x_next,
                                                       float* x0_out, int form, int N, int D, int H, int W, int P, int stride, int G0,
                                                       int G1, int G2, int fz, int fy, int fx, float weight, float shrink, float kx,
                                                       float k0, float kp, float kn, float lo, float hi, int clamp_mode,
                                                       unsigned long long seed, unsigned draw, unsigned sample, void* stream) {
    const char* who = "volume_joint_consistent_noise_step";
    DIQT_REQUIRE(form == 0 || form == 2, DIQT_E_UNSUPPORTED, "%s: form %d (0 = first order, 2 = multistep with noise: those with a normal)",
                 who, form);
    DIQT_REQUIRE(kn != 0.f, DIQT_E_UNSUPPORTED, "%s: kn == 0, a step without a normal has nothing to shape", who);
    DIQT_REQUIRE(shrink > 0.f && shrink <= 1.f, DIQT_E_UNSUPPORTED, "%s: shrink %g outside (0, 1]", who, (double)shrink);
    return joint_consistent_launch(who, y, slot, taps, x_t, x0_prev, meas_up, table, x_next, x0_out, form, N, D, H, W, P, stride, G0, G1, G2,
                                   fz, fy, fx, weight, kx, k0, kp, kn, lo, hi, clamp_mode, seed, draw, sample, stream, true, shrink);
}

extern "C" int diqt_tile_measure(const float* x, const float* A, float* out, int m, int D, int H, int W, int fz, int fy, int fx,
                                 void* stream) {
    DIQT_REQUIRE(x && A && out, DIQT_E_ALIGN, "tile_measure: null pointer");
    int rc = cell_ok("tile_measure", fz, fy, fx, 1.f);
    if (rc) return rc;
    DIQT_REQUIRE(m >= 1, DIQT_E_SHAPE, "tile_measure: %d rows", m);
    DIQT_REQUIRE(D > 0 && H > 0 && W > 0 && D % fz == 0 && H % fy == 0 && W % fx == 0, DIQT_E_SHAPE,
                 "tile_measure: the cell %dx%dx%d does not divide the volume %dx%dx%d", fz, fy, fx, D, H, W);
    const size_t tiles = (size_t)(D / fz) * (H / fy) * (W / fx);
    DIQT_REQUIRE((tiles * m + 255) / 256 <= 0x7fffffffu, DIQT_E_SHAPE, "tile_measure: more than 2^31 - 1 blocks");
    hipLaunchKernelGGL(tile_measure_kernel, dim3((unsigned)((tiles * m + 255) / 256)), dim3(256), 0, STREAM, x, A, out, tiles, m, H, W,
                       Cell{fz, fy, fx});
    return check_launch("tile_measure");
}

extern "C" int diqt_tile_backproject(const float* y, const float* Ap, float* out, int m, int D, int H, int W, int fz, int fy, int fx,
                                     void* stream) {
    DIQT_REQUIRE(y && Ap && out, DIQT_E_ALIGN, "tile_backproject: null pointer");
    int rc = cell_ok("tile_backproject", fz, fy, fx, 1.f);
    if (rc) return rc;
    DIQT_REQUIRE(m >= 1, DIQT_E_SHAPE, "tile_backproject: %d rows", m);
    DIQT_REQUIRE(D > 0 && H > 0 && W > 0 && D % fz == 0 && H % fy == 0 && W % fx == 0, DIQT_E_SHAPE,
                 "tile_backproject: the cell %dx%dx%d does not divide the volume %dx%dx%d", fz, fy, fx, D, H, W);
    const size_t total = (size_t)D * H * W;
    DIQT_REQUIRE((total + 255) / 256 <= 0x7fffffffu, DIQT_E_SHAPE, "tile_backproject: more than 2^31 - 1 blocks");
    hipLaunchKernelGGL(tile_backproject_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, STREAM, y, Ap, out, total,
                       total / ((size_t)fz * fy * fx), m, H, W, Cell{fz, fy, fx});
    return check_launch("tile_backproject");
}

extern "C" int diqt_tile_project(const float* x0, const float* target, const float* table, float* out, size_t cubes, int P, int fz, int fy,
                                 int fx, float weight, float lo, float hi, int clamp_mode, void* stream) {
    DIQT_REQUIRE(x0 && target && table && out, DIQT_E_ALIGN, "tile_project: null pointer");
    int rc = cell_ok("tile_project", fz, fy, fx, weight);
    if (rc) return rc;
    DIQT_REQUIRE(clamp_mode >= 0 && clamp_mode <= 2, DIQT_E_UNSUPPORTED, "tile_project: clamp_mode %d (0 = min, 1 = box, 2 = none)",
                 clamp_mode);
    DIQT_REQUIRE(cubes > 0 && P > 0 && P % fz == 0 && P % fy == 0 && P % fx == 0, DIQT_E_SHAPE,
                 "tile_project: the cell %dx%dx%d does not divide the %zu cubes of edge %d", fz, fy, fx, cubes, P);
    const Cell c{fz, fy, fx};
    CellBox b = cell_box(c);                           // clipped to the cube: P is a multiple of fy and fx, so the box stays whole tiles
    b.by = b.by < P ? b.by : P;
    b.bx = b.bx < P ? b.bx : P;
    const size_t n = (size_t)fz * fy * fx, lds = ((size_t)fz * b.by * b.bx + n * n) * sizeof(float);
    DIQT_REQUIRE(lds <= 65536, DIQT_E_SHAPE, "tile_project: the cell %dx%dx%d needs %zu bytes of LDS", fz, fy, fx, lds);
    const int gx = (P + b.bx - 1) / b.bx, gy = (P + b.by - 1) / b.by;
    const size_t blocks = (size_t)gx * gy * (cubes * (size_t)(P / fz));
    DIQT_REQUIRE(blocks <= 0x7fffffffu, DIQT_E_SHAPE, "tile_project: more than 2^31 - 1 blocks");
    hipLaunchKernelGGL(tile_project_kernel, dim3((unsigned)blocks), dim3(256), lds, STREAM, x0, target, table, out, P, P, gx, gy, c, b,
                       weight, ProjectClamp{lo, hi, clamp_mode});
    return check_launch("tile_project");
}

extern "C" int diqt_volume_joint_consistent_tile_step(const float* y, const int* slot, const float* taps, const float* x_t,
                                                      const float* x0_prev, const float* meas_up, const float* table, float* x_next,
                                                      float* x0_out, int form, int N, int D, int H, int W, int P, int stride, int G0,
                                                      int G1, int G2, int fz, int fy, int fx, float weight, float kx, float k0, float kp,
                                                      float kn, float lo, float hi, int clamp_mode, unsigned long long seed,
                                                      unsigned draw, unsigned sample, void* stream) {
    DIQT_REQUIRE(table, DIQT_E_ALIGN, "volume_joint_consistent_tile_step: null pointer");
    return joint_consistent_launch("volume_joint_consistent_tile_step", y, slot, taps, x_t, x0_prev, meas_up, table, x_next, x0_out, form,
                                   N, D, H, W, P, stride, G0, G1, G2, fz, fy, fx, weight, kx, k0, kp, kn, lo, hi, clamp_mode, seed, draw,
                                   sample, stream, false, 0.f, true);
}

extern "C" int diqt_tile_project_noise(const float* x0, const float* target, const float* noise, const float* tables, float* out,
                                       float* out_noise, size_t cubes, int P, int fz, int fy, int fx, float lo, float hi, int clamp_mode,
                                       void* stream) {
    DIQT_REQUIRE(x0 && target && noise && tables && out && out_noise, DIQT_E_ALIGN, "tile_project_noise: null pointer");
    int rc = cell_ok("tile_project_noise", fz, fy, fx, 1.f);
    if (rc) return rc;
    DIQT_REQUIRE(clamp_mode >= 0 && clamp_mode <= 2, DIQT_E_UNSUPPORTED, "tile_project_noise: clamp_mode %d (0 = min, 1 = box, 2 = none)",
                 clamp_mode);
    DIQT_REQUIRE(cubes > 0 && P > 0 && P % fz == 0 && P % fy == 0 && P % fx == 0, DIQT_E_SHAPE,
                 "tile_project_noise: the cell %dx%dx%d does not divide the %zu cubes of edge %d", fz, fy, fx, cubes, P);
    const Cell c{fz, fy, fx};
    CellBox b = cell_box(c);                           // clipped to the cube, as diqt_tile_project does
    b.by = b.by < P ? b.by : P;
    b.bx = b.bx < P ? b.bx : P;
    const size_t n = (size_t)fz * fy * fx, lds = (3 * (size_t)fz * b.by * b.bx + 2 * n * n) * sizeof(float);
    DIQT_REQUIRE(lds <= 65536, DIQT_E_SHAPE, "tile_project_noise: the cell %dx%dx%d needs %zu bytes of LDS", fz, fy, fx, lds);
    const int gx = (P + b.bx - 1) / b.bx, gy = (P + b.by - 1) / b.by;
    const size_t blocks = (size_t)gx * gy * (cubes * (size_t)(P / fz));
    DIQT_REQUIRE(blocks <= 0x7fffffffu, DIQT_E_SHAPE, "tile_project_noise: more than 2^31 - 1 blocks");
    hipLaunchKernelGGL(tile_project_noise_kernel, dim3((unsigned)blocks), dim3(256), lds, STREAM, x0, target, noise, tables, out,
                       out_noise, P, P, gx, gy, c, b, ProjectClamp{lo, hi, clamp_mode});
    return check_launch("tile_project_noise");
}

extern "C" int diqt_volume_joint_consistent_tile_noise_step(const float* y, const int* slot, const float* taps, const float* x_t,
                                                            const float* x0_prev, const float* meas_up, const float* tables,
                                                            float* x_next, float* x0_out, int form, int N, int D, int H, int W, int P,
                                                            int stride, int G0, int G1, int G2, int fz, int fy, int fx, float kx, float k0,
                                                            float kp, float kn, float lo, float hi, int clamp_mode,
                                                            unsigned long long seed, unsigned draw, unsigned sample, void* stream) {
    const char* who = "volume_joint_consistent_tile_noise_step";
    DIQT_REQUIRE(tables, DIQT_E_ALIGN, "%s: null pointer", who);
    DIQT_REQUIRE(form == 0 || form == 2, DIQT_E_UNSUPPORTED, "%s: form %d (0 = first order, 2 = multistep with noise: those with a normal)",
                 who, form);
    DIQT_REQUIRE(kn != 0.f, DIQT_E_UNSUPPORTED, "%s: kn == 0, a step without a normal has nothing to shape", who);
    return joint_consistent_launch(who, y, slot, taps, x_t, x0_prev, meas_up, tables, x_next, x0_out, form, N, D, H, W, P, stride, G0, G1,
                                   G2, fz, fy, fx, 1.f, kx, k0, kp, kn, lo, hi, clamp_mode, seed, draw, sample, stream, false, 0.f, false,
                                   true);
}

// The cell, the reach and the table length of the slab entries: cell_ok's rules, 1 <= r, 2r <= fz and jmax >= 1.
static int slab_ok(const char* who, int fz, int fy, int fx, int r, int jmax, float w) {
    int rc = cell_ok(who, fz, fy, fx, w);
    if (rc) return rc;
    DIQT_REQUIRE(r >= 1 && 2 * r <= fz, DIQT_E_UNSUPPORTED, "%s: reach %d (1 <= r and 2r <= fz = %d)", who, r, fz);
    DIQT_REQUIRE(jmax >= 1, DIQT_E_UNSUPPORTED, "%s: a table of %d run positions", who, jmax);
    return DIQT_OK;
}

extern "C" int diqt_slab_measure(const float* x, const float* table, float* out, int D, int H, int W, int fz, int fy, int fx, int r,
                                 int jmax, void* stream) {
    DIQT_REQUIRE(x && table && out, DIQT_E_ALIGN, "slab_measure: null pointer");
    int rc = slab_ok("slab_measure", fz, fy, fx, r, jmax, 1.f);
    if (rc) return rc;
    DIQT_REQUIRE(D > 0 && H > 0 && W > 0 && D % fz == 0 && H % fy == 0 && W % fx == 0, DIQT_E_SHAPE,
                 "slab_measure: the cell %dx%dx%d does not divide the volume %dx%dx%d", fz, fy, fx, D, H, W);
    const size_t rows = (size_t)(D / fz) * (H / fy) * (W / fx);
    DIQT_REQUIRE((rows + 255) / 256 <= 0x7fffffffu, DIQT_E_SHAPE, "slab_measure: more than 2^31 - 1 blocks");
    hipLaunchKernelGGL(slab_measure_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, STREAM, x, table, out, rows, D, H, W,
                       Slab{fz, fy, fx, r, jmax});
    return check_launch("slab_measure");
}

extern "C" int diqt_slab_project(const float* x0, const float* meas_up, const float* table, float* out, size_t cubes, int P, int fz,
                                 int fy, int fx, int r, int jmax, float weight, float lo, float hi, int clamp_mode, void* stream) {
    DIQT_REQUIRE(x0 && meas_up && table && out, DIQT_E_ALIGN, "slab_project: null pointer");
    int rc = slab_ok("slab_project", fz, fy, fx, r, jmax, weight);
    if (rc) return rc;
    DIQT_REQUIRE(clamp_mode >= 0 && clamp_mode <= 2, DIQT_E_UNSUPPORTED, "slab_project: clamp_mode %d (0 = min, 1 = box, 2 = none)",
                 clamp_mode);
    DIQT_REQUIRE(cubes > 0 && P > 0 && P % fz == 0 && P % fy == 0 && P % fx == 0, DIQT_E_SHAPE,
                 "slab_project: the cell %dx%dx%d does not divide the %zu cubes of edge %d", fz, fy, fx, cubes, P);
    const int S = P / fz;
    DIQT_REQUIRE(jmax >= S, DIQT_E_SHAPE, "slab_project: the table has %d run positions, a cube has %d slices", jmax, S);
    const size_t lds = (size_t)S * 256 * sizeof(float);
    DIQT_REQUIRE(lds <= 65536, DIQT_E_SHAPE, "slab_project: %d slices need %zu bytes of LDS", S, lds);
    const size_t cols = cubes * (size_t)(P / fy) * (P / fx);
    DIQT_REQUIRE((cols + 255) / 256 <= 0x7fffffffu, DIQT_E_SHAPE, "slab_project: more than 2^31 - 1 blocks");
    hipLaunchKernelGGL(slab_project_kernel, dim3((unsigned)((cols + 255) / 256)), dim3(256), lds, STREAM, x0, meas_up, table, out, cols, P,
                       Slab{fz, fy, fx, r, jmax}, weight, ProjectClamp{lo, hi, clamp_mode});
    return check_launch("slab_project");
}

// The workspace of the two joint slab entries, in floats: pm [D][ch][cw], covered [D][ch][cw], then the run positions [D / fz][ch][cw].
static size_t slab_workspace_floats(int D, int H, int W, int fz, int fy, int fx) {
    return (size_t)(2 * (size_t)D + D / fz) * (H / fy) * (W / fx);
}
static int joint_slab_ok(const char* who, int D, int H, int W, int fz, int fy, int fx, int jmax, size_t workspace_floats) {
    DIQT_REQUIRE(D > 0 && H > 0 && W > 0 && D % fz == 0 && H % fy == 0 && W % fx == 0, DIQT_E_SHAPE,
                 "%s: the cell %dx%dx%d does not divide the volume %dx%dx%d", who, fz, fy, fx, D, H, W);
    DIQT_REQUIRE(jmax >= D / fz, DIQT_E_SHAPE, "%s: the table has %d run positions, the volume has %d slices", who, jmax, D / fz);
    DIQT_REQUIRE(workspace_floats >= slab_workspace_floats(D, H, W, fz, fy, fx), DIQT_E_SHAPE, "%s: the workspace holds %zu floats, %zu needed",
                 who, workspace_floats, slab_workspace_floats(D, H, W, fz, fy, fx));
    return DIQT_OK;
}

extern "C" int diqt_volume_joint_slab_coeffs(const float* y, const int* slot, const float* taps, const float* meas_up, const float* table,
                                             float* workspace, size_t workspace_floats, float* coef, int N, int D, int H, int W, int P,
                                             int stride, int G0, int G1, int G2, int fz, int fy, int fx, int r, int jmax, float lo,
                                             float hi, int clamp_mode, void* stream) {
    const char* who = "volume_joint_slab_coeffs";
    DIQT_REQUIRE(meas_up && table && workspace && coef && slot && taps && (y || N == 0), DIQT_E_ALIGN, "%s: null pointer", who);
    int rc = slab_ok(who, fz, fy, fx, r, jmax, 1.f);
    if (rc) return rc;
    JointGrid g;
    rc = joint_launch_plan(who, coef, true, true, N, D, H, W, P, stride, G0, G1, G2, clamp_mode, g);
    if (rc) return rc;
    rc = joint_slab_ok(who, D, H, W, fz, fy, fx, jmax, workspace_floats);
    if (rc) return rc;
    const int cw = W / fx, ch = H / fy;
    const size_t cols = (size_t)cw * ch, planes = (size_t)D * cols;
    DIQT_REQUIRE((cols + 63) / 64 <= 0x7fffffffu, DIQT_E_SHAPE, "%s: more than 2^31 - 1 blocks", who);
    const Slab sl{fz, fy, fx, r, jmax};
    const CellBox b = cell_box(Cell{1, fy, fx});
    const size_t lds = ((size_t)P + 2 * (size_t)b.by * b.bx) * sizeof(float);
    DIQT_REQUIRE(lds <= 65536, DIQT_E_SHAPE, "%s: P %d needs %zu bytes of LDS", who, P, lds);
    DIQT_REQUIRE((H + b.by - 1) / b.by <= 65535, DIQT_E_SHAPE, "%s: more than 65535 rows of boxes", who);
    hipLaunchKernelGGL(volume_joint_slab_planes_kernel, dim3((W + b.bx - 1) / b.bx, (H + b.by - 1) / b.by, D), dim3(64, 4), lds, STREAM, y,
                       slot, taps, table, workspace, workspace + planes, N, D, H, W, P, stride, G0, G1, G2, sl, lo, hi, clamp_mode);
    rc = check_launch(who);
    if (rc) return rc;
    hipLaunchKernelGGL(volume_joint_slab_solve_kernel, dim3((unsigned)((cols + 63) / 64)), dim3(64, 4), 0, STREAM, workspace,
                       workspace + planes, meas_up, table, coef, workspace + 2 * planes, cols, D, H, W, sl);
    return check_launch(who);
}

extern "C" int diqt_volume_joint_consistent_slab_step(const float* y, const int* slot, const float* taps, const float* x_t,
                                                      const float* x0_prev, const float* table, const float* coef, const float* workspace,
                                                      size_t workspace_floats, float* x_next, float* x0_out, int form, int N, int D, int H,
                                                      int W, int P, int stride, int G0, int G1, int G2, int fz, int fy, int fx, int r,
                                                      int jmax, float weight, float kx, float k0, float kp, float kn, float lo, float hi,
                                                      int clamp_mode, unsigned long long seed, unsigned draw, unsigned sample,
                                                      void* stream) {
    const char* who = "volume_joint_consistent_slab_step";
    DIQT_REQUIRE(x_t && table && coef && workspace && x_next && x0_out && slot && taps && (y || N == 0), DIQT_E_ALIGN, "%s: null pointer",
                 who);
    DIQT_REQUIRE(form >= 0 && form <= 2, DIQT_E_UNSUPPORTED, "%s: form %d (0 = first order, 1 = multistep, 2 = multistep with noise)", who,
                 form);
    int rc = slab_ok(who, fz, fy, fx, r, jmax, weight);
    if (rc) return rc;
    JointGrid g;
    rc = joint_launch_plan(who, x_next, true, true, N, D, H, W, P, stride, G0, G1, G2, clamp_mode, g);
    if (rc) return rc;
    rc = joint_slab_ok(who, D, H, W, fz, fy, fx, jmax, workspace_floats);
    if (rc) return rc;
    // first order: no history; multistep: no normal (and with it no key)
    const bool first = form == 0, noisy = form != 1;
    const size_t planes = (size_t)D * (H / fy) * (W / fx);
    hipLaunchKernelGGL(volume_joint_slab_kernel, g.grid, dim3(64, 4), g.lds, STREAM, y, slot, taps, x_t, first ? nullptr : x0_prev, table,
                       coef, workspace + 2 * planes, x_next, x0_out, N, D, H, W, P, stride, G0, G1, G2, Slab{fz, fy, fx, r, jmax}, weight,
                       kx, k0, first ? 0.f : kp, noisy ? kn : 0.f, lo, hi, clamp_mode, first ? 1 : 0, (unsigned)seed,
                       (unsigned)(seed >> 32), draw, sample);
    return check_launch(who);
}

// ---- the band operator's entries ----------------------------------------------------------------------------------------------------------
// The LDS of one band_pass_kernel launch on an axis of N voxels: the padded doubled table and one panel.
static size_t band_lds(int N) { return ((size_t)2 * N + 2 * BAND_PAD + (size_t)BAND_J * (BAND_C + 1)) * sizeof(float); }
// The domain, the cell and the active axes of the band entries: every axis 1 .. BAND_MAX_N voxels and a multiple of its factor, `active`
// a mask of bits 0 (z), 1 (y), 2 (x) with at least one set, and an axis outside it has factor 1.
static int band_ok(const char* who, const int* n, const int* f, int active) {
    DIQT_REQUIRE(active >= 1 && active <= 7, DIQT_E_UNSUPPORTED, "%s: active axes %d (a mask of z = 1, y = 2, x = 4, not empty)", who, active);
    for (int a = 0; a < 3; ++a) {
        DIQT_REQUIRE(f[a] >= 1 && (((active >> a) & 1) || f[a] == 1), DIQT_E_UNSUPPORTED, "%s: axis %d has factor %d and is not active", who,
                     a, f[a]);
        DIQT_REQUIRE(n[a] > 0 && n[a] % f[a] == 0, DIQT_E_SHAPE, "%s: the factor %d does not divide the %d voxels of axis %d", who, f[a], n[a],
                     a);
        DIQT_REQUIRE(n[a] <= BAND_MAX_N, DIQT_E_SHAPE, "%s: axis %d has %d voxels, above the %d a band pass takes", who, a, n[a], BAND_MAX_N);
        DIQT_REQUIRE(band_lds(n[a]) <= 65536, DIQT_E_SHAPE, "%s: axis %d needs %zu bytes of LDS", who, a, band_lds(n[a]));
    }
    return DIQT_OK;
}
// One pass: the array is [O][Nin][I] -> [O][Nout][I], T the table of the axis (N floats).
template <class Load, class Store>
static int band_pass(const char* who, const float* T, size_t O, int Nin, int Nout, size_t I, int N, int si, int sj, bool slide, Load load,
                     Store store, void* stream) {
    const size_t C = O * I, bx = (C + BAND_C - 1) / BAND_C;
    DIQT_REQUIRE(bx <= 0x7fffffffu && I <= 0x7fffffffu, DIQT_E_SHAPE, "%s: more than 2^31 - 1 blocks", who);
    const dim3 grid((unsigned)bx, (Nout + BAND_I - 1) / BAND_I);
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, dim3(64, 4), band_lds(N), STREAM, T, C, (int)I, Nin, Nout, N, si, sj, load, store);
    };
    if (I == 1)
        slide ? launch(band_pass_kernel<true, true, Load, Store>) : launch(band_pass_kernel<true, false, Load, Store>);
    else
        slide ? launch(band_pass_kernel<false, true, Load, Store>) : launch(band_pass_kernel<false, false, Load, Store>);
    return check_launch(who);
}
// The table of axis `a` in the flat table: 0 = d, 1 = a, 2 = g.
static const float* band_axis_table(const float* table, const int* n, int a, int which) {
    size_t off = 0;
    for (int b = 0; b < a; ++b) off += 3 * (size_t)n[b];
    return table + off + (size_t)which * n[a];
}
// The rectangular passes of A (`forward`: z, y, x, each axis N -> N / f) or A+ (x, y, z, each N / f -> N) from `x` to `out` through the two
// halves of the workspace.  `plan_only`: only `need`, the floats of workspace the passes use, is computed.
static int band_rect(const char* who, bool forward, const float* x, const float* table, float* out, float* workspace,
                     size_t workspace_floats, const int* n, const int* f, int active, bool plan_only, size_t& need, void* stream) {
    int dims[3], order[3], passes = 0;
    for (int a = 0; a < 3; ++a) {
        dims[a] = forward ? n[a] : n[a] / f[a];
        if ((active >> a) & 1) ++passes;
    }
    for (int p = 0; p < 3; ++p) order[p] = forward ? p : 2 - p;
    size_t half = 0;
    for (int round = 0; round < 2; ++round) {          // 0: the size of an intermediate; 1: the launches
        if (round == 1) {
            need = passes > 1 ? 2 * half : 0;
            if (plan_only) return DIQT_OK;
            DIQT_REQUIRE(passes == 1 || (workspace && workspace_floats >= need), DIQT_E_SHAPE, "%s: the workspace holds %zu floats, %zu needed",
                         who, workspace ? workspace_floats : (size_t)0, need);
            for (int a = 0; a < 3; ++a) dims[a] = forward ? n[a] : n[a] / f[a];
        }
        const float* src = x;
        for (int p = 0, done = 0; p < 3; ++p) {
            const int a = order[p];
            if (!((active >> a) & 1)) continue;
            const int Nin = dims[a], Nout = forward ? n[a] / f[a] : n[a];
            dims[a] = Nout;
            const size_t total = (size_t)dims[0] * dims[1] * dims[2];
            ++done;
            if (round == 0) {
                if (done < passes) half = total > half ? total : half;
                continue;
            }
            float* dst = done == passes ? out : workspace + (done % 2) * half;
            size_t O = 1, I = 1;
            for (int b = 0; b < a; ++b) O *= dims[b];
            for (int b = a + 1; b < 3; ++b) I *= dims[b];
            int rc = band_pass(who, band_axis_table(table, n, a, forward ? 1 : 2), O, Nin, Nout, I, n[a], forward ? f[a] : -1,
                               forward ? -1 : f[a], false, BandLoad{src}, BandStore{dst}, stream);
            if (rc) return rc;
            src = dst;
        }
    }
    return DIQT_OK;
}

extern "C" int diqt_band_measure(const float* x, const float* table, float* out, float* workspace, size_t workspace_floats, int D, int H,
                                 int W, int fz, int fy, int fx, int active, void* stream) {
    DIQT_REQUIRE(x && table && out, DIQT_E_ALIGN, "band_measure: null pointer");
    const int n[3] = {D, H, W}, f[3] = {fz, fy, fx};
    int rc = band_ok("band_measure", n, f, active);
    if (rc) return rc;
    size_t need;
    return band_rect("band_measure", true, x, table, out, workspace, workspace_floats, n, f, active, false, need, stream);
}

extern "C" int diqt_band_backproject(const float* y, const float* table, float* out, float* workspace, size_t workspace_floats, int D,
                                     int H, int W, int fz, int fy, int fx, int active, void* stream) {
    DIQT_REQUIRE(y && table && out, DIQT_E_ALIGN, "band_backproject: null pointer");
    const int n[3] = {D, H, W}, f[3] = {fz, fy, fx};
    int rc = band_ok("band_backproject", n, f, active);
    if (rc) return rc;
    size_t need;
    return band_rect("band_backproject", false, y, table, out, workspace, workspace_floats, n, f, active, false, need, stream);
}

// The projector passes z, y, x over `batch` domains [n0][n1][n2]: x -> out through `ws0` / `ws1` (each batch n0 n1 n2 floats; ws1 is
// looked at only with three active axes).  `project`: the first loader forms t - clamp(x0) from (x = x0, t) and the result is
// out = fmaf(w, c, clamp(x0)), where out may alias x0: formed in the last storer, or with one active axis by band_shift_kernel.
static int band_square(const char* who, const float* x, const float* t, const float* table, float* out, float* ws0, float* ws1,
                       size_t batch, const int* n, int active, bool project, float w, ProjectClamp clamp, void* stream) {
    int passes = 0, done = 0;
    for (int a = 0; a < 3; ++a) passes += (active >> a) & 1;
    const size_t total = batch * n[0] * n[1] * n[2];
    // the chain of buffers: project x0 -> ws0 [-> ws1] -> out (one pass: x0 -> ws0, then the shift); apply x -> [out -> ws0 ->] out
    const float* src = x;
    for (int a = 0; a < 3; ++a) {
        if (!((active >> a) & 1)) continue;
        ++done;
        const bool first = done == 1, last = done == passes;
        float* dst = project ? (last && passes > 1 ? out : done == 1 ? ws0 : ws1) : (last ? out : passes - done == 2 ? out : ws0);
        size_t O = batch, I = 1;
        for (int b = 0; b < a; ++b) O *= n[b];
        for (int b = a + 1; b < 3; ++b) I *= n[b];
        const float* T = band_axis_table(table, n, a, 0);
        int rc;
        if (project && first)
            rc = band_pass(who, T, O, n[a], n[a], I, n[a], 1, -1, true, BandResidualLoad{t, x, clamp}, BandStore{dst}, stream);
        else if (project && last)
            rc = band_pass(who, T, O, n[a], n[a], I, n[a], 1, -1, true, BandLoad{src}, BandShiftStore{x, out, w, clamp}, stream);
        else
            rc = band_pass(who, T, O, n[a], n[a], I, n[a], 1, -1, true, BandLoad{src}, BandStore{dst}, stream);
        if (rc) return rc;
        src = dst;
    }
    if (project && passes == 1) {
        DIQT_REQUIRE((total + 255) / 256 <= 0x7fffffffu, DIQT_E_SHAPE, "%s: more than 2^31 - 1 blocks", who);
        hipLaunchKernelGGL(band_shift_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, STREAM, x, ws0, out, total, w, clamp);
        return check_launch(who);
    }
    return DIQT_OK;
}

extern "C" int diqt_band_project(const float* x0, const float* target, const float* table, float* workspace, float* out, size_t cubes,
                                 int P, int fz, int fy, int fx, size_t workspace_floats, int active, float weight, float lo, float hi,
                                 int clamp_mode, void* stream) {
    const char* who = "band_project";
    DIQT_REQUIRE(x0 && target && table && workspace && out, DIQT_E_ALIGN, "%s: null pointer", who);
    int rc = cell_ok(who, fz, fy, fx, weight);
    if (rc) return rc;
    DIQT_REQUIRE(clamp_mode >= 0 && clamp_mode <= 2, DIQT_E_UNSUPPORTED, "%s: clamp_mode %d (0 = min, 1 = box, 2 = none)", who, clamp_mode);
    const int n[3] = {P, P, P}, f[3] = {fz, fy, fx};
    DIQT_REQUIRE(cubes > 0 && P > 0, DIQT_E_SHAPE, "%s: %zu cubes of edge %d", who, cubes, P);
    rc = band_ok(who, n, f, active);
    if (rc) return rc;
    const size_t total = cubes * (size_t)P * P * P;
    DIQT_REQUIRE(workspace_floats >= 2 * total, DIQT_E_SHAPE, "%s: the workspace holds %zu floats, %zu needed", who, workspace_floats,
                 2 * total);
    DIQT_REQUIRE(workspace != out && workspace != x0 && workspace + total != out && workspace + total != x0, DIQT_E_ALIGN,
                 "%s: the workspace may alias neither x0 nor out", who);
    return band_square(who, x0, target, table, out, workspace, workspace + total, cubes, n, active, true, weight,
                       ProjectClamp{lo, hi, clamp_mode}, stream);
}

extern "C" int diqt_band_apply(const float* x, const float* table, float* out, float* workspace, size_t workspace_floats, int D, int H,
                               int W, int active, void* stream) {
    const char* who = "band_apply";
    DIQT_REQUIRE(x && table && out && workspace, DIQT_E_ALIGN, "%s: null pointer", who);
    DIQT_REQUIRE(x != out && x != workspace && out != workspace, DIQT_E_ALIGN, "%s: x, out and the workspace must be three volumes", who);
    const int n[3] = {D, H, W}, f[3] = {1, 1, 1};
    int rc = band_ok(who, n, f, 7);                    // the shape rules; the factors are not this entry's
    if (rc) return rc;
    DIQT_REQUIRE(active >= 1 && active <= 7, DIQT_E_UNSUPPORTED, "%s: active axes %d (a mask of z = 1, y = 2, x = 4, not empty)", who, active);
    const size_t total = (size_t)D * H * W;
    DIQT_REQUIRE(workspace_floats >= total, DIQT_E_SHAPE, "%s: the workspace holds %zu floats, %zu needed", who, workspace_floats, total);
    return band_square(who, x, nullptr, table, out, workspace, nullptr, 1, n, active, false, 0.f, ProjectClamp{0.f, 0.f, 2}, stream);
}

extern "C" int diqt_volume_joint_band_residual(const float* y, const int* slot, const float* taps, const float* target, float* a_out,
                                               float* covered_out, float* r_out, int N, int D, int H, int W, int P, int stride, int G0,
                                               int G1, int G2, float lo, float hi, int clamp_mode, void* stream) {
    const char* who = "volume_joint_band_residual";
    DIQT_REQUIRE(target && a_out && covered_out && r_out && slot && taps && (y || N == 0), DIQT_E_ALIGN, "%s: null pointer", who);
    JointGrid g;
    int rc = joint_launch_plan(who, a_out, true, true, N, D, H, W, P, stride, G0, G1, G2, clamp_mode, g);
    if (rc) return rc;
    hipLaunchKernelGGL(volume_joint_band_residual_kernel, g.grid, dim3(64, 4), g.lds, STREAM, y, slot, taps, target, a_out, covered_out,
                       r_out, N, D, H, W, P, stride, G0, G1, G2, lo, hi, clamp_mode);
    return check_launch(who);
}

extern "C" int diqt_volume_joint_consistent_band_step(const float* y, const int* slot, const float* taps, const float* x_t,
                                                      const float* x0_prev, const float* a, const float* covered, const float* c,
                                                      float* x_next, float* x0_out, int form, int N, int D, int H, int W, int P,
                                                      int stride, int G0, int G1, int G2, int fz, int fy, int fx, float weight, float kx,
                                                      float k0, float kp, float kn, float lo, float hi, int clamp_mode,
                                                      unsigned long long seed, unsigned draw, unsigned sample, void* stream) {
    const char* who = "volume_joint_consistent_band_step";
    DIQT_REQUIRE(x_t && a && covered && c && x_next && x0_out, DIQT_E_ALIGN, "%s: null pointer", who);
    DIQT_REQUIRE(form >= 0 && form <= 2, DIQT_E_UNSUPPORTED, "%s: form %d (0 = first order, 1 = multistep, 2 = multistep with noise)", who,
                 form);
    int rc = cell_ok(who, fz, fy, fx, weight);
    if (rc) return rc;
    JointGrid g;                                       // the windows are not walked: y, slot, taps, the lattice and the clamp are not looked at
    rc = joint_launch_plan(who, x_next, false, true, N, D, H, W, P, stride, G0, G1, G2, clamp_mode, g);
    if (rc) return rc;
    const bool first = form == 0, noisy = form != 1;
    hipLaunchKernelGGL(volume_joint_band_kernel, g.grid, dim3(64, 4), 0, STREAM, x_t, first ? nullptr : x0_prev, a, covered, c, x_next,
                       x0_out, H, W, weight, kx, k0, first ? 0.f : kp, noisy ? kn : 0.f, first ? 1 : 0, (unsigned)seed,
                       (unsigned)(seed >> 32), draw, sample);
    return check_launch(who);
}

extern "C" int diqt_volume_joint_heun(const float* y, const int* slot, const float* taps, float* xh, float* xn, float* x0, int phase, int N,
                                      int D, int H, int W, int P, int stride, int G0, int G1, int G2, float a, float b, float c, float d,
                                      float kc, float lo, float hi, int clamp_mode, unsigned long long seed, unsigned draw,
                                      unsigned sample, void* stream) {
    DIQT_REQUIRE(phase >= 0 && phase <= 2, DIQT_E_UNSUPPORTED, "volume_joint_heun: phase %d (0 = init, 1 = predictor, 2 = corrector)",
                 phase);
    JointGrid g;
    int rc = joint_launch_plan("volume_joint_heun", xh, phase != 0, xn && x0 && slot && taps && (y || N == 0), N, D, H, W, P, stride, G0,
                               G1, G2, clamp_mode, g);
    if (rc) return rc;
    DIQT_REQUIRE(phase != 0 || draw != 0xffffffffu, DIQT_E_SHAPE, "volume_joint_heun: phase 0 uses draw and draw + 1");
    hipLaunchKernelGGL(volume_joint_heun_kernel, g.grid, dim3(64, 4), g.lds, STREAM, y, slot, taps, xh, xn, x0, phase, N, D, H, W, P, stride,
                       G0, G1, G2, a, b, c, d, kc, lo, hi, clamp_mode, (unsigned)seed, (unsigned)(seed >> 32), draw, sample);
    return check_launch("volume_joint_heun");
}

extern "C" int diqt_volume_joint_consistent_heun(const float* y, const int* slot, const float* taps, float* xh, float* xn, float* x0,
                                                 const float* meas_up, const float* table, int phase, int mode, int N, int D, int H,
                                                 int W, int P, int stride, int G0, int G1, int G2, int fz, int fy, int fx, float weight,
                                                 float a, float b, float c, float d, float kc, float lo, float hi, int clamp_mode,
                                                 unsigned long long seed, unsigned draw, unsigned sample, void* stream) {
    const char* who = "volume_joint_consistent_heun";
    DIQT_REQUIRE(phase == 1 || phase == 2, DIQT_E_UNSUPPORTED,
                 "%s: phase %d (1 = predictor, 2 = corrector; the init is volume_joint_heun's)", who, phase);
    DIQT_REQUIRE(mode >= 0 && mode <= 2, DIQT_E_UNSUPPORTED, "%s: mode %d (0 = uniform, 1 = profile, 2 = tile operator)", who, mode);
    DIQT_REQUIRE(xh && xn && x0 && meas_up && (table || mode == 0) && slot && taps && (y || N == 0), DIQT_E_ALIGN, "%s: null pointer", who);
    int rc = cell_ok(who, fz, fy, fx, weight);
    if (rc) return rc;
    DIQT_REQUIRE(D > 0 && H > 0 && W > 0 && D % fz == 0 && H % fy == 0 && W % fx == 0, DIQT_E_SHAPE,
                 "%s: the cell %dx%dx%d does not divide the volume %dx%dx%d", who, fz, fy, fx, D, H, W);
    JointGrid g;                                       // the shape, lattice and clamp checks of the plain launch; the grid is the boxes'
    rc = joint_launch_plan(who, xh, true, true, N, D, H, W, P, stride, G0, G1, G2, clamp_mode, g);
    if (rc) return rc;
    const Cell cell{fz, fy, fx};
    const CellBox box = cell_box(cell);
    const size_t n = (size_t)fz * fy * fx;
    const size_t lds = ((size_t)P + 2 * (size_t)fz * box.by * box.bx + (mode == 2 ? n * n : mode == 1 ? 2 * n : 0)) * sizeof(float);
    DIQT_REQUIRE(lds <= 65536, DIQT_E_SHAPE, "%s: P %d needs %zu bytes of LDS", who, P, lds);
    DIQT_REQUIRE((H + box.by - 1) / box.by <= 65535, DIQT_E_SHAPE, "%s: more than 65535 rows of boxes", who);
    const dim3 grid((W + box.bx - 1) / box.bx, (H + box.by - 1) / box.by, D / fz);
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, dim3(64, 4), lds, STREAM, y, slot, taps, xh, xn, x0, meas_up, table, phase, N, D, H, W, P, stride,
                           G0, G1, G2, cell, weight, a, b, c, d, phase == 2 ? kc : 0.f, lo, hi, clamp_mode, (unsigned)seed,
                           (unsigned)(seed >> 32), draw, sample);
    };
    if (mode == 2)
        launch(volume_joint_consistent_heun_kernel<2>);
    else if (mode == 1)
        launch(volume_joint_consistent_heun_kernel<1>);
    else
        launch(volume_joint_consistent_heun_kernel<0>);
    return check_launch(who);
}

extern "C" int diqt_edm_inpaint_churn(const float* x, const float* renoise, const float* known, const unsigned char* mask,
                                      const float* eps, const float* kr, const float* kc, float* out, int B, size_t per_batch,
                                      void* stream) {
    DIQT_REQUIRE(x && known && mask && eps && kc && out && (kr || !renoise), DIQT_E_ALIGN, "edm_inpaint_churn: null pointer");
    DIQT_REQUIRE(B > 0 && per_batch > 0, DIQT_E_SHAPE, "edm_inpaint_churn: bad shape (B %d, per_batch %zu)", B, per_batch);
    DIQT_REQUIRE(B <= 65535 && (per_batch + 255) / 256 <= 0x7fffffffu, DIQT_E_SHAPE,
                 "edm_inpaint_churn: more than 65535 samples or 2^31 - 1 blocks per sample");
    hipLaunchKernelGGL(edm_inpaint_churn_kernel, dim3((unsigned)((per_batch + 255) / 256), B), dim3(64, 4), 0, STREAM, x, renoise, known,
                       mask, eps, kr, kc, out, per_batch);
    return check_launch("edm_inpaint_churn");
}

extern "C" int diqt_volume_joint_heun_inpaint(const float* y, const int* slot, const float* taps, float* xh, const float* xn, float* x0,
                                              const float* known, const unsigned char* mask, int phase, int N, int D, int H, int W,
                                              int P, int stride, int G0, int G1, int G2, float a, float b, float c, float d, float kr,
                                              float kc, float lo, float hi, int clamp_mode, unsigned long long seed, unsigned draw,
                                              unsigned draw_r, unsigned sample, void* stream) {
    DIQT_REQUIRE(phase == 0 || phase == 2 || phase == 3, DIQT_E_UNSUPPORTED,
                 "volume_joint_heun_inpaint: phase %d (0 = init, 2 = corrector, 3 = re-churn; the predictor is volume_joint_heun's)", phase);
    DIQT_REQUIRE(known && mask && (phase != 3 || xn), DIQT_E_ALIGN, "volume_joint_heun_inpaint: null pointer");
    JointGrid g;
    int rc = joint_launch_plan("volume_joint_heun_inpaint", xh, phase == 2, xn && x0 && slot && taps && (y || N == 0), N, D, H, W, P,
                               stride, G0, G1, G2, clamp_mode, g);
    if (rc) return rc;
    DIQT_REQUIRE(phase != 0 || draw != 0xffffffffu, DIQT_E_SHAPE, "volume_joint_heun_inpaint: phase 0 uses draw and draw + 1");
    hipLaunchKernelGGL(volume_joint_heun_inpaint_kernel, g.grid, dim3(64, 4), g.lds, STREAM, y, slot, taps, xh, xn, x0, known, mask, phase,
                       N, D, H, W, P, stride, G0, G1, G2, a, b, c, d, kr, kc, lo, hi, clamp_mode, (unsigned)seed, (unsigned)(seed >> 32),
                       draw, draw_r, sample);
    return check_launch("volume_joint_heun_inpaint");
}

extern "C" int diqt_ddpm_inpaint_paste(const float* x, const float* renoise, const float* known, const unsigned char* mask,
                                       const float* qnoise, const float* kr0, const float* kr1, const float* al, const float* sg,
                                       float* out, int B, size_t per_batch, void* stream) {
    DIQT_REQUIRE(x && known && mask && qnoise && al && sg && out && ((kr0 && kr1) || !renoise), DIQT_E_ALIGN,
                 "ddpm_inpaint_paste: null pointer");
    DIQT_REQUIRE(B > 0 && per_batch > 0, DIQT_E_SHAPE, "ddpm_inpaint_paste: bad shape (B %d, per_batch %zu)", B, per_batch);
    DIQT_REQUIRE(B <= 65535 && (per_batch + 255) / 256 <= 0x7fffffffu, DIQT_E_SHAPE,
                 "ddpm_inpaint_paste: more than 65535 samples or 2^31 - 1 blocks per sample");
    hipLaunchKernelGGL(ddpm_inpaint_paste_kernel, dim3((unsigned)((per_batch + 255) / 256), B), dim3(64, 4), 0, STREAM, x, renoise, known,
                       mask, qnoise, kr0, kr1, al, sg, out, per_batch);
    return check_launch("ddpm_inpaint_paste");
}

extern "C" int diqt_volume_joint_step_inpaint(const float* y, const int* slot, const float* taps, float* x, float* x0_out,
                                              const float* known, const unsigned char* mask, int phase, int flags, int N, int D, int H,
                                              int W, int P, int stride, int G0, int G1, int G2, float kx, float k0, float kn, float kr0,
                                              float kr1, float al, float sg, float lo, float hi, int clamp_mode, unsigned long long seed,
                                              unsigned draw, unsigned draw_r, unsigned draw_q, unsigned sample, void* stream) {
    DIQT_REQUIRE(phase == 0 || phase == 1, DIQT_E_UNSUPPORTED, "volume_joint_step_inpaint: phase %d (0 = init and paste, 1 = step)", phase);
    DIQT_REQUIRE(flags >= 0 && flags <= 3, DIQT_E_UNSUPPORTED, "volume_joint_step_inpaint: flags %d (bit 0 = re-noise, bit 1 = paste)",
                 flags);
    DIQT_REQUIRE(known && mask, DIQT_E_ALIGN, "volume_joint_step_inpaint: null pointer");
    JointGrid g;
    int rc = joint_launch_plan("volume_joint_step_inpaint", x, phase == 1, slot && taps && (y || N == 0), N, D, H, W, P, stride, G0, G1,
                               G2, clamp_mode, g);
    if (rc) return rc;
    hipLaunchKernelGGL(volume_joint_step_inpaint_kernel, g.grid, dim3(64, 4), g.lds, STREAM, y, slot, taps, x, x0_out, known, mask, phase,
                       flags, N, D, H, W, P, stride, G0, G1, G2, kx, k0, kn, kr0, kr1, al, sg, lo, hi, clamp_mode, (unsigned)seed,
                       (unsigned)(seed >> 32), draw, draw_r, draw_q, sample);
    return check_launch("volume_joint_step_inpaint");
}

extern "C" int diqt_volume_joint_finish(const float* x, const int* slot, const float* vol, float* mean_io, float* m2_io, float* out_std,
                                        int s, int S, int D, int H, int W, int P, int stride, int G0, int G1, int G2, float mean,
                                        float stdv, float min_val, float fill, void* stream) {
    DIQT_REQUIRE(x && slot && mean_io, DIQT_E_ALIGN, "volume_joint_finish: null pointer");
    int rc = joint_lattice_ok("volume_joint_finish", D, H, W, P, stride, G0, G1, G2);
    if (rc) return rc;
    DIQT_REQUIRE(S > 0 && s >= 0 && s < S, DIQT_E_SHAPE, "volume_joint_finish: sample %d of %d", s, S);
    DIQT_REQUIRE(!(S == 1 && (m2_io || out_std)) && !(out_std && !m2_io), DIQT_E_SHAPE,
                 "volume_joint_finish: m2_io and out_std must be NULL for one sample, and a deviation map needs m2_io");
    DIQT_REQUIRE(!vol || stdv != 0.f, DIQT_E_SHAPE, "volume_joint_finish: std == 0");
    DIQT_REQUIRE(D <= 65535 && (H + 3) / 4 <= 65535, DIQT_E_SHAPE, "volume_joint_finish: more than 65535 planes / row groups");
    hipLaunchKernelGGL(volume_joint_finish_kernel, dim3((W + 63) / 64, (H + 3) / 4, D), dim3(64, 4), 0, STREAM, x, slot, vol, mean_io,
                       m2_io, out_std, s, S, D, H, W, P, stride, G0, G1, G2, mean, stdv, min_val, fill);
    return check_launch("volume_joint_finish");
}
