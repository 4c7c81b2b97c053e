// The tap-paired build of the three-product split conv on the 256-voxel tile (round 11; conv_f9p_kernel.h has the body,
// conv_split16.hip the scheme and the plan):
//   variant 9  H9S_333_256  4 x 8 x 8 voxels, 14 pair steps of 48 v_mfma_f32_16x16x32_f16 per chunk, two accumulator sets
// for the launches of the pair plan (diqt_conv3d_fwd_split16_pair*).  One workgroup per CU as variant 6; x', the packed weights, the
// tiles, the statistics rows and the epilogue are variant 6's.
#include "conv_f9p_kernel.h"

namespace diqt {
namespace h9 {

constexpr int PAIR_PD = 7;       // weight-ring slots (pair steps): six steps = 4.6k MFMA cycles ahead; with 2 slots (one step ahead)
                                 // 128 -> 64 @ 8 x 32^3 took 352 us against 320 us, and 333 us on variant 6

int launch_split_c(const void* x, const unsigned short* wp, const float* bias, const float* residual, void* y, const H9Geom& g, size_t lds,
                   unsigned grid, void* stream) {
    using C = H9S_333_256;
    static_assert(C::LDS_BYTES + BIASB <= 160 * 1024, "LDS budget with the staged bias");
    if (g.variant != 9) {
        set_error("conv3d_fwd_split16_pair(v9p): no variant %d", g.variant);
        return DIQT_E_UNSUPPORTED;
    }
    typedef void (*KP)(const void*, const unsigned short*, const float*, const float*, void*, H9Geom);
    static const KP kerns[4] = {conv_f9p_kernel<C, 0, PAIR_PD>, conv_f9p_kernel<C, 1, PAIR_PD>, conv_f9p_kernel<C, 2, PAIR_PD>,
                                conv_f9p_kernel<C, 3, PAIR_PD>};
    const KP kern = kerns[(residual ? 1 : 0) | (g.stats ? 2 : 0)];
    lds += BIASB;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    DIQT_REQUIRE(e == hipSuccess, DIQT_E_LAUNCH, "conv3d_fwd_split16_pair(v9p): hipFuncSetAttribute: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, (hipStream_t)stream, x, wp, bias, residual, y, g);
    return check_launch("conv3d_fwd_split16(v9h)");
}

}  // namespace h9
}  // namespace diqt

// host-only: the worst number of distinct addresses on one 16-byte LDS slot over every ds_read_b128 service group of the pair body
// (14 steps, both fragments, all eight column blocks, both voxel halves), from the kernel header's own address function.  1 = conflict-free.
extern "C" int diqt_conv_split16_pair_lds_conflicts(void) { return diqt::h9::pair_lds_conflicts<diqt::h9::H9S_333_256>(); }
