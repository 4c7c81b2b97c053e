// The fill tiles of the three-product split build of conv_f9h_kernel (round 10; conv_split16.hip has the scheme and the plan):
//   variant 7  H9S_333_128  2 x 8 x 8 voxels, NVB = 2   (64 -> 64 @ 8 x 16^3: 256 workgroups instead of 128)
//   variant 8  H9S_333_64   1 x 8 x 8 voxels, NVB = 1   (128 -> 128 @ 8 x 8^3: 128 workgroups instead of 32)
// for launches whose 256-voxel tiles (variant 6) leave half the chip or more without a workgroup.  A smaller tile changes which
// workgroup computes a voxel, not how: chunk -> tap -> k-half order, the three accumulator sets and the bias behind the K sum are the
// kernel's, so y is bit-identical to variant 6 (the statistics rows are sums over other voxel sets).  One workgroup per CU as there.
// With 6 / 3 MFMAs per tap the 3-slot weight ring of variant 6 would reach 384 / 192 cycles ahead, less than an L2 round trip: both
// tiles take the 9-slot ring of the 16-bit builds (72 registers, which the smaller accumulator sets leave free).
#include "conv_f9h_kernel.h"

namespace diqt {
namespace h9 {

int launch_split_b(const void* x, const unsigned short* wp, const float* bias, const float* residual, void* y, const H9Geom& g, size_t lds,
                   unsigned grid, void* stream) {
    if (g.variant == 7) return launch_split_cfg<H9S_333_128>(x, wp, bias, residual, y, g, lds, grid, stream);
    if (g.variant == 8) return launch_split_cfg<H9S_333_64>(x, wp, bias, residual, y, g, lds, grid, stream);
    set_error("conv3d_fwd_split16(v9h): no variant %d", g.variant);
    return DIQT_E_UNSUPPORTED;
}

}  // namespace h9
}  // namespace diqt
