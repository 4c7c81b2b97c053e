// conv_fwd9_kernel, Winograd F(2,3) 3x3x3 variant (see conv_fwd9.hip)
#include "conv_fwd9_kernel.h"

namespace diqt {

int fwd9_launch_j(const float* x, const float* packed, const float* bias, const float* residual, float* y, const F9Geom& g, size_t lds,
                  unsigned grid, void* stream) {
    if (g.variant == 7) return f9_launch<F9_333W>(x, packed + g.wOff, bias, residual, y, g, lds, grid, stream);
    set_error("conv3d_fwd(v9): no variant %d in this unit", g.variant);
    return DIQT_E_UNSUPPORTED;
}

}  // namespace diqt
