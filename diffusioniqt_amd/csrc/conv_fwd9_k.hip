// conv_fwd9_kernel with the GroupNorm-apply prologue (see conv_fwd9_kernel.h): the Winograd F(2,3) 3x3x3 variant with Mish
#include "conv_fwd9_kernel.h"

namespace diqt {

int fwd9_launch_k(const float* x, const float* packed, const float* bias, const float* residual, float* y, const F9Geom& g, size_t lds,
                  unsigned grid, void* stream) {
    if (g.variant == 7 && g.gnaAct == DIQT_ACT_MISH)
        return f9_launch<F9_333W, false, DIQT_ACT_MISH>(x, packed + g.wOff, bias, residual, y, g, lds, grid, stream);
    set_error("conv3d_fwd(v9, GroupNorm-apply prologue): no variant %d / activation %d in this unit", g.variant, g.gnaAct);
    return DIQT_E_UNSUPPORTED;
}

}  // namespace diqt
