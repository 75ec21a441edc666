// 1x1 convolutions on the MFMA implicit-GEMM kernel: every tile variant x fused epilogue instance.
// (the kernel template and its launch helpers: conv_kernel.hpp)
#include "conv_kernel.hpp"

namespace kfk {

void launch_conv_k1(const uint16_t *x, const uint16_t *w, uint16_t *y, Geo g, const EpiArgs &ea, int epi,
                    hipStream_t s, int variant) {
    // stride 1 onto the input's own pixels (every 1x1 of a ResNet step but the stride-2 shortcuts): the
    // instances without a pixel decode, built in their own file so the two sets compile side by side
    if (conv_fast1(g)) launch_conv_k1_fast(x, w, y, g, ea, epi, s, variant);
    else launch_ks<1>(x, w, y, g, ea, epi, s, variant);
}

}  // namespace kfk
