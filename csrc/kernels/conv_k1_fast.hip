// 1x1 convolutions whose output pixel m reads input pixel m (stride 1, no padding; conv_fast1): the
// FAST1 instances of every tile variant x fused epilogue -- A rows at m * Cin, no pixel decode.
// (the kernel template and its launch helpers: conv_kernel.hpp; the general instances: conv_k1.hip)
#include "conv_kernel.hpp"

namespace kfk {

void launch_conv_k1_fast(const uint16_t *x, const uint16_t *w, uint16_t *y, Geo g, const EpiArgs &ea, int epi,
                         hipStream_t s, int variant) {
    launch_ks<1, true>(x, w, y, g, ea, epi, s, variant);
}

}  // namespace kfk
