// SwiGLU, the gated FFN activation of the LLaMA family, bf16 in/out, f32 arithmetic, for gfx950.
//
//   forward   h = bf16(g * sigmoid(g) * u)                                   gu [rows, 2F] -> h [rows, F]
//   backward  sg = sigmoid(g);  dg = dh * u * sg * (1 + g * (1 - sg));  du = dh * g * sg
//                                                                            dh [rows, F], gu -> dgu [rows, 2F]
//
// Interface    gu is the output of ONE Linear(d, 2F): columns 0 .. F-1 of a row are the gate g, columns F .. 2F-1 the
//              up projection u (half-split, as the rotary kernels pair i with i + dh/2).  F % 8 == 0, any rows.
//              dgu has gu's layout: both halves are written once into the one tensor, there is no concatenation.
//              The backward recomputes sigmoid from gu; h is not saved.
// Work split   One thread per (row, 8-column group): it reads the 8 gates and the 8 matching ups (two 16-byte
//              loads F elements apart; F % 8 == 0 keeps both 16-byte aligned), the backward also 8 dh, and writes
//              one (forward) or two (backward) 16-byte words.  256-thread workgroups, grid-stride over the
//              rows * F/8 groups; a thread divides once for its first (row, group) and then steps both by the
//              constant stride's quotient and remainder, so the loop has no division.  The last workgroup's tail is
//              the loop condition idx < rows * F/8: no address beyond the tensors is formed.
// HBM          Every input element is read once and every output element written once per direction; no LDS, no
//              scratch.
// Math         sigmoid through e = expf(-|g|) <= 1 (no overflow for any g) and p = 1 / (1 + e):
//                g >= 0: sg = p, 1 - sg = e * p;      g < 0: sg = e * p, 1 - sg = p
//              so both sg and 1 - sg keep a RELATIVE error of a few ulp (1 - fl(sg) would lose it for large g, where
//              the factor 1 + g (1 - sg) multiplies that error by g).  The f32 functions: expf (HIP math API: at most
//              1 ulp) and the IEEE f32 division and multiplication / addition (correctly rounded; hipcc's default
//              correctly-rounded divide).  In units of 2^-24: sg and 1 - sg carry expf 1 + add 1 + divide 1 +
//              multiply 1 = 4; h and du two more multiplies = 6; dg = ((dh * u) * sg) * (1 + g * (1 - sg)) = 13.
//              g = -100: e flushes to 0 or stays tiny, h = -0 or 0;  g = +100: sg = 1, h = u * g;  nothing overflows.
#include "common.hpp"
#include "kernels.hpp"

namespace kfk {

namespace {

// sg = sigmoid(g) and om = 1 - sigmoid(g), both to relative accuracy
__device__ __forceinline__ void sigmoid_pair(float g, float &sg, float &om) {
    const float e = expf(-fabsf(g));
    const float p = 1.f / (1.f + e);
    const float q = e * p;
    sg = g >= 0.f ? p : q;
    om = g >= 0.f ? q : p;
}

// The (row, group) walk of a thread: idx = row * fg + cg for idx = first, first + stride, ...
struct GroupWalk {
    int64_t idx, row, stride, srow;
    int cg, scg;
    __device__ GroupWalk(int fg) {
        idx = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
        stride = static_cast<int64_t>(gridDim.x) * kBlock;
        row = idx / fg;
        cg = static_cast<int>(idx - row * fg);
        srow = stride / fg;
        scg = static_cast<int>(stride - srow * fg);
    }
    __device__ void next(int fg) {
        idx += stride;
        row += srow;
        cg += scg;
        if (cg >= fg) {
            cg -= fg;
            ++row;
        }
    }
};

__global__ __launch_bounds__(kBlock) void swiglu_fwd_kernel(const uint4 *__restrict__ gu, uint4 *__restrict__ h,
                                                            int64_t n, int fg) {
    for (GroupWalk w(fg); w.idx < n; w.next(fg)) {
        const int64_t at = w.row * 2 * fg + w.cg;  // in 16-byte words: a row of gu is 2 fg of them
        float g[8], u[8], o[8];
        unpack_bf16x8(gu[at], g);
        unpack_bf16x8(gu[at + fg], u);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            float sg, om;
            sigmoid_pair(g[k], sg, om);
            o[k] = (g[k] * sg) * u[k];
        }
        h[w.idx] = pack_bf16x8(o);
    }
}

__global__ __launch_bounds__(kBlock) void swiglu_bwd_kernel(const uint4 *__restrict__ dh, const uint4 *__restrict__ gu,
                                                            uint4 *__restrict__ dgu, int64_t n, int fg) {
    for (GroupWalk w(fg); w.idx < n; w.next(fg)) {
        const int64_t at = w.row * 2 * fg + w.cg;
        float d[8], g[8], u[8], og[8], ou[8];
        unpack_bf16x8(dh[w.idx], d);
        unpack_bf16x8(gu[at], g);
        unpack_bf16x8(gu[at + fg], u);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            float sg, om;
            sigmoid_pair(g[k], sg, om);
            og[k] = ((d[k] * u[k]) * sg) * (1.f + g[k] * om);
            ou[k] = (d[k] * g[k]) * sg;
        }
        dgu[at] = pack_bf16x8(og);
        dgu[at + fg] = pack_bf16x8(ou);
    }
}

}  // namespace

void launch_swiglu_forward(const uint16_t *gu, uint16_t *h, int64_t rows, int64_t F, hipStream_t st) {
    const int64_t n = rows * (F / 8);
    if (n <= 0) return;
    swiglu_fwd_kernel<<<grid_for(static_cast<size_t>(n)), kBlock, 0, st>>>(
        reinterpret_cast<const uint4 *>(gu), reinterpret_cast<uint4 *>(h), n, static_cast<int>(F / 8));
}

void launch_swiglu_backward(const uint16_t *dh, const uint16_t *gu, uint16_t *dgu, int64_t rows, int64_t F,
                            hipStream_t st) {
    const int64_t n = rows * (F / 8);
    if (n <= 0) return;
    swiglu_bwd_kernel<<<grid_for(static_cast<size_t>(n)), kBlock, 0, st>>>(
        reinterpret_cast<const uint4 *>(dh), reinterpret_cast<const uint4 *>(gu), reinterpret_cast<uint4 *>(dgu), n,
        static_cast<int>(F / 8));
}

}  // namespace kfk
