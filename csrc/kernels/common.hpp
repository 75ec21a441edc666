// Shared device helpers for the kungfu-amd CDNA4 (gfx950) kernels.
//
// Conventions for every bandwidth-bound kernel here (cdna_hip_programming.md
// §6 G11/G13, App. B):
//   * 256-thread blocks (4 waves of 64), 16-byte vector loads/stores per lane,
//   * grid = min(ceil(n / (256 * VEC)), 2048) with a grid-stride loop, so a
//     launch fills all 256 CUs and long tensors amortise launch cost,
//   * f32 accumulation for bf16/f16 data, round-to-nearest-even on store,
//   * wave64 reductions via __shfl_xor (64-lane), then LDS across the 4 waves.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>

namespace kfk {

// Developer A/B switches (kungfu_amd/knobs.py kind "dev"): `name` is read from the environment
// only when KUNGFU_DEV_KNOBS=1 is set too; otherwise the measured default `def` holds, so a
// stale shell variable cannot change a production run.
inline int dev_knob(const char *name, int def) {
    static const bool dev = [] {
        const char *e = std::getenv("KUNGFU_DEV_KNOBS");
        return e && *e && std::atoi(e) != 0;
    }();
    if (!dev) return def;
    const char *e = std::getenv(name);
    return e && *e ? std::atoi(e) : def;
}

constexpr int kBlock = 256;
constexpr int kWave = 64;
constexpr int kMaxGrid = 2048;

inline int grid_for(size_t n_vec) {
    size_t g = (n_vec + kBlock - 1) / kBlock;
    if (g < 1) g = 1;
    if (g > static_cast<size_t>(kMaxGrid)) g = kMaxGrid;
    return static_cast<int>(g);
}

__device__ __forceinline__ float bf16_to_f32(uint16_t h) { return __uint_as_float(static_cast<uint32_t>(h) << 16); }
// the two bf16 halves of a 32-bit word as f32
__device__ __forceinline__ float bf16_lo(uint32_t w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float bf16_hi(uint32_t w) { return __uint_as_float(w & 0xffff0000u); }

// f32 pair -> bf16 pair comes in THREE forms that give the same bits for finite inputs and differ in
// what the compiler makes of the code around them: pack_bf16x2 (integer arithmetic), cvt_pk_bf16
// (v_cvt_pk_bf16_f32 through inline asm) and pack_bf16x2_hw (the same instruction through
// __builtin_convertvector).  Which one a call site uses is measured per kernel; a helper that moves
// between files keeps the form it had.
//
// f32 -> bf16, round to nearest even, in integer arithmetic (about 2.5 vector instructions per
// value).  Finite inputs and infinities only: a NaN is NOT guaranteed to stay one (0x7f800001
// rounds to +inf, 0x7fffffff carries into the sign and gives -0).  gfx950's v_cvt_pk_bf16_f32 gives
// the same bits for every finite input (tools/diag/cvt_check.hip, 2^26 patterns) and is not a slow
// instruction; what round 6 measured when it replaced this function everywhere through
// __builtin_convertvector (the NT GEMM 6.5x slower, ResNet-50 21.17 vs 20.35 ms/step) was register
// allocation: 156-444 bytes of scratch per lane in gemm_nt_kernel<192|256, *>, and in the conv
// kernels a second accumulator set (96 instead of 64 AGPRs), which took the row-image kernel from
// two waves per SIMD to one (profiles/conv_epilogue_rounding.md).  So this stays the default, and
// cvt_pk_bf16 below is used site by site where the kernel's resource line does not get worse.
__device__ __forceinline__ uint16_t f32_to_bf16(float f) {
    uint32_t u = __float_as_uint(f);
    u += 0x7fffu + ((u >> 16) & 1u);
    return static_cast<uint16_t>(u >> 16);
}
// (lo, hi) -> one 32-bit word, lo in the low half
__device__ __forceinline__ uint32_t pack_bf16x2(float lo, float hi) {
    return static_cast<uint32_t>(f32_to_bf16(lo)) | (static_cast<uint32_t>(f32_to_bf16(hi)) << 16);
}
// The same pair in ONE instruction, v_cvt_pk_bf16_f32: round to nearest even, bit-identical to
// pack_bf16x2 for every finite input and the infinities (overflow rounds to +-inf, f32 subnormals
// to +-0 or the smallest bf16 subnormal, the sign of zero is kept); a NaN input comes out as a NaN
// (quiet), which the integer formula does not guarantee.  Inline asm with "v" operands, not
// __builtin_convertvector: the asm reads the accumulators where they are, while the builtin made the
// compiler keep a second accumulator set in the conv kernels (see f32_to_bf16).
__device__ __forceinline__ uint32_t cvt_pk_bf16(float lo, float hi) {
    uint32_t r;
    asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
    return r;
}
// The same instruction as a builtin conversion, schedulable like any other op.  Used where it measured
// faster than the integer form: the stem forward epilogue and the stem weight gradient's dx, stem3's
// im2col packing and the attention kernels' P / dS / output packs (r6t15: ResNet-50 20.24-20.27 vs
// 20.35-20.42 ms/step with attention / stem / stem3 on it).  In gemm.hip's epilogues the same builtin
// measured 6.5x slower (r6t14, the scratch described at f32_to_bf16), so it is never the default.
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
__device__ __forceinline__ uint32_t pack_bf16x2_hw(float lo, float hi) {
    const bf16x2 v = __builtin_convertvector(f32x2{lo, hi}, bf16x2);
    return __builtin_bit_cast(uint32_t, v);
}

// 8 (16 bytes) or 4 (8 bytes) bf16 <-> f32; the packs round with pack_bf16x2 (the integer form)
__device__ __forceinline__ void unpack_bf16x8(const uint4 &v, float (&f)[8]) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        f[2 * i] = bf16_lo(w[i]);
        f[2 * i + 1] = bf16_hi(w[i]);
    }
}
__device__ __forceinline__ uint4 pack_bf16x8(const float (&f)[8]) {
    uint32_t w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] = pack_bf16x2(f[2 * i], f[2 * i + 1]);
    return make_uint4(w[0], w[1], w[2], w[3]);
}
// acc += the 8 bf16 of v
__device__ __forceinline__ void add_bf16x8(const uint4 &v, float (&acc)[8]) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        acc[2 * i] += bf16_lo(w[i]);
        acc[2 * i + 1] += bf16_hi(w[i]);
    }
}
__device__ __forceinline__ void unpack_bf16x4(const uint2 &v, float (&f)[4]) {
    f[0] = bf16_lo(v.x);
    f[1] = bf16_hi(v.x);
    f[2] = bf16_lo(v.y);
    f[3] = bf16_hi(v.y);
}
__device__ __forceinline__ uint2 pack_bf16x4(const float (&f)[4]) {
    return make_uint2(pack_bf16x2(f[0], f[1]), pack_bf16x2(f[2], f[3]));
}

__device__ __forceinline__ float f16_to_f32(uint16_t h) {
    _Float16 x;
    __builtin_memcpy(&x, &h, 2);
    return static_cast<float>(x);
}

__device__ __forceinline__ uint16_t f32_to_f16(float f) {
    _Float16 x = static_cast<_Float16>(f);
    uint16_t h;
    __builtin_memcpy(&h, &x, 2);
    return h;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Block-wide sum of up to two values; result valid in thread 0.
template <int N>
__device__ __forceinline__ void block_sum(float (&v)[N], float (*lds)[kBlock / kWave]) {
    const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        v[i] = wave_sum(v[i]);
        if (lane == 0) lds[i][wid] = v[i];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < N; ++i) {
            float s = 0;
#pragma unroll
            for (int w = 0; w < kBlock / kWave; ++w) s += lds[i][w];
            v[i] = s;
        }
    }
}

enum DT : int { DT_U8 = 0, DT_I32 = 6, DT_I64 = 7, DT_F16 = 8, DT_BF16 = 9, DT_F32 = 10, DT_F64 = 11 };
enum OP : int { OP_SUM = 0, OP_MIN = 1, OP_MAX = 2, OP_PROD = 3 };

// gelu'(x) = Phi(x) + x phi(x) with ONE exponential: erf(x / sqrt 2) by Abramowitz-Stegun 7.1.26
// (|error| < 1.5e-7, far below a bf16 ulp of the result) whose e^{-x^2/2} factor is phi's own.
// ~12 vector instructions instead of erff + expf (~40): the fused pass below is memory-bound.
__device__ __forceinline__ float gelu_grad_fast(float x) {
    const float z = fabsf(x) * 0.70710678118654752f;
    const float e = __expf(-0.5f * x * x);  // = e^{-z^2}
    const float t = __frcp_rn(1.f + 0.3275911f * z);
    const float poly = t * (0.254829592f + t * (-0.284496736f + t * (1.421413741f + t * (-1.453152027f +
                                                                                            t * 1.061405429f))));
    const float erf_abs = 1.f - poly * e;
    const float cdf = 0.5f * (1.f + (x < 0.f ? -erf_abs : erf_abs));
    return cdf + x * (e * 0.39894228040143268f);
}

// Phi(x) = 0.5 (1 + erf(x / sqrt 2)) by the same Abramowitz-Stegun form (one exponential)
__device__ __forceinline__ float gelu_cdf_fast(float x) {
    const float z = fabsf(x) * 0.70710678118654752f;
    const float e = __expf(-0.5f * x * x);
    const float t = __frcp_rn(1.f + 0.3275911f * z);
    const float poly = t * (0.254829592f + t * (-0.284496736f + t * (1.421413741f + t * (-1.453152027f +
                                                                                            t * 1.061405429f))));
    const float erf_abs = 1.f - poly * e;
    return 0.5f * (1.f + (x < 0.f ? -erf_abs : erf_abs));
}

}  // namespace kfk
