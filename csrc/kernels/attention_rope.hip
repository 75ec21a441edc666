// Rotary position embeddings (RoPE) for the head dim 128 attention kernels: the forward rotation of the Q and K heads
// of a grouped-query qkv tensor, one streaming pass.  Its output is what attention_d128.hip's forward reads and what is
// saved for the backward; the transposed rotation of dq / dk runs in the epilogues of attention_d128.hip's dQ and dK/dV
// kernels (template parameter ROPE there), so the backward has no pass of its own.
//
// Convention   Half-split ("rotate_half": Hugging Face LLaMA, GPT-NeoX) over the whole head, positions 0 .. S - 1.
//              With c = cos[t][i], s = sin[t][i] of position t, i = 0 .. 63:
//                x'[i] = x[i] c - x[i + 64] s        x'[i + 64] = x[i + 64] c + x[i] s
//              cos and sin are f32 [S, 64] tables made on the host (angles reach 8191 rad: no sine is evaluated here).
//              S = 64 .. 8192 in steps of 64: beyond 1024 for attention_d128.hip's band kernels.
// Interface    qkv and the result [B, S, NH * 128] bf16 with NH = H + 2 Hkv: a row (token) holds the H query heads,
//              the Hkv key heads, the Hkv value heads, 256 bytes each.  Heads 0 .. H + Hkv - 1 are rotated in f32 (one
//              product and one fma per element) and rounded once (pack_bf16x2_hw); the value heads are copied bit for
//              bit.  Every output element is written once.  No LDS, no atomics: bitwise reproducible.
// Work split   8 lanes per token, 32 tokens per workgroup of 256 threads, B * S / 32 workgroups (S % 64 == 0: no tail,
//              and a workgroup's tokens are 32 consecutive positions of one sequence).  Lane j = 0 .. 7 of a token owns
//              the 16-byte piece j of every head's lower half (elements 8 j .. 8 j + 7) and the matching piece of the
//              upper half 128 bytes on (elements 64 + 8 j ..): both members of its 8 rotary pairs, so no lane talks to
//              another.  It loads its 32 bytes of cos and of sin (columns 8 j .. 8 j + 7 of row t) once and keeps them
//              in registers while it walks the token's heads, 4 heads per step: 8 loads in flight, then 8 stores.
// Coalescing   The 8 lanes of a token read or write one whole 128-byte head half per instruction; a wave touches the
//              same half of the same head of 8 consecutive tokens, 8 full 128-byte lines RS = NH * 256 bytes apart.
//
// Rows and columns touched, by hand (tok = 32 blockIdx.x + threadIdx.x / 8 < B * S since the grid is B * S / 32):
//   qkv, result   row tok, bytes 256 h + 16 j .. + 15 and 256 h + 128 + 16 j .. + 15 for h = 0 .. NH - 1: the last
//                 byte is 256 (NH - 1) + 128 + 16 * 7 + 15 = 256 NH - 1, the row's last.  A range [h0, h1) (rotated
//                 heads [0, H + Hkv), copied heads [H + Hkv, NH)) is walked in steps of 4 heads while h + 4 <= h1 and
//                 one step of the h1 - h = 1 .. 3 heads left: no head outside the range.
//   cos, sin      row t = tok mod S < S, floats 8 j .. 8 j + 7 <= 63.
//
// Compiled without packed f32 instructions (KFK_NO_PK_F32), the precaution attention_lengths.hip's header explains.
#include "attention_common.hpp"

#include <stdexcept>

namespace kfk {

namespace {

constexpr int ROPE_D = 128;      // head dim
constexpr int ROPE_HALF = 64;    // rotary pairs per head: the table row length
constexpr int ROPE_TOKENS = 32;  // tokens per workgroup
constexpr int ROPE_STEP = 4;     // heads per step of a lane's walk

// The lane's table pieces: cos and sin of columns 8 j .. 8 j + 7 of the token's row
struct RopeCoef {
    float4 c0, c1, s0, s1;
};

// Two rotary pairs: a holds x[i], x[i + 1] and b holds x[i + 64], x[i + 65] as bf16 pairs
__device__ __forceinline__ void rope_pair2(uint32_t &a, uint32_t &b, float c0, float c1, float s0, float s1) {
    const float a0 = bf16_lo(a), a1 = bf16_hi(a), b0 = bf16_lo(b), b1 = bf16_hi(b);
    a = pack_bf16x2_hw(fmaf(a0, c0, -(b0 * s0)), fmaf(a1, c1, -(b1 * s1)));
    b = pack_bf16x2_hw(fmaf(b0, c0, a0 * s0), fmaf(b1, c1, a1 * s1));
}

// N heads from h on of the lane's token: src / dst point at the lane's piece of head 0's lower half.  All 2 N loads
// are issued before the first store.
template <bool ROTATE, int N>
__device__ __forceinline__ void rope_step(const uint16_t *__restrict__ src, uint16_t *__restrict__ dst, int h,
                                          const RopeCoef &k) {
    uint4 lo[N], hi[N];
#pragma unroll
    for (int u = 0; u < N; ++u) {
        lo[u] = *reinterpret_cast<const uint4 *>(src + (h + u) * ROPE_D);
        hi[u] = *reinterpret_cast<const uint4 *>(src + (h + u) * ROPE_D + ROPE_HALF);
    }
#pragma unroll
    for (int u = 0; u < N; ++u) {
        if constexpr (ROTATE) {
            rope_pair2(lo[u].x, hi[u].x, k.c0.x, k.c0.y, k.s0.x, k.s0.y);
            rope_pair2(lo[u].y, hi[u].y, k.c0.z, k.c0.w, k.s0.z, k.s0.w);
            rope_pair2(lo[u].z, hi[u].z, k.c1.x, k.c1.y, k.s1.x, k.s1.y);
            rope_pair2(lo[u].w, hi[u].w, k.c1.z, k.c1.w, k.s1.z, k.s1.w);
        }
        *reinterpret_cast<uint4 *>(dst + (h + u) * ROPE_D) = lo[u];
        *reinterpret_cast<uint4 *>(dst + (h + u) * ROPE_D + ROPE_HALF) = hi[u];
    }
}

// Heads h0 .. h1 - 1: whole steps of ROPE_STEP heads, then the 1 .. 3 that remain
template <bool ROTATE>
__device__ __forceinline__ void rope_heads(const uint16_t *__restrict__ src, uint16_t *__restrict__ dst, int h0, int h1,
                                           const RopeCoef &k) {
    int h = h0;
    for (; h + ROPE_STEP <= h1; h += ROPE_STEP) rope_step<ROTATE, ROPE_STEP>(src, dst, h, k);
    static_assert(ROPE_STEP == 4, "the tail below");
    if (h1 - h == 3) rope_step<ROTATE, 3>(src, dst, h, k);
    else if (h1 - h == 2) rope_step<ROTATE, 2>(src, dst, h, k);
    else if (h1 - h == 1) rope_step<ROTATE, 1>(src, dst, h, k);
}

// NR = H + Hkv rotated heads, then NH - NR copied ones
KFK_NO_PK_F32 __global__ __launch_bounds__(256) void rope_fwd_kernel(const uint16_t *__restrict__ qkv,
                                                                     uint16_t *__restrict__ out,
                                                                     const float *__restrict__ cos_t,
                                                                     const float *__restrict__ sin_t, int S, int NR,
                                                                     int NH) {
    const int64_t tok = static_cast<int64_t>(blockIdx.x) * ROPE_TOKENS + (threadIdx.x >> 3);
    const int j = threadIdx.x & 7;
    const int t = static_cast<int>(tok % S);  // the position
    const float4 *cp = reinterpret_cast<const float4 *>(cos_t + t * ROPE_HALF + 8 * j);
    const float4 *sp = reinterpret_cast<const float4 *>(sin_t + t * ROPE_HALF + 8 * j);
    const RopeCoef k = {cp[0], cp[1], sp[0], sp[1]};
    const int64_t row = tok * NH * ROPE_D + 8 * j;
    rope_heads<true>(qkv + row, out + row, 0, NR, k);
    rope_heads<false>(qkv + row, out + row, NR, NH, k);
}

}  // namespace

void launch_rope_forward(const uint16_t *qkv, uint16_t *out, const float *cos, const float *sin, int B, int S, int H,
                         int Hkv, hipStream_t s) {
    if (!attention_gqa_supported(S, H, Hkv, 64))  // (any window: the S of the band kernels that read long results)
        throw std::invalid_argument("rope: needs S % 64 == 0, 64 <= S <= 8192, 1 <= kv_heads <= heads and "
                                    "heads % kv_heads == 0");
    const int64_t tokens = static_cast<int64_t>(B) * S;  // a multiple of 64
    if (tokens / ROPE_TOKENS > INT32_MAX) throw std::invalid_argument("rope: too many tokens for one grid");
    if (tokens == 0) return;
    rope_fwd_kernel<<<static_cast<int>(tokens / ROPE_TOKENS), 256, 0, s>>>(qkv, out, cos, sin, S, H + Hkv, H + 2 * Hkv);
}

}  // namespace kfk
