// Device pieces shared by the streaming attention kernels (attention_long.hip: every sequence fills all S
// tokens; attention_lengths.hip: per-sequence lengths): the block constants, the two LDS-only
// synchronisations and the backward's per-block products, D sums and P / dS images.  MASK = false is the
// code of the full-length kernels; MASK = true additionally zeroes P for keys at or beyond the
// sequence's length L (query rows at or beyond L need no test here: their saved lse is +inf, so
// exp(s - lse) is already zero).  Private to those two files, as attention_common.hpp.
#pragma once
#include "attention_common.hpp"

namespace kfk {

namespace {

constexpr int BK = 64;          // rows of a streamed block (and of every resident backward block)
constexpr int BLK = BK * 128;   // bytes of one 64-row image
constexpr int TK = BK / 16;

// Orders a wave's own LDS writes before its own later reads of them (the forward's P rows and the dQ
// kernel's dS rows never leave their wave): no workgroup barrier, and no drain of the DMA in flight.
__device__ __forceinline__ void lds_wave_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
// Workgroup barrier that publishes LDS writes only: unlike __syncthreads it leaves the LDS-DMA of the
// next block in flight (that one is waited for, counted, at the top of the next step).
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// S^T and dP^T of 16 queries (rows qw0.. of Qi / Oi) against the 64 keys of a block, as attention.hip's
// backward phase 1: sc / dp[j] hold keys 16 j + 4 lg + r of query qw0 + lc.
__device__ __forceinline__ void bwd_block_products(const uint8_t *Qi, const uint8_t *Oi, const uint8_t *Ki,
                                                   const uint8_t *Vi, int qw0, int lane, f32x4 (&sc)[TK],
                                                   f32x4 (&dp)[TK]) {
#pragma unroll
    for (int j = 0; j < TK; ++j) sc[j] = dp[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < DH / 32; ++s) {
        const bf16x8 qa = row_frag<128>(Qi, qw0, 32 * s, lane);
        const bf16x8 ga = row_frag<128>(Oi, qw0, 32 * s, lane);
        bf16x8 kf[TK], vf[TK];
#pragma unroll
        for (int j = 0; j < TK; ++j) {
            kf[j] = row_frag<128>(Ki, 16 * j, 32 * s, lane);
            vf[j] = row_frag<128>(Vi, 16 * j, 32 * s, lane);
        }
#pragma unroll
        for (int j = 0; j < TK; ++j) {
            sc[j] = mfma(kf[j], qa, sc[j]);
            dp[j] = mfma(vf[j], ga, dp[j]);
        }
    }
}

// This lane's share of D[q] = sum_key P_drop[q][key] dP[q][key] over the block (= rowsum(dO o O) with
// the f32 O; the saved bf16 O would put its rounding into dS = P o (dP - D), which cancels where the
// softmax is nearly one-hot).  MASK: keys >= L count as P = 0.
template <bool MASK = false>
__device__ __forceinline__ float bwd_block_dsum(const AttnArgs &a, uint32_t seed, int bh, const uint8_t *Qi,
                                                const uint8_t *Oi, const uint8_t *Ki, const uint8_t *Vi, int qw0,
                                                int row, int key0, float l, int lane, int L = 0) {
    const int lg = lane >> 4;
    f32x4 sc[TK], dp[TK];
    bwd_block_products(Qi, Oi, Ki, Vi, qw0, lane, sc, dp);
    float t = 0.f;
#pragma unroll
    for (int j = 0; j < TK; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int key = key0 + 16 * j + 4 * lg + r;
            float p = __expf(sc[j][r] * a.scale - l);
            if constexpr (MASK) p = key < L ? p : 0.f;
            if (keep_elem(seed, bh, row, key, a.thresh)) t += p * dp[j][r];
        }
    return t * a.inv_keep;
}

// P and dS^T of the same 16 x 64 tile.  Writes dS (and P_drop when Pi) rows qw0 + lc of the images.
// MASK: keys >= L get P = dS = 0.
template <bool MASK = false>
__device__ __forceinline__ void bwd_block_scores(const AttnArgs &a, uint32_t seed, int bh, const uint8_t *Qi,
                                                 const uint8_t *Oi, const uint8_t *Ki, const uint8_t *Vi, uint8_t *Pi,
                                                 uint8_t *Si, int qw0, int row, int key0, float l, float dd, int lane,
                                                 int L = 0) {
    const int lg = lane >> 4, lc = lane & 15;
    f32x4 sc[TK], dp[TK];
    bwd_block_products(Qi, Oi, Ki, Vi, qw0, lane, sc, dp);
#pragma unroll
    for (int j = 0; j < TK; ++j) {
        const int kb0 = 16 * j + 4 * lg;
        float pv[4], sv[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float p = __expf(sc[j][r] * a.scale - l);
            if constexpr (MASK) p = key0 + kb0 + r < L ? p : 0.f;
            const bool kp = keep_elem(seed, bh, row, key0 + kb0 + r, a.thresh);
            const float dpd = kp ? dp[j][r] * a.inv_keep : 0.f;
            pv[r] = kp ? p * a.inv_keep : 0.f;
            sv[r] = p * (dpd - dd);
        }
        if (Pi)
            *reinterpret_cast<uint2 *>(Pi + off<128>(qw0 + lc, kb0)) = make_uint2(pack_bf16x2_hw(pv[0], pv[1]),
                                                                                  pack_bf16x2_hw(pv[2], pv[3]));
        *reinterpret_cast<uint2 *>(Si + off<128>(qw0 + lc, kb0)) = make_uint2(pack_bf16x2_hw(sv[0], sv[1]),
                                                                              pack_bf16x2_hw(sv[2], sv[3]));
    }
}

}  // namespace

}  // namespace kfk
