// Device pieces shared by the head dim 128 attention kernels (attention_d128.hip: [B, S, 3, H, 128]; attention_gqa.hip:
// grouped-query heads, [B, S, (H + 2 Hkv) * 128]): the 256-byte-row stager, the register-resident Q / dO pieces, the
// workgroup order, and the block steps of the forward and the backward.  None of them knows the qkv layout: they get
// pointers, LDS images and the (sequence * heads + head) index of the hash.  Private to those two files, as
// attention_common.hpp.
#pragma once
#include "attention_stream.hpp"

#if defined(__HIP_DEVICE_COMPILE__)
#define KFK_NO_PK_F32 __attribute__((target("no-packed-fp32-ops")))
#else
#define KFK_NO_PK_F32
#endif

namespace kfk {

namespace {

constexpr int D2 = 128;         // head dim
constexpr int IMG = BK * 256;   // bytes of a 64-row image of 256-byte rows
constexpr int TD = D2 / 16;     // accumulator tiles over the head dim
constexpr int KS = D2 / 32;     // MFMA K-steps over the head dim
constexpr int FWD_LDS = 4 * IMG + BLK;      // ring 2 x (K, V); P
constexpr int DQ_LDS = 4 * IMG + BLK;       // ring 2 x (K, V); dS
constexpr int DKV_LDS = 6 * IMG + 2 * BLK;  // K, V; ring 2 x (Q, dO); P_drop; dS

// Stage NIMG images of 64 rows x 128 bf16 (256-byte rows) with 16-byte global_load_lds: image t row r comes from
// src[t] + r * stride[t].  One load fills 1 KB = rows 4 pc .. 4 pc + 3, lane l the 16-byte piece l & 15 of row
// 4 pc + (l >> 4); the piece's 32-byte group is the source's group XOR hswz<256>(row).  The 4 waves split the
// 16 NIMG pieces.
template <int NIMG>
__device__ __forceinline__ void stage_rows256(uint8_t *lds, const uint16_t *const (&src)[NIMG],
                                              const int (&stride)[NIMG], int wave, int lane) {
    constexpr int PIECES = BK / 4;
    const int pch = lane & 15;
#pragma unroll
    for (int u = 0; u < NIMG * PIECES / 4; ++u) {
        const int gp = wave + 4 * u;
        const int t = gp / PIECES, pc = gp - t * PIECES;
        const int r = pc * 4 + (lane >> 4);
        const int col = ((((pch >> 1) ^ hswz<256>(r)) << 1) | (pch & 1)) * 8;
        const uint16_t *s = src[t] + static_cast<int64_t>(r) * stride[t] + col;
        __builtin_amdgcn_global_load_lds(s, lds + t * IMG + pc * 1024, 16, 0, 0);
    }
}

// The lane's four B-operand pieces of one row of 128 bf16 in global memory (what row_frag reads from an image)
__device__ __forceinline__ void load_row_frags(const uint16_t *rowp, int lane, bf16x8 (&f)[KS]) {
#pragma unroll
    for (int s = 0; s < KS; ++s) f[s] = *reinterpret_cast<const bf16x8 *>(rowp + 32 * s + 8 * (lane >> 4));
}

// score * scale as a rounded product of its own: the empty asm keeps the compiler from fusing it into the subtraction
// that follows (fma(score, scale, -max) carries the product's rounding error into the exponent).  Forward and backward
// then see the same number, and where a causal row has one visible key, score - max and score - lse are exactly 0, P
// exactly 1 and dS exactly 0.
__device__ __forceinline__ float scaled(float s, float scale) {
    float x = s * scale;
    asm("" : "+v"(x));
    return x;
}

// blockIdx.x -> (sequence * heads + head, 64-row block).  Causal: block-major, heaviest block first (`descending`:
// the heaviest is the last one: forward, dQ; else the first: dK/dV).  Bidirectional: (sequence, head)-major.
template <bool CAUSAL>
__device__ __forceinline__ void block_of(int n, bool descending, int &bh, int &blk) {
    if constexpr (CAUSAL) {
        const int nbh = gridDim.x / n, rank = blockIdx.x / nbh;
        bh = blockIdx.x - rank * nbh, blk = descending ? n - 1 - rank : rank;
    } else {
        bh = blockIdx.x / n, blk = blockIdx.x - bh * n;
    }
}

// The diagonal block's O^T += V^T P^T for this wave's 16 queries (rows q0 .. q0 + 15 of the block; P in Pi), the
// three-way split of attention_causal.hip's pv_diagonal on 8 accumulator tiles:
//   keys < q0            the MFMA; where the upper 16 of a 32-key step are the triangle's (q0 = 16, 48) the V operand
//                        is zeroed in the lanes that hold them (lane >> 4 >= 2), and P there is finite
//   keys q0 .. q0 + 15   the 16 x 16 triangle on the VALU: the lane of query q0 + lc adds key q0 + kk only if kk <= lc
//   keys >= q0 + 16      not read
__device__ __forceinline__ void pv_diagonal(const uint8_t *Vi, const uint8_t *Pi, int q0, int lane, f32x4 (&o)[TD]) {
    const int lg = lane >> 4, lc = lane & 15;
    const int qu = __builtin_amdgcn_readfirstlane(q0);
#pragma unroll
    for (int s = 0; s < BK / 32; ++s) {
        if (32 * s + 16 > qu) continue;
        const bool half = 32 * s + 32 > qu;
        bf16x8 va[TD];
#pragma unroll
        for (int c = 0; c < TD; ++c) {
            va[c] = tr_frag<256>(Vi, 32 * s, 16 * c, lane);
            if (half && lg >= 2) va[c] = __builtin_bit_cast(bf16x8, make_uint4(0, 0, 0, 0));
        }
        const bf16x8 pb = row_frag<128>(Pi, qu, 32 * s, lane);
#pragma unroll
        for (int c = 0; c < TD; ++c) o[c] = mfma(va[c], pb, o[c]);
    }
    const uint8_t *prow = Pi + off<128>(qu + lc, qu);  // P[query][keys q0 .. q0 + 15]: 32 contiguous bytes
    const uint4 plo = *reinterpret_cast<const uint4 *>(prow), phi = *reinterpret_cast<const uint4 *>(prow + 16);
    const uint32_t pw[8] = {plo.x, plo.y, plo.z, plo.w, phi.x, phi.y, phi.z, phi.w};
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) {
        const float p = kk & 1 ? bf16_hi(pw[kk >> 1]) : bf16_lo(pw[kk >> 1]);
        if (kk <= lc) {
#pragma unroll
            for (int c = 0; c < TD; ++c) {
                const uint2 v = *reinterpret_cast<const uint2 *>(Vi + off<256>(qu + kk, 16 * c + 4 * lg));
                o[c][0] = fmaf(p, bf16_lo(v.x), o[c][0]);
                o[c][1] = fmaf(p, bf16_hi(v.x), o[c][1]);
                o[c][2] = fmaf(p, bf16_lo(v.y), o[c][2]);
                o[c][3] = fmaf(p, bf16_hi(v.y), o[c][3]);
            }
        }
    }
}

// One step of the forward on the staged key block at key0 for this wave's 16 queries (Q pieces in qf, query `row`
// in this lane, rows q0 .. of the block's P image): scores, online softmax, dropout, P V.  MASK (the diagonal
// block) sets the scores of keys > row to -inf first; every row sees its own key there, and for query blocks > 0
// the running max is already finite, so exp(-inf - m) = 0 exactly and no row is empty.
template <bool MASK>
__device__ __forceinline__ void fwd_block(const AttnArgs &a, uint32_t seed, int bh, const bf16x8 (&qf)[KS],
                                          const uint8_t *Ki, const uint8_t *Vi, uint8_t *Pi, int q0, int row, int key0,
                                          int lane, float &m_run, float &l_run, f32x4 (&o)[TD]) {
    const int lg = lane >> 4, lc = lane & 15;
    f32x4 acc[TK];  // acc[j]: keys key0 + 16 j + 4 lg + r of query row
#pragma unroll
    for (int j = 0; j < TK; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        bf16x8 kf[TK];
#pragma unroll
        for (int j = 0; j < TK; ++j) kf[j] = row_frag<256>(Ki, 16 * j, 32 * s, lane);
#pragma unroll
        for (int j = 0; j < TK; ++j) acc[j] = mfma(kf[j], qf[s], acc[j]);
    }
    float m = m_run;
#pragma unroll
    for (int j = 0; j < TK; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            acc[j][r] = scaled(acc[j][r], a.scale);
            if constexpr (MASK) acc[j][r] = key0 + 16 * j + 4 * lg + r > row ? -INFINITY : acc[j][r];
            m = fmaxf(m, acc[j][r]);
        }
    m = fmaxf(m, __shfl_xor(m, 16));
    m = fmaxf(m, __shfl_xor(m, 32));
    const float alpha = __expf(m_run - m);  // 0 at the first block (m_run = -inf, m finite)
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < TK; ++j) {
        const int kb0 = 16 * j + 4 * lg;
        float p[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float e = __expf(acc[j][r] - m);
            sum += e;
            p[r] = keep_elem(seed, bh, row, key0 + kb0 + r, a.thresh) ? e * a.inv_keep : 0.f;
        }
        *reinterpret_cast<uint2 *>(Pi + off<128>(q0 + lc, kb0)) = make_uint2(pack_bf16x2_hw(p[0], p[1]),
                                                                             pack_bf16x2_hw(p[2], p[3]));
    }
    sum += __shfl_xor(sum, 16);
    sum += __shfl_xor(sum, 32);
    l_run = l_run * alpha + sum;
    m_run = m;
#pragma unroll
    for (int c = 0; c < TD; ++c)
#pragma unroll
        for (int r = 0; r < 4; ++r) o[c][r] *= alpha;
    lds_wave_sync();
    if constexpr (MASK) {
        pv_diagonal(Vi, Pi, q0, lane, o);
    } else {
#pragma unroll
        for (int s = 0; s < BK / 32; ++s) {
            bf16x8 va[TD];
#pragma unroll
            for (int c = 0; c < TD; ++c) va[c] = tr_frag<256>(Vi, 32 * s, 16 * c, lane);
            const bf16x8 pb = row_frag<128>(Pi, q0, 32 * s, lane);
#pragma unroll
            for (int c = 0; c < TD; ++c) o[c] = mfma(va[c], pb, o[c]);
        }
    }
}

// S^T and dP^T of 16 queries (Q pieces qf, dO pieces gf) against the 64 keys of a block: sc / dp[j] hold keys
// 16 j + 4 lg + r of the lane's query.
__device__ __forceinline__ void bwd_products(const bf16x8 (&qf)[KS], const bf16x8 (&gf)[KS], const uint8_t *Ki,
                                             const uint8_t *Vi, int lane, f32x4 (&sc)[TK], f32x4 (&dp)[TK]) {
#pragma unroll
    for (int j = 0; j < TK; ++j) sc[j] = dp[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        bf16x8 kf[TK], vf[TK];
#pragma unroll
        for (int j = 0; j < TK; ++j) {
            kf[j] = row_frag<256>(Ki, 16 * j, 32 * s, lane);
            vf[j] = row_frag<256>(Vi, 16 * j, 32 * s, lane);
        }
#pragma unroll
        for (int j = 0; j < TK; ++j) {
            sc[j] = mfma(kf[j], qf[s], sc[j]);
            dp[j] = mfma(vf[j], gf[s], dp[j]);
        }
    }
}

// This lane's share of D[q] = sum_key P_drop[q][key] dP[q][key] over the block (f32 throughout: the saved bf16 O
// would put its rounding into dS = P o (dP - D)).  MASK: keys > row count as P = 0.
template <bool MASK>
__device__ __forceinline__ float bwd_dsum(const AttnArgs &a, uint32_t seed, int bh, const bf16x8 (&qf)[KS],
                                          const bf16x8 (&gf)[KS], const uint8_t *Ki, const uint8_t *Vi, int row,
                                          int key0, float l, int lane) {
    const int lg = lane >> 4;
    f32x4 sc[TK], dp[TK];
    bwd_products(qf, gf, Ki, Vi, lane, sc, dp);
    float t = 0.f;
#pragma unroll
    for (int j = 0; j < TK; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int key = key0 + 16 * j + 4 * lg + r;
            float p = __expf(scaled(sc[j][r], a.scale) - l);
            if constexpr (MASK) p = key <= row ? p : 0.f;
            if (keep_elem(seed, bh, row, key, a.thresh)) t += p * dp[j][r];
        }
    return t * a.inv_keep;
}

// P_drop and dS of the same 16 x 64 tile into row `lrow` of the 64 x 64 images Si (and Pi when not null).
template <bool MASK>
__device__ __forceinline__ void bwd_scores(const AttnArgs &a, uint32_t seed, int bh, const bf16x8 (&qf)[KS],
                                           const bf16x8 (&gf)[KS], const uint8_t *Ki, const uint8_t *Vi, uint8_t *Pi,
                                           uint8_t *Si, int lrow, int row, int key0, float l, float dd, int lane) {
    const int lg = lane >> 4;
    f32x4 sc[TK], dp[TK];
    bwd_products(qf, gf, Ki, Vi, lane, sc, dp);
#pragma unroll
    for (int j = 0; j < TK; ++j) {
        const int kb0 = 16 * j + 4 * lg;
        float pv[4], sv[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float p = __expf(scaled(sc[j][r], a.scale) - l);
            if constexpr (MASK) p = key0 + kb0 + r <= row ? p : 0.f;
            const bool kp = keep_elem(seed, bh, row, key0 + kb0 + r, a.thresh);
            const float dpd = kp ? dp[j][r] * a.inv_keep : 0.f;
            pv[r] = kp ? p * a.inv_keep : 0.f;
            sv[r] = p * (dpd - dd);
        }
        if (Pi)
            *reinterpret_cast<uint2 *>(Pi + off<128>(lrow, kb0)) = make_uint2(pack_bf16x2_hw(pv[0], pv[1]),
                                                                              pack_bf16x2_hw(pv[2], pv[3]));
        *reinterpret_cast<uint2 *>(Si + off<128>(lrow, kb0)) = make_uint2(pack_bf16x2_hw(sv[0], sv[1]),
                                                                          pack_bf16x2_hw(sv[2], sv[3]));
    }
}

// past the 64 KB static LDS limit: raised once per kernel
template <class K>
void raise_lds(K kern, int bytes) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
}

}  // namespace

}  // namespace kfk
