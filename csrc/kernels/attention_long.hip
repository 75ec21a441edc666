// Fused multi-head self-attention for 192 to 512 tokens (every multiple of 64; head dim 64, bf16,
// dropout on the probabilities, no mask): streaming kernels.  attention.hip keeps Q, K, V and the
// whole S x S probability image of one (sequence, head) in LDS, which stops at S = 128; here one
// block of rows stays resident and the other operand streams past it in blocks of 64 rows
// through a two-slot LDS ring filled by LDS-DMA, so LDS per workgroup does not grow with S
// (56 to 64 KB: two workgroups per CU).  Same interface, same dropout hash (keep_elem on the
// global query / key index), same MFMA fragment layouts as attention.hip.
//
//   forward   one workgroup per (sequence, head, query block of BQ = 128 rows, 64 where S is no
//             multiple of 128).  Per key block: S^T = K Q^T (the swapped product: a query's 16
//             scores of the block sit in one lane and its three partners), running max m and sum
//             l per query, e = exp(s - m) unnormalised (dropped) into the P image, the O^T
//             accumulators rescaled by exp(m_old - m_new) -- they hold the same query on the same
//             lane, no shuffle -- then O^T += V^T P^T.  At the end O / l and lse = m + log l.
//   backward  two kernels of that skeleton, both recomputing P = exp(S*scale - lse), no atomics,
//             no zeroed scratch, no workgroup waits on another (bitwise reproducible):
//             attn_long_dq_kernel   per (sequence, head, 64 queries): Q, dO resident, K / V
//                                   streamed twice: first D = rowsum(P_drop o dP) in f32 (that is
//                                   rowsum(dO o O) without the bf16 rounding of the saved O, which
//                                   dS = P o (dP - D) amplifies where the softmax is nearly one-hot),
//                                   written to the [B, H, S] f32 buffer dsum; then dQ^T += K^T dS^T.
//             attn_long_dkv_kernel  per (sequence, head, 64 keys), launched after it: K, V
//                                   resident, Q / dO streamed, lse and D of the streamed rows
//                                   read from global; dV^T += dO^T P_drop, dK^T += Q^T dS.
//             (D recomputed per streamed block inside the dK/dV kernel instead of the buffer
//             measured 8 to 10 % slower for the backward, profiles/attention_long.md.)
//
// Every step of the block loop is: wait for the block's DMA (issued one step earlier: all that is
// outstanding), barrier, issue the next block's DMA into the slot the barrier just freed, compute.
// Between writing and reading the P / dS images the dK/dV kernel needs a second barrier (one that
// leaves the DMA in flight); in the forward and the dQ kernel those rows never leave their wave.
// Trip counts depend on S only.  All lengths are multiples of the block sizes, so no row index leaves [0, S).
#include "attention_common.hpp"

#include <stdexcept>

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

template <int BQ>
__global__ __launch_bounds__(256) void attn_long_fwd_kernel(AttnArgs a, int S) {
    constexpr int QW = BQ / 4;  // query rows per wave
    constexpr int TQ = QW / 16;
    __shared__ __attribute__((aligned(1024))) uint8_t lds[BQ * 128 + 4 * BLK + BQ * 128];
    uint8_t *Qi = lds, *ring = lds + BQ * 128, *Pi = ring + 4 * BLK;  // ring: 2 x (K block, V block)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t seed = call_seed(a);
    const int nqb = S / BQ, nkb = S / BK;
    const int bh = blockIdx.x / nqb, qb = blockIdx.x - bh * nqb, b = bh / a.H, h = bh - b * a.H;
    const int D = a.H * DH, RS = 3 * D;  // qkv row stride (elements)
    const uint16_t *base = a.qkv + static_cast<int64_t>(b) * S * RS + h * DH;
    const int strd1[1] = {RS}, strd2[2] = {RS, RS};
    {
        const uint16_t *src[1] = {base + static_cast<int64_t>(qb) * BQ * RS};
        stage_images<BQ, 1>(Qi, src, strd1, wave, lane);
        const uint16_t *kv[2] = {base + D, base + 2 * D};
        stage_images<BK, 2>(ring, kv, strd2, wave, lane);
    }
    const int lg = lane >> 4, lc = lane & 15;
    const int q0 = wave * QW;
    float m_run[TQ], l_run[TQ];
    f32x4 o[4][TQ];  // O^T[d][q]: lane -> 4 consecutive d of one query
#pragma unroll
    for (int i = 0; i < TQ; ++i) {
        m_run[i] = -INFINITY, l_run[i] = 0.f;
#pragma unroll
        for (int c = 0; c < 4; ++c) o[c][i] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    for (int kb = 0; kb < nkb; ++kb) {
        wait_vmcnt<0>();
        __syncthreads();
        const uint8_t *Ki = ring + (kb & 1) * 2 * BLK, *Vi = Ki + BLK;
        if (kb + 1 < nkb) {
            const int64_t r0 = static_cast<int64_t>(kb + 1) * BK * RS;
            const uint16_t *kv[2] = {base + D + r0, base + 2 * D + r0};
            stage_images<BK, 2>(ring + ((kb + 1) & 1) * 2 * BLK, kv, strd2, wave, lane);
        }
        // acc[j][i]: keys 64 kb + 16 j + 4 lg + r of query q0 + 16 i + lc
        f32x4 acc[TK][TQ];
#pragma unroll
        for (int j = 0; j < TK; ++j)
#pragma unroll
            for (int i = 0; i < TQ; ++i) acc[j][i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < DH / 32; ++s) {
            bf16x8 qa[TQ], kf[TK];
#pragma unroll
            for (int i = 0; i < TQ; ++i) qa[i] = row_frag<128>(Qi, q0 + 16 * i, 32 * s, lane);
#pragma unroll
            for (int j = 0; j < TK; ++j) kf[j] = row_frag<128>(Ki, 16 * j, 32 * s, lane);
#pragma unroll
            for (int j = 0; j < TK; ++j)
#pragma unroll
                for (int i = 0; i < TQ; ++i) acc[j][i] = mfma(kf[j], qa[i], acc[j][i]);
        }
#pragma unroll
        for (int i = 0; i < TQ; ++i) {
            const int lrow = q0 + 16 * i + lc;   // row of the resident block
            const int row = qb * BQ + lrow;      // the query
            float m = m_run[i];
#pragma unroll
            for (int j = 0; j < TK; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) m = fmaxf(m, acc[j][i][r] * a.scale);
            m = fmaxf(m, __shfl_xor(m, 16));
            m = fmaxf(m, __shfl_xor(m, 32));
            const float alpha = __expf(m_run[i] - m);  // 0 at the first block (m_run = -inf)
            float sum = 0.f;
#pragma unroll
            for (int j = 0; j < TK; ++j) {
                const int kb0 = 16 * j + 4 * lg;
                float p[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float e = __expf(acc[j][i][r] * a.scale - m);
                    sum += e;
                    p[r] = keep_elem(seed, bh, row, kb * BK + kb0 + r, a.thresh) ? e * a.inv_keep : 0.f;
                }
                *reinterpret_cast<uint2 *>(Pi + off<128>(lrow, kb0)) = make_uint2(pack_bf16x2_hw(p[0], p[1]),
                                                                                  pack_bf16x2_hw(p[2], p[3]));
            }
            sum += __shfl_xor(sum, 16);
            sum += __shfl_xor(sum, 32);
            l_run[i] = l_run[i] * alpha + sum;
            m_run[i] = m;
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int r = 0; r < 4; ++r) o[c][i][r] *= alpha;
        }
        lds_wave_sync();
#pragma unroll
        for (int s = 0; s < BK / 32; ++s) {
            bf16x8 va[4], pb[TQ];
#pragma unroll
            for (int c = 0; c < 4; ++c) va[c] = tr_frag<128>(Vi, 32 * s, 16 * c, lane);
#pragma unroll
            for (int i = 0; i < TQ; ++i) pb[i] = row_frag<128>(Pi, q0 + 16 * i, 32 * s, lane);
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int i = 0; i < TQ; ++i) o[c][i] = mfma(va[c], pb[i], o[c][i]);
        }
    }
#pragma unroll
    for (int i = 0; i < TQ; ++i) {
        const int q = qb * BQ + q0 + 16 * i + lc;
        const float inv = 1.f / l_run[i];
        if (lg == 0) a.lse[static_cast<int64_t>(bh) * S + q] = m_run[i] + __logf(l_run[i]);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            uint16_t *dst = a.out + (static_cast<int64_t>(b) * S + q) * D + h * DH + 16 * c + 4 * lg;
            *reinterpret_cast<uint2 *>(dst) =
                make_uint2(pack_bf16x2_hw(o[c][i][0] * inv, o[c][i][1] * inv),
                           pack_bf16x2_hw(o[c][i][2] * inv, o[c][i][3] * inv));
        }
    }
}

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
// softmax is nearly one-hot).
__device__ __forceinline__ float bwd_block_dsum(const AttnArgs &a, uint32_t seed, int bh, const uint8_t *Qi,
                                                const uint8_t *Oi, const uint8_t *Ki, const uint8_t *Vi, int qw0,
                                                int row, int key0, float l, int lane) {
    const int lg = lane >> 4;
    f32x4 sc[TK], dp[TK];
    bwd_block_products(Qi, Oi, Ki, Vi, qw0, lane, sc, dp);
    float t = 0.f;
#pragma unroll
    for (int j = 0; j < TK; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float p = __expf(sc[j][r] * a.scale - l);
            if (keep_elem(seed, bh, row, key0 + 16 * j + 4 * lg + r, a.thresh)) t += p * dp[j][r];
        }
    return t * a.inv_keep;
}

// P and dS^T of the same 16 x 64 tile.  Writes dS (and P_drop when Pi) rows qw0 + lc of the images.
__device__ __forceinline__ void bwd_block_scores(const AttnArgs &a, uint32_t seed, int bh, const uint8_t *Qi,
                                                 const uint8_t *Oi, const uint8_t *Ki, const uint8_t *Vi, uint8_t *Pi,
                                                 uint8_t *Si, int qw0, int row, int key0, float l, float dd, int lane) {
    const int lg = lane >> 4, lc = lane & 15;
    f32x4 sc[TK], dp[TK];
    bwd_block_products(Qi, Oi, Ki, Vi, qw0, lane, sc, dp);
#pragma unroll
    for (int j = 0; j < TK; ++j) {
        const int kb0 = 16 * j + 4 * lg;
        float pv[4], sv[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float p = __expf(sc[j][r] * a.scale - l);
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

__global__ __launch_bounds__(256) void attn_long_dq_kernel(AttnArgs a, float *dsum_g, int S) {
    __shared__ __attribute__((aligned(1024))) uint8_t lds[7 * BLK];
    uint8_t *Qi = lds, *Oi = lds + BLK, *ring = lds + 2 * BLK, *Si = lds + 6 * BLK;  // Oi: dO; ring: 2 x (K, V)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t seed = call_seed(a);
    const int nb = S / BK;
    const int bh = blockIdx.x / nb, qb = blockIdx.x - bh * nb, b = bh / a.H, h = bh - b * a.H;
    const int D = a.H * DH, RS = 3 * D;
    const uint16_t *base = a.qkv + static_cast<int64_t>(b) * S * RS + h * DH;
    const uint16_t *dob = a.dout + static_cast<int64_t>(b) * S * D + h * DH;
    const int strd_kv[2] = {RS, RS};
    {
        const uint16_t *src[2] = {base + static_cast<int64_t>(qb) * BK * RS, dob + static_cast<int64_t>(qb) * BK * D};
        const int strd[2] = {RS, D};
        stage_images<BK, 2>(lds, src, strd, wave, lane);
        const uint16_t *kv[2] = {base + D, base + 2 * D};
        stage_images<BK, 2>(ring, kv, strd_kv, wave, lane);
    }
    const int lg = lane >> 4, lc = lane & 15;
    const int qw0 = wave * 16;           // this wave's rows of the resident block
    const int row = qb * BK + qw0 + lc;  // the query
    const float l = a.lse[static_cast<int64_t>(bh) * S + row];
    float dd = 0.f;  // D of the query: summed over the first pass, used by the second
    f32x4 o[4];      // dQ^T[d][q]
#pragma unroll
    for (int c = 0; c < 4; ++c) o[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    // the K / V blocks stream past twice: steps 0 .. nb - 1 sum D, steps nb .. 2 nb - 1 form dS and dQ
    for (int it = 0; it < 2 * nb; ++it) {
        wait_vmcnt<0>();
        __syncthreads();
        const int kb = it < nb ? it : it - nb;
        const uint8_t *Ki = ring + (it & 1) * 2 * BLK, *Vi = Ki + BLK;
        if (it + 1 < 2 * nb) {
            const int nx = it + 1 < nb ? it + 1 : it + 1 - nb;
            const int64_t r0 = static_cast<int64_t>(nx) * BK * RS;
            const uint16_t *kv[2] = {base + D + r0, base + 2 * D + r0};
            stage_images<BK, 2>(ring + ((it + 1) & 1) * 2 * BLK, kv, strd_kv, wave, lane);
        }
        if (it < nb) {
            dd += bwd_block_dsum(a, seed, bh, Qi, Oi, Ki, Vi, qw0, row, kb * BK, l, lane);
            if (it == nb - 1) {  // the query's four lanes (lg) hold 16 keys of every block each
                dd += __shfl_xor(dd, 16);
                dd += __shfl_xor(dd, 32);
                if (lg == 0) dsum_g[static_cast<int64_t>(bh) * S + row] = dd;
            }
            continue;
        }
        bwd_block_scores(a, seed, bh, Qi, Oi, Ki, Vi, nullptr, Si, qw0, row, kb * BK, l, dd, lane);
        lds_wave_sync();
        // dQ^T[d][q] += sum_key K[key][d] dS[q][key]
#pragma unroll
        for (int s = 0; s < BK / 32; ++s) {
            bf16x8 ka[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) ka[c] = tr_frag<128>(Ki, 32 * s, 16 * c, lane);
            const bf16x8 sb = row_frag<128>(Si, qw0, 32 * s, lane);
#pragma unroll
            for (int c = 0; c < 4; ++c) o[c] = mfma(ka[c], sb, o[c]);
        }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        uint16_t *dst = a.dqkv + (static_cast<int64_t>(b) * S + row) * RS + h * DH + 16 * c + 4 * lg;
        *reinterpret_cast<uint2 *>(dst) =
            make_uint2(pack_bf16x2_hw(o[c][0] * a.scale, o[c][1] * a.scale),
                       pack_bf16x2_hw(o[c][2] * a.scale, o[c][3] * a.scale));
    }
}

__global__ __launch_bounds__(256) void attn_long_dkv_kernel(AttnArgs a, const float *dsum_g, int S) {
    __shared__ __attribute__((aligned(1024))) uint8_t lds[8 * BLK];
    uint8_t *Ki = lds, *Vi = lds + BLK, *ring = lds + 2 * BLK;  // ring: 2 x (Q block, dO block)
    uint8_t *Pi = lds + 6 * BLK, *Si = lds + 7 * BLK;           // P_drop, dS: [query][key]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t seed = call_seed(a);
    const int nb = S / BK;
    const int bh = blockIdx.x / nb, kbk = blockIdx.x - bh * nb, b = bh / a.H, h = bh - b * a.H;
    const int D = a.H * DH, RS = 3 * D;
    const uint16_t *base = a.qkv + static_cast<int64_t>(b) * S * RS + h * DH;
    const uint16_t *dob = a.dout + static_cast<int64_t>(b) * S * D + h * DH;
    const int strd_qo[2] = {RS, D};
    {
        const int64_t r0 = static_cast<int64_t>(kbk) * BK * RS;
        const uint16_t *kv[2] = {base + D + r0, base + 2 * D + r0};
        const int strd[2] = {RS, RS};
        stage_images<BK, 2>(lds, kv, strd, wave, lane);
        const uint16_t *qo[2] = {base, dob};
        stage_images<BK, 2>(ring, qo, strd_qo, wave, lane);
    }
    const int lg = lane >> 4, lc = lane & 15;
    const int w0 = wave * 16;  // this wave's queries of the streamed block (scores) and keys of the resident one (sums)
    f32x4 dv[4], dk[4];        // dV^T[d][key], dK^T[d][key]
#pragma unroll
    for (int c = 0; c < 4; ++c) dv[c] = dk[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int qb = 0; qb < nb; ++qb) {
        const int row = qb * BK + w0 + lc;  // the query
        const float l = a.lse[static_cast<int64_t>(bh) * S + row];
        const float dd = dsum_g[static_cast<int64_t>(bh) * S + row];
        wait_vmcnt<0>();
        __syncthreads();
        const uint8_t *Qi = ring + (qb & 1) * 2 * BLK, *Oi = Qi + BLK;
        if (qb + 1 < nb) {
            const uint16_t *qo[2] = {base + static_cast<int64_t>(qb + 1) * BK * RS,
                                     dob + static_cast<int64_t>(qb + 1) * BK * D};
            stage_images<BK, 2>(ring + ((qb + 1) & 1) * 2 * BLK, qo, strd_qo, wave, lane);
        }
        bwd_block_scores(a, seed, bh, Qi, Oi, Ki, Vi, Pi, Si, w0, row, kbk * BK, l, dd, lane);
        lds_barrier();
        // dV^T[d][key] += sum_q dO[q][d] P_drop[q][key]; dK^T[d][key] += sum_q Q[q][d] dS[q][key]
#pragma unroll
        for (int s = 0; s < BK / 32; ++s) {
            bf16x8 ga[4], qa[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                ga[c] = tr_frag<128>(Oi, 32 * s, 16 * c, lane);
                qa[c] = tr_frag<128>(Qi, 32 * s, 16 * c, lane);
            }
            const bf16x8 pb = tr_frag<128>(Pi, 32 * s, w0, lane);
            const bf16x8 sb = tr_frag<128>(Si, 32 * s, w0, lane);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                dv[c] = mfma(ga[c], pb, dv[c]);
                dk[c] = mfma(qa[c], sb, dk[c]);
            }
        }
    }
    const int key = kbk * BK + w0 + lc;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        uint16_t *rowp = a.dqkv + (static_cast<int64_t>(b) * S + key) * RS + h * DH + 16 * c + 4 * lg;
        *reinterpret_cast<uint2 *>(rowp + D) =
            make_uint2(pack_bf16x2_hw(dk[c][0] * a.scale, dk[c][1] * a.scale),
                       pack_bf16x2_hw(dk[c][2] * a.scale, dk[c][3] * a.scale));
        *reinterpret_cast<uint2 *>(rowp + 2 * D) = make_uint2(pack_bf16x2_hw(dv[c][0], dv[c][1]),
                                                              pack_bf16x2_hw(dv[c][2], dv[c][3]));
    }
}

}  // namespace

bool attention_long_supported(int S) { return S % BK == 0 && S >= 2 * BK && S <= 512; }

void launch_attention_long_forward(const uint16_t *qkv, uint16_t *out, float *lse, int B, int S, int H, float scale,
                                   uint32_t seed, float p_drop, hipStream_t s) {
    if (!attention_long_supported(S)) throw std::invalid_argument("attention: the streaming kernels need S % 64 == 0, 128 <= S <= 512");
    const AttnArgs a = make_args(qkv, out, lse, nullptr, nullptr, H, scale, seed, p_drop);
    if (S % 128 == 0) attn_long_fwd_kernel<128><<<B * H * (S / 128), 256, 0, s>>>(a, S);
    else attn_long_fwd_kernel<64><<<B * H * (S / 64), 256, 0, s>>>(a, S);
}

void launch_attention_long_backward(const uint16_t *qkv, const uint16_t *out, const float *lse, const uint16_t *dout,
                                    uint16_t *dqkv, float *dsum, int B, int S, int H, float scale, uint32_t seed,
                                    float p_drop, hipStream_t s) {
    if (!attention_long_supported(S)) throw std::invalid_argument("attention: the streaming kernels need S % 64 == 0, 128 <= S <= 512");
    if (!dsum) throw std::invalid_argument("attention: the streaming backward needs the [B, H, S] f32 dsum buffer");
    const AttnArgs a = make_args(qkv, const_cast<uint16_t *>(out), const_cast<float *>(lse), dout, dqkv, H, scale, seed,
                                 p_drop);
    const int grid = B * H * (S / BK);
    attn_long_dq_kernel<<<grid, 256, 0, s>>>(a, dsum, S);   // fills dsum
    attn_long_dkv_kernel<<<grid, 256, 0, s>>>(a, dsum, S);  // reads it (stream order)
}

}  // namespace kfk
