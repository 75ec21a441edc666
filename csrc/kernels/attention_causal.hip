// Causal fused multi-head self-attention (query q attends to keys k <= q): the streaming kernels of
// attention_long.hip with triangular trip counts (S = 64 .. 1024 in steps of 64, head dim 64, bf16, dropout).
//
// Same interface, LDS images, MFMA fragment layouts, two-slot LDS-DMA ring and wait / barrier / prefetch /
// compute step as attention_long.hip (see its header), same keep_elem hash on the global (query, key) index
// (the hash packs q << 16 | k: S <= 1024 leaves room).  No atomics, no zeroed scratch, no workgroup waits on
// another: bitwise reproducible.  What is different:
//   which blocks  All blocks are 64 rows (BQ = BK = 64), so query block i needs key blocks 0 .. i and key
//                 block j is needed by query blocks j .. n - 1 (n = S / 64).  Blocks outside that range are
//                 never staged: about half of the DMA and MFMA work of the bidirectional call, (n + 1) / 2n.
//   the mask      Only the diagonal block (key block == query block) holds keys beyond a query.  It is the
//                 LAST block of the forward's and the dQ kernel's stream and the FIRST of the dK/dV kernel's,
//                 peeled out of the loop; every other step is the unmasked code.
//                 Forward: scores with key > query become -inf before the running max.  Every row sees its own
//                 key in the diagonal block, and for query blocks > 0 the max is already finite when the first
//                 masked score arrives, so exp(-inf - m) = 0 exactly and no row is empty.  The diagonal block's
//                 P V product keeps each wave's 16 x 16 triangle out of the MFMA (pv_diagonal): a V row of a
//                 masked key is never multiplied with an earlier query's 0, so NaN or inf in future rows of V
//                 cannot reach the output.  (The backward has no such guard: its dP = dO V^T is one MFMA.)
//                 Backward: bwd_block_dsum / bwd_block_scores <true> of attention_stream.hpp zero P for
//                 keys >= L, and L is a per-lane argument: L = query + 1 is the causal mask.
//   BQ            64 only: one diagonal block, all four waves do the same work.  (A 128-row query block has two
//                 diagonal blocks of which half the waves skip one; not built, profiles/attention_causal.md.)
//   work order    Query block i takes i + 1 steps (forward; dQ: 2 (i + 1)), key block j takes n - j (dK/dV).
//                 blockIdx.x is block-major, (sequence, head)-minor, heaviest block first (descending query
//                 block in the forward and dQ, ascending key block in dK/dV), so the tail of the grid is made
//                 of short workgroups.  `plain` selects the (sequence, head)-major ascending order of the
//                 bidirectional kernels instead (tools/bench_attention.py measures one against the other).
//
// Rows read or staged, by hand (n = S / 64; a block b is rows 64 b .. 64 b + 63, inside [0, S) iff 0 <= b < n):
//   forward, dQ   resident: Q (and dO) block qb.  Streamed K / V: first block 0, last block qb (the prefetch
//                 of step kb stages block kb + 1 only if kb + 1 <= qb; the dQ kernel's second pass starts over
//                 at block 0).  qb = 0: block 0 only, no prefetch (dQ: block 0 twice).  qb = n - 1: blocks
//                 0 .. n - 1.  S = 64: n = 1, qb = 0, block 0 only.  lse / dsum rows: 64 qb + 0 .. 63.
//   dK/dV         resident: K, V block kbk.  Streamed Q / dO, lse and dsum rows: first block kbk, last block
//                 n - 1 (the prefetch of step qb stages qb + 1 only if qb + 1 <= n - 1).  kbk = 0: blocks
//                 0 .. n - 1.  kbk = n - 1: block n - 1 only, no prefetch.  S = 64: block 0 only.
//   dsum          The dQ kernel writes all 64 rows of its block and every block has a workgroup: all S rows are
//                 written before the dK/dV kernel (stream order) reads rows >= 64 kbk.
//
// The backward's per-block helpers are the templates of attention_stream.hpp; the forward's block step is a copy of
// attn_long_fwd_kernel's loop body with the mask added, as in attention_lengths.hip and for the same reason
// (calling one shared template from the old kernel changes that kernel's schedule and registers).
//
// Compiled without packed f32 instructions (KFK_NO_PK_F32: v_pk_add / mul / fma_f32 become their scalar forms,
// the same IEEE results), the precaution attention_lengths.hip's header explains.
#include "attention_stream.hpp"

#include <stdexcept>

namespace kfk {

namespace {

// blockIdx.x -> (sequence * heads + head, 64-row block): heaviest-first, or (plain) the order of the
// bidirectional kernels.  `descending`: the heaviest block is the last one (forward, dQ), else the first (dK/dV).
__device__ __forceinline__ void block_of(int n, bool plain, bool descending, int &bh, int &blk) {
    if (plain) {
        bh = blockIdx.x / n, blk = blockIdx.x - bh * n;
    } else {
        const int nbh = gridDim.x / n, rank = blockIdx.x / nbh;
        bh = blockIdx.x - rank * nbh, blk = descending ? n - 1 - rank : rank;
    }
}

// The diagonal block's O^T += V^T P^T for this wave's 16 queries (rows q0 .. q0 + 15 of the block; P in Pi).  A
// masked probability is exactly 0, but an MFMA product over its key would still multiply it with that key's V row,
// and 0 * NaN = NaN: a V row must not meet an earlier query at all.  So the block's keys are split three ways:
//   keys < q0            visible to all 16 queries: the MFMA.  Its K index spans 32 keys; where the upper 16 of them
//                        are the triangle's (q0 = 16, 48) the V operand is zeroed in the lanes that hold them
//                        (lane >> 4 >= 2: keys 32 s + 16 ..), and P there is finite.
//   keys q0 .. q0 + 15   the 16 x 16 triangle, on the VALU: the lane of query q0 + lc (d = 16 c + 4 lg + r, the
//                        MFMA's own accumulator layout) adds key q0 + kk only if kk <= lc.
//   keys >= q0 + 16      beyond every query of the wave: not read.
// The choice is wave-uniform; P rows stay in their wave as before.
__device__ __forceinline__ void pv_diagonal(const uint8_t *Vi, const uint8_t *Pi, int q0, int lane, f32x4 (&o)[4]) {
    const int lg = lane >> 4, lc = lane & 15;
    const int qu = __builtin_amdgcn_readfirstlane(q0);
#pragma unroll
    for (int s = 0; s < BK / 32; ++s) {
        if (32 * s + 16 > qu) continue;
        const bool half = 32 * s + 32 > qu;
        bf16x8 va[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            va[c] = tr_frag<128>(Vi, 32 * s, 16 * c, lane);
            if (half && lg >= 2) va[c] = __builtin_bit_cast(bf16x8, make_uint4(0, 0, 0, 0));
        }
        const bf16x8 pb = row_frag<128>(Pi, qu, 32 * s, lane);
#pragma unroll
        for (int c = 0; c < 4; ++c) o[c] = mfma(va[c], pb, o[c]);
    }
    const uint8_t *prow = Pi + off<128>(qu + lc, qu);  // P[query][keys q0 .. q0 + 15]: 32 contiguous bytes
    const uint4 plo = *reinterpret_cast<const uint4 *>(prow), phi = *reinterpret_cast<const uint4 *>(prow + 16);
    const uint32_t pw[8] = {plo.x, plo.y, plo.z, plo.w, phi.x, phi.y, phi.z, phi.w};
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) {
        const float p = kk & 1 ? bf16_hi(pw[kk >> 1]) : bf16_lo(pw[kk >> 1]);
        if (kk <= lc) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const uint2 v = *reinterpret_cast<const uint2 *>(Vi + off<128>(qu + kk, 16 * c + 4 * lg));
                o[c][0] = fmaf(p, bf16_lo(v.x), o[c][0]);
                o[c][1] = fmaf(p, bf16_hi(v.x), o[c][1]);
                o[c][2] = fmaf(p, bf16_lo(v.y), o[c][2]);
                o[c][3] = fmaf(p, bf16_hi(v.y), o[c][3]);
            }
        }
    }
}

// One step of the forward's block loop on the staged key block at key0 for this wave's 16 queries (rows q0 .. of
// the resident block, query `row` in this lane): attn_long_fwd_kernel's arithmetic at BQ = 64; MASK sets the
// scores of keys > row to -inf first.
template <bool MASK>
__device__ __forceinline__ void fwd_block(const AttnArgs &a, uint32_t seed, int bh, const uint8_t *Qi, const uint8_t *Ki,
                                          const uint8_t *Vi, uint8_t *Pi, int q0, int row, int key0, int lane,
                                          float &m_run, float &l_run, f32x4 (&o)[4]) {
    const int lg = lane >> 4, lc = lane & 15;
    // acc[j]: keys key0 + 16 j + 4 lg + r of query row
    f32x4 acc[TK];
#pragma unroll
    for (int j = 0; j < TK; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < DH / 32; ++s) {
        const bf16x8 qa = row_frag<128>(Qi, q0, 32 * s, lane);
        bf16x8 kf[TK];
#pragma unroll
        for (int j = 0; j < TK; ++j) kf[j] = row_frag<128>(Ki, 16 * j, 32 * s, lane);
#pragma unroll
        for (int j = 0; j < TK; ++j) acc[j] = mfma(kf[j], qa, acc[j]);
    }
    if constexpr (MASK) {
#pragma unroll
        for (int j = 0; j < TK; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[j][r] = key0 + 16 * j + 4 * lg + r > row ? -INFINITY : acc[j][r];
    }
    const int lrow = q0 + lc;  // row of the resident block
    float m = m_run;
#pragma unroll
    for (int j = 0; j < TK; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) m = fmaxf(m, acc[j][r] * a.scale);
    m = fmaxf(m, __shfl_xor(m, 16));
    m = fmaxf(m, __shfl_xor(m, 32));
    const float alpha = __expf(m_run - m);  // 0 at the first block (m_run = -inf, m finite: key key0 <= row)
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < TK; ++j) {
        const int kb0 = 16 * j + 4 * lg;
        float p[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float e = __expf(acc[j][r] * a.scale - m);
            sum += e;
            p[r] = keep_elem(seed, bh, row, key0 + kb0 + r, a.thresh) ? e * a.inv_keep : 0.f;
        }
        *reinterpret_cast<uint2 *>(Pi + off<128>(lrow, kb0)) = make_uint2(pack_bf16x2_hw(p[0], p[1]),
                                                                          pack_bf16x2_hw(p[2], p[3]));
    }
    sum += __shfl_xor(sum, 16);
    sum += __shfl_xor(sum, 32);
    l_run = l_run * alpha + sum;
    m_run = m;
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int r = 0; r < 4; ++r) o[c][r] *= alpha;
    lds_wave_sync();
    if constexpr (MASK) {
        pv_diagonal(Vi, Pi, q0, lane, o);
    } else {
#pragma unroll
        for (int s = 0; s < BK / 32; ++s) {
            bf16x8 va[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) va[c] = tr_frag<128>(Vi, 32 * s, 16 * c, lane);
            const bf16x8 pb = row_frag<128>(Pi, q0, 32 * s, lane);
#pragma unroll
            for (int c = 0; c < 4; ++c) o[c] = mfma(va[c], pb, o[c]);
        }
    }
}

KFK_NO_PK_F32 __global__ __launch_bounds__(256) void attn_causal_fwd_kernel(AttnArgs a, int S, bool plain) {
    __shared__ __attribute__((aligned(1024))) uint8_t lds[6 * BLK];
    uint8_t *Qi = lds, *ring = lds + BLK, *Pi = ring + 4 * BLK;  // ring: 2 x (K block, V block)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int bh, qb;
    block_of(S / BK, plain, true, bh, qb);
    const int b = bh / a.H, h = bh - b * a.H;
    const int D = a.H * DH, RS = 3 * D;  // qkv row stride (elements)
    const uint32_t seed = call_seed(a);
    const uint16_t *base = a.qkv + static_cast<int64_t>(b) * S * RS + h * DH;
    const int strd1[1] = {RS}, strd2[2] = {RS, RS};
    {
        const uint16_t *src[1] = {base + static_cast<int64_t>(qb) * BK * RS};
        stage_images<BK, 1>(Qi, src, strd1, wave, lane);
        const uint16_t *kv[2] = {base + D, base + 2 * D};
        stage_images<BK, 2>(ring, kv, strd2, wave, lane);
    }
    const int lg = lane >> 4, lc = lane & 15;
    const int q0 = wave * 16;
    const int row = qb * BK + q0 + lc;  // the query
    float m_run = -INFINITY, l_run = 0.f;
    f32x4 o[4];  // O^T[d][q]: lane -> 4 consecutive d of one query
#pragma unroll
    for (int c = 0; c < 4; ++c) o[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    // key blocks 0 .. qb - 1 lie wholly below the diagonal: the unmasked step; block kb + 1 <= qb always exists
    for (int kb = 0; kb < qb; ++kb) {
        wait_vmcnt<0>();
        __syncthreads();
        const uint8_t *Ki = ring + (kb & 1) * 2 * BLK, *Vi = Ki + BLK;
        const int64_t r0 = static_cast<int64_t>(kb + 1) * BK * RS;
        const uint16_t *kv[2] = {base + D + r0, base + 2 * D + r0};
        stage_images<BK, 2>(ring + ((kb + 1) & 1) * 2 * BLK, kv, strd2, wave, lane);
        fwd_block<false>(a, seed, bh, Qi, Ki, Vi, Pi, q0, row, kb * BK, lane, m_run, l_run, o);
    }
    {  // the diagonal block qb, last: nothing left to prefetch
        wait_vmcnt<0>();
        __syncthreads();
        const uint8_t *Ki = ring + (qb & 1) * 2 * BLK, *Vi = Ki + BLK;
        fwd_block<true>(a, seed, bh, Qi, Ki, Vi, Pi, q0, row, qb * BK, lane, m_run, l_run, o);
    }
    const float inv = 1.f / l_run;  // l_run >= 1: the row's own key
    if (lg == 0) a.lse[static_cast<int64_t>(bh) * S + row] = m_run + __logf(l_run);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        uint16_t *dst = a.out + (static_cast<int64_t>(b) * S + row) * D + h * DH + 16 * c + 4 * lg;
        *reinterpret_cast<uint2 *>(dst) = make_uint2(pack_bf16x2_hw(o[c][0] * inv, o[c][1] * inv),
                                                     pack_bf16x2_hw(o[c][2] * inv, o[c][3] * inv));
    }
}

KFK_NO_PK_F32 __global__ __launch_bounds__(256) void attn_causal_dq_kernel(AttnArgs a, float *dsum_g, int S, bool plain) {
    __shared__ __attribute__((aligned(1024))) uint8_t lds[7 * BLK];
    uint8_t *Qi = lds, *Oi = lds + BLK, *ring = lds + 2 * BLK, *Si = lds + 6 * BLK;  // Oi: dO; ring: 2 x (K, V)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int bh, qb;
    block_of(S / BK, plain, true, bh, qb);
    const int b = bh / a.H, h = bh - b * a.H;
    const int D = a.H * DH, RS = 3 * D;
    const int nb = qb + 1;  // streamed key blocks 0 .. qb
    const uint32_t seed = call_seed(a);
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
    const int row = qb * BK + qw0 + lc;  // the query: keys >= row + 1 are masked
    const float l = a.lse[static_cast<int64_t>(bh) * S + row];
    float dd = 0.f;  // D of the query: summed over the first pass, used by the second
    f32x4 o[4];      // dQ^T[d][q]
#pragma unroll
    for (int c = 0; c < 4; ++c) o[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    // the K / V blocks stream past twice: steps 0 .. nb - 1 sum D, steps nb .. 2 nb - 1 form dS and dQ;
    // the last step of each pass is the diagonal block
    for (int it = 0; it < 2 * nb; ++it) {
        wait_vmcnt<0>();
        __syncthreads();
        const int kb = it < nb ? it : it - nb;
        const bool diag = kb == qb;
        const uint8_t *Ki = ring + (it & 1) * 2 * BLK, *Vi = Ki + BLK;
        if (it + 1 < 2 * nb) {
            const int nx = it + 1 < nb ? it + 1 : it + 1 - nb;  // <= qb
            const int64_t r0 = static_cast<int64_t>(nx) * BK * RS;
            const uint16_t *kv[2] = {base + D + r0, base + 2 * D + r0};
            stage_images<BK, 2>(ring + ((it + 1) & 1) * 2 * BLK, kv, strd_kv, wave, lane);
        }
        if (it < nb) {
            dd += diag ? bwd_block_dsum<true>(a, seed, bh, Qi, Oi, Ki, Vi, qw0, row, kb * BK, l, lane, row + 1)
                       : bwd_block_dsum<false>(a, seed, bh, Qi, Oi, Ki, Vi, qw0, row, kb * BK, l, lane);
            if (diag) {  // the query's four lanes (lg) hold 16 keys of every block each
                dd += __shfl_xor(dd, 16);
                dd += __shfl_xor(dd, 32);
                if (lg == 0) dsum_g[static_cast<int64_t>(bh) * S + row] = dd;
            }
            continue;
        }
        if (diag) bwd_block_scores<true>(a, seed, bh, Qi, Oi, Ki, Vi, nullptr, Si, qw0, row, kb * BK, l, dd, lane, row + 1);
        else bwd_block_scores<false>(a, seed, bh, Qi, Oi, Ki, Vi, nullptr, Si, qw0, row, kb * BK, l, dd, lane);
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
        *reinterpret_cast<uint2 *>(dst) = make_uint2(pack_bf16x2_hw(o[c][0] * a.scale, o[c][1] * a.scale),
                                                     pack_bf16x2_hw(o[c][2] * a.scale, o[c][3] * a.scale));
    }
}

// The dK/dV steps on the streamed query blocks qb0 .. qb1 - 1 of nbs; the ring slot of block qb is
// (qb - kbk) & 1.  MASK: the diagonal block (qb == kbk: keys beyond a query give P = dS = 0), chosen outside.
template <bool MASK>
__device__ __forceinline__ void dkv_loop(const AttnArgs &a, const float *dsum_g, uint32_t seed, int bh, int S, int qb0,
                                         int qb1, int kbk, const uint16_t *base, const uint16_t *dob, uint8_t *lds,
                                         int wave, int lane, f32x4 (&dv)[4], f32x4 (&dk)[4]) {
    uint8_t *Ki = lds, *Vi = lds + BLK, *ring = lds + 2 * BLK, *Pi = lds + 6 * BLK, *Si = lds + 7 * BLK;
    const int D = a.H * DH, RS = 3 * D, nbs = S / BK;
    const int strd_qo[2] = {RS, D};
    const int lc = lane & 15, w0 = wave * 16;
    for (int qb = qb0; qb < qb1; ++qb) {
        const int row = qb * BK + w0 + lc;  // the query, < S
        const float l = a.lse[static_cast<int64_t>(bh) * S + row];
        const float dd = dsum_g[static_cast<int64_t>(bh) * S + row];
        wait_vmcnt<0>();
        __syncthreads();
        const uint8_t *Qi = ring + ((qb - kbk) & 1) * 2 * BLK, *Oi = Qi + BLK;
        if (qb + 1 < nbs) {
            const uint16_t *qo[2] = {base + static_cast<int64_t>(qb + 1) * BK * RS,
                                     dob + static_cast<int64_t>(qb + 1) * BK * D};
            stage_images<BK, 2>(ring + ((qb + 1 - kbk) & 1) * 2 * BLK, qo, strd_qo, wave, lane);
        }
        bwd_block_scores<MASK>(a, seed, bh, Qi, Oi, Ki, Vi, Pi, Si, w0, row, kbk * BK, l, dd, lane, row + 1);
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
}

KFK_NO_PK_F32 __global__ __launch_bounds__(256) void attn_causal_dkv_kernel(AttnArgs a, const float *dsum_g, int S, bool plain) {
    __shared__ __attribute__((aligned(1024))) uint8_t lds[8 * BLK];  // K, V resident; ring 2 x (Q, dO); P_drop; dS
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nbs = S / BK;
    int bh, kbk;
    block_of(nbs, plain, false, bh, kbk);
    const int b = bh / a.H, h = bh - b * a.H;
    const int D = a.H * DH, RS = 3 * D;
    const uint32_t seed = call_seed(a);
    const uint16_t *base = a.qkv + static_cast<int64_t>(b) * S * RS + h * DH;
    const uint16_t *dob = a.dout + static_cast<int64_t>(b) * S * D + h * DH;
    {
        const int64_t r0 = static_cast<int64_t>(kbk) * BK * RS;
        const uint16_t *kv[2] = {base + D + r0, base + 2 * D + r0};
        const int strd[2] = {RS, RS};
        stage_images<BK, 2>(lds, kv, strd, wave, lane);
        const uint16_t *qo[2] = {base + r0, dob + static_cast<int64_t>(kbk) * BK * D};  // the diagonal block first
        const int strd_qo[2] = {RS, D};
        stage_images<BK, 2>(lds + 2 * BLK, qo, strd_qo, wave, lane);
    }
    const int lg = lane >> 4, lc = lane & 15;
    const int w0 = wave * 16;  // this wave's queries of the streamed block (scores) and keys of the resident one (sums)
    f32x4 dv[4], dk[4];        // dV^T[d][key], dK^T[d][key]
#pragma unroll
    for (int c = 0; c < 4; ++c) dv[c] = dk[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    dkv_loop<true>(a, dsum_g, seed, bh, S, kbk, kbk + 1, kbk, base, dob, lds, wave, lane, dv, dk);
    dkv_loop<false>(a, dsum_g, seed, bh, S, kbk + 1, nbs, kbk, base, dob, lds, wave, lane, dv, dk);
    uint16_t *dkv0 = a.dqkv + (static_cast<int64_t>(b) * S + kbk * BK) * RS + h * DH;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        uint16_t *rowp = dkv0 + static_cast<int64_t>(w0 + lc) * RS + 16 * c + 4 * lg;
        *reinterpret_cast<uint2 *>(rowp + D) = make_uint2(pack_bf16x2_hw(dk[c][0] * a.scale, dk[c][1] * a.scale),
                                                          pack_bf16x2_hw(dk[c][2] * a.scale, dk[c][3] * a.scale));
        *reinterpret_cast<uint2 *>(rowp + 2 * D) = make_uint2(pack_bf16x2_hw(dv[c][0], dv[c][1]),
                                                              pack_bf16x2_hw(dv[c][2], dv[c][3]));
    }
}

void check(int S) {
    if (!attention_causal_supported(S))
        throw std::invalid_argument("attention: causal needs S % 64 == 0, 64 <= S <= 1024");
}

}  // namespace

bool attention_causal_supported(int S) { return S >= 64 && S <= 1024 && S % 64 == 0; }

void launch_attention_causal_forward(const uint16_t *qkv, uint16_t *out, float *lse, int B, int S, int H, float scale,
                                     uint32_t seed, float p_drop, hipStream_t s, bool plain_order) {
    check(S);
    const AttnArgs a = make_args(qkv, out, lse, nullptr, nullptr, H, scale, seed, p_drop);
    attn_causal_fwd_kernel<<<B * H * (S / BK), 256, 0, s>>>(a, S, plain_order);
}

void launch_attention_causal_backward(const uint16_t *qkv, const uint16_t *out, const float *lse, const uint16_t *dout,
                                      uint16_t *dqkv, float *dsum, int B, int S, int H, float scale, uint32_t seed,
                                      float p_drop, hipStream_t s, bool plain_order) {
    check(S);
    if (!dsum) throw std::invalid_argument("attention: the streaming backward needs the [B, H, S] f32 dsum buffer");
    const AttnArgs a = make_args(qkv, const_cast<uint16_t *>(out), const_cast<float *>(lse), dout, dqkv, H, scale, seed,
                                 p_drop);
    const int grid = B * H * (S / BK);
    attn_causal_dq_kernel<<<grid, 256, 0, s>>>(a, dsum, S, plain_order);   // fills all S rows of dsum
    attn_causal_dkv_kernel<<<grid, 256, 0, s>>>(a, dsum, S, plain_order);  // reads them (stream order)
}

}  // namespace kfk
