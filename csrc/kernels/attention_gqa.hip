// Grouped-query attention at head dim 128 (LLaMA-2 70B and later, Mistral; one K/V head: multi-query attention):
// H query heads share Hkv = H / G key/value heads, query head h reads K/V head h / G.  Streaming kernels on
// attention_d128.hpp's block steps, bidirectional or causal (template parameter CAUSAL), S = 64 .. 1024 in steps of
// 64, bf16, dropout.  G is a run-time value: every H % Hkv == 0 is served by the same three kernels.
//
// Interface    qkv [B, S, (H + 2 Hkv) * 128], the output of one Linear(d, (H + 2 Hkv) * 128): a row holds the H query
//              heads, then the Hkv key heads, then the Hkv value heads, 128 bf16 each.  Q of head h is at column
//              h * 128, K at (H + h / G) * 128, V at (H + Hkv + h / G) * 128; row stride RS = (H + 2 Hkv) * 128.
//              out [B, S, H, 128]; lse and dsum [B, H, S] f32 per query head; dqkv in qkv's layout, every element
//              written once.  The keep_elem hash is keyed on the query head: (seed, b * H + h, query, key).  At
//              Hkv = H this is attention_d128.hip's layout and its results bit for bit (same arithmetic per query head,
//              same order of accumulation).  No atomics, no zeroed scratch, no workgroup waits on another: bitwise
//              reproducible.  No per-sequence lengths.  The argument block is attention_common.hpp's with H the query
//              heads; Hkv is a kernel argument of its own.
// Work split   Forward and dQ: one workgroup (4 waves) per (sequence, query head, 64-row query block), wave w owns
//              rows 16 w .. 16 w + 15, its Q (and dO) rows in registers, the K / V blocks of head h / G stream through
//              a 2-slot ring: attention_d128.hip's kernels on the grouped addressing.
//              dK/dV: one workgroup per (sequence, K/V head, 64-row key block): B * Hkv * n workgroups, not B * H * n.
//              K and V of the block stay resident in LDS, and the 16 accumulator tiles (dV^T and dK^T, 128 d x 16 keys
//              per wave) stay in registers while the (Q, dO) blocks of the whole group stream past: the G query heads
//              are summed in f32 in those registers and rounded to bf16 once, at the single store.  No partial
//              buffers, no second pass, no atomics.
// Grid order   The G workgroups of the forward and of dQ that stream the same K/V head are neighbours in dispatch:
//              within a block rank the heads run in ascending order, so a group's G heads are adjacent.  They walk the
//              same K/V blocks at the same pace: a block comes from HBM once per group and the other G - 1 workgroups
//              find it in L2.
//                causal         block-major, heaviest query block (n - 1) first; inside a rank b * H + h ascending
//                bidirectional  (sequence, K/V head)-major; inside a group block-major, the G heads of a block adjacent
//              dK/dV: causal block-major, heaviest key block (0) first; bidirectional (sequence, K/V head)-major.
// LDS          As attention_d128.hip, dynamic (raised at first launch): forward and dQ 72 KB (ring 2 x (K, V) 64 KB +
//              P or dS 8 KB), dK/dV 112 KB (K, V resident 32 KB + ring 2 x (Q, dO) 64 KB + P, dS 16 KB): the group
//              adds no byte, its heads reuse the ring.
// dK/dV stream One stream of G * (n - first) steps through the 2-slot ring (first = kbk when causal, 0 otherwise):
//              step t is query head hk * G + t / (n - first), query block first + t % (n - first); heads ascending,
//              blocks ascending inside a head; ring slot t & 1.  Each step: wait for its DMA, workgroup barrier, start
//              the DMA of step t + 1 into the other slot, compute.  The prefetch of a head's last block stages the
//              next head's block `first`, so the ring never drains at a head boundary.  lse and dsum rows and the
//              hash's b * H + h follow the streamed head.
// Causal       Forward and dQ: key blocks 0 .. qb, only the diagonal block (the last step) masked; pv_diagonal keeps
//              each wave's 16 x 16 triangle off the MFMA, so NaN or inf in future V rows cannot reach earlier queries.
//              dK/dV: the diagonal block is the first step of every head's sub-stream, G times per workgroup: each
//              head runs one masked step (dkv_step<true>) and then its loop of unmasked ones (dkv_step<false>), so the
//              unmasked steps carry no mask code.
//
// Rows read or staged, by hand (n = S / 64; block b is rows 64 b .. 64 b + 63, inside [0, S) iff 0 <= b < n;
// `last` = qb when causal, n - 1 when not; `first` = kbk when causal, 0 when not; hk = h / G < Hkv):
//   forward, dQ   as attention_d128.hip: registers Q (and dO), lse rows 64 qb + 16 w + 0 .. 15; streamed K / V blocks
//                 0 .. `last` of head hk (the prefetch of step kb stages kb + 1 only if kb + 1 <= last; dQ twice).
//                   S = 64         n = 1, block 0 only (dQ: twice).
//   dK/dV         resident: K, V block kbk = 0 .. n - 1 of head hk.  Streamed Q / dO, lse and dsum rows:
//                   first step     t = 0: head hk * G, block `first`, staged before the loop into slot 0.
//                   inside a head  the prefetch of (head, qb) with qb < n - 1 stages (head, qb + 1), qb + 1 <= n - 1.
//                   head boundary  the prefetch of (head, n - 1) with head < hk * G + G - 1 stages (head + 1, first);
//                                  head + 1 <= hk * G + G - 1 <= H - 1.
//                   last step      head hk * G + G - 1, block n - 1: t + 1 = G * (n - first), no prefetch.
//                   last workgroup kbk = n - 1; causal: first = n - 1, G steps, each block n - 1 of the next head.
//                   S = 64         n = 1, first = 0: G steps, block 0 of heads hk * G .. hk * G + G - 1; every
//                                  prefetch is a head switch; G = 1: one step, no prefetch.
//   columns       every staged or loaded row is 128 bf16 (256 bytes): Q, dq at h * 128 < H * 128; K, dk at
//                 (H + hk) * 128 < (H + Hkv) * 128; V, dv at (H + Hkv + hk) * 128 < RS; dO, out at h * 128 of H * 128.
//   dsum          the dQ kernel writes all 64 rows of its block and every (query head, block) has a workgroup: all
//                 [B, H, S] values are written before the dK/dV kernel reads them (stream order).
//
// Rotary position embeddings (template parameter ROPE of the dQ and dK/dV kernels; attention_rope.hip rotates the
// forward's input): qkv holds the rotated Q and K, so the sums above are the gradients of the rotated heads, and
// the epilogue applies the transposed rotation before the store.  A lane's tiles o[c] and o[c + 4] (dk[c], dk[c + 4]),
// c = 0 .. 3, hold columns i = 16 c + 4 lg + r and i + 64 of the same row, a rotary pair of the half-split convention:
//   dx[i] = dx'[i] cos[t][i] + dx'[i + 64] sin[t][i]        dx[i + 64] = dx'[i + 64] cos[t][i] - dx'[i] sin[t][i]
// in f32, no shuffle, no LDS, ahead of * scale and the one rounding to bf16.  t is the lane's query row (dQ) or key row
// (dK): row < S of the f32 [S, 64] tables cos and sin, floats 16 c + 4 lg .. + 3 <= 63 as one 16-byte load each.  dv is
// not touched.  The tables are two kernel arguments of their own (unused, and null, without ROPE); ROPE = false is the
// code it was.
//
// Compiled without packed f32 instructions (KFK_NO_PK_F32), the precaution attention_lengths.hip's header explains.
#include "attention_d128.hpp"

#include <stdexcept>

namespace kfk {

namespace {

// blockIdx.x -> (sequence * H + query head, query block) of the forward and dQ (header: Grid order)
template <bool CAUSAL>
__device__ __forceinline__ void gqa_block_of(int n, int G, int &bh, int &qb) {
    if constexpr (CAUSAL) {
        block_of<true>(n, true, bh, qb);
    } else {
        const int gn = G * n, grp = blockIdx.x / gn, r = blockIdx.x - grp * gn;  // grp = sequence * Hkv + K/V head
        qb = r / G;
        bh = grp * G + (r - qb * G);
    }
}

// (two waves per SIMD, two workgroups per CU, as attn_d128_fwd_kernel)
template <bool CAUSAL>
KFK_NO_PK_F32 __global__ __launch_bounds__(256, 2) void attn_gqa_fwd_kernel(AttnArgs a, int Hkv, int S) {
    extern __shared__ __attribute__((aligned(1024))) uint8_t lds[];
    uint8_t *ring = lds, *Pi = lds + 4 * IMG;  // ring: 2 x (K block, V block)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = S / BK, G = a.H / Hkv;
    int bh, qb;
    gqa_block_of<CAUSAL>(n, G, bh, qb);
    const int b = bh / a.H, h = bh - b * a.H, hk = h / G;
    const int D = a.H * D2, RS = D + 2 * Hkv * D2;  // out / qkv row stride (elements)
    const uint32_t seed = call_seed(a);
    const uint16_t *seq = a.qkv + static_cast<int64_t>(b) * S * RS;
    const uint16_t *kbase = seq + D + hk * D2, *vbase = kbase + Hkv * D2;
    const int strd[2] = {RS, RS};
    {
        const uint16_t *kv[2] = {kbase, vbase};
        stage_rows256<2>(ring, kv, strd, wave, lane);
    }
    const int lg = lane >> 4, lc = lane & 15;
    const int q0 = wave * 16;
    const int row = qb * BK + q0 + lc;  // the query
    bf16x8 qf[KS];
    load_row_frags(seq + static_cast<int64_t>(row) * RS + h * D2, lane, qf);
    float m_run = -INFINITY, l_run = 0.f;
    f32x4 o[TD];  // O^T[d][q]: lane -> d = 16 c + 4 lg + r of query lc
#pragma unroll
    for (int c = 0; c < TD; ++c) o[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int nkb = CAUSAL ? qb + 1 : n;     // streamed key blocks 0 .. nkb - 1
    const int nfull = CAUSAL ? qb : n;       // of which unmasked
    for (int kb = 0; kb < nfull; ++kb) {
        wait_vmcnt<0>();
        __syncthreads();
        const uint8_t *Ki = ring + (kb & 1) * 2 * IMG, *Vi = Ki + IMG;
        if (kb + 1 < nkb) {
            const int64_t r0 = static_cast<int64_t>(kb + 1) * BK * RS;
            const uint16_t *kv[2] = {kbase + r0, vbase + r0};
            stage_rows256<2>(ring + ((kb + 1) & 1) * 2 * IMG, kv, strd, wave, lane);
        }
        fwd_block<false>(a, seed, bh, qf, Ki, Vi, Pi, q0, row, kb * BK, lane, m_run, l_run, o);
    }
    if constexpr (CAUSAL) {  // the diagonal block qb, last: nothing left to prefetch
        wait_vmcnt<0>();
        __syncthreads();
        const uint8_t *Ki = ring + (qb & 1) * 2 * IMG, *Vi = Ki + IMG;
        fwd_block<true>(a, seed, bh, qf, Ki, Vi, Pi, q0, row, qb * BK, lane, m_run, l_run, o);
    }
    const float inv = 1.f / l_run;  // l_run >= 1: the row's maximal key
    if (lg == 0) a.lse[static_cast<int64_t>(bh) * S + row] = m_run + __logf(l_run);
#pragma unroll
    for (int c = 0; c < TD; ++c) {
        uint16_t *dst = a.out + (static_cast<int64_t>(b) * S + row) * D + h * D2 + 16 * c + 4 * lg;
        *reinterpret_cast<uint2 *>(dst) = make_uint2(pack_bf16x2_hw(o[c][0] * inv, o[c][1] * inv),
                                                     pack_bf16x2_hw(o[c][2] * inv, o[c][3] * inv));
    }
}

// The transposed rotation of a rotary pair of gradient tiles, in place (header: Rotary position embeddings): lo holds
// columns 16 c + 4 lg + r, hi the columns 64 on, of table row t.
__device__ __forceinline__ void rope_transposed(const float *cos_t, const float *sin_t, int t, int c, int lg, f32x4 &lo,
                                                f32x4 &hi) {
    const float4 cs = *reinterpret_cast<const float4 *>(cos_t + t * (D2 / 2) + 16 * c + 4 * lg);
    const float4 sn = *reinterpret_cast<const float4 *>(sin_t + t * (D2 / 2) + 16 * c + 4 * lg);
    const float cv[4] = {cs.x, cs.y, cs.z, cs.w}, sv[4] = {sn.x, sn.y, sn.z, sn.w};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float x = lo[r], y = hi[r];
        lo[r] = fmaf(x, cv[r], y * sv[r]);
        hi[r] = fmaf(y, cv[r], -(x * sv[r]));
    }
}

template <bool CAUSAL, bool ROPE>
KFK_NO_PK_F32 __global__ __launch_bounds__(256) void attn_gqa_dq_kernel(AttnArgs a, float *dsum_g, int Hkv, int S,
                                                                        const float *cos_t, const float *sin_t) {
    extern __shared__ __attribute__((aligned(1024))) uint8_t lds[];
    uint8_t *ring = lds, *Si = lds + 4 * IMG;  // ring: 2 x (K, V)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = S / BK, G = a.H / Hkv;
    int bh, qb;
    gqa_block_of<CAUSAL>(n, G, bh, qb);
    const int b = bh / a.H, h = bh - b * a.H, hk = h / G;
    const int D = a.H * D2, RS = D + 2 * Hkv * D2;
    const int nb = CAUSAL ? qb + 1 : n;  // streamed key blocks 0 .. nb - 1
    const uint32_t seed = call_seed(a);
    const uint16_t *seq = a.qkv + static_cast<int64_t>(b) * S * RS;
    const uint16_t *kbase = seq + D + hk * D2, *vbase = kbase + Hkv * D2;
    const uint16_t *dob = a.dout + static_cast<int64_t>(b) * S * D + h * D2;
    const int strd[2] = {RS, RS};
    {
        const uint16_t *kv[2] = {kbase, vbase};
        stage_rows256<2>(ring, kv, strd, wave, lane);
    }
    const int lg = lane >> 4, lc = lane & 15;
    const int qw0 = wave * 16;           // this wave's rows of the block
    const int row = qb * BK + qw0 + lc;  // the query
    bf16x8 qf[KS], gf[KS];
    load_row_frags(seq + static_cast<int64_t>(row) * RS + h * D2, lane, qf);
    load_row_frags(dob + static_cast<int64_t>(row) * D, lane, gf);
    const float l = a.lse[static_cast<int64_t>(bh) * S + row];
    float dd = 0.f;  // D of the query: summed over the first pass, used by the second
    f32x4 o[TD];     // dQ^T[d][q]
#pragma unroll
    for (int c = 0; c < TD; ++c) o[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    // the K / V blocks stream past twice: steps 0 .. nb - 1 sum D, steps nb .. 2 nb - 1 form dS and dQ; causal: the
    // last step of each pass is the diagonal block
    for (int it = 0; it < 2 * nb; ++it) {
        wait_vmcnt<0>();
        __syncthreads();
        const int kb = it < nb ? it : it - nb;
        const bool diag = CAUSAL && kb == qb;
        const uint8_t *Ki = ring + (it & 1) * 2 * IMG, *Vi = Ki + IMG;
        if (it + 1 < 2 * nb) {
            const int nx = it + 1 < nb ? it + 1 : it + 1 - nb;  // <= nb - 1
            const int64_t r0 = static_cast<int64_t>(nx) * BK * RS;
            const uint16_t *kv[2] = {kbase + r0, vbase + r0};
            stage_rows256<2>(ring + ((it + 1) & 1) * 2 * IMG, kv, strd, wave, lane);
        }
        if (it < nb) {
            dd += diag ? bwd_dsum<true>(a, seed, bh, qf, gf, Ki, Vi, row, kb * BK, l, lane)
                       : bwd_dsum<false>(a, seed, bh, qf, gf, Ki, Vi, row, kb * BK, l, lane);
            if (it == nb - 1) {  // the query's four lanes (lg) hold 16 keys of every block each
                dd += __shfl_xor(dd, 16);
                dd += __shfl_xor(dd, 32);
                if (lg == 0) dsum_g[static_cast<int64_t>(bh) * S + row] = dd;
            }
            continue;
        }
        if (diag) bwd_scores<true>(a, seed, bh, qf, gf, Ki, Vi, nullptr, Si, qw0 + lc, row, kb * BK, l, dd, lane);
        else bwd_scores<false>(a, seed, bh, qf, gf, Ki, Vi, nullptr, Si, qw0 + lc, row, kb * BK, l, dd, lane);
        lds_wave_sync();
        // dQ^T[d][q] += sum_key K[key][d] dS[q][key]
#pragma unroll
        for (int s = 0; s < BK / 32; ++s) {
            bf16x8 ka[TD];
#pragma unroll
            for (int c = 0; c < TD; ++c) ka[c] = tr_frag<256>(Ki, 32 * s, 16 * c, lane);
            const bf16x8 sb = row_frag<128>(Si, qw0, 32 * s, lane);
#pragma unroll
            for (int c = 0; c < TD; ++c) o[c] = mfma(ka[c], sb, o[c]);
        }
    }
    if constexpr (ROPE) {  // the position is the query row
#pragma unroll
        for (int c = 0; c < TD / 2; ++c) rope_transposed(cos_t, sin_t, row, c, lg, o[c], o[c + TD / 2]);
    }
#pragma unroll
    for (int c = 0; c < TD; ++c) {
        uint16_t *dst = a.dqkv + (static_cast<int64_t>(b) * S + row) * RS + h * D2 + 16 * c + 4 * lg;
        *reinterpret_cast<uint2 *>(dst) = make_uint2(pack_bf16x2_hw(o[c][0] * a.scale, o[c][1] * a.scale),
                                                     pack_bf16x2_hw(o[c][2] * a.scale, o[c][3] * a.scale));
    }
}

// What a dK/dV workgroup streams: the sequence's qkv and dO rows (column 0) and their strides, the blocks per head
struct GroupStream {
    const uint16_t *seq, *dseq;  // qkv [S, RS], dout [S, D] of the sequence
    int RS, D, S, n, first;      // a head's sub-stream is blocks first .. n - 1
    int hlast;                   // the group's last query head
};

// One dK/dV step on the staged block qb of query head h (ring slot `slot`), after starting the DMA of the stream's next
// step into the other slot: block qb + 1 of h, or block `first` of head h + 1 behind h's last block; nothing behind
// the last head's last block.  MASK: the diagonal block (keys beyond a query give P = dS = 0), chosen outside.
template <bool MASK>
__device__ __forceinline__ void dkv_step(const AttnArgs &a, const float *dsum_g, uint32_t seed, const GroupStream &g,
                                         int b, int h, int qb, int kbk, int slot, uint8_t *lds, int wave, int lane,
                                         f32x4 (&dv)[TD], f32x4 (&dk)[TD]) {
    uint8_t *Ki = lds, *Vi = lds + IMG, *ring = lds + 2 * IMG, *Pi = lds + 6 * IMG, *Si = Pi + BLK;
    const int lc = lane & 15, w0 = wave * 16;
    const int bh = b * a.H + h;
    const int row = qb * BK + w0 + lc;  // the query, < S
    const float l = a.lse[static_cast<int64_t>(bh) * g.S + row];
    const float dd = dsum_g[static_cast<int64_t>(bh) * g.S + row];
    wait_vmcnt<0>();
    __syncthreads();
    const uint8_t *Qi = ring + slot * 2 * IMG, *Oi = Qi + IMG;
    const bool inside = qb + 1 < g.n;
    if (inside || h < g.hlast) {
        const int nh = inside ? h : h + 1, nqb = inside ? qb + 1 : g.first;  // nh <= hlast, first <= nqb <= n - 1
        const uint16_t *qo[2] = {g.seq + static_cast<int64_t>(nqb) * BK * g.RS + nh * D2,
                                 g.dseq + static_cast<int64_t>(nqb) * BK * g.D + nh * D2};
        const int strd_qo[2] = {g.RS, g.D};
        stage_rows256<2>(ring + (slot ^ 1) * 2 * IMG, qo, strd_qo, wave, lane);
    }
    {
        bf16x8 qf[KS], gf[KS];  // this wave's 16 queries of the streamed block
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            qf[s] = row_frag<256>(Qi, w0, 32 * s, lane);
            gf[s] = row_frag<256>(Oi, w0, 32 * s, lane);
        }
        bwd_scores<MASK>(a, seed, bh, qf, gf, Ki, Vi, Pi, Si, w0 + lc, row, kbk * BK, l, dd, lane);
    }
    lds_barrier();
    // dV^T[d][key] += sum_q dO[q][d] P_drop[q][key]; dK^T[d][key] += sum_q Q[q][d] dS[q][key]
#pragma unroll
    for (int s = 0; s < BK / 32; ++s) {
        const bf16x8 pb = tr_frag<128>(Pi, 32 * s, w0, lane);
        const bf16x8 sb = tr_frag<128>(Si, 32 * s, w0, lane);
#pragma unroll
        for (int c = 0; c < TD; ++c) {
            dv[c] = mfma(tr_frag<256>(Oi, 32 * s, 16 * c, lane), pb, dv[c]);
            dk[c] = mfma(tr_frag<256>(Qi, 32 * s, 16 * c, lane), sb, dk[c]);
        }
    }
}

template <bool CAUSAL, bool ROPE>
KFK_NO_PK_F32 __global__ __launch_bounds__(256) void attn_gqa_dkv_kernel(AttnArgs a, const float *dsum_g, int Hkv,
                                                                         int S, const float *cos_t,
                                                                         const float *sin_t) {
    extern __shared__ __attribute__((aligned(1024))) uint8_t lds[];  // K, V resident; ring 2 x (Q, dO); P_drop; dS
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nbs = S / BK, G = a.H / Hkv;
    int bhk, kbk;  // sequence * Hkv + K/V head, key block
    block_of<CAUSAL>(nbs, false, bhk, kbk);
    const int b = bhk / Hkv, hk = bhk - b * Hkv, h0 = hk * G;
    const int D = a.H * D2, RS = D + 2 * Hkv * D2;
    const uint32_t seed = call_seed(a);
    GroupStream g;
    g.seq = a.qkv + static_cast<int64_t>(b) * S * RS, g.dseq = a.dout + static_cast<int64_t>(b) * S * D;
    g.RS = RS, g.D = D, g.S = S, g.n = nbs, g.first = CAUSAL ? kbk : 0, g.hlast = h0 + G - 1;
    const int kcol = D + hk * D2, vcol = kcol + Hkv * D2;  // the K/V head's columns of a qkv (and dqkv) row
    {
        const uint16_t *krow = g.seq + static_cast<int64_t>(kbk) * BK * RS;
        const uint16_t *kv[2] = {krow + kcol, krow + vcol};
        const int strd[2] = {RS, RS};
        stage_rows256<2>(lds, kv, strd, wave, lane);
        const uint16_t *qo[2] = {g.seq + static_cast<int64_t>(g.first) * BK * RS + h0 * D2,
                                 g.dseq + static_cast<int64_t>(g.first) * BK * D + h0 * D2};
        const int strd_qo[2] = {RS, D};
        stage_rows256<2>(lds + 2 * IMG, qo, strd_qo, wave, lane);
    }
    const int lg = lane >> 4, lc = lane & 15;
    const int w0 = wave * 16;  // this wave's queries of the streamed block (scores) and keys of the resident one (sums)
    f32x4 dv[TD], dk[TD];      // dV^T[d][key], dK^T[d][key]: the sums over the whole group
#pragma unroll
    for (int c = 0; c < TD; ++c) dv[c] = dk[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    int slot = 0;  // step t of the stream sits in ring slot t & 1
    for (int h = h0; h <= g.hlast; ++h) {
        int qb = g.first;
        if constexpr (CAUSAL) {  // the diagonal block opens every head's sub-stream
            dkv_step<true>(a, dsum_g, seed, g, b, h, qb, kbk, slot, lds, wave, lane, dv, dk);
            ++qb, slot ^= 1;
        }
        for (; qb < nbs; ++qb, slot ^= 1)
            dkv_step<false>(a, dsum_g, seed, g, b, h, qb, kbk, slot, lds, wave, lane, dv, dk);
    }
    if constexpr (ROPE) {  // the position is the key row
#pragma unroll
        for (int c = 0; c < TD / 2; ++c)
            rope_transposed(cos_t, sin_t, kbk * BK + w0 + lc, c, lg, dk[c], dk[c + TD / 2]);
    }
    uint16_t *dkv0 = a.dqkv + (static_cast<int64_t>(b) * S + kbk * BK) * RS;
#pragma unroll
    for (int c = 0; c < TD; ++c) {
        uint16_t *rowp = dkv0 + static_cast<int64_t>(w0 + lc) * RS + 16 * c + 4 * lg;
        *reinterpret_cast<uint2 *>(rowp + kcol) = make_uint2(pack_bf16x2_hw(dk[c][0] * a.scale, dk[c][1] * a.scale),
                                                             pack_bf16x2_hw(dk[c][2] * a.scale, dk[c][3] * a.scale));
        *reinterpret_cast<uint2 *>(rowp + vcol) = make_uint2(pack_bf16x2_hw(dv[c][0], dv[c][1]),
                                                             pack_bf16x2_hw(dv[c][2], dv[c][3]));
    }
}

void check(int S, int H, int Hkv) {
    if (!attention_gqa_supported(S, H, Hkv))
        throw std::invalid_argument("attention: grouped-query heads need S % 64 == 0, 64 <= S <= 1024, "
                                    "1 <= kv_heads <= heads and heads % kv_heads == 0");
}

template <bool CAUSAL>
void forward(const AttnArgs &a, int Hkv, int grid, int S, hipStream_t s) {
    static const bool attr = (raise_lds(attn_gqa_fwd_kernel<CAUSAL>, FWD_LDS), true);
    (void)attr;
    attn_gqa_fwd_kernel<CAUSAL><<<grid, 256, FWD_LDS, s>>>(a, Hkv, S);
}

template <bool CAUSAL, bool ROPE>
void backward(const AttnArgs &a, float *dsum, int Hkv, int B, int S, const float *cos, const float *sin,
              hipStream_t s) {
    static const bool attr = (raise_lds(attn_gqa_dq_kernel<CAUSAL, ROPE>, DQ_LDS),
                              raise_lds(attn_gqa_dkv_kernel<CAUSAL, ROPE>, DKV_LDS), true);
    (void)attr;
    const int n = S / BK;
    // the dQ kernel fills all [B, H, S] of dsum, the dK/dV kernel reads them (stream order)
    attn_gqa_dq_kernel<CAUSAL, ROPE><<<B * a.H * n, 256, DQ_LDS, s>>>(a, dsum, Hkv, S, cos, sin);
    attn_gqa_dkv_kernel<CAUSAL, ROPE><<<B * Hkv * n, 256, DKV_LDS, s>>>(a, dsum, Hkv, S, cos, sin);
}

}  // namespace

bool attention_gqa_supported(int S, int heads, int kv_heads) {
    return attention_d128_supported(S) && kv_heads >= 1 && heads >= kv_heads && heads % kv_heads == 0;
}

void launch_attention_gqa_forward(const uint16_t *qkv, uint16_t *out, float *lse, int B, int S, int H, int Hkv,
                                  float scale, uint32_t seed, float p_drop, bool causal, hipStream_t s) {
    check(S, H, Hkv);
    const AttnArgs a = make_args(qkv, out, lse, nullptr, nullptr, H, scale, seed, p_drop);
    const int grid = B * H * (S / BK);
    if (causal) forward<true>(a, Hkv, grid, S, s);
    else forward<false>(a, Hkv, grid, S, s);
}

void launch_attention_gqa_backward(const uint16_t *qkv, const uint16_t *out, const float *lse, const uint16_t *dout,
                                   uint16_t *dqkv, float *dsum, int B, int S, int H, int Hkv, float scale,
                                   uint32_t seed, float p_drop, bool causal, hipStream_t s, const float *cos,
                                   const float *sin) {
    check(S, H, Hkv);
    if (!cos != !sin) throw std::invalid_argument("attention: the rotary tables cos and sin come together");
    if (!dsum) throw std::invalid_argument("attention: the grouped-query backward needs the [B, H, S] f32 dsum buffer");
    const AttnArgs a = make_args(qkv, const_cast<uint16_t *>(out), const_cast<float *>(lse), dout, dqkv, H, scale, seed,
                                 p_drop);
    if (cos) {
        if (causal) backward<true, true>(a, dsum, Hkv, B, S, cos, sin, s);
        else backward<false, true>(a, dsum, Hkv, B, S, cos, sin, s);
    } else {
        if (causal) backward<true, false>(a, dsum, Hkv, B, S, nullptr, nullptr, s);
        else backward<false, false>(a, dsum, Hkv, B, S, nullptr, nullptr, s);
    }
}

}  // namespace kfk
