// Fused multi-head self-attention at head dim 128 (GPT-3 6.7 B and up, the LLaMA family): streaming kernels of
// their own, bidirectional or causal (template parameter CAUSAL), S = 64 .. 1024 in steps of 64, bf16, dropout.
//
// Interface as the 64-wide family: qkv [B, S, 3, H, 128] -> out [B, S, H, 128], lse and dsum [B, H, S] f32, the
// keep_elem hash on the global (query, key) index recomputed in the backward (q << 16 | k: S <= 1024 leaves room).
// No atomics, no zeroed scratch, no workgroup waits on another: bitwise reproducible.  No per-sequence lengths.
// Nothing of the 64-wide kernels is called or changed; what is shared is attention_common.hpp's addressing
// (off / row_frag / tr_frag at ROW = 256), the hash and the argument block, and attention_stream.hpp's two
// LDS-only synchronisations.
//
// Work split   One workgroup (4 waves) per (sequence, head, 64-row block), BQ = BK = 64, wave w owns rows
//              16 w .. 16 w + 15 of the block.  Forward and dQ: the block is a query block and K / V blocks stream
//              past; dK/dV: the block is a key block and Q / dO blocks stream past.
// Registers    The wave's own Q rows (and the dQ kernel's dO rows) never enter LDS: each lane loads its four
//              16-byte MFMA B-operand pieces (row 16 w + (lane & 15), columns 32 s + 8 (lane >> 4) .., s = 0 .. 3)
//              straight from global memory once, 16 VGPRs per operand, and keeps them for the whole stream.
// LDS          K, V, and the dK/dV kernel's Q and dO, are 64 x 128 bf16 images of 256-byte rows (16 KB), swizzled
//              by hswz<256>, staged by stage_rows256: one global_load_lds moves 1 KB = 4 rows, a lane 16 bytes, the
//              swizzle applied to the source column.  P (and dS) are 64 x 64 bf16 images of 128-byte rows (8 KB).
//                forward, dQ   ring 2 x (K, V) 64 KB + P or dS 8 KB                     = 72 KB: two workgroups fit
//                              a CU's 160 KB (with Q, and dO, as LDS images it is 88 / 104 KB: one workgroup).  The
//                              forward's registers allow it too; the dQ kernel's do not (more than 256 VGPRs + AGPRs:
//                              one wave per SIMD, profiles/attention_d128.md)
//                dK/dV         K, V resident 32 KB + ring 2 x (Q, dO) 64 KB + P, dS 16 KB = 112 KB: one workgroup
//              All three exceed the 64 KB static limit: dynamic LDS, the function attribute raised at first launch.
// MFMA         v_mfma_f32_16x16x32_bf16.  S^T = K Q^T: four K-steps per 16 x 16 tile, 4 tiles (64 keys) per wave.
//              O^T += V^T P^T and dQ^T += K^T dS^T: 8 accumulator tiles (128 d x 16 queries) per wave, two K-steps
//              per block.  dK/dV: 16 tiles (dV^T and dK^T, 128 d x 16 keys each).
// Step         wait for the DMA of this step's block (counted), workgroup barrier, start the DMA of the next block
//              into the other ring slot, compute.  P / dS rows of the forward and the dQ kernel stay inside their
//              wave (lds_wave_sync); the dK/dV kernel's cross the waves (lds_barrier, DMA left in flight).
// Backward     As the family: the dQ kernel streams K / V twice, first summing D = rowsum(P_drop o dP) in f32 (not
//              from the rounded bf16 O), then forming dS and dQ; it writes D to dsum for the dK/dV kernel, which
//              follows it in stream order.
// Causal       Query block i needs key blocks 0 .. i; key block j is needed by query blocks j .. n - 1 (n = S / 64).
//              Only the diagonal block is masked: the last step of the forward's and dQ's stream, the first of the
//              dK/dV kernel's, peeled out of the loops.  blockIdx.x is block-major, heaviest block first.  The
//              forward's diagonal P V keeps each wave's 16 x 16 triangle out of the MFMA (pv_diagonal): a V row of a
//              masked key never meets an earlier query in a product, so NaN or inf in future rows of V cannot reach
//              earlier output rows.  (The backward has no such guard, as at head dim 64.)
// Bidirectional  Every block, nothing masked, workgroups (sequence, head)-major.
//
// Rows read or staged, by hand (n = S / 64; block b is rows 64 b .. 64 b + 63, inside [0, S) iff 0 <= b < n;
// `last` = qb when causal, n - 1 when not; `first` = kbk when causal, 0 when not):
//   forward, dQ   registers: Q (and dO), lse rows 64 qb + 16 w + 0 .. 15, qb = 0 .. n - 1.  Streamed K / V: first
//                 block 0, last block `last` (the prefetch of step kb stages kb + 1 only if kb + 1 <= last; the dQ
//                 kernel's second pass starts over at block 0 and ends at `last` again).
//                   first workgroup  causal: qb = n - 1, blocks 0 .. n - 1.  bidirectional: qb = 0, blocks 0 .. n - 1.
//                   last workgroup   causal: qb = 0, block 0 only, no prefetch (dQ: block 0 twice).
//                                    bidirectional: qb = n - 1, blocks 0 .. n - 1.
//                   S = 64           n = 1, qb = 0, block 0 only (dQ: twice), no other row touched.
//   dK/dV         resident: K, V block kbk = 0 .. n - 1.  Streamed Q / dO, lse and dsum rows: first block `first`,
//                 last block n - 1 (the prefetch of step qb stages qb + 1 only if qb + 1 <= n - 1).
//                   first workgroup  kbk = 0, blocks 0 .. n - 1 (either mask).
//                   last workgroup   kbk = n - 1; causal: block n - 1 only, no prefetch; bidirectional: 0 .. n - 1.
//                   S = 64           block 0 only.
//   columns       every staged or loaded row is the head's 128 bf16 (256 bytes) at h * 128 of its q, k, v or dO part.
//   dsum          the dQ kernel writes all 64 rows of its block and every block has a workgroup: all S rows are
//                 written before the dK/dV kernel reads them.
//   pv_diagonal   LDS rows of V: keys < q0 by MFMA (32-key steps below q0 + 16, the upper half zeroed in registers
//                 where it is the triangle's), keys q0 .. q0 + 15 on the VALU, none beyond (q0 = 16 w).
//
// Compiled without packed f32 instructions (KFK_NO_PK_F32), the precaution attention_lengths.hip's header explains.
// The device helpers (stage_rows256, the block steps) are attention_d128.hpp's, shared with attention_gqa.hip.
#include "attention_d128.hpp"

#include <stdexcept>

namespace kfk {

namespace {

// (two waves per SIMD: the register budget that lets two workgroups share a CU, as their 72 KB of LDS do)
template <bool CAUSAL>
KFK_NO_PK_F32 __global__ __launch_bounds__(256, 2) void attn_d128_fwd_kernel(AttnArgs a, int S) {
    extern __shared__ __attribute__((aligned(1024))) uint8_t lds[];
    uint8_t *ring = lds, *Pi = lds + 4 * IMG;  // ring: 2 x (K block, V block)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = S / BK;
    int bh, qb;
    block_of<CAUSAL>(n, true, bh, qb);
    const int b = bh / a.H, h = bh - b * a.H;
    const int D = a.H * D2, RS = 3 * D;  // qkv row stride (elements)
    const uint32_t seed = call_seed(a);
    const uint16_t *base = a.qkv + static_cast<int64_t>(b) * S * RS + h * D2;
    const int strd[2] = {RS, RS};
    {
        const uint16_t *kv[2] = {base + D, base + 2 * D};
        stage_rows256<2>(ring, kv, strd, wave, lane);
    }
    const int lg = lane >> 4, lc = lane & 15;
    const int q0 = wave * 16;
    const int row = qb * BK + q0 + lc;  // the query
    bf16x8 qf[KS];
    load_row_frags(base + static_cast<int64_t>(row) * RS, lane, qf);
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
            const uint16_t *kv[2] = {base + D + r0, base + 2 * D + r0};
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

template <bool CAUSAL>
KFK_NO_PK_F32 __global__ __launch_bounds__(256) void attn_d128_dq_kernel(AttnArgs a, float *dsum_g, int S) {
    extern __shared__ __attribute__((aligned(1024))) uint8_t lds[];
    uint8_t *ring = lds, *Si = lds + 4 * IMG;  // ring: 2 x (K, V)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = S / BK;
    int bh, qb;
    block_of<CAUSAL>(n, true, bh, qb);
    const int b = bh / a.H, h = bh - b * a.H;
    const int D = a.H * D2, RS = 3 * D;
    const int nb = CAUSAL ? qb + 1 : n;  // streamed key blocks 0 .. nb - 1
    const uint32_t seed = call_seed(a);
    const uint16_t *base = a.qkv + static_cast<int64_t>(b) * S * RS + h * D2;
    const uint16_t *dob = a.dout + static_cast<int64_t>(b) * S * D + h * D2;
    const int strd[2] = {RS, RS};
    {
        const uint16_t *kv[2] = {base + D, base + 2 * D};
        stage_rows256<2>(ring, kv, strd, wave, lane);
    }
    const int lg = lane >> 4, lc = lane & 15;
    const int qw0 = wave * 16;           // this wave's rows of the block
    const int row = qb * BK + qw0 + lc;  // the query
    bf16x8 qf[KS], gf[KS];
    load_row_frags(base + static_cast<int64_t>(row) * RS, lane, qf);
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
            const uint16_t *kv[2] = {base + D + r0, base + 2 * D + r0};
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
#pragma unroll
    for (int c = 0; c < TD; ++c) {
        uint16_t *dst = a.dqkv + (static_cast<int64_t>(b) * S + row) * RS + h * D2 + 16 * c + 4 * lg;
        *reinterpret_cast<uint2 *>(dst) = make_uint2(pack_bf16x2_hw(o[c][0] * a.scale, o[c][1] * a.scale),
                                                     pack_bf16x2_hw(o[c][2] * a.scale, o[c][3] * a.scale));
    }
}

// The dK/dV steps on the streamed query blocks qb0 .. qb1 - 1; the ring slot of block qb is (qb - first) & 1.
// MASK: the diagonal block (keys beyond a query give P = dS = 0), chosen outside.
template <bool MASK>
__device__ __forceinline__ void dkv_loop(const AttnArgs &a, const float *dsum_g, uint32_t seed, int bh, int S, int qb0,
                                         int qb1, int first, int kbk, const uint16_t *base, const uint16_t *dob,
                                         uint8_t *lds, int wave, int lane, f32x4 (&dv)[TD], f32x4 (&dk)[TD]) {
    uint8_t *Ki = lds, *Vi = lds + IMG, *ring = lds + 2 * IMG, *Pi = lds + 6 * IMG, *Si = Pi + BLK;
    const int D = a.H * D2, RS = 3 * D, nbs = S / BK;
    const int strd_qo[2] = {RS, D};
    const int lc = lane & 15, w0 = wave * 16;
    for (int qb = qb0; qb < qb1; ++qb) {
        const int row = qb * BK + w0 + lc;  // the query, < S
        const float l = a.lse[static_cast<int64_t>(bh) * S + row];
        const float dd = dsum_g[static_cast<int64_t>(bh) * S + row];
        wait_vmcnt<0>();
        __syncthreads();
        const uint8_t *Qi = ring + ((qb - first) & 1) * 2 * IMG, *Oi = Qi + IMG;
        if (qb + 1 < nbs) {
            const uint16_t *qo[2] = {base + static_cast<int64_t>(qb + 1) * BK * RS,
                                     dob + static_cast<int64_t>(qb + 1) * BK * D};
            stage_rows256<2>(ring + ((qb + 1 - first) & 1) * 2 * IMG, qo, strd_qo, wave, lane);
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
}

template <bool CAUSAL>
KFK_NO_PK_F32 __global__ __launch_bounds__(256) void attn_d128_dkv_kernel(AttnArgs a, const float *dsum_g, int S) {
    extern __shared__ __attribute__((aligned(1024))) uint8_t lds[];  // K, V resident; ring 2 x (Q, dO); P_drop; dS
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nbs = S / BK;
    int bh, kbk;
    block_of<CAUSAL>(nbs, false, bh, kbk);
    const int b = bh / a.H, h = bh - b * a.H;
    const int D = a.H * D2, RS = 3 * D;
    const int first = CAUSAL ? kbk : 0;  // the first streamed query block
    const uint32_t seed = call_seed(a);
    const uint16_t *base = a.qkv + static_cast<int64_t>(b) * S * RS + h * D2;
    const uint16_t *dob = a.dout + static_cast<int64_t>(b) * S * D + h * D2;
    {
        const int64_t r0 = static_cast<int64_t>(kbk) * BK * RS;
        const uint16_t *kv[2] = {base + D + r0, base + 2 * D + r0};
        const int strd[2] = {RS, RS};
        stage_rows256<2>(lds, kv, strd, wave, lane);
        const uint16_t *qo[2] = {base + static_cast<int64_t>(first) * BK * RS,
                                 dob + static_cast<int64_t>(first) * BK * D};
        const int strd_qo[2] = {RS, D};
        stage_rows256<2>(lds + 2 * IMG, qo, strd_qo, wave, lane);
    }
    const int lg = lane >> 4, lc = lane & 15;
    const int w0 = wave * 16;  // this wave's queries of the streamed block (scores) and keys of the resident one (sums)
    f32x4 dv[TD], dk[TD];      // dV^T[d][key], dK^T[d][key]
#pragma unroll
    for (int c = 0; c < TD; ++c) dv[c] = dk[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    if constexpr (CAUSAL) {
        dkv_loop<true>(a, dsum_g, seed, bh, S, kbk, kbk + 1, first, kbk, base, dob, lds, wave, lane, dv, dk);
        dkv_loop<false>(a, dsum_g, seed, bh, S, kbk + 1, nbs, first, kbk, base, dob, lds, wave, lane, dv, dk);
    } else {
        dkv_loop<false>(a, dsum_g, seed, bh, S, 0, nbs, first, kbk, base, dob, lds, wave, lane, dv, dk);
    }
    uint16_t *dkv0 = a.dqkv + (static_cast<int64_t>(b) * S + kbk * BK) * RS + h * D2;
#pragma unroll
    for (int c = 0; c < TD; ++c) {
        uint16_t *rowp = dkv0 + static_cast<int64_t>(w0 + lc) * RS + 16 * c + 4 * lg;
        *reinterpret_cast<uint2 *>(rowp + D) = make_uint2(pack_bf16x2_hw(dk[c][0] * a.scale, dk[c][1] * a.scale),
                                                          pack_bf16x2_hw(dk[c][2] * a.scale, dk[c][3] * a.scale));
        *reinterpret_cast<uint2 *>(rowp + 2 * D) = make_uint2(pack_bf16x2_hw(dv[c][0], dv[c][1]),
                                                              pack_bf16x2_hw(dv[c][2], dv[c][3]));
    }
}

void check(int S) {
    if (!attention_d128_supported(S))
        throw std::invalid_argument("attention: head dim 128 needs S % 64 == 0, 64 <= S <= 1024");
}

template <bool CAUSAL>
void forward(const AttnArgs &a, int grid, int S, hipStream_t s) {
    static const bool attr = (raise_lds(attn_d128_fwd_kernel<CAUSAL>, FWD_LDS), true);
    (void)attr;
    attn_d128_fwd_kernel<CAUSAL><<<grid, 256, FWD_LDS, s>>>(a, S);
}

template <bool CAUSAL>
void backward(const AttnArgs &a, float *dsum, int grid, int S, hipStream_t s) {
    static const bool attr = (raise_lds(attn_d128_dq_kernel<CAUSAL>, DQ_LDS),
                              raise_lds(attn_d128_dkv_kernel<CAUSAL>, DKV_LDS), true);
    (void)attr;
    attn_d128_dq_kernel<CAUSAL><<<grid, 256, DQ_LDS, s>>>(a, dsum, S);    // fills all S rows of dsum
    attn_d128_dkv_kernel<CAUSAL><<<grid, 256, DKV_LDS, s>>>(a, dsum, S);  // reads them (stream order)
}

}  // namespace

bool attention_d128_supported(int S) { return S >= 64 && S <= 1024 && S % 64 == 0; }

void launch_attention_d128_forward(const uint16_t *qkv, uint16_t *out, float *lse, int B, int S, int H, float scale,
                                   uint32_t seed, float p_drop, bool causal, hipStream_t s) {
    check(S);
    const AttnArgs a = make_args(qkv, out, lse, nullptr, nullptr, H, scale, seed, p_drop);
    const int grid = B * H * (S / BK);
    if (causal) forward<true>(a, grid, S, s);
    else forward<false>(a, grid, S, s);
}

void launch_attention_d128_backward(const uint16_t *qkv, const uint16_t *out, const float *lse, const uint16_t *dout,
                                    uint16_t *dqkv, float *dsum, int B, int S, int H, float scale, uint32_t seed,
                                    float p_drop, bool causal, hipStream_t s) {
    check(S);
    if (!dsum) throw std::invalid_argument("attention: the head dim 128 backward needs the [B, H, S] f32 dsum buffer");
    const AttnArgs a = make_args(qkv, const_cast<uint16_t *>(out), const_cast<float *>(lse), dout, dqkv, H, scale, seed,
                                 p_drop);
    const int grid = B * H * (S / BK);
    if (causal) backward<true>(a, dsum, grid, S, s);
    else backward<false>(a, dsum, grid, S, s);
}

}  // namespace kfk
