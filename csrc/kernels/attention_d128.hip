// Fused self-attention at head dim 128 (GPT-3 6.7 B and up, the LLaMA family, Mistral): one family of streaming
// kernels, bidirectional or causal (template parameter CAUSAL), S = 64 .. 1024 in steps of 64, bf16, dropout.  H query
// heads share Hkv = H / G key/value heads, query head h reads K/V head h / G.  G is a run-time value: multi-head
// attention (Hkv = H, G = 1), grouped-query attention and multi-query attention (Hkv = 1) are the same three kernels.
// Causal with a sliding window (template parameter BAND; "Band" below): S = 64 .. 8192.
//
// Interface    qkv [B, S, (H + 2 Hkv) * 128], the output of one Linear(d, (H + 2 Hkv) * 128): a row holds the H query
//              heads, then the Hkv key heads, then the Hkv value heads, 128 bf16 each.  Q of head h is at column
//              h * 128, K at (H + h / G) * 128, V at (H + Hkv + h / G) * 128; row stride RS = (H + 2 Hkv) * 128.  At
//              Hkv = H that is [B, S, 3, H, 128], what the attention_d128_* bindings pass.
//              out [B, S, H, 128]; lse and dsum [B, H, S] f32 per query head; dqkv in qkv's layout, every element
//              written once.  The keep_elem hash is on the global (query, key) index (q << 16 | k: S <= 8192 leaves
//              room), recomputed in the backward, and keyed on the query head: (seed, b * H + h, query, key).  No
//              atomics, no zeroed scratch, no workgroup waits on another: bitwise reproducible.  No per-sequence
//              lengths.  The argument block is attention_common.hpp's with H the query heads; Hkv is a kernel argument
//              of its own.  Nothing of the 64-wide kernels is called; shared are attention_common.hpp's addressing
//              (off / row_frag / tr_frag at ROW = 256), the hash and the argument block, and attention_stream.hpp's
//              two LDS-only synchronisations.
// Work split   One workgroup is 4 waves, BQ = BK = 64, wave w owns rows 16 w .. 16 w + 15 of its block.
//              Forward and dQ: one workgroup per (sequence, query head, 64-row query block); the K / V blocks of head
//              h / G stream past through a 2-slot ring.
//              dK/dV: one workgroup per (sequence, K/V head, 64-row key block): B * Hkv * n workgroups, not B * H * n.
//              K and V of the block stay resident in LDS, and the 16 accumulator tiles (dV^T and dK^T, 128 d x 16 keys
//              per wave) stay in registers while the (Q, dO) blocks of the whole group stream past: the G query heads
//              are summed in f32 in those registers and rounded to bf16 once, at the single store.  No partial
//              buffers, no second pass, no atomics.
// Registers    The wave's own Q rows (and the dQ kernel's dO rows) never enter LDS: each lane loads its four
//              16-byte MFMA B-operand pieces (row 16 w + (lane & 15), columns 32 s + 8 (lane >> 4) .., s = 0 .. 3)
//              straight from global memory once, 16 VGPRs per operand, and keeps them for the whole stream.
// Grid order   The G workgroups of the forward and of dQ that stream the same K/V head are neighbours in dispatch:
//              within a block rank the heads run in ascending order, so a group's G heads are adjacent.  They walk the
//              same K/V blocks at the same pace: a block comes from HBM once per group and the other G - 1 workgroups
//              find it in L2.
//                causal         block-major, heaviest query block (n - 1) first; inside a rank b * H + h ascending
//                bidirectional  (sequence, K/V head)-major; inside a group block-major, the G heads of a block adjacent
//              dK/dV: causal block-major, heaviest key block (0) first; bidirectional (sequence, K/V head)-major.
// LDS          K, V, and the dK/dV kernel's Q and dO, are 64 x 128 bf16 images of 256-byte rows (16 KB), swizzled
//              by hswz<256>, staged by stage_rows256: one global_load_lds moves 1 KB = 4 rows, a lane 16 bytes, the
//              swizzle applied to the source column.  P (and dS) are 64 x 64 bf16 images of 128-byte rows (8 KB).
//                forward, dQ   ring 2 x (K, V) 64 KB + P or dS 8 KB                     = 72 KB: two workgroups fit
//                              a CU's 160 KB (with Q, and dO, as LDS images it is 88 / 104 KB: one workgroup).  The
//                              forward's registers allow it too; the dQ kernel's do not (more than 256 VGPRs + AGPRs:
//                              one wave per SIMD, profiles/attention_gqa.md)
//                dK/dV         K, V resident 32 KB + ring 2 x (Q, dO) 64 KB + P, dS 16 KB = 112 KB: one workgroup
//              All three exceed the 64 KB static limit: dynamic LDS, the function attribute raised at first launch.
//              The group adds no byte, its heads reuse the ring.
// MFMA         v_mfma_f32_16x16x32_bf16.  S^T = K Q^T: four K-steps per 16 x 16 tile, 4 tiles (64 keys) per wave.
//              O^T += V^T P^T and dQ^T += K^T dS^T: 8 accumulator tiles (128 d x 16 queries) per wave, two K-steps
//              per block.  dK/dV: 16 tiles (dV^T and dK^T, 128 d x 16 keys each).
// Step         wait for the DMA of this step's block (counted), workgroup barrier, start the DMA of the next block
//              into the other ring slot, compute.  P / dS rows of the forward and the dQ kernel stay inside their
//              wave (lds_wave_sync); the dK/dV kernel's cross the waves (lds_barrier, DMA left in flight).
// Backward     As the 64-wide family: the dQ kernel streams K / V twice, first summing D = rowsum(P_drop o dP) in f32
//              (not from the rounded bf16 O), then forming dS and dQ; it writes D to dsum for the dK/dV kernel, which
//              follows it in stream order.
// dK/dV stream One stream of G * (n - first) steps through the 2-slot ring (first = kbk when causal, 0 otherwise):
//              step t is query head hk * G + t / (n - first), query block first + t % (n - first); heads ascending,
//              blocks ascending inside a head; ring slot t & 1.  The prefetch of a head's last block stages the
//              next head's block `first`, so the ring never drains at a head boundary.  lse and dsum rows and the
//              hash's b * H + h follow the streamed head.
// Causal       Query block i needs key blocks 0 .. i; key block j is needed by query blocks j .. n - 1 (n = S / 64).
//              Forward and dQ: only the diagonal block (the last step) is masked.  The forward's diagonal P V keeps
//              each wave's 16 x 16 triangle out of the MFMA (pv_diagonal): a V row of a masked key never meets an
//              earlier query in a product, so NaN or inf in future rows of V cannot reach earlier output rows.  (The
//              backward has no such guard, as at head dim 64.)
//              dK/dV: the diagonal block is the first step of every head's sub-stream, G times per workgroup: each
//              head runs one masked step (dkv_step<true>) and then its loop of unmasked ones (dkv_step<false>), so the
//              unmasked steps carry no mask code.
// Band         BAND (causal only; w = window / 64 >= 1, a kernel argument of its own): query q sees keys q - 64 w < k <= q.
//              Query block i needs key blocks max(0, i - w) .. i; key block j is needed by query blocks j ..
//              min(n - 1, j + w).  Two blocks are masked, complementary triangles: the diagonal block (kk <= qq) and,
//              for i >= w, the edge block i - w (kk > qq, MASK = EDGE); the blocks between carry no mask code.
//              Forward and dQ stream in ascending order, the edge block first, the diagonal last: with w >= n there
//              is no edge block and the steps, their order and their ring slots are the causal kernel's, so the
//              results are its results bit for bit.  (The diagonal first and the edge last would never meet an empty
//              row but would reorder those sums.)  The price is that the first step may see an empty row: qq = 63 has no
//              key in its edge block and m_run is still -inf.  fwd_block<EDGE> takes that step's exponentials against 0
//              where the maximum is -inf: alpha = e = 0, l_run and o stay 0 and m_run -inf, and the next step rescales
//              by exp(-inf - m) = 0 as a first step does.  The diagonal block ends every stream and holds the row's
//              own key, so l_run >= 1 at the division.  The ring slot follows the step, (kb - first) & 1, not the
//              block.  The edge block has no pv_diagonal-style guard: its masked keys are past keys that other rows
//              of the block read, their P is an exact 0, and V is assumed finite there, as the backward assumes
//              everywhere.  dK/dV: each head's sub-stream is the diagonal step, unmasked steps, and the edge step
//              kbk + w when kbk + w <= n - 1: G (min(n - 1, kbk + w) - kbk + 1) steps, the head boundary's prefetch
//              going from a head's edge block to the next head's diagonal block.  The grid orders stay: all blocks
//              with qb >= w (kbk <= n - 1 - w) weigh the same, so heaviest-first is harmless.
//
// Rows read or staged, by hand (n = S / 64; block b is rows 64 b .. 64 b + 63, inside [0, S) iff 0 <= b < n;
// `last` = qb when causal, n - 1 when not; `first` = kbk when causal, 0 when not; hk = h / G < Hkv):
//   forward, dQ   registers: Q (and dO), lse rows 64 qb + 16 w + 0 .. 15, qb = 0 .. n - 1.  Streamed K / V of head
//                 hk: first block 0, last block `last` (the prefetch of step kb stages kb + 1 only if kb + 1 <= last;
//                 the dQ kernel's second pass starts over at block 0 and ends at `last` again).
//                   first workgroup  causal: qb = n - 1, blocks 0 .. n - 1.  bidirectional: qb = 0, blocks 0 .. n - 1.
//                   last workgroup   causal: qb = 0, block 0 only, no prefetch (dQ: block 0 twice).
//                                    bidirectional: qb = n - 1, blocks 0 .. n - 1.
//                   S = 64           n = 1, qb = 0, block 0 only (dQ: twice), no other row touched.
//   dK/dV         resident: K, V block kbk = 0 .. n - 1 of head hk.  Streamed Q / dO, lse and dsum rows:
//                   first step     t = 0: head hk * G, block `first`, staged before the loop into slot 0.
//                   inside a head  the prefetch of (head, qb) with qb < n - 1 stages (head, qb + 1), qb + 1 <= n - 1.
//                   head boundary  the prefetch of (head, n - 1) with head < hk * G + G - 1 stages (head + 1, first);
//                                  head + 1 <= hk * G + G - 1 <= H - 1.
//                   last step      head hk * G + G - 1, block n - 1: t + 1 = G * (n - first), no prefetch.
//                   last workgroup kbk = n - 1; causal: first = n - 1, G steps, each block n - 1 of the next head.
//                   G = 1          hk = h: blocks `first` .. n - 1 of the one head, no head boundary; the last
//                                  workgroup, causal: block n - 1 only, no prefetch.
//                   S = 64         n = 1, first = 0: G steps, block 0 of heads hk * G .. hk * G + G - 1; every
//                                  prefetch is a head switch; G = 1: one step, no prefetch.
//   band          forward, dQ: first block max(0, qb - w) >= 0, last block qb <= n - 1; the edge step (qb >= w) stages
//                 qb - w + 1 <= qb since w >= 1; the dQ kernel's second pass starts over at the same first block.
//                 dK/dV: a head's blocks are kbk .. last = min(n - 1, kbk + w) (GroupStream.n = last + 1); inside a
//                 head the prefetch stages qb + 1 <= last, at a head boundary (head + 1, kbk), nothing behind the last
//                 head's block `last`.
//                   first workgroup  forward, dQ: qb = n - 1, blocks max(0, n - 1 - w) .. n - 1.  dK/dV: kbk = 0,
//                                    blocks 0 .. min(n - 1, w) of each head.
//                   last workgroup   forward, dQ: qb = 0, first = 0, block 0 only, no edge step (0 >= w is false).
//                                    dK/dV: kbk = n - 1, kbk + w > n - 1: no edge step, block n - 1 of each head.
//                   S = 64           n = 1: qb = kbk = 0, block 0 only, no edge step in any kernel.
//                   w >= n           qb - w < 0 and kbk + w > n - 1 everywhere: no edge step, first = 0, last = n - 1,
//                                    the causal rows above.
//                   w = 1            forward, dQ, qb >= 1: the edge block qb - 1 (slot 0) and the diagonal qb (slot 1),
//                                    the loop of unmasked steps is empty.  dK/dV, kbk <= n - 2: the diagonal step kbk
//                                    and the edge step kbk + 1 per head, 2 G steps.
//   columns       every staged or loaded row is 128 bf16 (256 bytes): Q, dq at h * 128 < H * 128; K, dk at
//                 (H + hk) * 128 < (H + Hkv) * 128; V, dv at (H + Hkv + hk) * 128 < RS; dO, out at h * 128 of H * 128.
//   dsum          the dQ kernel writes all 64 rows of its block and every (query head, block) has a workgroup: all
//                 [B, H, S] values are written before the dK/dV kernel reads them (stream order).
//   pv_diagonal   LDS rows of V: keys < q0 by MFMA (32-key steps below q0 + 16, the upper half zeroed in registers
//                 where it is the triangle's), keys q0 .. q0 + 15 on the VALU, none beyond (q0 = 16 w).
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
#include "attention_stream.hpp"

#include <stdexcept>

namespace kfk {

namespace {

constexpr int D2 = 128;         // head dim
constexpr int IMG = BK * 256;   // bytes of a 64-row image of 256-byte rows
constexpr int TD = D2 / 16;     // accumulator tiles over the head dim
constexpr int KS = D2 / 32;     // MFMA K-steps over the head dim
constexpr int FWD_LDS = 4 * IMG + BLK;      // ring 2 x (K, V); P
constexpr int DQ_LDS = 4 * IMG + BLK;       // ring 2 x (K, V); dS
constexpr int DKV_LDS = 6 * IMG + 2 * BLK;  // K, V; ring 2 x (Q, dO); P_drop; dS
// The MASK of a block step, with qq / kk the query's and the key's row inside their 64-row blocks:
constexpr int NOMASK = 0;  // every key visible
constexpr int DIAG = 1;    // the diagonal block: visible iff kk <= qq
constexpr int EDGE = 2;    // the band's edge block, w blocks before the query block: visible iff kk > qq

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
// in this lane, rows q0 .. of the block's P image): scores, online softmax, dropout, P V.  DIAG (the diagonal
// block) sets the scores of keys > row to -inf first; every row sees its own key there, and for query blocks > 0
// the running max is already finite, so exp(-inf - m) = 0 exactly and no row is empty.
// EDGE (the band's first step, m_run = -inf, l_run = 0, o = 0) sets the keys kk <= qq to -inf: the block's last row
// sees none, its m stays -inf, and the exponentials are taken against 0 instead (header: Band), so alpha = e = 0 and
// the row leaves the step as it entered it.  The plain MFMA follows: the masked P are exact zeros and V is finite.
template <int MASK>
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
            if constexpr (MASK == DIAG) acc[j][r] = key0 + 16 * j + 4 * lg + r > row ? -INFINITY : acc[j][r];
            if constexpr (MASK == EDGE) acc[j][r] = 16 * j + 4 * lg + r > q0 + lc ? acc[j][r] : -INFINITY;
            m = fmaxf(m, acc[j][r]);
        }
    m = fmaxf(m, __shfl_xor(m, 16));
    m = fmaxf(m, __shfl_xor(m, 32));
    float mref = m;  // what the exponentials are taken against: the maximum, but never -inf
    if constexpr (MASK == EDGE) mref = m == -INFINITY ? 0.f : m;
    const float alpha = __expf(m_run - mref);  // 0 at the first block (m_run = -inf, mref finite)
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < TK; ++j) {
        const int kb0 = 16 * j + 4 * lg;
        float p[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float e = __expf(acc[j][r] - mref);
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
    if constexpr (MASK == DIAG) {
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
// would put its rounding into dS = P o (dP - D)).  DIAG: keys > row count as P = 0; EDGE: keys kk <= qq do
// (qq = row % 64: a query block starts at a multiple of 64).
template <int MASK>
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
            if constexpr (MASK == DIAG) p = key <= row ? p : 0.f;
            if constexpr (MASK == EDGE) p = key - key0 > (row & (BK - 1)) ? p : 0.f;
            if (keep_elem(seed, bh, row, key, a.thresh)) t += p * dp[j][r];
        }
    return t * a.inv_keep;
}

// P_drop and dS of the same 16 x 64 tile into row `lrow` of the 64 x 64 images Si (and Pi when not null).
template <int MASK>
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
            if constexpr (MASK == DIAG) p = key0 + kb0 + r <= row ? p : 0.f;
            if constexpr (MASK == EDGE) p = kb0 + r > (row & (BK - 1)) ? p : 0.f;
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

// (two waves per SIMD: the register budget that lets two workgroups share a CU, as their 72 KB of LDS do)
// w: the band's width in blocks (BAND only; header: Band)
template <bool CAUSAL, bool BAND = false>
KFK_NO_PK_F32 __global__ __launch_bounds__(256, 2) void attn_gqa_fwd_kernel(AttnArgs a, int Hkv, int S, int w) {
    static_assert(CAUSAL || !BAND, "a band is causal");
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
    const int first = BAND ? max(0, qb - w) : 0;  // the first streamed key block; the edge block iff qb >= w
    {
        const int64_t r0 = static_cast<int64_t>(first) * BK * RS;
        const uint16_t *kv[2] = {kbase + r0, vbase + r0};
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
    const int nkb = CAUSAL ? qb + 1 : n;     // streamed key blocks first .. nkb - 1
    const int nfull = CAUSAL ? qb : n;       // of which not the diagonal
    int kb = first;  // block kb is step kb - first of the stream, in ring slot (kb - first) & 1
    if constexpr (BAND) {
        if (qb >= w) {  // the edge block qb - w, the first step (slot 0), outside the loop; block first + 1 <= qb is next
            wait_vmcnt<0>();
            __syncthreads();
            const int64_t r0 = static_cast<int64_t>(kb + 1) * BK * RS;
            const uint16_t *kv[2] = {kbase + r0, vbase + r0};
            stage_rows256<2>(ring + 2 * IMG, kv, strd, wave, lane);
            fwd_block<EDGE>(a, seed, bh, qf, ring, ring + IMG, Pi, q0, row, kb * BK, lane, m_run, l_run, o);
            ++kb;
        }
    }
    for (; kb < nfull; ++kb) {
        wait_vmcnt<0>();
        __syncthreads();
        const uint8_t *Ki = ring + ((kb - first) & 1) * 2 * IMG, *Vi = Ki + IMG;
        if (kb + 1 < nkb) {
            const int64_t r0 = static_cast<int64_t>(kb + 1) * BK * RS;
            const uint16_t *kv[2] = {kbase + r0, vbase + r0};
            stage_rows256<2>(ring + ((kb + 1 - first) & 1) * 2 * IMG, kv, strd, wave, lane);
        }
        fwd_block<NOMASK>(a, seed, bh, qf, Ki, Vi, Pi, q0, row, kb * BK, lane, m_run, l_run, o);
    }
    if constexpr (CAUSAL) {  // the diagonal block qb, last: nothing left to prefetch
        wait_vmcnt<0>();
        __syncthreads();
        const uint8_t *Ki = ring + ((qb - first) & 1) * 2 * IMG, *Vi = Ki + IMG;
        fwd_block<DIAG>(a, seed, bh, qf, Ki, Vi, Pi, q0, row, qb * BK, lane, m_run, l_run, o);
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

template <bool CAUSAL, bool ROPE, bool BAND = false>
KFK_NO_PK_F32 __global__ __launch_bounds__(256) void attn_gqa_dq_kernel(AttnArgs a, float *dsum_g, int Hkv, int S,
                                                                        const float *cos_t, const float *sin_t,
                                                                        int w) {
    static_assert(CAUSAL || !BAND, "a band is causal");
    extern __shared__ __attribute__((aligned(1024))) uint8_t lds[];
    uint8_t *ring = lds, *Si = lds + 4 * IMG;  // ring: 2 x (K, V)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = S / BK, G = a.H / Hkv;
    int bh, qb;
    gqa_block_of<CAUSAL>(n, G, bh, qb);
    const int b = bh / a.H, h = bh - b * a.H, hk = h / G;
    const int D = a.H * D2, RS = D + 2 * Hkv * D2;
    const int first = BAND ? max(0, qb - w) : 0;        // the edge block iff qb >= w
    const int nb = (CAUSAL ? qb + 1 : n) - first;       // streamed key blocks first .. first + nb - 1
    const uint32_t seed = call_seed(a);
    const uint16_t *seq = a.qkv + static_cast<int64_t>(b) * S * RS;
    const uint16_t *kbase = seq + D + hk * D2 + static_cast<int64_t>(first) * BK * RS;  // row 0 of block `first`
    const uint16_t *vbase = kbase + Hkv * D2;
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
    // last step of each pass is the diagonal block; band: the first is the edge block where there is one
    for (int it = 0; it < 2 * nb; ++it) {
        wait_vmcnt<0>();
        __syncthreads();
        const int kb = first + (it < nb ? it : it - nb);
        const bool diag = CAUSAL && kb == qb;
        const bool edge = BAND && kb + w == qb;
        const uint8_t *Ki = ring + (it & 1) * 2 * IMG, *Vi = Ki + IMG;
        if (it + 1 < 2 * nb) {
            const int nx = it + 1 < nb ? it + 1 : it + 1 - nb;  // <= nb - 1: block first + nx <= qb (n - 1)
            const int64_t r0 = static_cast<int64_t>(nx) * BK * RS;
            const uint16_t *kv[2] = {kbase + r0, vbase + r0};
            stage_rows256<2>(ring + ((it + 1) & 1) * 2 * IMG, kv, strd, wave, lane);
        }
        if (it < nb) {
            dd += diag   ? bwd_dsum<DIAG>(a, seed, bh, qf, gf, Ki, Vi, row, kb * BK, l, lane)
                  : edge ? bwd_dsum<EDGE>(a, seed, bh, qf, gf, Ki, Vi, row, kb * BK, l, lane)
                         : bwd_dsum<NOMASK>(a, seed, bh, qf, gf, Ki, Vi, row, kb * BK, l, lane);
            if (it == nb - 1) {  // the query's four lanes (lg) hold 16 keys of every block each
                dd += __shfl_xor(dd, 16);
                dd += __shfl_xor(dd, 32);
                if (lg == 0) dsum_g[static_cast<int64_t>(bh) * S + row] = dd;
            }
            continue;
        }
        if (diag) bwd_scores<DIAG>(a, seed, bh, qf, gf, Ki, Vi, nullptr, Si, qw0 + lc, row, kb * BK, l, dd, lane);
        else if (edge) bwd_scores<EDGE>(a, seed, bh, qf, gf, Ki, Vi, nullptr, Si, qw0 + lc, row, kb * BK, l, dd, lane);
        else bwd_scores<NOMASK>(a, seed, bh, qf, gf, Ki, Vi, nullptr, Si, qw0 + lc, row, kb * BK, l, dd, lane);
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
    int RS, D, S, n, first;      // a head's sub-stream is blocks first .. n - 1 (band: n - 1 is min(S / 64 - 1, first + w))
    int hlast;                   // the group's last query head
};

// One dK/dV step on the staged block qb of query head h (ring slot `slot`), after starting the DMA of the stream's next
// step into the other slot: block qb + 1 of h, or block `first` of head h + 1 behind h's last block; nothing behind
// the last head's last block.  MASK: the diagonal block (keys beyond a query give P = dS = 0) or the band's edge block
// (keys kk <= qq do), chosen outside.
template <int MASK>
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

template <bool CAUSAL, bool ROPE, bool BAND = false>
KFK_NO_PK_F32 __global__ __launch_bounds__(256) void attn_gqa_dkv_kernel(AttnArgs a, const float *dsum_g, int Hkv,
                                                                         int S, const float *cos_t,
                                                                         const float *sin_t, int w) {
    static_assert(CAUSAL || !BAND, "a band is causal");
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
    // band: query blocks beyond kbk + w see nothing of this key block, and block kbk + w is the edge block
    const bool has_edge = BAND && kbk + w < nbs;
    g.RS = RS, g.D = D, g.S = S, g.n = has_edge ? kbk + w + 1 : nbs, g.first = CAUSAL ? kbk : 0, g.hlast = h0 + G - 1;
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
            dkv_step<DIAG>(a, dsum_g, seed, g, b, h, qb, kbk, slot, lds, wave, lane, dv, dk);
            ++qb, slot ^= 1;
        }
        for (; qb < g.n - has_edge; ++qb, slot ^= 1)
            dkv_step<NOMASK>(a, dsum_g, seed, g, b, h, qb, kbk, slot, lds, wave, lane, dv, dk);
        if (has_edge) {  // and the edge block kbk + w >= kbk + 1 closes it
            dkv_step<EDGE>(a, dsum_g, seed, g, b, h, qb, kbk, slot, lds, wave, lane, dv, dk);
            slot ^= 1;
        }
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

// -> the band's width in blocks (0: no window)
int check(int B, int S, int H, int Hkv, bool causal, int window) {
    if (!attention_gqa_supported(S, H, Hkv, window))
        throw std::invalid_argument("attention: head dim 128 needs S % 64 == 0, 64 <= S <= 1024 (8192 with a window, "
                                    "a positive multiple of 64), 1 <= kv_heads <= heads and heads % kv_heads == 0");
    if (window && !causal) throw std::invalid_argument("attention: a window needs causal attention");
    if (static_cast<int64_t>(B) * H * (S / BK) > INT32_MAX)
        throw std::invalid_argument("attention: B * heads * S / 64 workgroups do not fit one grid");
    return window / BK;
}

template <bool CAUSAL, bool BAND = false>
void forward(const AttnArgs &a, int Hkv, int grid, int S, hipStream_t s, int w = 0) {
    static const bool attr = (raise_lds(attn_gqa_fwd_kernel<CAUSAL, BAND>, FWD_LDS), true);
    (void)attr;
    attn_gqa_fwd_kernel<CAUSAL, BAND><<<grid, 256, FWD_LDS, s>>>(a, Hkv, S, w);
}

template <bool CAUSAL, bool ROPE, bool BAND = false>
void backward(const AttnArgs &a, float *dsum, int Hkv, int B, int S, const float *cos, const float *sin,
              hipStream_t s, int w = 0) {
    static const bool attr = (raise_lds(attn_gqa_dq_kernel<CAUSAL, ROPE, BAND>, DQ_LDS),
                              raise_lds(attn_gqa_dkv_kernel<CAUSAL, ROPE, BAND>, DKV_LDS), true);
    (void)attr;
    const int n = S / BK;
    // the dQ kernel fills all [B, H, S] of dsum, the dK/dV kernel reads them (stream order)
    attn_gqa_dq_kernel<CAUSAL, ROPE, BAND><<<B * a.H * n, 256, DQ_LDS, s>>>(a, dsum, Hkv, S, cos, sin, w);
    attn_gqa_dkv_kernel<CAUSAL, ROPE, BAND><<<B * Hkv * n, 256, DKV_LDS, s>>>(a, dsum, Hkv, S, cos, sin, w);
}

}  // namespace

bool attention_d128_supported(int S) { return S >= 64 && S <= 1024 && S % 64 == 0; }

bool attention_gqa_supported(int S, int heads, int kv_heads, int window) {
    const bool s_ok = window == 0 ? attention_d128_supported(S)
                                  : window > 0 && window % 64 == 0 && S >= 64 && S <= kAttentionWindowMaxS && S % 64 == 0;
    return s_ok && kv_heads >= 1 && heads >= kv_heads && heads % kv_heads == 0;
}

void launch_attention_gqa_forward(const uint16_t *qkv, uint16_t *out, float *lse, int B, int S, int H, int Hkv,
                                  float scale, uint32_t seed, float p_drop, bool causal, hipStream_t s, int window) {
    const int w = check(B, S, H, Hkv, causal, window);
    const AttnArgs a = make_args(qkv, out, lse, nullptr, nullptr, H, scale, seed, p_drop);
    const int grid = B * H * (S / BK);
    if (w) forward<true, true>(a, Hkv, grid, S, s, w);
    else if (causal) forward<true>(a, Hkv, grid, S, s);
    else forward<false>(a, Hkv, grid, S, s);
}

void launch_attention_gqa_backward(const uint16_t *qkv, const uint16_t *out, const float *lse, const uint16_t *dout,
                                   uint16_t *dqkv, float *dsum, int B, int S, int H, int Hkv, float scale,
                                   uint32_t seed, float p_drop, bool causal, hipStream_t s, const float *cos,
                                   const float *sin, int window) {
    const int w = check(B, S, H, Hkv, causal, window);
    if (!cos != !sin) throw std::invalid_argument("attention: the rotary tables cos and sin come together");
    if (!dsum) throw std::invalid_argument("attention: the head dim 128 backward needs the [B, H, S] f32 dsum buffer");
    const AttnArgs a = make_args(qkv, const_cast<uint16_t *>(out), const_cast<float *>(lse), dout, dqkv, H, scale, seed,
                                 p_drop);
    if (w) {
        if (cos) backward<true, true, true>(a, dsum, Hkv, B, S, cos, sin, s, w);
        else backward<true, false, true>(a, dsum, Hkv, B, S, nullptr, nullptr, s, w);
    } else if (cos) {
        if (causal) backward<true, true>(a, dsum, Hkv, B, S, cos, sin, s);
        else backward<false, true>(a, dsum, Hkv, B, S, cos, sin, s);
    } else {
        if (causal) backward<true, false>(a, dsum, Hkv, B, S, nullptr, nullptr, s);
        else backward<false, false>(a, dsum, Hkv, B, S, nullptr, nullptr, s);
    }
}

}  // namespace kfk
