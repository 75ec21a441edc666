// Weight gradient of the 1x1 / 3x3 NHWC bf16 convolutions (stride 1 or 2) on CDNA4
// matrix cores, for gfx950: a split-K GEMM over output pixels.
//
//   dw[co, kh, kw, ci] = sum_p dy[p, co] * x[n, oh*s + kh - pad, ow*s + kw - pad, ci]
//   GEMM: M = Cout, N = Cin (one tap per tile), K = P = N*OH*OW output pixels
//
// Why: the weight gradients were the last convolution pass on MIOpen (5.4 ms of a 25 ms
// ResNet-50 step plus 0.6 ms of its split-K zero-fills and casts, profiles/README.md).
// Both operands carry the reduction index (the pixel) as their ROW and the GEMM index
// (channel) contiguous, the "NT" layout: tiles are staged global->LDS unchanged
// (16-byte global_load_lds, rows of BM or BN channels) and every MFMA operand is read
// with the gfx950 transposing LDS read ds_read_b64_tr_b16, which hands each lane 4
// pixels of one channel -- no register/ds_write transpose pass.
//
// LDS image: rows of 128 or 256 bytes (64 / 128 channels), 32-byte column groups
// XOR-swizzled by the row (hswz, mfma_util.hpp) so the 8 rows one 32-lane half of a
// transposing read touches (two 4-row blocks 8 rows apart) land on 8 distinct
// 32-byte bank groups: conflict-free.  The swizzle is applied on the staging source
// address (global_load_lds writes fixed LDS offsets) and on the read address.
//
// Split-K: P is 12.5 K .. 800 K pixels while M x N is at most 2048 x 512, so each
// workgroup reduces a contiguous pixel range; partial f32 tiles go to a workspace in
// the accumulator's native register order (coalesced 16-byte stores) and a second
// kernel sums the splits, converts and scatters to [Cout][KS*KS][Cin] (deterministic).
// Accumulating into an f32 destination (e.g. a flat f32 gradient slot) the splits add
// their tiles with f32 atomics instead: no workspace, no second pass.  Workgroups of one
// split are launched together (same pixel rows in L2) and remapped XCD-contiguously.
//
// Reference parity: the reference has no kernels of its own; it trains
// tf.keras.applications ResNet-50 with TF's stock convolutions
// (benchmarks/system/benchmark_kungfu.py:96).
//
// Which of these kernels a shape gets, on which tile and with how many splits, is decided in
// wgrad_plan.cpp (host-only); this file holds the kernels, whose geometry arguments (WGeo, RGeo,
// RRGeo) that planner fills, and the one launcher that runs a plan.
#include "common.hpp"
#include "kernels.hpp"
#include "mfma_util.hpp"

#include <stdexcept>

namespace kfk {

const void *zero_page();  // conv.hip

namespace {

constexpr int kBK = 64;  // pixels per K-step

// Cache policy of the split-K kernel's LDS-DMA operand loads: non-temporal (aux = 2).  Measured
// on the ResNet-50 step (r3h, tools/gpu_r3_ntconv.sh): +1 % with nt on both operands; the same
// hint on the forward / data-gradient conv kernel's activation loads cost 1.5-2 %.
constexpr int kWgradAux = 2;

// WM x WN waves (wave tile 64 co x 16*TN ci), STAGES-deep global_load_lds ring; S = stride.
// KS = 1 | 3 (pad (KS-1)/2), or 0: a KH x KW window with padding (g.kwin, g.ph, g.pw) at run
// time (Inception-v3's 1x7 / 7x1 / 1x3 / 3x1 / 5x5 / 3x3-pad-0).  Channel counts that are not
// multiples of the tile: channels past Cout / Cin read the zero page, their outputs are dropped.
// KB: pixels per staged K-step (64, or 32 with a deeper ring: the 256x256 tile holds only two
// 64-deep stages -- every K-step then waits for ALL its LDS-DMA -- but four 32-deep ones, which
// keep two K-steps in flight across the barrier; gemm.hip uses the same structure).
template <int KS, int S, int WM, int WN, int STAGES, int TN = 4, int KB = 64>
__global__ __launch_bounds__(64 * WM * WN) void wgrad_kernel(const uint16_t *__restrict__ dy,
                                                             const uint16_t *__restrict__ x,
                                                             float *__restrict__ part, void *__restrict__ dw,
                                                             const uint16_t *__restrict__ zero, WGeo g,
                                                             int out_f32, int accumulate, int atomic_out,
                                                             int stagger) {
    constexpr int BM = 64 * WM, BN = 16 * TN * WN, NW = WM * WN, NT = 64 * NW;
    constexpr int PAD = KS > 0 ? (KS - 1) / 2 : 0;
    constexpr int ROWA = BM * 2, ROWB = BN * 2;  // bytes per staged pixel row
    constexpr int CPRA = ROWA / 16, CPRB = ROWB / 16;
    constexpr int RPIA = 64 / CPRA, RPIB = 64 / CPRB;  // rows per 1 KB glds instruction
    constexpr int A_BYTES = KB * ROWA, B_BYTES = KB * ROWB, STAGE = A_BYTES + B_BYTES;
    constexpr int A_INST = KB / RPIA / NW, B_INST = KB / RPIB / NW;
    constexpr int LOADS = A_INST + B_INST;
    static_assert(A_INST >= 1 && B_INST >= 1 && A_INST * NW * RPIA == KB && B_INST * NW * RPIB == KB, "split");
    static_assert(KB == 32 || KB == 64, "K-step of 32 or 64 pixels");
    constexpr bool IDENT = KS == 1 && S == 1;
    __shared__ __attribute__((aligned(1024))) uint8_t lds[STAGES * STAGE];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wg = xcd_remap(blockIdx.x, gridDim.x);
    const int split = wg / g.tiles, tile = wg - split * g.tiles;
    const int mn = g.mtiles * g.ntiles;
    const int tap = tile / mn, rem = tile - tap * mn;
    const int mt = rem / g.ntiles, nt = rem - mt * g.ntiles;
    const int kwin = KS > 0 ? KS : g.kwin;
    const int kh = tap / kwin, kw = tap - kh * kwin;
    const int pad_h = KS > 0 ? PAD : g.ph, pad_w = KS > 0 ? PAD : g.pw;
    const int m0 = mt * BM, n0 = nt * BN;
    const int p_begin = split * g.kps * kBK;  // the plan's splits are in 64-pixel steps
    int nsteps = (g.P - p_begin + KB - 1) / KB;
    if (nsteps > g.kps * (kBK / KB)) nsteps = g.kps * (kBK / KB);

    // ---- staging descriptors: lane l of an instruction writes image bytes [16l, 16l+16)
    int a_row[A_INST], a_col[A_INST];
#pragma unroll
    for (int j = 0; j < A_INST; ++j) {
        const int r = (wave * A_INST + j) * RPIA + lane / CPRA;
        const int pc = lane % CPRA;
        const int lc = (((pc >> 1) ^ hswz<ROWA>(r)) << 1) | (pc & 1);
        a_row[j] = r;
        a_col[j] = m0 + lc * 8;
    }
    int b_row[B_INST], b_col[B_INST];
#pragma unroll
    for (int j = 0; j < B_INST; ++j) {
        const int r = (wave * B_INST + j) * RPIB + lane / CPRB;
        const int pc = lane % CPRB;
        const int lc = (((pc >> 1) ^ hswz<ROWB>(r)) << 1) | (pc & 1);
        b_row[j] = r;
        b_col[j] = n0 + lc * 8;
    }

    auto stage = [&](int ks, int buf) {
        const int p0 = p_begin + ks * KB;
        uint8_t *abase = lds + buf * STAGE;
        uint8_t *bbase = abase + A_BYTES;
#pragma unroll
        for (int j = 0; j < A_INST; ++j) {
            const int p = p0 + a_row[j];
            const uint16_t *src = p < g.P && a_col[j] < g.K ? dy + static_cast<uint32_t>(p * g.K + a_col[j]) : zero;
            __builtin_amdgcn_global_load_lds(src, abase + (wave * A_INST + j) * 1024, 16, 0, kWgradAux);
        }
#pragma unroll
        for (int j = 0; j < B_INST; ++j) {
            const int p = p0 + b_row[j];
            uint32_t eo = 0xFFFFFFFFu;  // element offset into x, or out of range
            if constexpr (IDENT) {
                if (p < g.P && b_col[j] < g.C) eo = static_cast<uint32_t>(p * g.C + b_col[j]);
            } else {
                const int n = fdiv(p, g.m_hw);
                const int r = p - n * g.HW;
                const int oh = fdiv(r, g.m_ow);
                const int ow = r - oh * g.OW;
                const int ih = oh * S + kh - pad_h, iw = ow * S + kw - pad_w;
                if (p < g.P && b_col[j] < g.C && static_cast<unsigned>(ih) < static_cast<unsigned>(g.H) &&
                    static_cast<unsigned>(iw) < static_cast<unsigned>(g.W))
                    eo = static_cast<uint32_t>(((n * g.H + ih) * g.W + iw) * g.C + b_col[j]);
            }
            const uint16_t *src = eo == 0xFFFFFFFFu ? zero : x + eo;
            __builtin_amdgcn_global_load_lds(src, bbase + (wave * B_INST + j) * 1024, 16, 0, kWgradAux);
        }
    };

    // ---- fragment read addresses (transposing reads; see file comment)
    // lane = 16 g + 4 q + p: block rows kb + q (kb = 32 s + 8 g [+4]), columns 16 c + 4 p.
    const int wm = wave / WN, wn = wave % WN;
    const int fg = lane >> 4, fq = (lane >> 2) & 3, fp = lane & 3;
    const int rowa0 = 8 * fg + fq;  // hswz is the same for rows rowa0 + {0, 4, 32, 36}
    int aoff[4], boff[TN];
#pragma unroll
    for (int i = 0; i < 4; ++i) aoff[i] = rowa0 * ROWA + 32 * ((wm * 4 + i) ^ hswz<ROWA>(rowa0)) + 8 * fp;
#pragma unroll
    for (int j = 0; j < TN; ++j) boff[j] = rowa0 * ROWB + 32 * ((wn * TN + j) ^ hswz<ROWB>(rowa0)) + 8 * fp;

    f32x4 acc[4][TN];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    auto mfma_block = [&](const bf16x8 (&af)[4], const bf16x8 (&bfr)[TN]) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
    };

#pragma unroll
    for (int p = 0; p < STAGES - 1; ++p)
        if (p < nsteps) stage(p, p);
    int buf = 0;
    // stagger (fixed per tile in the launcher): the upper half of the waves (one per SIMD with 8 waves) issues its
    // LDS-DMA staging before its fragment reads instead of between its two MFMA clusters, so the two
    // waves sharing a SIMD do not stall on staging issue at the same time
    // stagger 1: stage before the fragment reads; 2: after the second MFMA cluster (upper wave half)
    const bool upper = NW >= 8 && ((wave >> 2) & 1);
    const bool early = (stagger & 3) == 1 && upper, late = (stagger & 3) == 2 && upper;
    if ((stagger & 4) && upper) __builtin_amdgcn_s_setprio(1);  // stagger bit 2: static priority
    for (int ks = 0; ks < nsteps; ++ks) {
        if (ks + STAGES - 1 <= nsteps) wait_vmcnt<LOADS * (STAGES - 2)>();
        else wait_vmcnt<0>();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        if (early && ks + STAGES - 1 < nsteps) {
            int nb = buf + STAGES - 1;
            if (nb >= STAGES) nb -= STAGES;
            stage(ks + STAGES - 1, nb);
        }
        __builtin_amdgcn_sched_barrier(0);
        const uint8_t *abase = lds + buf * STAGE;
        const uint8_t *bbase = abase + A_BYTES;
        bf16x8 af0[4], bf0[TN];
#pragma unroll
        for (int i = 0; i < 4; ++i) af0[i] = tr_frag(abase + aoff[i], abase + aoff[i] + 4 * ROWA);
#pragma unroll
        for (int j = 0; j < TN; ++j) bf0[j] = tr_frag(bbase + boff[j], bbase + boff[j] + 4 * ROWB);
        if constexpr (KB == 64) {
            bf16x8 af1[4], bf1[TN];
#pragma unroll
            for (int i = 0; i < 4; ++i) af1[i] = tr_frag(abase + aoff[i] + 32 * ROWA, abase + aoff[i] + 36 * ROWA);
#pragma unroll
            for (int j = 0; j < TN; ++j) bf1[j] = tr_frag(bbase + boff[j] + 32 * ROWB, bbase + boff[j] + 36 * ROWB);
            mfma_block(af0, bf0);
            __builtin_amdgcn_sched_barrier(0);
            if (!early && !late && ks + STAGES - 1 < nsteps) {
                int nb = buf + STAGES - 1;
                if (nb >= STAGES) nb -= STAGES;
                stage(ks + STAGES - 1, nb);
            }
            __builtin_amdgcn_sched_barrier(0);
            mfma_block(af1, bf1);
        } else {
            // one 32-deep sub-step: stage the slot read at ks-1 first, then compute
            if (!early && !late && ks + STAGES - 1 < nsteps) {
                int nb = buf + STAGES - 1;
                if (nb >= STAGES) nb -= STAGES;
                stage(ks + STAGES - 1, nb);
            }
            __builtin_amdgcn_sched_barrier(0);
            mfma_block(af0, bf0);
        }
        if (late && ks + STAGES - 1 < nsteps) {
            __builtin_amdgcn_sched_barrier(0);
            int nb = buf + STAGES - 1;
            if (nb >= STAGES) nb -= STAGES;
            stage(ks + STAGES - 1, nb);
        }
        buf = buf + 1 == STAGES ? 0 : buf + 1;
    }
    wait_vmcnt<0>();

    // ---- epilogue.  C map (16x16): col (ci) = lane & 15, row (co) = (lane >> 4) * 4 + r.
    if (atomic_out) {
        // f32 destination, every split adds its tile in place (no workspace, no reduce pass)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int co = m0 + wm * 64 + i * 16 + (lane >> 4) * 4 + r;
                    const int ci = n0 + wn * 16 * TN + j * 16 + (lane & 15);
                    if (co >= g.K || ci >= g.C) continue;
                    const int64_t e = (static_cast<int64_t>(co) * g.taps + tap) * g.C + ci;
                    atomicAdd(static_cast<float *>(dw) + e, acc[i][j][r]);
                }
    } else if (g.splits == 1) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int co = m0 + wm * 64 + i * 16 + (lane >> 4) * 4 + r;
                    const int ci = n0 + wn * 16 * TN + j * 16 + (lane & 15);
                    if (co >= g.K || ci >= g.C) continue;
                    const int64_t e = (static_cast<int64_t>(co) * g.taps + tap) * g.C + ci;
                    float v = acc[i][j][r];
                    if (out_f32) {
                        float *o = static_cast<float *>(dw) + e;
                        *o = accumulate ? *o + v : v;
                    } else {
                        uint16_t *o = static_cast<uint16_t *>(dw) + e;
                        if (accumulate) v += bf16_to_f32(*o);
                        *o = f32_to_bf16(v);
                    }
                }
    } else {
        f32x4 *dst = reinterpret_cast<f32x4 *>(part + static_cast<int64_t>(wg) * (BM * BN)) + tid;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) dst[(i * TN + j) * NT] = acc[i][j];
    }
}

// ---------------------------------------------------------------------------------------
// Row-image 3x3 / stride-1 weight gradient for narrow channel tiles (64 co x 64 ci per tap).
//
// wgrad_kernel runs one workgroup per TAP: every tap re-stages its own copy of dy and of the
// shifted input, and a 64x64 tile is one wave whose 16 LDS-DMA pieces per K-step cost more
// issue time than its 32 MFMAs (VGG-16 64->64 at 224x224: 247 TF/s; ResNet-50 layer1: 238).
// Here ONE workgroup of 9 waves (wave = tap) shares each K-step's staging:
//   * a K-step is a segment of 64 output pixels: 64 consecutive pixels of one output row
//     (OW >= 64) or R = 64 / OW whole rows (OW < 64);
//   * dy is staged as 64 pixel rows (A operand, as in wgrad_kernel), the input as an image of
//     the (R + 2) input rows x (L + 2) pixels around the segment, zero-padded at the borders;
//   * tap (kh, kw)'s B operand is that image read at row offset kh * (L + 2) + kw: the
//     transposing reads (ds_read_b64_tr_b16) take per-lane row addresses, so the im2col shift
//     is only an address offset -- every input pixel is staged once per segment.
// 33-35 LDS-DMA pieces per K-step are spread over the 9 waves (4 each) against 32 MFMAs per
// wave.  Partial tiles use wgrad_kernel's workspace order (reduced by wgrad_reduce_kernel).
__global__ __launch_bounds__(576) void wgrad_rows_kernel(const uint16_t *__restrict__ dy,
                                                         const uint16_t *__restrict__ x,
                                                         float *__restrict__ part, void *__restrict__ dw,
                                                         const uint16_t *__restrict__ zero, RGeo g, int out_f32,
                                                         int accumulate, int atomic_out, int stagger) {
    constexpr int STAGES = 2;           // LDS ring depth (34 KB per stage)
    constexpr int ROW = 128;            // 64 channels
    constexpr int MAXP = 4;             // pieces per wave per K-step (9 * 4 >= 8 + 25)
    constexpr int STAGE = (8 + 25 + 1) * 1024;  // dy 8 KB | input image <= 25 KB | dummy 1 KB
    constexpr int DUMMY = (8 + 25) * 1024;
    __shared__ __attribute__((aligned(1024))) uint8_t lds[STAGES * STAGE];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // = tap
    const int kh = wave / 3, kw = wave - 3 * (wave / 3);
    const int wg = xcd_remap(blockIdx.x, gridDim.x);
    const int mn = g.mtiles * g.ntiles;
    const int split = wg / mn, ctile = wg - split * mn;
    const int mt = ctile / g.ntiles, nt = ctile - mt * g.ntiles;
    const int m0 = mt * 64, n0 = nt * 64;
    const int seg0 = split * g.kps;
    int nsteps = g.nseg - seg0;
    if (nsteps > g.kps) nsteps = g.kps;

    // ---- staging descriptors: wave issues pieces wave + 9u; piece < 8: dy, else input image
    const int total = 8 + g.xpieces;
    int p_kind[MAXP], p_r[MAXP], p_c[MAXP], p_col[MAXP];  // kind 0 dy, 1 x, 2 dummy
#pragma unroll
    for (int u = 0; u < MAXP; ++u) {
        const int pq = wave + 9 * u;
        const int pc = lane & 7;
        if (pq < 8) {
            const int t = pq * 8 + (lane >> 3);  // dy slot
            p_kind[u] = 0;
            p_r[u] = t / g.L;
            p_c[u] = t - p_r[u] * g.L;
            if (p_r[u] >= g.R) p_r[u] = 1 << 20;  // slot past the segment: invalid
            p_col[u] = m0 + ((((pc >> 1) ^ hswz<ROW>(t)) << 1) | (pc & 1)) * 8;
        } else if (pq < total) {
            const int t = (pq - 8) * 8 + (lane >> 3);  // image row
            p_kind[u] = 1;
            p_r[u] = t / g.XW;
            p_c[u] = t - p_r[u] * g.XW;
            if (t >= g.xrows) p_r[u] = 1 << 20;
            p_col[u] = n0 + ((((pc >> 1) ^ hswz<ROW>(t)) << 1) | (pc & 1)) * 8;
        } else {
            p_kind[u] = 2;
            p_r[u] = p_c[u] = p_col[u] = 0;
        }
    }
    const int segs_img = g.gpi * g.spr;
    auto stage = [&](int ks, int buf) {
        const int seg = seg0 + ks;
        const int n = seg / segs_img, rem = seg - n * segs_img;
        const int grp = rem / g.spr, sidx = rem - grp * g.spr;
        const int oh0 = grp * g.R, ow0 = sidx * 64;
        uint8_t *base = lds + buf * STAGE;
#pragma unroll
        for (int u = 0; u < MAXP; ++u) {
            const int pq = wave + 9 * u;
            const uint16_t *src = zero;
            uint8_t *dst = base + DUMMY;
            if (p_kind[u] == 0) {
                const int oh = oh0 + p_r[u], ow = ow0 + p_c[u];
                if (oh < g.H && ow < g.W) src = dy + static_cast<uint32_t>(((n * g.H + oh) * g.W + ow) * g.K + p_col[u]);
                dst = base + pq * 1024;
            } else if (p_kind[u] == 1) {
                const int ih = oh0 + p_r[u] - 1, iw = ow0 + p_c[u] - 1;
                if (static_cast<unsigned>(ih) < static_cast<unsigned>(g.H) &&
                    static_cast<unsigned>(iw) < static_cast<unsigned>(g.W))
                    src = x + static_cast<uint32_t>(((n * g.H + ih) * g.W + iw) * g.C + p_col[u]);
                dst = base + pq * 1024;
            }
            __builtin_amdgcn_global_load_lds(src, dst, 16, 0, 0);
        }
    };

    // ---- fragment addresses.  lane = 16 fg + 4 fq + fp; K-slots j = 8 fg + fq + {0, 4, 32, 36}.
    const int fg = lane >> 4, fq = (lane >> 2) & 3, fp = lane & 3;
    const int rowa0 = 8 * fg + fq;
    int aoff[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) aoff[i] = rowa0 * ROW + 32 * (i ^ hswz<ROW>(rowa0)) + 8 * fp;
    int boff[4][4];  // [sub-read][ci block]
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int j = rowa0 + (s & 1) * 4 + (s >> 1) * 32;
        const int r = j / g.L, c = j - r * g.L;
        const int jrow = r < g.R ? r * g.XW + c : 0;  // slots past the segment read a staged row (dy is 0)
        const int trow = jrow + kh * g.XW + kw;
        const int h = hswz<ROW>(trow);
#pragma unroll
        for (int i = 0; i < 4; ++i) boff[s][i] = 8192 + trow * ROW + 32 * (i ^ h) + 8 * fp;
    }

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    auto mfma_block = [&](const bf16x8 (&af)[4], const bf16x8 (&bfr)[4]) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
    };

#pragma unroll
    for (int p = 0; p < STAGES - 1; ++p)
        if (p < nsteps) stage(p, p);
    int buf = 0;
    const bool early = stagger && ((wave >> 2) & 1);  // see wgrad_kernel: staggered staging issue
    for (int ks = 0; ks < nsteps; ++ks) {
        if (ks + STAGES - 1 <= nsteps) wait_vmcnt<MAXP * (STAGES - 2)>();
        else wait_vmcnt<0>();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        if (early && ks + STAGES - 1 < nsteps) {
            int nb = buf + STAGES - 1;
            if (nb >= STAGES) nb -= STAGES;
            stage(ks + STAGES - 1, nb);
        }
        __builtin_amdgcn_sched_barrier(0);
        const uint8_t *base = lds + buf * STAGE;
        bf16x8 af0[4], bf0[4], af1[4], bf1[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            af0[i] = tr_frag(base + aoff[i], base + aoff[i] + 4 * ROW);
            bf0[i] = tr_frag(base + boff[0][i], base + boff[1][i]);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            af1[i] = tr_frag(base + aoff[i] + 32 * ROW, base + aoff[i] + 36 * ROW);
            bf1[i] = tr_frag(base + boff[2][i], base + boff[3][i]);
        }
        mfma_block(af0, bf0);
        __builtin_amdgcn_sched_barrier(0);
        if (!early && ks + STAGES - 1 < nsteps) {
            int nb = buf + STAGES - 1;
            if (nb >= STAGES) nb -= STAGES;
            stage(ks + STAGES - 1, nb);
        }
        __builtin_amdgcn_sched_barrier(0);
        mfma_block(af1, bf1);
        buf = buf + 1 == STAGES ? 0 : buf + 1;
    }
    wait_vmcnt<0>();

    // ---- epilogue (wgrad_kernel's three forms; tile = this wave's tap)
    const int tap = wave, taps = 9;
    if (atomic_out || g.splits == 1) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int co = m0 + i * 16 + (lane >> 4) * 4 + r;
                    const int ci = n0 + j * 16 + (lane & 15);
                    const int64_t e = (static_cast<int64_t>(co) * taps + tap) * g.C + ci;
                    float v = acc[i][j][r];
                    if (atomic_out) {
                        atomicAdd(static_cast<float *>(dw) + e, v);
                    } else if (out_f32) {
                        float *o = static_cast<float *>(dw) + e;
                        *o = accumulate ? *o + v : v;
                    } else {
                        uint16_t *o = static_cast<uint16_t *>(dw) + e;
                        if (accumulate) v += bf16_to_f32(*o);
                        *o = f32_to_bf16(v);
                    }
                }
    } else {
        const int tile = tap * mn + mt * g.ntiles + nt;
        f32x4 *dst = reinterpret_cast<f32x4 *>(part + (static_cast<int64_t>(split) * g.tiles + tile) * 4096) + lane;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) dst[(i * 4 + j) * 64] = acc[i][j];
    }
}

// ---------------------------------------------------------------------------------------
// Row-image weight gradient for ANY stride-1 KH x KW window with zero padding and channel
// counts % 8 (Inception-v3's narrow multi-tap layers: 32..192 channels, 1x7 / 7x1 / 3x3 /
// 5x5, pad 0 or (K-1)/2), the generalisation of wgrad_rows_kernel above:
//   * output tile 64 co x 64 ci per wave and tap; channels past Cout / Cin are staged from the
//     zero page and their outputs dropped (48 -> one half-empty tile, 80 -> 64 + 16, ...);
//   * a workgroup holds NWV waves = NWV consecutive taps of the window (taps > NWV: the window
//     is split over tap groups, e.g. 5x5 = 9 + 9 + 7 taps; idle waves of the last group only
//     stage) and shares one K-step's staging among them: dy as 64 pixel rows, the input as the
//     (R + KH - 1) x (L + KW - 1) image around the segment of 64 output pixels;
//   * tap (kh, kw) reads the image at row offset kh * XW + kw (transposing LDS reads with
//     per-lane row addresses: the im2col shift is only an address offset).
// CT = the channel tile (both co and ci): 64, or 32 for the channel counts that are not multiples
// of 64 (Inception's 32 / 80 / 96 / 160 / 48: no zero-padded half tiles, 64-byte staged rows, a
// 32 x 32 wave tile) -- CT 32 also writes its split partials in dw layout ([split][co][tap][ci],
// exactly K * taps * C floats, no tile padding), summed by wgrad_dense_reduce_kernel.
// Replaces MIOpen's igemm_wrw for these shapes (r2o_inception_wgrad.txt: 170-275 TF/s there).
// s_waitcnt until at most n * (S - 2) loads of this wave are in flight (n = its loads per stage,
// wave-uniform, 1..5): the oldest outstanding stage of an S-deep ring has landed
template <int S>
__device__ __forceinline__ void wait_ring(int n) {
    if constexpr (S <= 2) {
        wait_vmcnt<0>();
    } else {
        switch (n) {
            case 1: wait_vmcnt<1 * (S - 2)>(); break;
            case 2: wait_vmcnt<2 * (S - 2)>(); break;
            case 3: wait_vmcnt<3 * (S - 2)>(); break;
            case 4: wait_vmcnt<4 * (S - 2)>(); break;
            case 5: wait_vmcnt<5 * (S - 2)>(); break;
            default: wait_vmcnt<0>();
        }
    }
}

template <int NWV, int STAGES, int CT = 64, bool DENSE = (CT == 32)>
__global__ __launch_bounds__(64 * NWV) void wgrad_rows_rect_kernel(const uint16_t *__restrict__ dy,
                                                                   const uint16_t *__restrict__ x,
                                                                   float *__restrict__ part, void *__restrict__ dw,
                                                                   const uint16_t *__restrict__ zero, RRGeo g,
                                                                   int out_f32, int accumulate, int atomic_out,
                                                                   int stagger) {
    constexpr int ROW = 2 * CT;                    // staged bytes per pixel (CT channels)
    constexpr int TI = CT / 16;                    // 16-wide MFMA blocks per tile side
    constexpr int LPR = ROW / 16;                  // lanes (16 B each) per staged row
    constexpr int RPP = 64 / LPR;                  // rows per 1 KB piece
    constexpr int DYP = 64 / RPP;                  // dy pieces per K-step (64 pixels)
    constexpr int DYB = DYP * 1024;
    constexpr int MAXP = (DYP + 25 + NWV - 1) / NWV;  // 1 KB pieces per wave per K-step (bound)
    static_assert(MAXP <= 5, "wait_ring covers 5 loads per stage");
    extern __shared__ __attribute__((aligned(1024))) uint8_t lds[];  // STAGES x g.stage bytes
    const int STAGE = g.stage;                   // dy | input image (<= 25 KB) | dummy 1 KB
    const int DUMMY = g.stage - 1024;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wg = xcd_remap(blockIdx.x, gridDim.x);
    const int mn = g.mtiles * g.ntiles;
    const int per_split = mn * g.tgroups;
    const int split = wg / per_split, rem0 = wg - split * per_split;
    const int tg = rem0 / mn, ctile = rem0 - tg * mn;
    const int mt = ctile / g.ntiles, nt = ctile - mt * g.ntiles;
    const int m0 = mt * CT, n0 = nt * CT;
    const int tap = tg * NWV + wave;  // >= g.taps: staging-only wave
    const bool has_tap = tap < g.taps;
    const int kh = has_tap ? tap / g.KW : 0, kw = has_tap ? tap - kh * g.KW : 0;
    const int seg0 = split * g.kps;
    int nsteps = g.nseg - seg0;
    if (nsteps > g.kps) nsteps = g.kps;

    // ---- staging descriptors: wave issues pieces wave + NWV u; piece < 8: dy, else input image
    const int total = DYP + g.xpieces;
    const int nload = (total + NWV - 1) / NWV;  // pieces per wave per stage (a ring > 2 issues them all)
    int p_kind[MAXP], p_r[MAXP], p_c[MAXP], p_col[MAXP];  // kind 0 dy, 1 x, 2 dummy
    bool p_cok[MAXP];
#pragma unroll
    for (int u = 0; u < MAXP; ++u) {
        const int pq = wave + NWV * u;
        const int pc = lane % LPR;
        p_cok[u] = false;
        if (pq < DYP) {
            const int t = pq * RPP + lane / LPR;  // dy slot
            p_kind[u] = 0;
            p_r[u] = t / g.L;
            p_c[u] = t - p_r[u] * g.L;
            if (p_r[u] >= g.R) p_r[u] = 1 << 20;  // slot past the segment: invalid
            p_col[u] = m0 + ((((pc >> 1) ^ hswz<ROW>(t)) << 1) | (pc & 1)) * 8;
            p_cok[u] = p_col[u] < g.K;
        } else if (pq < total) {
            const int t = (pq - DYP) * RPP + lane / LPR;  // image row
            p_kind[u] = 1;
            p_r[u] = t / g.XW;
            p_c[u] = t - p_r[u] * g.XW;
            if (t >= g.xrows) p_r[u] = 1 << 20;
            p_col[u] = n0 + ((((pc >> 1) ^ hswz<ROW>(t)) << 1) | (pc & 1)) * 8;
            p_cok[u] = p_col[u] < g.C;
        } else {
            p_kind[u] = 2;
            p_r[u] = p_c[u] = p_col[u] = 0;
        }
    }
    const int segs_img = g.gpi * g.spr;
    auto stage = [&](int ks, int buf) {
        const int seg = seg0 + ks;
        const int n = seg / segs_img, rem = seg - n * segs_img;
        const int grp = rem / g.spr, sidx = rem - grp * g.spr;
        const int oh0 = grp * g.R, ow0 = sidx * g.L;
        uint8_t *base = lds + buf * STAGE;
#pragma unroll
        for (int u = 0; u < MAXP; ++u) {
            if (u >= nload) break;
            const int pq = wave + NWV * u;
            if constexpr (STAGES == 2) {
                // every K-step waits for all of its loads (vmcnt 0), so no dummy issue keeps the
                // count; lanes of channels past Cout / Cin leave their LDS bytes stale (they only
                // reach outputs that are dropped)
                if (p_kind[u] == 2 || !p_cok[u]) continue;
            }
            const uint16_t *src = zero;
            uint8_t *dst = base + DUMMY;
            if (p_kind[u] == 0) {
                const int oh = oh0 + p_r[u], ow = ow0 + p_c[u];
                if (oh < g.OH && ow < g.OW && p_cok[u])
                    src = dy + static_cast<uint32_t>(((n * g.OH + oh) * g.OW + ow) * g.K + p_col[u]);
                dst = base + pq * 1024;
            } else if (p_kind[u] == 1) {
                const int ih = oh0 * g.S + p_r[u] - g.ph, iw = ow0 * g.S + p_c[u] - g.pw;
                if (static_cast<unsigned>(ih) < static_cast<unsigned>(g.H) &&
                    static_cast<unsigned>(iw) < static_cast<unsigned>(g.W) && p_cok[u])
                    src = x + static_cast<uint32_t>(((n * g.H + ih) * g.W + iw) * g.C + p_col[u]);
                dst = base + pq * 1024;
            }
            __builtin_amdgcn_global_load_lds(src, dst, 16, 0, 0);
        }
    };

    // ---- fragment addresses.  lane = 16 fg + 4 fq + fp; K-slots j = 8 fg + fq + {0, 4, 32, 36}.
    const int fg = lane >> 4, fq = (lane >> 2) & 3, fp = lane & 3;
    const int rowa0 = 8 * fg + fq;
    int aoff[TI];
#pragma unroll
    for (int i = 0; i < TI; ++i) aoff[i] = rowa0 * ROW + 32 * (i ^ hswz<ROW>(rowa0)) + 8 * fp;
    int boff[4][TI];  // [sub-read][ci block]
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int j = rowa0 + (s & 1) * 4 + (s >> 1) * 32;
        const int r = j / g.L, c = j - r * g.L;
        // output (r, c) of the segment sits at image row S r, column S c; slots past it read a staged
        // row (their dy is 0)
        const int jrow = r < g.R ? r * g.S * g.XW + g.S * c : 0;
        const int trow = jrow + kh * g.XW + kw;
        const int h = hswz<ROW>(trow);
#pragma unroll
        for (int i = 0; i < TI; ++i) boff[s][i] = DYB + trow * ROW + 32 * (i ^ h) + 8 * fp;
    }

    f32x4 acc[TI][TI];
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < TI; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    auto mfma_block = [&](const bf16x8 (&af)[TI], const bf16x8 (&bfr)[TI]) {
#pragma unroll
        for (int i = 0; i < TI; ++i)
#pragma unroll
            for (int j = 0; j < TI; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
    };

#pragma unroll
    for (int p = 0; p < STAGES - 1; ++p)
        if (p < nsteps) stage(p, p);
    int buf = 0;
    const bool early = stagger && ((wave >> 2) & 1);  // see wgrad_kernel: staggered staging issue
    for (int ks = 0; ks < nsteps; ++ks) {
        if (ks + STAGES - 1 <= nsteps) wait_ring<STAGES>(nload);
        else wait_vmcnt<0>();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        if ((early || !has_tap) && ks + STAGES - 1 < nsteps) {
            int nb = buf + STAGES - 1;
            if (nb >= STAGES) nb -= STAGES;
            stage(ks + STAGES - 1, nb);
        }
        __builtin_amdgcn_sched_barrier(0);
        const uint8_t *base = lds + buf * STAGE;
        if (has_tap) {  // wave-uniform
            bf16x8 af0[TI], bf0[TI], af1[TI], bf1[TI];
#pragma unroll
            for (int i = 0; i < TI; ++i) {
                af0[i] = tr_frag(base + aoff[i], base + aoff[i] + 4 * ROW);
                bf0[i] = tr_frag(base + boff[0][i], base + boff[1][i]);
            }
#pragma unroll
            for (int i = 0; i < TI; ++i) {
                af1[i] = tr_frag(base + aoff[i] + 32 * ROW, base + aoff[i] + 36 * ROW);
                bf1[i] = tr_frag(base + boff[2][i], base + boff[3][i]);
            }
            mfma_block(af0, bf0);
            __builtin_amdgcn_sched_barrier(0);
            if (!early && ks + STAGES - 1 < nsteps) {
                int nb = buf + STAGES - 1;
                if (nb >= STAGES) nb -= STAGES;
                stage(ks + STAGES - 1, nb);
            }
            __builtin_amdgcn_sched_barrier(0);
            mfma_block(af1, bf1);
        }
        buf = buf + 1 == STAGES ? 0 : buf + 1;
    }
    wait_vmcnt<0>();
    if (!has_tap) return;

    // ---- epilogue (wgrad_kernel's three forms; tile = this wave's tap)
    if constexpr (DENSE) {
        if (!atomic_out && g.splits > 1) {  // dw-layout partial of this split: plain f32 stores
            float *dst = part + static_cast<int64_t>(split) * g.K * g.taps * g.C;
#pragma unroll
            for (int i = 0; i < TI; ++i)
#pragma unroll
                for (int j = 0; j < TI; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int co = m0 + i * 16 + (lane >> 4) * 4 + r;
                        const int ci = n0 + j * 16 + (lane & 15);
                        if (co < g.K && ci < g.C) dst[(static_cast<int64_t>(co) * g.taps + tap) * g.C + ci] = acc[i][j][r];
                    }
            return;
        }
    }
    if (atomic_out || g.splits == 1) {
#pragma unroll
        for (int i = 0; i < TI; ++i)
#pragma unroll
            for (int j = 0; j < TI; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int co = m0 + i * 16 + (lane >> 4) * 4 + r;
                    const int ci = n0 + j * 16 + (lane & 15);
                    if (co >= g.K || ci >= g.C) continue;
                    const int64_t e = (static_cast<int64_t>(co) * g.taps + tap) * g.C + ci;
                    float v = acc[i][j][r];
                    if (atomic_out) {
                        atomicAdd(static_cast<float *>(dw) + e, v);
                    } else if (out_f32) {
                        float *o = static_cast<float *>(dw) + e;
                        *o = accumulate ? *o + v : v;
                    } else {
                        uint16_t *o = static_cast<uint16_t *>(dw) + e;
                        if (accumulate) v += bf16_to_f32(*o);
                        *o = f32_to_bf16(v);
                    }
                }
    } else if constexpr (!DENSE) {
        const int tile = tap * mn + mt * g.ntiles + nt;
        f32x4 *dst = reinterpret_cast<f32x4 *>(part + (static_cast<int64_t>(split) * g.tiles + tile) * 4096) + lane;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) dst[(i * 4 + j) * 64] = acc[i][j];
    }
}

// dw[e] (+)= the sum over the splits of part[split][e] (deterministic: a fixed order for a given
// shape); e over the n = K * taps * C outputs in dw layout, as float4 columns (n % 4 == 0: C % 8).
// Block = 256 threads = (256 >> sgl) columns x (1 << sgl) split groups: group g sums splits g, g + G,
// ... in order, then the G group sums meet in LDS in group order -- a few thousand columns over
// hundreds of splits (Conv2d_2a: 2,304 x 768) still keep every CU's loads in flight.
__global__ __launch_bounds__(256) void wgrad_dense_reduce_kernel(const float *__restrict__ part, int splits, int64_t n,
                                                                 void *__restrict__ dw, int out_f32, int accumulate,
                                                                 int sgl) {
    __shared__ f32x4 red[256];
    const int G = 1 << sgl, COLS = 256 >> sgl;
    const int t = threadIdx.x, c = t & (COLS - 1), grp = t >> (8 - sgl);
    const int64_t n4 = n / 4, col = static_cast<int64_t>(blockIdx.x) * COLS + c;
    f32x4 a = f32x4{0.f, 0.f, 0.f, 0.f};
    if (col < n4) {
        const f32x4 *src = reinterpret_cast<const f32x4 *>(part) + col;
        int sp = grp;
        for (; sp + G < splits; sp += 2 * G) {
            const f32x4 u = src[sp * n4], v = src[(sp + G) * n4];
            a += u;
            a += v;
        }
        if (sp < splits) a += src[sp * n4];
    }
    red[t] = a;
    __syncthreads();
    if (grp != 0 || col >= n4) return;
    f32x4 sum = red[c];
    for (int k = 1; k < G; ++k) sum += red[k * COLS + c];
    const int64_t e = col * 4;
    if (out_f32) {
        f32x4 *o = reinterpret_cast<f32x4 *>(static_cast<float *>(dw) + e);
        if (accumulate) sum += *o;
        *o = sum;
    } else {
        uint16_t *o = static_cast<uint16_t *>(dw) + e;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float v = sum[k];
            if (accumulate) v += bf16_to_f32(o[k]);
            o[k] = f32_to_bf16(v);
        }
    }
}

// Sum the split partials (workspace order of wgrad_kernel) and scatter to dw.
// Block = 256 threads = OUT float4 outputs x SG split groups (SG = 256 / OUT, a power of
// two <= splits): a few K outputs with hundreds of splits (the 56x56 layers) still keep
// every CU's loads in flight; the SG partial sums meet in LDS.
template <int WM, int WN, int TN = 4>
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float *__restrict__ part, void *__restrict__ dw,
                                                           WGeo g, int out_f32, int accumulate, int sg_log2) {
    constexpr int BM = 64 * WM, BN = 16 * TN * WN, NT = 64 * WM * WN;
    constexpr int TILE4 = BM * BN / 4;
    __shared__ f32x4 red[256];
    const int SG = 1 << sg_log2, OUT = 256 >> sg_log2;
    const int t = threadIdx.x, o = t & (OUT - 1), sg = t >> (8 - sg_log2);
    const int64_t total = static_cast<int64_t>(g.tiles) * TILE4;
    const int64_t idx = static_cast<int64_t>(blockIdx.x) * OUT + o;
    const int64_t stride_split = total;
    f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
    if (idx < total) {
        const f32x4 *src = reinterpret_cast<const f32x4 *>(part) + idx;
        int sp = sg;
        for (; sp + 3 * SG < g.splits; sp += 4 * SG) {
            const f32x4 a = src[sp * stride_split];
            const f32x4 b = src[(sp + SG) * stride_split];
            const f32x4 c = src[(sp + 2 * SG) * stride_split];
            const f32x4 d = src[(sp + 3 * SG) * stride_split];
            s += (a + b) + (c + d);
        }
        for (; sp < g.splits; sp += SG) s += src[sp * stride_split];
    }
    red[t] = s;
    __syncthreads();
    if (sg == 0 && idx < total) {
        for (int k = 1; k < SG; ++k) s += red[o + k * OUT];
        const int tile = static_cast<int>(idx / TILE4);
        const int rem = static_cast<int>(idx - static_cast<int64_t>(tile) * TILE4);
        const int ij = rem / NT, tid = rem - ij * NT;
        const int mn = g.mtiles * g.ntiles;
        const int tap = tile / mn, r2 = tile - tap * mn;
        const int mt = r2 / g.ntiles, nt = r2 - mt * g.ntiles;
        const int lane = tid & 63, wave = tid >> 6;
        const int wm = wave / WN, wn = wave % WN;
        const int i = ij / TN, j = ij % TN;
        const int ci = nt * BN + wn * 16 * TN + j * 16 + (lane & 15);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int co = mt * BM + wm * 64 + i * 16 + (lane >> 4) * 4 + r;
            if (co >= g.K || ci >= g.C) continue;
            const int64_t e = (static_cast<int64_t>(co) * g.taps + tap) * g.C + ci;
            float v = s[r];
            if (out_f32) {
                float *d = static_cast<float *>(dw) + e;
                *d = accumulate ? *d + v : v;
            } else {
                uint16_t *d = static_cast<uint16_t *>(dw) + e;
                if (accumulate) v += bf16_to_f32(*d);
                *d = f32_to_bf16(v);
            }
        }
    }
}

// Staggered staging issue (see wgrad_kernel) is on in every row-image launch below (stagger = 1; same-box
// A/Bs: Inception-v3 21.62 -> 21.45 ms/step, VGG-16 34.85 -> 34.62, ResNet-50 neutral).

template <int WM, int WN, int TN = 4>
void reduce_tiles(const float *part, void *dw, const WGeo &g, bool out_f32, bool accumulate, hipStream_t s) {
    const WgradReduceLaunch r = wgrad_reduce_launch(static_cast<int64_t>(g.tiles) * (64 * WM) * (16 * TN * WN) / 4, g.splits);
    wgrad_reduce_kernel<WM, WN, TN><<<r.grid, 256, 0, s>>>(part, dw, g, out_f32, accumulate, r.sg_log2);
}

// the fields wgrad_reduce_kernel reads, for the row-image kernels' 64 x 64 partial tiles
WGeo reduce_geo(int Cin, int Cout, int mtiles, int ntiles, int taps, int tiles, int splits) {
    WGeo g{};
    g.C = Cin, g.K = Cout, g.mtiles = mtiles, g.ntiles = ntiles, g.taps = taps, g.tiles = tiles, g.splits = splits;
    return g;
}

template <int KS, int S, int WM, int WN, int TN = 4>
void launch_t(const uint16_t *dy, const uint16_t *x, void *dw, float *part, const WGeo &g, bool out_f32,
              bool accumulate, bool atomic_out, hipStream_t s) {
    // 3-deep global_load_lds ring (tools/bench_wgrad.py --sweep: 2 stages starve the 8-wave
    // 256x128 tiles, 4 stages cost the 1-2 wave tiles their second/third workgroup per CU);
    // 2 for the 256x256 tile (64 KB per stage)
    constexpr int STAGE_BYTES = 64 * (64 * WM + 16 * TN * WN) * 2;
    constexpr int STAGES = 3 * STAGE_BYTES <= 160 * 1024 ? 3 : 2;
    // staggered staging issue: on for the 256x256 tiles only -- BERT-base's long-K linear weight
    // gradients +1.5 % step time, ResNet-50's 256x128 tiles -0.8 % with it (tools/gpu_r3_envab.sh)
    const int stagger = TN == 8 ? 1 : 0;
    // (256x256 tiles with four 32-pixel stages, KB = 32, instead of two 64-pixel ones: measured no better, r4t1)
    wgrad_kernel<KS, S, WM, WN, STAGES, TN><<<g.tiles * g.splits, 64 * WM * WN, 0, s>>>(
        dy, x, part, dw, reinterpret_cast<const uint16_t *>(zero_page()), g, out_f32, accumulate, atomic_out, stagger);
    if (g.splits > 1 && !atomic_out) reduce_tiles<WM, WN, TN>(part, dw, g, out_f32, accumulate, s);
}

template <int KS, int S>
void launch_ks(const uint16_t *dy, const uint16_t *x, void *dw, float *part, const WGeo &g, int variant,
               bool out_f32, bool accumulate, bool atomic_out, hipStream_t s) {
    switch (variant) {
    case kWgradTile128x128: launch_t<KS, S, 2, 2>(dy, x, dw, part, g, out_f32, accumulate, atomic_out, s); break;
    case kWgradTile128x64: launch_t<KS, S, 2, 1>(dy, x, dw, part, g, out_f32, accumulate, atomic_out, s); break;
    case kWgradTile64x128: launch_t<KS, S, 1, 2>(dy, x, dw, part, g, out_f32, accumulate, atomic_out, s); break;
    case kWgradTile64x64: launch_t<KS, S, 1, 1>(dy, x, dw, part, g, out_f32, accumulate, atomic_out, s); break;
    case kWgradTile256x128: launch_t<KS, S, 4, 2>(dy, x, dw, part, g, out_f32, accumulate, atomic_out, s); break;
    case kWgradTile128x256: launch_t<KS, S, 2, 4>(dy, x, dw, part, g, out_f32, accumulate, atomic_out, s); break;
    default: launch_t<KS, S, 4, 2, 8>(dy, x, dw, part, g, out_f32, accumulate, atomic_out, s); break;  // 256x256
    }
}

void launch_tiled(const uint16_t *dy, const uint16_t *x, void *dw, float *part, const WgradPlan &plan, bool out_f32,
                  bool accumulate, bool atomic_out, hipStream_t s) {
    const WGeo &g = plan.tiled;
    const int64_t P = plan.shape.P();
    if (P * g.HW >= (int64_t(1) << 40) || P >= (1 << 23))
        throw std::invalid_argument("conv_wgrad: too many pixels for the 40-bit division");
    // 1x1 and 3x3 / pad 1 have the window compiled in, any other window reads it from g
    const bool k1 = g.taps == 1 && g.ph == 0 && g.pw == 0, k3 = g.taps == 9 && g.kwin == 3 && g.ph == 1 && g.pw == 1;
    if (plan.shape.stride == 1) {
        if (k1) launch_ks<1, 1>(dy, x, dw, part, g, plan.variant, out_f32, accumulate, atomic_out, s);
        else if (k3) launch_ks<3, 1>(dy, x, dw, part, g, plan.variant, out_f32, accumulate, atomic_out, s);
        else launch_ks<0, 1>(dy, x, dw, part, g, plan.variant, out_f32, accumulate, atomic_out, s);
    } else {
        if (k1) launch_ks<1, 2>(dy, x, dw, part, g, plan.variant, out_f32, accumulate, atomic_out, s);
        else if (k3) launch_ks<3, 2>(dy, x, dw, part, g, plan.variant, out_f32, accumulate, atomic_out, s);
        else launch_ks<0, 2>(dy, x, dw, part, g, plan.variant, out_f32, accumulate, atomic_out, s);
    }
}

// RowsRect: wgrad_rows_rect_kernel<7|9, 2>, 64 x 64 partial tiles; RowsRing: <7|9, stages, ct, true>, dw-layout partials
void launch_rows_rect(const uint16_t *dy, const uint16_t *x, void *dw, float *part, const WgradPlan &plan, bool out_f32,
                      bool accumulate, bool atomic_out, hipStream_t s) {
    const RRGeo &g = plan.rect;
    const int grid = g.mtiles * g.ntiles * g.tgroups * g.splits;
    const uint16_t *z = reinterpret_cast<const uint16_t *>(zero_page());
    const int lds = plan.stages * g.stage;
    const bool t7 = g.taps % 7 == 0;  // 7 waves for the 1x7 / 7x1 / 7x7 windows, else 9
    static bool attr_set[kWgradRing64x4 + 1][2] = {};  // per instantiation, once
    auto go = [&](auto kern, int nwv) {
        bool &done = attr_set[plan.variant][t7 ? 1 : 0];
        if (!done) {
            (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      160 * 1024);
            done = true;
        }
        kern<<<grid, 64 * nwv, lds, s>>>(dy, x, part, dw, z, g, out_f32, accumulate, atomic_out, 1);
    };
    switch (plan.variant) {
    case kWgradRows: t7 ? go(wgrad_rows_rect_kernel<7, 2>, 7) : go(wgrad_rows_rect_kernel<9, 2>, 9); break;
    case kWgradRing32x2: t7 ? go(wgrad_rows_rect_kernel<7, 2, 32, true>, 7) : go(wgrad_rows_rect_kernel<9, 2, 32, true>, 9); break;
    case kWgradRing32x3: t7 ? go(wgrad_rows_rect_kernel<7, 3, 32, true>, 7) : go(wgrad_rows_rect_kernel<9, 3, 32, true>, 9); break;
    case kWgradRing32x4: t7 ? go(wgrad_rows_rect_kernel<7, 4, 32, true>, 7) : go(wgrad_rows_rect_kernel<9, 4, 32, true>, 9); break;
    case kWgradRing64x3: t7 ? go(wgrad_rows_rect_kernel<7, 3, 64, true>, 7) : go(wgrad_rows_rect_kernel<9, 3, 64, true>, 9); break;
    default: t7 ? go(wgrad_rows_rect_kernel<7, 4, 64, true>, 7) : go(wgrad_rows_rect_kernel<9, 4, 64, true>, 9); break;  // 64x4
    }
    if (g.splits == 1 || atomic_out) return;
    if (plan.kernel == WgradKernel::RowsRect) {
        reduce_tiles<1, 1>(part, dw, reduce_geo(g.C, g.K, g.mtiles, g.ntiles, g.taps, g.tiles, g.splits), out_f32, accumulate, s);
    } else {
        const int64_t n = static_cast<int64_t>(g.K) * g.taps * g.C;
        // split groups: up to 64, ~8 splits each, while >= 1,024 blocks of columns... or fewer
        int sgl = 0;
        while (sgl < 6 && (8 << sgl) < g.splits && (n / 4) * (2 << sgl) <= int64_t(1024) * 256) ++sgl;
        const int cols = 256 >> sgl;
        wgrad_dense_reduce_kernel<<<static_cast<int>((n / 4 + cols - 1) / cols), 256, 0, s>>>(part, g.splits, n, dw, out_f32,
                                                                                           accumulate, sgl);
    }
}

}  // namespace

void launch_conv_wgrad(const uint16_t *dy, const uint16_t *x, void *dw, float *part, const WgradPlan &plan, bool out_f32,
                       bool accumulate, hipStream_t s, bool atomics) {
    // split-K accumulating into an f32 destination: every split adds its tile with atomics (unless
    // `atomics` is off: then partial tiles + the deterministic reduce, which adds into dw)
    const bool atomic_out = atomics && out_f32 && accumulate && plan.splits > 1;
    if (plan.splits > 1 && !atomic_out && part == nullptr) throw std::invalid_argument("conv_wgrad: split-K needs the workspace");
    switch (plan.kernel) {
    case WgradKernel::Tiled: launch_tiled(dy, x, dw, part, plan, out_f32, accumulate, atomic_out, s); break;
    case WgradKernel::Rows3x3: {
        const RGeo &g = plan.rows;
        wgrad_rows_kernel<<<g.mtiles * g.ntiles * g.splits, 576, 0, s>>>(
            dy, x, part, dw, reinterpret_cast<const uint16_t *>(zero_page()), g, out_f32, accumulate, atomic_out, 1);
        if (g.splits > 1 && !atomic_out)
            reduce_tiles<1, 1>(part, dw, reduce_geo(g.C, g.K, g.mtiles, g.ntiles, 9, g.tiles, g.splits), out_f32, accumulate, s);
        break;
    }
    default: launch_rows_rect(dy, x, dw, part, plan, out_f32, accumulate, atomic_out, s); break;
    }
}

}  // namespace kfk
