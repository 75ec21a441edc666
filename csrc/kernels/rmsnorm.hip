// Fused residual-add + RMSNorm for pre-norm decoder blocks (the LLaMA family), bf16 in/out, f32 gamma and
// statistics, for gfx950.  No mean, no beta, no dropout.
//
//   forward   s = bf16(x + r) (optional r; f32 add, one rounding);  rstd = rsqrt(mean(s^2) + eps) over the STORED s;
//             y = bf16(s * rstd * gamma)
//   backward  g = dy * gamma;  c = rstd^3 * (sum_D g * s) / D;  ds = bf16(ds_in + rstd * g - s * c)
//             dgamma[col] = sum_rows dy * s * rstd                                           (f32)
//             ds_in (optional) is the gradient reaching s from its other consumer, the skip path of the next add:
//             it joins in f32 ahead of the one rounding, so pre-norm's sum of the two gradients of s is no pass.
//             The row sum is taken over g * s, not over g * (s * rstd): one multiply less per element, and a sum
//             of small integers stays exact in any order.
//
// Interface    rows of D contiguous bf16, D % 256 == 0, 256 <= D <= 8192; gamma f32 [D]; rstd f32 [rows].
//              s is written only when r is given (otherwise s is x).
// Work split   A row belongs to a TEAM of T threads: one wave (T = 64) while D <= 2048, the whole 256-thread
//              workgroup (T = 256) above.  Thread t of its team owns the 8-element groups t, t + T, t + 2T, ... of
//              the row (16-byte accesses, coalesced across the team; NP = ceil(D / 8T) <= 4 groups, the last one
//              predicated on D), so its columns are FIXED over the rows it visits: gamma is loaded once per thread
//              and the backward's dgamma columns accumulate in registers over the team's grid-stride row loop.
//                D <= 2048   4 teams (waves) per workgroup, 4 rows in flight, the row sum by wave shuffles alone
//                D >  2048   1 team per workgroup: layernorm.hip's one-wave rows would need 128 f32 of row + 128
//                            of gamma per lane at D = 8192 (and dgamma on top); a quarter of that per thread here.
//                            The four waves' partial sums meet in LDS: lane 0 of each wave writes one float, one
//                            workgroup barrier, every thread adds the four in the same order.  The 4-float buffer
//                            alternates between two slots by row parity, so a row costs ONE barrier (a wave can
//                            write slot p again only after the barrier of the row between, which every wave
//                            reaches only after reading slot p).
//              The crossover is where a wave's registers stop holding the row: at D = 2048 a lane of the backward
//              holds 32 f32 of gamma, 32 of dgamma and the packed row, 154 VGPRs, three waves per SIMD; a fifth
//              group (D = 2304 .. 2560) would pass 170 VGPRs and leave two.  Both schemes top out at NP = 4 and
//              the same registers: the workgroup scheme carries four times the row on them
//              (profiles/llama_block.md has the table).
// Registers    Forward: the row as f32 (the rounded s when r is given) between the reduction and the store.
//              Backward: dy and s stay PACKED (the 16-byte words as loaded, 8 VGPRs per group instead of 16) and
//              are unpacked a second time after the reduction; g = dy * gamma is recomputed, one multiply.
// HBM          Each input element is read once per direction and each output element written once; gamma once per
//              thread (L2 after the first workgroup).  No scratch in any instantiation (kernel-resource-usage
//              remarks, recorded with VGPRs and occupancy in profiles/llama_block.md).
// dgamma       Deterministic, no atomics, no zeroed scratch: per-thread column sums in registers, then partial
//              [blocks][D] f32 (T = 64: the workgroup's four waves summed through a [4][D] LDS image first;
//              T = 256: every column has one owner, stored straight from registers), then rms_colsum_kernel with
//              16 independent f64 chains per column, the scheme of ln_bwd_kernel / ln_colsum_kernel.
// Rows read    Team `team` of workgroup b visits rows b * TEAMS + team + i * gridDim.x * TEAMS < rows; a group index
//              gi = p * T + t is touched only if gi < D / 8: no address beyond rows * D elements is formed.
#include "common.hpp"
#include "kernels.hpp"

#include <stdexcept>
#include <type_traits>

namespace kfk {

namespace {

constexpr int kRmsWaveMaxD = 2048;  // the crossover: one wave per row up to here, one workgroup per row above
constexpr int kRmsMaxD = 8192;

// Sum over the team; every thread of the team gets the same value.  T = 256: `red` is the [2][4] LDS buffer and
// `par` the row parity (see the header); all threads of the workgroup call this the same number of times.
template <int T>
__device__ __forceinline__ float team_sum(float v, float (*red)[4], int par) {
    v = wave_sum(v);
    if constexpr (T == 64) {
        return v;
    } else {
        if ((threadIdx.x & 63) == 0) red[par][threadIdx.x >> 6] = v;
        __syncthreads();
        return (red[par][0] + red[par][1]) + (red[par][2] + red[par][3]);
    }
}

__device__ __forceinline__ void load_gamma8(const float4 *gamma, int gi, float (&g)[8]) {
    const float4 a = gamma[2 * gi], b = gamma[2 * gi + 1];
    g[0] = a.x, g[1] = a.y, g[2] = a.z, g[3] = a.w;
    g[4] = b.x, g[5] = b.y, g[6] = b.z, g[7] = b.w;
}

template <int NP, int T>
__global__ __launch_bounds__(kBlock) void rms_fwd_kernel(const uint4 *__restrict__ x, const uint4 *__restrict__ r,
                                                         const float4 *__restrict__ gamma, uint4 *__restrict__ y,
                                                         uint4 *__restrict__ s_out, float *__restrict__ rstd,
                                                         int64_t rows, int D, float eps) {
    constexpr int TEAMS = kBlock / T;
    __shared__ float red[2][4];
    const int t = threadIdx.x & (T - 1), team = threadIdx.x / T;
    const int ng = D >> 3;
    const float inv_d = 1.f / D;
    float gm[NP][8];
#pragma unroll
    for (int p = 0; p < NP; ++p)
        if (p * T + t < ng) load_gamma8(gamma, p * T + t, gm[p]);
    const int64_t stride = static_cast<int64_t>(gridDim.x) * TEAMS;
    int par = 0;
    for (int64_t row = static_cast<int64_t>(blockIdx.x) * TEAMS + team; row < rows; row += stride, par ^= 1) {
        const int64_t base = row * ng;
        float v[NP][8];
        float ss = 0.f;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const int gi = p * T + t;
            if (gi < ng) {
                unpack_bf16x8(x[base + gi], v[p]);
                if (r) {
                    add_bf16x8(r[base + gi], v[p]);
                    // the residual stream is bf16: normalise exactly the values that are stored
                    const uint4 sv = pack_bf16x8(v[p]);
                    s_out[base + gi] = sv;
                    unpack_bf16x8(sv, v[p]);
                }
#pragma unroll
                for (int k = 0; k < 8; ++k) ss += v[p][k] * v[p][k];
            }
        }
        const float rs = rsqrtf(team_sum<T>(ss, red, par) * inv_d + eps);
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const int gi = p * T + t;
            if (gi < ng) {
                float o[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) o[k] = v[p][k] * rs * gm[p][k];
                y[base + gi] = pack_bf16x8(o);
            }
        }
        if (t == 0) rstd[row] = rs;
    }
}

template <int NP, int T>
__global__ __launch_bounds__(kBlock) void rms_bwd_kernel(const uint4 *__restrict__ dy, const uint4 *__restrict__ ds_in,
                                                         const uint4 *__restrict__ s, const float4 *__restrict__ gamma,
                                                         const float *__restrict__ rstd, uint4 *__restrict__ ds,
                                                         float *__restrict__ partial, int64_t rows, int D) {
    constexpr int TEAMS = kBlock / T;
    __shared__ float red[2][4];
    const int t = threadIdx.x & (T - 1), team = threadIdx.x / T;
    const int ng = D >> 3;
    const float inv_d = 1.f / D;
    float gm[NP][8], dg[NP][8];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        if (p * T + t < ng) load_gamma8(gamma, p * T + t, gm[p]);
#pragma unroll
        for (int k = 0; k < 8; ++k) dg[p][k] = 0.f;
    }
    const int64_t stride = static_cast<int64_t>(gridDim.x) * TEAMS;
    int par = 0;
    for (int64_t row = static_cast<int64_t>(blockIdx.x) * TEAMS + team; row < rows; row += stride, par ^= 1) {
        const int64_t base = row * ng;
        const float rs = rstd[row];
        uint4 dyw[NP], sw[NP];  // the row, packed as loaded
        float a = 0.f;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const int gi = p * T + t;
            if (gi < ng) {
                dyw[p] = dy[base + gi];
                sw[p] = s[base + gi];
                float d[8], sv[8];
                unpack_bf16x8(dyw[p], d);
                unpack_bf16x8(sw[p], sv);
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    a += (d[k] * gm[p][k]) * sv[k];
                    dg[p][k] += (d[k] * sv[k]) * rs;
                }
            }
        }
        const float c = ((rs * rs) * rs) * (team_sum<T>(a, red, par) * inv_d);
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const int gi = p * T + t;
            if (gi < ng) {
                float d[8], sv[8], o[8];
                unpack_bf16x8(dyw[p], d);
                unpack_bf16x8(sw[p], sv);
#pragma unroll
                for (int k = 0; k < 8; ++k) o[k] = rs * (d[k] * gm[p][k]);
                if (ds_in) add_bf16x8(ds_in[base + gi], o);
#pragma unroll
                for (int k = 0; k < 8; ++k) o[k] -= sv[k] * c;
                ds[base + gi] = pack_bf16x8(o);
            }
        }
    }
    // the per-thread column sums -> partial[block][D]
    float *out = partial + static_cast<int64_t>(blockIdx.x) * D;
    if constexpr (T == kBlock) {  // every column has one owner in the workgroup
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const int gi = p * T + t;
            if (gi < ng) {
                float4 *o4 = reinterpret_cast<float4 *>(out) + 2 * gi;
                o4[0] = make_float4(dg[p][0], dg[p][1], dg[p][2], dg[p][3]);
                o4[1] = make_float4(dg[p][4], dg[p][5], dg[p][6], dg[p][7]);
            }
        }
    } else {  // the four waves own the same columns: sum them through LDS in a fixed order
        __shared__ float cols[TEAMS][kRmsWaveMaxD];
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const int gi = p * T + t;
            if (gi < ng) {
#pragma unroll
                for (int k = 0; k < 8; ++k) cols[team][gi * 8 + k] = dg[p][k];
            }
        }
        __syncthreads();
        for (int col = threadIdx.x; col < D; col += kBlock) {
            float u = 0.f;
#pragma unroll
            for (int w = 0; w < TEAMS; ++w) u += cols[w][col];
            out[col] = u;
        }
    }
}

// dgamma[col] = sum_b partial[b][col].  Block = 64 consecutive columns x 16 row groups (coalesced 256-byte row
// segments, 16 independent f64 chains per column), then an LDS reduction over the groups in a fixed order.
constexpr int kRmsColGroups = 16;
__global__ __launch_bounds__(64 * kRmsColGroups) void rms_colsum_kernel(const float *__restrict__ partial, int nblocks,
                                                                        int D, float *__restrict__ dgamma) {
    __shared__ double red[kRmsColGroups][64];
    const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6;
    const int col = blockIdx.x * 64 + lane;  // D % 64 == 0: always a column
    double u = 0;
#pragma unroll 8
    for (int b = grp; b < nblocks; b += kRmsColGroups) u += partial[static_cast<int64_t>(b) * D + col];
    red[grp][lane] = u;
    __syncthreads();
    if (grp == 0) {
        double v = 0;
#pragma unroll
        for (int g = 0; g < kRmsColGroups; ++g) v += red[g][lane];
        dgamma[col] = static_cast<float>(v);
    }
}

// f(NP constant, T constant) for the row length D
template <typename F>
void dispatch_rms(int D, F &&f) {
    if (!rmsnorm_supported(D)) throw std::invalid_argument("rmsnorm: D must be a multiple of 256 from 256 to 8192");
    const bool wave = D <= kRmsWaveMaxD;
    const int per_pass = wave ? 512 : 2048;
    switch ((wave ? 0 : 4) + (D + per_pass - 1) / per_pass) {
    case 1: f(std::integral_constant<int, 1>(), std::integral_constant<int, 64>()); break;
    case 2: f(std::integral_constant<int, 2>(), std::integral_constant<int, 64>()); break;
    case 3: f(std::integral_constant<int, 3>(), std::integral_constant<int, 64>()); break;
    case 4: f(std::integral_constant<int, 4>(), std::integral_constant<int, 64>()); break;
    case 6: f(std::integral_constant<int, 2>(), std::integral_constant<int, 256>()); break;
    case 7: f(std::integral_constant<int, 3>(), std::integral_constant<int, 256>()); break;
    default: f(std::integral_constant<int, 4>(), std::integral_constant<int, 256>()); break;
    }
}

}  // namespace

bool rmsnorm_supported(int D) { return D >= 256 && D <= kRmsMaxD && D % 256 == 0; }

// Workgroups of the backward = rows of its [blocks][D] partials.  4 rows per team: fewer rows -> more partials for
// the column sums, more rows -> fewer waves in flight (layernorm.hip measured 2 / 4 / 8 within noise of each other)
int rmsnorm_bwd_blocks(int64_t rows, int D) {
    const bool wave = D <= kRmsWaveMaxD;
    const int64_t per_block = wave ? 16 : 4, cap = wave ? 2048 : 1024;
    int64_t b = (rows + per_block - 1) / per_block;
    if (b > cap) b = cap;
    return static_cast<int>(b < 1 ? 1 : b);
}

void launch_rmsnorm_forward(const uint16_t *x, const uint16_t *r, const float *gamma, uint16_t *y, uint16_t *s,
                            float *rstd, int64_t rows, int D, float eps, hipStream_t st) {
    if (rows <= 0) return;
    dispatch_rms(D, [&](auto np, auto tc) {
        constexpr int NP = decltype(np)::value, T = decltype(tc)::value;
        constexpr int TEAMS = kBlock / T;
        int64_t blocks = (rows + TEAMS - 1) / TEAMS;
        const int64_t cap = T == 64 ? 8192 : 2048;
        if (blocks > cap) blocks = cap;
        rms_fwd_kernel<NP, T><<<static_cast<int>(blocks), kBlock, 0, st>>>(
            reinterpret_cast<const uint4 *>(x), reinterpret_cast<const uint4 *>(r),
            reinterpret_cast<const float4 *>(gamma), reinterpret_cast<uint4 *>(y), reinterpret_cast<uint4 *>(s), rstd,
            rows, D, eps);
    });
}

void launch_rmsnorm_backward(const uint16_t *dy, const uint16_t *ds_in, const uint16_t *s, const float *gamma,
                             const float *rstd, uint16_t *ds, float *partial, float *dgamma, int64_t rows, int D,
                             hipStream_t st) {
    if (rows <= 0) return;
    const int blocks = rmsnorm_bwd_blocks(rows, D);
    dispatch_rms(D, [&](auto np, auto tc) {
        constexpr int NP = decltype(np)::value, T = decltype(tc)::value;
        rms_bwd_kernel<NP, T><<<blocks, kBlock, 0, st>>>(
            reinterpret_cast<const uint4 *>(dy), reinterpret_cast<const uint4 *>(ds_in),
            reinterpret_cast<const uint4 *>(s), reinterpret_cast<const float4 *>(gamma), rstd,
            reinterpret_cast<uint4 *>(ds), partial, rows, D);
    });
    rms_colsum_kernel<<<D / 64, 64 * kRmsColGroups, 0, st>>>(partial, blocks, D, dgamma);
}

}  // namespace kfk
