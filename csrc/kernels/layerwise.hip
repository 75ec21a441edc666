// Layer-wise trust-ratio optimizers on the flat parameter space: LARS and LAMB.
//
// Slots of a FlatParamSpace start at multiples of 64 elements and slot k spans [off_k, off_{k+1})
// with its alignment padding, so every access is a float4 and there are no scalar tails.  The
// padding holds zeros in w, g and every state buffer and both updates map zeros to zeros, so it is
// summed into the norms and updated like everything else.
//
// A step is three launches with fixed shapes (a hipGraph replays them; the host never waits):
//   1. partial: one workgroup per chunk (<= kLayerChunk elements of ONE slot, grid-stride over the
//      chunk table) writes the chunk's sum(w^2) and sum(x^2), x = g (LARS) or u (LAMB, which also
//      updates m and v here).  Wave shuffle + LDS, one f32 pair per chunk.
//   2. coef: one wave per slot folds the slot's chunk partials in f64, lane l the l-th run of
//      consecutive chunks and lane 0 the 64 lane sums in order; writes ||w||, ||x|| and the ratio.
//   3. apply: same chunking; reads the slot's ratio and weight decay and updates w (LARS: and m;
//      LAMB recomputes u from the m, v of stage 1), optionally the bf16 shadow of w.
// HBM traffic per parameter without the shadow: LARS 2 + 3 reads + 2 writes = 28 B, LAMB
// 4 + 3 reads + 2 + 1 writes = 40 B.  No float atomics: every sum has a fixed order, so a step is
// bit-reproducible and a slot's update depends on that slot's data alone.
#include "common.hpp"
#include "kernels.hpp"

namespace kfk {

namespace {

constexpr int kU = kLayerChunk / (kBlock * 4);  // float4 per lane and operand in one chunk
static_assert(kLayerChunk % (kBlock * 4) == 0 && kLayerChunk % 64 == 0, "a chunk is whole float4 rows of the block");
static_assert(kLayerGridCap == kMaxGrid, "the chunk loop is capped like every flat kernel");

// chunks[c] = {first element, slot, length}.  The tables come from the caller: an entry that does
// not describe float4s of one slot inside the buffer is given no work (len4 = 0) instead of trust.
struct Chunk {
    int64_t b4;  // first float4
    int len4, slot;
};
__device__ __forceinline__ Chunk load_chunk(const int64_t *__restrict__ chunks, int c, int64_t n, int nseg) {
    const int64_t start = chunks[3 * c], slot = chunks[3 * c + 1], len = chunks[3 * c + 2];
    const bool ok = start >= 0 && len > 0 && len <= kLayerChunk && start <= n - len && ((start | len) & 3) == 0 &&
                    slot >= 0 && slot < nseg;
    Chunk k;
    k.b4 = ok ? start / 4 : 0;
    k.len4 = ok ? static_cast<int>(len / 4) : 0;
    k.slot = ok ? static_cast<int>(slot) : 0;
    return k;
}

__device__ __forceinline__ float sq4(const float4 &a) { return a.x * a.x + a.y * a.y + a.z * a.z + a.w * a.w; }

__device__ __forceinline__ ushort4 bf16x4(const float4 &a) {
    return make_ushort4(f32_to_bf16(a.x), f32_to_bf16(a.y), f32_to_bf16(a.z), f32_to_bf16(a.w));
}

// thread 0 stores the chunk's pair; the barrier frees the LDS words for the block's next chunk
__device__ __forceinline__ void store_partial(float (&acc)[2], float (*lds)[kBlock / kWave], float *partials, int c) {
    block_sum<2>(acc, lds);
    if (threadIdx.x == 0) {
        partials[2 * c] = acc[0];
        partials[2 * c + 1] = acc[1];
    }
    __syncthreads();
}

// ---------------------------------------------------------------- LARS

__global__ __launch_bounds__(kBlock) void lars_partial(const float4 *__restrict__ w, const float4 *__restrict__ g,
                                                       int64_t n, const int64_t *__restrict__ chunks, int nchunks,
                                                       int nseg, float gscale, float *__restrict__ partials) {
    __shared__ float lds[2][kBlock / kWave];
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const Chunk ch = load_chunk(chunks, c, n, nseg);
        float4 wv[kU], gv[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const int j = threadIdx.x + u * kBlock;
            if (j < ch.len4) {
                wv[u] = w[ch.b4 + j];
                gv[u] = g[ch.b4 + j];
            }
        }
        float acc[2] = {0.f, 0.f};
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            if (static_cast<int>(threadIdx.x) + u * kBlock >= ch.len4) break;
            float4 x = gv[u];
            x.x *= gscale, x.y *= gscale, x.z *= gscale, x.w *= gscale;
            acc[0] += sq4(wv[u]);
            acc[1] += sq4(x);
        }
        store_partial(acc, lds, partials, c);
    }
}

template <bool NESTEROV, bool MOM>
__global__ __launch_bounds__(kBlock) void lars_apply(float4 *__restrict__ w, const float4 *__restrict__ g,
                                                     float4 *__restrict__ m, ushort4 *__restrict__ shadow, int64_t n,
                                                     const int64_t *__restrict__ chunks, int nchunks, int nseg,
                                                     const float *__restrict__ ratio, const float *__restrict__ wd_tab,
                                                     float lr, const float *lr_dev, float mu, float gscale) {
    if (lr_dev) lr = *lr_dev;
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const Chunk ch = load_chunk(chunks, c, n, nseg);
        const float q = ratio[ch.slot], wd = wd_tab[ch.slot];
        float4 wv[kU], gv[kU], mv[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const int j = threadIdx.x + u * kBlock;
            if (j < ch.len4) {
                wv[u] = w[ch.b4 + j];
                gv[u] = g[ch.b4 + j];
                if (MOM) mv[u] = m[ch.b4 + j];
            }
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const int j = threadIdx.x + u * kBlock;
            if (j >= ch.len4) break;
            float *pw = reinterpret_cast<float *>(&wv[u]);
            const float *pg = reinterpret_cast<const float *>(&gv[u]);
            float *pm = reinterpret_cast<float *>(&mv[u]);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float d = q * (pg[k] * gscale + wd * pw[k]);
                if (MOM) {
                    pm[k] = mu * pm[k] + d;
                    d = NESTEROV ? d + mu * pm[k] : pm[k];
                }
                pw[k] -= lr * d;
            }
            w[ch.b4 + j] = wv[u];
            if (MOM) m[ch.b4 + j] = mv[u];
            if (shadow) shadow[ch.b4 + j] = bf16x4(wv[u]);
        }
    }
}

// ---------------------------------------------------------------- LAMB

// b^t for a whole-numbered t, in f64: 1 - b^t loses everything below b's own rounding in f32
// (1 - 0.999f is already 5e-5 off 0.001), and the update is linear in it where trust is off
__device__ __forceinline__ double ipow(double b, unsigned t) {
    double r = 1.0;
    for (; t; t >>= 1, b *= b)
        if (t & 1u) r *= b;
    return r;
}

struct LambCoef {
    float b1, omb1, b2, omb2;  // beta, 1 - beta
    float rbc1, rbc2s;         // 1 / (1 - b1^t), 1 / sqrt(1 - b2^t)
    float eps;
};
__device__ __forceinline__ LambCoef lamb_coef(double b1, double b2, float eps, const float *step_dev, bool bias) {
    LambCoef k;
    k.b1 = static_cast<float>(b1), k.omb1 = static_cast<float>(1.0 - b1);
    k.b2 = static_cast<float>(b2), k.omb2 = static_cast<float>(1.0 - b2);
    k.rbc1 = k.rbc2s = 1.f;
    k.eps = eps;
    if (bias) {
        const unsigned t = static_cast<unsigned>(*step_dev + 0.5f);
        k.rbc1 = static_cast<float>(1.0 / (1.0 - ipow(b1, t)));
        k.rbc2s = static_cast<float>(1.0 / sqrt(1.0 - ipow(b2, t)));
    }
    return k;
}

// the update direction from the moments of this step: both stages call it on the same values
__device__ __forceinline__ float lamb_u(float m, float v, float w, float wd, const LambCoef &k) {
    return (m * k.rbc1) / (sqrtf(v) * k.rbc2s + k.eps) + wd * w;
}

__global__ __launch_bounds__(kBlock) void lamb_partial(const float4 *__restrict__ w, const float4 *__restrict__ g,
                                                       float4 *__restrict__ m, float4 *__restrict__ v, int64_t n,
                                                       const int64_t *__restrict__ chunks, int nchunks, int nseg,
                                                       const float *__restrict__ wd_tab, double b1, double b2,
                                                       float eps, float gscale, const float *step_dev, bool bias,
                                                       float max_grad_norm, const float *gsq,
                                                       float *__restrict__ partials) {
    __shared__ float lds[2][kBlock / kWave];
    const LambCoef k = lamb_coef(b1, b2, eps, step_dev, bias);
    if (gsq) gscale *= fminf(1.f, max_grad_norm / (fabsf(gscale) * sqrtf(*gsq)));  // x / 0 = inf: no clip
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const Chunk ch = load_chunk(chunks, c, n, nseg);
        const float wd = wd_tab[ch.slot];
        float4 wv[kU], gv[kU], mv[kU], vv[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const int j = threadIdx.x + u * kBlock;
            if (j < ch.len4) {
                wv[u] = w[ch.b4 + j];
                gv[u] = g[ch.b4 + j];
                mv[u] = m[ch.b4 + j];
                vv[u] = v[ch.b4 + j];
            }
        }
        float acc[2] = {0.f, 0.f};
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const int j = threadIdx.x + u * kBlock;
            if (j >= ch.len4) break;
            const float *pw = reinterpret_cast<const float *>(&wv[u]);
            const float *pg = reinterpret_cast<const float *>(&gv[u]);
            float *pm = reinterpret_cast<float *>(&mv[u]);
            float *pv = reinterpret_cast<float *>(&vv[u]);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float gg = pg[e] * gscale;
                pm[e] = k.b1 * pm[e] + k.omb1 * gg;
                pv[e] = k.b2 * pv[e] + k.omb2 * gg * gg;
                const float uu = lamb_u(pm[e], pv[e], pw[e], wd, k);
                acc[0] += pw[e] * pw[e];
                acc[1] += uu * uu;
            }
            m[ch.b4 + j] = mv[u];
            v[ch.b4 + j] = vv[u];
        }
        store_partial(acc, lds, partials, c);
    }
}

__global__ __launch_bounds__(kBlock) void lamb_apply(float4 *__restrict__ w, const float4 *__restrict__ m,
                                                     const float4 *__restrict__ v, ushort4 *__restrict__ shadow,
                                                     int64_t n, const int64_t *__restrict__ chunks, int nchunks,
                                                     int nseg, const float *__restrict__ ratio,
                                                     const float *__restrict__ wd_tab, float lr, const float *lr_dev,
                                                     double b1, double b2, float eps, const float *step_dev,
                                                     bool bias) {
    if (lr_dev) lr = *lr_dev;
    const LambCoef k = lamb_coef(b1, b2, eps, step_dev, bias);
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const Chunk ch = load_chunk(chunks, c, n, nseg);
        const float wd = wd_tab[ch.slot], step = lr * ratio[ch.slot];
        float4 wv[kU], mv[kU], vv[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const int j = threadIdx.x + u * kBlock;
            if (j < ch.len4) {
                wv[u] = w[ch.b4 + j];
                mv[u] = m[ch.b4 + j];
                vv[u] = v[ch.b4 + j];
            }
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const int j = threadIdx.x + u * kBlock;
            if (j >= ch.len4) break;
            float *pw = reinterpret_cast<float *>(&wv[u]);
            const float *pm = reinterpret_cast<const float *>(&mv[u]);
            const float *pv = reinterpret_cast<const float *>(&vv[u]);
#pragma unroll
            for (int e = 0; e < 4; ++e) pw[e] -= step * lamb_u(pm[e], pv[e], pw[e], wd, k);
            w[ch.b4 + j] = wv[u];
            if (shadow) shadow[ch.b4 + j] = bf16x4(wv[u]);
        }
    }
}

// ---------------------------------------------------------------- per-slot norms and ratio

// One wave per slot.  LARS: q = tc * ||w|| / (||g|| + wd * ||w|| + eps); LAMB: r = ||w|| / ||u||;
// 1 where the slot's trust switch is off or a norm is zero.
template <bool LAMB>
__global__ __launch_bounds__(kWave) void layer_coef(const float *__restrict__ partials,
                                                    const int64_t *__restrict__ slot_chunk0, int nchunks,
                                                    const float *__restrict__ wd_tab,
                                                    const float *__restrict__ trust_tab, float tc, float eps,
                                                    float *__restrict__ w_norm, float *__restrict__ x_norm,
                                                    float *__restrict__ ratio) {
    __shared__ double lds[2][kWave];
    const int k = blockIdx.x, lane = threadIdx.x;
    int64_t c0 = slot_chunk0[k], c1 = slot_chunk0[k + 1];
    c0 = c0 < 0 ? 0 : (c0 > nchunks ? nchunks : c0);
    c1 = c1 < c0 ? c0 : (c1 > nchunks ? nchunks : c1);
    const int64_t per = (c1 - c0 + kWave - 1) / kWave;
    int64_t lo = c0 + lane * per, hi = lo + per;
    if (lo > c1) lo = c1;
    if (hi > c1) hi = c1;
    double a = 0.0, b = 0.0;
    for (int64_t c = lo; c < hi; ++c) {
        a += static_cast<double>(partials[2 * c]);
        b += static_cast<double>(partials[2 * c + 1]);
    }
    lds[0][lane] = a;
    lds[1][lane] = b;
    __syncthreads();
    if (lane != 0) return;
    a = b = 0.0;
    for (int l = 0; l < kWave; ++l) {
        a += lds[0][l];
        b += lds[1][l];
    }
    const double wn = sqrt(a), xn = sqrt(b);
    double r = 1.0;
    if (trust_tab[k] != 0.f && wn > 0.0 && xn > 0.0)
        r = LAMB ? wn / xn : static_cast<double>(tc) * wn / (xn + static_cast<double>(wd_tab[k]) * wn + eps);
    w_norm[k] = static_cast<float>(wn);
    x_norm[k] = static_cast<float>(xn);
    ratio[k] = static_cast<float>(r);
}

inline int chunk_grid(int nchunks) { return nchunks < kLayerGridCap ? nchunks : kLayerGridCap; }

}  // namespace

void launch_lars(float *w, const float *g, float *m, uint16_t *shadow, size_t n, const LayerTables &t, float lr,
                 const float *lr_dev, float mu, float tc, float eps, float gscale, bool nesterov, hipStream_t s) {
    if (n == 0 || t.nchunks <= 0 || t.nseg <= 0) return;
    const int grid = chunk_grid(t.nchunks);
    const int64_t n64 = static_cast<int64_t>(n);
    auto w4 = reinterpret_cast<float4 *>(w);
    auto g4 = reinterpret_cast<const float4 *>(g);
    auto m4 = reinterpret_cast<float4 *>(m);
    auto sh4 = reinterpret_cast<ushort4 *>(shadow);
    lars_partial<<<grid, kBlock, 0, s>>>(w4, g4, n64, t.chunks, t.nchunks, t.nseg, gscale, t.partials);
    layer_coef<false><<<t.nseg, kWave, 0, s>>>(t.partials, t.slot_chunk0, t.nchunks, t.wd_tab, t.trust_tab, tc, eps,
                                              t.w_norm, t.x_norm, t.ratio);
#define KFK_LARS(NES, MOM)                                                                                         \
    lars_apply<NES, MOM><<<grid, kBlock, 0, s>>>(w4, g4, m4, sh4, n64, t.chunks, t.nchunks, t.nseg, t.ratio, t.wd_tab, \
                                                 lr, lr_dev, mu, gscale)
    if (mu == 0.f || !m) KFK_LARS(false, false);
    else if (nesterov) KFK_LARS(true, true);
    else KFK_LARS(false, true);
#undef KFK_LARS
}

void launch_lamb(float *w, const float *g, float *m, float *v, uint16_t *shadow, size_t n, const LayerTables &t,
                 float lr, const float *lr_dev, double b1, double b2, float eps, float gscale, const float *step_dev,
                 bool bias_correction, float max_grad_norm, const float *gsq, hipStream_t s) {
    if (n == 0 || t.nchunks <= 0 || t.nseg <= 0) return;
    const int grid = chunk_grid(t.nchunks);
    const int64_t n64 = static_cast<int64_t>(n);
    auto w4 = reinterpret_cast<float4 *>(w);
    auto m4 = reinterpret_cast<float4 *>(m);
    auto v4 = reinterpret_cast<float4 *>(v);
    lamb_partial<<<grid, kBlock, 0, s>>>(w4, reinterpret_cast<const float4 *>(g), m4, v4, n64, t.chunks, t.nchunks,
                                         t.nseg, t.wd_tab, b1, b2, eps, gscale, step_dev, bias_correction,
                                         max_grad_norm, gsq, t.partials);
    layer_coef<true><<<t.nseg, kWave, 0, s>>>(t.partials, t.slot_chunk0, t.nchunks, t.wd_tab, t.trust_tab, 0.f, 0.f,
                                             t.w_norm, t.x_norm, t.ratio);
    lamb_apply<<<grid, kBlock, 0, s>>>(w4, m4, v4, reinterpret_cast<ushort4 *>(shadow), n64, t.chunks, t.nchunks,
                                       t.nseg, t.ratio, t.wd_tab, lr, lr_dev, b1, b2, eps, step_dev, bias_correction);
}

}  // namespace kfk
