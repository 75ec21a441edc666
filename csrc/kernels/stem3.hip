// Small image-stem convolution on CDNA4 matrix cores, for gfx950: a KH x KW (<= 4 x 4) window over
// a 3-channel image, 32 or 64 output channels (a compile-time count CO), any stride / zero padding:
//   CO = 32  Inception-v3's Conv2d_1a (3x3, stride 2, no padding), with the following BN's statistics in
//            the epilogue (MIOpen before: fwd 0.10 + weight gradient 0.23 ms per 256-image step,
//            profiles/r4z_inception_v3_summary.md, plus the f32 -> bf16 image cast and the BN's statistics pass);
//   CO = 64  VGG-16's first layer (3x3, stride 1, padding 1, 224 x 224), with bias + ReLU in the epilogue
//            (MIOpen before: igemm fwd 0.60 + wrw 0.42 + the cast 0.34 ms, profiles/r6x_vgg16_summary.md,
//            plus a separate bias + ReLU pass over the 1.64 GB output).
//
// Layout: the image is read as it is (f32 or bf16 NHWC, 3 channels: no cast / pad pass); the im2col
// K index is k = kh*16 + kw*4 + c (kw padded to 4, c to 4: zero weights), so one lane's 8-element MFMA
// fragment is 2 neighbouring pixels of one window row (3 channels each, converted to bf16 on load).
// K <= 64 = two K-steps of v_mfma_f32_16x16x32_bf16.
//
// Forward: a wave computes 64 output pixels x CO channels per trip (4 x CO/16 MFMA tiles, 2 K-steps) with
// the weights held in registers for the whole kernel; the product is computed transposed (weights as
// the MFMA A operand), and the weight rows are permuted so that each lane ends with runs of 8 CONSECUTIVE
// channels of one pixel (rows 4q+t of the 16-channel blocks 2u and 2u+1 are channels 32u+8q+t and
// 32u+8q+4+t) -- one 16-byte bf16 store per run, 64 bytes of a pixel from 4 lanes.  Epilogues (template
// flags, so the plain Cout-32 kernel computes what it always did): EPI adds an f32 bias to the f32
// accumulator, then an optional ReLU (NaN kept), before the ONE rounding to bf16; STATS reduces the
// following BN's per-channel sum / sum of squares of the stored bf16 values with lane shuffles and LDS and
// adds them to the BN's f64 slotted workspace (as conv.hip) once per workgroup.
// Weight gradient: per trip a workgroup stages 256 pixels (64 per wave) of dy and of the im2col rows
// TRANSPOSED into LDS (feature-major, 16-byte pixel runs: the MFMA's K dimension is the pixels), so
// the fragments are ds_read_b128 row reads; each wave accumulates its CO x 64 tile over the trips,
// the workgroup folds its 4 waves and writes one f32 partial; stem3_wgrad_reduce_kernel sums the
// partials in a fixed order (deterministic) and unpacks [co][kh][kw][c].
// LDS of the weight gradient: the per-wave images are 4 x (CO + 64) x 144 B = 55.3 KB at CO 32 and 73.7 KB
// at CO 64, past what a static __shared__ array may hold, so the kernel takes DYNAMIC LDS (16-byte aligned
// base, no static beside it) with the function attribute raised; two workgroups (147.4 KB of the CU's
// 160 KB) stay resident per CU.  Chosen over one shared im2col image per workgroup / splitting Cout over
// the waves because it keeps the waves independent between the two barriers of a trip and leaves the
// Cout-32 kernel as it was.
#include "common.hpp"
#include "kernels.hpp"
#include "mfma_util.hpp"

#include <stdexcept>

namespace kfk {

namespace {

constexpr int kKp = 64;       // padded K: 4 kh x 4 kw x 4 c
constexpr int kRowS = 144;    // LDS bytes per transposed row (64 pixels x 2 B + 16 pad)

struct S3Geo {
    int N, H, W, OH, OW, M, KH, KW, stride, ph, pw;
};

__device__ __forceinline__ float ldf(const float *p) { return *p; }
__device__ __forceinline__ float ldf(const uint16_t *p) { return __uint_as_float(static_cast<uint32_t>(*p) << 16); }

// One K-chunk of the im2col row of output pixel p, unconverted: window row ih, columns iw0, iw0+1, the 3
// channels of each; out-of-image pixels and chunks past the window are zero
template <class T>
__device__ __forceinline__ void im2col_raw(const T *__restrict__ x, const S3Geo &g, int n, int ih, int iw0, bool valid,
                                           float (&v)[6]) {
#pragma unroll
    for (int c = 0; c < 6; ++c) v[c] = 0.f;
    if (valid && static_cast<unsigned>(ih) < static_cast<unsigned>(g.H)) {
        const T *row = x + (static_cast<int64_t>(n) * g.H + ih) * g.W * 3;
        if (static_cast<unsigned>(iw0) < static_cast<unsigned>(g.W)) {
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = ldf(row + iw0 * 3 + c);
        }
        if (static_cast<unsigned>(iw0 + 1) < static_cast<unsigned>(g.W)) {
#pragma unroll
            for (int c = 0; c < 3; ++c) v[3 + c] = ldf(row + (iw0 + 1) * 3 + c);
        }
    }
}

// the 8 bf16 of a chunk (a zero 4th channel per pixel)
__device__ __forceinline__ uint4 pack_chunk(const float (&v)[6]) {
    return make_uint4(pack_bf16x2_hw(v[0], v[1]), pack_bf16x2_hw(v[2], 0.f), pack_bf16x2_hw(v[3], v[4]),
                      pack_bf16x2_hw(v[5], 0.f));
}

template <class T>
__device__ __forceinline__ uint4 im2col_chunk(const T *__restrict__ x, const S3Geo &g, int n, int ih, int iw0,
                                              bool valid) {
    float v[6];
    im2col_raw(x, g, n, ih, iw0, valid, v);
    return pack_chunk(v);
}

// MFMA row rho (0..CO-1 over the CO/16 16-row blocks) -> output channel: lane rows 4q+t of block j hold
// channel 32(j/2) + 8q + 4(j%2) + t, so a lane's results of blocks 2u, 2u+1 are 8 consecutive channels
__device__ __forceinline__ int perm_ch(int rho) {
    return (rho >> 5) * 32 + ((rho & 15) >> 2) * 8 + ((rho >> 4) & 1) * 4 + (rho & 3);
}

// EPI: y = [relu](acc + bias) before the rounding (bias may be null: ReLU alone); STATS: the BN sums
template <class T, int CO, bool EPI, bool STATS>
__global__ __launch_bounds__(256) void stem3_fwd_kernel(const T *__restrict__ x, const uint4 *__restrict__ wp,
                                                        uint4 *__restrict__ y, double *__restrict__ stats,
                                                        const float *__restrict__ bias, int relu, S3Geo g) {
    constexpr int JB = CO / 16;  // 16-channel MFMA row blocks
    __shared__ float red[STATS ? 4 : 1][2][CO];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = lane >> 4, r = lane & 15;
    // weights as the MFMA A operand: rows = output channels, K chunk q of K-step s
    bf16x8 wa[JB][2];
#pragma unroll
    for (int j = 0; j < JB; ++j)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const uint4 v = wp[(perm_ch(j * 16 + r) * kKp + s * 32 + q * 8) / 8];
            __builtin_memcpy(&wa[j][s], &v, 16);
        }
    // this lane's result rows 4q+t of block j are channels perm_ch(j*16 + 4q + t): their biases
    float bv[EPI ? JB : 1][4];
    if constexpr (EPI) {
#pragma unroll
        for (int j = 0; j < JB; ++j)
#pragma unroll
            for (int t = 0; t < 4; ++t) bv[j][t] = bias != nullptr ? bias[perm_ch(j * 16 + 4 * q + t)] : 0.f;
    }
    // this lane's K chunks: (s, q) -> window row kh, first column kw0
    int ckh[2], ckw[2];
    bool cval[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int k0 = s * 32 + q * 8;
        ckh[s] = k0 >> 4;
        ckw[s] = (k0 & 15) >> 2;
        cval[s] = ckh[s] < g.KH && ckw[s] < g.KW;
    }
    float s1[JB][4], s2[JB][4];
#pragma unroll
    for (int j = 0; j < JB; ++j)
#pragma unroll
        for (int t = 0; t < 4; ++t) s1[j][t] = s2[j][t] = 0.f;
    const int ntiles = (g.M + 63) / 64;
    for (int tile = blockIdx.x * 4 + wave; tile < ntiles; tile += gridDim.x * 4) {
        f32x4 acc[JB][4];
#pragma unroll
        for (int j = 0; j < JB; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[j][i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int p = tile * 64 + i * 16 + r;
            int n = 0, ih0 = 0, iw0 = 0;
            const bool pin = p < g.M;
            if (pin) {
                const int ow = p % g.OW, t = p / g.OW, oh = t % g.OH;
                n = t / g.OH;
                ih0 = oh * g.stride - g.ph;
                iw0 = ow * g.stride - g.pw;
            }
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const uint4 v = im2col_chunk(x, g, n, ih0 + ckh[s], iw0 + ckw[s], pin && cval[s]);
                bf16x8 b;
                __builtin_memcpy(&b, &v, 16);
#pragma unroll
                for (int j = 0; j < JB; ++j) acc[j][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa[j][s], b, acc[j][i], 0, 0, 0);
            }
        }
        // lane holds channels 32u + 8q + 4(j%2) + (0..3) (j = 2u, 2u+1) of pixel i*16 + r: one 16-byte store
        // of 8 channels per u
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int p = tile * 64 + i * 16 + r;
            if (p >= g.M) continue;
            uint32_t w[2 * JB];
#pragma unroll
            for (int j = 0; j < JB; ++j) {
                float v[4] = {acc[j][i][0], acc[j][i][1], acc[j][i][2], acc[j][i][3]};
                if constexpr (EPI) {
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        v[t] += bv[j][t];
                        if (relu && v[t] <= 0.f) v[t] = 0.f;  // keeps NaN, as torch.relu
                    }
                }
                w[2 * j] = pack_bf16x2_hw(v[0], v[1]);
                w[2 * j + 1] = pack_bf16x2_hw(v[2], v[3]);
            }
#pragma unroll
            for (int u = 0; u < JB / 2; ++u)
                y[static_cast<int64_t>(p) * (CO / 8) + u * 4 + q] = make_uint4(w[4 * u], w[4 * u + 1], w[4 * u + 2], w[4 * u + 3]);
            if constexpr (STATS) {
#pragma unroll
                for (int j = 0; j < JB; ++j) {
                    const float v[4] = {__uint_as_float(w[2 * j] << 16), __uint_as_float(w[2 * j] & 0xffff0000u),
                                        __uint_as_float(w[2 * j + 1] << 16), __uint_as_float(w[2 * j + 1] & 0xffff0000u)};
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        s1[j][t] += v[t];
                        s2[j][t] += v[t] * v[t];
                    }
                }
            }
        }
    }
    if constexpr (STATS) {
        // fold the 16 pixel lanes of each channel quad, then the 4 waves, then one f64 add per channel
#pragma unroll
        for (int j = 0; j < JB; ++j)
#pragma unroll
            for (int t = 0; t < 4; ++t) {
#pragma unroll
                for (int o = 1; o < 16; o <<= 1) {
                    s1[j][t] += __shfl_xor(s1[j][t], o, 64);
                    s2[j][t] += __shfl_xor(s2[j][t], o, 64);
                }
            }
        if (r == 0) {
#pragma unroll
            for (int j = 0; j < JB; ++j)
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    red[wave][0][perm_ch(j * 16 + 4 * q + t)] = s1[j][t];
                    red[wave][1][perm_ch(j * 16 + 4 * q + t)] = s2[j][t];
                }
        }
        __syncthreads();
        if (threadIdx.x < 2 * CO) {
            const int which = threadIdx.x / CO, c = threadIdx.x % CO;
            double a = 0.0;
            for (int w = 0; w < 4; ++w) a += red[w][which][c];
            atomicAdd(stats + (blockIdx.x % kStatSlots) * 2 * CO + which * CO + c, a);
        }
    }
}

constexpr int wgrad_lds_bytes(int co) { return 4 * (co + kKp) * kRowS; }  // >= the 4 x co x 64 f32 fold image

// dy [M, CO] bf16, x [N, H, W, 3] f32 / bf16 -> part[block][CO][64] f32 (one per workgroup);
// dynamic LDS: wgrad_lds_bytes(CO)
template <class T, int CO>
__global__ __launch_bounds__(256) void stem3_wgrad_kernel(const uint4 *__restrict__ dy, const T *__restrict__ x,
                                                          float *__restrict__ part, S3Geo g) {
    constexpr int JB = CO / 16;  // 16-channel MFMA row blocks
    constexpr int DU = CO / 8;   // 16-byte pieces of a dy row
    static_assert(4 * CO * kKp * 4 <= wgrad_lds_bytes(CO), "the wave fold reuses the images");
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = lane >> 4, r = lane & 15;
    uint8_t *dyT = lds + wave * (CO + kKp) * kRowS;  // [CO co][64 px]
    uint8_t *colT = dyT + CO * kRowS;                 // [64 k][64 px]
    const int nkb = (g.KH * 16 + 15) / 16;            // 16-wide k blocks that carry the window
    f32x4 acc[JB][4];
#pragma unroll
    for (int j = 0; j < JB; ++j)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[j][b] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int nblk = (g.M + 255) / 256;
    // next trip's dy row and raw im2col chunks, loaded into registers while this trip's MFMAs run
    uint4 d[DU];
    float xv[4][2][6];
    auto fetch = [&](int blk) {
        const int p = blk * 256 + wave * 64 + lane;
        const bool pin = blk < nblk && p < g.M;
#pragma unroll
        for (int u = 0; u < DU; ++u) d[u] = pin ? dy[static_cast<int64_t>(p) * DU + u] : make_uint4(0u, 0u, 0u, 0u);
        int n = 0, ih0 = 0, iw0 = 0;
        if (pin) {
            const int ow = p % g.OW, t = p / g.OW, oh = t % g.OH;
            n = t / g.OH;
            ih0 = oh * g.stride - g.ph;
            iw0 = ow * g.stride - g.pw;
        }
#pragma unroll
        for (int kh = 0; kh < 4; ++kh)
#pragma unroll
            for (int h = 0; h < 2; ++h) im2col_raw(x, g, n, ih0 + kh, iw0 + 2 * h, pin && kh < g.KH && 2 * h < g.KW, xv[kh][h]);
    };
    fetch(blockIdx.x);
    for (int blk = blockIdx.x; blk < nblk; blk += gridDim.x) {  // uniform trip count per workgroup
        // dy row of this lane's pixel -> column `lane` of dyT
#pragma unroll
        for (int u = 0; u < DU; ++u) {
            const uint32_t w4[4] = {d[u].x, d[u].y, d[u].z, d[u].w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                *reinterpret_cast<uint16_t *>(dyT + (u * 8 + 2 * e) * kRowS + lane * 2) = static_cast<uint16_t>(w4[e]);
                *reinterpret_cast<uint16_t *>(dyT + (u * 8 + 2 * e + 1) * kRowS + lane * 2) =
                    static_cast<uint16_t>(w4[e] >> 16);
            }
        }
        // im2col row of this lane's pixel -> column `lane` of colT (rows k = kh*16 + kw*4 + c)
#pragma unroll
        for (int kh = 0; kh < 4; ++kh) {
            if (kh >= g.KH) break;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const uint4 v = pack_chunk(xv[kh][h]);
                const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int k = kh * 16 + h * 8 + 2 * e;
                    *reinterpret_cast<uint16_t *>(colT + k * kRowS + lane * 2) = static_cast<uint16_t>(w4[e]);
                    *reinterpret_cast<uint16_t *>(colT + (k + 1) * kRowS + lane * 2) = static_cast<uint16_t>(w4[e] >> 16);
                }
            }
        }
        fetch(blk + gridDim.x);
        __syncthreads();
        // dW[co][k] += sum over this wave's 64 pixels: two 32-pixel K-steps
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            bf16x8 a[JB];
#pragma unroll
            for (int j = 0; j < JB; ++j) a[j] = *reinterpret_cast<const bf16x8 *>(dyT + (j * 16 + r) * kRowS + (s * 32 + q * 8) * 2);
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                if (b >= nkb) break;
                const bf16x8 c = *reinterpret_cast<const bf16x8 *>(colT + (b * 16 + r) * kRowS + (s * 32 + q * 8) * 2);
#pragma unroll
                for (int j = 0; j < JB; ++j) acc[j][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[j], c, acc[j][b], 0, 0, 0);
            }
        }
        __syncthreads();  // the next trip overwrites the images
    }
    // fold the 4 waves through LDS (the images are dead): lane holds C[co = j*16 + 4q + t][k = b*16 + r]
    float *fr = reinterpret_cast<float *>(lds);  // [4 waves][CO][64]
#pragma unroll
    for (int j = 0; j < JB; ++j)
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int t = 0; t < 4; ++t) fr[(wave * CO + j * 16 + q * 4 + t) * kKp + b * 16 + r] = acc[j][b][t];
    __syncthreads();
    float *dst = part + static_cast<int64_t>(blockIdx.x) * CO * kKp;
    for (int e = threadIdx.x; e < CO * kKp; e += 256)
        dst[e] = (fr[e] + fr[CO * kKp + e]) + (fr[2 * CO * kKp + e] + fr[3 * CO * kKp + e]);
}

// Level 1 of the partial sum: mid[rg][e] = sum of partial rows [rg*16, rg*16+16) (e over the tile = Cout x 64
// padded elements, a multiple of 256); coalesced across threads, 16 loads per thread
__global__ __launch_bounds__(256) void stem3_wgrad_fold_kernel(const float *__restrict__ part, int blocks,
                                                               float *__restrict__ mid, int tile) {
    const int e = blockIdx.x * 256 + threadIdx.x, rg = blockIdx.y;
    float a = 0.f;
    const int b1 = min(blocks, rg * 16 + 16);
    for (int b = rg * 16; b < b1; ++b) a += part[static_cast<int64_t>(b) * tile + e];
    mid[rg * tile + e] = a;
}

// dw[co][kh][kw][c] (PyTorch [Cout, Cin, KH, KW] memory in channels_last = [co][kh][kw][c]) = the sum of
// the level-1 rows, in order (deterministic); f32 or bf16 output
__global__ __launch_bounds__(256) void stem3_wgrad_reduce_kernel(const float *__restrict__ mid, int rows,
                                                                 void *__restrict__ dw, int out_f32, int Cout, int KH,
                                                                 int KW) {
    const int e = blockIdx.x * 256 + threadIdx.x;  // [co][kh][kw][c] element
    const int nout = Cout * KH * KW * 3;
    if (e >= nout) return;
    const int c = e % 3, t = e / 3, kw = t % KW, t2 = t / KW, kh = t2 % KH, co = t2 / KH;
    const int k = kh * 16 + kw * 4 + c;
    float a = 0.f;
    for (int rg = 0; rg < rows; ++rg) a += mid[(static_cast<int64_t>(rg) * Cout + co) * kKp + k];
    if (out_f32) static_cast<float *>(dw)[e] = a;
    else static_cast<uint16_t *>(dw)[e] = f32_to_bf16(a);
}

// w [co][kh][kw][c] bf16 (channels_last [Cout, 3, KH, KW]) -> wp [Cout][64] (k = kh*16 + kw*4 + c, zeros)
__global__ void stem3_pack_weight_kernel(const uint16_t *__restrict__ w, uint16_t *__restrict__ wp, int Cout, int KH,
                                         int KW) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= Cout * kKp) return;
    const int co = e / kKp, k = e % kKp, kh = k >> 4, kw = (k >> 2) & 3, c = k & 3;
    uint16_t v = 0;
    if (kh < KH && kw < KW && c < 3) v = w[((co * KH + kh) * KW + kw) * 3 + c];
    wp[e] = v;
}

void check_cout(int Cout) {
    if (Cout != 32 && Cout != 64) throw std::invalid_argument("stem3: Cout must be 32 or 64");
}

S3Geo make_geo(int N, int H, int W, int KH, int KW, int stride, int ph, int pw) {
    if (KH < 1 || KH > 4 || KW < 1 || KW > 4 || stride < 1 || ph < 0 || pw < 0 || ph >= KH || pw >= KW)
        throw std::invalid_argument("stem3: window <= 4x4, stride >= 1, 0 <= padding < window");
    S3Geo g;
    g.N = N, g.H = H, g.W = W, g.KH = KH, g.KW = KW, g.stride = stride, g.ph = ph, g.pw = pw;
    g.OH = (H + 2 * ph - KH) / stride + 1;
    g.OW = (W + 2 * pw - KW) / stride + 1;
    if (g.OH < 1 || g.OW < 1) throw std::invalid_argument("stem3: empty output");
    const int64_t m = static_cast<int64_t>(N) * g.OH * g.OW;
    if (m >= (int64_t(1) << 31) || static_cast<int64_t>(N) * H * W >= (int64_t(1) << 31))
        throw std::invalid_argument("stem3: too many pixels");
    g.M = static_cast<int>(m);
    return g;
}

}  // namespace

int stem3_out(int h, int k, int stride, int pad) { return (h + 2 * pad - k) / stride + 1; }

void launch_stem3_pack_weight(const uint16_t *w, uint16_t *wp, int Cout, int KH, int KW, hipStream_t s) {
    check_cout(Cout);
    stem3_pack_weight_kernel<<<(Cout * kKp + 255) / 256, 256, 0, s>>>(w, wp, Cout, KH, KW);
}

namespace {

template <class T, int CO>
void fwd_launch(const T *x, const uint4 *w4, uint4 *y4, double *stats, const float *bias, bool relu, const S3Geo &g,
                int grid, hipStream_t s) {
    const bool epi = bias != nullptr || relu;
    const int r = relu ? 1 : 0;
    if (epi && stats) stem3_fwd_kernel<T, CO, true, true><<<grid, 256, 0, s>>>(x, w4, y4, stats, bias, r, g);
    else if (epi) stem3_fwd_kernel<T, CO, true, false><<<grid, 256, 0, s>>>(x, w4, y4, stats, bias, r, g);
    else if (stats) stem3_fwd_kernel<T, CO, false, true><<<grid, 256, 0, s>>>(x, w4, y4, stats, bias, r, g);
    else stem3_fwd_kernel<T, CO, false, false><<<grid, 256, 0, s>>>(x, w4, y4, stats, bias, r, g);
}

template <class T, int CO>
void wgrad_launch(const uint4 *d4, const T *x, float *part, const S3Geo &g, int blocks, hipStream_t s) {
    static const bool attr = [] {  // past the 64 KB default at CO 64
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(stem3_wgrad_kernel<T, CO>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, wgrad_lds_bytes(CO));
        return true;
    }();
    (void)attr;
    stem3_wgrad_kernel<T, CO><<<blocks, 256, wgrad_lds_bytes(CO), s>>>(d4, x, part, g);
}

}  // namespace

void launch_stem3_forward(const void *x, bool x_f32, const uint16_t *wp, uint16_t *y, double *stats, const float *bias,
                          bool relu, int Cout, int N, int H, int W, int KH, int KW, int stride, int ph, int pw,
                          hipStream_t s) {
    check_cout(Cout);
    const S3Geo g = make_geo(N, H, W, KH, KW, stride, ph, pw);
    const int tiles = (g.M + 63) / 64;
    int grid = (tiles + 3) / 4;
    if (grid > 2048) grid = 2048;
    const uint4 *w4 = reinterpret_cast<const uint4 *>(wp);
    uint4 *y4 = reinterpret_cast<uint4 *>(y);
    if (x_f32 && Cout == 32) fwd_launch<float, 32>(static_cast<const float *>(x), w4, y4, stats, bias, relu, g, grid, s);
    else if (x_f32) fwd_launch<float, 64>(static_cast<const float *>(x), w4, y4, stats, bias, relu, g, grid, s);
    else if (Cout == 32) fwd_launch<uint16_t, 32>(static_cast<const uint16_t *>(x), w4, y4, stats, bias, relu, g, grid, s);
    else fwd_launch<uint16_t, 64>(static_cast<const uint16_t *>(x), w4, y4, stats, bias, relu, g, grid, s);
}

int stem3_wgrad_blocks(int Cout, int N, int H, int W, int KH, int KW, int stride, int ph, int pw) {
    check_cout(Cout);
    const S3Geo g = make_geo(N, H, W, KH, KW, stride, ph, pw);
    const int nblk = (g.M + 255) / 256;
    // two resident per CU (55 / 74 KB LDS each at Cout 32 / 64); one partial row each, then a 16-row fold
    return nblk < 512 ? nblk : 512;
}

int64_t stem3_wgrad_workspace(int Cout, int N, int H, int W, int KH, int KW, int stride, int ph, int pw) {
    const int blocks = stem3_wgrad_blocks(Cout, N, H, W, KH, KW, stride, ph, pw);
    return static_cast<int64_t>(blocks + (blocks + 15) / 16) * Cout * kKp;
}

void launch_stem3_wgrad(const uint16_t *dy, const void *x, bool x_f32, void *dw, bool out_f32, float *part, int Cout,
                        int N, int H, int W, int KH, int KW, int stride, int ph, int pw, hipStream_t s) {
    const S3Geo g = make_geo(N, H, W, KH, KW, stride, ph, pw);
    const int blocks = stem3_wgrad_blocks(Cout, N, H, W, KH, KW, stride, ph, pw);
    const uint4 *d4 = reinterpret_cast<const uint4 *>(dy);
    if (x_f32 && Cout == 32) wgrad_launch<float, 32>(d4, static_cast<const float *>(x), part, g, blocks, s);
    else if (x_f32) wgrad_launch<float, 64>(d4, static_cast<const float *>(x), part, g, blocks, s);
    else if (Cout == 32) wgrad_launch<uint16_t, 32>(d4, static_cast<const uint16_t *>(x), part, g, blocks, s);
    else wgrad_launch<uint16_t, 64>(d4, static_cast<const uint16_t *>(x), part, g, blocks, s);
    const int rows = (blocks + 15) / 16;
    const int tile = Cout * kKp;
    float *mid = part + static_cast<int64_t>(blocks) * tile;
    stem3_wgrad_fold_kernel<<<dim3(tile / 256, rows), 256, 0, s>>>(part, blocks, mid, tile);
    const int nout = Cout * KH * KW * 3;
    stem3_wgrad_reduce_kernel<<<(nout + 255) / 256, 256, 0, s>>>(mid, rows, dw, out_f32 ? 1 : 0, Cout, KH, KW);
}

}  // namespace kfk
