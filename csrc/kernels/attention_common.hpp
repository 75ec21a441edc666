// Device helpers shared by the fused attention kernels (attention.hip: whole sequence in LDS,
// attention_long.hip: streamed blocks): the swizzled LDS image addressing, the MFMA operand
// fragments, the dropout hash, the LDS-DMA staging and the kernel argument block.  Private to
// those two files: everything sits in an unnamed namespace.
#pragma once
#include "common.hpp"
#include "kernels.hpp"
#include "mfma_util.hpp"

namespace kfk {

namespace {

constexpr int DH = 64;  // head dim

// byte offset of bf16 (row, col) in an image of ROW-byte rows (128: 64 bf16, or 256), swizzled by hswz
template <int ROW>
__device__ __forceinline__ int off(int row, int col) {
    return row * ROW + (((col >> 4) ^ hswz<ROW>(row)) << 5) + (col & 15) * 2;
}

__device__ __forceinline__ bf16x8 rd128(const uint8_t *p) { return *reinterpret_cast<const bf16x8 *>(p); }

// operand fragment from an image whose ROWS are the MFMA K index: lane 16g+4q+p reads row
// k0 + 8g + q (+4), columns c0 + 4p..4p+3; lane i of the 16-group receives column c0 + i
template <int ROW>
__device__ __forceinline__ bf16x8 tr_frag(const uint8_t *img, int k0, int c0, int lane) {
    const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
    const int r = k0 + 8 * g + q, c = c0 + 4 * p;
    // (not through the pointer-pair tr_frag: forming both addresses before the first read reorders
    // these kernels' LDS reads)
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4 *)(img + off<ROW>(r, c)));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4 *)(img + off<ROW>(r + 4, c)));
    return __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}
// operand fragment from an image whose COLUMNS are the MFMA K index: lane l reads row
// r0 + (l & 15), columns k0 + 8 (l >> 4) .. +7
template <int ROW>
__device__ __forceinline__ bf16x8 row_frag(const uint8_t *img, int r0, int k0, int lane) {
    return rd128(img + off<ROW>(r0 + (lane & 15), k0 + 8 * (lane >> 4)));
}

__device__ __forceinline__ f32x4 mfma(const bf16x8 &a, const bf16x8 &b, const f32x4 &c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// Dropout keep test: a counter hash of (seed, sequence*heads + head, query, key).  The same
// function is reproduced in torch by the tests (kungfu_amd/ops/attention.py: dropout_keep).
__device__ __forceinline__ bool keep_elem(uint32_t seed, uint32_t bh, uint32_t q, uint32_t k, uint32_t thresh) {
    uint32_t x = ((q << 16) | k) ^ seed;
    x *= 0x9E3779B1u;
    x ^= bh * 0x85EBCA77u + (x >> 15);
    x ^= x >> 16;
    x *= 0x7FEB352Du;
    x ^= x >> 15;
    x *= 0x846CA68Bu;
    x ^= x >> 16;
    return x >= thresh;
}

// Stage NIMG images of S rows x 64 bf16 (128-byte rows) with 16-byte global_load_lds: image t
// row r comes from src[t] + r * stride[t]; the NW waves split the 1 KB (8-row) pieces.
template <int S, int NIMG, int NW = 4>
__device__ __forceinline__ void stage_images(uint8_t *lds, const uint16_t *const (&src)[NIMG],
                                             const int (&stride)[NIMG], int wave, int lane) {
    constexpr int PIECES = S / 8;
    static_assert((NIMG * PIECES) % NW == 0, "pieces per wave");
    const int pch = lane & 7;
#pragma unroll
    for (int u = 0; u < NIMG * PIECES / NW; ++u) {
        const int gp = wave + NW * u;
        const int t = gp / PIECES, pc = gp - t * PIECES;
        const int r = pc * 8 + (lane >> 3);
        const int col = ((((pch >> 1) ^ hswz<128>(r)) << 1) | (pch & 1)) * 8;
        const uint16_t *s = src[t] + static_cast<int64_t>(r) * stride[t] + col;
        __builtin_amdgcn_global_load_lds(s, lds + t * S * 128 + pc * 1024, 16, 0, 0);
    }
}

struct AttnArgs {
    const uint16_t *qkv;  // [B, S, 3, H, 64]
    uint16_t *out;        // [B, S, H, 64]
    float *lse;           // [B, H, S]
    const uint16_t *dout; // [B, S, H, 64]
    uint16_t *dqkv;       // [B, S, 3, H, 64]
    int H;
    float scale;
    uint32_t seed, thresh;
    float inv_keep;
    const uint32_t *seed_base;  // device word mixed into the seed (graph replays advance it), or null
};

// the per-call seed mixed with the device seed base (dropout_seed_base)
__device__ __forceinline__ uint32_t call_seed(const AttnArgs &a) {
    return a.seed_base ? a.seed ^ (a.seed_base[0] * 0x85EBCA6Bu) : a.seed;
}

inline AttnArgs make_args(const uint16_t *qkv, uint16_t *out, float *lse, const uint16_t *dout, uint16_t *dqkv, int H,
                          float scale, uint32_t seed, float p_drop) {
    AttnArgs a;
    a.qkv = qkv, a.out = out, a.lse = lse, a.dout = dout, a.dqkv = dqkv, a.H = H, a.scale = scale, a.seed = seed;
    a.seed_base = dropout_seed_base();
    const double t = static_cast<double>(p_drop) * 4294967296.0;
    a.thresh = p_drop <= 0.f ? 0u : (t >= 4294967295.0 ? 0xffffffffu : static_cast<uint32_t>(t));
    a.inv_keep = p_drop < 1.f ? 1.f / (1.f - p_drop) : 0.f;
    return a;
}

}  // namespace

// attention_long.hip: the streaming kernels, every S that is a multiple of 64 from 128 to 512
// (dsum: [B, H, S] f32 scratch the backward fills with rowsum(dO o O))
bool attention_long_supported(int S);
void launch_attention_long_forward(const uint16_t *qkv, uint16_t *out, float *lse, int B, int S, int H, float scale,
                                   uint32_t seed, float p_drop, hipStream_t s);
void launch_attention_long_backward(const uint16_t *qkv, const uint16_t *out, const float *lse, const uint16_t *dout,
                                    uint16_t *dqkv, float *dsum, int B, int S, int H, float scale, uint32_t seed,
                                    float p_drop, hipStream_t s);

}  // namespace kfk
