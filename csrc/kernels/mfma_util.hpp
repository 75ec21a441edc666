// Device helpers shared by the MFMA / LDS-DMA kernels (conv_kernel.hpp, conv_wgrad.hip, gemm.hip,
// stem.hip, stem3.hip, attention_common.hpp): the vector types, the counted vmcnt wait, the LDS
// address-space cast, the transposing operand read, the 32-byte column-group swizzle of an LDS image
// row, the 40-bit magic division and the XCD-aware workgroup remap.  Everything sits in an unnamed
// namespace: private to each including file, no exported symbol.
#pragma once
#include "common.hpp"

namespace kfk {

namespace {

// (f32x2 and bf16x2 are in common.hpp, with pack_bf16x2_hw, which needs them)
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned u32x2;
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

// s_waitcnt until at most N of this wave's vector-memory operations (LDS-DMA included) are in flight
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// the LDS (address space 3) form of a pointer into __shared__ memory, as the LDS-DMA builtins take it
__device__ __forceinline__ __attribute__((address_space(3))) void *lds_ptr(uint8_t *p) {
    return (__attribute__((address_space(3))) void *)(p);
}

// One MFMA operand from two transposing reads (ds_read_b64_tr_b16): p0 / p1 are the lane's addresses in
// the two 4-row blocks of an image whose ROWS are the MFMA K index; each read hands the lane 4 rows of
// one column.
__device__ __forceinline__ bf16x8 tr_frag(const uint8_t *p0, const uint8_t *p1) {
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4 *)(p0));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4 *)(p1));
    const s16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(bf16x8, v);
}

// 32-byte column-group swizzle of an LDS image row (ROW = 64, 128, 256 or 512 bytes), XOR-ed into the
// group index on the staging source address and on the read address: the 8 rows one 32-lane half of a
// transposing read touches (two 4-row blocks 8 rows apart) land on 8 distinct 32-byte bank groups.  A
// 512-byte row spans two 256-byte bank cycles, so the 3-bit swizzle of 256-byte rows serves it too.
template <int ROW>
__device__ __forceinline__ int hswz(int row) {
    static_assert(ROW == 64 || ROW == 128 || ROW == 256 || ROW == 512, "staged row bytes");
    if constexpr (ROW >= 256) return (row & 3) | (((row >> 3) & 1) << 2);
    else if constexpr (ROW == 64) return (row >> 3) & 1;  // 4 rows per 256-byte bank cycle: flip rows 8..15
    else return ((row >> 1) & 1) | (((row >> 3) & 1) << 1);
}

// floor(p / d) with the host's magic m = 2^40 / d + 1 (wgrad_plan.cpp magic40), exact for p * d < 2^40.
// The weight-gradient and stem kernels keep this 40-bit form; recip_div.hpp's is the conv kernels'.
__device__ __forceinline__ int fdiv(int p, uint64_t m) {
    return static_cast<int>((static_cast<uint64_t>(static_cast<uint32_t>(p)) * m) >> 40);
}

// Bijective XCD remap: hardware workgroup `orig` of `nwg` runs on XCD orig % 8; the workgroups that
// share an XCD (and its L2) get a contiguous run of the logical indices.
__device__ __forceinline__ int xcd_remap(int orig, int nwg) {
    const int q8 = nwg >> 3, rr = nwg & 7, xcd = orig & 7;
    return (xcd < rr ? xcd * (q8 + 1) : rr * (q8 + 1) + (xcd - rr) * q8) + (orig >> 3);
}

}  // namespace

}  // namespace kfk
