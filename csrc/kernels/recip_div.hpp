// Exact division of a non-negative 31-bit integer by a divisor that is fixed for a whole launch, as a
// shift, one multiply-high and a shift -- instead of the ~20-instruction expansion the compiler emits
// for a runtime divisor.  Host and device code (plain C++, no HIP header): the conv kernels decode
// output pixels with it (conv_kernel.hpp), tests/native/recip_div_check.cpp checks it on the CPU.
//
//   L = ceil(log2 d)   (0 for d = 1),   k = 31 + L,   magic = floor(2^k / d) + 1
//   n / d = floor(n * magic / 2^k) = mulhi(2 n, magic) >> L     for 0 <= n < 2^31, 1 <= d < 2^31.
//
// Proof.  magic * d = 2^k + e with 0 < e <= d.  Write n = q d + r, 0 <= r <= d - 1.  Then
//   n * magic / 2^k = n / d + n e / (d 2^k) = q + (r + n e / 2^k) / d,
// whose floor is q as long as n e / 2^k < 1.  n < 2^31 and e <= d <= 2^L give n e < 2^(31 + L) = 2^k.
// magic fits 32 bits: for d > 1, d > 2^(L-1) so 2^k / d < 2^32, and floor(2^k / d) = 2^32 - 1 would
// need d <= 2^(L-1) (1 + 2^-32), i.e. d = 2^(L-1); for d = 1, magic = 2^31 + 1.  2 n < 2^32 fits too.
// The launchers admit divisors up to 2^15 + 2 (image sides up to 2^15, padded by 2) and dividends
// below 2^31 (pixel counts are ints), well inside both ranges.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define KFK_HD __host__ __device__
#else
#define KFK_HD
#endif

namespace kfk {

// ceil(log2 d), 0 for d = 1 (d >= 1)
KFK_HD inline int recip_shift(uint32_t d) { return d > 1 ? 32 - __builtin_clz(d - 1) : 0; }

// host side: the multiplier of divisor d (1 <= d < 2^31)
inline uint32_t recip_magic(uint32_t d) {
    return static_cast<uint32_t>((static_cast<uint64_t>(1) << (31 + recip_shift(d))) / d + 1);
}

// n / d for 0 <= n < 2^31, with magic = recip_magic(d) and shift = recip_shift(d)
KFK_HD inline int recip_div(int n, uint32_t magic, int shift) {
    const uint64_t p = static_cast<uint64_t>(static_cast<uint32_t>(n) << 1) * magic;
    return static_cast<int>(static_cast<uint32_t>(p >> 32) >> shift);
}

}  // namespace kfk
