// csrc/kernels/recip_div.hpp on the CPU (tests/test_rounding_cases.py): for every divisor d in
// [1, 32770] and a few larger ones, recip_div(n, recip_magic(d), recip_shift(d)) against n / d at the extreme
// and boundary dividends; exits 1 at the first mismatch.  Prints one line per divisor,
//   d magic shift  n:q n:q ...
// so the caller can compare the quotients with its own integer division too.
#include "recip_div.hpp"

#include <cstdint>
#include <cstdio>
#include <vector>

int main() {
    const int64_t kMax = (int64_t(1) << 31) - 1;  // dividends are ints below 2^31
    std::vector<uint32_t> ds;
    for (uint32_t d = 1; d <= 32770; ++d) ds.push_back(d);
    for (uint32_t d : {65535u, 65536u, 65537u, 1u << 20, (1u << 30) + 1u, (1u << 31) - 1u}) ds.push_back(d);
    for (uint32_t d : ds) {
        const uint32_t magic = kfk::recip_magic(d);
        const int shift = kfk::recip_shift(d);
        std::vector<int64_t> ns = {0, 1, 2, kMax, kMax - 1, kMax - d, int64_t(1) << 30, (int64_t(1) << 30) - 1};
        const int64_t top = kMax / d;  // the largest quotient
        for (int64_t q : {int64_t(1), int64_t(2), int64_t(3), top / 2, top - 1, top})
            for (int64_t off : {-1, 0, 1}) ns.push_back(q * d + off);
        // the small dividends, and a stride of odd steps across the whole range
        for (int64_t n = 0; n < 4 * int64_t(d) && n < 2048; ++n) ns.push_back(n);
        for (int64_t n = d; n <= kMax; n += int64_t(100891939) + d) ns.push_back(n);
        std::printf("%u %u %d ", d, magic, shift);
        int shown = 0;
        for (int64_t n : ns) {
            if (n < 0 || n > kMax) continue;
            const int q = kfk::recip_div(static_cast<int>(n), magic, shift);
            if (q != n / d) {
                std::printf("\nMISMATCH n=%lld d=%u got %d want %lld\n", static_cast<long long>(n), d, q,
                            static_cast<long long>(n / d));
                return 1;
            }
            if (shown < 26) {
                std::printf(" %lld:%d", static_cast<long long>(n), q);
                ++shown;
            }
        }
        std::printf("\n");
    }
    return 0;
}
