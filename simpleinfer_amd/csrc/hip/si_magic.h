// si_magic.h -- division by a run-time constant that the host prepared: one multiply-high and one correction step instead of the
// ~40 instructions of an emulated integer division.  Pure: plain C++ and constexpr, so the same two functions serve host code and
// kernels, and the contract below is exercised without a device (tests/cpp/test_magic_div.cpp).
//
// Contract: 0 <= n < 2^31, d >= 1, mg = si_magic(d); then si_fast_div(n, d, mg) == n / d.
// With mg = floor(2^32 / d) the estimate q = floor(n * mg / 2^32) falls short of n / d by n * (2^32 / d - mg) / 2^32 < 1/2 for
// n < 2^31, plus the floor: q is the quotient or one less, and one correction step reaches it.  d == 1 has no 32-bit
// floor(2^32 / d); 0xFFFFFFFF gives q = n - 1 (0 for n = 0), corrected to n.
//
// A different scheme -- floor(2^32 / d) + 1 without a correction, for a narrower range of n -- lives in pixel_shuffle.hip; the two
// constants are not interchangeable.
#ifndef SI_MAGIC_H_
#define SI_MAGIC_H_

#include <cstdint>

// the constant of a divisor d >= 1
constexpr unsigned si_magic(int d) { return d > 1 ? (unsigned)(0x100000000ull / (unsigned)d) : 0xFFFFFFFFu; }

// n / d for 0 <= n < 2^31, d >= 1, mg = si_magic(d).  The high half of the 32x32 product compiles to one v_mul_hi_u32 / s_mul_hi_u32.
__attribute__((always_inline)) constexpr int si_fast_div(int n, int d, unsigned mg) {
    unsigned q = (unsigned)(((uint64_t)(unsigned)n * mg) >> 32);
    if ((unsigned)n - q * (unsigned)d >= (unsigned)d) ++q;
    return (int)q;
}

// quotient and remainder at once, same contract: what an index decomposition (item -> row, column) asks for at every level
__attribute__((always_inline)) constexpr int si_fast_divmod(int n, int d, unsigned mg, int& rem) {
    const int q = si_fast_div(n, d, mg);
    rem = n - q * d;
    return q;
}

#endif  // SI_MAGIC_H_
