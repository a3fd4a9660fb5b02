// The division by a prepared constant that six kernels use (simpleinfer_amd/csrc/hip/si_magic.h): si_fast_div(n, d, si_magic(d)) == n / d for
// 0 <= n < 2^31 and d >= 1.  Stand-alone; built with -fsanitize=address,undefined by tests/test_magic_div_cpu.py.  Every d in 1..4096 and a few
// around 2^16, 2^20, 2^30 and at 2^31 - 1; per d the values of n next to the multiples of d where an estimate that is one short shows, the ends of
// the range and 10 000 values of a fixed-seed generator.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "si_magic.h"

static_assert(si_magic(1) == 0xFFFFFFFFu && si_magic(2) == 0x80000000u && si_magic(3) == 0x55555555u, "floor(2^32 / d), all ones for d = 1");
static_assert(si_fast_div(0, 1, si_magic(1)) == 0 && si_fast_div(7, 1, si_magic(1)) == 7 && si_fast_div(0x7fffffff, 3, si_magic(3)) == 0x7fffffff / 3,
              "usable in constant expressions");

static constexpr int64_t kLimit = (int64_t)1 << 31;   // n < 2^31

static long long failures = 0, checked = 0;

static void check(int64_t n, int d, unsigned mg) {
    if (n < 0 || n >= kLimit) return;   // outside the contract (d + 1 or k * d + 1 at the top of the range)
    ++checked;
    const int got = si_fast_div((int)n, d, mg), want = (int)n / d;
    if (got != want && ++failures <= 20) std::printf("si_fast_div(%d, %d, 0x%08x) = %d, n / d = %d\n", (int)n, d, mg, got, want);
}

// xorshift64*, fixed seed: the same 31-bit values in every run
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static int next31() {
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return (int)((rng_state * 0x2545F4914F6CDD1Dull) >> 33);
}

int main() {
    std::vector<int> divisors;
    for (int d = 1; d <= 4096; ++d) divisors.push_back(d);
    for (int d : {65535, 65536, 65537, 409600, (1 << 20) - 1, (1 << 20) + 1, 1 << 30, 0x7fffffff}) divisors.push_back(d);

    for (int d : divisors) {
        const unsigned mg = si_magic(d);
        const int64_t dd = d;
        for (int64_t n : {(int64_t)0, (int64_t)1, dd - 1, dd, dd + 1, kLimit - 1}) check(n, d, mg);
        const int64_t kmax = (kLimit - 1) / dd;   // the largest k with k * d < 2^31
        for (int64_t k : {(int64_t)2, (int64_t)3, (int64_t)1000, kmax})
            for (int64_t n : {k * dd - 1, k * dd, k * dd + 1}) check(n, d, mg);
        for (int i = 0; i < 10000; ++i) check(next31(), d, mg);
    }
    if (failures) {
        std::printf("%lld of %lld quotients wrong\n", failures, checked);
        return 1;
    }
    std::printf("magic div ok (%zu divisors, %lld quotients)\n", divisors.size(), checked);
    return 0;
}
