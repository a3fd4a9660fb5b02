// The host-side view rules every kernel file shares (simpleinfer_amd/csrc/hip/si_views.h): alignment and vector width, byte-range overlap,
// the extent of a strided view, and the strided-window test behind reduce.hip's and activation_param.hip's views_overlap.  Stand-alone; built
// with -fsanitize=address,undefined by tests/test_views_cpu.py.  The addresses are numbers: nothing here is dereferenced.
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "si_views.h"

static long long failures = 0, checked = 0;

#define EXPECT(cond)                                                                  \
    do {                                                                              \
        ++checked;                                                                    \
        if (!(cond) && ++failures <= 20) std::printf("line %d: %s\n", __LINE__, #cond); \
    } while (0)

static const void* at(uint64_t address) { return reinterpret_cast<const void*>(static_cast<uintptr_t>(address)); }

static void test_alignment_and_width() {
    EXPECT(si_aligned_to(at(0x1000), 16) && !si_aligned_to(at(0x1008), 16) && si_aligned_to(at(0x1008), 8) && !si_aligned_to(at(0x1001), 2));
    EXPECT(si_aligned_to(at(0x1003), 1));
    // fp32: 4 elements; fp16: 8
    EXPECT(si_vector_width<float>(8, 8, 12, at(0x1000), at(0x2000)) == 4);
    EXPECT(si_vector_width<uint16_t>(8, 8, 16, at(0x1000), at(0x2000)) == 8);
    EXPECT(si_vector_width<uint16_t>(12, 16, 16, at(0x1000), at(0x2000)) == 1);   // c a multiple of 4, not of 8
    EXPECT(si_vector_width<float>(12, 16, 16, at(0x1000), at(0x2000)) == 4);
    EXPECT(si_vector_width<float>(6, 8, 8, at(0x1000), at(0x2000)) == 1);         // c
    EXPECT(si_vector_width<float>(8, 10, 8, at(0x1000), at(0x2000)) == 1);        // input stride
    EXPECT(si_vector_width<float>(8, 8, 10, at(0x1000), at(0x2000)) == 1);        // output stride
    EXPECT(si_vector_width<float>(8, 8, 8, at(0x1004), at(0x2000)) == 1);         // input pointer
    EXPECT(si_vector_width<float>(8, 8, 8, at(0x1000), at(0x2008)) == 1);         // output pointer
}

static void test_ranges() {
    const void* a = at(0x1000);
    EXPECT(!si_ranges_overlap(a, 16, at(0x1010), 16) && !si_ranges_overlap(at(0x1010), 16, a, 16));   // touching
    EXPECT(si_ranges_overlap(a, 17, at(0x1010), 16) && si_ranges_overlap(at(0x1010), 16, a, 17));     // one byte shared
    EXPECT(si_ranges_overlap(a, 64, at(0x1010), 4) && si_ranges_overlap(at(0x1010), 4, a, 64));       // nested
    EXPECT(si_ranges_overlap(a, 8, a, 8));                                                           // the same range
    EXPECT(!si_ranges_overlap(a, 16, at(0x4000), 16) && !si_ranges_overlap(at(0x4000), 16, a, 16));   // disjoint
    // zero length: nothing shared at either end or outside; an empty range strictly inside another one counts as inside it
    EXPECT(!si_ranges_overlap(a, 0, a, 16) && !si_ranges_overlap(a, 16, a, 0));
    EXPECT(!si_ranges_overlap(at(0x1010), 0, a, 16) && !si_ranges_overlap(a, 0, at(0x1000), 0));
    EXPECT(si_ranges_overlap(at(0x1008), 0, a, 16));
}

static void test_extent() {
    const uint64_t L = SI_INDEX_LIMIT;
    EXPECT(L == 0x7fffffffull);
    EXPECT(si_view_extent(2, 3, 4, 10, 7) == 23 * 10 + 7);
    EXPECT(si_view_extent(1, 1, 1, 1000000, 5) == 5);            // one pixel: the stride does not count
    EXPECT(si_view_extent(1, 1, 1, 5, L) == L && si_view_extent(1, 1, 1, 5, L + 1) == 0);
    EXPECT(si_view_extent(1, 1, L, 1, 1) == L && si_view_extent(1, 1, L + 1, 1, 1) == 0);      // pixels at and beyond the limit
    EXPECT(si_view_extent(L, 1, 1, 1, 1) == L && si_view_extent(L + 1, 1, 1, 1, 1) == 0);      // rows at and beyond the limit
    EXPECT(si_view_extent(1, 1, 2, L - 1, 1) == L && si_view_extent(1, 1, 2, L, 1) == 0);      // the last element at and beyond the limit
    EXPECT(si_view_extent(L, L, 2, 1, 1) == 0);                   // rows < 2^62: no wrap on the way
    EXPECT(si_view_extent(1u << 16, 1u << 15, 1, 1, 1) == 0);     // rows == 2^31
}

// do an element of a and an element of b share a byte?  Every pair of windows.
static bool oracle(int64_t ab, int pa, int lda, int wa, int64_t bb, int pb, int ldb, int wb, int es) {
    for (int i = 0; i < pa; ++i) {
        const int64_t a0 = ab + (int64_t)i * lda * es, a1 = a0 + (int64_t)wa * es;
        for (int j = 0; j < pb; ++j) {
            const int64_t b0 = bb + (int64_t)j * ldb * es, b1 = b0 + (int64_t)wb * es;
            if (a0 < b1 && b0 < a1) return true;
        }
    }
    return false;
}

// The rule must never miss a shared element, whatever the strides; for a common stride (the case it decides exactly) it must also not
// refuse two views that share none.  Every byte offset of b against a within two periods on either side, aligned to an element or not.
static void test_strided_windows() {
    const int64_t base = 1 << 20;
    const int pixel_counts[] = {1, 2, 3, 6}, widths[] = {1, 2, 3, 6};
    long long cases = 0, exact_no = 0;
    for (int es : {2, 4})
        for (int lda = 1; lda <= 12; ++lda)
            for (int ldb : {lda, lda % 12 + 1, 13 - lda})
                for (int wa : widths)
                    for (int wb : widths) {
                        if (wa > lda || wb > ldb) continue;
                        for (int pa : pixel_counts)
                            for (int pb : pixel_counts) {
                                const int reach = 2 * (lda > ldb ? lda : ldb) * es;
                                const int64_t span_b = ((int64_t)(pb - 1) * ldb + wb) * es, span_a = ((int64_t)(pa - 1) * lda + wa) * es;
                                for (int64_t off = -span_b - reach; off <= span_a + reach; ++off) {
                                    const bool want = oracle(base, pa, lda, wa, base + off, pb, ldb, wb, es);
                                    const bool got = si_strided_windows_overlap(at(base), pa, lda, wa, at(base + off), pb, ldb, wb, es);
                                    ++cases;
                                    if (want) EXPECT(got);
                                    if (lda == ldb) {
                                        EXPECT(got == want);
                                        if (!want && off > 0 && off < span_a) ++exact_no;
                                    }
                                }
                            }
                    }
    // the documented case: one pixel grid, channel windows [0, 4) and [4, 8) of 8-channel pixels, interleaved over 6 pixels: nothing shared
    EXPECT(!si_strided_windows_overlap(at(base), 6, 8, 4, at(base + 4 * 4), 6, 8, 4, 4));
    EXPECT(si_strided_windows_overlap(at(base), 6, 8, 5, at(base + 4 * 4), 6, 8, 4, 4));      // ... one channel wider: shared
    EXPECT(si_strided_windows_overlap(at(base), 6, 8, 4, at(base + 4 * 4), 6, 8, 5, 4));      // ... b reaches the next pixel's window
    EXPECT(!si_strided_windows_overlap(at(base + 4 * 4), 6, 8, 4, at(base), 6, 8, 4, 4));     // ... b below a
    EXPECT(si_strided_windows_overlap(at(base), 6, 8, 4, at(base + 4 * 4), 6, 12, 4, 4));     // unequal strides inside one range: refused
    EXPECT(exact_no > 0);   // interleaved views without a shared element were among the cases
    std::printf("%lld strided-window cases\n", cases);
}

int main() {
    test_alignment_and_width();
    test_ranges();
    test_extent();
    test_strided_windows();
    if (failures) {
        std::printf("%lld of %lld checks failed\n", failures, checked);
        return 1;
    }
    std::printf("views ok (%lld checks)\n", checked);
    return 0;
}
