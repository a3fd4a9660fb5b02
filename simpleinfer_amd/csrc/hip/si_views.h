// si_views.h -- what the host side of every kernel file asks about its views before a launch: is this pointer aligned, how far does this
// view reach, do these two views share a byte.  Pure: plain C++, so the rules are exercised without a device (tests/cpp/test_views.cpp).
// Sums of an address and a byte count are taken as written (no wrap-around handling): the callers pass extents that fit 31-bit element
// offsets, far below the top of the address space.
#ifndef SI_VIEWS_H_
#define SI_VIEWS_H_

#include <cstdint>

// kernels index with 32-bit element offsets: a view whose last element lies beyond this is SI_E_UNSUPPORTED
constexpr uint64_t SI_INDEX_LIMIT = 0x7fffffffull;

// `bytes`: a power of two
static inline bool si_aligned_to(const void* p, uint64_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0; }

// 16-byte channel vectors when c, both strides and both pointers allow it; single elements otherwise
template <typename T>
static inline int si_vector_width(int c, int in_ld, int out_ld, const void* in, const void* out) {
    const int full = (int)(16 / sizeof(T));
    const bool vec = c % full == 0 && in_ld % full == 0 && out_ld % full == 0 && si_aligned_to(in, 16) && si_aligned_to(out, 16);
    return vec ? full : 1;
}

// do the byte ranges [a, a + a_bytes) and [b, b + b_bytes) share a byte?  (an empty range shares none with a range it does not lie inside)
static inline bool si_ranges_overlap(const void* a, uint64_t a_bytes, const void* b, uint64_t b_bytes) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

// elements from the first to the last element of a view of n h w pixels of c channels, ld apart; 0: beyond the index limit
static inline uint64_t si_view_extent(uint64_t n, uint64_t h, uint64_t w, uint64_t ld, uint64_t c) {
    const uint64_t rows = n * h;   // < 2^62
    if (rows > SI_INDEX_LIMIT) return 0;
    const uint64_t pixels = rows * w;
    if (pixels > SI_INDEX_LIMIT) return 0;
    const uint64_t e = (pixels - 1) * ld + c;
    return e > SI_INDEX_LIMIT ? 0 : e;
}

// Two strided views -- `pixels` windows of `width` elements, `ld` elements apart, elements of `esize` bytes: may they share an element?
// False when their byte ranges are apart, and when both lie on one pixel grid (a common stride) as channel windows that do not meet
// inside a pixel; true otherwise (conservative for unequal strides).
static inline bool si_strided_windows_overlap(const void* a, uint64_t a_pixels, uint64_t a_ld, uint64_t a_width, const void* b, uint64_t b_pixels,
                                              uint64_t b_ld, uint64_t b_width, uint64_t esize) {
    const uintptr_t ab = reinterpret_cast<uintptr_t>(a), bb = reinterpret_cast<uintptr_t>(b);
    const uintptr_t ae = ab + (uintptr_t)(((a_pixels - 1) * a_ld + a_width) * esize);
    const uintptr_t be = bb + (uintptr_t)(((b_pixels - 1) * b_ld + b_width) * esize);
    if (ae <= bb || be <= ab) return false;
    if (a_ld == b_ld) {
        const uint64_t pitch = a_ld * esize;
        const uint64_t m = bb >= ab ? (uint64_t)(bb - ab) % pitch : (pitch - (uint64_t)(ab - bb) % pitch) % pitch;   // b's window inside a's period
        if (m >= a_width * esize && m + b_width * esize <= pitch) return false;
    }
    return true;
}

#endif  // SI_VIEWS_H_
