// xcorr_plan.h -- the host arithmetic of the cross-correlation kernels (include/si_xcorr.h): which form serves a shape, torch's output extent
// with an implied far pad, `same` / `valid` pads, view extents and stride rules, tile counts, the grid and the 31-bit checks.  Pure: standard
// headers only, nothing of the device runtime, so it is exercised without a device (tests/cpp/test_xcorr_plan.cpp).
#ifndef SI_XCORR_PLAN_H_
#define SI_XCORR_PLAN_H_

#include <cstdint>

namespace si_xcorr_plan {

constexpr uint64_t kIndexLimit = 0x7fffffffull;   // kernels index with 32-bit element offsets
constexpr uint64_t kGridLimitYZ = 65535;          // a grid's y and z extents
constexpr uint64_t kLdsBytes = 0;                 // neither kernel stages anything in LDS: a need above this is refused (none arises)

constexpr int kTileOc = 16;        // filters of one MFMA tile (the M of both instructions)
constexpr int kWaveTiles = 4;      // filter tiles a wave keeps accumulators for: 64 filters per workgroup row
constexpr int kBlockOc = kTileOc * kWaveTiles;
constexpr int kWavePix = 16;       // output pixels of a wave (the N of both instructions)
constexpr int kBlockPix = 64;      // output pixels of a dense workgroup of four waves
constexpr int kChanF32 = 16;       // channels of one fp32 block (one tap): four v_mfma_f32_16x16x4_f32 steps on 16-byte fragments
constexpr int kChanF16 = 32;       // channels of one v_mfma_f32_16x16x32_f16 step (one tap)
constexpr int kThreads = 256;
constexpr int kDwRunF32 = 4;       // consecutive channels of a depthwise lane: 16 bytes of the storage type
constexpr int kDwRunF16 = 8;

enum Form { kNone = 0, kDense = 1, kDepthwise = 2 };

struct Shape {
    int n = 0, h = 0, w = 0, c = 0, oc = 0, ho = 0, wo = 0, kh = 0, kw = 0;
    int stride_h = 0, stride_w = 0, dilation_h = 0, dilation_w = 0, pad_top = 0, pad_left = 0, groups = 0;
    int per_sample = 0;   // depthwise alone: filter n meets image n
};

// sizes alone (SI_E_BADARG otherwise); the group count is judged by FormOf
inline bool Positive(const Shape& s) {
    return s.n > 0 && s.h > 0 && s.w > 0 && s.c > 0 && s.oc > 0 && s.ho > 0 && s.wo > 0 && s.kh > 0 && s.kw > 0 && s.stride_h > 0 && s.stride_w > 0 &&
           s.dilation_h > 0 && s.dilation_w > 0 && s.pad_top >= 0 && s.pad_left >= 0 && s.groups > 0;
}

// the one place that chooses the kernel family: groups == C == OC (multiplier 1; one channel and one filter included, where both forms
// compute the same thing) is the VALU kernel, every other groups == 1 the MFMA kernel; other group counts, and per-sample filters with
// anything but the depthwise form, have no kernel (SI_E_UNSUPPORTED)
inline Form FormOf(const Shape& s) {
    if (!Positive(s)) return kNone;
    if (s.groups == s.c && s.groups == s.oc) return kDepthwise;
    if (s.groups == 1 && !s.per_sample) return kDense;
    return kNone;
}

// the fp16 rule of the dense form: a lane's fragment is 8 consecutive channels
inline bool HalfOk(const Shape& s) { return FormOf(s) == kDepthwise || (FormOf(s) == kDense && s.c % 8 == 0); }

// torch's output extent: floor((L + p0 + p1 - d (K - 1) - 1) / s) + 1, or 0 when the padded input is smaller than the window
inline int64_t OutExtent(int64_t l, int64_t p0, int64_t p1, int64_t k, int64_t s, int64_t d) {
    const int64_t e = l + p0 + p1 - d * (k - 1) - 1;
    return e < 0 ? 0 : e / s + 1;
}

// the smallest far pad >= 0 with which torch's formula gives `lo`, or -1 when none does
inline int64_t ImpliedFarPad(int64_t l, int64_t p0, int64_t lo, int64_t k, int64_t s, int64_t d) {
    if (l <= 0 || p0 < 0 || lo <= 0 || k <= 0 || s <= 0 || d <= 0) return -1;
    const int64_t need = (lo - 1) * s + d * (k - 1) + 1 - l - p0;
    const int64_t p1 = need > 0 ? need : 0;
    return OutExtent(l, p0, p1, k, s, d) == lo ? p1 : -1;
}

inline bool ExtentsOk(const Shape& s) {
    return ImpliedFarPad(s.h, s.pad_top, s.ho, s.kh, s.stride_h, s.dilation_h) >= 0 &&
           ImpliedFarPad(s.w, s.pad_left, s.wo, s.kw, s.stride_w, s.dilation_w) >= 0;
}

// torch's padding='same' (stride 1): total d (K - 1), the near half rounded down, the odd one on the far side
inline int SamePadNear(int k, int d) { return (int)(((int64_t)d * (k - 1)) / 2); }
inline int SamePadFar(int k, int d) { return (int)((int64_t)d * (k - 1) - SamePadNear(k, d)); }

// one past the last element offset of a view [n][h][w][c] with the element strides (sn, sh, sp, sc), or 0 when a stride is negative or
// the offset beyond 31 bits
inline uint64_t ViewExtent(int n, int h, int w, int c, long long sn, long long sh, long long sp, long long sc) {
    if (n <= 0 || h <= 0 || w <= 0 || c <= 0 || sn < 0 || sh < 0 || sp < 0 || sc < 0) return 0;
    if ((uint64_t)sn > kIndexLimit || (uint64_t)sh > kIndexLimit || (uint64_t)sp > kIndexLimit || (uint64_t)sc > kIndexLimit) return 0;
    const uint64_t last = (uint64_t)(n - 1) * (uint64_t)sn + (uint64_t)(h - 1) * (uint64_t)sh + (uint64_t)(w - 1) * (uint64_t)sp +
                          (uint64_t)(c - 1) * (uint64_t)sc;
    return last > kIndexLimit ? 0 : last + 1;
}

// the strides of a view that is WRITTEN (channels contiguous): pixels at least c apart, rows at least a row apart, images an image apart,
// so that no two elements share an address
inline bool NestedStrides(int n, int h, int w, int c, long long sn, long long sh, long long sp) {
    if (sp < c) return false;
    if (h > 1 && sh < (long long)(w - 1) * sp + c) return false;
    if (n > 1 && sn < (long long)(h - 1) * sh + (long long)(w - 1) * sp + c) return false;
    return sn >= 0 && sh >= 0;
}

inline uint64_t OutPixels(const Shape& s) { return (uint64_t)s.ho * (uint64_t)s.wo; }
inline int OcTiles(const Shape& s) { return (s.oc + kTileOc - 1) / kTileOc; }
inline int OcBlocks(const Shape& s) { return (s.oc + kBlockOc - 1) / kBlockOc; }
// filter tiles a wave keeps accumulators for: all of them up to four (then the filters are walked in blocks of 64)
inline int WaveTiles(const Shape& s) { return OcTiles(s) < kWaveTiles ? OcTiles(s) : kWaveTiles; }
inline int ChanSteps(const Shape& s, bool half) {
    const int per = half ? kChanF16 : kChanF32;
    return (s.c + per - 1) / per;
}
inline int DwRun(bool half) { return half ? kDwRunF16 : kDwRunF32; }
inline int DwChanRuns(const Shape& s, bool half) { return (s.c + DwRun(half) - 1) / DwRun(half); }

struct Grid {
    unsigned x = 0, y = 0, z = 0;
};

// dense: (tile of 64 output pixels of one image, block of 64 filters, image); depthwise: (256 items of (pixel, channel run) of one image, 1,
// image).  false: a y / z extent beyond 65535 or x beyond 31 bits
inline bool MakeGrid(const Shape& s, bool half, Grid& g) {
    const Form f = FormOf(s);
    if (f == kNone) return false;
    uint64_t x, y;
    if (f == kDense) {
        x = (OutPixels(s) + kBlockPix - 1) / kBlockPix;
        y = (uint64_t)OcBlocks(s);
    } else {
        const uint64_t items = OutPixels(s) * (uint64_t)DwChanRuns(s, half);
        if (items > kIndexLimit) return false;   // (an item index is a 32-bit value on the device)
        x = (items + kThreads - 1) / kThreads;
        y = 1;
    }
    if (x > kIndexLimit || y > kGridLimitYZ || (uint64_t)s.n > kGridLimitYZ) return false;
    g.x = (unsigned)x; g.y = (unsigned)y; g.z = (unsigned)s.n;
    return true;
}

// the device computes input coordinates as o s - p + k d and output pixel indices with the tile rounded up in 32 bits: the largest must fit
inline bool PositionsFit(const Shape& s) {
    const uint64_t wh = (uint64_t)s.ho * (uint64_t)s.stride_h + (uint64_t)s.kh * (uint64_t)s.dilation_h + (uint64_t)s.pad_top;
    const uint64_t ww = (uint64_t)s.wo * (uint64_t)s.stride_w + (uint64_t)s.kw * (uint64_t)s.dilation_w + (uint64_t)s.pad_left;
    return wh <= kIndexLimit && ww <= kIndexLimit && OutPixels(s) + kBlockPix <= kIndexLimit;
}

}  // namespace si_xcorr_plan

#endif  // SI_XCORR_PLAN_H_
