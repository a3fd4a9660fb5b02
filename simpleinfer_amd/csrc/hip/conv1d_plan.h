// conv1d_plan.h -- the host arithmetic of the temporal convolution kernels (include/si_conv1d.h): which form serves a shape, torch's output
// length with an implied right pad, tile spans, LDS sizes, weight-image sizes and indices, the grid and the 31-bit checks.  Pure: nothing of
// the device runtime, so it is exercised without a device (tests/cpp/test_conv1d_plan.cpp).
#ifndef SI_CONV1D_PLAN_H_
#define SI_CONV1D_PLAN_H_

#include <cstdint>

namespace si_conv1d_plan {

constexpr uint64_t kIndexLimit = 0x7fffffffull;   // kernels index with 32-bit element offsets
constexpr uint64_t kGridLimitYZ = 65535;          // a grid's y and z extents
constexpr uint64_t kLdsLimit = 64 * 1024;         // no kernel here asks for more dynamic LDS than the default allows

constexpr int kTileOc = 16;          // output channels of a wave (the M of both MFMAs)
constexpr int kBlockOc = 64;         // output channels of a workgroup of four waves
constexpr int kTilePos = 64;         // output positions of a dense workgroup: four 16-column MFMA tiles per wave
constexpr int kChanF32 = 4;          // channels of one v_mfma_f32_16x16x4_f32 step (one tap)
constexpr int kChanF16 = 32;         // channels of one v_mfma_f32_16x16x32_f16 step (one tap)
constexpr int kMaxChunkF16 = 128;    // most channels the fp16 LDS image holds at a time
constexpr int kRowPadF16 = 8;        // halves of padding behind the channels of one position's row of the fp16 LDS image
constexpr int kMaxChunkF32 = 32;     // most channels the fp32 LDS image holds at a time
constexpr int kDwRows = 4;           // (n, c) rows of a depthwise workgroup: one per wave
constexpr int kDwRun = 4;            // consecutive outputs of a depthwise lane
constexpr int kDwPos = 64 * kDwRun;  // output positions of a depthwise workgroup

enum Form { kNone = 0, kDense = 1, kDepthwise = 2 };

struct Shape {
    int n = 0, c = 0, l = 0, oc = 0, lo = 0, k = 0, stride = 0, dilation = 0, pad_left = 0, groups = 0;
};

inline bool Positive(const Shape& s) {
    return s.n > 0 && s.c > 0 && s.l > 0 && s.oc > 0 && s.lo > 0 && s.k > 0 && s.stride > 0 && s.dilation > 0 && s.pad_left >= 0 && s.groups > 0;
}

inline bool GroupsDivide(const Shape& s) { return s.groups > 0 && s.c % s.groups == 0 && s.oc % s.groups == 0; }

// the one place that chooses the kernel family: plain depthwise (groups == C == OC) is the VALU kernel, everything else the MFMA kernel
inline Form FormOf(const Shape& s) {
    if (!Positive(s) || !GroupsDivide(s)) return kNone;
    return (s.groups == s.c && s.groups == s.oc) ? kDepthwise : kDense;
}

// the fp16 rule of the dense form: a lane's B fragment is 8 consecutive channels
inline bool HalfOk(const Shape& s) { return FormOf(s) == kDepthwise || (FormOf(s) == kDense && (s.c / s.groups) % 8 == 0); }

// torch's output length: floor((L + pl + pr - d (K - 1) - 1) / s) + 1, or 0 when the padded input is shorter than the window
inline int64_t OutLen(int64_t l, int64_t pl, int64_t pr, int64_t k, int64_t s, int64_t d) {
    const int64_t e = l + pl + pr - d * (k - 1) - 1;
    return e < 0 ? 0 : e / s + 1;
}

// the smallest right pad >= 0 with which torch's formula gives `lo`, or -1 when none does (lo is too small for the left pad alone)
inline int64_t ImpliedRightPad(const Shape& s) {
    if (!Positive(s)) return -1;
    const int64_t need = (int64_t)(s.lo - 1) * s.stride + (int64_t)s.dilation * (s.k - 1) + 1 - s.l - s.pad_left;
    const int64_t pr = need > 0 ? need : 0;
    return OutLen(s.l, s.pad_left, pr, s.k, s.stride, s.dilation) == s.lo ? pr : -1;
}

// torch's padding='same' (stride 1): total d (K - 1), the left half rounded down
inline int SamePadLeft(int k, int d) { return (int)(((int64_t)d * (k - 1)) / 2); }
inline int SamePadRight(int k, int d) { return (int)((int64_t)d * (k - 1) - SamePadLeft(k, d)); }

// input positions a tile of `tile` outputs reads: (tile - 1) s + (K - 1) d + 1
inline uint64_t Span(const Shape& s, int tile) { return (uint64_t)(tile - 1) * (uint64_t)s.stride + (uint64_t)(s.k - 1) * (uint64_t)s.dilation + 1; }

// fp32 LDS row pitch in words: the span rounded up to 16 mod 32, so that the two channel rows a 32-lane half reads take different banks
inline uint64_t PitchF32(uint64_t span) { return (span + 15) / 32 * 32 + 16; }

inline int Cg(const Shape& s) { return s.c / s.groups; }
inline int Ocg(const Shape& s) { return s.oc / s.groups; }
inline int OcTiles(const Shape& s) { return (Ocg(s) + kTileOc - 1) / kTileOc; }      // per group
inline int OcBlocks(const Shape& s) { return (Ocg(s) + kBlockOc - 1) / kBlockOc; }   // per group
inline int ChanSteps(const Shape& s, bool half) {                                     // channel groups of one MFMA step, per conv group
    const int per = half ? kChanF16 : kChanF32;
    return (Cg(s) + per - 1) / per;
}

// channels the fp32 LDS image holds at a time: the largest multiple of 4 up to 32 (and up to the padded group) that fits; 0: none does
inline int ChunkF32(const Shape& s) {
    const uint64_t pitch = PitchF32(Span(s, kTilePos));
    const int padded = ChanSteps(s, false) * kChanF32;
    for (int cc = padded < kMaxChunkF32 ? padded : kMaxChunkF32; cc >= kChanF32; cc -= kChanF32)
        if ((uint64_t)cc * pitch * 4 <= kLdsLimit) return cc;
    return 0;
}

// channels the fp16 LDS image holds at a time: 128, 64 or 32 (at most the padded group), the largest whose rows fit; 0: none does
inline int ChunkF16(const Shape& s) {
    const uint64_t span = Span(s, kTilePos);
    const int padded = ChanSteps(s, true) * kChanF16;
    for (int cc = kMaxChunkF16; cc >= kChanF16; cc /= 2)
        if (cc <= padded || cc == kChanF16)
            if (span * (uint64_t)(cc + kRowPadF16) * 2 <= kLdsLimit) return cc;
    return 0;
}

// dynamic LDS bytes of a launch; 0: the span does not fit
inline uint64_t LdsBytes(const Shape& s, bool half) {
    const Form f = FormOf(s);
    uint64_t bytes = 0;
    if (f == kDepthwise) bytes = (uint64_t)kDwRows * (Span(s, kDwPos) + (uint64_t)s.k) * 4;   // per row: the span, then the K taps, as floats
    else if (f == kDense && half) bytes = ChunkF16(s) == 0 ? 0 : Span(s, kTilePos) * (uint64_t)(ChunkF16(s) + kRowPadF16) * 2;
    else if (f == kDense) bytes = (uint64_t)ChunkF32(s) * PitchF32(Span(s, kTilePos)) * 4;
    return bytes > kLdsLimit ? 0 : bytes;
}

// elements of the weight image (floats, or halves):
//   dense      [group][oc tile][channel step][tap][64 lanes][1 float | 8 halves]
//   depthwise  [C][K], the filters as torch stores them
inline uint64_t WeightElems(const Shape& s, bool half) {
    const Form f = FormOf(s);
    if (f == kDepthwise) return (uint64_t)s.c * (uint64_t)s.k;
    if (f != kDense) return 0;
    return (uint64_t)s.groups * (uint64_t)OcTiles(s) * (uint64_t)ChanSteps(s, half) * (uint64_t)s.k * 64ull * (half ? 8ull : 1ull);
}

// where (group, oc tile, channel step, tap, lane) starts in the dense image, in operand elements (floats, or groups of 8 halves)
inline uint64_t WeightIndex(const Shape& s, bool half, int group, int tile, int step, int tap, int lane) {
    return ((((uint64_t)group * OcTiles(s) + tile) * ChanSteps(s, half) + step) * (uint64_t)s.k + tap) * 64 + lane;
}

struct Grid {
    unsigned x = 0, y = 0, z = 0;
    int oc_blocks_per_wg = 0;   // dense: output-channel blocks a workgroup walks (1 without groups; all of its group's with groups)
};

// dense: (tile of 64 positions, output-channel block [groups == 1] or group [groups > 1], batch item); depthwise: (tile of 256 positions,
// four channels, batch item).  false: a y / z extent beyond 65535 or x beyond 31 bits
inline bool MakeGrid(const Shape& s, Grid& g) {
    const Form f = FormOf(s);
    if (f == kNone) return false;
    const uint64_t tile = f == kDepthwise ? kDwPos : kTilePos;
    const uint64_t x = ((uint64_t)s.lo + tile - 1) / tile;
    uint64_t y;
    if (f == kDepthwise) { y = ((uint64_t)s.c + kDwRows - 1) / kDwRows; g.oc_blocks_per_wg = 0; }
    else if (s.groups == 1) { y = (uint64_t)OcBlocks(s); g.oc_blocks_per_wg = 1; }
    else { y = (uint64_t)s.groups; g.oc_blocks_per_wg = OcBlocks(s); }
    if (x > kIndexLimit || y > kGridLimitYZ || (uint64_t)s.n > kGridLimitYZ) return false;
    g.x = (unsigned)x; g.y = (unsigned)y; g.z = (unsigned)s.n;
    return true;
}

// one past the last element offset of a view of n x c rows of `width` elements, or 0 when a stride is negative or the offset beyond 31 bits
inline uint64_t ViewExtent(int n, int c, long long sn, long long sc, long long width) {
    if (n <= 0 || c <= 0 || width <= 0 || sn < 0 || sc < 0) return 0;
    if ((uint64_t)sn > kIndexLimit || (uint64_t)sc > kIndexLimit || (uint64_t)width > kIndexLimit) return 0;
    const uint64_t last = (uint64_t)(n - 1) * (uint64_t)sn + (uint64_t)(c - 1) * (uint64_t)sc + (uint64_t)width - 1;
    return last > kIndexLimit ? 0 : last + 1;
}

// a view's strides: the channel rows at least their width apart, the batch items at least one item apart
inline bool StridesOk(int n, int c, long long sn, long long sc, long long width) {
    if (sc < width) return false;
    if (n > 1 && sn < (long long)(c - 1) * sc + width) return false;
    return sn >= 0;
}

// the device computes input positions as (lo0 + i) s - pl + k d in 32 bits: the largest one, with the tile rounded up, must fit
inline bool PositionsFit(const Shape& s) {
    const uint64_t tile = FormOf(s) == kDepthwise ? kDwPos : kTilePos;
    const uint64_t worst = ((uint64_t)s.lo + tile) * (uint64_t)s.stride + (uint64_t)s.k * (uint64_t)s.dilation + (uint64_t)s.pad_left;
    return worst <= kIndexLimit;
}

}  // namespace si_conv1d_plan

#endif  // SI_CONV1D_PLAN_H_
