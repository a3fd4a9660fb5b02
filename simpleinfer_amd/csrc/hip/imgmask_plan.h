// imgmask_plan.h -- the host arithmetic of the image-size instance masks (include/si_imgmask.h): what the entry refuses, the output tile, the
// LDS a workgroup of the shared arm gets, and which arm a descriptor takes.  Pure: standard headers only, nothing of the device runtime, so it
// is exercised without a device (tests/cpp/test_imgmask_plan.cpp).
#ifndef SI_IMGMASK_PLAN_H_
#define SI_IMGMASK_PLAN_H_

#include <cstddef>
#include <cstdint>

#include "detect_plan.h"

namespace si_imgmask_plan {

namespace base = si_detect_plan;

// The output tile of a workgroup: 128 x 8 pixels, 256 lanes of 4 consecutive bytes each.  32 lanes store one whole 128-byte line of a row (a
// 64-wide tile would leave every row's store half a line), and at the usual x4 the tile's prototype footprint is 34 x 4 pixels: 18 KB at
// nm = 32.  8 rows, not 16: the footprint of a taller tile grows by whole prototype rows of 34 pixels, that of a wider one by single columns.
constexpr int kTileW = 128, kTileH = 8, kThreads = 256, kLaneBytes = 4;
constexpr size_t kLdsBudget = 48u * 1024u;   // of the 160 KB of a CU: three workgroups of the shared arm stay resident
constexpr int kShareFactor = 4;              // a footprint of more than 4 pixels per output pixel shares nothing: the direct arm does less

enum Crop { kCropAfter = 0, kCropFirst = 1 };
enum Flags { kForceDirect = 1 };
enum Arm { kNone = 0, kShared = 1, kDirect = 2 };

struct Shape {
    int n = 0, mh = 0, mw = 0, nm = 0, proto_ld = 0, max_det = 0, extra = 0, coef_off = 0, oh = 0, ow = 0, box_ld = 0, crop = 0, flags = 0;
};

inline base::MaskShape MaskPart(const Shape& s) {
    base::MaskShape m;
    m.n = s.n; m.mh = s.mh; m.mw = s.mw; m.nm = s.nm; m.proto_ld = s.proto_ld; m.max_det = s.max_det; m.extra = s.extra; m.coef_off = s.coef_off;
    return m;
}

inline bool Valid(const Shape& s) {
    return base::MaskValid(MaskPart(s)) && s.oh > 0 && s.ow > 0 && s.box_ld >= 4 && (s.crop == kCropAfter || s.crop == kCropFirst) &&
           (s.flags & ~kForceDirect) == 0;
}

// the limits of detect_masks on the prototypes and the payload; an output plane inside 31 bits, all planes and all boxes inside 2^46
inline bool Supported(const Shape& s) {
    if (!Valid(s) || base::MaskFormOf(MaskPart(s), false) == base::kMaskNone) return false;
    const uint64_t plane = (uint64_t)s.oh * (uint64_t)s.ow;
    if (plane > base::kIndexLimit) return false;
    const uint64_t dets = (uint64_t)s.n * (uint64_t)s.max_det;        // < 2^47
    return dets <= base::kElementLimit / plane && dets <= base::kElementLimit / (uint64_t)s.box_ld;
}

inline int StatusOf(const Shape& s) { return !Valid(s) ? base::kBadArg : !Supported(s) ? base::kUnsupported : base::kOk; }

// LDS row of one footprint pixel's prototypes, in floats.  Odd, so that lane l reading word l * stride + k meets bank (l * stride + k) mod B,
// and multiplying by an odd number permutes the residues of B = 32 and of B = 64: the lanes of a pass meet distinct banks for every k.
constexpr int RowStride(int nm) { return nm | 1; }

// source pixels `out` output pixels of an axis touch at most when `in` source pixels map onto `total` output pixels: ceil(out * in / total) + 2
inline int64_t Span(int in, int total, int out) {
    const int64_t v = ((int64_t)out * (int64_t)in + (int64_t)total - 1) / (int64_t)total + 2;
    return v < (int64_t)in ? v : (int64_t)in;
}

// the footprint of a whole tile under the nominal geometry, the whole plane onto OH x OW
inline int64_t NominalFootprint(const Shape& s) {
    const int tw = s.ow < kTileW ? s.ow : kTileW, th = s.oh < kTileH ? s.oh : kTileH;
    return Span(s.mw, s.ow, tw) * Span(s.mh, s.oh, th);
}

// footprint pixels a workgroup's LDS holds: a row of prototypes and one float in each of the two logit tiles per pixel.  What the budget
// allows, but never more than the plane or than twice the nominal footprint: asking for the whole budget would keep workgroups off a CU that
// has room for them (x4 at nm = 32: 38 KB for 272 pixels, four workgroups where 48 KB leave three).
inline int Capacity(const Shape& s) {
    uint64_t cap = kLdsBudget / (sizeof(float) * (size_t)(RowStride(s.nm) + 2));
    const uint64_t plane = (uint64_t)s.mh * (uint64_t)s.mw, twice = 2 * (uint64_t)NominalFootprint(s);
    cap = cap < plane ? cap : plane;
    return (int)(cap < twice ? cap : twice);
}

inline size_t LdsBytes(const Shape& s) { return sizeof(float) * (size_t)Capacity(s) * (size_t)(RowStride(s.nm) + 2); }

// the rule a tile is held to, on the device with its own footprint and here with the nominal one: it fits, and it shares
constexpr bool TileShares(int64_t foot, int64_t live, int capacity) { return foot <= (int64_t)capacity && foot <= (int64_t)kShareFactor * live; }

// The arm of a launch.  The geometry is on the device, so the choice is made for the nominal one, the whole plane onto OH x OW; a tile whose
// own record breaks the rule runs the direct arm's code inside the shared kernel.
inline Arm ArmOf(const Shape& s) {
    if (!Supported(s)) return kNone;
    if (s.flags & kForceDirect) return kDirect;
    const int tw = s.ow < kTileW ? s.ow : kTileW, th = s.oh < kTileH ? s.oh : kTileH;
    // (held against the budget alone: Capacity is cut to twice this footprint)
    const uint64_t budget = kLdsBudget / (sizeof(float) * (size_t)(RowStride(s.nm) + 2));
    return TileShares(NominalFootprint(s), (int64_t)tw * th, (int)budget) ? kShared : kDirect;
}

inline int64_t TilesX(const Shape& s) { return ((int64_t)s.ow + kTileW - 1) / kTileW; }
inline int64_t TilesY(const Shape& s) { return ((int64_t)s.oh + kTileH - 1) / kTileH; }

// packed stores: every row of every plane starts on a 4-byte boundary
inline bool WordStores(const Shape& s, bool masks_aligned4) { return s.ow % kLaneBytes == 0 && masks_aligned4; }
// 16-byte loads while staging
inline bool VectorLoads(const Shape& s, bool protos_aligned16) { return s.nm % 4 == 0 && s.proto_ld % 4 == 0 && protos_aligned16; }

}  // namespace si_imgmask_plan

#endif  // SI_IMGMASK_PLAN_H_
