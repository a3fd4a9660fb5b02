// detect_plan.h -- the host arithmetic of the detection post-processing entries (include/si_detect.h and the si_hip_yolo_postprocess_* pair of
// include/si_hip.h): the workspace layout, which filter form serves a descriptor, the extents a view covers and the index checks.  Pure:
// standard headers only, nothing of the device runtime, so it is exercised without a device (tests/cpp/test_detect_plan.cpp).
#ifndef SI_DETECT_PLAN_H_
#define SI_DETECT_PLAN_H_

#include <cstddef>
#include <cstdint>

namespace si_detect_plan {

constexpr uint64_t kIndexLimit = 0x7fffffffull;       // offsets inside one image are 32-bit values on the device
constexpr uint64_t kElementLimit = 1ull << 46;        // elements of a whole operand or output (offsets across images are 64-bit)
constexpr int kGridLimitY = 65535;                    // images are a grid's y extent
constexpr int kStageRows = 128;                       // prediction rows one workgroup of the staged form holds in LDS
constexpr int kStageNe = 128;                         // ... of at most this many elements each: 64 KB
constexpr int kMaskNm = 64;                           // prototypes per mask, at most
constexpr int kMaskRegNm = 32;                        // the register-resident form's prototype count

enum Layout { kRows = 0, kChannels = 1 };
enum BoxFormat { kCxCyWh = 0, kXyXy = 1 };
enum Form { kNone = 0, kRowsStaged = 1, kChannelLanes = 2 };
enum Status { kOk = 0, kBadArg = -1, kUnsupported = -2 };

struct Shape {
    int n = 0, rows = 0, classes = 0, objectness = 0, extra = 0, layout = 0, ld = 0;
    long long image_ld = 0;
    int box_format = 0, agnostic = 0, max_det = 0;
};

inline int64_t Ne(const Shape& s) { return 4 + (int64_t)s.objectness + (int64_t)s.classes + (int64_t)s.extra; }
// elements the filter reads of a row: the box, the box score, the class scores -- never the payload
inline int64_t Scan(const Shape& s) { return 4 + (int64_t)s.objectness + (int64_t)s.classes; }
// bins of the label histogram: label -1 ("no class") and every class
inline int64_t Bins(const Shape& s) { return (int64_t)s.classes + 1; }

// one past the last element offset of one image's view, or 0 when it does not fit 31 bits
inline uint64_t ImageExtent(const Shape& s) {
    if (s.rows <= 0 || s.ld <= 0 || Ne(s) <= 0) return 0;
    const uint64_t ne = (uint64_t)Ne(s);
    const uint64_t last = s.layout == kRows ? (uint64_t)(s.rows - 1) * (uint64_t)s.ld + (ne - 1)
                                            : (ne - 1) * (uint64_t)s.ld + (uint64_t)(s.rows - 1);
    return last >= kIndexLimit ? 0 : last + 1;
}

// SI_E_BADARG: sizes, enums, strides (the null pointers are the entry's own check)
inline bool Valid(const Shape& s) {
    if (s.n <= 0 || s.rows <= 0 || s.classes <= 0 || s.extra < 0 || s.max_det < 0) return false;
    if (s.objectness != 0 && s.objectness != 1) return false;
    if (s.layout != kRows && s.layout != kChannels) return false;
    if (s.box_format != kCxCyWh && s.box_format != kXyXy) return false;
    if (s.ld <= 0 || s.image_ld < 0) return false;
    if ((int64_t)s.ld < (s.layout == kRows ? Ne(s) : (int64_t)s.rows)) return false;
    // images may not interleave: an image is at least its own extent away from the next (the comparison is in 64 bits: rows * ld < 2^62)
    if (s.n > 1) {
        const uint64_t ne = (uint64_t)Ne(s);
        const uint64_t extent = s.layout == kRows ? (uint64_t)(s.rows - 1) * (uint64_t)s.ld + ne : (ne - 1) * (uint64_t)s.ld + (uint64_t)s.rows;
        if ((uint64_t)s.image_ld < extent) return false;
    }
    return true;
}

// SI_E_UNSUPPORTED of a valid shape: the grid, the staged form's LDS, the index types
inline Form FormOf(const Shape& s) {
    if (!Valid(s)) return kNone;
    if (s.n > kGridLimitY) return kNone;
    if (Ne(s) > (int64_t)kIndexLimit || ImageExtent(s) == 0) return kNone;
    // (every product below is of factors whose bounds keep it inside 64 bits: n < 2^16, image_ld <= 2^46, max_det < 2^31)
    if (s.n > 1 && ((uint64_t)s.image_ld > kElementLimit || (uint64_t)(s.n - 1) * (uint64_t)s.image_ld + ImageExtent(s) > kElementLimit)) return kNone;
    const uint64_t per_det = (uint64_t)(s.extra > 6 ? s.extra : 6);
    if ((uint64_t)s.n * (uint64_t)s.max_det > kElementLimit / per_det) return kNone;
    if (s.layout == kRows) return Ne(s) <= kStageNe ? kRowsStaged : kNone;
    return kChannelLanes;
}

inline int StatusOf(const Shape& s) { return !Valid(s) ? kBadArg : FormOf(s) == kNone ? kUnsupported : kOk; }

// bytes of LDS the staged form asks for: the scanned part of kStageRows rows
inline size_t StageBytes(const Shape& s) { return (size_t)kStageRows * (size_t)Scan(s) * sizeof(float); }

// ---- the workspace ---------------------------------------------------------------------------------------------------------------------------
// per image, cap = rows candidates, nbins = classes + 1:
//   count[n] | bin_count[n][nbins] | keep[n][cap]            zeroed at the start of every call, one memset of zero_bytes
//   gbox float4, grank | key u64 | box float4, label          candidates in arrival order, and sorted by (label, confidence)
//   sbox float4, slabel, sprob                                sorted by confidence
//   pbox float4, plabel, parea                                boxes picked so far
//   srow, drow  (the general entry alone)                     prediction row of each sorted candidate, of each stored detection
// Every region starts 256-byte aligned.  The first fifteen regions are the layout of si_hip_yolo_postprocess_workspace_bytes, byte for byte.
constexpr size_t kAlign = 256;
inline size_t Align(size_t v) { return (v + (kAlign - 1)) & ~(kAlign - 1); }

enum Region { kCount, kBinCount, kKeep, kGbox, kGrank, kKey, kBox, kLabel, kSbox, kSlabel, kSprob, kPbox, kPlabel, kParea, kSrow, kDrow, kRegions };
constexpr int kBaseRegions = kSrow;     // regions of the YOLOv5 entry's layout

struct Workspace {
    size_t offset[kRegions] = {};
    size_t bytes[kRegions] = {};        // unaligned size of each region; 0: absent
    size_t zero_bytes = 0;              // the leading bytes a call clears
    size_t total = 0;
};

inline Workspace Layout(int n, int cap, int64_t nbins, bool general) {
    Workspace w;
    if (n <= 0 || cap <= 0 || nbins <= 0) return w;
    const size_t nc = (size_t)n * (size_t)cap;
    const size_t each[kRegions] = {sizeof(int) * (size_t)n, sizeof(int) * (size_t)n * (size_t)nbins, sizeof(int) * nc,
                                   16 * nc, sizeof(int) * nc, 8 * nc, 16 * nc, sizeof(int) * nc,
                                   16 * nc, sizeof(int) * nc, sizeof(float) * nc,
                                   16 * nc, sizeof(int) * nc, sizeof(float) * nc,
                                   sizeof(int) * nc, sizeof(int) * nc};
    size_t off = 0;
    const int regions = general ? kRegions : kBaseRegions;
    for (int r = 0; r < regions; ++r) {
        w.offset[r] = off;
        w.bytes[r] = each[r];
        off += Align(each[r]);
        if (r == kKeep) w.zero_bytes = off;
    }
    w.total = off;
    return w;
}

inline size_t WorkspaceBytes(const Shape& s) { return FormOf(s) == kNone ? 0 : Layout(s.n, s.rows, Bins(s), true).total; }

// ---- masks -----------------------------------------------------------------------------------------------------------------------------------
struct MaskShape {
    int n = 0, mh = 0, mw = 0, nm = 0, proto_ld = 0, max_det = 0, extra = 0, coef_off = 0;
};

enum MaskForm { kMaskNone = 0, kMaskGeneric = 1, kMaskRegisters = 2 };

inline bool MaskValid(const MaskShape& s) {
    return s.n > 0 && s.mh > 0 && s.mw > 0 && s.nm > 0 && s.proto_ld >= s.nm && s.max_det >= 0 && s.extra > 0 && s.coef_off >= 0 &&
           (int64_t)s.coef_off + (int64_t)s.nm <= (int64_t)s.extra;
}

// protos_aligned: the prototypes' address is a multiple of 16
inline MaskForm MaskFormOf(const MaskShape& s, bool protos_aligned) {
    if (!MaskValid(s)) return kMaskNone;
    if (s.n > kGridLimitY || s.nm > kMaskNm) return kMaskNone;
    const uint64_t pixels = (uint64_t)s.mh * (uint64_t)s.mw;
    if (pixels * (uint64_t)s.proto_ld > kIndexLimit) return kMaskNone;                       // offsets inside one image's prototypes
    if ((uint64_t)s.n * (uint64_t)s.max_det > kElementLimit / pixels) return kMaskNone;      // mask bytes (pixels < 2^31: no product overflows)
    if ((uint64_t)s.n * (uint64_t)s.max_det > kElementLimit / (uint64_t)s.extra) return kMaskNone;
    return s.nm == kMaskRegNm && s.proto_ld % 4 == 0 && protos_aligned ? kMaskRegisters : kMaskGeneric;
}

inline int MaskStatusOf(const MaskShape& s) { return !MaskValid(s) ? kBadArg : MaskFormOf(s, false) == kMaskNone ? kUnsupported : kOk; }

// four mask bytes per store: whole planes are a multiple of four bytes and start on one
inline bool MaskWordStores(const MaskShape& s, bool masks_aligned4) { return s.mw % 4 == 0 && masks_aligned4; }

}  // namespace si_detect_plan

#endif  // SI_DETECT_PLAN_H_
