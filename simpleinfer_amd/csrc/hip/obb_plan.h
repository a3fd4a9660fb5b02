// obb_plan.h -- the host arithmetic of the oriented-box post-processing entry (include/si_obb.h): what it refuses, and the workspace regions it
// appends behind the general entry's layout (detect_plan.h, which stays byte for byte what it is).  Pure: standard headers only, nothing of
// the device runtime, so it is exercised without a device (tests/cpp/test_obb_plan.cpp).
#ifndef SI_OBB_PLAN_H_
#define SI_OBB_PLAN_H_

#include <cstddef>
#include <cstdint>

#include "detect_plan.h"

namespace si_obb_plan {

namespace base = si_detect_plan;

constexpr int kTile = 1024;          // records of one LDS tile of the suppression kernel
constexpr int kRecordBytes = 32;     // {cx, cy, A, B | C, max(AB - C^2, 0), label, 0}: two 16-byte words
constexpr int kRawBytes = 16;        // {w, h, angle, confidence}: what the store needs beside the centre
constexpr int kThreads = 256;        // candidates of one workgroup

struct Shape {
    base::Shape post;                // the general entry's fields, box_format fixed to centre + size
    int angle_off = 0;
    float nms_threshold = 0.0f;
};

inline bool Valid(const Shape& s) {
    if (!base::Valid(s.post) || s.post.box_format != base::kCxCyWh) return false;
    if (s.post.extra < 1 || s.angle_off < 0 || s.angle_off >= s.post.extra) return false;
    return s.nms_threshold > 0.0f && s.nms_threshold <= 1.0f;      // false for a NaN
}

// the limits of the general entry, and the 7-wide output rows inside 2^46 elements
inline bool Supported(const Shape& s) {
    if (!Valid(s) || base::FormOf(s.post) == base::kNone) return false;
    return (uint64_t)s.post.n * (uint64_t)s.post.max_det <= base::kElementLimit / 7;
}

inline int StatusOf(const Shape& s) { return !Valid(s) ? base::kBadArg : !Supported(s) ? base::kUnsupported : base::kOk; }

// element offset of the angle inside a prediction row
inline int64_t AngleElement(const Shape& s) { return base::Scan(s.post) + (int64_t)s.angle_off; }

// ---- the workspace: the general entry's regions, then per image and candidate slot (cap = rows)
//   record 32 bytes    confidence-ordered {cx, cy, A, B, C, det, label, 0}: what a pair test reads
//   raw    16 bytes    {w, h, angle, confidence} in the same order: what the store reads
//   keep   4 bytes     1 / 0 per confidence rank, every rank below count[b] written by the suppression kernel (nothing to clear)
// Every region starts 256-byte aligned (the general layout's total is a multiple of 256).
enum Region { kRecord, kRaw, kKeep, kRegions };

struct Workspace {
    size_t offset[kRegions] = {};
    size_t bytes[kRegions] = {};
    size_t base_total = 0;           // si_detect_plan::Layout(n, cap, nbins, true).total
    size_t total = 0;
};

inline Workspace Layout(int n, int cap, int64_t nbins) {
    Workspace w;
    const base::Workspace b = base::Layout(n, cap, nbins, true);
    if (b.total == 0) return w;
    const size_t nc = (size_t)n * (size_t)cap;       // n < 2^16, cap < 2^31: 32 * nc < 2^52
    const size_t each[kRegions] = {(size_t)kRecordBytes * nc, (size_t)kRawBytes * nc, sizeof(int) * nc};
    size_t off = b.total;
    w.base_total = b.total;
    for (int r = 0; r < kRegions; ++r) {
        w.offset[r] = off;
        w.bytes[r] = each[r];
        off += base::Align(each[r]);
    }
    w.total = off;
    return w;
}

inline size_t WorkspaceBytes(const Shape& s) { return Supported(s) ? Layout(s.post.n, s.post.rows, base::Bins(s.post)).total : 0; }

}  // namespace si_obb_plan

#endif  // SI_OBB_PLAN_H_
