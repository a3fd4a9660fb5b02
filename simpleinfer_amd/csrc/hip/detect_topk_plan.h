// detect_topk_plan.h -- the host arithmetic of the top-k detection post-processing (include/si_topk.h): the refusals, the chunking, the radix
// levels and the workspace layout.  Pure: standard headers only, nothing of the device runtime, so it is exercised without a device
// (tests/cpp/test_topk_plan.cpp).
#ifndef SI_DETECT_TOPK_PLAN_H_
#define SI_DETECT_TOPK_PLAN_H_

#include <cstddef>
#include <cstdint>

namespace si_topk_plan {

constexpr uint64_t kIndexLimit = 0x7fffffffull;       // flat indices and offsets inside one image are 31-bit values
constexpr uint64_t kElementLimit = 1ull << 46;        // elements of a whole operand or output
constexpr int kGridLimitY = 65535;                    // images are a grid's y extent
constexpr int kThreads = 256;                         // lanes of every workgroup
constexpr int kChunkRows = 256;                       // prediction rows of one chunk: a lane owns a row
constexpr int kSlabClasses = 32;                      // SI_DETECT_ROWS: classes staged in LDS at a time, kChunkRows x (kSlabClasses + 1) words
constexpr int kLevels = 3;                            // radix levels over the 32 key bits
constexpr int kBins = 2048;                           // bins of a level's histogram (the last level uses 1024 of them)
constexpr int kMaxDet = 1024;                         // keys the final LDS sort holds
constexpr int kStateWords = 8;                        // per image: what the select kernels hand on (State below)

enum Layout { kRows = 0, kChannels = 1 };
enum BoxFormat { kCxCyWh = 0, kXyXy = 1 };
enum Status { kOk = 0, kBadArg = -1, kUnsupported = -2 };

// key bits below level l and the bits level l bins: 11 | 11 | 10
constexpr int LevelShift(int level) { return level == 0 ? 21 : level == 1 ? 10 : 0; }
constexpr int LevelBits(int level) { return level == 2 ? 10 : 11; }

// words of an image's state
enum State { kTotal = 0, kTake = 1, kPrefix = 2, kAbove = 3 };
//   kTotal   kept candidates (counts[b]);  kTake  min(kTotal, max_det): the keys to store
//   kPrefix  the key bits fixed so far, in place (after the last level: the threshold key T)
//   kAbove   keys above every key under the prefix (after the last level: gt = #{key > T}; need = kTake - gt)

struct Shape {
    int n = 0, rows = 0, classes = 0, extra = 0, layout = 0, ld = 0;
    long long image_ld = 0;
    int box_format = 0, multi_label = 0, max_det = 0;
};

inline int64_t Ne(const Shape& s) { return 4 + (int64_t)s.classes + (int64_t)s.extra; }

// one past the last element offset of one image's view (64-bit: rows, ld < 2^31 and ne < 2^33)
inline uint64_t ImageExtent(const Shape& s) {
    const uint64_t ne = (uint64_t)Ne(s);
    return s.layout == kRows ? (uint64_t)(s.rows - 1) * (uint64_t)s.ld + ne : (ne - 1) * (uint64_t)s.ld + (uint64_t)s.rows;
}

inline bool Valid(const Shape& s) {
    if (s.n <= 0 || s.rows <= 0 || s.classes <= 0 || s.extra < 0 || s.max_det < 0) return false;
    if (s.layout != kRows && s.layout != kChannels) return false;
    if (s.box_format != kCxCyWh && s.box_format != kXyXy) return false;
    if (s.multi_label != 0 && s.multi_label != 1) return false;
    if (s.ld <= 0 || s.image_ld < 0) return false;
    if ((int64_t)s.ld < (s.layout == kRows ? Ne(s) : (int64_t)s.rows)) return false;
    if (s.n > 1 && (uint64_t)s.image_ld < ImageExtent(s)) return false;      // images may not interleave
    return true;
}

// candidates of one image = one past the largest flat index
inline uint64_t Candidates(const Shape& s) { return s.multi_label ? (uint64_t)s.rows * (uint64_t)s.classes : (uint64_t)s.rows; }

inline int StatusOf(const Shape& s) {
    if (!Valid(s)) return kBadArg;
    if (s.max_det > kMaxDet || s.n > kGridLimitY) return kUnsupported;
    // the flat index of the multi-label form bounds both modes: one descriptor is either servable or not, whatever multi_label says
    if ((uint64_t)s.rows * (uint64_t)s.classes > kIndexLimit) return kUnsupported;
    if (ImageExtent(s) > kIndexLimit) return kUnsupported;
    if (s.n > 1 && ((uint64_t)s.image_ld > kElementLimit || (uint64_t)(s.n - 1) * (uint64_t)s.image_ld + ImageExtent(s) > kElementLimit))
        return kUnsupported;
    const uint64_t per_det = (uint64_t)(s.extra > 6 ? s.extra : 6);
    if ((uint64_t)s.n * (uint64_t)s.max_det > kElementLimit / per_det) return kUnsupported;
    return kOk;
}

// chunks of kChunkRows rows: a grid's x extent (rows < 2^31: at most 2^23)
inline int Chunks(int rows) { return (int)(((int64_t)rows + kChunkRows - 1) / kChunkRows); }
inline int ChunkFirstRow(int chunk) { return chunk * kChunkRows; }     // chunk < 2^23: inside int
inline int ChunkRows(int rows, int chunk) {
    const int64_t left = (int64_t)rows - (int64_t)chunk * kChunkRows;
    return left <= 0 ? 0 : left < kChunkRows ? (int)left : kChunkRows;
}

// ---- the workspace -----------------------------------------------------------------------------------------------------------------------------
//   keys  u64 [n][max_det]          the selected keys in arrival order: {ordered score << 32 | ~f}
//   hist  u32 [n][kLevels][kBins]   | slot u32 [n]      cleared at the start of every call by topk_clear_kernel, one range of zero_words
//   state u32 [n][kStateWords]
//   ties  u32 [n][chunks]           keys equal to T in each chunk
// Every region starts 256-byte aligned.
constexpr size_t kAlign = 256;
inline size_t Align(size_t v) { return (v + (kAlign - 1)) & ~(kAlign - 1); }

enum Region { kKeys, kHist, kSlot, kStateRegion, kTies, kRegions };

struct Workspace {
    size_t offset[kRegions] = {};
    size_t bytes[kRegions] = {};
    size_t zero_words = 0;      // 32-bit words from offset[kHist] on
    size_t total = 0;
};

inline Workspace LayoutOf(int n, int rows, int max_det) {
    Workspace w;
    if (n <= 0 || rows <= 0 || max_det < 0) return w;
    const size_t each[kRegions] = {8 * (size_t)n * (size_t)max_det, 4 * (size_t)n * kLevels * kBins, 4 * (size_t)n,
                                   4 * (size_t)n * kStateWords, 4 * (size_t)n * (size_t)Chunks(rows)};
    size_t off = 0;
    for (int r = 0; r < kRegions; ++r) {
        w.offset[r] = off;
        w.bytes[r] = each[r];
        off += r == kHist ? each[r] : Align(each[r]);      // slot follows hist without a gap (4 * n * 6144 is a multiple of 256 anyway)
    }
    w.zero_words = (each[kHist] + each[kSlot]) / 4;
    w.total = off;
    return w;
}

inline size_t WorkspaceBytes(const Shape& s) { return StatusOf(s) != kOk ? 0 : LayoutOf(s.n, s.rows, s.max_det).total; }

}  // namespace si_topk_plan

#endif  // SI_DETECT_TOPK_PLAN_H_
