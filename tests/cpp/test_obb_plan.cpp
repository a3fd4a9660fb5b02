// Stand-alone program over simpleinfer_amd/csrc/hip/obb_plan.h (built with -fsanitize=address,undefined by tests/test_obb_cpu.py): what the
// oriented-box entry refuses, and its workspace regions next to 2^31 and 2^46 -- no overflow, no overlap, the general layout untouched in front.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <limits>

#include "obb_plan.h"

namespace op = si_obb_plan;
namespace dp = si_detect_plan;

#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);    \
            std::exit(1);                                                 \
        }                                                                 \
    } while (0)

static op::Shape shape(int n, int rows, int classes, int extra, int angle_off, int layout = dp::kRows, float thr = 0.45f) {
    op::Shape s;
    s.post.n = n; s.post.rows = rows; s.post.classes = classes; s.post.extra = extra; s.post.layout = layout;
    const long long ne = 4 + (long long)classes + extra;
    s.post.ld = layout == dp::kRows ? (int)ne : rows;
    s.post.image_ld = layout == dp::kRows ? (long long)rows * ne : ne * (long long)rows;
    s.post.max_det = rows;
    s.angle_off = angle_off;
    s.nms_threshold = thr;
    return s;
}

static void check_layout(int n, int cap, int64_t nbins) {
    const op::Workspace w = op::Layout(n, cap, nbins);
    const dp::Workspace b = dp::Layout(n, cap, nbins, true);
    CHECK(w.base_total == b.total && w.offset[op::kRecord] == b.total && b.total % dp::kAlign == 0);
    const size_t nc = (size_t)n * (size_t)cap;
    size_t end = b.total;
    const size_t per[op::kRegions] = {32, 16, 4};
    for (int r = 0; r < op::kRegions; ++r) {
        CHECK(w.offset[r] == end && w.offset[r] % dp::kAlign == 0 && w.bytes[r] == per[r] * nc);
        CHECK(w.bytes[r] / per[r] == nc);      // no wrap
        end = w.offset[r] + dp::Align(w.bytes[r]);
    }
    CHECK(w.total == end && w.total > b.total);
}

int main() {
    // refusals
    CHECK(op::StatusOf(shape(2, 300, 15, 1, 0)) == dp::kOk);
    CHECK(op::StatusOf(shape(2, 300, 15, 0, 0)) == dp::kBadArg);
    CHECK(op::StatusOf(shape(2, 300, 15, 1, 1)) == dp::kBadArg && op::StatusOf(shape(2, 300, 15, 1, -1)) == dp::kBadArg);
    CHECK(op::StatusOf(shape(2, 300, 15, 4, 3)) == dp::kOk && op::AngleElement(shape(2, 300, 15, 4, 3)) == 4 + 15 + 3);
    CHECK(op::StatusOf(shape(2, 300, 15, std::numeric_limits<int>::max(), std::numeric_limits<int>::max() - 1)) == dp::kBadArg);   // ld < ne
    for (float thr : {0.0f, -0.1f, 1.0001f, std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity()})
        CHECK(op::StatusOf(shape(2, 300, 15, 1, 0, dp::kRows, thr)) == dp::kBadArg);
    CHECK(op::StatusOf(shape(2, 300, 15, 1, 0, dp::kRows, 1.0f)) == dp::kOk);
    op::Shape s = shape(2, 300, 15, 1, 0);
    s.post.box_format = dp::kXyXy;
    CHECK(op::StatusOf(s) == dp::kBadArg && op::WorkspaceBytes(s) == 0);
    CHECK(op::StatusOf(shape(65536, 4, 15, 1, 0)) == dp::kUnsupported && op::StatusOf(shape(65535, 4, 15, 1, 0)) == dp::kOk);
    CHECK(op::StatusOf(shape(2, 300, 124, 1, 0)) == dp::kUnsupported);                          // ROWS with ne = 129
    CHECK(op::StatusOf(shape(2, 300, 124, 1, 0, dp::kChannels)) == dp::kOk);
    // next to 2^31: an image of 2^31 - 1 elements is the last one served (ne = 7: rows * 7 - 1 < 2^31 - 1)
    const int rows31 = (int)(0x7fffffffLL / 7);
    CHECK(op::StatusOf(shape(1, rows31, 2, 1, 0, dp::kChannels)) == dp::kOk);
    CHECK(op::StatusOf(shape(1, rows31 + 1, 2, 1, 0, dp::kChannels)) == dp::kUnsupported);
    CHECK(op::WorkspaceBytes(shape(1, rows31, 2, 1, 0, dp::kChannels)) == op::Layout(1, rows31, 3).total);
    // next to 2^46: 7-wide rows of n * max_det detections
    s = shape(65535, 1 << 20, 2, 1, 0, dp::kChannels);
    s.post.image_ld = 1 << 23;
    s.post.max_det = (int)((1ull << 46) / 7 / 65535);
    CHECK(op::StatusOf(s) == dp::kOk);
    s.post.max_det += 1;
    CHECK(op::StatusOf(s) == dp::kUnsupported && op::WorkspaceBytes(s) == 0);
    // the regions: small, at the tile, at the largest n and cap the entry serves (n * cap < 2^47: 32 bytes each stay inside 2^52)
    check_layout(1, 1, 2);
    check_layout(2, 300, 16);
    check_layout(32, 21504, 16);
    check_layout(1, std::numeric_limits<int>::max(), 2);
    check_layout(65535, std::numeric_limits<int>::max(), 1 << 20);
    CHECK(op::Layout(0, 5, 2).total == 0 && op::Layout(5, 0, 2).total == 0);
    std::printf("obb plan ok\n");
    return 0;
}
