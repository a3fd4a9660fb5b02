// The host arithmetic of the top-k detection post-processing: detect_topk_plan.h (simpleinfer_amd/csrc/hip: the refusals, the chunking next to
// 2^31, the radix levels, the workspace layout).  Stand-alone (plain C++ headers only); built with -fsanitize=address,undefined by
// tests/test_topk_cpu.py.
#include <cstdio>
#include <initializer_list>

#include "detect_topk_plan.h"

namespace plan = si_topk_plan;

static int failures = 0;
#define EXPECT(cond) \
    do { if (!(cond)) { std::printf("%s:%d: EXPECT(%s) failed\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static plan::Shape Dense(int n, int rows, int classes, int extra = 0, int layout = plan::kRows, int max_det = 300) {
    plan::Shape s;
    s.n = n; s.rows = rows; s.classes = classes; s.extra = extra; s.layout = layout; s.max_det = max_det; s.multi_label = 1;
    const long long ne = 4LL + classes + extra;
    s.ld = (int)(layout == plan::kRows ? ne : rows);
    s.image_ld = layout == plan::kRows ? (long long)rows * s.ld : ne * s.ld;
    return s;
}

int main() {
    // the levels tile the 32 key bits, and a level's bins fit the histogram
    EXPECT(plan::LevelShift(0) + plan::LevelBits(0) == 32 && plan::LevelShift(1) + plan::LevelBits(1) == plan::LevelShift(0));
    EXPECT(plan::LevelShift(2) == 0 && plan::LevelBits(2) == plan::LevelShift(1));
    for (int l = 0; l < plan::kLevels; ++l) EXPECT((1 << plan::LevelBits(l)) <= plan::kBins && (1 << plan::LevelBits(l)) % plan::kThreads == 0);

    // refusals
    EXPECT(plan::StatusOf(Dense(32, 8400, 80, 0, plan::kChannels)) == plan::kOk && plan::StatusOf(Dense(1, 1, 1)) == plan::kOk);
    for (int field = 0; field < 4; ++field)
        for (int bad : {0, -3}) {
            plan::Shape s = Dense(2, 100, 3);
            (field == 0 ? s.n : field == 1 ? s.rows : field == 2 ? s.classes : s.ld) = bad;
            EXPECT(plan::StatusOf(s) == plan::kBadArg && plan::WorkspaceBytes(s) == 0);
        }
    for (int field = 0; field < 6; ++field) {
        plan::Shape s = Dense(2, 100, 3, 2, field % 2);
        if (field == 0) s.extra = -1; else if (field == 1) s.max_det = -1; else if (field == 2) s.layout = 2; else if (field == 3) s.box_format = 2;
        else if (field == 4) s.multi_label = 2; else s.ld -= 1;
        EXPECT(plan::StatusOf(s) == plan::kBadArg);
    }
    plan::Shape meet = Dense(2, 100, 3);
    meet.image_ld -= 1;
    EXPECT(plan::StatusOf(meet) == plan::kBadArg);
    meet.n = 1;
    EXPECT(plan::StatusOf(meet) == plan::kOk);                 // a single image has no neighbour to meet
    EXPECT(plan::StatusOf(Dense(1, 10, 3, 0, 0, plan::kMaxDet)) == plan::kOk && plan::StatusOf(Dense(1, 10, 3, 0, 0, plan::kMaxDet + 1)) == plan::kUnsupported);
    EXPECT(plan::StatusOf(Dense(65535, 10, 3)) == plan::kOk && plan::StatusOf(Dense(65536, 10, 3)) == plan::kUnsupported);

    // next to 2^31: the flat index (rows * classes) and the image's extent
    plan::Shape wide = Dense(1, 1 << 20, 2047, 0, plan::kChannels);      // 2^31 - 2^20 flat indices, extent (2047 + 4) * 2^20 > 2^31
    EXPECT(plan::Candidates(wide) == 2146435072ull && plan::StatusOf(wide) == plan::kUnsupported);
    plan::Shape flat = Dense(1, 1 << 20, 2040, 0, plan::kChannels);      // extent 2044 * 2^20 < 2^31
    EXPECT(plan::ImageExtent(flat) == 2143289344ull && plan::StatusOf(flat) == plan::kOk);
    flat.multi_label = 0;
    EXPECT(plan::Candidates(flat) == (1ull << 20) && plan::StatusOf(flat) == plan::kOk);
    EXPECT(plan::StatusOf(Dense(1, 1 << 16, 1 << 15)) == plan::kUnsupported);                              // 2^31 flat indices
    plan::Shape tall = Dense(1, 2147483647, 1);
    tall.multi_label = 0;
    EXPECT(plan::StatusOf(tall) == plan::kUnsupported);                                                    // extent 5 * (2^31 - 1)
    EXPECT(plan::Chunks(2147483647) == (1 << 23) && plan::ChunkRows(2147483647, (1 << 23) - 1) == 255 && plan::ChunkRows(2147483647, 1 << 23) == 0);
    EXPECT(plan::ChunkFirstRow((1 << 23) - 1) == 2147483392);
    EXPECT(plan::Chunks(1) == 1 && plan::Chunks(256) == 1 && plan::Chunks(257) == 2 && plan::ChunkRows(257, 1) == 1 && plan::ChunkRows(256, 0) == 256);

    // the workspace: aligned regions in order, never a multiple of rows * classes
    const plan::Workspace w = plan::LayoutOf(32, 8400, 300);
    for (int r = 0; r < plan::kRegions; ++r) EXPECT(w.offset[r] % plan::kAlign == 0 || r == plan::kSlot);
    for (int r = 1; r < plan::kRegions; ++r) EXPECT(w.offset[r] >= w.offset[r - 1] + w.bytes[r - 1]);
    EXPECT(w.offset[plan::kSlot] == w.offset[plan::kHist] + w.bytes[plan::kHist] && w.zero_words == 32u * (3 * 2048 + 1));
    EXPECT(w.total >= w.offset[plan::kTies] + w.bytes[plan::kTies] && w.bytes[plan::kTies] == 4u * 32 * 33 && w.bytes[plan::kKeys] == 8u * 32 * 300);
    EXPECT(w.total < 1000000 && plan::WorkspaceBytes(Dense(32, 8400, 80)) == w.total && plan::WorkspaceBytes(Dense(32, 8400, 8000)) == w.total);
    EXPECT(plan::LayoutOf(1, 10, 0).bytes[plan::kKeys] == 0 && plan::LayoutOf(1, 10, 0).total > 0);
    const plan::Workspace big = plan::LayoutOf(65535, 2147483647, plan::kMaxDet);                          // no product leaves 64 bits
    EXPECT(big.bytes[plan::kTies] == 4ull * 65535 * (1 << 23) && big.total > big.bytes[plan::kTies]);

    if (failures == 0) std::printf("topk plan ok\n");
    return failures == 0 ? 0 : 1;
}
