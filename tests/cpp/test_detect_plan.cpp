// The host arithmetic of the detection post-processing entries (simpleinfer_amd/csrc/hip/detect_plan.h): the workspace regions (disjoint,
// aligned, the YOLOv5 entry's byte count unchanged), the form choice, the refusals, sizes next to 2^31 and n = 65535.  Stand-alone; built with
// -fsanitize=address,undefined by tests/test_detect_post_cpu.py, so an overflow in a size computation ends the program.
#include <cstdint>
#include <cstdio>

#include "detect_plan.h"

namespace plan = si_detect_plan;

static int failures = 0;
#define EXPECT(cond)                                                              \
    do {                                                                          \
        if (!(cond)) {                                                            \
            std::printf("%s:%d: EXPECT(%s) failed\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                           \
        }                                                                         \
    } while (0)

static plan::Shape S(int n, int rows, int classes, int objectness, int extra, int layout, int max_det = -1, int ld = 0, long long image_ld = -1) {
    plan::Shape s;
    s.n = n; s.rows = rows; s.classes = classes; s.objectness = objectness; s.extra = extra; s.layout = layout;
    const long long ne = 4ll + objectness + classes + extra;
    s.ld = ld ? ld : (layout == plan::kRows ? (int)ne : rows);
    s.image_ld = image_ld >= 0 ? image_ld : (layout == plan::kRows ? (long long)rows * s.ld : ne * s.ld);
    s.box_format = plan::kCxCyWh;
    s.max_det = max_det < 0 ? rows : max_det;
    return s;
}

// the byte count si_hip_yolo_postprocess_workspace_bytes has always returned, restated: fifteen regions, each rounded up to 256 bytes
static size_t OldBytes(size_t n, size_t cap, size_t nbins) {
    auto a = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t nc = n * cap;
    return a(4 * n) + a(4 * n * nbins) + a(4 * nc) + a(16 * nc) + a(4 * nc) + a(8 * nc) + a(16 * nc) + a(4 * nc) + a(16 * nc) + a(4 * nc) + a(4 * nc) +
           a(16 * nc) + a(4 * nc) + a(4 * nc);
}

static void CheckLayout(int n, int cap, int64_t nbins) {
    for (int general = 0; general < 2; ++general) {
        const plan::Workspace w = plan::Layout(n, cap, nbins, general != 0);
        const int regions = general ? plan::kRegions : plan::kBaseRegions;
        size_t end = 0;
        for (int r = 0; r < regions; ++r) {
            EXPECT(w.bytes[r] > 0);
            EXPECT(w.offset[r] % plan::kAlign == 0);
            EXPECT(w.offset[r] >= end);                 // disjoint, in order
            end = w.offset[r] + w.bytes[r];
        }
        EXPECT(end <= w.total && w.total % plan::kAlign == 0);
        EXPECT(w.zero_bytes == w.offset[plan::kGbox]);   // count, bin_count and keep are what a call clears
        if (!general) {
            EXPECT(w.total == OldBytes((size_t)n, (size_t)cap, (size_t)nbins));
            EXPECT(w.bytes[plan::kSrow] == 0 && w.bytes[plan::kDrow] == 0);
        } else {
            const plan::Workspace base = plan::Layout(n, cap, nbins, false);
            for (int r = 0; r < plan::kBaseRegions; ++r) EXPECT(w.offset[r] == base.offset[r] && w.bytes[r] == base.bytes[r]);
            EXPECT(w.offset[plan::kSrow] == base.total);
            EXPECT(w.bytes[plan::kSrow] == sizeof(int) * (size_t)n * (size_t)cap && w.bytes[plan::kDrow] == w.bytes[plan::kSrow]);
        }
    }
}

int main() {
    const int big = 0x7fffffff;

    // the workspace
    CheckLayout(1, 1, 2);
    CheckLayout(32, 25200, 81);
    CheckLayout(3, 129, 1265);
    CheckLayout(65535, 7, 3);
    CheckLayout(65535, 40000, 81);        // 2.6e9 candidates: sizes are 64-bit
    CheckLayout(2, big, 2);
    EXPECT(plan::Layout(0, 5, 2, true).total == 0 && plan::Layout(5, 0, 2, true).total == 0 && plan::Layout(5, 5, 0, false).total == 0);
    EXPECT(plan::Layout(32, 25200, 81, false).total == OldBytes(32, 25200, 81));

    // element counts
    EXPECT(plan::Ne(S(1, 10, 80, 1, 0, plan::kRows)) == 85 && plan::Scan(S(1, 10, 80, 0, 32, plan::kRows)) == 84 && plan::Ne(S(1, 10, 80, 0, 32, plan::kRows)) == 116);
    EXPECT(plan::Bins(S(1, 10, 80, 1, 0, plan::kRows)) == 81);
    EXPECT(plan::Ne(S(1, 10, big, 1, big, plan::kChannels)) == 2ll * big + 5);       // (64-bit inside)

    // forms
    EXPECT(plan::FormOf(S(2, 8400, 80, 0, 32, plan::kRows)) == plan::kRowsStaged);
    EXPECT(plan::FormOf(S(2, 8400, 80, 0, 32, plan::kChannels)) == plan::kChannelLanes);
    EXPECT(plan::FormOf(S(2, 100, 123, 1, 0, plan::kRows)) == plan::kRowsStaged);     // ne = 128
    EXPECT(plan::StatusOf(S(2, 100, 124, 1, 0, plan::kRows)) == plan::kUnsupported);  // ne = 129
    EXPECT(plan::StatusOf(S(2, 100, 92, 0, 33, plan::kRows)) == plan::kUnsupported);  // ... by the payload
    EXPECT(plan::FormOf(S(2, 100, 1264, 0, 32, plan::kChannels)) == plan::kChannelLanes);   // no limit on ne
    EXPECT(plan::StageBytes(S(2, 100, 123, 1, 0, plan::kRows)) == 65536 && plan::StageBytes(S(2, 100, 80, 0, 32, plan::kRows)) == 128 * 84 * 4);

    // SI_E_BADARG
    EXPECT(plan::StatusOf(S(0, 10, 3, 1, 0, plan::kRows)) == plan::kBadArg && plan::StatusOf(S(-1, 10, 3, 1, 0, plan::kRows)) == plan::kBadArg);
    EXPECT(plan::StatusOf(S(1, 0, 3, 1, 0, plan::kRows)) == plan::kBadArg && plan::StatusOf(S(1, 10, 0, 1, 0, plan::kRows)) == plan::kBadArg);
    EXPECT(plan::StatusOf(S(1, 10, 3, 2, 0, plan::kRows)) == plan::kBadArg && plan::StatusOf(S(1, 10, 3, -1, 0, plan::kRows)) == plan::kBadArg);
    EXPECT(plan::StatusOf(S(1, 10, 3, 1, -1, plan::kRows)) == plan::kBadArg && plan::StatusOf(S(1, 10, 3, 1, 0, 2)) == plan::kBadArg);
    EXPECT(plan::StatusOf(S(1, 10, 3, 1, 0, plan::kRows, 0)) == plan::kOk);           // max_det 0 is a size
    {
        plan::Shape s = S(1, 10, 3, 1, 0, plan::kRows);
        s.max_det = -1;
        EXPECT(plan::StatusOf(s) == plan::kBadArg);
        s.max_det = 1; s.box_format = 2;
        EXPECT(plan::StatusOf(s) == plan::kBadArg);
        s.box_format = plan::kXyXy;
        EXPECT(plan::StatusOf(s) == plan::kOk);
    }
    EXPECT(plan::StatusOf(S(2, 10, 3, 1, 0, plan::kRows, -1, 7)) == plan::kBadArg);             // ld < ne = 8
    EXPECT(plan::StatusOf(S(2, 10, 3, 1, 0, plan::kRows, -1, 8)) == plan::kOk && plan::StatusOf(S(2, 10, 3, 1, 0, plan::kRows, -1, 11)) == plan::kOk);
    EXPECT(plan::StatusOf(S(2, 10, 3, 1, 0, plan::kChannels, -1, 9)) == plan::kBadArg);         // ld < rows
    EXPECT(plan::StatusOf(S(2, 10, 3, 1, 0, plan::kChannels, -1, 13)) == plan::kOk);
    EXPECT(plan::StatusOf(S(2, 10, 3, 1, 0, plan::kRows, -1, 11, 9 * 11 + 7)) == plan::kBadArg);   // images interleave: one short of the extent
    EXPECT(plan::StatusOf(S(2, 10, 3, 1, 0, plan::kRows, -1, 11, 9 * 11 + 8)) == plan::kOk);
    EXPECT(plan::StatusOf(S(2, 10, 3, 1, 0, plan::kChannels, -1, 13, 7 * 13 + 9)) == plan::kBadArg);
    EXPECT(plan::StatusOf(S(2, 10, 3, 1, 0, plan::kChannels, -1, 13, 7 * 13 + 10)) == plan::kOk);
    EXPECT(plan::StatusOf(S(1, 10, 3, 1, 0, plan::kRows, -1, 8, 0)) == plan::kOk);               // one image: image_ld is not used

    // SI_E_UNSUPPORTED: the grid, 31 bits inside an image, 2^46 elements in all
    EXPECT(plan::StatusOf(S(65535, 4, 3, 1, 0, plan::kRows)) == plan::kOk && plan::StatusOf(S(65536, 4, 3, 1, 0, plan::kRows)) == plan::kUnsupported);
    EXPECT(plan::WorkspaceBytes(S(65535, 4, 3, 1, 0, plan::kRows)) == plan::Layout(65535, 4, 4, true).total);
    EXPECT(plan::WorkspaceBytes(S(65536, 4, 3, 1, 0, plan::kRows)) == 0 && plan::WorkspaceBytes(S(0, 4, 3, 1, 0, plan::kRows)) == 0);
    {
        // rows * ld next to 2^31: (rows - 1) * 8 + 7 is the last offset
        const int rows_ok = (big - 8) / 8 + 1;       // last offset = (rows - 1) * 8 + 7 <= 2^31 - 2
        EXPECT(plan::ImageExtent(S(1, rows_ok, 3, 1, 0, plan::kRows, 1)) == (uint64_t)(rows_ok - 1) * 8 + 8);
        EXPECT(plan::StatusOf(S(1, rows_ok, 3, 1, 0, plan::kRows, 1)) == plan::kOk);
        EXPECT(plan::ImageExtent(S(1, rows_ok + 1, 3, 1, 0, plan::kRows, 1)) == 0);
        EXPECT(plan::StatusOf(S(1, rows_ok + 1, 3, 1, 0, plan::kRows, 1)) == plan::kUnsupported);
        EXPECT(plan::StatusOf(S(1, big, 3, 1, 0, plan::kChannels, 1)) == plan::kUnsupported);    // 8 channels of 2^31 - 1 rows
        EXPECT(plan::StatusOf(S(1, big / 8, 3, 1, 0, plan::kChannels, 1)) == plan::kOk);
        EXPECT(plan::StatusOf(S(1, 2, big - 8, 1, 0, plan::kChannels, 1)) == plan::kUnsupported);
        EXPECT(plan::StatusOf(S(1, 1, big, 1, big, plan::kChannels, 1)) == plan::kUnsupported);  // ne itself beyond 31 bits
    }
    EXPECT(plan::StatusOf(S(65535, 1 << 20, 3, 1, 0, plan::kRows, 1, 8, 1ll << 31)) == plan::kUnsupported);   // 2^47 elements across the images
    EXPECT(plan::StatusOf(S(32768, 1 << 20, 3, 1, 0, plan::kRows, 1, 8, 1ll << 30)) == plan::kOk);
    EXPECT(plan::StatusOf(S(4096, 1 << 20, 3, 0, 1 << 10, plan::kChannels, 1 << 25)) == plan::kUnsupported);   // the extras output: 2^47 elements
    EXPECT(plan::StatusOf(S(2, 1 << 20, 3, 0, 32, plan::kChannels, big)) == plan::kOk);           // max_det larger than rows is a size like another
    EXPECT(plan::StatusOf(S(65535, 1 << 20, 3, 0, big - 7, plan::kChannels, big, 1 << 20, 1ll << 62)) == plan::kUnsupported);   // every factor at its largest

    // masks
    {
        plan::MaskShape m;
        m.n = 2; m.mh = 160; m.mw = 160; m.nm = 32; m.proto_ld = 32; m.max_det = 300; m.extra = 32; m.coef_off = 0;
        EXPECT(plan::MaskFormOf(m, true) == plan::kMaskRegisters && plan::MaskFormOf(m, false) == plan::kMaskGeneric);
        EXPECT(plan::MaskWordStores(m, true) && !plan::MaskWordStores(m, false));
        m.proto_ld = 33;
        EXPECT(plan::MaskFormOf(m, true) == plan::kMaskGeneric);
        m.proto_ld = 31;
        EXPECT(plan::MaskStatusOf(m) == plan::kBadArg);
        m.proto_ld = 64; m.nm = 64; m.extra = 64;
        EXPECT(plan::MaskFormOf(m, true) == plan::kMaskGeneric);
        m.nm = 65; m.proto_ld = 65; m.extra = 65;
        EXPECT(plan::MaskStatusOf(m) == plan::kUnsupported);
        m.nm = 32; m.proto_ld = 32; m.extra = 51; m.coef_off = 19;
        EXPECT(plan::MaskStatusOf(m) == plan::kOk);
        m.coef_off = 20;
        EXPECT(plan::MaskStatusOf(m) == plan::kBadArg);
        m.coef_off = -1;
        EXPECT(plan::MaskStatusOf(m) == plan::kBadArg);
        m.coef_off = 0; m.mw = 7;
        EXPECT(!plan::MaskWordStores(m, true));
        m.mw = 160; m.max_det = 0;
        EXPECT(plan::MaskStatusOf(m) == plan::kOk);
        m.max_det = -1;
        EXPECT(plan::MaskStatusOf(m) == plan::kBadArg);
        m.max_det = 300; m.n = 65536;
        EXPECT(plan::MaskStatusOf(m) == plan::kUnsupported);
        m.n = 65535;
        EXPECT(plan::MaskStatusOf(m) == plan::kOk);
        m.n = 1; m.mh = 46341; m.mw = 46341; m.nm = 1; m.proto_ld = 1; m.extra = 1;    // 46341^2 > 2^31
        EXPECT(plan::MaskStatusOf(m) == plan::kUnsupported);
        m.mh = 8192; m.mw = 8192; m.proto_ld = 32;                                      // 2^26 pixels of 32: 2^31 elements
        EXPECT(plan::MaskStatusOf(m) == plan::kUnsupported);
        m.proto_ld = 31;
        EXPECT(plan::MaskStatusOf(m) == plan::kOk);
        m.n = 65535; m.max_det = big;                                                   // mask bytes beyond 2^46
        EXPECT(plan::MaskStatusOf(m) == plan::kUnsupported);
    }

    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("detect plan ok\n");
    return 0;
}
