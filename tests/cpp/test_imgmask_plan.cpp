// Stand-alone program over simpleinfer_amd/csrc/hip/imgmask_plan.h (built with -fsanitize=address,undefined by tests/test_image_masks_cpu.py):
// what the image-size mask entry refuses, the arm rule at the LDS budget's boundary, and the limits next to 2^31, 2^46 and 65535 images.
#include <cstdio>
#include <cstdlib>
#include <limits>

#include "imgmask_plan.h"

namespace ip = si_imgmask_plan;
namespace dp = si_detect_plan;

#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);    \
            std::exit(1);                                                 \
        }                                                                 \
    } while (0)

static ip::Shape shape(int n, int mh, int mw, int nm, int oh, int ow, int max_det = 300) {
    ip::Shape s;
    s.n = n; s.mh = mh; s.mw = mw; s.nm = nm; s.proto_ld = nm; s.max_det = max_det; s.extra = nm; s.oh = oh; s.ow = ow; s.box_ld = 4;
    return s;
}

int main() {
    const int big = std::numeric_limits<int>::max();
    // refusals
    ip::Shape s = shape(32, 160, 160, 32, 640, 640);
    CHECK(ip::StatusOf(s) == dp::kOk && ip::ArmOf(s) == ip::kShared);
    for (int field = 0; field < 8; ++field) {
        ip::Shape b = s;
        int* at[] = {&b.n, &b.mh, &b.mw, &b.nm, &b.oh, &b.ow, &b.extra, &b.box_ld};
        *at[field] = field == 7 ? 3 : 0;
        CHECK(ip::StatusOf(b) == dp::kBadArg && ip::ArmOf(b) == ip::kNone);
    }
    s.proto_ld = 31; CHECK(ip::StatusOf(s) == dp::kBadArg); s.proto_ld = 32;
    s.coef_off = 1; CHECK(ip::StatusOf(s) == dp::kBadArg); s.extra = 33; CHECK(ip::StatusOf(s) == dp::kOk);
    s.coef_off = -1; CHECK(ip::StatusOf(s) == dp::kBadArg); s.coef_off = big; CHECK(ip::StatusOf(s) == dp::kBadArg); s.coef_off = 0;
    s.crop = 2; CHECK(ip::StatusOf(s) == dp::kBadArg); s.crop = ip::kCropFirst; CHECK(ip::StatusOf(s) == dp::kOk);
    s.flags = 2; CHECK(ip::StatusOf(s) == dp::kBadArg); s.flags = ip::kForceDirect; CHECK(ip::ArmOf(s) == ip::kDirect);
    s.max_det = -1; CHECK(ip::StatusOf(s) == dp::kBadArg); s.max_det = 0; CHECK(ip::StatusOf(s) == dp::kOk);
    CHECK(ip::StatusOf(shape(2, 160, 160, 65, 640, 640)) == dp::kUnsupported && ip::StatusOf(shape(2, 160, 160, 64, 640, 640)) == dp::kOk);
    CHECK(ip::StatusOf(shape(65536, 4, 4, 1, 4, 4)) == dp::kUnsupported && ip::StatusOf(shape(65535, 4, 4, 1, 4, 4)) == dp::kOk);
    // 2^31: an output plane of 2^31 - 1 bytes is the last one served, the prototypes of an image likewise
    CHECK(ip::StatusOf(shape(1, 4, 4, 1, 1, big, 1)) == dp::kOk && ip::TilesX(shape(1, 4, 4, 1, 1, big, 1)) == (1 << 24));
    CHECK(ip::StatusOf(shape(1, 4, 4, 1, 2, 1 << 30, 1)) == dp::kUnsupported && ip::StatusOf(shape(1, 4, 4, 1, big, big, 1)) == dp::kUnsupported);
    CHECK(ip::StatusOf(shape(1, 1 << 15, 1 << 15, 2, 8, 8, 1)) == dp::kUnsupported && ip::StatusOf(shape(1, 1 << 15, 1 << 15, 1, 8, 8, 1)) == dp::kOk);
    CHECK(ip::Capacity(shape(1, 1 << 15, 1 << 15, 1, 8, 8, 1)) == 4096 && ip::ArmOf(shape(1, 1 << 15, 1 << 15, 1, 8, 8, 1)) == ip::kDirect);
    // 2^46: all planes, and all box rows
    s = shape(65535, 160, 160, 32, 1024, 1024, (int)((1ull << 46) / (1024 * 1024) / 65535));
    CHECK(ip::StatusOf(s) == dp::kOk);
    s.max_det += 1; CHECK(ip::StatusOf(s) == dp::kUnsupported);
    s = shape(65535, 1, 1, 1, 1, 1, 1 << 27); s.box_ld = 8; CHECK(ip::StatusOf(s) == dp::kOk);      // 65535 * 2^27 * 8 < 2^46
    s.box_ld = 9; CHECK(ip::StatusOf(s) == dp::kUnsupported);
    // the LDS budget: a pixel costs (nm | 1) + 2 floats; the layout holds twice the nominal footprint where the budget allows and never exceeds
    // the budget or the plane
    for (int nm = 1; nm <= 64; ++nm) {
        s = shape(2, 160, 160, nm, 640, 640);
        const int cap = ip::Capacity(s);
        CHECK(ip::RowStride(nm) % 2 == 1 && ip::RowStride(nm) >= nm && ip::RowStride(nm) <= nm + 1);
        CHECK(ip::LdsBytes(s) <= ip::kLdsBudget && cap == (nm <= 43 ? 272 : (int)(ip::kLdsBudget / (4 * (ip::RowStride(nm) + 2)))) && cap >= 136);
        CHECK(ip::TileShares(cap, 1024, cap) && !ip::TileShares(cap + 1, 1024, cap) && !ip::TileShares(5, 1, cap));
        // x4: the nominal footprint is 34 x 4 pixels, held for every nm up to 64
        CHECK(ip::Span(160, 640, ip::kTileW) == 34 && ip::Span(160, 640, ip::kTileH) == 4 && ip::ArmOf(s) == ip::kShared);
        CHECK(ip::Capacity(shape(2, 5, 7, nm, 20, 28)) == 35);
    }
    // the boundary: at nm = 64 the budget holds 183 pixels; a nominal footprint of 183 shares, one of 184 does not
    CHECK(ip::Capacity(shape(1, 200, 200, 64, 8, 8)) == 183);
    CHECK(ip::ArmOf(shape(1, 3, 61, 64, 3, 61)) == ip::kShared && ip::ArmOf(shape(1, 4, 46, 64, 4, 46)) == ip::kDirect);
    // identity at 160 x 160: 129 x 9 pixels do not fit; strong down-scaling shares nothing
    CHECK(ip::ArmOf(shape(2, 160, 160, 32, 160, 160)) == ip::kDirect && ip::ArmOf(shape(2, 160, 160, 1, 40, 40)) == ip::kDirect);
    CHECK(ip::Span(big, 1, 1) == big && ip::Span(1, big, big) == 1 && ip::Span(big, big, big) == big);
    CHECK(ip::WordStores(shape(1, 4, 4, 1, 8, 8), true) && !ip::WordStores(shape(1, 4, 4, 1, 8, 9), true) && !ip::WordStores(shape(1, 4, 4, 1, 8, 8), false));
    s = shape(1, 4, 4, 32, 8, 8);
    CHECK(ip::VectorLoads(s, true) && !ip::VectorLoads(s, false));
    s.proto_ld = 34; CHECK(!ip::VectorLoads(s, true));
    std::printf("imgmask plan ok\n");
    return 0;
}
