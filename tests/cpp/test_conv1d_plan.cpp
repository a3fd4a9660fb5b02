// The host arithmetic of the temporal convolution kernels (simpleinfer_amd/csrc/hip/conv1d_plan.h): the form choice, torch's output length with
// an implied right pad (`same` pads, K > L), tile spans and LDS sizes, the weight image and its index, the grid limits, view extents next to
// 2^31.  Stand-alone; built with -fsanitize=address,undefined by tests/test_conv1d_cpu.py, so an overflow in a size computation or an image
// index out of its buffer ends the program.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "conv1d_plan.h"

namespace plan = si_conv1d_plan;

static int failures = 0;
#define EXPECT(cond)                                                              \
    do {                                                                          \
        if (!(cond)) {                                                            \
            std::printf("%s:%d: EXPECT(%s) failed\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                           \
        }                                                                         \
    } while (0)

static plan::Shape S(int n, int c, int l, int oc, int k, int s, int pl, int pr, int d, int g) {
    plan::Shape v;
    v.n = n; v.c = c; v.l = l; v.oc = oc; v.k = k; v.stride = s; v.dilation = d; v.pad_left = pl; v.groups = g;
    v.lo = (int)plan::OutLen(l, pl, pr, k, s, d);
    return v;
}

int main() {
    const int big = 0x7fffffff;

    // the form: plain depthwise is groups == C == OC, everything else that divides is dense
    EXPECT(plan::FormOf(S(2, 4, 16, 16, 1, 1, 0, 0, 1, 1)) == plan::kDense);
    EXPECT(plan::FormOf(S(2, 8, 40, 8, 33, 1, 16, 16, 1, 8)) == plan::kDepthwise);
    EXPECT(plan::FormOf(S(1, 4, 20, 8, 5, 1, 2, 2, 1, 4)) == plan::kDense);       // multiplier 2
    EXPECT(plan::FormOf(S(1, 1, 20, 1, 5, 1, 2, 2, 1, 1)) == plan::kDepthwise);   // one channel is its own group
    EXPECT(plan::FormOf(S(1, 6, 20, 8, 5, 1, 2, 2, 1, 4)) == plan::kNone);        // 4 divides neither 6 ...
    EXPECT(plan::FormOf(S(1, 8, 20, 6, 5, 1, 2, 2, 1, 4)) == plan::kNone);        // ... nor 6 filters
    EXPECT(plan::FormOf(S(0, 4, 16, 16, 1, 1, 0, 0, 1, 1)) == plan::kNone);
    EXPECT(plan::HalfOk(S(1, 16, 40, 32, 3, 1, 1, 1, 1, 1)) && !plan::HalfOk(S(1, 12, 40, 32, 3, 1, 1, 1, 1, 1)));
    EXPECT(plan::HalfOk(S(1, 16, 40, 32, 3, 1, 1, 1, 1, 2)) && !plan::HalfOk(S(1, 16, 40, 32, 3, 1, 1, 1, 1, 4)));
    EXPECT(plan::HalfOk(S(1, 5, 19, 5, 3, 2, 1, 1, 1, 5)));                       // depthwise has no such rule

    // torch's output length; K > L with enough padding; a window longer than the padded input gives none
    EXPECT(plan::OutLen(16, 0, 0, 1, 1, 1) == 16 && plan::OutLen(33, 2, 2, 5, 2, 1) == 17 && plan::OutLen(21, 0, 0, 3, 3, 2) == 6);
    EXPECT(plan::OutLen(8, 5, 5, 11, 1, 1) == 8 && plan::OutLen(9, 4, 4, 9, 1, 1) == 9 && plan::OutLen(8, 0, 0, 11, 1, 1) == 0);
    EXPECT(plan::OutLen(big, big, big, 1, 1, 1) == 3ll * big);                    // (64-bit inside)

    // `same`: d (K - 1) in all, the odd one on the right
    EXPECT(plan::SamePadLeft(3, 4) == 4 && plan::SamePadRight(3, 4) == 4);
    EXPECT(plan::SamePadLeft(4, 1) == 1 && plan::SamePadRight(4, 1) == 2);
    EXPECT(plan::SamePadLeft(2, 3) == 1 && plan::SamePadRight(2, 3) == 2);
    EXPECT(plan::SamePadLeft(1, 7) == 0 && plan::SamePadRight(1, 7) == 0);
    for (int k = 1; k <= 9; ++k)
        for (int d = 1; d <= 5; ++d) {
            const int pl = plan::SamePadLeft(k, d), pr = plan::SamePadRight(k, d);
            EXPECT(pl + pr == d * (k - 1) && pr - pl >= 0 && pr - pl <= 1);
            EXPECT(plan::OutLen(20, pl, pr, k, 1, d) == 20);
            plan::Shape s = S(1, 8, 20, 8, k, 1, pl, pr, d, 1);
            EXPECT(plan::ImpliedRightPad(s) == (pr > 0 ? pr : 0));                // the descriptor carries pl and lo: pr follows
        }

    // the implied right pad: the smallest pr >= 0 that gives lo, -1 for an lo no right pad gives
    {
        plan::Shape s = S(2, 8, 33, 24, 5, 2, 2, 2, 1, 1);
        EXPECT(s.lo == 17 && plan::ImpliedRightPad(s) == 2);
        s.lo = 16;                                   // what the left pad alone gives
        EXPECT(plan::ImpliedRightPad(s) == 0);
        s.lo = 15;                                   // one more window fits without any right pad: too small
        EXPECT(plan::ImpliedRightPad(s) == -1);
        s.lo = 18;                                   // a larger right pad
        EXPECT(plan::ImpliedRightPad(s) == 4);
        s.lo = 0;
        EXPECT(plan::ImpliedRightPad(s) == -1);
        plan::Shape t = S(1, 5, 8, 3, 11, 1, 5, 5, 1, 1);   // K > L
        EXPECT(t.lo == 8 && plan::ImpliedRightPad(t) == 5);
        plan::Shape u = S(1, 4, 10, 4, 3, 2, 0, 0, 1, 1);   // stride 2 leaves one position unused: pr = 0 still
        EXPECT(u.lo == 4 && plan::ImpliedRightPad(u) == 0);
        plan::Shape v = S(1, 1, big, 1, big, 1, 0, 0, 1, 1);   // K = L = 2^31 - 1
        EXPECT(v.lo == 1 && plan::ImpliedRightPad(v) == 0);
        v.lo = big;                                            // ... asked for 2^31 - 1 outputs: pr = 2^31 - 2, no overflow
        EXPECT(plan::ImpliedRightPad(v) == (int64_t)big - 1);
    }

    // spans and LDS: (tile - 1) s + (K - 1) d + 1; the fp32 pitch is 16 mod 32 and at least the span
    {
        plan::Shape s = S(32, 64, 500, 256, 33, 2, 16, 16, 1, 1);
        EXPECT(plan::Span(s, plan::kTilePos) == 63 * 2 + 32 + 1 && plan::Span(s, plan::kDwPos) == 255 * 2 + 32 + 1);
        for (uint64_t span : {1ull, 15ull, 16ull, 17ull, 48ull, 49ull, 159ull, 4096ull}) {
            const uint64_t p = plan::PitchF32(span);
            EXPECT(p >= span && p % 32 == 16 && p < span + 32);
        }
        EXPECT(plan::ChunkF32(s) == 32 && plan::LdsBytes(s, false) == 32 * plan::PitchF32(159) * 4);
        EXPECT(plan::ChunkF16(s) == 64 && plan::LdsBytes(s, true) == 159 * (64 + 8) * 2);
        plan::Shape c3 = S(1, 3, 17, 5, 3, 1, 1, 1, 1, 1);
        EXPECT(plan::ChanSteps(c3, false) == 1 && plan::ChunkF32(c3) == 4 && plan::ChanSteps(c3, true) == 1 && plan::ChunkF16(c3) == 32);
        EXPECT(plan::ChunkF16(S(1, 512, 500, 512, 1, 1, 0, 0, 1, 1)) == 128 && plan::ChunkF16(S(1, 96, 500, 8, 1, 1, 0, 0, 1, 1)) == 64);
        EXPECT(plan::ChunkF16(S(1, 128, 9000, 8, 3, 1, 0, 0, 150, 1)) == 64);    // span 364: rows of 136 halves do not fit, rows of 72 do
        plan::Shape wide = S(1, 64, 9000, 64, 3, 1, 0, 0, 1000, 1);      // span 2064: four channels of 2064 words fit, eight do not
        EXPECT(plan::Span(wide, plan::kTilePos) == 2064 && plan::PitchF32(2064) == 2064 && plan::ChunkF32(wide) == 4);
        EXPECT(plan::LdsBytes(wide, false) == 4 * 2064 * 4 && plan::LdsBytes(wide, true) == 0);   // fp16: 2064 rows of 80 bytes do not
        plan::Shape huge = S(1, 4, 100000, 4, 3, 1, 0, 0, 3000, 1);      // span 6064: not even four channels
        EXPECT(plan::ChunkF32(huge) == 0 && plan::LdsBytes(huge, false) == 0);
        plan::Shape dw = S(1, 16, 64, 16, 87, 1, 43, 43, 1, 16);
        EXPECT(plan::LdsBytes(dw, false) == 4 * (255 + 86 + 1 + 87) * 4 && plan::LdsBytes(dw, true) == plan::LdsBytes(dw, false));
        plan::Shape dwide = S(1, 16, 100000, 16, 3, 20, 0, 0, 1, 16);    // 255 * 20 + 3 positions per row, four rows: beyond 64 KB
        EXPECT(plan::LdsBytes(dwide, false) == 0);
    }

    // the weight image: every (group, tile, step, tap, lane) has its own slot inside the buffer, in order
    for (int half = 0; half < 2; ++half) {
        plan::Shape s = S(1, 24, 10, 40, 3, 1, 1, 1, 1, 1);
        const uint64_t per = half ? 8 : 1;
        EXPECT(plan::OcTiles(s) == 3 && plan::ChanSteps(s, half != 0) == (half ? 1 : 6));
        EXPECT(plan::WeightElems(s, half != 0) == 3ull * (half ? 1 : 6) * 3 * 64 * per);
        std::vector<char> seen(plan::WeightElems(s, half != 0) / per, 0);
        uint64_t expect = 0;
        for (int t = 0; t < plan::OcTiles(s); ++t)
            for (int q = 0; q < plan::ChanSteps(s, half != 0); ++q)
                for (int k = 0; k < s.k; ++k)
                    for (int lane = 0; lane < 64; ++lane) {
                        const uint64_t i = plan::WeightIndex(s, half != 0, 0, t, q, k, lane);
                        EXPECT(i == expect++);
                        seen.at(i) = 1;
                    }
        EXPECT(expect == seen.size());
        plan::Shape g3 = S(2, 12, 21, 18, 3, 3, 0, 0, 2, 3);
        EXPECT(plan::Cg(g3) == 4 && plan::Ocg(g3) == 6 && plan::OcTiles(g3) == 1 && plan::OcBlocks(g3) == 1);
        EXPECT(plan::WeightIndex(g3, false, 2, 0, 0, 2, 63) == plan::WeightElems(g3, false) - 1);
    }
    EXPECT(plan::WeightElems(S(1, 16, 64, 16, 87, 1, 43, 43, 1, 16), true) == 16 * 87);

    // the grid and its limits
    {
        plan::Grid g;
        EXPECT(plan::MakeGrid(S(2, 4, 16, 16, 1, 1, 0, 0, 1, 1), g) && g.x == 1 && g.y == 1 && g.z == 2 && g.oc_blocks_per_wg == 1);
        EXPECT(plan::MakeGrid(S(1, 3, 65, 65, 1, 1, 0, 0, 1, 1), g) && g.x == 2 && g.y == 2);
        EXPECT(plan::MakeGrid(S(2, 12, 21, 18, 3, 3, 0, 0, 2, 3), g) && g.x == 1 && g.y == 3 && g.oc_blocks_per_wg == 1);
        EXPECT(plan::MakeGrid(S(1, 2, 8, 260, 1, 1, 0, 0, 1, 2), g) && g.y == 2 && g.oc_blocks_per_wg == 3);   // 130 filters a group
        EXPECT(plan::MakeGrid(S(1, 5, 257, 5, 3, 1, 1, 1, 1, 5), g) && g.x == 2 && g.y == 2 && g.z == 1);
        EXPECT(plan::MakeGrid(S(65535, 1, 1, 1, 1, 1, 0, 0, 1, 1), g) && !plan::MakeGrid(S(65536, 1, 1, 1, 1, 1, 0, 0, 1, 1), g));
        EXPECT(plan::MakeGrid(S(1, 1, 1, 64 * 65535, 1, 1, 0, 0, 1, 1), g) && !plan::MakeGrid(S(1, 1, 1, 64 * 65535 + 1, 1, 1, 0, 0, 1, 1), g));
        EXPECT(plan::MakeGrid(S(1, 65535 * 2, 1, 65535 * 2, 1, 1, 0, 0, 1, 65535), g) && !plan::MakeGrid(S(1, 131072, 1, 131072, 1, 1, 0, 0, 1, 65536), g));
        EXPECT(plan::MakeGrid(S(1, 1, big, 1, 1, 1, 0, 0, 1, 1), g) && g.x == (1u << 23));                     // depthwise: 256 positions a tile
        EXPECT(plan::MakeGrid(S(1, 2, big, 1, 1, 1, 0, 0, 1, 1), g) && g.x == (1u << 25));
    }

    // views next to 2^31 and the stride rule
    EXPECT(plan::ViewExtent(1, 1, 0, 0, big) == (uint64_t)big && plan::ViewExtent(2, 1, (1ll << 30) + 1, 1 << 30, 1 << 30) == 0);
    EXPECT(plan::ViewExtent(2, 1, (1ll << 30) - 1, 1 << 30, 1 << 30) == (uint64_t)big && plan::ViewExtent(2, 1, 1 << 30, 1 << 30, 1 << 30) == 1ull << 31);
    EXPECT(plan::ViewExtent(1, 2, 0, 1ll << 31, 4) == 0 && plan::ViewExtent(1, 1, -1, 4, 4) == 0 && plan::ViewExtent(0, 1, 4, 4, 4) == 0);
    EXPECT(plan::ViewExtent(65535, 65535, 65535ll * 8, 8, 8) == 0);
    EXPECT(plan::StridesOk(2, 3, 30, 10, 10) && !plan::StridesOk(2, 3, 29, 10, 10) && !plan::StridesOk(1, 3, 0, 9, 10) && plan::StridesOk(1, 3, 0, 10, 10));
    EXPECT(plan::StridesOk(2, 3, 100, 40, 10) && !plan::StridesOk(2, 3, 89, 40, 10) && plan::StridesOk(2, 3, 90, 40, 10));
    // positions are computed in 32 bits on the device: refused where (lo + tile) s + K d + pl leaves them
    EXPECT(plan::PositionsFit(S(1, 4, 1000, 4, 3, 1, 1, 1, 1, 1)));
    {
        plan::Shape s = S(1, 1, big, 1, 3, 1, 1, 1, 1, 1);
        EXPECT(s.lo == big && !plan::PositionsFit(s));
        s = S(1, 1, big - 1024, 1, 3, 1, 1, 1, 1, 1);
        EXPECT(plan::PositionsFit(s));
        s = S(1, 1, big / 2, 1, 3, 2, 1, 1, 1, 1);
        s.lo = big / 2;                                        // a huge implied right pad with stride 2
        EXPECT(!plan::PositionsFit(s));
    }

    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("conv1d plan ok\n");
    return 0;
}
