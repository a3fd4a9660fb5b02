// The host arithmetic of the cross-correlation kernels (simpleinfer_amd/csrc/hip/xcorr_plan.h): the form choice, torch's output extent with an
// implied far pad (`same` / `valid`, kernels larger than the image), view extents and stride rules next to 2^31, tile counts and the grid limits.
// Stand-alone; built with -fsanitize=address,undefined by tests/test_xcorr_cpu.py, so an overflow in a size computation ends the program.
#include <cstdint>
#include <cstdio>

#include "xcorr_plan.h"

namespace plan = si_xcorr_plan;

static int failures = 0;
#define EXPECT(cond)                                                              \
    do {                                                                          \
        if (!(cond)) {                                                            \
            std::printf("%s:%d: EXPECT(%s) failed\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                           \
        }                                                                         \
    } while (0)

// a square-parameter shape with torch's output extent for the pads (p0, p1) on both axes
static plan::Shape S(int n, int c, int h, int w, int oc, int kh, int kw, int s, int p0, int p1, int d, int g, int per_sample = 0) {
    plan::Shape v;
    v.n = n; v.c = c; v.h = h; v.w = w; v.oc = oc; v.kh = kh; v.kw = kw; v.stride_h = v.stride_w = s; v.dilation_h = v.dilation_w = d;
    v.pad_top = v.pad_left = p0; v.groups = g; v.per_sample = per_sample;
    v.ho = (int)plan::OutExtent(h, p0, p1, kh, s, d);
    v.wo = (int)plan::OutExtent(w, p0, p1, kw, s, d);
    return v;
}

int main() {
    const int big = 0x7fffffff;

    // the form: groups == C == OC is depthwise (one channel and one filter included), every other groups == 1 dense, nothing else
    EXPECT(plan::FormOf(S(1, 16, 22, 22, 1, 6, 6, 1, 0, 0, 1, 1)) == plan::kDense);
    EXPECT(plan::FormOf(S(2, 64, 31, 31, 64, 7, 7, 1, 0, 0, 1, 64)) == plan::kDepthwise);
    EXPECT(plan::FormOf(S(1, 1, 9, 9, 1, 3, 3, 1, 0, 0, 1, 1)) == plan::kDepthwise);
    EXPECT(plan::FormOf(S(1, 1, 9, 9, 3, 3, 3, 1, 0, 0, 1, 1)) == plan::kDense);
    EXPECT(plan::FormOf(S(1, 8, 9, 9, 8, 3, 3, 1, 0, 0, 1, 2)) == plan::kNone);        // groups 2 of 8
    EXPECT(plan::FormOf(S(1, 8, 9, 9, 16, 3, 3, 1, 0, 0, 1, 8)) == plan::kNone);       // multiplier 2
    EXPECT(plan::FormOf(S(0, 8, 9, 9, 8, 3, 3, 1, 0, 0, 1, 1)) == plan::kNone);
    EXPECT(plan::FormOf(S(2, 8, 9, 9, 8, 3, 3, 1, 0, 0, 1, 8, 1)) == plan::kDepthwise);
    EXPECT(plan::FormOf(S(2, 8, 9, 9, 4, 3, 3, 1, 0, 0, 1, 1, 1)) == plan::kNone);     // per-sample filters have no dense form
    EXPECT(plan::HalfOk(S(1, 16, 9, 9, 3, 3, 3, 1, 0, 0, 1, 1)) && !plan::HalfOk(S(1, 12, 9, 9, 3, 3, 3, 1, 0, 0, 1, 1)));
    EXPECT(plan::HalfOk(S(1, 7, 9, 9, 7, 3, 3, 1, 0, 0, 1, 7)) && !plan::HalfOk(S(1, 8, 9, 9, 8, 3, 3, 1, 0, 0, 1, 2)));
    {
        plan::Shape s = S(1, 8, 9, 9, 8, 3, 3, 1, 0, 0, 1, 1);
        s.pad_top = -1;
        EXPECT(!plan::Positive(s) && plan::FormOf(s) == plan::kNone);
        s.pad_top = 0; s.dilation_w = 0;
        EXPECT(!plan::Positive(s));
    }

    // torch's output extent; `valid`; a kernel larger than the image with and without enough padding
    EXPECT(plan::OutExtent(22, 0, 0, 6, 1, 1) == 17 && plan::OutExtent(31, 0, 0, 7, 1, 1) == 25 && plan::OutExtent(16, 1, 1, 3, 2, 1) == 8);
    EXPECT(plan::OutExtent(3, 2, 2, 5, 1, 1) == 3 && plan::OutExtent(3, 0, 0, 5, 1, 1) == 0 && plan::OutExtent(6, 0, 0, 6, 1, 1) == 1);
    EXPECT(plan::OutExtent(big, big, big, 1, 1, 1) == 3ll * big);                      // (64-bit inside)
    EXPECT(plan::ImpliedFarPad(3, 2, 3, 5, 1, 1) == 2 && plan::ImpliedFarPad(3, 0, 1, 5, 1, 1) == 2 && plan::ImpliedFarPad(3, 0, 0, 5, 1, 1) == -1);

    // `same`: d (K - 1) in all, the odd one on the far side; the descriptor carries the near pad and the output extent, the far pad follows
    EXPECT(plan::SamePadNear(4, 1) == 1 && plan::SamePadFar(4, 1) == 2 && plan::SamePadNear(2, 1) == 0 && plan::SamePadFar(2, 1) == 1);
    EXPECT(plan::SamePadNear(3, 2) == 2 && plan::SamePadFar(3, 2) == 2 && plan::SamePadNear(1, 7) == 0 && plan::SamePadFar(1, 7) == 0);
    for (int k = 1; k <= 9; ++k)
        for (int d = 1; d <= 5; ++d) {
            const int p0 = plan::SamePadNear(k, d), p1 = plan::SamePadFar(k, d);
            EXPECT(p0 + p1 == d * (k - 1) && p1 - p0 >= 0 && p1 - p0 <= 1);
            EXPECT(plan::OutExtent(20, p0, p1, k, 1, d) == 20);
            EXPECT(plan::ImpliedFarPad(20, p0, 20, k, 1, d) == p1);
        }
    // an extent torch's formula gives for no far pad: too small for the near pad alone, or zero
    {
        plan::Shape s = S(2, 8, 33, 33, 24, 5, 5, 2, 2, 2, 1, 1);
        EXPECT(s.ho == 17 && plan::ExtentsOk(s));
        s.ho = 16; EXPECT(plan::ExtentsOk(s));      // what the near pad alone gives
        s.ho = 18; EXPECT(plan::ExtentsOk(s));      // a larger far pad
        s.ho = 15; EXPECT(!plan::ExtentsOk(s));
        s.ho = 17; s.wo = 15; EXPECT(!plan::ExtentsOk(s));
    }

    // view extents next to 2^31: the last element offset must fit 31 bits
    EXPECT(plan::ViewExtent(2, 3, 4, 5, 60, 20, 5, 1) == 120);
    EXPECT(plan::ViewExtent(2, 3, 4, 5, 100, 30, 7, 1) == 100 + 60 + 21 + 4 + 1);
    EXPECT(plan::ViewExtent(1, 1, 1, big, 0, 0, 0, 1) == (uint64_t)big);
    EXPECT(plan::ViewExtent(1, 1, 2, big, 0, 0, 1, 1) == (uint64_t)big + 1 && plan::ViewExtent(1, 1, 3, big, 0, 0, 1, 1) == 0);
    EXPECT(plan::ViewExtent(3, 1, 1, 1, 1 << 30, 0, 0, 1) == 0 && plan::ViewExtent(2, 1, 1, 1, 1 << 30, 0, 0, 1) == (1ull << 30) + 1);
    EXPECT(plan::ViewExtent(2, 1, 1, 1, (long long)big + 1, 0, 0, 1) == 0 && plan::ViewExtent(1, 2, 2, 2, 0, -4, 2, 1) == 0);
    EXPECT(plan::ViewExtent(65535, 65535, 2, 2, 65535ll * 4, 4, 2, 1) == 0);           // (the products are 64-bit)
    EXPECT(plan::ViewExtent(0, 1, 1, 1, 1, 1, 1, 1) == 0);
    // a shared depthwise filter: image stride 0, the channels kh kw ld apart
    EXPECT(plan::ViewExtent(1, 7, 7, 64, 0, 7, 1, 49) == 63 * 49 + 48 + 1);
    // the strides of a written view nest
    EXPECT(plan::NestedStrides(2, 3, 4, 5, 60, 20, 5) && plan::NestedStrides(2, 3, 4, 5, 200, 40, 8));
    EXPECT(!plan::NestedStrides(2, 3, 4, 5, 60, 20, 4) && !plan::NestedStrides(2, 3, 4, 5, 60, 19, 5) && !plan::NestedStrides(2, 3, 4, 5, 59, 20, 5));
    EXPECT(plan::NestedStrides(1, 1, 4, 5, 0, 0, 5) && !plan::NestedStrides(1, 1, 4, 5, -1, 0, 5));

    // tiles and the grid
    {
        plan::Shape s = S(3, 8, 7, 9, 70, 3, 3, 1, 1, 1, 1, 1);
        plan::Grid g;
        EXPECT(plan::OutPixels(s) == 63 && plan::OcTiles(s) == 5 && plan::OcBlocks(s) == 2 && plan::ChanSteps(s, false) == 1 && plan::ChanSteps(s, true) == 1);
        EXPECT(plan::MakeGrid(s, false, g) && g.x == 1 && g.y == 2 && g.z == 3);
        s = S(1, 4, 5, 13, 16, 3, 3, 1, 1, 1, 1, 1);
        EXPECT(plan::OutPixels(s) == 65 && plan::MakeGrid(s, false, g) && g.x == 2 && g.y == 1);
        s = S(2, 12, 9, 9, 12, 3, 3, 1, 1, 1, 1, 12);
        EXPECT(plan::DwChanRuns(s, false) == 3 && plan::DwChanRuns(s, true) == 2);
        EXPECT(plan::MakeGrid(s, false, g) && g.x == (81 * 3 + 255) / 256 && g.y == 1 && g.z == 2);
        EXPECT(plan::MakeGrid(s, true, g) && g.x == 1);
        // limits: the batch and the filter blocks beyond a grid's y / z, the depthwise items beyond 31 bits
        s = S(65536, 1, 1, 1, 3, 1, 1, 1, 0, 0, 1, 1);
        EXPECT(!plan::MakeGrid(s, false, g));
        s = S(65535, 1, 1, 1, 3, 1, 1, 1, 0, 0, 1, 1);
        EXPECT(plan::MakeGrid(s, false, g) && g.z == 65535);
        s = S(1, 1, 1, 1, 65535 * 64 + 1, 1, 1, 1, 0, 0, 1, 1);
        EXPECT(!plan::MakeGrid(s, false, g));
        s = S(1, 4096, 2048, 2048, 4096, 1, 1, 1, 0, 0, 1, 4096);
        EXPECT(!plan::MakeGrid(s, false, g));                                         // 2^22 pixels x 2^10 runs
        s = S(1, 4096, 1024, 1024, 4096, 1, 1, 1, 0, 0, 1, 4096);
        EXPECT(plan::MakeGrid(s, false, g) && g.x == 1u << 22);
        s = S(1, 8, 9, 9, 8, 3, 3, 1, 0, 0, 1, 2);
        EXPECT(!plan::MakeGrid(s, false, g));
    }
    // the device's 32-bit coordinates
    {
        plan::Shape s = S(1, 1, 1 << 20, 4, 1, 3, 3, 1, 1, 1, 1, 1);
        EXPECT(plan::PositionsFit(s));
        s.stride_h = 1 << 12;
        EXPECT(!plan::PositionsFit(s));
        s.stride_h = 1; s.dilation_w = big;
        EXPECT(!plan::PositionsFit(s));
    }
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("xcorr plan ok\n");
    return 0;
}
