// The termination arithmetic of RoIAlign (simpleinfer_amd/csrc/hip/roi_interval.h, the header the kernel includes) on the CPU, under
// AddressSanitizer and UBSan with the float-cast check: this program is where the extreme boxes are tried before a GPU sees them.
//   1. map extents 1..12 x pooled sizes 1..7 x a sweep of roi starts and sizes (negative, x2 < x1, zero, up to 1e3) x both `aligned` x adaptive
//      and fixed sampling: si_roi_axis_interval contains every index whose sample passes the inside test -- brute force over the full loop is
//      the judge --, and with adaptive sampling its length is within SI_ROI_TRIP_BOUND(size)
//   2. roi sizes 1e6, 1e9, 1e30 and FLT_MAX: the box is invalid or the trip count is within the bound, and no float -> int conversion of the
//      setup, the interval or the taps overflows (UBSan aborts the program if one does)
//   3. NaN, +-Inf, and image indices that are no integer in [0, n) take the invalid path
// Built by tests/test_roi_cpu.py with -ffp-contract=off: the header's arithmetic has no fused operation.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "roi_interval.h"

static int failures = 0;
static long long checked_axes = 0, checked_samples = 0, searched_axes = 0;
#define EXPECT(cond)                                                              \
    do {                                                                          \
        if (!(cond)) {                                                            \
            if (failures < 20) std::printf("%s:%d: EXPECT(%s) failed\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                           \
        }                                                                         \
    } while (0)

// the taps of an inside sample as the kernel forms them: the conversion must be defined and the indices inside the map
static void CheckTaps(float y, int size) {
    y = fmaxf(y, 0.0f);
    int lo = (int)y;
    int hi;
    if (lo >= size - 1) {
        lo = hi = size - 1;
    } else {
        hi = lo + 1;
    }
    EXPECT(lo >= 0 && lo < size && hi >= 0 && hi < size);
}

// one axis of one bin: the interval against the full loop (brute: 0 skips the full loop, for counts too large to walk more than once)
static void CheckAxis(float start, float bin, int i, int g, float gf, int size, bool adaptive, bool brute) {
    int lo = -1, hi = -1;
    si_roi_axis_interval(start, bin, i, g, gf, size, lo, hi);
    ++checked_axes;
    if (g > SI_ROI_FULL_LOOP) ++searched_axes;
    EXPECT(0 <= lo && lo <= hi && hi <= g);
    if (adaptive) EXPECT(hi - lo <= SI_ROI_TRIP_BOUND(size));
    if (failures) return;
    if (brute) {
        for (int iy = 0; iy < g; ++iy) {
            const float y = si_roi_sample(start, bin, i, iy, gf);
            ++checked_samples;
            if (si_roi_outside(y, size)) continue;
            EXPECT(lo <= iy && iy < hi);
            CheckTaps(y, size);
        }
    } else {
        for (int iy = lo; iy < hi; ++iy) {
            const float y = si_roi_sample(start, bin, i, iy, gf);
            if (!si_roi_outside(y, size)) CheckTaps(y, size);
        }
        // the neighbours of the interval and a scatter of indices outside it are outside the map
        const int probes[] = {0, lo - 2, lo - 1, hi, hi + 1, g / 3, g / 2, g - 1};
        for (int iy : probes) {
            if (iy < 0 || iy >= g || (iy >= lo && iy < hi)) continue;
            EXPECT(si_roi_outside(si_roi_sample(start, bin, i, iy, gf), size));
        }
    }
}

static void CheckBox(const float roi[5], int n, int h, int w, int ph, int pw, float scale, int ratio, int aligned, bool brute) {
    const SiRoiBox b = si_roi_setup(roi, n, ph, pw, scale, ratio, aligned);
    if (!b.valid) return;
    EXPECT(b.img >= 0 && b.img < n && b.gh >= 0 && b.gh <= SI_ROI_GRID_LIMIT && b.gw >= 0 && b.gw <= SI_ROI_GRID_LIMIT && b.count >= 1.0f);
    if (ratio > 0) EXPECT(b.gh == ratio && b.gw == ratio);
    for (int i = 0; i < ph; ++i) CheckAxis(b.sh, b.bh, i, b.gh, b.ghf, h, ratio <= 0, brute);
    for (int j = 0; j < pw; ++j) CheckAxis(b.sw, b.bw, j, b.gw, b.gwf, w, ratio <= 0, brute);
}

static bool Valid(float idx, float x1, float y1, float x2, float y2, float scale = 1.0f, int ratio = 0, int aligned = 0, int n = 2) {
    const float roi[5] = {idx, x1, y1, x2, y2};
    return si_roi_setup(roi, n, 7, 7, scale, ratio, aligned).valid != 0;
}

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    // ---- 1. the sweep: x and y share the code, so the map is size x size and the box is the same on both axes
    const float starts[] = {-1e3f, -40.5f, -7.25f, -1.0f, -0.5f, 0.0f, 0.3f, 2.75f, 6.0f, 11.5f, 13.0f, 250.0f, 1e3f};
    const float sizes[] = {-1e3f, -30.0f, -3.5f, -0.001f, 0.0f, 0.001f, 0.5f, 1.0f, 2.5f, 7.0f, 12.0f, 33.3f, 100.0f, 1e3f};
    const int ratios[] = {-1, 0, 1, 2, 3, 12, 37};
    for (int size = 1; size <= 12; ++size)
        for (int pooled = 1; pooled <= 7; ++pooled)
            for (float s : starts)
                for (float len : sizes)
                    for (int ratio : ratios)
                        for (int aligned = 0; aligned < 2; ++aligned) {
                            const float roi[5] = {0.0f, s, s, s + len, s + len};
                            CheckBox(roi, 1, size, size, pooled, pooled, 1.0f, ratio, aligned, true);
                            const float scaled[5] = {0.0f, s * 4.0f, s * 4.0f, (s + len) * 4.0f, (s + len) * 4.0f};
                            if (ratio <= 0) CheckBox(scaled, 1, size, size, pooled, pooled, 0.25f, ratio, aligned, true);
                        }
    std::printf("sweep: %lld axes (%lld through the search), %lld samples walked, %d failures\n", checked_axes, searched_axes, checked_samples, failures);
    EXPECT(searched_axes > 100000);

    // ---- 2. huge boxes
    const float huge[] = {1e6f, 1e9f, 1e30f, FLT_MAX};
    const float hstarts[] = {0.0f, -3.0f, -5e5f, -1e9f, -1e30f, -FLT_MAX, 5.0f, 1e9f};
    int valid_huge = 0;
    for (float len : huge)
        for (float s : hstarts)
            for (int ratio : {-1, 0, 2, 256})
                for (int aligned = 0; aligned < 2; ++aligned)
                    for (float scale : {1.0f, 0.0625f, 16.0f})
                        for (int pooled : {1, 7}) {
                            const float roi[5] = {1.0f, s, s, s + len, s + len};
                            const SiRoiBox b = si_roi_setup(roi, 2, pooled, pooled, scale, ratio, aligned);
                            valid_huge += b.valid;
                            // a count beyond the limit never reaches an int
                            if (ratio <= 0 && len * scale / (float)pooled > 1.01f * (float)SI_ROI_GRID_LIMIT && s + len > s) EXPECT(!b.valid);
                            // (the full loop is walked where it is short; elsewhere the interval's neighbours are probed)
                            CheckBox(roi, 2, 9, 11, pooled, pooled, scale, ratio, aligned, b.valid && b.gh <= 100000 && b.gw <= 100000);
                        }
    EXPECT(valid_huge > 0);
    // 1e6 px over one bin with adaptive sampling is served: 1e6 samples per axis, of which at most 2 size + 8 are visited
    {
        const float roi[5] = {0.0f, -5e5f, -5e5f, 5e5f, 5e5f};
        const SiRoiBox b = si_roi_setup(roi, 1, 1, 1, 1.0f, 0, 0);
        EXPECT(b.valid && b.gh == 1000000 && b.gw == 1000000);
        int lo, hi;
        si_roi_axis_interval(b.sh, b.bh, 0, b.gh, b.ghf, 9, lo, hi);
        EXPECT(hi - lo <= SI_ROI_TRIP_BOUND(9) && hi - lo >= 9);
        CheckBox(roi, 1, 9, 11, 1, 1, 1.0f, 0, 0, true);
    }
    EXPECT(!Valid(0.0f, 0.0f, 0.0f, 1e9f, 1e9f));                   // 1e9 samples: beyond the limit
    EXPECT(!Valid(0.0f, 0.0f, 0.0f, 1e30f, 1e30f));
    EXPECT(!Valid(0.0f, 0.0f, 0.0f, FLT_MAX, FLT_MAX));
    EXPECT(!Valid(0.0f, -FLT_MAX, 0.0f, FLT_MAX, 1.0f, 1.0f, 2));     // the ends are finite, their distance is not
    EXPECT(!Valid(0.0f, 0.0f, 0.0f, FLT_MAX, 1.0f, 16.0f, 2));       // the scaled end is not finite
    EXPECT(Valid(0.0f, 0.0f, 0.0f, 1e30f, 1e30f, 1.0f, 2));          // fixed sampling: two samples per axis, wherever they fall
    EXPECT(Valid(0.0f, 0.0f, 0.0f, 0.0f, 0.0f) && Valid(1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0, 1));   // a zero-padded slot

    // ---- 3. the invalid path
    for (float bad : {nan, inf, -inf}) {
        EXPECT(!Valid(bad, 1.0f, 1.0f, 2.0f, 2.0f));
        EXPECT(!Valid(0.0f, bad, 1.0f, 2.0f, 2.0f) && !Valid(0.0f, 1.0f, bad, 2.0f, 2.0f) && !Valid(0.0f, 1.0f, 1.0f, bad, 2.0f) &&
               !Valid(0.0f, 1.0f, 1.0f, 2.0f, bad));
        EXPECT(!Valid(0.0f, bad, 1.0f, 2.0f, 2.0f, 1.0f, 2, 1) && !Valid(0.0f, 1.0f, 1.0f, 2.0f, bad, 1.0f, 2, 1));
        EXPECT(!Valid(0.0f, 1.0f, 1.0f, 2.0f, 2.0f, bad));            // the scale
    }
    for (float idx : {-1.0f, 2.0f, 0.5f, 1.5f, -0.25f, 1e9f, -1e30f}) EXPECT(!Valid(idx, 1.0f, 1.0f, 2.0f, 2.0f));
    EXPECT(Valid(0.0f, 1.0f, 1.0f, 2.0f, 2.0f) && Valid(1.0f, 1.0f, 1.0f, 2.0f, 2.0f) && Valid(-0.0f, 1.0f, 1.0f, 2.0f, 2.0f));

    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("roi interval ok: %lld axes, %lld samples\n", checked_axes, checked_samples);
    return 0;
}
