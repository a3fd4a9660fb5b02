// roi_interval.h -- the per-roi and per-axis arithmetic of RoIAlign (include/si_roi.h) that decides how long a loop runs and whether a roi is
// served at all.  Plain C++ for host AND device: roi_align.hip includes it for the kernel, tests/cpp/test_roi_interval.cpp compiles it for
// the CPU under AddressSanitizer and UBSan and tries the extreme values there (a roi of 1e30 px, FLT_MAX, NaN, +-Inf) before a GPU sees them.
//
// Everything is fp32 with contraction off and IEEE division, every operation exactly as written, so host and device decide the same.
//
// Termination.  With sampling_ratio <= 0 the number of samples per bin and axis, g = ceilf(roi extent / pooled size), comes from the DATA.
//   * g is compared IN FLOAT with SI_ROI_GRID_LIMIT before it becomes an int; a roi beyond it (or with a NaN / Inf anywhere) is invalid:
//     the kernel writes NaN to its rows and reads nothing.
//   * the loop over an axis runs over si_roi_axis_interval() only: the indices whose sample CAN lie in [-1, size].  The sample coordinate
//     y(iy) = start + i * bin + (iy + 0.5f) * bin / g is monotone in iy (every operation is a monotone fp32 function of iy; non-decreasing for
//     bin >= 0, non-increasing for bin < 0), so the indices that pass the inside test are one contiguous run and two binary searches over
//     the SAME expression the loop evaluates find it exactly -- at most 2 * 23 evaluations.  The run is widened by one on each side and
//     clamped to [0, g); the loop still applies the inside test to every sample, so the sum and its order are those of the full loop.
//   * Bound.  Adaptive: g = ceilf(bin), so neighbouring samples are bin / g in [0.5, 1] apart and at most
//     2 (size + 1) + 1 of them lie in [-1, size]; with one unit of rounding slack and the widening the trip count per axis and bin is
//     at most SI_ROI_TRIP_BOUND(size) = 2 size + 8.  Fixed sampling_ratio: at most sampling_ratio (<= SI_ROI_RATIO_LIMIT, checked with the
//     descriptor), a number the caller chose.
#ifndef SI_ROI_INTERVAL_H_
#define SI_ROI_INTERVAL_H_

#include <math.h>

#if defined(__HIPCC__) || defined(__HIP_DEVICE_COMPILE__)
#define SI_ROI_HD __host__ __device__ __forceinline__
#else
#define SI_ROI_HD static inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

// samples per bin and axis a roi may ask for; beyond it the roi is invalid.  (float)(g - 1) + 0.5f is exact below 2^23.
#define SI_ROI_GRID_LIMIT 4194304   /* 2^22 */
// the largest sampling_ratio a descriptor may carry
#define SI_ROI_RATIO_LIMIT 256
// trip count of an axis loop per bin, adaptive sampling (see above)
#define SI_ROI_TRIP_BOUND(size) (2 * (size) + 8)
// below this many samples the loop runs whole: nothing to find
#define SI_ROI_FULL_LOOP 8

// IEEE division on both sides
SI_ROI_HD float si_roi_div(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fdiv_rn(a, b);
#else
    return a / b;
#endif
}

SI_ROI_HD bool si_roi_finite(float v) { return v - v == 0.0f; }   // (false for NaN and +-Inf)

// one roi, as the kernel uses it
struct SiRoiBox {
    int valid;          // 0: NaN rows, nothing read
    int img;            // image index, in [0, n)
    float sw, sh;       // start of the roi on the map
    float bw, bh;       // bin size
    int gw, gh;         // samples per bin and axis, in [0, SI_ROI_GRID_LIMIT]
    float gwf, ghf;     // the same as floats (the divisor of the sample coordinate)
    float count;        // fmaxf(gh * gw, 1)
};

// roi: (image index, x1, y1, x2, y2)
SI_ROI_HD SiRoiBox si_roi_setup(const float roi[5], int n, int ph, int pw, float scale, int sampling_ratio, int aligned) {
    SiRoiBox b;
    b.valid = 0;
    b.img = 0;
    b.sw = b.sh = b.bw = b.bh = 0.0f;
    b.gw = b.gh = 0;
    b.gwf = b.ghf = 0.0f;
    b.count = 1.0f;
    const float idx = roi[0];
    // an integer in [0, n): every comparison is false for a NaN
    if (!(idx >= 0.0f && idx < (float)n && idx == floorf(idx))) return b;
    const float o = aligned ? 0.5f : 0.0f;
    const float sw = roi[1] * scale - o, sh = roi[2] * scale - o, ew = roi[3] * scale - o, eh = roi[4] * scale - o;
    if (!si_roi_finite(sw) || !si_roi_finite(sh) || !si_roi_finite(ew) || !si_roi_finite(eh)) return b;
    float rw = ew - sw, rh = eh - sh;
    if (!aligned) {
        rw = fmaxf(rw, 1.0f);
        rh = fmaxf(rh, 1.0f);
    }
    // (two finite ends of opposite sign can still be Inf apart)
    if (!si_roi_finite(rw) || !si_roi_finite(rh)) return b;
    const float bh = si_roi_div(rh, (float)ph), bw = si_roi_div(rw, (float)pw);
    float ghf = sampling_ratio > 0 ? (float)sampling_ratio : ceilf(si_roi_div(rh, (float)ph));
    float gwf = sampling_ratio > 0 ? (float)sampling_ratio : ceilf(si_roi_div(rw, (float)pw));
    if (!(ghf <= (float)SI_ROI_GRID_LIMIT) || !(gwf <= (float)SI_ROI_GRID_LIMIT)) return b;
    // a roi with x2 < x1 under `aligned` has a negative count: no sample, as the loop `iy < gh` has none
    ghf = fmaxf(ghf, 0.0f);
    gwf = fmaxf(gwf, 0.0f);
    b.valid = 1;
    b.img = (int)idx;
    b.sw = sw; b.sh = sh; b.bw = bw; b.bh = bh;
    b.ghf = ghf; b.gwf = gwf;
    b.gh = (int)ghf; b.gw = (int)gwf;
    b.count = fmaxf(ghf * gwf, 1.0f);
    return b;
}

// coordinate of sample iy of bin i on one axis: start + i * bin + (iy + 0.5f) * bin / g
SI_ROI_HD float si_roi_sample(float start, float bin, int i, int iy, float g) {
    const float base = start + (float)i * bin;
    const float t = si_roi_div(((float)iy + 0.5f) * bin, g);
    return base + t;
}

// the inside test of one axis (a sample outside adds nothing)
SI_ROI_HD bool si_roi_outside(float y, int size) { return y < -1.0f || y > (float)size; }

// [lo, hi) within [0, g): every iy whose sample of bin i passes the inside test lies in it
SI_ROI_HD void si_roi_axis_interval(float start, float bin, int i, int g, float gf, int size, int& lo, int& hi) {
    lo = 0;
    hi = g;
    if (g <= SI_ROI_FULL_LOOP) return;
    const float fs = (float)size;
    const bool up = bin >= 0.0f;
    // the first index that is no longer "before" the inside run: y >= -1 going up, y <= size going down
    int a = 0, e = g;
    while (a < e) {
        const int m = a + (e - a) / 2;
        const float y = si_roi_sample(start, bin, i, m, gf);
        const bool before = up ? y < -1.0f : y > fs;
        if (before) a = m + 1; else e = m;
    }
    const int first = a;
    // the first index behind the run: y > size going up, y < -1 going down
    e = g;
    while (a < e) {
        const int m = a + (e - a) / 2;
        const float y = si_roi_sample(start, bin, i, m, gf);
        const bool behind = up ? y > fs : y < -1.0f;
        if (behind) e = m; else a = m + 1;
    }
    lo = first > 0 ? first - 1 : 0;
    hi = a < g ? a + 1 : g;
}

#endif  // SI_ROI_INTERVAL_H_
