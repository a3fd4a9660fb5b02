/*
 * si_roi.h -- C-ABI of torchvision.ops.RoIAlign / roi_align (the semantics of torchvision's CPU kernel; no reference counterpart).  The
 * symbols live in libsi_hip.so beside those of include/si_hip.h; a header of its own as include/si_grid.h and include/si_deform.h have.
 *
 * Operands:
 *     x     [n, h, w, c]      NHWC, pixels in_ld elements apart, fp32 or fp16 storage
 *     rois  [k, 5]            ALWAYS fp32, rows rois_ld >= 5 elements apart; row r is (image index, x1, y1, x2, y2).  fp16 cannot hold
 *                             pixel coordinates (at 2048 px its ulp is 1 px), so the boxes keep fp32 also beside half features
 *     out   [k, ph, pw, c]    NHWC, pixels out_ld elements apart, the storage type of x
 *
 * The rule: fp32 throughout, no operation contracted, IEEE division, every operation exactly as written.
 *   per roi, o = aligned ? 0.5f : 0.0f:
 *     sw = x1 * scale - o, sh = y1 * scale - o, ew = x2 * scale - o, eh = y2 * scale - o;  rw = ew - sw, rh = eh - sh;
 *     without `aligned`: rw = fmaxf(rw, 1), rh = fmaxf(rh, 1);  bh = rh / ph, bw = rw / pw;
 *     gh = sampling_ratio > 0 ? sampling_ratio : ceilf(rh / ph), gw likewise (a negative value counts as 0: no sample);
 *     count = fmaxf(gh * gw, 1), in float
 *   per sample -- bin (i, j), then iy < gh (outer loop), then ix < gw:
 *     y = sh + i * bh + (iy + 0.5f) * bh / gh          (that is (sh + i * bh) + (((iy + 0.5f) * bh) / gh)),  x likewise
 *     y < -1 || y > h || x < -1 || x > w: the sample adds nothing and nothing is read for it; otherwise
 *     y = fmaxf(y, 0); yl = (int)y; if (yl >= h - 1) { yl = yh = h - 1; y = yl; } else yh = yl + 1;  ly = y - yl, hy = 1 - ly;  x likewise
 *     w1 = hy * hx, w2 = hy * lx, w3 = ly * hx, w4 = ly * lx;  v1 = x[yl][xl], v2 = x[yl][xh], v3 = x[yh][xl], v4 = x[yh][xh]
 *     acc = acc + (((w1 * v1 + w2 * v2) + w3 * v3) + w4 * v4)       four multiplications and four additions, none of them fused
 *   result: acc / count, rounded once to the storage type
 *
 * Termination.  With sampling_ratio <= 0 the loop length comes from the data.  gh and gw are compared in float with SI_ROI_GRID_LIMIT
 * (2^22) before the conversion to int, and each axis loop runs only over the index interval whose samples can lie in [-1, size]
 * (csrc/hip/roi_interval.h: exact by monotonicity, widened by one on each side, clamped to [0, g)); the inside test still runs per
 * sample, so the sum and its order are those of the full loop.  Trip count per axis and bin: at most 2 size + 8 (adaptive), at most
 * sampling_ratio <= 256 (fixed).  A roi 1e9 px wide costs what a roi as wide as the map costs.
 *
 * Invalid rois.  The image index is not an integer in [0, n); one of the four scaled coordinates, rw or rh is not finite; gh or gw exceeds
 * SI_ROI_GRID_LIMIT.  Every element of such a roi's output is NaN and nothing of x is read (the convention of si_grid.h for "nothing is
 * read"; torchvision's behaviour is undefined there).  A zero-padded slot (0, 0, 0, 0, 0) is valid and follows the rule.
 *
 * Kernel.  A gather bound by HBM / L2; no LDS, no scratch, no atomics, no workspace.  A lane owns one channel vector of one output bin
 * (r, i, j), channel vectors fastest across lanes; a capped grid strides over the items in one consecutive run per XCD.  Vector widths:
 * fp32 4 | 1, fp16 8 | 4 | 2 | 1, the widest that c, both pixel strides and both pointers allow; every arm computes the same bits.  Names:
 *     roi_align_kernel<float|_Float16, VW>
 *
 * Refused before any device call: a null descriptor or pointer, non-positive sizes, a pixel stride below c, rois_ld below 5, `out`
 * intersecting the extent of x or of the rois (SI_E_BADARG); h or w beyond 2^24 (they are used as floats), sampling_ratio beyond 256,
 * element offsets or an item count beyond 31 bits (SI_E_UNSUPPORTED).
 */
#ifndef SI_ROI_H_
#define SI_ROI_H_

#include "si_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct SiRoiAlignDesc {
    int n, c, h, w;                    /* the feature map */
    int k, ph, pw;                     /* boxes, pooled size */
    int in_ld, out_ld;                 /* pixel strides of x and out; 0: dense (c) */
    int rois_ld;                       /* row stride of the rois in floats; 0: dense (5) */
    int sampling_ratio;                /* > 0: samples per bin and axis; <= 0: ceilf(roi extent / pooled size) */
    int aligned;
    float spatial_scale;
} SiRoiAlignDesc;

int si_hip_roi_align_f32(const SiRoiAlignDesc* d, const float* x, const float* rois, float* out, si_stream_t stream);
int si_hip_roi_align_f16(const SiRoiAlignDesc* d, const void* x, const float* rois, void* out, si_stream_t stream);

/* the kernel a launch with these pointers takes; "none" for a descriptor or pointers the launch would refuse */
const char* si_hip_roi_align_kernel_name(const SiRoiAlignDesc* d, const void* x, const void* rois, const void* out, int half);

#ifdef __cplusplus
}
#endif

#endif /* SI_ROI_H_ */
