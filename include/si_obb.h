/*
 * si_obb.h -- C-ABI of the oriented-box (OBB) detection post-processing: filter, sort, rotated NMS by ProbIoU and compaction on the device, for
 * the `-obb` heads of anchor-free exports.  The symbols live in libsi_hip.so beside those of include/si_detect.h; a header of its own as
 * include/si_detect.h has.
 *
 * ---- si_hip_detect_obb_postprocess_f32 ----
 * pred holds, for n images, `rows` prediction rows of ne = 4 + objectness + classes + extra fp32 elements, in the two layouts and with the
 * strides of include/si_detect.h:
 *     cx, cy, w, h | box score (objectness == 1 only) | class scores (classes) | payload (extra)
 * The box is always centre, size and an angle in radians; the angle is payload element angle_off, 0 <= angle_off < extra, extra >= 1.
 *
 * Front end.  The filter and the sort are those of si_hip_detect_postprocess_f32, the same kernels: confidence = the first-maximum class score
 * (times the box score when objectness == 1), kept when >= prob_threshold, ordered by descending confidence with ties broken by the element
 * index (earlier row first).  That is "the confidence order" below.
 *
 * The rule.  ultralytics' nms_rotated with batch_probiou, stated exactly.  A candidate is kept exactly when no EARLIER candidate of the same
 * label (any earlier candidate when agnostic != 0) overlaps it; earlier candidates count even if they were themselves dropped (the matrix form,
 * not a greedy chain).  So the first candidate of a label is always kept and different labels never interact: ultralytics moves the centres by
 * label * 7680 to get that approximately, this entry compares the labels.  Candidate 1 (earlier) overlaps candidate 2 when
 *     !(max(bd, eps) > bd_max),    bd_max = (float)-log(1 + eps - (1 - nms_threshold)^2) formed once on the host in double,  eps = 1e-7
 * which is !(iou < nms_threshold) for iou = 1 - sqrt(1 - exp(-clamp(bd, eps, 100)) + eps) moved onto bd (bd_max < 16.2, so the upper clamp
 * never decides); a NaN bd overlaps, as torch's max hands a NaN on.  bd in fp32, in this order, every operation rounded on its own:
 *     per box   a = w * w / 12, b = h * h / 12, c = cos(angle), s = sin(angle), A = a * (c * c) + b * (s * s), B = a * (s * s) + b * (c * c),
 *               C = ((a - b) * c) * s, det = A * B - C * C, det < 0 replaced by 0
 *     per pair  sA = A1 + A2, sB = B1 + B2, sC = C1 + C2, D = sA * sB - sC * sC, dx = x1 - x2, dy = y1 - y2, r = 1 / (D + eps),
 *               t12 = (0.25 * (sA * (dy * dy) + sB * (dx * dx)) + 0.5 * ((sC * (x2 - x1)) * dy)) * r,
 *               t3 = 0.5 * log(D * (1 / (4 * sqrt(det1 * det2) + eps)) + eps),  bd = t12 + t3
 * with the device's reciprocal, square root and logarithm instructions (1 ulp each).  Decisions therefore equal those of the float64 rule
 * (tests/obb_reference.py) for every pair whose ProbIoU is not within the fp32 error of nms_threshold; the measured error is in DESIGN.md.
 *
 * Outputs (device memory).  obbs [n][max_det][7] = {cx, cy, w, h, angle, confidence, label} in the confidence order; counts [n], the kept
 * candidates, not capped by max_det; src_rows (NULL or [n][max_det]): the prediction row of each stored detection; extras (NULL or
 * [n][max_det][extra]): its payload copied as 32-bit words, a NaN keeps its bits.  Rows behind min(counts[b], max_det) are not written, in
 * any output.  With adjust == NULL the five box elements are the prediction's bits.  With adjust ([n][5] = pad_l, pad_t, scale, width,
 * height as for the other entries) the box is cx' = (cx - pad_l) / scale, cy' = (cy - pad_t) / scale, w / scale, h / scale in fp32 with IEEE
 * division; the angle is untouched and nothing is clipped: a rotated box has no rectangle to clip to (width and height are not read).
 *
 * What is read.  As include/si_detect.h: the scores of every row, the box of the rows the filter keeps, here also their angle, the rest of the
 * payload for the stored detections alone.  Nothing between rows, channels or images is read.
 *
 * Kernels.  detect_filter_rows_kernel or detect_filter_channels_kernel and yolo_rank_sort_kernel (unchanged), then "obb_record_kernel" (a
 * 32-byte record {cx, cy, A, B, C, det, label} per candidate in the confidence order), "obb_suppress_kernel" (one lane per candidate, the
 * earlier candidates' records walked through LDS tiles of 1024; no dependency chain), "obb_compact_kernel", and detect_gather_kernel when
 * extras != NULL.  No host round trip, no synchronisation, no allocation: counts stays on the device and every launch is safe inside a
 * captured graph.  What the workspace holds on entry does not matter.
 *
 * Refused before any device call.  SI_E_BADARG: a null descriptor, pred, out, counts or workspace, a pred off its 4-byte element, obbs NULL
 * with max_det > 0, non-positive n / rows / classes, extra < 1, angle_off outside [0, extra), objectness or layout out of range, ld or
 * image_ld too small, max_det < 0, nms_threshold not in (0, 1] (a NaN included), a workspace smaller than
 * si_hip_detect_obb_postprocess_workspace_bytes.  SI_E_UNSUPPORTED: the limits of si_hip_detect_postprocess_f32 (n > 65535, SI_DETECT_ROWS
 * with ne > 128, an image's extent beyond 31 bits, a whole operand or output beyond 2^46 elements).
 *
 * Out of scope: ultralytics' regularize_rboxes (angle mod pi with a w / h swap: a caller's step on the few stored rows), a greedy-chain
 * option, the exact polygon IoU, and the max_nms cap on the candidates (every candidate the filter keeps takes part).
 */
#ifndef SI_OBB_H_
#define SI_OBB_H_

#include "si_detect.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct SiDetectObbDesc {
    int n, rows;            /* images, prediction rows per image */
    int classes;            /* >= 1 */
    int objectness;         /* 1: element 4 is a box score */
    int extra;              /* >= 1 payload elements behind the class scores; one of them is the angle */
    int layout;             /* SI_DETECT_ROWS / SI_DETECT_CHANNELS */
    int ld; long long image_ld;
    int angle_off;          /* the angle is payload element angle_off */
    float prob_threshold, nms_threshold;
    int agnostic, max_det;
} SiDetectObbDesc;           /* ne = 4 + objectness + classes + extra */

typedef struct SiDetectObbOut {
    float* obbs;       /* [n][max_det][7] {cx, cy, w, h, angle, confidence, label} */
    int*   counts;     /* [n] kept candidates, uncapped */
    int*   src_rows;   /* NULL or [n][max_det] */
    float* extras;     /* NULL or [n][max_det][extra], bit for bit */
} SiDetectObbOut;

/* 0 for a descriptor the launch would refuse */
size_t si_hip_detect_obb_postprocess_workspace_bytes(const SiDetectObbDesc* d);
int si_hip_detect_obb_postprocess_f32(const SiDetectObbDesc* d, const float* pred, const float* adjust /* NULL or [n][5] */,
                                      const SiDetectObbOut* out, void* workspace, size_t workspace_bytes, si_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* SI_OBB_H_ */
