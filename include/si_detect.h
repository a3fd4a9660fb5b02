/*
 * si_detect.h -- C-ABI of the general detection post-processing: the filter / sort / NMS / un-letterbox of si_hip_yolo_postprocess_f32
 * (include/si_hip.h) for heads without a box score, channel-major outputs, corner boxes and rows that carry a payload behind the class scores
 * (mask coefficients, keypoints), and the instance masks made from that payload.  The symbols live in libsi_hip.so beside those of
 * include/si_hip.h; a header of its own as include/si_softmax.h and include/si_roi.h have.
 *
 * ---- si_hip_detect_postprocess_f32 ----
 * pred holds, for n images, `rows` prediction rows of ne = 4 + objectness + classes + extra fp32 elements:
 *     box (4) | box score (objectness == 1 only) | class scores (classes) | payload (extra)
 * SI_DETECT_ROWS: element e of row r of image b at pred[b * image_ld + r * ld + e], ld >= ne;  SI_DETECT_CHANNELS: at
 * pred[b * image_ld + e * ld + r], ld >= rows (a [N, ne, rows] export without its closing permute).  image_ld is at least one image's extent.
 *
 * The rule is that of si_hip_yolo_postprocess_f32, with its four documented rules on ties, equalities, label -1 and limits (include/si_hip.h),
 * the select-based intersection, the reference's clip, per-class segments or the agnostic chain, max_det and uncapped counts; bit for bit
 * tests/detect_reference.py.  Only the front end differs:
 *   confidence   objectness == 1: box score * first-maximum class score;  objectness == 0: the first-maximum class score.  The compare is a
 *                strict '>' starting from -FLT_MAX: a row with no maximum has label -1 and class score -FLT_MAX.
 *   box          SI_DETECT_CXCYWH: x0 = cx - w * 0.5f, x1 = cx + w * 0.5f, the box {x0, y0, x1 - x0, y1 - y0} (the existing arithmetic);
 *                SI_DETECT_XYXY: {x0, y0, x1 - x0, y1 - y0}.
 * With objectness = 1, SI_DETECT_ROWS, SI_DETECT_CXCYWH, extra = 0 and dense strides the entry writes the bytes si_hip_yolo_postprocess_f32
 * writes: both run the same kernels.
 *
 * Outputs (device memory).  dets and counts as si_hip_yolo_postprocess_f32 has them: rows behind min(counts[b], max_det) are not written, in
 * any output.  src_rows: the prediction row r of each stored detection.  net_boxes: its box {x, y, w, h} in network coordinates, before
 * `adjust`.  extras: the `extra` payload elements of that row, copied as 32-bit words: a NaN keeps its bits.  Each of the three may be NULL.
 *
 * What is read.  The filter reads the box score and the class scores of every row and the box of the rows it keeps; the payload is read for
 * the stored detections alone.  Nothing between rows (ld > ne), channels (ld > rows) or images is read.
 *
 * Kernels.  SI_DETECT_ROWS with ne <= 128: "detect_filter_rows_kernel", 128 rows staged in LDS with coalesced loads, one lane per row.
 * SI_DETECT_CHANNELS: "detect_filter_channels_kernel", one lane per row, the lanes walk the elements so that neighbouring lanes read
 * neighbouring addresses; nothing is staged and ne has no limit.  Then yolo_rank_sort_kernel, yolo_nms_kernel or yolo_nms_segments_kernel +
 * yolo_compact_kernel, and detect_gather_kernel when extras != NULL.  No host round trip, no synchronisation, no allocation: counts stays on
 * the device and every launch is safe inside a captured graph.  Candidate slots are taken with atomicAdd; the result does not depend on the
 * arrival order because the sort keys are unique.  What the workspace holds on entry does not matter.
 *
 * Refused before any device call.  SI_E_BADARG: a null descriptor, pred, out, counts or workspace, a pred off its 4-byte element, dets NULL
 * with max_det > 0, non-positive n / rows / classes, extra < 0, objectness, layout or box_format out of range, ld or image_ld too small,
 * max_det < 0, a workspace smaller than si_hip_detect_postprocess_workspace_bytes.  SI_E_UNSUPPORTED: n > 65535, SI_DETECT_ROWS with ne > 128, an image's extent beyond 31
 * bits, a whole operand or output beyond 2^46 elements.
 *
 * ---- si_hip_detect_masks_f32 ----
 * ultralytics' process_mask without the upsample.  protos [n][mh][mw][nm] (the engine's NHWC storage of a [N, nm, mh, mw] output), pixels
 * proto_ld >= nm elements apart; extras / net_boxes / counts as the entry above wrote them with the same max_det and extra; the coefficients of
 * detection d are extras[b][d][coef_off .. coef_off + nm).  masks [n][max_det][mh][mw] bytes: for d < min(counts[b], max_det) the whole plane
 * is written, planes behind that are not touched.  Pixel (r, c) is 1 exactly when
 *   crop   (float)c >= x1 && (float)c < x2 && (float)r >= y1 && (float)r < y2,  x1 = bx * ratio_w, x2 = (bx + bw) * ratio_w, y1 = by * ratio_h,
 *          y2 = (by + bh) * ratio_h, all in fp32 (a NaN box gives an empty mask), and
 *   dot    (((0 + c0 p0) + c1 p1) + ...) > 0 in index order, every product and every sum rounded to fp32 on its own (no fused multiply-add).
 * Kernels: "detect_masks_kernel<32>" (nm == 32, proto_ld % 4 == 0, protos 16-byte aligned: a lane keeps its pixel's prototypes in registers)
 * and "detect_masks_kernel<0>" (1 <= nm <= 64: a tile's prototypes staged in LDS); both produce the same bits.  A workgroup takes a tile of
 * pixels of one image and loops over that image's detections, so the prototypes are read once per tile; the coefficients are wave-uniform; the
 * dot is computed only by waves with a pixel inside the crop; four mask bytes per store when mw % 4 == 0 and masks is 4-byte aligned.  The
 * matrix cores are not used: their accumulation order would give up the bit rule.
 * Refused before any device call.  SI_E_BADARG: a null descriptor or pointer, non-positive n / mh / mw / nm / extra, proto_ld < nm,
 * max_det < 0, coef_off < 0 or coef_off + nm > extra.  SI_E_UNSUPPORTED: nm > 64, n > 65535, an image's prototypes beyond 31 bits of
 * elements, masks or extras beyond 2^46 elements.
 */
#ifndef SI_DETECT_H_
#define SI_DETECT_H_

#include "si_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { SI_DETECT_ROWS = 0, SI_DETECT_CHANNELS = 1 };      /* layout */
enum { SI_DETECT_CXCYWH = 0, SI_DETECT_XYXY = 1 };        /* box_format */

typedef struct SiDetectPostDesc {
    int n, rows;            /* images, prediction rows per image */
    int classes;            /* >= 1 */
    int objectness;         /* 0: confidence = the first-maximum class score
                               1: element 4 is a box score, confidence = box score * class score (YOLOv5 / YOLOX) */
    int extra;              /* >= 0 payload elements behind the class scores: carried as bits, never interpreted */
    int layout;             /* ROWS:     element e of row r of image b at pred[b * image_ld + r * ld + e], ld >= ne
                               CHANNELS: at pred[b * image_ld + e * ld + r], ld >= rows */
    int ld; long long image_ld;
    int box_format;
    float prob_threshold, nms_threshold;
    int agnostic, max_det;
} SiDetectPostDesc;          /* ne = 4 + objectness + classes + extra */

typedef struct SiDetectPostOut {
    float* dets;       /* [n][max_det][6] {x, y, w, h, confidence, label}: exactly the existing entry's rows */
    int*   counts;     /* [n] picks, uncapped, as today */
    int*   src_rows;   /* NULL or [n][max_det]: the prediction row of each stored detection */
    float* net_boxes;  /* NULL or [n][max_det][4]: x, y, w, h in network coordinates, before `adjust` */
    float* extras;     /* NULL or [n][max_det][extra]: the payload of that row, bit for bit */
} SiDetectPostOut;

/* 0 for a descriptor the launch would refuse */
size_t si_hip_detect_postprocess_workspace_bytes(const SiDetectPostDesc* d);
int si_hip_detect_postprocess_f32(const SiDetectPostDesc* d, const float* pred, const float* adjust /* NULL or [n][5] */,
                                  const SiDetectPostOut* out, void* workspace, size_t workspace_bytes, si_stream_t stream);
/* the filter kernel a launch takes; "none" for a descriptor or a pointer the launch would refuse */
const char* si_hip_detect_filter_kernel_name(const SiDetectPostDesc* d, const void* pred);

typedef struct SiDetectMaskDesc {
    int n, mh, mw, nm;      /* prototypes [n][mh][mw][nm]: the engine's NHWC storage of a [N, nm, mh, mw] output */
    int proto_ld;           /* pixel stride >= nm */
    int max_det, extra, coef_off;   /* coefficients of detection d: extras[b][d][coef_off .. coef_off + nm) */
    float ratio_w, ratio_h; /* mw / network width, mh / network height, formed by the caller in fp32 */
} SiDetectMaskDesc;

int si_hip_detect_masks_f32(const SiDetectMaskDesc* d, const float* protos, const float* extras, const float* net_boxes,
                            const int* counts, unsigned char* masks /* [n][max_det][mh][mw] */, si_stream_t stream);
/* the kernel a launch with these pointers takes; "none" when refused */
const char* si_hip_detect_masks_kernel_name(const SiDetectMaskDesc* d, const void* protos);

#ifdef __cplusplus
}
#endif

#endif /* SI_DETECT_H_ */
