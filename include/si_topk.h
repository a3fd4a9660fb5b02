/*
 * si_topk.h -- C-ABI of the NMS-free detection post-processing: the max_det best (row, class) pairs of a score matrix, selected on the device.
 * End-to-end heads (YOLOv10's one2one head and its successors, RT-DETR's decoder) post-process by `scores.flatten(1).topk(max_det)`; label and
 * row come from the flat index, and one row may appear with several labels.  The symbols live in libsi_hip.so beside those of include/si_hip.h;
 * a header of its own as include/si_obb.h and include/si_imgmask.h have.  Layouts, box formats and the output structure are those of
 * include/si_detect.h.
 *
 * ---- si_hip_detect_topk_postprocess_f32 ----
 * Operand.  pred holds, for n images, `rows` prediction rows of ne = 4 + classes + extra fp32 elements:  box (4) | class scores | payload.
 * SI_DETECT_ROWS: element e of row r of image b at pred[b * image_ld + r * ld + e], ld >= ne;  SI_DETECT_CHANNELS: at
 * pred[b * image_ld + e * ld + r], ld >= rows.  There is no box score (the `objectness = 0` front end of SiDetectPostDesc).  Nothing between
 * rows (ld > ne), channels (ld > rows) or images is read.
 *
 * Candidates.  multi_label = 1: every pair (r, c) with score s = the class score and flat index f = r * classes + c.  multi_label = 0: one
 * candidate per row, its first-maximum class by a strict '>' starting from -FLT_MAX (a row with no maximum has label -1 and score -FLT_MAX),
 * with f = r.  A candidate is kept when s > prob_threshold; a NaN score is therefore never kept, and a NaN threshold keeps nothing.
 *
 * Order.  Score descending as fp32 values (-0.0 and +0.0 are equal), ties by ascending f.  These keys are unique, so the result is a function
 * of the input alone: not of atomic arrival order, the grid, or what the workspace held.
 *
 * Outputs (device memory).  counts[b]: the number of kept candidates, uncapped.  For d < min(counts[b], max_det): dets[b][d] = {x, y, w, h,
 * confidence, label} with the box arithmetic and the `adjust` un-letterbox / clip of si_hip_detect_postprocess_f32 (the same device code),
 * confidence = the stored score with its bits (a -0.0 stays -0.0);  src_rows[b][d] = r;  net_boxes[b][d] = the box before `adjust`;
 * extras[b][d] = the row's payload as 32-bit words.  Each of the three may be NULL.  Rows behind min(counts[b], max_det) are not written.
 *
 * Kernels.  A radix select over the order-preserving integer image of the scores (11 + 11 + 10 bits), then a sort of the selected keys alone.
 * Ten launches, fixed by the descriptor: "topk_clear_kernel"; three times "topk_hist_kernel<LAYOUT, LEVEL>" (images x chunks of 256 rows: a
 * lane owns a row and walks its classes, neighbouring lanes read neighbouring rows of a class in SI_DETECT_CHANNELS and an LDS stage of 32
 * classes x 256 rows in SI_DETECT_ROWS; an LDS histogram of the level's bits under the prefix found so far, flushed with integer atomic adds,
 * which commute) and "topk_select_kernel<LEVEL>" (one workgroup per image: suffix scan of the bins, the bin in which the running count reaches
 * max_det);  "topk_collect_kernel<LAYOUT>" (keys above the threshold key T take slots by atomic add; the keys equal to T are counted per
 * chunk);  "topk_collect_ties_kernel<LAYOUT>" (a chunk whose equal keys rank below `need` -- the chunk counts before it summed in order,
 * then an ordered scan over the lanes -- stores the `need` lowest flat indices; every other chunk returns at once);
 * "topk_sort_write_kernel" (one workgroup per image: LDS bitonic sort of at most 1024 keys {ordered score, ~f}, then all outputs).
 * No host round trip, no synchronisation, no allocation, no memset node: every launch is legal inside a captured graph.  The workspace is
 * n * (3 * 2048 histogram words + chunks + max_det keys + a few words), never a multiple of rows * classes.
 *
 * Refused before any device call.  SI_E_BADARG: a null descriptor, pred, out, counts or workspace, a pred off its 4-byte element, dets NULL
 * with max_det > 0, non-positive n / rows / classes, extra < 0, layout, box_format or multi_label out of range, ld or image_ld too small,
 * max_det < 0, a workspace smaller than si_hip_detect_topk_workspace_bytes.  SI_E_UNSUPPORTED: max_det > SI_DETECT_TOPK_MAX_DET (what the final
 * sort holds in LDS; ultralytics' default is 300), n > 65535, rows * classes beyond 31 bits (the flat index), an image's extent beyond 31 bits,
 * a whole operand or output beyond 2^46 elements.
 */
#ifndef SI_TOPK_H_
#define SI_TOPK_H_

#include "si_detect.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { SI_DETECT_TOPK_MAX_DET = 1024 };

typedef struct SiDetectTopkDesc {
    int n, rows;            /* images, prediction rows per image */
    int classes;            /* >= 1 */
    int extra;              /* >= 0 payload elements behind the class scores: carried as bits, never interpreted */
    int layout;             /* SI_DETECT_ROWS / SI_DETECT_CHANNELS, as SiDetectPostDesc */
    int ld; long long image_ld;
    int box_format;         /* SI_DETECT_CXCYWH / SI_DETECT_XYXY */
    float prob_threshold;   /* kept: score > prob_threshold */
    int multi_label;        /* 1: every (row, class) pair is a candidate;  0: the first-maximum class of each row */
    int max_det;            /* 0 .. SI_DETECT_TOPK_MAX_DET */
} SiDetectTopkDesc;         /* ne = 4 + classes + extra */

/* 0 for a descriptor the launch would refuse */
size_t si_hip_detect_topk_workspace_bytes(const SiDetectTopkDesc* d);
int si_hip_detect_topk_postprocess_f32(const SiDetectTopkDesc* d, const float* pred, const float* adjust /* NULL or [n][5] */,
                                       const SiDetectPostOut* out, void* workspace, size_t workspace_bytes, si_stream_t stream);
/* the histogram kernel a launch takes: "topk_hist_kernel<SI_DETECT_ROWS>" or "topk_hist_kernel<SI_DETECT_CHANNELS>"; "none" for a descriptor
 * or a pointer the launch would refuse */
const char* si_hip_detect_topk_kernel_name(const SiDetectTopkDesc* d, const void* pred);

#ifdef __cplusplus
}
#endif

#endif /* SI_TOPK_H_ */
