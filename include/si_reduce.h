/*
 * si_reduce.h -- C-ABI of torch.sum / torch.mean / torch.amax / torch.amin over axes of an NHWC tensor, torch's semantics.  The symbols
 * live in libsi_hip.so beside those of include/si_hip.h; they have a header of their own as include/si_softmax.h and include/si_slice.h
 * have.
 *
 * The output is NHWC with every reduced axis of extent 1 (keepdim; a caller that drops the axes reinterprets the same memory).  Tensors
 * carry pixel strides in_ld / out_ld (in elements) on both sides: what lies between two pixels (ld > channels) is never read and never
 * written.  A rank-2 [N, F] tensor is n = N, h = w = 1, c = F.  `in` and `out` must not overlap (two disjoint channel slices of one
 * buffer with a common pixel stride do not overlap).
 *
 * Arithmetic, the same in every form:
 *   - all accumulation is in float32; the fp16 entry widens halves on load and rounds once, to nearest even, at the store;
 *   - mean is the sum followed by ONE IEEE division by (float)count, count = the product of the reduced extents (the promise of
 *     include/si_pool.h for its divisor);
 *   - amax / amin select and never round;
 *   - a NaN anywhere in the reduced set gives NaN (torch's rule; a bare fmaxf / v_max would drop it), and makes no other result NaN;
 *   - sum / mean follow IEEE for infinities: one +inf gives +inf, +inf together with -inf gives NaN.
 *
 * Supported masks: axes == 8 (the channel axis alone, contiguous per pixel), and every non-empty subset of {n, h, w} with the channel
 * axis kept.  A mask that mixes c with another axis is SI_E_UNSUPPORTED.
 *
 * Forms, chosen from the descriptor and the pointers' alignment alone, and never from n unless the n axis is itself reduced;
 * si_hip_reduce_kernel_name reports which:
 *   row_group  axes == 8, c <= SI_REDUCE_GROUP_MAX_C.  A group of 2^k <= 64 lanes per pixel, sized from c, several pixels per wave; lane j
 *              adds (selects) items j, j + L, ... in that order; __shfl_xor butterflies combine the lanes of the group.
 *   row_block  axes == 8, longer rows.  A workgroup of 256 threads per pixel; thread t takes items t, t + 256, ...; butterflies per wave,
 *              then the four wave partials from LDS in index order.
 *   col_lane   axes within {n, h, w}.  One lane per (kept pixel, channel vector); neighbouring lanes take neighbouring channels; the lane
 *              walks the reduced positions in increasing (n, h, w) order.
 *   col_coop   the same masks with at least SI_REDUCE_COOP_MIN_POSITIONS reduced positions and at most SI_REDUCE_COOP_MAX_OUTPUTS
 *              outputs per image (kept h x kept w x c elements: a kept n is never counted).  A workgroup of
 *              SI_REDUCE_COOP_PARTS x SI_REDUCE_COOP_SLOTS threads serves SI_REDUCE_COOP_SLOTS (kept pixel, channel vector) items; the
 *              reduced positions are cut into SI_REDUCE_COOP_PARTS runs of ceil(positions / parts) consecutive positions, part g walks
 *              run g in order, and the non-empty partials are combined from LDS in the order g = 0, 1, ...
 * Each form has a 16-byte vector instantiation (4 floats / 8 halves across channels) and a single-element one.  The row forms store one
 * element per pixel, so they take the vector one when c, in_ld and `in` allow it; the col forms when c, both strides and both pointers
 * do.  Every reduction runs in a fixed order: no atomics, no workspace, no host round trip; two launches give the same bits, a result
 * does not depend on the other results of the launch, image i of a batch has the bits of that image run alone (n not reduced), and every
 * launch is safe inside a captured graph.
 *
 * Refused before any device call: a null descriptor or tensor, non-positive sizes, in_ld < c, out_ld < the output's channels, axes
 * outside 1 .. 15, op outside 0 .. 3, overlapping in / out (SI_E_BADARG); a mask that mixes c with n, h or w, element offsets that do
 * not fit 31 bits (SI_E_UNSUPPORTED).
 */
#ifndef SI_REDUCE_H_
#define SI_REDUCE_H_

#include "si_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { SI_REDUCE_SUM = 0, SI_REDUCE_MEAN = 1, SI_REDUCE_AMAX = 2, SI_REDUCE_AMIN = 3 };

/* the bits of SiReduceDesc::axes */
enum { SI_REDUCE_AXIS_N = 1, SI_REDUCE_AXIS_H = 2, SI_REDUCE_AXIS_W = 4, SI_REDUCE_AXIS_C = 8 };

/* the form switches.
 * SI_REDUCE_GROUP_MAX_C: a choice of parallelism, not a register budget (a lane keeps one accumulator): up to 1024 channels a group of at
 *   most 64 lanes takes at most 16 floats per lane, beyond that a row is worth a workgroup.
 * SI_REDUCE_COOP_PARTS x SI_REDUCE_COOP_SLOTS: the workgroup of col_coop, 64 x 8 = 512 threads; the 8 slots of a part read 128
 *   consecutive bytes of a position with 16-byte vectors; the partials take parts x slots x 8 floats = 16 KiB of LDS at most.
 * SI_REDUCE_COOP_MIN_POSITIONS / SI_REDUCE_COOP_MAX_OUTPUTS: the col_lane / col_coop switch, a performance choice.  16384 outputs are
 *   4096 float4 lanes = 64 waves of col_lane for one image, one wave for every fourth compute unit of a 256-CU part, so below that
 *   col_lane cannot fill the chip whatever the batch is: derived, not measured.  The positions started at 64 (one per part) and moved to
 *   32 on the measurement: at 49 positions col_coop already runs at 0.87x (fp32) / 0.65x (fp16) of col_lane, at 400 at 0.21x / 0.15x
 *   (DESIGN.md 9i); between 32 and 48 positions nothing is measured. */
enum {
    SI_REDUCE_GROUP_MAX_C = 1024,
    SI_REDUCE_COOP_PARTS = 64,
    SI_REDUCE_COOP_SLOTS = 8,
    SI_REDUCE_COOP_MIN_POSITIONS = 32,
    SI_REDUCE_COOP_MAX_OUTPUTS = 16384
};

typedef struct SiReduceDesc {
    int n, h, w, c;      /* input NHWC; a rank-2 [N, F] tensor is n = N, h = w = 1, c = F */
    int in_ld, out_ld;   /* pixel strides in elements; in_ld >= c, out_ld >= output channels */
    int axes;            /* bit mask of the NHWC axes reduced over: 1 n, 2 h, 4 w, 8 c */
    int op;              /* SI_REDUCE_* */
} SiReduceDesc;

int si_hip_reduce_f32(const SiReduceDesc* d, const float* in, float* out, si_stream_t stream);

/* half in, half out */
int si_hip_reduce_f16(const SiReduceDesc* d, const void* in, void* out, si_stream_t stream);

/* the kernel a launch with these pointers takes: "reduce_row_group_kernel<T, VW>", "reduce_row_block_kernel<T, VW>",
 * "reduce_col_lane_kernel<T, VW>" or "reduce_col_coop_kernel<T, VW>" with <float, 4>, <float, 1>, <_Float16, 8> or <_Float16, 1>;
 * "none" for a descriptor the launch would refuse (the pointers are looked at for their alignment only) */
const char* si_hip_reduce_kernel_name(const SiReduceDesc* d, const void* in, const void* out, int half);

#ifdef __cplusplus
}
#endif

#endif /* SI_REDUCE_H_ */
