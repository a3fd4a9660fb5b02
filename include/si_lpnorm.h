/*
 * si_lpnorm.h -- C-ABI of torch.norm (p = 1, 2, inf over axes of an NHWC tensor) and F.normalize (x / max(norm, eps) along one axis),
 * torch's semantics.  The symbols live in libsi_hip.so beside those of include/si_hip.h; they have a header of their own as
 * include/si_reduce.h and include/si_softmax.h have.
 *
 * Tensors are NHWC with pixel strides in_ld / out_ld (in elements) on both sides: what lies between two pixels (ld > channels) is never
 * read and never written.  A rank-2 [N, F] tensor is n = N, h = w = 1, c = F.  `in` and `out` must not overlap (two disjoint channel
 * slices of one buffer with a common pixel stride do not overlap).  With normalize = 0 the output is NHWC with every reduced axis of
 * extent 1 (keepdim; a caller that drops the axes reinterprets the same memory); with normalize = 1 it has the input's shape.
 *
 * Arithmetic, the same in every form.  A SET is the elements one norm is taken over.
 *   - all accumulation is in float32 whatever the storage; the fp16 entry widens halves on load and rounds once, to nearest even, at
 *     the store;
 *   - p = 1: the sum of |x|;
 *   - p = 2: sqrtf(the sum of x * x).  Each square is rounded to float32 on its own and then added (no fma contraction: the file is
 *     compiled with `#pragma clang fp contract(off)`, the promise include/si_act.h makes for mish); the square root is correctly rounded;
 *   - p = inf: the maximum of |x|, a selection that never rounds; it keeps a NaN as SI_REDUCE_AMAX does
 *     (max(a, b) = (a != a || a > b) ? a : b);
 *   - there is no rescaling, the rule is what torch does on a GPU: for p = 2 an |x| above sqrt(FLT_MAX) ~ 1.8e19 squares to +inf (the
 *     norm is +inf), squares below 2^-126 (|x| < ~1.1e-19) are subnormal and lose bits, and an |x| below 2^-75 ~ 2.6e-23 squares to 0;
 *   - normalize: d = norm < eps ? eps : norm (a NaN norm passes through, as torch's clamp_min does), then out = x / d with ONE IEEE
 *     (correctly rounded) division per element -- torch's arithmetic, not a multiplication by a reciprocal;
 *   - special values follow from that: a NaN anywhere in a set makes that set's norm NaN and that set's outputs NaN and touches no
 *     other set; an infinite element gives the norm +inf, the finite elements of the set map to +-0 and the infinite ones to NaN; a set
 *     of zeros gives 0 / eps = 0 with the sign kept, and with eps = 0 gives 0 / 0 = NaN.
 *
 * Supported masks: axes == 8 (the channel axis alone, contiguous per pixel), and every non-empty subset of {n, h, w} with the channel
 * axis kept.  A mask that mixes c with another axis is SI_E_UNSUPPORTED (the rule of include/si_reduce.h).  With normalize = 1 the mask
 * is a single axis.
 *
 * Forms, chosen from the descriptor, the strides and the pointers' alignment alone, never from n unless the n axis is itself reduced
 * and never from the grid; si_hip_lpnorm_kernel_name reports which.  An ITEM is a 16-byte channel vector (4 floats / 8 halves), or a
 * single element in the single-element instantiation; VW is its width; the elements of an item enter the accumulator in channel order.
 * Every accumulator starts at +0.
 *   row_group        axes == 8, c <= SI_LPNORM_GROUP_MAX_C.  A group of L = 2^k <= 64 lanes per pixel, several pixels per wave64.  With
 *                    cv = c / VW items and per = min(16 / VW, 4): L is the smallest power of two with L * per >= cv, at most 64.  Lane j
 *                    adds (selects) items j, j + L, j + 2L, ... in that order; then a __shfl_xor butterfly over the offsets L / 2, L / 4,
 *                    ..., 1: at every step lane j's value becomes v[j] + v[j ^ offset] (a pairwise tree).  With normalize the row stays
 *                    in registers: one read, one write.
 *   row_block        axes == 8, SI_LPNORM_GROUP_MAX_C < c <= SI_LPNORM_BLOCK_MAX_C.  A workgroup of 256 threads per pixel, the row in
 *                    registers; thread t adds items t, t + 256, ...; the butterfly above over each wave of 64 (offsets 32 .. 1), then
 *                    ((w0 + w1) + w2) + w3 over the four wave values from LDS.
 *   row_block_2pass  axes == 8, longer rows.  The same workgroup and the same order of additions; with normalize a second read of the
 *                    row applies the division.
 *   col_lane         masks within {n, h, w}.  One lane per (kept pixel, item); neighbouring lanes take neighbouring channels; every
 *                    channel is a set of its own, and the lane adds its reduced positions one after the other in increasing (n, h, w)
 *                    order.  With normalize an axis of at most SI_LPNORM_COL_REG_POSITIONS positions stays in registers (one read),
 *                    a longer one is walked twice.
 * The square root (p = 2) is taken once per set, after the last addition.  Each form has a 16-byte vector instantiation and a
 * single-element one.  The vector one is taken when c, both strides and both pointers allow it; the row forms with normalize = 0 store
 * one element per pixel, so there c, in_ld and `in` decide.  Grids are capped and the kernels loop over the rest (grid-stride); the
 * result of a set does not depend on which pass or workgroup computed it.
 *
 * Every reduction runs in the order above: no atomics, no workspace, no host round trip; two launches give the same bits, a set's
 * result does not depend on the other sets of the launch, image i of a batch has the bits of that image run alone (n not reduced), and
 * every launch is safe inside a captured graph.
 *
 * Refused before any device call: a null descriptor or tensor, non-positive sizes, in_ld < c, out_ld < the output's channels, axes
 * outside 1 .. 15, p outside 0 .. 2, normalize outside 0 / 1, a negative or NaN eps (whatever normalize is), normalize with more than
 * one axis, overlapping in / out (SI_E_BADARG); a mask that mixes c with n, h or w, element offsets that do not fit 31 bits
 * (SI_E_UNSUPPORTED).  SI_E_BADARG is looked for first.
 */
#ifndef SI_LPNORM_H_
#define SI_LPNORM_H_

#include "si_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { SI_LPNORM_P1 = 0, SI_LPNORM_P2 = 1, SI_LPNORM_PINF = 2 };

/* the form switches: the register budgets of include/si_softmax.h.  A lane keeps 16 floats of its row, a group has at most 64 lanes
 * (1024) and a workgroup 256 threads (4096); a col_lane lane keeps 8 positions of a 16-byte vector (64 floats for halves). */
enum { SI_LPNORM_GROUP_MAX_C = 1024, SI_LPNORM_BLOCK_MAX_C = 4096, SI_LPNORM_COL_REG_POSITIONS = 8 };

typedef struct SiLpNormDesc {
    int n, h, w, c;      /* input NHWC; a rank-2 [N, F] tensor is n = N, h = w = 1, c = F */
    int in_ld, out_ld;   /* pixel strides in elements; in_ld >= c, out_ld >= output channels */
    int axes;            /* bit mask of the NHWC axes reduced over, as SI_REDUCE_AXIS_*: 1 n, 2 h, 4 w, 8 c */
    int p;               /* SI_LPNORM_P* */
    int normalize;       /* 0: write the norm (reduced axes have extent 1); 1: write x / max(norm, eps) in x's shape */
    float eps;           /* normalize only; >= 0; 0 gives plain x / norm */
} SiLpNormDesc;

int si_hip_lpnorm_f32(const SiLpNormDesc* d, const float* in, float* out, si_stream_t stream);

/* half in, half out */
int si_hip_lpnorm_f16(const SiLpNormDesc* d, const void* in, void* out, si_stream_t stream);

/* the kernel a launch with these pointers takes: "lpnorm_row_group_kernel<T, VW>", "lpnorm_row_block_kernel<T, VW>",
 * "lpnorm_row_block_2pass_kernel<T, VW>", "lpnorm_col_lane_kernel<T, VW>" or, for normalize over an axis that stays in registers,
 * "lpnorm_col_lane_reg_kernel<T, VW>", with <float, 4>, <float, 1>, <_Float16, 8> or <_Float16, 1>; "none" for a descriptor the launch
 * would refuse (the pointers are looked at for their alignment only) */
const char* si_hip_lpnorm_kernel_name(const SiLpNormDesc* d, const void* in, const void* out, int half);

#ifdef __cplusplus
}
#endif

#endif /* SI_LPNORM_H_ */
