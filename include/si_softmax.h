/*
 * si_softmax.h -- C-ABI of nn.Softmax / nn.LogSoftmax / nn.Softmax2d / F.softmax / F.log_softmax along one axis of an NHWC tensor,
 * torch's semantics.  The symbols live in libsi_hip.so beside those of include/si_hip.h; they have a header of their own as
 * include/si_norm.h, include/si_pad.h and include/si_pool.h have.
 *
 * Arithmetic, the same in every form and in float32 throughout: m = the maximum over the axis, s = sum exp(x - m);
 *     softmax      exp(x - m) / s        (as exp(x - m) * rcp(s): one reciprocal per row)
 *     log_softmax  (x - m) - log(s)
 * with the hardware's exp2 / log2 (__expf, __logf).  The fp16 entry widens halves on load and rounds once, to nearest even, at the
 * store.  Subtracting the maximum keeps every exponent at or below 0: finite inputs of any magnitude never overflow.  Special values
 * follow torch: a -inf element of a row with a finite maximum gives exactly 0 (softmax) or -inf (log_softmax); a row whose maximum is
 * +inf and a row of only -inf are NaN throughout; a NaN makes its own row NaN and no other.
 *
 * Tensors are NHWC with pixel strides in_ld / out_ld (in elements) on both sides: what lies between two pixels (ld > c) is never read
 * and never written.  A rank-2 [N, F] tensor is n = N, h = w = 1, c = F.  `in` and `out` must not overlap.
 *
 * Forms, chosen from the shape, the strides and the pointers' alignment alone (never from n or the row count);
 * si_hip_softmax_kernel_name reports which:
 *   group           axis 3, c <= SI_SOFTMAX_GROUP_MAX_C.  A group of 2^k <= 64 lanes per row, sized from c, several rows per wave; the row
 *                   stays in registers (one read); the maximum and the sum are __shfl_xor butterflies inside the group.
 *   block           axis 3, SI_SOFTMAX_GROUP_MAX_C < c <= SI_SOFTMAX_BLOCK_MAX_C.  A workgroup of 256 threads per row, the row in
 *                   registers (one read); butterflies per wave, then the four wave partials from LDS in index order.
 *   block_online    axis 3, longer rows.  The same workgroup; every thread runs the online recurrence (running maximum, rescaled sum) over
 *                   its share, the partials are rescaled to the row's maximum and added as above; a second pass reads the row again.
 *   strided         axes 0, 1, 2 of at most SI_SOFTMAX_STRIDED_REG_A positions.  One lane per (outer index, 16-byte channel vector);
 *                   neighbouring lanes take neighbouring channels; the lane keeps the axis in registers (one read).
 *   strided_online  longer axes 0, 1, 2.  The lane walks the axis with the online recurrence, then walks it again to write.
 * Each form has a 16-byte vector instantiation (4 floats / 8 halves), taken when c, both strides and both pointers allow it, and a
 * single-element one.  Every reduction runs in a fixed order: no atomics, no workspace, no host round trip; two launches give the same
 * bits, a row's result does not depend on the other rows of the launch, image i of a batch has the bits of that image run alone (axis
 * != 0), and every launch is safe inside a captured graph.
 *
 * Refused before any device call: a null descriptor or tensor, non-positive sizes, ld < c, axis outside 0 .. 3, log outside 0 / 1
 * (SI_E_BADARG); element offsets that do not fit 31 bits (SI_E_UNSUPPORTED).
 */
#ifndef SI_SOFTMAX_H_
#define SI_SOFTMAX_H_

#include "si_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the form switches.  Register budgets, not measurements: a lane keeps 16 floats of its row, a group has at most 64 lanes (1024) and a
 * workgroup 256 threads (4096); a strided lane keeps 8 positions of a 16-byte vector (64 floats for halves). */
enum { SI_SOFTMAX_GROUP_MAX_C = 1024, SI_SOFTMAX_BLOCK_MAX_C = 4096, SI_SOFTMAX_STRIDED_REG_A = 8 };

typedef struct SiSoftmaxDesc {
    int n, h, w, c;      /* NHWC; a rank-2 [N, F] tensor is n = N, h = w = 1, c = F */
    int in_ld, out_ld;   /* pixel strides in elements, >= c */
    int axis;            /* NHWC axis reduced over: 0 n, 1 h, 2 w, 3 c */
    int log;             /* 0 softmax, 1 log_softmax */
} SiSoftmaxDesc;

int si_hip_softmax_f32(const SiSoftmaxDesc* d, const float* in, float* out, si_stream_t stream);

/* half in, half out */
int si_hip_softmax_f16(const SiSoftmaxDesc* d, const void* in, void* out, si_stream_t stream);

/* the kernel a launch with these pointers takes: "softmax_group_kernel<T, VW>", "softmax_block_kernel<T, VW>",
 * "softmax_block_online_kernel<T, VW>", "softmax_strided_kernel<T, VW>" or "softmax_strided_online_kernel<T, VW>" with <float, 4>,
 * <float, 1>, <_Float16, 8> or <_Float16, 1>; "none" for a descriptor the launch would refuse */
const char* si_hip_softmax_kernel_name(const SiSoftmaxDesc* d, const void* in, const void* out, int half);

#ifdef __cplusplus
}
#endif

#endif /* SI_SOFTMAX_H_ */
