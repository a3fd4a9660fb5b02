/*
 * si_norm.h -- C-ABI of the normalisation layers whose statistics come from the activation itself: nn.GroupNorm and
 * nn.InstanceNorm2d in eval mode (torch's semantics).  The symbols live in libsi_hip.so beside those of include/si_hip.h; they
 * have a header of their own as include/si_shard.h has.
 *
 * For image n and group g over channels [g * cg, (g + 1) * cg), cg = c / groups:
 *     mean, var  over the h * w * cg elements of (n, g)             (biased variance: divided by the count)
 *     y[n, p, ch] = act( (x[n, p, ch] - mean) * (rsqrt(var + eps) * gamma[ch]) + beta[ch] )
 * affine == 0: gamma = 1, beta = 0 (the pointers are ignored).  nn.InstanceNorm2d is groups == c; GroupNorm(1, c) is the
 * layer norm over (c, h, w).
 *
 * Tensors are NHWC with pixel strides in_ld / out_ld (in elements) on both sides: what lies between two pixels (ld > c) is
 * never read into a statistic and never written.  `in` and `out` must not overlap.
 *
 * Arithmetic: the statistics are fp32 whatever the storage type, by Welford's update per lane and Chan's formula between
 * partials -- the error does not grow with mean^2 / var.  The reduction tree depends on (h, w, c, groups, ld's) only, never on n
 * or on the grid: two launches give the same bits and image i of a batch has the bits of the same image run alone.  No atomics,
 * no host round trip: every launch is safe inside a captured graph.  The fp16 entry rounds once, at the store.
 *
 * Two forms, chosen from the shape (si_hip_groupnorm_kernel_name reports which):
 *   one launch    a workgroup owns a bundle of whole (n, g) slabs of at most 8192 elements, keeps them in LDS between the
 *                 statistics and the store: one read and one write of the tensor, no workspace;
 *   two launches  a statistics pass writes per-slice (mean, M2) partials to workspace[n][slices][groups] (float pairs; the
 *                 slice count comes from h * w alone), an apply pass combines them in a fixed order and normalises.
 *
 * Refused before any device call: null descriptor / tensors, non-positive sizes, groups <= 0 or c % groups != 0, ld < c,
 * affine without gamma or beta, act outside SI_ACT_*, a null workspace when _workspace_bytes > 0 (SI_E_BADARG); n * h * w >= 2^31,
 * element offsets that do not fit 31 bits, n > 65535, a single group wider than 6144 channels (SI_E_UNSUPPORTED).
 */
#ifndef SI_NORM_H_
#define SI_NORM_H_

#include <stddef.h>

#include "si_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct SiGroupNormDesc {
    int n, h, w, c, groups, in_ld, out_ld;
    float eps;
    int affine;      /* 1: gamma and beta are [c] fp32 device arrays */
    int act;         /* SI_ACT_* applied to the normalised value */
    float act_param; /* SI_ACT_LEAKYRELU: the negative slope */
} SiGroupNormDesc;

/* bytes of device workspace the two-launch form needs for this shape; 0: this shape runs in one launch and needs none
 * (also 0 for a descriptor the launch would refuse) */
size_t si_hip_groupnorm_workspace_bytes(const SiGroupNormDesc* d);

int si_hip_groupnorm_f32(const SiGroupNormDesc* d, const float* in, const float* gamma, const float* beta, float* out, void* workspace,
                         si_stream_t stream);

/* half in, half out; statistics, gamma and beta fp32 */
int si_hip_groupnorm_f16(const SiGroupNormDesc* d, const void* in, const float* gamma, const float* beta, void* out, void* workspace,
                         si_stream_t stream);

/* the kernel(s) a launch with these pointers takes: "groupnorm_slab_kernel<float, 4>", or
 * "groupnorm_stats_kernel<float, 4> + groupnorm_apply_kernel<float, 4>"; "none" for a descriptor the launch would refuse */
const char* si_hip_groupnorm_kernel_name(const SiGroupNormDesc* d, const void* in, const void* out, int half);

#ifdef __cplusplus
}
#endif

#endif /* SI_NORM_H_ */
