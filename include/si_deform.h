/*
 * si_deform.h -- C-ABI of deformable convolution (torchvision.ops.deform_conv2d: DCNv1 without a mask, DCNv2 with one), the kernel behind
 * torchvision.ops.DeformConv2d (torch semantics, no reference counterpart).  The symbols live in libsi_hip.so beside those of
 * include/si_hip.h; they have a header of their own as include/si_attention.h and include/si_norm.h have.
 *
 * Operands (NHWC, fp32):  x [n, ih, iw, ic]   offset [n, oh, ow, 2 og kh kw]   mask [n, oh, ow, og kh kw] (optional)   out [n, oh, ow, oc]
 * with og = offset_groups, oh = (ih + 2 ph - dh (kh - 1) - 1) / sh + 1 and likewise ow.  For offset group g and tap (i, j) the offset channel
 * 2 (g kh kw + i kw + j) is dy, the next one dx, and the mask channel is g kh kw + i kw + j; input channel c belongs to offset group
 * c / (ic / og) and to weight group c / (ic / groups).
 *
 *     y = float(ho sh - ph + i dh) + dy                  (one fp32 addition; likewise x)
 *     sample(c) = NaN                                     if y or x is NaN (no address is formed from it)
 *               = 0                                       unless y > -1 and y < ih and x > -1 and x < iw (so +-Inf gives 0)
 *               else, hl = floor(y), wl = floor(x), lh = y - hl, lw = x - wl, hh = 1 - lh, hw = 1 - lw:
 *                 (hh hw) X[hl, wl] + (hh lw) X[hl, wl + 1] + (lh hw) X[hl + 1, wl] + (lh lw) X[hl + 1, wl + 1]      summed in this order
 *                 a corner outside the image contributes exactly 0 and is never read; a corner inside is multiplied by its weight even when
 *                 the weight is 0 (0 * Inf is NaN, as in torch); the conversion to an integer happens only after the range test
 *     col(c, i, j) = mask * sample(c)                     (no mask: sample(c))
 *     out[n, ho, wo, co] = act( bias[co] + sum over the channels c of co's weight group and the taps of  W[co, c_local, i, j] col(c, i, j) )
 *
 * Views.  Each of x, offset, mask, out is a set of pixels of `c` channels whose pixels are in_ld / off_ld / mask_ld / out_ld elements
 * apart.  The kernel reads and writes only the c channels of each view: what lies between two pixels' channels is neither read nor
 * written.  The extent of `out` (first to last element) must not intersect the extent of an input.
 *
 * Kernel.  An implicit GEMM on v_mfma_f32_32x32x2_f32 (exact fp32, a k-ordered fma chain) whose A operand is produced by the bilinear gather:
 * M = n oh ow pixels, N = oc / groups, K = kh kw (ic / groups) tap-major with the channels inside; 64 x 64 tiles, four waves, the weight
 * group on a grid dimension.  One launch, no workspace, no atomics; exactly one lane stores each output element, once: two launches give
 * the same bits, the bits of an output pixel depend on that pixel's operands alone (not on n or on its position in a tile), and the launch
 * is safe inside a captured graph.  Two arms: 16-byte corner loads when ic, in_ld, ic / groups and ic / og are multiples of 4 and x is
 * 16-byte aligned, scalar loads otherwise.
 *
 * Refused before any device call: a null descriptor or tensor (mask with has_mask, bias with has_bias), non-positive sizes, ic or oc no
 * multiple of groups, ic no multiple of offset_groups, oh / ow that disagree with the formula, a stride below its channel count, `out`
 * intersecting an input (SI_E_BADARG); an activation outside SI_ACT_*, element offsets or a workgroup count beyond 31 bits
 * (SI_E_UNSUPPORTED).
 */
#ifndef SI_DEFORM_H_
#define SI_DEFORM_H_

#include "si_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct SiDeformConv2dDesc {
    int n, ih, iw, ic, in_ld;
    int oh, ow, oc, out_ld;
    int off_ld, mask_ld;   /* pixel strides of offset and mask (mask_ld is not looked at without has_mask) */
    int kh, kw, sh, sw, ph, pw, dh, dw;
    int groups, offset_groups;
    int has_mask, has_bias;
    int act;               /* SI_ACT_* */
    float act_param;       /* the slope of SI_ACT_LEAKYRELU */
} SiDeformConv2dDesc;

/* elements of the kernel's weight image: [kh][kw][oc][ic / groups rounded up to 4]; 0 for sizes the kernel refuses */
size_t si_hip_deform_conv2d_weight_elems(const SiDeformConv2dDesc* d);

/* torch's [oc][ic / groups][kh][kw] -> the kernel's image (host only) */
int si_hip_deform_conv2d_pack_weight_host(const SiDeformConv2dDesc* d, const float* w_oihw, float* w_packed);

int si_hip_deform_conv2d_f32(const SiDeformConv2dDesc* d, const float* x, const float* offset, const float* mask_or_null, const float* w_packed,
                             const float* bias_or_null, float* out, si_stream_t stream);

/* the kernel a launch with these pointers takes: "deform_conv_f32_kernel<true>" (16-byte corner loads) or "deform_conv_f32_kernel<false>"
 * (scalar loads); "none" for a descriptor or pointers the launch would refuse */
const char* si_hip_deform_conv2d_kernel_name(const SiDeformConv2dDesc* d, const void* x, const void* offset, const void* mask_or_null, const void* out);

#ifdef __cplusplus
}
#endif

#endif /* SI_DEFORM_H_ */
