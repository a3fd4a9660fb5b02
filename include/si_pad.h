/*
 * si_pad.h -- C-ABI of the explicit 2-D padding layers: nn.ReflectionPad2d, nn.ReplicationPad2d, nn.ZeroPad2d,
 * nn.ConstantPad2d, nn.CircularPad2d and F.pad on the last two dimensions (torch's semantics).  The symbols live in
 * libsi_hip.so beside those of include/si_hip.h; they have a header of their own as include/si_norm.h and include/si_shard.h have.
 *
 * The rule is per axis and independent in H and W.  On the W axis of size iw with left pad pl, output column o reads source
 * column i = o - pl:
 *     SI_PAD_CONSTANT    x[i] if 0 <= i < iw, else `value`
 *     SI_PAD_REPLICATE   x[clamp(i, 0, iw - 1)]
 *     SI_PAD_REFLECT     i < 0 -> -i;  i > iw - 1 -> 2 (iw - 1) - i      (the edge is not repeated)
 *     SI_PAD_CIRCULAR    x[i mod iw]
 * A negative pad crops.  Accepted: oh = ih + pad_t + pad_b >= 1 and ow = iw + pad_l + pad_r >= 1, equal to the descriptor's
 * oh / ow; after cropping at least one row and one column remain (iw + min(pad_l, 0) + min(pad_r, 0) >= 1, the same for H);
 * reflect: max(pad_l, pad_r) < iw and max(pad_t, pad_b) < ih; circular: no negative pad, max(pad_l, pad_r) <= iw and
 * max(pad_t, pad_b) <= ih.  On this set the rule is torch.nn.functional.pad bit for bit.  torch accepts a little more
 * (circular with negative pads, constant crops that leave nothing) with results that are not this rule: those are refused.
 *
 * Tensors are NHWC with pixel strides in_ld / out_ld (in elements) on both sides: what lies between two pixels (ld > c) is
 * never read and never written.  `in` and `out` must not overlap.
 *
 * The kernel moves bits and does no arithmetic on a value: NaN payloads, -0.0 and denormals come out as they went in.  The
 * fp16 entry rounds the constant `value` once to half, round-to-nearest-even.  No LDS, no atomics, no workspace, no host
 * round trip: every launch is safe inside a captured graph and two launches give the same bits.
 *
 * Two forms (si_hip_pad2d_kernel_name reports which): 16-byte channel vectors (4 floats / 8 halves) when c, both strides and
 * both pointers allow it, single elements otherwise.
 *
 * Refused before any device call: a null descriptor or tensor, non-positive sizes, ld < c, a mode outside 0..3, oh / ow
 * inconsistent with the pads (SI_E_BADARG); the per-mode limits above, n * oh * ow >= 2^31, element offsets that do not fit
 * 31 bits, n > 65535 (SI_E_UNSUPPORTED).
 */
#ifndef SI_PAD_H_
#define SI_PAD_H_

#include "si_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { SI_PAD_CONSTANT = 0, SI_PAD_REFLECT = 1, SI_PAD_REPLICATE = 2, SI_PAD_CIRCULAR = 3 };

typedef struct SiPad2dDesc {
    int n, ih, iw, c, in_ld, oh, ow, out_ld;
    int pad_l, pad_r, pad_t, pad_b; /* may be negative: crop */
    int mode;                       /* SI_PAD_* */
    float value;                    /* SI_PAD_CONSTANT only */
} SiPad2dDesc;

int si_hip_pad2d_f32(const SiPad2dDesc* d, const float* in, float* out, si_stream_t stream);

/* half in, half out */
int si_hip_pad2d_f16(const SiPad2dDesc* d, const void* in, void* out, si_stream_t stream);

/* the kernel a launch with these pointers takes: "pad2d_kernel<float, 4>", "pad2d_kernel<float, 1>", "pad2d_kernel<_Float16, 8>"
 * or "pad2d_kernel<_Float16, 1>"; "none" for a descriptor the launch would refuse */
const char* si_hip_pad2d_kernel_name(const SiPad2dDesc* d, const void* in, const void* out, int half);

#ifdef __cplusplus
}
#endif

#endif /* SI_PAD_H_ */
