/*
 * si_pool.h -- C-ABI of the window-mean layers: nn.AvgPool2d / F.avg_pool2d and the general (non-divisible) case of
 * nn.AdaptiveAvgPool2d / F.adaptive_avg_pool2d, torch's semantics.  The symbols live in libsi_hip.so beside those of
 * include/si_hip.h; they have a header of their own as include/si_norm.h and include/si_pad.h have.  (The divisible adaptive shapes
 * keep si_hip_adaptive_avgpool2d_f32 / _f16 of si_hip.h and their bits.)
 *
 * Windows, per axis and independent in H and W (size i, kernel k, stride s, pad p on both sides):
 *     o = floor_or_ceil((i + 2p - k) / s) + 1; with the ceiling, o is decremented when (o - 1) s >= i + p (the last window starts
 *     inside the input or its left pad).  The descriptor carries oh / ow: either rounding is accepted, which is how ceil_mode travels.
 *     Output j covers [a, b), a = j s - p, b = min(a + k, i + p); its padded extent is b - a; it is clipped to [max(a, 0), min(b, i)).
 *     adaptive = 1: [floor(j i / o), ceil((j + 1) i / o)) for any oh, ow >= 1 (o > i pools "up"); kh .. pl are ignored.
 * Divisor: divisor_override if non-zero; else the product of the two padded extents when count_include_pad, of the two clipped extents
 * otherwise; adaptive windows always use the clipped extents.
 * Accepted: k, s >= 1 and 0 <= p <= k / 2 (torch refuses more: SI_E_UNSUPPORTED); every clipped window is then non-empty.  No dilation.
 *
 * Tensors are NHWC with pixel strides in_ld / out_ld (in elements) on both sides: what lies between two pixels (ld > c) is
 * never read and never written.  `in` and `out` must not overlap.
 *
 * Two forms, chosen from the shape alone (never from n): si_hip_avgpool2d_kernel_name reports which.
 *   windowed     the largest window of the launch has fewer than SI_AVGPOOL_COOP_TAPS taps.  One lane per (output pixel, 16-byte
 *                channel vector).  Arithmetic: the clipped window's elements are added in float32, row by row and left to right,
 *                starting from +0.0f; one IEEE division by (float)divisor; no contraction.  The fp16 entry reads halves, does the
 *                same in float32 and rounds once, to nearest even, at the store.  On finite data this is bit for bit what torch's CPU
 *                kernels give for float32 and half tensors.
 *   cooperative  larger windows.  A workgroup owns one output pixel and a chunk of channels; its thread groups stride over the
 *                window's taps in row-major order (group g takes taps g, g + G, ...), each adding its taps in float32 from +0.0f; the G
 *                partial sums are added in LDS in the order g = 0 .. G - 1; one IEEE division; one rounding for fp16.  G is 16 (float
 *                vectors), 32 (half vectors) or 4 (single elements): the order of additions is a function of the window's extents and
 *                the vector width only.
 * Either way: no atomics, no workspace, no host round trip; two launches give the same bits, image i of a batch has the bits of that
 * image run alone, and every launch is safe inside a captured graph.  16-byte channel vectors (4 floats / 8 halves) when c, both
 * strides and both pointers allow it, single elements otherwise.
 *
 * Refused before any device call: a null descriptor or tensor, non-positive sizes, ld < c, k or s < 1, p < 0, oh / ow that is neither
 * rounding of the rule (SI_E_BADARG); p > k / 2, n > 65535, n * oh * ow or n * ih * iw >= 2^31, element offsets that do not fit 31 bits,
 * ih * oh or iw * ow >= 2^31 for adaptive windows (SI_E_UNSUPPORTED).
 */
#ifndef SI_POOL_H_
#define SI_POOL_H_

#include "si_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the form switch: a launch whose largest window has at least this many taps takes the cooperative form */
enum { SI_AVGPOOL_COOP_TAPS = 256 };

typedef struct SiAvgPool2dDesc {
    int n, ih, iw, c, in_ld, oh, ow, out_ld;
    int kh, kw, sh, sw, pt, pl; /* ignored when adaptive */
    int adaptive;               /* 1: torch's adaptive windows from (ih, iw) -> (oh, ow) */
    int count_include_pad;
    int divisor_override;       /* 0 = none */
} SiAvgPool2dDesc;

int si_hip_avgpool2d_f32(const SiAvgPool2dDesc* d, const float* in, float* out, si_stream_t stream);

/* half in, half out */
int si_hip_avgpool2d_f16(const SiAvgPool2dDesc* d, const void* in, void* out, si_stream_t stream);

/* the kernel a launch with these pointers takes: "avgpool2d_window_kernel<T, VW>" or "avgpool2d_coop_kernel<T, VW>" with <float, 4>,
 * <float, 1>, <_Float16, 8> or <_Float16, 1>; "none" for a descriptor the launch would refuse */
const char* si_hip_avgpool2d_kernel_name(const SiAvgPool2dDesc* d, const void* in, const void* out, int half);

#ifdef __cplusplus
}
#endif

#endif /* SI_POOL_H_ */
