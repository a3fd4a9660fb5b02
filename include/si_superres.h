/*
 * si_superres.h -- C-ABI of the sub-pixel super-resolution layers: nn.PixelShuffle / F.pixel_shuffle (depth-to-space),
 * nn.PixelUnshuffle / F.pixel_unshuffle (space-to-depth) and nn.PReLU (torch's semantics).  The symbols live in libsi_hip.so beside
 * those of include/si_hip.h; they have a header of their own as include/si_pad.h and include/si_softmax.h have.
 *
 * ---- pixel shuffle --------------------------------------------------------------------------------------------------------
 * The rule, in NHWC with q = i * r + j, 0 <= i, j < r:
 *     shuffle   (inverse = 0)   in [n, h, w, C r r]      -> out [n, h r, w r, C]:   out[n, h r + i, w r + j, c] = in[n, h, w, c r r + q]
 *     unshuffle (inverse = 1)   in [n, h r, w r, C]      -> out [n, h, w, C r r]:   out[n, h, w, c r r + q] = in[n, h r + i, w r + j, c]
 * which is torch.nn.functional.pixel_shuffle / pixel_unshuffle on the NCHW view, bit for bit.  r = 1 is a copy.
 *
 * Tensors are NHWC with pixel strides in_ld >= ic / out_ld >= oc (in elements) on both sides: what lies between two pixels is
 * never read and never written (concat slices, channel-offset views).  `in` and `out` must not overlap.
 *
 * The kernels move bits and do no arithmetic on a value: NaN payloads, -0.0 and denormals come out as they went in.  No atomics,
 * no workspace, no host round trip: every launch is safe inside a captured graph and two launches give the same bits.
 *
 * Forms (si_hip_pixel_shuffle_kernel_name reports which), T = float / _Float16, V = 16 bytes of T (4 / 8):
 *     "pixel_shuffle_elem<T>"     one lane per output element; any c, stride and alignment
 *     "pixel_shuffle_lds<T, V>"   a workgroup reads a run of pixels of one row of the deep ([.., C r r]) tensor, or the r rows of
 *                                 the wide ([.., C]) tensor under it, with 16-byte loads, transposes through LDS and writes whole
 *                                 runs with 16-byte stores; the wide side moves 16-byte channel vectors through LDS (C % V == 0)
 *     "pixel_shuffle_lds<T, 1>"   the same with the wide side gathered element by element in LDS: a dense wide tensor with
 *                                 C % V != 0 (the C = 3 tails of x3 / x4 networks, the 3 -> 12 unshuffle)
 * The LDS form is taken when r >= 2, both pointers are 16-byte aligned, a pixel of the deep tensor is at most 2 KiB, and on each
 * side either the channel count and the stride are multiples of V, or the tensor is dense (ld == c) with a row that is a multiple
 * of V elements.  Otherwise the element form runs.  The 2 KiB limit and the 16 KiB of LDS a workgroup uses are register / LDS
 * budgets nobody measured; whether the LDS form beats the element form on a shape is a matter of measurement, and DESIGN.md
 * section 9g says what has been measured.
 *
 * Refused before any device call: a null descriptor or tensor, non-positive sizes, r < 1, ld < c, shapes inconsistent with the
 * rule -- ic != oc r r, oh != ih r, ow != iw r; for the inverse oc != ic r r, ih % r or iw % r non-zero, oh != ih / r,
 * ow != iw / r (SI_E_BADARG); n * h * w >= 2^31 on either side, element offsets that do not fit 31 bits, n > 65535
 * (SI_E_UNSUPPORTED).
 *
 * ---- PReLU ----------------------------------------------------------------------------------------------------------------
 * y = x > 0 ? x : slope[ch] * x over [pixels, c] with pixel strides; `slope` is an fp32 device vector of slope_count = 1 (shared)
 * or c (per channel) elements.  This is torch's CPU formula: -0.0 and NaN go through the multiply.  The arithmetic is fp32; the
 * fp16 entry rounds once at the store.  16-byte vectors ("prelu_kernel<T, V>") when c, both strides and both pointers allow it,
 * single elements ("prelu_kernel<T, 1>") otherwise.  `in` and `out` may be the same tensor.
 * Refused before any device call: a null pointer, pixels == 0, c <= 0, ld < c, slope_count neither 1 nor c (SI_E_BADARG);
 * element offsets that do not fit 31 bits (SI_E_UNSUPPORTED).
 */
#ifndef SI_SUPERRES_H_
#define SI_SUPERRES_H_

#include "si_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct SiPixelShuffleDesc {
    int n, ih, iw, ic, in_ld, oh, ow, oc, out_ld;
    int r;       /* upscale_factor / downscale_factor */
    int inverse; /* 0: shuffle (depth-to-space), 1: unshuffle (space-to-depth) */
} SiPixelShuffleDesc;

int si_hip_pixel_shuffle_f32(const SiPixelShuffleDesc* d, const float* in, float* out, si_stream_t stream);

/* half in, half out */
int si_hip_pixel_shuffle_f16(const SiPixelShuffleDesc* d, const void* in, void* out, si_stream_t stream);

/* the kernel a launch with these pointers takes (the names above); "none" for a descriptor the launch would refuse */
const char* si_hip_pixel_shuffle_kernel_name(const SiPixelShuffleDesc* d, const void* in, const void* out, int half);

int si_hip_prelu_f32(const float* in, size_t pixels, int c, int in_ld, const float* slope, int slope_count, float* out, int out_ld,
                     si_stream_t stream);

/* half in, half out, fp32 slopes */
int si_hip_prelu_f16(const void* in, size_t pixels, int c, int in_ld, const float* slope, int slope_count, void* out, int out_ld,
                     si_stream_t stream);

/* "prelu_kernel<float, 4>", "prelu_kernel<float, 1>", "prelu_kernel<_Float16, 8>" or "prelu_kernel<_Float16, 1>"; "none" for
 * arguments the launch would refuse (the slope pointer is not looked at) */
const char* si_hip_prelu_kernel_name(const void* in, size_t pixels, int c, int in_ld, int slope_count, const void* out, int out_ld, int half);

#ifdef __cplusplus
}
#endif

#endif /* SI_SUPERRES_H_ */
