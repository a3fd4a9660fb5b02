/*
 * si_slice.h -- C-ABI of the operators that take part of a tensor: torch.chunk, torch.split and Tensor.slice (torch semantics, no
 * reference counterpart).  The symbols live in libsi_hip.so beside those of include/si_hip.h; they have a header of their own as
 * include/si_pad.h and include/si_superres.h have.
 *
 * Tensors are NHWC with pixel strides in_ld >= ic / out_ld >= oc (in elements): what lies between two pixels is never read and never
 * written (concat slices, channel-offset views).  Source and destinations must not overlap.
 *
 * The kernels move bits -- 4-byte words for fp32, 2-byte words for fp16 -- and do no arithmetic on a value: NaN payloads, -0.0 and
 * denormals come out as they went in.  No atomics, no workspace, no host round trip: every launch is safe inside a captured graph
 * and two launches give the same bits.  Both kernels are grid-stride loops over the output (at most 2048 workgroups of 256 lanes).
 *
 * ---- strided slice --------------------------------------------------------------------------------------------------------
 *     out[n, h, w, c] = in[start[0] + n step[0], start[1] + h step[1], start[2] + w step[2], start[3] + c step[3]]
 * for 0 <= (n, h, w, c) < (on, oh, ow, oc); start[] and step[] are in NHWC order, every step >= 1.
 * Forms (si_hip_slice_kernel_name reports which), T = float / _Float16, V = 16 bytes of T (4 / 8):
 *     "slice_vec<T, V>"   16-byte loads and stores: step[3] == 1, and start[3], oc, in_ld, out_ld multiples of V, both pointers
 *                         16-byte aligned
 *     "slice_elem<T>"     one element per lane: everything else (channel steps, C = 3 images, odd strides)
 * Refused before any device call: a null descriptor or tensor, non-positive sizes, ld < c, a step < 1, a negative start, an output
 * extent whose last index start + (o - 1) step leaves the input (SI_E_BADARG); n > 65535, n h w >= 2^31 on either side, element
 * offsets that do not fit 31 bits (SI_E_UNSUPPORTED).
 *
 * ---- channel split --------------------------------------------------------------------------------------------------------
 * k destinations, destination i receiving channels [offsets[i], offsets[i] + widths[i]) of every input pixel at its own pointer and
 * pixel stride out_lds[i]:   dsts[i][p, c] = src[p, offsets[i] + c].   One launch serves up to SI_SPLIT_MAX destinations and reads
 * each of their input vectors once; for more the launcher loops.
 * Forms (si_hip_split_channels_kernel_name), chosen once over ALL k destinations:
 *     "split_vec<T, V>"   in_ld, every offset, width and out_ld multiples of V, all pointers 16-byte aligned
 *     "split_elem<T>"     everything else
 * Refused before any device call: a null pointer (the arrays, the source, any destination), pixels == 0, c <= 0, in_ld < c, k < 1,
 * a width < 1, an offset < 0, offset + width > c, out_ld < width (SI_E_BADARG); pixels >= 2^31, element offsets or a launch's item
 * count that do not fit 31 bits (SI_E_UNSUPPORTED).
 */
#ifndef SI_SLICE_H_
#define SI_SLICE_H_

#include "si_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SI_SPLIT_MAX 8 /* destinations of one split launch */

typedef struct SiSliceDesc {
    int n, ih, iw, ic, in_ld;
    int start[4]; /* NHWC order */
    int step[4];  /* NHWC order, each >= 1 */
    int on, oh, ow, oc, out_ld;
} SiSliceDesc;

int si_hip_slice_f32(const SiSliceDesc* d, const void* src, void* dst, si_stream_t stream);

/* half in, half out */
int si_hip_slice_f16(const SiSliceDesc* d, const void* src, void* dst, si_stream_t stream);

/* the kernel a launch with these pointers takes (the names above); "none" for a descriptor the launch would refuse */
const char* si_hip_slice_kernel_name(const SiSliceDesc* d, const void* src, const void* dst, int half);

int si_hip_split_channels_f32(const void* src, size_t pixels, int c, int in_ld, int k, const int* offsets, const int* widths,
                              void* const* dsts, const int* out_lds, si_stream_t stream);

/* half in, half out */
int si_hip_split_channels_f16(const void* src, size_t pixels, int c, int in_ld, int k, const int* offsets, const int* widths,
                              void* const* dsts, const int* out_lds, si_stream_t stream);

/* "split_vec<float, 4>", "split_elem<float>", "split_vec<_Float16, 8>" or "split_elem<_Float16>"; "none" for arguments the launch
 * would refuse */
const char* si_hip_split_channels_kernel_name(const void* src, size_t pixels, int c, int in_ld, int k, const int* offsets,
                                              const int* widths, void* const* dsts, const int* out_lds, int half);

#ifdef __cplusplus
}
#endif

#endif /* SI_SLICE_H_ */
