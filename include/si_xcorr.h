/*
 * si_xcorr.h -- C-ABI of the cross-correlation kernels behind F.conv2d with a TENSOR filter (torch semantics, zero padding; no reference
 * counterpart).  The symbols live in libsi_hip.so beside those of include/si_hip.h; they have a header of their own as include/si_conv1d.h has.
 *
 *     y[n, oy, ox, o] = act(b[o] + sum over ky, kx, c of x[n, oy sh - pt + ky dh, ox sw - pl + kx dw, c] * w[o, ky, kx, c])
 *
 * Layout.  x, w and y are NHWC views.  Element (n, iy, ix, c) of x lies n x_sn + iy x_sh + ix x_sp + c elements into its tensor, element
 * (n, oy, ox, o) of y n y_sn + oy y_sh + ox y_sp + o: the channels of x and y are contiguous; a channel slice, a crop and a concat member are
 * views.  The filter is read from the tensor AS STORED -- a rank-4 filter [O, C, KH, KW] lies in NHWC storage as [O][KH][KW][C], every
 * filter one K-vector of the implicit GEMM: there is no pack step, no weight image and no workspace.  Its element (i, ky, kx, c) lies
 * i w_sn + ky w_sh + kx w_sp + c w_sc elements into its tensor, where i and c mean, by form:
 *   dense      i = the filter o, c = the input channel of the reduction (w_sc is 1 for a stored filter)
 *   depthwise  c = the channel (= the filter); i = the IMAGE n when per_sample is set, else w_sn is not used: every image meets the same
 *              filters.  Two addressings of the one kernel:
 *                unfused     x [1, H, W, N C], w [N C][kh][kw][1]:  per_sample = 0, w_sc = kh kw ld, w_sp = ld
 *                per-sample  x [N, H, W, C],   w [N][kh][kw][C]:    per_sample = 1, w_sn = kh kw ld, w_sc = 1, w_sp = ld -- filter n meets image n
 * pad_top / pad_left are the near pads; the far pads are implied by ho / wo (torch's padding='same' with an even d (K - 1) pads one more
 * on the far side).  Positions outside the image count as zeros and are never read; a kernel larger than the unpadded image is fine.
 *
 * Forms, chosen by ONE host function that si_hip_xcorr_kernel_name also asks.
 *   dense      groups == 1 (and not c == oc == 1, which the depthwise kernel serves).  D[o, pixel] = W[o, (ky, kx, c)] X[(ky, kx, c), pixel] per image on v_mfma_f32_16x16x4_f32 (fp32) or
 *              v_mfma_f32_16x16x32_f16 (fp16 storage, fp32 accumulation, c % 8 == 0).  The filters are the A operand, the pixels the B
 *              operand, both read straight from global memory: the C/D map then leaves one pixel on the lane and FOUR CONSECUTIVE output
 *              channels in its registers, stored as one 16-byte (fp16: 8-byte) write where y is aligned.  A workgroup of four waves owns 64
 *              output pixels x up to 64 filters of one image, a wave 16 pixels in up to four accumulators of 16 filters: the launch is the
 *              instance with as many tiles as the filters need (O is often 1 .. 20 here), and beyond 64 filters the grid walks blocks of 64.
 *              A lane's fragment is 16 bytes of consecutive channels, one read where x and w are aligned and the channel stride of w is 1.
 *   depthwise  groups == c == oc.  A VALU kernel: a lane owns 16 bytes of consecutive channels of one output pixel (4 floats / 8 halves),
 *              fp32 fmaf for both storage types; 16-byte loads where the channel stride of w is 1 and x, w and y are aligned, one element
 *              path for everything else -- the same arithmetic in the same order.
 *
 * Reduction order, fixed and ascending: two runs give the same bits, and an aligned and a misaligned view of the same data do too.
 *   dense fp32     tap (ky, kx) ascending, then the channel block of 16 (ascending), then four MFMA steps j = 0..3, step j summing the
 *                  channels 4 i + j (i = 0..3) of the block inside one instruction
 *   dense fp16     tap (ky, kx) ascending, then the channel group of 32 (ascending), then the 32 channels inside one MFMA
 *   depthwise      tap (ky, kx) ascending, one fmaf each; a tap outside the image is skipped, not multiplied by zero
 * In the dense form a tap outside the image, and the channels beyond c of the last group, enter as zeros on the x side.  The bias is added
 * to the finished sum, then the activation of SiXcorrDesc::act (the SI_ACT_* codes of include/si_hip.h, act_param the leaky slope).
 *
 * fp16 storage.  x, w and y are halves, the bias is fp32, every sum is fp32; the stored half is ONE round-to-nearest-even of the fp32 result.
 *
 * Contract.  The bits of image n depend on image n alone (and, per-sample, on filter n); the bits of output channel o on filter o and its
 * bias alone -- not on the batch, the other filters or where the filter sits in its tile.  Nothing outside the extents is read or written.
 * Every launch is safe inside a captured graph; the entries never allocate and use no LDS.
 *
 * Refused before any device call.  SI_E_BADARG: a null descriptor, x, w or y; non-positive sizes, negative pads; an ho / wo torch's formula
 * gives for no far pad >= 0; negative strides; strides of y that let two elements share an address; y overlapping x, w or the bias.
 * SI_E_UNSUPPORTED: element offsets beyond 31 bits; a grid extent beyond its limit (n or the filter blocks above 65535); group counts other
 * than 1 and c == oc, per_sample with anything but the depthwise form; the dense fp16 form with c % 8 != 0; pointers not aligned to their element.  (An LDS need beyond what the kernel has
 * would be refused here too: neither kernel has one.)
 */
#ifndef SI_XCORR_H_
#define SI_XCORR_H_

#include "si_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct SiXcorrDesc {
    int n, h, w, c, oc, ho, wo, kh, kw;
    int stride_h, stride_w, dilation_h, dilation_w, pad_top, pad_left, groups;
    long long x_sn, x_sh, x_sp;         /* element strides of the image, the row and the pixel */
    long long w_sn, w_sh, w_sp, w_sc;   /* ... of the filter (depthwise: the image), the tap row, the tap and the channel */
    long long y_sn, y_sh, y_sp;
    int per_sample;                     /* depthwise alone: filter n meets image n (w_sn is then the image stride) */
    int act;                            /* SI_ACT_* */
    float act_param;                    /* SI_ACT_LEAKYRELU: the slope */
} SiXcorrDesc;

/* w: the filter tensor as stored; bias: fp32 [oc] or null */
int si_hip_xcorr_f32(const SiXcorrDesc* d, const float* x, const float* w, const float* bias, float* y, si_stream_t stream);
int si_hip_xcorr_f16(const SiXcorrDesc* d, const void* x, const void* w, const float* bias, void* y, si_stream_t stream);

/* "xcorr_dense_kernel<float>" / "<_Float16>", "xcorr_depthwise_kernel<float>" / "<_Float16>"; "none" for what the launch refuses */
const char* si_hip_xcorr_kernel_name(const SiXcorrDesc* d, const void* x, const void* w, const void* y, int half);

#ifdef __cplusplus
}
#endif

#endif /* SI_XCORR_H_ */
