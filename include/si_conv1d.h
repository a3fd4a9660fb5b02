/*
 * si_conv1d.h -- C-ABI of the temporal convolution kernels behind nn.Conv1d (torch semantics, zero padding; no reference counterpart).  The
 * symbols live in libsi_hip.so beside those of include/si_hip.h; they have a header of their own as include/si_rnn.h has.
 *
 *     y[n, oc, lo] = act(b[oc] + sum over c in the group, k < K of w[oc, c, k] * x[n, c, lo * s - pl + k * d])
 *
 * Layout.  x is [N, C, L] and y is [N, OC, Lo] as the file stores a rank-3 tensor: the positions are the contiguous axis.  Row (n, c) of x
 * starts n * x_sn + c * x_sc elements into its tensor, row (n, oc) of y n * y_sn + oc * y_sc: a channel slice or a crop along L of a wider
 * tensor is a view.  pad_left is the LEFT pad; the right pad is implied by lo (torch's padding='same' with an even d (K - 1) pads one more
 * on the right).  Positions outside [0, L) count as zeros and are never read.
 *
 * Forms, chosen by ONE host function that si_hip_conv1d_kernel_name also asks.
 *   dense      groups == 1 and every grouped case that is not plain depthwise.  D[oc, lo] = W[oc, (c, k)] X[(c, k), lo] per batch item and
 *              group on v_mfma_f32_16x16x4_f32 (fp32) or v_mfma_f32_16x16x32_f16 (fp16 storage, fp32 accumulation, (C / groups) % 8 == 0).
 *              The filters are the A operand, read from the image si_hip_conv1d_pack_weights_* wrote in MFMA lane order; the input rows are
 *              the B operand, staged in LDS; a workgroup of four waves owns 64 output channels x 64 positions of one batch item, a wave 16
 *              channels in four independent accumulators.  The C/D map leaves a position on the lane and four channels in the registers.
 *   depthwise  groups == C == OC.  A VALU kernel: a wave stages the span of one (n, c) row in LDS, a lane produces four consecutive
 *              outputs; fp32 arithmetic (fmaf) for both storage types.  Any K, K > L included.
 *
 * Reduction order, fixed and ascending: two runs give the same bits.
 *   dense fp32     channel group of 4 (ascending), then tap k (ascending), then the 4 channels inside one MFMA
 *   dense fp16     channel group of 32 (ascending), then tap k (ascending), then the 32 channels inside one MFMA
 *   depthwise      tap k ascending, one fmaf each
 * The channels of a group are zero-padded to the instruction's k, in the image and in LDS.  The bias is added to the finished sum, then the
 * activation of SiConv1dDesc::act (the SI_ACT_* codes of include/si_hip.h, act_param the leaky slope) is applied; there is no residual operand.
 *
 * fp16 storage.  x, y and the weight image are halves, the bias is fp32, every sum is fp32; the stored half is ONE round-to-nearest-even of
 * the fp32 result.  Any L, any OC, any 2-byte aligned row; the image is 16-byte aligned.
 *
 * Contract.  The bits of batch item n depend on that item's data alone, the bits of output channel oc on that channel's filter and bias
 * alone -- not on the batch, on the other filters or on where the channel sits in its tile.  Nothing beyond the extents is read or written:
 * of y exactly the lo positions of every row, the space between rows is untouched.  Every launch is safe inside a captured graph; the entries
 * never allocate.
 *
 * Refused before any device call: a null descriptor, x, weight image or y; non-positive sizes, a negative pad_left; groups that do not
 * divide c and oc; an lo that torch's formula gives for no right pad >= 0; a stride below the row width (x_sc < l, y_sc < lo) or batch items
 * that share a row; y overlapping x, the weight image or the bias (SI_E_BADARG); element offsets beyond 31 bits, a grid extent beyond its
 * limit (n, groups, output-channel blocks or channels / 4 above 65535), a tile's span beyond the 64 KB of LDS, an unaligned fp16 image, and
 * for the dense fp16 form (c / groups) % 8 != 0 (SI_E_UNSUPPORTED).
 */
#ifndef SI_CONV1D_H_
#define SI_CONV1D_H_

#include "si_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct SiConv1dDesc {
    int n, c, l, oc, lo, k, stride, dilation, pad_left, groups;
    long long x_sn, x_sc;   /* element strides of the batch index and of the channel row */
    long long y_sn, y_sc;
    int act;                /* SI_ACT_* */
    float act_param;        /* SI_ACT_LEAKYRELU: the slope */
} SiConv1dDesc;

/* weights: the image of si_hip_conv1d_pack_weights_*; bias: fp32 [oc] or null */
int si_hip_conv1d_f32(const SiConv1dDesc* d, const float* x, const float* weights, const float* bias, float* y, si_stream_t stream);
int si_hip_conv1d_f16(const SiConv1dDesc* d, const void* x, const void* weights, const float* bias, void* y, si_stream_t stream);

/* bytes of the weight image of a storage type; 0 for a refused descriptor */
size_t si_hip_conv1d_weight_bytes(const SiConv1dDesc* d, int half);

/* host: w fp32 [oc][c / groups][k] (torch's weight) -> the image, si_hip_conv1d_weight_bytes bytes.  Only c, oc, k and groups are read. */
int si_hip_conv1d_pack_weights_f32(const SiConv1dDesc* d, const float* w, float* image);
int si_hip_conv1d_pack_weights_f16(const SiConv1dDesc* d, const float* w, void* image);

/* "conv1d_dense_kernel<float>" / "<_Float16>", "conv1d_depthwise_kernel<float>" / "<_Float16>"; "none" for what the launch refuses */
const char* si_hip_conv1d_kernel_name(const SiConv1dDesc* d, const void* x, const void* y, int half);

#ifdef __cplusplus
}
#endif

#endif /* SI_CONV1D_H_ */
