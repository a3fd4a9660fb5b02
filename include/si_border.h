/*
 * si_border.h -- C-ABI of the border-mapped convolution behind nn.Conv2d(padding_mode = "reflect" | "replicate" | "circular") (torch's
 * semantics; the reference pads with zeros in every mode).  The symbols live in libsi_hip.so beside those of include/si_hip.h; they have a
 * header and a descriptor of their own as include/si_xcorr.h and include/si_conv1d.h have.
 *
 *     y[n, oy, ox, o] = act2(act1(b[o] + sum over ky, kx, c of x[n, my(oy sh - pt + ky dh), mx(ox sw - pl + kx dw), c] * w[o, c, ky, kx]) + r[n, oy, ox, o])
 *
 * which is torch's conv2d(F.pad(x, (pl, pl, pt, pt), mode), w, b, stride, 0, dilation): an out-of-image tap reads the MAPPED source pixel
 * instead of zero, in one launch, with no padded copy of the activation in memory.  With i the unclamped source coordinate and n the
 * extent, the map m is the rule of include/si_pad.h, per axis:
 *     SI_PAD_REPLICATE   clamp(i, 0, n - 1)                              any pad
 *     SI_PAD_REFLECT     i < 0 -> -i;  i > n - 1 -> 2 (n - 1) - i        pad <= n - 1 (torch raises otherwise)
 *     SI_PAD_CIRCULAR    i < 0 -> i + n;  i > n - 1 -> i - n             pad <= n     (torch raises otherwise)
 * The preconditions make ONE fold enough: compares and adds only, no division.  si_hip_conv2d_border_source_index is that function on the
 * host -- the kernel's tables are built from the same inline function -- so the map is checked without a device.  SI_PAD_CONSTANT is not a
 * mode of this header: a zero-padded convolution is include/si_hip.h's.
 *
 * Scope.  Dense convolutions (groups == 1) on the matrix cores: fp32 on v_mfma_f32_16x16x4_f32 for any channel counts; fp16 storage on
 * v_mfma_f32_16x16x32_f16 with fp32 accumulation, ic % 8 == 0.  Tensors are NHWC with pixel strides in_ld / out_ld / res_ld (elements):
 * what lies between two pixels is never read and never written, so a channel slice of a concat buffer is a view on either side.
 *
 * Work split.  A workgroup of four waves owns SI_BORDER_TH x SI_BORDER_TW output pixels x SI_BORDER_OC output channels of one image; wave
 * w owns row w of the tile: its 16 lanes x are 16 CONSECUTIVE output pixels, its accumulators up to four 16-filter MFMA tiles (the launch
 * is the instance with as many tiles as the filters need).  The filters are the A operand, the pixels the B operand: a lane ends with four
 * consecutive output channels of one pixel, stored as one 16-byte (fp16: 8-byte) write where y is aligned.
 *
 * Tables.  The map is separable.  The workgroup first writes ymap[PH] and xmap[PW] to LDS, PH = (TH - 1) sh + (kh - 1) dh + 1 and PW
 * likewise: the mapped source row / column of every patch row / column (rows and columns that only dead outputs of a ragged tile would
 * read are clamped into the image).  The map is paid once per staged pixel, not once per tap.
 *
 * Staging.  Per chunk of SI_BORDER_KC input channels the patch [PH][PW][KC] is staged global -> LDS through the tables: 16-byte loads
 * where the base, in_ld and ic allow it, single elements with the same arithmetic otherwise.  Every staged pixel exists in the image: there
 * is no zero-fill arm; the only zeros are the channels beyond ic of the last chunk.  All kh x kw taps then read their B fragments from the
 * patch.  The A fragments (16 bytes of consecutive channels of one filter and tap) come straight from GLOBAL memory (L2): a workgroup reads
 * each once per chunk and tap, and the weight image of a layer is small next to L2.
 *
 * LDS layout.  Pixel pitch = KC + SI_BORDER_PAD_F32 floats = 36 words = 9 sixteen-byte slots (fp16: KC + SI_BORDER_PAD_F16 halves = 80
 * bytes = 5 slots).  The LDS array is 64 banks of 4 bytes, and a 16-byte read is served 16 lanes at a time, a lane taking one slot of four
 * banks: the 16 lanes of a group are free of conflicts when their slot numbers differ modulo 16.  Those lanes are the consecutive output
 * pixels of a wave at one tap and one channel offset, so their addresses are (a constant) + x * (distance of two neighbours in slots).
 * The patch columns are stored PHASE-MAJOR: column p lies at position (p mod sw) * CW + p / sw, CW = ceil(PW / sw).  The columns a tap
 * reads, ox sw + kx dw, share one phase, so neighbours are ONE position = 9 (5) slots apart at every stride, and x * 9 mod 16 (x * 5 mod
 * 16) takes 16 different values for x = 0..15: an odd pitch in slots is all that is needed.  (Column-major order would put neighbours
 * 9 sw slots apart: a two-way conflict at every even stride.)  The position of kx's first column is one more small table, kpos[kw].
 * The staging WRITES are not free of conflicts, and are left so: 16 consecutive threads store the 8 (fp16: 4) vectors of 2 (4) neighbouring
 * pixels, slots 9 p + v, v = 0..7, p and p + 1 (5 p + v, v = 0..3, p .. p + 3); slot 9 p + 16 meets slot 9 p (fp16: 5 p + 16, 17, 18 meet
 * 5 p, 5 p + 1, 5 p + 2): one two-way conflict per fp32 group of 16 stores, three per fp16 group.  A pixel is written once per chunk and read
 * kh kw times, so the pitch is chosen for the reads.
 *
 * Weights.  One image for both types: [oc][kh][kw][icp], icp = ic rounded up to the fragment (4 floats / 8 halves), zero filled, floats
 * for the fp32 kernel and halves (one round-to-nearest-even of the fp32 weight) for the fp16 kernel: si_hip_conv2d_border_weight_elems /
 * _pack_weight_host.  (A deliberate departure from the plan this kernel was built to, which had the fp32 path read the image of
 * si_hip_conv2d_pack_weight_host.  That image is not reused: its K order is one of three -- transposed for
 * 1..3 input channels, channel-block-major for ic % 32 == 0, tap-major otherwise -- by rules that belong to those kernels.)
 *
 * Reduction order, fixed: channel chunk of KC ascending; inside a chunk the tap (ky, kx) ascending; inside a tap, fp32: the channel block
 * of 16 ascending, then four MFMA steps j = 0..3, step j summing the channels 4 i + j (i = 0..3) of the block inside one instruction;
 * fp16: the 32 channels of the chunk inside one MFMA.  Two runs give the same bits.  The bits of image n depend on image n alone; the bits of
 * output channel o depend on filter o and its bias alone -- not on the batch, the other filters or where the filter sits in its tile.
 * The bias is added to the finished sum, then act1, the residual, act2 (the SI_ACT_* codes of include/si_hip.h).
 *
 * fp16 storage.  x, w, the residual and y are halves, the bias is fp32, every sum is fp32; the stored half is ONE round-to-nearest-even of
 * the fp32 result.
 *
 * Limits.  The patch and the tables must fit SI_BORDER_LDS_BYTES: a patch that does not (large dilated kernels at a stride) runs with 2 or 1
 * of the tile's rows live; one that still does not fit is SI_E_UNSUPPORTED.  Every launch is safe inside a captured graph; the entries
 * never allocate.
 *
 * Refused before any device call.  SI_E_BADARG: a null descriptor, x, w or y (a bias or residual the descriptor asks for); non-positive
 * sizes, negative pads, ld < c; a mode other than the three; oh / ow that are not torch's for pads (pt, pt) and (pl, pl); y overlapping x, w
 * or the bias (the residual may be y itself: an element is read by the lane that writes it).  SI_E_UNSUPPORTED: pads beyond the table
 * above; groups != 1; fp16 with ic % 8 != 0; element offsets beyond 31 bits; a grid extent beyond its limit (n or the filter blocks above
 * 65535); pointers not aligned to their element; a patch beyond LDS.
 */
#ifndef SI_BORDER_H_
#define SI_BORDER_H_

#include "si_hip.h"
#include "si_pad.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
    SI_BORDER_TH = 4,          /* output rows of a workgroup's tile: one per wave */
    SI_BORDER_TW = 16,         /* output columns: the 16 pixel lanes of an MFMA tile */
    SI_BORDER_OC = 64,         /* output channels of a workgroup: four MFMA tiles of 16 filters */
    SI_BORDER_KC = 32,         /* input channels of one staged chunk */
    SI_BORDER_PAD_F32 = 4,     /* floats behind the KC of a staged pixel: pitch 36 words = 9 slots */
    SI_BORDER_PAD_F16 = 8,     /* halves behind the KC of a staged pixel: pitch 80 bytes = 5 slots */
    SI_BORDER_LDS_BYTES = 65536,
    SI_BORDER_REFUSED = -1     /* si_hip_conv2d_border_source_index outside the preconditions */
};

typedef struct SiBorderConvDesc {
    int n, ih, iw, ic, in_ld;
    int oh, ow, oc, out_ld;
    int kh, kw, sh, sw, dh, dw;
    int pt, pl;         /* the pad of both sides of H / of W */
    int mode;           /* SI_PAD_REFLECT, SI_PAD_REPLICATE or SI_PAD_CIRCULAR */
    int groups;         /* 1 */
    int has_bias;
    int act1;           /* applied to conv + bias */
    int has_residual;   /* residual [n, oh, ow, oc] with pixel stride res_ld */
    int res_ld;
    int act2;           /* applied after the residual add */
    float act_param;    /* leaky-relu slope */
} SiBorderConvDesc;

/* 1: the launch would run (descriptor alone: sizes, mode and pads, channel rule, extents, grid, LDS); 0 otherwise */
int si_hip_conv2d_border_supported(const SiBorderConvDesc* d, int half);

/* elements of the weight image / the image of a torch [oc][ic][kh][kw] fp32 weight: floats (half == 0) or halves */
size_t si_hip_conv2d_border_weight_elems(const SiBorderConvDesc* d, int half);
int si_hip_conv2d_border_pack_weight_host(const SiBorderConvDesc* d, const float* w_oihw, void* w_packed, int half);

int si_hip_conv2d_border_f32(const SiBorderConvDesc* d, const float* in, const float* w_packed, const float* bias, const float* residual,
                             float* out, si_stream_t stream);
int si_hip_conv2d_border_f16(const SiBorderConvDesc* d, const void* in, const void* w_packed, const float* bias, const void* residual,
                             void* out, si_stream_t stream);

/* "conv_border_kernel<float>" / "conv_border_kernel<_Float16>"; "none" for what the launch refuses */
const char* si_hip_conv2d_border_kernel_name(const SiBorderConvDesc* d, const void* in, const void* out, int half);

/* host only: the source index of unclamped coordinate i on an axis of extent n, or SI_BORDER_REFUSED outside the mode's precondition
 * (reflect: -(n - 1) <= i <= 2 (n - 1); circular: -n <= i <= 2 n - 1), for another mode or n <= 0 */
int si_hip_conv2d_border_source_index(int mode, int i, int n);

#ifdef __cplusplus
}
#endif

#endif /* SI_BORDER_H_ */
