/*
 * si_imgmask.h -- C-ABI of the image-size instance masks: the product of coefficients and prototypes, the bilinear upsample to the network or
 * the source frame, the crop and the threshold in one kernel (ultralytics' process_mask(upsample=True), process_mask_native / scale_masks,
 * retina_masks=True).  The symbols live in libsi_hip.so beside those of include/si_detect.h; a header of its own as include/si_obb.h has.
 *
 * ---- si_hip_detect_image_masks_f32 ----
 * Inputs.  protos [n][mh][mw][nm] with pixels proto_ld >= nm elements apart, extras [n][max_det][extra] with the coefficients of detection d at
 * extras[b][d][coef_off .. coef_off + nm), counts [n]: exactly as si_hip_detect_masks_f32 (include/si_detect.h) reads them, the buffers
 * si_hip_detect_postprocess_f32 left on the device go in unchanged.  boxes [n][max_det] rows of box_ld >= 4 floats {x, y, w, h, ...} (the dets
 * rows of the post-processing pass as they are); their frame depends on `crop`.  geom [n][6] int32, per image
 *     {win_x0, win_y0, win_w, win_h, out_w, out_h}
 * the window is the part of the prototype plane that maps onto the output (the letterbox padding cut off as scale_masks cuts it), out_w <= OW
 * and out_h <= OH the image's own output size.  The whole plane as the window and the network size as the output give the network-frame
 * mask; the un-padded window and the source size give the source-frame mask.  The caller forms the record on the host.
 *
 * Output.  masks [n][max_det][OH][OW] bytes.  For d < min(counts[b], max_det) the whole plane is written, bytes outside out_h x out_w as 0;
 * planes behind that are not touched.
 *
 * The rule, in fp32, every operation rounded on its own (no fused multiply-add except the one named):
 *   logit of a prototype pixel   L(py, px) = (((0 + c0 p0) + c1 p1) + ...) in index order: the dot of si_hip_detect_masks_f32, bit for bit.
 *   taps of output column c      step = (float)win_w / (float)out_w,  src = max(0, fmaf(step, (float)c + 0.5f, -0.5f)),
 *                                i0 = min((int)src, win_w - 1),  i1 = i0 + (i0 < win_w - 1),  l1 = src - (float)i0,  l0 = 1 - l1
 *                                (the project's bilinear rule for align_corners=False with size=, include/si_hip.h "Upsample", applied INSIDE
 *                                the window: the clamps are against the window's edges, the prototype pixel is win_x0 + i).  Rows likewise
 *                                with win_h, out_h.
 *   logit of an output pixel     top = (l0w * v00) + (l1w * v01),  bot = (l0w * v10) + (l1w * v11),  v = (l0h * top) + (l1h * bot)
 *                                with v00 = value at (row i0h, column i0w), v01 at (i0h, i1w), v10 at (i1h, i0w), v11 at (i1h, i1w): the
 *                                order of the bilinear kernel, its three fused operations written as a product and a sum each.
 *   box                          x1 = x, x2 = x + w, y1 = y, y2 = y + h;  pass(r, c) = (float)c >= x1 && (float)c < x2 && (float)r >= y1 &&
 *                                (float)r < y2: the crop test of si_hip_detect_masks_f32, a NaN box passes nowhere.
 *   SI_IMGMASK_CROP_AFTER        (process_mask_native, retina masks) boxes in the output frame.  The value of a tap is its logit L; the byte is
 *                                1 exactly when pass(r, c) of the output pixel and v > 0.
 *   SI_IMGMASK_CROP_FIRST        (process_mask(upsample=True)) boxes in the window's frame, in prototype pixels.  The value of a tap is
 *                                pass(i_h, i_w) ? L : +0.0f with the tap's indices inside the window; the byte is 1 exactly when v > 0.
 * tests/imgmask_reference.py restates this in numpy float32 and reproduces the bits.
 *
 * A geom record lives on the device and cannot be checked on the host.  The kernel treats a window that leaves the plane (win_x0 < 0,
 * win_w <= 0, win_x0 + win_w > mw, likewise rows), a non-positive out_w / out_h, or out_w > OW / out_h > OH as "write the image's live planes
 * as zeros": nothing of the prototypes is read for that image.
 *
 * Kernels.  A workgroup of 256 lanes owns one 128 x 8 tile of the output of one image, a lane 4 consecutive bytes of a row, and loops over the
 * image's live detections.  "detect_image_masks_kernel<shared>": the tile's prototype footprint is staged into LDS once ([pixels][nm], rows
 * padded to an odd stride, 16-byte loads when nm % 4 == 0, proto_ld % 4 == 0 and protos is 16-byte aligned); per detection a wave-uniform test
 * stores zeros when the box does not meet the tile, else the lanes form the footprint's logits once per prototype pixel (coefficients
 * wave-uniform) into one of two LDS logit tiles, and after ONE barrier every lane blends, crops, thresholds and stores its four bytes.
 * "detect_image_masks_kernel<direct>": no LDS, a lane forms the dots of its own taps; the same bits.  The arm is chosen on the host for the
 * nominal geometry, the whole plane onto OH x OW: shared when that tile's footprint fits 48 KB of LDS and holds at most 4 prototype pixels per
 * output pixel (beyond that nothing is shared and the direct arm does less).  Inside the shared kernel a tile whose own geom record breaks
 * that rule runs the direct arm's code.  Four bytes per store when OW % 4 == 0 and masks is 4-byte aligned, single bytes otherwise.
 * Everything inside a plane is a 32-bit offset, plane and image bases are 64-bit.  No host round trip, no allocation, safe inside a captured
 * graph.  The matrix cores are deliberately not used: their accumulation order would give up the bit rule that ties this kernel to
 * si_hip_detect_masks_f32 and to the numpy restatement (include/si_detect.h says the same).
 *
 * Refused before any device call.  SI_E_BADARG: a null descriptor or pointer, a protos / extras / boxes / counts / geom off its 4-byte element,
 * non-positive n / mh / mw / nm / extra / OH / OW, proto_ld < nm, box_ld < 4, max_det < 0, coef_off < 0 or coef_off + nm > extra, crop or
 * flags out of range.  SI_E_UNSUPPORTED: nm > 64, n > 65535, an image's prototypes or an output plane beyond 31 bits of elements, masks,
 * extras or boxes beyond 2^46 elements.
 */
#ifndef SI_IMGMASK_H_
#define SI_IMGMASK_H_

#include "si_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { SI_IMGMASK_CROP_AFTER = 0, SI_IMGMASK_CROP_FIRST = 1 };   /* crop */
enum { SI_IMGMASK_FORCE_DIRECT = 1 };                            /* flags: take the direct arm whatever the rule says (for tests) */

typedef struct SiImageMaskDesc {
    int n, mh, mw, nm;      /* prototypes [n][mh][mw][nm] */
    int proto_ld;           /* pixel stride >= nm */
    int max_det, extra, coef_off;   /* coefficients of detection d: extras[b][d][coef_off .. coef_off + nm) */
    int oh, ow;             /* OH, OW: masks [n][max_det][OH][OW] */
    int box_ld;             /* floats between box rows, >= 4 */
    int crop;               /* SI_IMGMASK_CROP_AFTER / SI_IMGMASK_CROP_FIRST */
    int flags;              /* 0 or SI_IMGMASK_FORCE_DIRECT */
} SiImageMaskDesc;

int si_hip_detect_image_masks_f32(const SiImageMaskDesc* d, const float* protos, const float* extras, const float* boxes, const int* counts,
                                  const int* geom /* [n][6] */, unsigned char* masks /* [n][max_det][OH][OW] */, si_stream_t stream);
/* the kernel a launch with these pointers takes; "none" when refused */
const char* si_hip_detect_image_masks_kernel_name(const SiImageMaskDesc* d, const void* protos, const void* masks);

#ifdef __cplusplus
}
#endif

#endif /* SI_IMGMASK_H_ */
