/*
 * si_grid.h -- C-ABI of F.grid_sample (4-D, bilinear and nearest) and F.affine_grid (torch semantics, no reference counterpart).  The symbols
 * live in libsi_hip.so beside those of include/si_hip.h; they have a header of their own as include/si_deform.h and include/si_norm.h have.
 *
 * Operands (fp32 or fp16 storage, one type for all of them; every operation below is fp32):
 *     x     [n, h, w, c]       NHWC, pixels in_ld elements apart          out  [n, ho, wo, c]   NHWC, pixels out_ld elements apart
 *     grid  the element (img, oy, ox, k) lies at img gs_n + oy gs_h + ox gs_w + k gs_k;  k = 0 is the x (width) coordinate, k = 1 is y
 *     theta [n][2][3]          instead of a grid (grid_source = SI_GRID_THETA): the coordinates of F.affine_grid, computed in the kernel
 * Three grids matter: torch's dense [n, ho, wo, 2] is (ho wo 2, wo 2, 2, 1); a channels-first [n, 2, ho, wo] tensor stored NHWC with pixel
 * stride ld -- the tensor in FRONT of the permute(0, 2, 3, 1) that models write -- is (ho wo ld, wo ld, ld, 1) and is read in place; a rank-4
 * [n, ho, wo, 2] tensor in this project's storage order ([n][wo][2][ho], rows ld apart) is (2 wo ld, 1, 2 ld, ld).
 *
 * The rule, per output pixel and axis (size = w for x, h for y; g the grid value as fp32).  No operation is contracted: the fused
 * multiply-adds are the ones written here.
 *     unnormalise   align_corners: p = ((g + 1) * 0.5f) * (size - 1)              otherwise: p = ((g + 1) * size - 1) * 0.5f
 *     padding       zeros:      p stays
 *                   border:     p = fminf(fmaxf(p, 0), size - 1)                                (a NaN becomes 0)
 *                   reflection: lo = 0, span = size - 1 (align_corners) or lo = -0.5f, span = size (otherwise); span == 0 gives 0; else
 *                               a = fabsf(p - lo), e = fmodf(a, span), f = floorf(a / span), p = f even ? e + lo : span - e + lo -- the
 *                               parity of f taken in float, f - 2 floorf(f * 0.5f), so beyond 2^24 flips count as even -- then the border clip
 *     NaN           a coordinate that is NaN now (zeros padding only) makes every channel of the pixel NaN; nothing is read
 *     bilinear      x0 = floorf(px), wx1 = px - x0, wx0 = (x0 + 1) - px, likewise y; taps in the order (y0, x0), (y0, x0 + 1), (y0 + 1, x0),
 *                   (y0 + 1, x0 + 1) with weights wx0 wy0, wx1 wy0, wx0 wy1, wx1 wy1 (one multiplication each);
 *                   acc = 0, then for every tap INSIDE the image, in that order, acc = fmaf(weight, value, acc): a tap inside is multiplied
 *                   even by a weight of 0 (Inf * 0 is NaN, as in torch), a tap outside adds nothing and is not read
 *     nearest       the pixel (nearbyintf(py), nearbyintf(px)), half to even; outside the image: 0
 *     integers      x0 / nearbyint are clamped IN FLOAT to [-2, size] before the conversion: +-Inf and +-1e30 index nothing outside
 *
 * F.affine_grid for an output of [n, H, W]: base coordinates xb_j = (2 j + 1 - W) / W (one IEEE division of two exactly converted integers)
 * or, with align_corners, 2 j / (W - 1) - 1 (0 when W == 1); yb_i likewise; g_k = fmaf(theta[k][0], xb, fmaf(theta[k][1], yb, theta[k][2])).
 * The sampler's theta source computes exactly this and uses the fp32 value; si_hip_affine_grid_* rounds it to the storage type and writes
 * the rank-4 [n, H, W, 2] tensor in this project's storage order: element (img, i, j, k) at ((img W + j) 2 + k) out_ld + i.
 *
 * Kernels.  The sampler is a gather bound by HBM / L2: one read of the taps, one write of the output; no LDS, no scratch, no atomics, no
 * workspace.  A lane owns one channel vector of one output pixel, channel vectors fastest across lanes (a wave reads each tap of a pixel as
 * one contiguous stretch); a capped grid strides over the items.  Vector widths: fp32 4 | 1, fp16 8 | 4 | 2 | 1, the widest that c, both
 * pixel strides and both pointers allow.  With gs_k == 1, even gs_n / gs_h / gs_w and a grid pointer aligned to two elements the two
 * coordinates are one load ("pair"), otherwise two ("strided").  Every arm computes the same bits.  Names:
 *     grid_sample_kernel<float|_Float16, VW, pair|strided|theta>        affine_grid_kernel<float|_Float16>
 *
 * Refused before any device call: a null descriptor or pointer, non-positive sizes, a pixel stride below c, a negative grid stride, mode /
 * padding_mode / grid_source outside the enumerations, `out` intersecting the extent of x, of the grid or of theta (SI_E_BADARG); bicubic,
 * spatial_dims == 3 (5-D sampling), element offsets or an item count beyond 31 bits (SI_E_UNSUPPORTED).
 */
#ifndef SI_GRID_H_
#define SI_GRID_H_

#include "si_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { SI_GRID_BILINEAR = 0, SI_GRID_NEAREST = 1, SI_GRID_BICUBIC = 2 };
enum { SI_GRID_PAD_ZEROS = 0, SI_GRID_PAD_BORDER = 1, SI_GRID_PAD_REFLECTION = 2 };
enum { SI_GRID_TENSOR = 0, SI_GRID_THETA = 1 };

typedef struct SiGridSampleDesc {
    int n, c, h, w, ho, wo;
    int in_ld, out_ld;                 /* pixel strides of x and out; 0: dense (c) */
    int mode, padding_mode, align_corners;
    int grid_source;                   /* SI_GRID_TENSOR: the strides below; SI_GRID_THETA: the pointer is theta, the strides are not looked at */
    int spatial_dims;                  /* 2 (0 reads as 2); 3 is SI_E_UNSUPPORTED */
    long long gs_n, gs_h, gs_w, gs_k;  /* element strides of the grid */
} SiGridSampleDesc;

typedef struct SiAffineGridDesc {
    int n, h, w;
    int out_ld;                        /* row stride of the stored [n][w][2][h] image; 0: dense (h) */
    int align_corners;
} SiAffineGridDesc;

int si_hip_grid_sample_f32(const SiGridSampleDesc* d, const float* x, const float* grid_or_theta, float* out, si_stream_t stream);
int si_hip_grid_sample_f16(const SiGridSampleDesc* d, const void* x, const void* grid_or_theta, void* out, si_stream_t stream);

/* the kernel a launch with these pointers takes; "none" for a descriptor or pointers the launch would refuse */
const char* si_hip_grid_sample_kernel_name(const SiGridSampleDesc* d, const void* x, const void* grid_or_theta, const void* out, int half);

int si_hip_affine_grid_f32(const SiAffineGridDesc* d, const float* theta, float* out, si_stream_t stream);
int si_hip_affine_grid_f16(const SiAffineGridDesc* d, const void* theta, void* out, si_stream_t stream);
const char* si_hip_affine_grid_kernel_name(const SiAffineGridDesc* d, const void* theta, const void* out, int half);

#ifdef __cplusplus
}
#endif

#endif /* SI_GRID_H_ */
