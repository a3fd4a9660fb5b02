/*
 * si_cdist.h -- C-ABI of torch.cdist: the distance between every row of x1 and every row of x2, torch's semantics.  The symbols live in
 * libsi_hip.so beside those of include/si_hip.h; they have a header of their own as include/si_layernorm.h and include/si_attention.h have.
 *
 * The problem.  x1 is b1 x p x m, x2 is b2 x r x m, out is B x p x r with B = max(b1, b2); each of b1, b2 is B or 1.  Rows are m contiguous
 * elements; row i of batch item b of x1 is at x1 + b * x1_sb + i * x1_ld (strides in elements), likewise x2 and out (rows of r elements).
 * What lies between two rows (ld > m, out_ld > r) is never read and never written.  An operand with bi = 1 is read with batch stride 0
 * whatever its sb field holds: a rank-2 operand (the codebook of a VQ encoder) is bi = 1.
 *
 *   out[b, i, j] = ( sum_k |x1[b, i, k] - x2[b, j, k]|^norm )^(1 / norm)        norm 1 or 2,  or  max_k |x1 - x2|  for norm inf
 *
 * Arithmetic.  All of it is float32 whatever the storage; the fp16 entry widens halves on load and rounds the result once, to nearest
 * even, at the store.  No operation is contracted into an fma (`#pragma clang fp contract(off)` above the file's includes).
 *
 * cdist_mm_kernel<T, VEC> -- norm 2 on the matrix cores (SI_CDIST_MODE_* decides when, below).  One workgroup of 256 threads owns a
 * 64 x 64 tile of out for one batch item: 2 x 2 waves, 32 x 32 outputs per wave.  fp32: the 64 x 64 x 32 GEMM core of the conv-transpose
 * and deformable kernels on v_mfma_f32_32x32x2_f32 (a k-ordered fp32 fma chain); fp16: v_mfma_f32_16x16x32_f16 with fp32 accumulators on
 * an LDS image of [128 rows][64 + 8 halves].  The next K-tile's global loads are in flight during the MFMAs.
 *   acc  = sum_k x1[i, k] * x2[j, k]                       the MFMA chain, k ascending tile by tile
 *   s    = (n1[i] + n2[j]) - 2 * acc                       two roundings (2 * acc is exact)
 *   s    = s < 0 ? 0 : s                                   a NaN passes
 *   out  = sqrtf(s)                                        correctly rounded, then the store's cast
 * The squared row norms n1, n2 are no pre-pass and need no workspace.  Order of additions, the same for n1 and n2: an ITEM is the 16-byte
 * K vector a thread stages (4 floats / 8 halves; the single-element instantiation stages the same items element by element), a K-TILE is 8
 * items (32 floats / 64 halves).  Item v of K-tile t of a row is staged by ONE thread, the same for every t: it keeps a private accumulator
 * q[v], starting at +0, and adds the squares of its items' elements (each square rounded to float32 on its own) in k order, K-tile after
 * K-tile.  Elements at k >= m add +0.  After the K loop the row's eight partials meet in LDS and ONE thread adds them as
 *   n = ((((((q[0] + q[1]) + q[2]) + q[3]) + q[4]) + q[5]) + q[6]) + q[7].
 * tests/cdist_reference.py restates this in numpy (mm_sqnorm).
 *
 * cdist_direct_kernel<T, NORM> -- the difference form, on the vector ALU: norm 1, norm inf, and norm 2 when the mode asks for it.  A
 * workgroup of 256 threads owns a 64 x 64 tile, a lane 4 x 4 outputs (rows 4 ty + a, columns tx + 16 c: a wave writes runs of 16 columns).
 * m is staged through LDS in chunks of 32 (row pitch 33 words: the 16 x2 rows a wave reads at one k lie in 16 banks).  Per output ONE
 * accumulator, starting at +0, k ascending:
 *   norm 1     acc = acc + |a - b|
 *   norm inf   acc = (d > acc || d != d) ? d : acc,  d = |a - b|        a NaN stays
 *   norm 2     acc = acc + (a - b) * (a - b), each term rounded on its own; out = sqrtf(acc)
 *
 * The mode is torch's compute_mode and matters for norm 2 only; the choice is made from the descriptor alone, never from the grid:
 *   SI_CDIST_MODE_MM_IF_NECESSARY (the default)   the mm kernel when p > 25 || r > 25
 *   SI_CDIST_MODE_MM                              always the mm kernel
 *   SI_CDIST_MODE_NO_MM                           never
 * Each mm kernel has a 16-byte vector instantiation and a single-element one.  The vector one needs m, both row strides and the batch
 * strides of operands with bi > 1 to be multiples of 4 (8 under fp16) and x1, x2 16-byte aligned; everything else takes the
 * single-element form.  The direct kernel reads single elements.
 *
 * Special values follow from the arithmetic.  A NaN in a row of x1 (of x2) makes that row (column) of its batch item NaN and touches
 * nothing else.  An infinity gives inf in the direct form (NaN against an infinity of the same sign at the same k) and, in the mm form,
 * what inf - inf and 0 * inf give: NaN where the other row is positive or zero at that k, inf where it is negative -- torch's CPU results,
 * with one exception: under norm inf torch's CPU max drops the NaN of inf - inf and returns the largest other difference; here it stays.
 *
 * No atomics, no workspace: exactly one lane stores each output, once.  Two launches give the same bits; a batch item's bits do not
 * depend on B, an output row's bits do not depend on p (nor a column's on r).  Every launch is safe inside a captured graph.  The grid is
 * (tiles, 1, min(B, 65535)); the kernels loop over further batch items.  Tiles are numbered so that the tiles along r that share a panel
 * of x1 rows have the same index % 8 (one XCD, one L2).
 *
 * Refused before any device call.  SI_E_BADARG: a null descriptor or pointer; non-positive b1, b2, p, r or m; b1 != b2 with neither 1; a
 * row stride below the row (x1_ld < m, x2_ld < m, out_ld < r); a batch stride (of an operand with bi > 1, of out with B > 1) below the
 * item; out overlapping x1 or x2.  SI_E_UNSUPPORTED: a norm code other than the three below (torch's p = 0 and fractional p have none);
 * an unknown mode; element offsets that do not fit 31 bits.  SI_E_BADARG is looked for first.
 */
#ifndef SI_CDIST_H_
#define SI_CDIST_H_

#include "si_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { SI_CDIST_NORM_1 = 1, SI_CDIST_NORM_2 = 2, SI_CDIST_NORM_INF = 3 };
enum { SI_CDIST_MODE_MM_IF_NECESSARY = 0, SI_CDIST_MODE_MM = 1, SI_CDIST_MODE_NO_MM = 2 };
/* torch's threshold of the default mode: the mm kernel above it */
enum { SI_CDIST_MM_THRESHOLD = 25 };

typedef struct SiCdistDesc {
    int b1, b2;                  /* batch items of x1 and of x2: equal, or one of them 1 */
    int p, r, m;                 /* rows of x1, rows of x2, elements of a row */
    int x1_ld, x2_ld, out_ld;    /* row strides in elements */
    int x1_sb, x2_sb, out_sb;    /* batch strides in elements (x1_sb / x2_sb are not read when b1 / b2 is 1) */
    int norm;                    /* SI_CDIST_NORM_* */
    int mode;                    /* SI_CDIST_MODE_* */
} SiCdistDesc;

int si_hip_cdist_f32(const SiCdistDesc* d, const float* x1, const float* x2, float* out, si_stream_t stream);

/* halves in, halves out */
int si_hip_cdist_f16(const SiCdistDesc* d, const void* x1, const void* x2, void* out, si_stream_t stream);

/* the kernel a launch with these pointers takes: "cdist_mm_kernel<T, VEC>" with <float, true>, <float, false>, <_Float16, true> or
 * <_Float16, false>, or "cdist_direct_kernel<T, NORM>" with NORM 1, 2 or 3; "none" for a descriptor the launch would refuse (the
 * pointers are looked at for their alignment and overlap only) */
const char* si_hip_cdist_kernel_name(const SiCdistDesc* d, const void* x1, const void* x2, const void* out, int half);

#ifdef __cplusplus
}
#endif

#endif /* SI_CDIST_H_ */
