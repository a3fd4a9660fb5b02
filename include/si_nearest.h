/*
 * si_nearest.h -- C-ABI of the fused nearest-row search: for every row of x1 the nearest row (and, with k = 2, the second nearest) of x2
 * under the Euclidean distance -- torch.cdist(x1, x2).argmin(-1) and the codebook lookup x2[argmin] as ONE launch that never writes the
 * p x r distance matrix.  The symbols live in libsi_hip.so; they have a header of their own as include/si_cdist.h has.
 *
 * The problem.  x1 is b1 x p x m, x2 is b2 x r x m, B = max(b1, b2), each of b1, b2 is B or 1; rows are m contiguous elements, row i of
 * batch item b of x1 at x1 + b * x1_sb + i * x1_ld (strides in elements), likewise x2.  An operand with bi = 1 is read with batch stride
 * 0 (a codebook).  Outputs, each may be null:
 *   idx   int32   [B, p, k] dense     the column (row of x2) of the nearest, then of the second nearest
 *   dist  float32 [B, p, k] dense     their distances (float32 under fp16 storage too: it is rounded by no store)
 *   rows  storage [B, p, m]           x2[b, idx[b, i, 0], :] copied bit for bit to rows + b * rows_sb + i * rows_ld -- the quantised output
 *                                     of a VQ encoder; what lies between two rows (rows_ld > m) is never written
 *
 * Arithmetic.  That of cdist_mm_kernel (include/si_cdist.h), operation for operation, without the root:
 *   acc  = sum_k x1[i, k] * x2[j, k]          the same MFMA chain: v_mfma_f32_32x32x2_f32 on the 64 x 64 x 32 core (fp32),
 *                                             v_mfma_f32_16x16x32_f16 on K-tiles of 64 halves (fp16 storage)
 *   s    = (n1[i] + n2[j]) - 2 * acc          n1, n2: the squared row norms, added in the order si_cdist.h states
 *   s    = s < 0 ? 0 : s                      a NaN passes
 * s is the comparison key; sqrtf is taken of the winners only.  sqrtf is monotone, so idx[.., 0] is a column at which the row of
 * si_hip_cdist_* in mm mode has its minimum, and dist has the bits of that output before its store cast.  A NaN distance is returned as
 * the quiet NaN 0x7fc00000.
 *
 * The order rule.  Candidates are pairs (s, j) compared lexicographically: the smaller s wins, and on equal s the LOWER column j.  A NaN
 * key counts as smaller than every number and NaN keys tie, so the first NaN wins -- torch.argmin's rule.  (A NaN anywhere in row i of
 * x1 makes every key of that row NaN: idx 0, and 1 for the second.)  The second nearest is the best of the remaining columns under the
 * same rule.  The order is total over distinct columns, so the result depends on neither the tiling, the lane that held a candidate,
 * the split over r nor the order of any combine: two launches, any `splits`, a batch item alone give the same bits.
 *
 * nearest_kernel<T, VEC, K>.  A workgroup of 256 threads (2 x 2 waves) owns 64 rows of x1 of one batch item and walks the 64-column
 * tiles of its share of r.  Per tile: the K loop of cdist_mm_kernel (the A panel is staged again per tile -- it comes from L2 -- and the
 * next K-tile's loads are in flight during the MFMAs); n2 of the tile's columns, and on the first tile n1, meet in LDS; then every lane
 * folds its accumulators into a private (best, second best) per row it holds, kept in registers as (key, column) with
 *   key = NaN ? 0 : bits(s) + 1               unsigned: s >= +0, so the integer order is the order rule; 0xffffffff = no candidate yet
 * Lane maps (C/D of the MFMA): fp32 -- lane (l31, lh) of wave (wm, wn) holds column 32 wn + l31 and rows 32 wm + 4 lh + {0..3, 8..11,
 * 16..19, 24..27}: 16 rows, one column per tile; fp16 -- lane (l15, g4) holds columns 32 wn + 16 tj + l15 and rows 32 wm + 16 ti + 4 g4 +
 * e: 8 rows, two columns per tile.  A lane meets its columns in ascending order, so inside a lane a strict < keeps the lower column.  The
 * score tile is never written anywhere.  After the last tile the 32 (16) lanes that share a row combine by wave shuffles, the two waves
 * (wn) through LDS, one thread per row.
 *
 * The split over r.  p_tiles * B workgroups cannot fill the device when p is small, so `splits` workgroups may share a row panel, split s
 * taking column tiles [s * T, (s + 1) * T), T = ceil(r_tiles / splits) (a split may get none).  splits = 0 chooses: 1 when
 * p_tiles * B >= 256, else min(16, r_tiles, 256 / (p_tiles * B)) -- 256 is the MI355X's CU count as a constant, not a device query (the
 * choice and the workspace size answer without a device): a gfx950 part with fewer CUs gets the MI355X's choice, which is correct there and
 * at worst splits further than it needs.  With splits > 1 each workgroup writes its
 * (key, column) pairs to the workspace -- B * p * splits * k pairs of 8 bytes, si_hip_nearest_workspace_bytes -- and
 * nearest_combine_kernel<T> (one thread per row, 64 rows per workgroup) combines them under the same rule, takes the roots and copies
 * the rows.  Fixed launches, no atomics, no memset: every launch is safe inside a captured graph.  The workspace needs no
 * initialisation; 8-byte aligned.
 *
 * Instantiations: VEC as in si_cdist.h (m, both row strides, the batch strides of operands with bi > 1 multiples of 4 and x1, x2
 * 16-byte aligned; else single elements), fp32 only; the fp16 entry has the vector form alone.  rows is copied in 16-byte vectors when
 * rows, rows_ld (and rows_sb with B > 1) allow it too, else element by element.
 *
 * Refused before any device call.  SI_E_BADARG: a null descriptor, x1 or x2; idx, dist and rows all null; non-positive b1, b2, p, r or
 * m; b1 != b2 with neither 1; k outside {1, 2}; k = 2 with r < 2; splits outside 0 .. 16; a row stride below m; a batch stride below
 * the item; with more than one split a null or misaligned workspace, one smaller than workspace_bytes or one that shares a byte
 * with an operand or an output; an output overlapping an operand or another output.  SI_E_UNSUPPORTED: r >= 2^31 / 64; element offsets beyond 31 bits; under fp16 m % 8 != 0 or views that do not allow 16-byte
 * vectors.  SI_E_BADARG is looked for first.
 */
#ifndef SI_NEAREST_H_
#define SI_NEAREST_H_

#include <stddef.h>

#include "si_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { SI_NEAREST_MAX_SPLITS = 16 };

typedef struct SiNearestDesc {
    int b1, b2;                   /* batch items of x1 and of x2: equal, or one of them 1 */
    int p, r, m;                  /* rows of x1, rows of x2, elements of a row */
    int x1_ld, x2_ld, rows_ld;    /* row strides in elements */
    int x1_sb, x2_sb, rows_sb;    /* batch strides in elements (x1_sb / x2_sb are not read when b1 / b2 is 1) */
    int k;                        /* 1: the nearest; 2: and the second nearest */
    int splits;                   /* workgroups that share a row panel, 1 .. 16; 0: the plan chooses */
} SiNearestDesc;

/* bytes of workspace a launch with this descriptor needs (0 with one split, and for a descriptor the launch refuses) */
size_t si_hip_nearest_workspace_bytes(const SiNearestDesc* d);

int si_hip_nearest_f32(const SiNearestDesc* d, const float* x1, const float* x2, int* idx, float* dist, float* rows, void* workspace,
                       size_t workspace_bytes, si_stream_t stream);

/* halves in, rows in halves; idx and dist as above */
int si_hip_nearest_f16(const SiNearestDesc* d, const void* x1, const void* x2, int* idx, float* dist, void* rows, void* workspace,
                       size_t workspace_bytes, si_stream_t stream);

/* the kernel a launch with these pointers takes: "nearest_kernel<T, VEC, K>" with T float or _Float16; "none" for a descriptor the launch
 * would refuse (the pointers are looked at for their alignment only; rows may be null) */
const char* si_hip_nearest_kernel_name(const SiNearestDesc* d, const void* x1, const void* x2, const void* rows, int half);

#ifdef __cplusplus
}
#endif

#endif /* SI_NEAREST_H_ */
