/*
 * si_layernorm.h -- C-ABI of F.layer_norm over the last (contiguous) axis, torch's semantics.  The symbols live in libsi_hip.so beside
 * those of include/si_hip.h; they have a header of their own as include/si_lpnorm.h and include/si_softmax.h have.
 *
 * The problem is `rows` rows of `c` contiguous elements, row r at in + r * in_ld and out + r * out_ld (strides in elements): what lies
 * between two rows (ld > c) is never read and never written.  A rank-2 [N, F] tensor is rows = N, c = F; a rank-3 [A, B, E] token
 * tensor is rows = A * B, c = E.  `gamma` and `beta` are c float32 values each whatever the storage; either may be null (no scale /
 * no shift).  `in` and `out` must not overlap (two disjoint channel slices of one buffer with a common stride do not overlap).
 *
 * Arithmetic, the same in every form.  All of it is float32 whatever the storage; the fp16 entry widens halves on load and rounds once,
 * to nearest even, at the store.  cf = (float)c.
 *   mean = sum(x) / cf                          one IEEE division
 *   d    = x - mean                             per element, kept in the lane's registers (the 3-pass form recomputes it from x)
 *   var  = sum(d * d) / cf                      the biased variance of the CENTRED values, never E[x^2] - mean^2; each square is
 *                                               rounded to float32 on its own and then added
 *   rstd = 1.0f / sqrtf(var + eps)              one addition, one correctly rounded square root, one IEEE division
 *   y    = ((d * rstd) * gamma) + beta          each operation rounded on its own; a null gamma drops the product, a null beta the sum
 * No operation is contracted into an fma: the file is compiled with `#pragma clang fp contract(off)` above its includes (the promise
 * include/si_act.h makes for mish).
 *
 * Order of additions, for both sums alike.  An ITEM is a 16-byte channel vector (4 floats / 8 halves), or a single element in the
 * single-element instantiation; VW is its width, cv = c / VW.  Every accumulator starts at +0; the elements of an item enter it in
 * channel order.  A row is spread over L lanes; lane j adds items j, j + L, j + 2L, ... in that order.  Then a __shfl_xor butterfly over
 * the offsets L / 2, L / 4, ..., 1 (at most 32 .. 1): at every step lane j's value becomes v[j] + v[j ^ offset], a pairwise tree
 * (si_team of the reduction commons).  A whole workgroup then adds its four wave values from LDS as ((w0 + w1) + w2) + w3 (si_block).
 *
 * Special values follow from the arithmetic: a NaN or an infinity anywhere in a row makes every output of that row NaN (inf - inf in
 * the centring, or a NaN sum) and touches no other row.  A row of equal values whose sum is exact has d = +0 everywhere and gives
 * exactly beta (with eps > 0); with eps = 0 it gives 0 * inf = NaN, as torch does.
 *
 * Forms, chosen from c alone (the instantiation also from the strides and the pointers' alignment), never from rows or the grid;
 * si_hip_layernorm_kernel_name reports which:
 *   row_group        c <= SI_LAYERNORM_GROUP_MAX_C.  A group of L = 2^k <= 64 lanes per row, several rows per wave64: with
 *                    per = min(16 / VW, 4), L is the smallest power of two with L * per >= cv, at most 64.  The row stays in registers:
 *                    one read, one write.
 *   row_block        SI_LAYERNORM_GROUP_MAX_C < c <= SI_LAYERNORM_BLOCK_MAX_C.  A workgroup of 256 threads per row (L = 256), the row
 *                    in registers: one read, one write.
 *   row_block_3pass  longer rows.  The same workgroup and the same order of additions; the row is read three times (sum, centred
 *                    squares, result).
 * In the two register forms a lane owns the same items of every row it visits in the grid-stride loop.  It loads its gamma / beta items
 * ONCE, before the row loop, and keeps them in registers: the traffic is one read and one write of the activation plus 2 c floats per
 * workgroup.  The 3-pass form reads gamma / beta in its third pass, per row (they stay in cache).
 * Each form has a 16-byte vector instantiation and a single-element one; the vector one is taken when c, both strides and both
 * pointers allow it (gamma and beta are read as single floats and need no alignment).  Grids are capped at 2048 workgroups and the
 * kernels loop over the rest (grid-stride).
 *
 * No atomics, no workspace, no host round trip: two launches give the same bits, a row's bits do not depend on the other rows of the
 * launch, on rows, or on which pass or workgroup computed it, and every launch is safe inside a captured graph.
 *
 * Refused before any device call: a null descriptor, a null `in` or `out`, non-positive rows or c, in_ld < c, out_ld < c, a negative or
 * NaN eps, overlapping in / out (SI_E_BADARG); element offsets that do not fit 31 bits (SI_E_UNSUPPORTED).  SI_E_BADARG is looked for
 * first.
 */
#ifndef SI_LAYERNORM_H_
#define SI_LAYERNORM_H_

#include "si_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the form switches: the register budgets of include/si_softmax.h and include/si_lpnorm.h.  A lane keeps 16 floats of its row, a group
 * has at most 64 lanes (1024) and a workgroup 256 threads (4096) */
enum { SI_LAYERNORM_GROUP_MAX_C = 1024, SI_LAYERNORM_BLOCK_MAX_C = 4096 };

typedef struct SiLayerNormDesc {
    int rows, c;         /* rows of c contiguous elements */
    int in_ld, out_ld;   /* row strides in elements; >= c */
    float eps;           /* >= 0 */
} SiLayerNormDesc;

/* gamma, beta: c float32 values each, or null */
int si_hip_layernorm_f32(const SiLayerNormDesc* d, const float* in, const float* gamma, const float* beta, float* out, si_stream_t stream);

/* half in, half out; gamma and beta stay float32 */
int si_hip_layernorm_f16(const SiLayerNormDesc* d, const void* in, const float* gamma, const float* beta, void* out, si_stream_t stream);

/* the kernel a launch with these pointers takes: "layernorm_row_group_kernel<T, VW>", "layernorm_row_block_kernel<T, VW>" or
 * "layernorm_row_block_3pass_kernel<T, VW>" with <float, 4>, <float, 1>, <_Float16, 8> or <_Float16, 1>; "none" for a descriptor the
 * launch would refuse (the pointers are looked at for their alignment only) */
const char* si_hip_layernorm_kernel_name(const SiLayerNormDesc* d, const void* in, const void* out, int half);

#ifdef __cplusplus
}
#endif

#endif /* SI_LAYERNORM_H_ */
