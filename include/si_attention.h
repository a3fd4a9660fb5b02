/*
 * si_attention.h -- C-ABI of fused scaled dot-product attention without mask and without dropout, the kernel behind nn.MultiheadAttention
 * (torch semantics, no reference counterpart).  The symbols live in libsi_hip.so beside those of include/si_hip.h; they have a header of
 * their own as include/si_softmax.h and include/si_permute.h have.
 *
 *     O[b, h, i, :] = sum_j softmax_j(scale * <Q[b, h, i, :], K[b, h, j, :]>) * V[b, h, j, :]        i < lq, j < lk, vectors of d elements
 *
 * Views.  Each of q, k, v, o is a set of token rows: the row of token s of batch item b starts b * sb + s * ss elements into the tensor,
 * head h starts h * d elements into the row and its d elements are contiguous.  That serves seq-first [L, N, E] (sb = E, ss = N * E),
 * batch-first [N, L, E] (sb = L * E, ss = E) and column slices of a wider [rows, 3E] projection buffer with the same code.  The kernel reads
 * and writes only ptr[b * sb + s * ss + h * d + i] with i < d: what lies between two rows, or beside the heads * d columns of a row, is
 * never read and never written.  The extent of `o` (first to last element) must not intersect the extent of an input.
 *
 * One launch, no workspace, no atomics.  A workgroup of four waves owns one (batch, head, block of SI_ATTENTION_BLOCK_Q queries), a wave 16
 * query rows.  K and V are walked in tiles of SI_ATTENTION_TILE_K keys staged in LDS; every wave keeps a running row maximum, a running row
 * sum and the fp32 output accumulator in registers and rescales them when the maximum moves (online softmax); the score matrix reaches
 * neither LDS nor memory.  exp is the hardware exp2 with scale * log2(e) folded into one multiply, applied to the score's distance from the
 * maximum (the subtraction comes first and is exact for nearby scores: a weight keeps its relative precision however large the scores are).
 *     fp32  both products on v_mfma_f32_16x16x4_f32: the k-ordered fp32 fma chain of the project's fp32 convolutions.  Any d from 1 to
 *           SI_ATTENTION_MAX_D: the LDS image is zero-padded to the instantiated head dim (16 / 32 / 64 / 128).
 *     fp16  q / k / v / o are halves; both products on v_mfma_f32_16x16x32_f16; scores, maximum, sum and accumulator are fp32; P is rounded
 *           to fp16 for the second product (the row sum adds the rounded values); the result is rounded once, to nearest even, at the store.
 *           d % 8 == 0, every stride a multiple of 8 and every pointer 16-byte aligned; instantiated on 32 / 64 / 128.
 *
 * Contract.  Every reduction runs in a fixed order: two launches give the same bits; the bits of (b, h, i, :) depend on Q[b, h, i, :],
 * K[b, h] and V[b, h] alone -- not on batch, on heads, on the other heads' data, on lq or on the position of row i inside its block (a query
 * row run alone has the bits of the row inside a block); every launch is safe inside a captured graph.  The maximum is subtracted before exp:
 * inputs whose scores are finite never produce Inf or NaN.  Keys beyond lk contribute exactly 0 and are never read; query rows beyond lq are
 * neither read nor stored.  A NaN in Q[b, h, i, :] makes only output row i NaN; a NaN in K[b, h, j, :] makes every row of that (b, h) NaN
 * and no other; a NaN in V[b, h, j, c] makes column c of that (b, h) NaN, as in torch (0 * NaN is NaN).
 *
 * Refused before any device call: a null descriptor or tensor, non-positive sizes, a negative stride, a sequence stride below heads * d, an
 * output batch stride below heads * d when batch > 1, output strides under which two (batch item, token) rows share an element (neither
 * o_sb >= (lq - 1) o_ss + heads d nor o_ss >= (batch - 1) o_sb + heads d), `o` intersecting an input (SI_E_BADARG); element offsets or a workgroup count beyond
 * 31 bits, d > SI_ATTENTION_MAX_D, and for fp16 d % 8 != 0 or a stride / pointer that is not 16-byte aligned (SI_E_UNSUPPORTED).
 */
#ifndef SI_ATTENTION_H_
#define SI_ATTENTION_H_

#include "si_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { SI_ATTENTION_BLOCK_Q = 64, SI_ATTENTION_TILE_K = 64, SI_ATTENTION_MAX_D = 128 };

typedef struct SiAttentionDesc {
    int batch, heads, lq, lk, d;
    long long q_sb, q_ss;   /* element strides of the batch index and of the sequence index */
    long long k_sb, k_ss;
    long long v_sb, v_ss;
    long long o_sb, o_ss;
    float scale;            /* nn.MultiheadAttention: 1 / sqrt(d) */
} SiAttentionDesc;

int si_hip_attention_f32(const SiAttentionDesc* d, const float* q, const float* k, const float* v, float* o, si_stream_t stream);

/* halves in, halves out */
int si_hip_attention_f16(const SiAttentionDesc* d, const void* q, const void* k, const void* v, void* o, si_stream_t stream);

/* the kernel a launch with these pointers takes: "attention_kernel<float, DP>" with DP = 16 / 32 / 64 / 128, "attention_kernel<_Float16, DP>"
 * with DP = 32 / 64 / 128 (DP: the padded head dim); "none" for a descriptor the launch would refuse */
const char* si_hip_attention_kernel_name(const SiAttentionDesc* d, const void* q, const void* k, const void* v, const void* o, int half);

#ifdef __cplusplus
}
#endif

#endif /* SI_ATTENTION_H_ */
