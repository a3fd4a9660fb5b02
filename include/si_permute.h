/*
 * si_permute.h -- C-ABI of the strided-gather copy behind Tensor.permute / Tensor.reshape / Tensor.view / torch.transpose / torch.squeeze /
 * torch.unsqueeze (torch semantics, no reference counterpart).  The symbols live in libsi_hip.so beside those of include/si_hip.h; they have a
 * header of their own as include/si_slice.h and include/si_pad.h have.
 *
 * One operation: a dense output is written from a strided input.  The output is a loop nest of `rank` dimensions, outermost first; element
 * (i0, .., i_{rank-1}) of the nest is read at   src[sum_k i_k * in_stride[k]]   and written at   dst[row * out_ld + i_{rank-1}],   row being
 * the row-major index of (i0, .., i_{rank-2}).  What lies between two runs of the output (out_ld > dims[rank-1]) is never written; what the
 * strides skip in the input is never read.  Source and destination must not overlap.  The layout algebra that turns a chain of layout
 * operators into such a nest is host code (csrc/host/layout_plan.h, include/si_layout.h).
 *
 * The kernels move bits -- 4-byte words for fp32, 2-byte words for fp16 -- and do no arithmetic on a value: NaN payloads, -0.0 and denormals
 * come out as they went in.  No atomics, no workspace, no host round trip: every launch is safe inside a captured graph and two launches give
 * the same bits.  Every form is a grid-stride loop with a capped grid (the constants below).
 *
 * Forms (si_hip_permute_kernel_name reports which), T = float / _Float16, V = 16 bytes of T (4 / 8):
 *     "permute_rows<T, V>"   in_stride[rank-1] == 1: runs of dims[rank-1] elements are copied, with 16-byte loads and stores where the run
 *                            length, every other input stride, out_ld and both pointers are multiples of 16 bytes; V = 1 otherwise (K = 6,
 *                            C = 3, odd fp16 counts)
 *     "permute_tile<T>"      in_stride[rank-1] != 1 and another loop dimension j has in_stride[j] == 1: a 2-D transpose over (j, rank-1)
 *                            through an LDS tile of SI_PERMUTE_TILE x SI_PERMUTE_TILE elements, batched over the other dimensions.  Global reads
 *                            are coalesced along j, global writes along rank-1.  A tile row is padded by one 4-byte word (fp32: 65 words,
 *                            fp16: 66 halves = 33 words), which makes the column reads free of bank conflicts.  Taken by form 0 when both
 *                            tile extents are at least SI_PERMUTE_TILE_MIN
 *     "permute_elem<T>"      one element per lane: everything else
 * All forms produce the same bits; `form` forces one (tests, A/B), SI_E_BADARG when the nest is not eligible for it.
 *
 * Refused before any device call: a null descriptor or tensor, rank outside 1..4, a non-positive extent or stride, out_ld < dims[rank-1], a
 * form outside 0..3 or one the nest is not eligible for (SI_E_BADARG); an input or output element offset, or an item count, that does not fit
 * 31 bits (SI_E_UNSUPPORTED).
 */
#ifndef SI_PERMUTE_H_
#define SI_PERMUTE_H_

#include "si_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SI_PERMUTE_FORM_AUTO 0
#define SI_PERMUTE_FORM_ROWS 1
#define SI_PERMUTE_FORM_TILE 2
#define SI_PERMUTE_FORM_ELEM 3

#define SI_PERMUTE_TILE 64            /* elements per side of the LDS tile */
#define SI_PERMUTE_TILE_MIN 32        /* form 0 takes the tile form from this extent of BOTH tile dimensions on (measured; the guess was 8: DESIGN 9k) */
#define SI_PERMUTE_TILE_MAX_BLOCKS 2048 /* workgroups of a permute_tile launch (256 lanes, one tile per pass) */
#define SI_PERMUTE_MAX_BLOCKS 2048    /* workgroups of a permute_rows / permute_elem launch (256 lanes, one item per lane and pass) */

typedef struct SiPermuteDesc {
    int rank;               /* 1..4 loop dimensions, outermost first */
    int dims[4];            /* extents of the output loop nest */
    long long in_stride[4]; /* input element stride of each loop dimension, > 0 */
    int out_ld;             /* pitch, in elements, between two runs of dims[rank-1] output elements; >= dims[rank-1] */
    int form;               /* 0 auto; else force one of the forms above */
} SiPermuteDesc;

int si_hip_permute_f32(const SiPermuteDesc* d, const void* src, void* dst, si_stream_t stream);

/* half in, half out */
int si_hip_permute_f16(const SiPermuteDesc* d, const void* src, void* dst, si_stream_t stream);

/* the kernel a launch with these pointers takes (the names above); "none" for a descriptor the launch would refuse */
const char* si_hip_permute_kernel_name(const SiPermuteDesc* d, const void* src, const void* dst, int half);

#ifdef __cplusplus
}
#endif

#endif /* SI_PERMUTE_H_ */
