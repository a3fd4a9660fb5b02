/*
 * si_binary.h -- C-ABI of arithmetic against graph constants: out = stage1(stage0(x, c0), c1), the kernel behind a BinaryOp whose other
 * operand is a pnnx.Attribute (FrozenBatchNorm2d's x * scale + shift, layer scale, learned position embeddings, base grids, anchor tables).
 * The symbols live in libsi_hip.so beside those of include/si_hip.h; they have a header of their own as include/si_pad.h and
 * include/si_act.h have.
 *
 * Operands.  `x` and `out` are views of extents d[0..3] in storage order: d[3] is contiguous, consecutive "pixels" (the index
 * (i0 * d[1] + i1) * d[2] + i2) lie x_ld / out_ld elements apart, and what lies between two pixels (ld > d[3]) is never read and never
 * written.  out == x (the same pointer and stride) is allowed; any other overlap is not.  A constant is a dense tensor addressed by four
 * element strides: element (i0, i1, i2, i3) is c[i0 * s[0] + i1 * s[1] + i2 * s[2] + i3 * s[3]], and a stride is 0 where the constant is
 * broadcast.  A constant is only read.
 *
 * Stages.  One or two; stage k computes op[k](v, ck) with one of the ten BinaryOp codes of pnnx's expression lowering -- 0 add, 1 sub,
 * 2 mul, 3 div, 6 pow, 10 atan2, the value on the left -- and their operand-reversed forms 7 (c - v), 8 (c / v), 9 (pow(c, v)),
 * 11 (atan2(c, v)) for "constant on the left".
 *
 * Arithmetic.  fp32 throughout, no contraction of a multiply and an add into an fma, IEEE (correctly rounded) division, the library's
 * powf / atan2f.  The fp16 entry reads halves (x and both constants), computes in fp32 and rounds to half, round-to-nearest-even, ONCE
 * AFTER EACH STAGE: a two-stage launch has the bits of two one-stage launches, in fp32 and in fp16.  No LDS, no atomics, no workspace:
 * every launch is safe inside a captured graph and two launches give the same bits.
 *
 * Three forms (si_hip_binary_const_kernel_name reports which), each with a 16-byte arm (4 floats / 8 halves of x and out per lane, when
 * d[3], both strides and both pointers allow it) and a single-element arm:
 *     chan    every constant varies along d[3] only (s[0] = s[1] = s[2] = 0): a lane keeps its run of the constants in registers and
 *             walks over pixels
 *     pixel   every constant is constant along d[3] (s[3] = 0): one scalar per pixel and stage
 *     full    anything else: the pixel index is decomposed by magic division (no hardware division in the loop); a constant whose s[3]
 *             is 1 and whose other strides and pointer are 16-byte multiples is read as 16-byte vectors too
 * The grid is capped and the kernels grid-stride; grid_cap lowers the cap (tests: several passes over a small tensor).
 *
 * Refused before any device call: a null descriptor or pointer (c1 only with two stages), stages outside 1..2, a non-positive extent,
 * x_ld or out_ld below d[3], a negative constant stride or grid_cap, and extents or strides with which an operand's last element lies
 * at or beyond 2^31 - 1 elements (SI_E_BADARG); an op code outside the ten (SI_E_UNSUPPORTED).
 */
#ifndef SI_BINARY_H_
#define SI_BINARY_H_

#include "si_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct SiBinaryDesc {
    int d[4];            /* extents of x and out, storage order */
    int x_ld, out_ld;    /* pixel strides in elements, >= d[3] */
    int stages;          /* 1 or 2 */
    int op[2];           /* BinaryOp code of each stage */
    int c0_stride[4];    /* element strides of the first constant; 0: broadcast */
    int c1_stride[4];    /* ... of the second (two stages) */
    int grid_cap;        /* 0: the default cap; > 0: at most this many workgroups */
} SiBinaryDesc;

int si_hip_binary_const_f32(const SiBinaryDesc* d, const float* x, const float* c0, const float* c1, float* out, si_stream_t stream);

/* half x, half constants, half out */
int si_hip_binary_const_f16(const SiBinaryDesc* d, const void* x, const void* c0, const void* c1, void* out, si_stream_t stream);

/* the kernel a launch with these pointers takes: "binary_const_kernel<T, W, form>" with T float or _Float16, W the elements per lane
 * (4 / 8 or 1) and form chan, pixel or full; "none" for a call the launch would refuse */
const char* si_hip_binary_const_kernel_name(const SiBinaryDesc* d, const void* x, const void* c0, const void* c1, const void* out, int half);

#ifdef __cplusplus
}
#endif

#endif /* SI_BINARY_H_ */
