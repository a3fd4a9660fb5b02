/*
 * si_act.h -- C-ABI of the activations that carry parameters of their own or need an accurate evaluation: clamp (nn.ReLU6, nn.Hardtanh,
 * torch.clamp), softplus (nn.Softplus) and mish (nn.Mish), torch's semantics.  The symbols live in libsi_hip.so beside those of
 * include/si_hip.h; they have a header of their own as include/si_softmax.h, include/si_slice.h and include/si_reduce.h have.
 *
 * Tensors are [pixels, c] with pixel strides in_ld / out_ld (in elements) on both sides: what lies between two pixels (ld > c) is never
 * read and never written.  `in` and `out` must not overlap (two disjoint channel slices of one buffer with a common pixel stride do not
 * overlap: the rule of include/si_reduce.h).
 *
 * Arithmetic, the same in every arm.  The fp16 entry computes in float32 on the widened half and rounds once, to nearest even, at the
 * store.
 *   clamp     y = x < lo ? lo : x;  out = y > hi ? hi : y     (p0 = lo, p1 = hi; either may be -inf / +inf)
 *             A selection: it never rounds and is bit-exact in fp32.  A NaN passes through (both comparisons are false); lo > hi gives hi
 *             everywhere (torch's documented rule); -0.0 against lo = 0 stays -0.0 (it is not below the bound).  With fp16 storage the
 *             widened value is clamped against the fp32 bounds and rounded once at the store: exact whenever the result is the input or
 *             a bound fp16 can hold.
 *   softplus  z = beta * x;  out = z > threshold ? x : (max(z, 0) + log1p(exp(-|z|))) / beta     (p0 = beta, p1 = threshold)
 *             torch's rule, log1p(exp(z)) / beta below the threshold, in the form that neither overflows nor loses the negative tail:
 *             log(1 + exp(z)) is 0 below z = -16.6 where the true value is about e^z.  expf and logf are the library's accurate functions,
 *             the division is IEEE, and log1p(e) for the e in [0, 1] that occurs here is u = 1 + e, log(u) - ((u - 1) - e) / u: the
 *             logarithm of the rounded sum, corrected by the sum's rounding error (exact in fp32), which is e itself once u is 1.  z is
 *             rounded to fp32: for a beta that is no power of two the tail carries that rounding, |z| * 2^-24 relative.
 *   mish      out = x * tanh(softplus(x)) = x * n / (n + 2),  n = e * (e + 2),  e = exp(min(x, SI_PACT_MISH_CUT));  out = x above the cut
 *             torch's definition (beta 1, no threshold) with one exponential: tanh(log(1 + e)) = ((1 + e)^2 - 1) / ((1 + e)^2 + 1).
 *             Every operation rounds to fp32 on its own (no contraction), the division is IEEE.  Above the cut the factor is 1 to fp32's
 *             precision (it is from x = 9.1 on; the cut only has to keep e * e finite).
 *   special values: a NaN gives NaN.  softplus(-inf) = 0, softplus(+inf) = +inf, mish(+inf) = +inf; mish(-inf) = -inf * 0 = NaN as
 *             torch's formula gives (silu(-inf) of include/si_hip.h does the same).
 *
 * Arms, chosen from c, both strides, both pointers' alignment and -- the first one -- whether pixels * c fills whole vectors;
 * si_hip_param_act_kernel_name reports the instantiation:
 *   dense     in_ld == out_ld == c, both pointers 16-byte aligned, pixels * c a multiple of the vector: the tensor as ONE row of
 *             16-byte vectors (an odd c still takes the vector path)
 *   vector    c, in_ld and out_ld multiples of the vector (4 floats / 8 halves), both pointers aligned: 16-byte vectors inside each pixel
 *   element   everything else: single elements
 * One lane per item, consecutive lanes take consecutive addresses, a grid-stride loop of at most 2048 workgroups of 256 lanes.  The
 * operator is a template parameter (no per-element switch), the two parameters are kernel arguments.  No LDS, no scratch, no
 * workspace, no atomics: two launches give the same bits, an element does not depend on any other, and every launch is safe inside a
 * captured graph.
 *
 * Refused before any device call: a null descriptor or tensor, pixels == 0, c <= 0, in_ld < c, out_ld < c, op outside 0 .. 2, a NaN
 * clamp bound, a softplus beta that is zero or not finite, a NaN softplus threshold, overlapping in / out (SI_E_BADARG); element
 * offsets that do not fit 31 bits (SI_E_UNSUPPORTED).  mish ignores p0 and p1.
 */
#ifndef SI_ACT_H_
#define SI_ACT_H_

#include "si_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { SI_PACT_CLAMP = 0, SI_PACT_SOFTPLUS = 1, SI_PACT_MISH = 2 };

/* mish returns x above this: exp(30)^2 is still finite in fp32, and n / (n + 2) rounds to 1 long before */
enum { SI_PACT_MISH_CUT = 30 };

typedef struct SiParamActDesc {
    int op;              /* SI_PACT_* */
    float p0, p1;        /* clamp: lo, hi (either may be -inf / +inf); softplus: beta, threshold; mish: ignored */
    size_t pixels;
    int c, in_ld, out_ld;
} SiParamActDesc;

int si_hip_param_act_f32(const SiParamActDesc* d, const float* in, float* out, si_stream_t stream);

/* half in, half out */
int si_hip_param_act_f16(const SiParamActDesc* d, const void* in, void* out, si_stream_t stream);

/* the kernel a launch with these pointers takes: "param_act_kernel<OP, float, 4>", "<OP, float, 1>", "<OP, _Float16, 8>" or
 * "<OP, _Float16, 1>" with OP one of clamp, softplus, mish; "none" for a descriptor the launch would refuse (the pointers are looked at
 * for their alignment only) */
const char* si_hip_param_act_kernel_name(const SiParamActDesc* d, const void* in, const void* out, int half);

#ifdef __cplusplus
}
#endif

#endif /* SI_ACT_H_ */
