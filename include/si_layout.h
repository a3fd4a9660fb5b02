/*
 * si_layout.h -- C-ABI of the layout algebra (csrc/host/layout_plan.h): what a chain of Tensor.permute / Tensor.reshape / Tensor.view /
 * torch.transpose / torch.squeeze / torch.unsqueeze does to the bytes of its input.  Pure host code in libsimpleinfer_amd.so: no device is
 * touched, so the rule can be tested against numpy on any machine.
 *
 * Shapes are the FILE's (NCHW order for rank 4).  A rank-4 tensor is stored NHWC with pixel stride in_ld (0: dense), every other rank dense
 * row-major; the output is dense in its own storage order.  The answer is "view" (the output's bytes are the input's, in order) or the loop
 * nest of include/si_permute.h: extents of the output, outermost first, with the input element stride of every loop dimension.
 *
 * Returns a SimpleInfer::Status as int: 0, 3 kErrorShape (the operators do not produce out_shape, a dimension out of range), 5 kUnsupport (a
 * reshape boundary that does not divide a stored dimension, an output of rank > 4 -- such a tensor cannot exist in memory here -- or a nest
 * of more than 4 dimensions: `nest` then still holds its first SI_LAYOUT_MAX_NEST dimensions and its true rank).
 */
#ifndef SI_LAYOUT_H_
#define SI_LAYOUT_H_

#ifdef __cplusplus
extern "C" {
#endif

#define SI_LAYOUT_PERMUTE 0   /* args: the dims, one per input dimension */
#define SI_LAYOUT_RESHAPE 1   /* args: the new shape; one entry may be -1 */
#define SI_LAYOUT_TRANSPOSE 2 /* args: dim0, dim1 */
#define SI_LAYOUT_SQUEEZE 3   /* args: dim (a dimension that is not 1 stays: torch's rule) */
#define SI_LAYOUT_UNSQUEEZE 4 /* args: dim */
#define SI_LAYOUT_IDENTITY 5  /* no args (Tensor.contiguous) */

#define SI_LAYOUT_MAX_NEST 8

typedef struct SiLayoutNest {
    int view;                                   /* 1: the output is the input's bytes in order */
    int rank;                                   /* loop dimensions of the copy (0 for a view of one element) */
    int dims[SI_LAYOUT_MAX_NEST];
    long long in_stride[SI_LAYOUT_MAX_NEST];
} SiLayoutNest;

/* op k has kind kinds[k] and nargs[k] arguments, laid end to end in args; negative dims count from the end */
int si_layout_plan(int in_rank, const int* in_shape, int in_ld, int n_ops, const int* kinds, const int* nargs, const int* args, int out_rank,
                   const int* out_shape, SiLayoutNest* nest);

#ifdef __cplusplus
}
#endif

#endif /* SI_LAYOUT_H_ */
