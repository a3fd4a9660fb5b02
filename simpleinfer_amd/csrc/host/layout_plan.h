// layout_plan.h -- the layout algebra: what a chain of Tensor.permute / reshape / view / torch.transpose / squeeze / unsqueeze does to the
// stored bytes of its input.  A pure function: no tensor, no device, no engine (tests/test_layout_cpu.py drives it through include/si_layout.h).
//
// The logical tensor is carried as a list of logical dimensions, each a list of SUB-DIMENSIONS (size, stride into the root input's storage):
//   start     rank 4 (N, C, H, W), stored NHWC with pixel stride ld: strides (H W ld, 1, W ld, ld); any other rank: dense row-major
//   permute / transpose    reorder the dimensions
//   squeeze / unsqueeze    drop / insert a dimension without sub-dimensions
//   reshape / view         lay the sub-dimensions end to end in logical order (neighbours with t1 == s2 t2 merged: one run) and regroup them by
//                          the new shape (-1 from the element count);
//                          a boundary inside a sub-dimension (s, t) splits it into (s / k, t k), (k, t); one that does not divide: kUnsupport
//   end       the sub-dimensions in the OUTPUT's storage order (rank 4: dimensions 0, 2, 3, 1), sizes of 1 dropped, neighbours with
//             t1 == s2 t2 merged.  One dimension of stride 1 (or none): a view.  More than 4: kUnsupport.
#ifndef SIMPLE_INFER_SRC_LAYOUT_PLAN_H_
#define SIMPLE_INFER_SRC_LAYOUT_PLAN_H_

#include <string>
#include <vector>

#include "types.h"

namespace SimpleInfer {

struct LayoutOp {
    enum Kind { kPermute = 0, kReshape = 1, kTranspose = 2, kSqueeze = 3, kUnsqueeze = 4, kIdentity = 5 };
    int kind = kIdentity;
    std::vector<int> args;
};

struct LayoutPlan {
    bool view = false;
    std::vector<int> dims;              // the output loop nest, outermost first (may be longer than 4 when the status says so)
    std::vector<long long> in_stride;
    std::vector<int> out_shape;         // the file shape the chain produces
    bool late = false;                  // a kUnsupport that fusing the operator into a chain may lift (rank > 4 in memory, a nest of > 4 dimensions)
};

// kErrorShape: the chain does not fit its shapes (`out_shape` given and different, a dim out of range, a count that does not match);
// kUnsupport: a non-dividing boundary, an output of rank > 4, a nest of more than 4 dimensions (plan.dims is filled all the same).
// out_shape may be null: the chain's own result is taken (plan.out_shape).
Status PlanLayout(const std::vector<int>& in_shape, int in_ld, const std::vector<LayoutOp>& chain, const std::vector<int>* out_shape,
                  LayoutPlan& plan, std::string& why);

}  // namespace SimpleInfer

#endif
