// layer/layout.h -- Tensor.permute / torch.permute, Tensor.reshape / Tensor.view, torch.transpose, torch.squeeze / torch.unsqueeze and
// Tensor.contiguous (torch semantics, no reference counterpart), one class.  Dims are the file's (NCHW for rank 4; negative: from the end).
//
// The parameter keys are pnnx's spellings for the operators it passes through -- no pnnx converter was at hand to confirm them on an export:
//   Tensor.permute / torch.permute    dims=(..)
//   Tensor.reshape / Tensor.view      shape=(..), one entry may be -1; the form with the shape as a second input operand is kUnsupport
//   torch.transpose                   dim0= dim1=
//   torch.squeeze / torch.unsqueeze   dim=
//   Tensor.contiguous                 none (identity)
//
// The output operand's shape in the file is the truth: Validate() runs the layout algebra (layout_plan.h) over the operator -- or, after
// EngineImpl::FuseLayoutChains, over the whole chain of operators this layer stands for -- and a result that differs is kErrorShape.  Under
// SetOption("batch", B) a leading shape= entry equal to the file's batch follows the re-batch; a reshape that folds the batch into another
// dimension is served at the file's batch only (kUnsupport otherwise).  What can only be decided once the chains are fused -- a tensor of rank
// > 4 that would have to exist in memory, a copy of more than 4 loop dimensions -- is kept and reported by Final(), still at LoadModel.
//
// Forward: a plan that is a view whose output the engine has pointed at the input's buffer (EngineImpl::AliasViews) launches nothing; every
// other plan is ONE si_hip_permute_* launch (include/si_permute.h), fp32 or fp16 storage alike.
#ifndef SIMPLE_INFER_SRC_LAYER_LAYOUT_H_
#define SIMPLE_INFER_SRC_LAYER_LAYOUT_H_

#include "layer.h"
#include "layer_util.h"
#include "layout_plan.h"
#include "si_permute.h"

namespace SimpleInfer {

class Layout : public Layer {
public:
    virtual Status Init(const pnnx::Operator* op) override;
    virtual Status Validate() override;
    virtual Status Forward(const Tensor& input, Tensor& output) override;

    // "view" (the output is in place: no launch) or the form of the launch -- for the tensors bound now
    virtual const char* KernelName() const override;
    // (no arithmetic: Flops stays 0)

    // the operators this layer stands for, parameters resolved against the bound shapes (one after Validate; a chain after SetChain)
    const std::vector<LayoutOp>& Chain() const { return chain_; }
    // the plan of Chain() over the bound input and output (valid when Final() succeeds)
    const LayoutPlan& Plan() const { return plan_; }
    bool IsView() const { return final_ == Status::kSuccess && plan_.view; }
    // the chain `ops` from `root`'s storage to this layer's output: planned first, taken only when it can be served
    bool TryChain(TensorNode* root, const std::vector<LayoutOp>& ops);
    // what Validate() had to leave open; logs the reason when it is not kSuccess
    Status Final() const;

    // the file-order shape of a stored tensor (rank 4: NHWC -> NCHW)
    static std::vector<int> FileShape(const Tensor& t);

private:
    Status PlanBound(const std::vector<LayoutOp>& ops, const Tensor& in, const Tensor& out, LayoutPlan& plan, Status& final, std::string& why) const;
    bool Desc(const Tensor& in, const Tensor& out, SiPermuteDesc& d) const;

    LayoutOp own_;                   // this operator as the file has it
    std::vector<LayoutOp> chain_;
    LayoutPlan plan_;
    Status final_ = Status::kFail;
    std::string final_why_;
};

}  // namespace SimpleInfer

#endif
