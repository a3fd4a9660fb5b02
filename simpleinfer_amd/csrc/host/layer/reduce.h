// layer/reduce.h -- torch.mean, torch.sum, torch.amax and torch.amin (torch semantics; no reference counterpart), one class --
// si_hip_reduce_f32 / _f16 (include/si_reduce.h), one launch.  Parameters as pnnx writes them: `dim` an int or an int array ((2,3), (1));
// negative counts from the end, a repeated dim is an error, a missing dim (the reduction to a scalar) is kUnsupport; `keepdim` a bool
// (missing: False); `dtype`, if present, must be None.  The file's dims are NCHW (or [N, F]); Validate maps each to its NHWC axis as
// Softmax::NhwcAxis does and checks the file's output shape against the rule.
//
// keepdim=False is served in one case: dims {2, 3} of a rank-4 input, whose [N, C] result is the same memory as the [N, 1, 1, C] the
// kernel writes (the global pool in front of nn.Linear).  Every other keepdim=False, and a mask the C-ABI refuses (the channel dim
// together with another), is kUnsupport at load.
#ifndef SIMPLE_INFER_SRC_LAYER_REDUCE_H_
#define SIMPLE_INFER_SRC_LAYER_REDUCE_H_

#include "layer.h"
#include "layer_util.h"
#include "si_reduce.h"

namespace SimpleInfer {

class Reduce : public Layer {
public:
    virtual Status Init(const pnnx::Operator* op) override;
    virtual Status Validate() override;
    virtual Status Forward(const Tensor& input, Tensor& output) override;

    virtual const char* KernelName() const override;
    virtual double Flops() const override;
    // (Bytes: the base class's one read of the input plus one write of the output.  HalfStorageOk: the base class's -- halves in and
    // out run the fp16 kernel; a mixed pair at the graph boundary goes through the engine's fp32 fallback, as for Slice)

public:
    int op_code_ = SI_REDUCE_MEAN;   // SI_REDUCE_*
    std::vector<int> dims_;          // as the file has them
    bool keepdim_ = false;
    int axes_ = 0;                   // the NHWC mask, set by Validate

private:
    bool MakeDesc(const Tensor& input, const Tensor& output, SiReduceDesc& d) const;
};

}  // namespace SimpleInfer

#endif
