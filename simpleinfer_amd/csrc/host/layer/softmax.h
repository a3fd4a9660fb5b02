// layer/softmax.h -- nn.Softmax, nn.LogSoftmax, nn.Softmax2d, F.softmax and F.log_softmax (torch semantics; no reference counterpart),
// one class -- si_hip_softmax_f32 / _f16 (include/si_softmax.h), one launch.  The parameter key is torch's `dim` (an int, negative
// counts from the end), which is what pnnx writes for the four types that carry it; nn.Softmax2d has none and is dim = -3.  The file's
// dim is NCHW (or [N, F]); Validate maps it to the NHWC axis as Cat::NhwcAxis does and refuses other ranks and out-of-range dims.
#ifndef SIMPLE_INFER_SRC_LAYER_SOFTMAX_H_
#define SIMPLE_INFER_SRC_LAYER_SOFTMAX_H_

#include "layer.h"
#include "layer_util.h"
#include "si_softmax.h"

namespace SimpleInfer {

class Softmax : public Layer {
public:
    virtual Status Init(const pnnx::Operator* op) override;
    virtual Status Validate() override;
    virtual Status Forward(const Tensor& input, Tensor& output) override;

    virtual const char* KernelName() const override;
    virtual double Flops() const override;
    // (Bytes: the base class's one read plus one write of the tensor -- the algorithmic traffic, whichever form runs)

    // the NHWC axis of torch's dim on a tensor of this rank (2 or 4); -1: neither
    static int NhwcAxis(int dim, int rank);

public:
    int dim_ = 1;        // as the file has it
    bool log_ = false;   // nn.LogSoftmax / F.log_softmax
    int axis_ = -1;      // set by Validate

private:
    bool MakeDesc(const Tensor& input, const Tensor& output, SiSoftmaxDesc& d) const;
};

}  // namespace SimpleInfer

#endif
