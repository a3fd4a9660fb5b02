// layer/prelu.h -- nn.PReLU (torch semantics; no reference counterpart): y = x > 0 ? x : weight[ch] * x -- si_hip_prelu_f32 / _f16
// (include/si_superres.h), one launch.  Parameter `num_parameters` (1: one slope for every channel, or the channel count) and
// attribute `weight` of shape [num_parameters], torch's names, which is what pnnx writes for the module.  Rank 2 ([N, F]) and
// rank 4 tensors.  The slopes stay fp32 under fp16 storage.
#ifndef SIMPLE_INFER_SRC_LAYER_PRELU_H_
#define SIMPLE_INFER_SRC_LAYER_PRELU_H_

#include "layer.h"
#include "layer_util.h"
#include "si_superres.h"

namespace SimpleInfer {

class PReLU : public Layer {
public:
    virtual Status Init(const pnnx::Operator* op) override;
    virtual Status Deinit() override;
    virtual Status Validate() override;
    virtual Status Forward(const Tensor& input, Tensor& output) override;

    virtual const char* KernelName() const override;
    virtual double Flops() const override;

    Status PrepareDevice();

public:
    int num_parameters_ = 1;
    std::vector<float> weight_;

private:
    DeviceBuffer slope_dev_;
    bool device_ready_ = false;
};

}  // namespace SimpleInfer

#endif
