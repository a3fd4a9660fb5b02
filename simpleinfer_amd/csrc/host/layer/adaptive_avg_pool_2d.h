// layer/adaptive_avg_pool_2d.h -- nn.AdaptiveAvgPool2d / F.adaptive_avg_pool2d: global mean for 1x1, else uniform windows
// k = in/out where in % out == 0 (reference src/layer/adaptive_avg_pool_2d.cpp:54-116, which requires it); any other shape runs
// torch's general windows on si_hip_avgpool2d_f32 / _f16 (include/si_pool.h, adaptive = 1).
#pragma once

#include "layer.h"
#include "layer_util.h"
#include "si_pool.h"

namespace SimpleInfer {

class AdaptiveAvgPool2d : public Layer {
public:
    virtual Status Init(const pnnx::Operator* op) override;
    virtual Status Validate() override;
    virtual Status Forward(const Tensor& input, Tensor& output) override;
    virtual const char* KernelName() const override;

public:
    int output_h_ = 0;
    int output_w_ = 0;

private:
    // the descriptor of the general form; false: the shapes divide (or are not rank 4) and the uniform-window kernels run
    static bool MakeGeneralDesc(const Tensor& input, const Tensor& output, SiAvgPool2dDesc& d);
};

}  // namespace SimpleInfer
