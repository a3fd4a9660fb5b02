// layer/avg_pool_2d.h -- nn.AvgPool2d and F.avg_pool2d (torch semantics; no reference counterpart), one class -- si_hip_avgpool2d_f32 /
// _f16 (include/si_pool.h), one launch.  The parameter keys are torch's constructor / functional argument names, which is what pnnx
// writes: `kernel_size`, `stride`, `padding` (pairs), `ceil_mode`, `count_include_pad`, `divisor_override` (an int or None).  The file's
// output shape must be the rule's for the file's ceil_mode (kErrorShape); padding > kernel_size / 2 and divisor_override = 0 are
// kUnsupport (torch refuses them too).
#ifndef SIMPLE_INFER_SRC_LAYER_AVG_POOL_2D_H_
#define SIMPLE_INFER_SRC_LAYER_AVG_POOL_2D_H_

#include "layer.h"
#include "layer_util.h"
#include "si_pool.h"

namespace SimpleInfer {

class AvgPool2d : public Layer {
public:
    virtual Status Init(const pnnx::Operator* op) override;
    virtual Status Validate() override;
    virtual Status Forward(const Tensor& input, Tensor& output) override;

    virtual const char* KernelName() const override;
    // (Bytes: the base class's input bytes plus output bytes)

    // the rule's output size of one axis (include/si_pool.h)
    static int OutSize(int i, int k, int s, int p, bool ceil_mode);

public:
    int kernel_h_ = 0, kernel_w_ = 0;
    int stride_h_ = 0, stride_w_ = 0;
    int padding_h_ = 0, padding_w_ = 0;
    bool ceil_mode_ = false;
    bool count_include_pad_ = true;
    bool has_divisor_override_ = false;
    int divisor_override_ = 0;

private:
    bool MakeDesc(const Tensor& input, const Tensor& output, SiAvgPool2dDesc& d) const;
};

}  // namespace SimpleInfer

#endif
