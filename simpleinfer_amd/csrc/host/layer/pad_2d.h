// layer/pad_2d.h -- the explicit pads of the last two dimensions (torch semantics; no reference counterpart): nn.ReflectionPad2d,
// nn.ReplicationPad2d, nn.ZeroPad2d, nn.ConstantPad2d, nn.CircularPad2d and F.pad, one class -- si_hip_pad2d_f32 / _f16
// (include/si_pad.h), one launch, bits moved as they are.  The parameter keys are torch's constructor / functional argument
// names, which is what pnnx writes for the modules it passes through: `padding` (one int, or (l, r, t, b)) and, for
// nn.ConstantPad2d, `value`; F.pad: `pad` (2 ints: W only, or 4), `mode`, `value` (None: 0).
#ifndef SIMPLE_INFER_SRC_LAYER_PAD_2D_H_
#define SIMPLE_INFER_SRC_LAYER_PAD_2D_H_

#include "layer.h"
#include "layer_util.h"
#include "si_pad.h"

namespace SimpleInfer {

class Pad2d : public Layer {
public:
    virtual Status Init(const pnnx::Operator* op) override;
    virtual Status Deinit() override;
    virtual Status Validate() override;
    virtual Status Forward(const Tensor& input, Tensor& output) override;

    virtual const char* KernelName() const override;
    virtual bool HalfStorageOk(std::string& why) const override;
    // (Bytes: the base class's input bytes plus output bytes; no arithmetic: Flops stays 0)

public:
    int pad_l_ = 0, pad_r_ = 0, pad_t_ = 0, pad_b_ = 0;   // negative: crop
    int mode_ = SI_PAD_CONSTANT;
    float value_ = 0.0f;
    std::string unsupported_;   // why Validate refuses with kUnsupport (an unknown mode, more than two padded dimensions)

private:
    static bool StagesInput(const Tensor& input, const Tensor& output);
    bool MakeDesc(const Tensor& input, const Tensor& output, SiPad2dDesc& d) const;

    DeviceBuffer staging_dev_;   // the fp32 graph input rounded to half (fp16 storage only)
};

}  // namespace SimpleInfer

#endif
