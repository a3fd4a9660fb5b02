// layer/deform_conv_2d.h -- torchvision.ops.DeformConv2d (torch semantics; no reference counterpart) on the MI355X: one launch of
// si_hip_deform_conv2d_f32 (include/si_deform.h: the bilinear gather feeds an implicit GEMM on the fp32 matrix cores, bias and activation in
// its epilogue).  Two inputs (x, offset) are DCNv1, three (x, offset, mask) DCNv2; the offset-group count is read off the offset operand.
// fp32 only (an fp16-storage engine runs it between casts).  Deliberately NOT a Conv2d: none of the planner's Conv2d fusions apply to it.
#ifndef SIMPLE_INFER_SRC_LAYER_DEFORM_CONV_2D_H_
#define SIMPLE_INFER_SRC_LAYER_DEFORM_CONV_2D_H_

#include "layer.h"
#include "layer_util.h"
#include "si_deform.h"

namespace SimpleInfer {

class DeformConv2d : public Layer {
public:
    virtual Status Init(const pnnx::Operator* op) override;
    virtual Status Init(const std::map<std::string, pnnx::Parameter>& params,
                        const std::map<std::string, pnnx::Attribute>& attrs) override;
    virtual Status Deinit() override;
    virtual Status Validate() override;
    virtual Status Forward(const std::vector<Tensor>& inputs, Tensor& output) override;

    virtual const char* KernelName() const override;
    virtual bool HalfStorageOk(std::string& why) const override;
    virtual double Flops() const override;
    virtual double Bytes() const override;

    // engine fusion hook: y = act(deform_conv + bias)
    void SetFusion(int act, float act_param = 0.0f) {
        act_ = act;
        act_param_ = act_param;
    }

public:
    int in_channels_  = 0;
    int out_channels_ = 0;
    int kernel_h_ = 0, kernel_w_ = 0;
    int stride_h_ = 1, stride_w_ = 1;
    int padding_h_ = 0, padding_w_ = 0;
    int dilation_h_ = 1, dilation_w_ = 1;
    int groups_ = 1;
    bool use_bias_ = false;
    std::vector<float> weight_;   // [Cout][Cin/groups][kh][kw], the pnnx attribute layout
    std::vector<float> bias_;

    int act_ = SI_ACT_NONE;
    float act_param_ = 0.0f;

private:
    // false: the operands are not rank-4 tensors the descriptor can be made of
    bool MakeDesc(const std::vector<const Tensor*>& in, const Tensor& output, SiDeformConv2dDesc& d) const;
    Status PrepareDevice();

    DeviceBuffer weight_dev_, bias_dev_;
    bool device_ready_ = false;
};

}  // namespace SimpleInfer

#endif
