// layer/conv_1d.h -- nn.Conv1d (torch semantics, zero padding; no reference counterpart) on the MI355X: one launch of si_hip_conv1d_f32 / _f16
// (include/si_conv1d.h) on rank-3 operands [N, C, L] in their native layout, the positions contiguous.  Bias and a fused activation run in
// the kernel's epilogue.  Deliberately NOT a Conv2d with H = 1: every Conv2d kernel is NHWC, and going through one costs two permute launches.
#ifndef SIMPLE_INFER_SRC_LAYER_CONV_1D_H_
#define SIMPLE_INFER_SRC_LAYER_CONV_1D_H_

#include "layer.h"
#include "layer_util.h"
#include "si_conv1d.h"

namespace SimpleInfer {

class Conv1d : public Layer {
public:
    virtual Status Init(const pnnx::Operator* op) override;
    virtual Status Deinit() override;
    virtual Status Validate() override;
    virtual Status Forward(const Tensor& input, Tensor& output) override;

    virtual const char* KernelName() const override;
    virtual bool HalfStorageOk(std::string& why) const override;
    virtual double Flops() const override;
    virtual double Bytes() const override;

    // engine fusion hook: y = act(conv + bias)
    void SetFusion(int act, float act_param = 0.0f) {
        act_ = act;
        act_param_ = act_param;
    }

public:
    int in_channels_ = 0;
    int out_channels_ = 0;
    int kernel_ = 0;
    int stride_ = 1;
    int dilation_ = 1;
    int groups_ = 1;
    int pad_left_ = 0, pad_right_ = 0;   // padding='same': d (K - 1) split with the odd one on the right
    bool same_ = false;
    bool use_bias_ = false;
    std::string padding_mode_ = "zeros";
    std::vector<float> weight_;   // [Cout][Cin/groups][K], the pnnx attribute layout
    std::vector<float> bias_;

    int act_ = SI_ACT_NONE;
    float act_param_ = 0.0f;

private:
    // false: the operands are not rank-3 tensors the descriptor can be made of
    bool MakeDesc(const Tensor& in, const Tensor& out, SiConv1dDesc& d) const;
    Status PrepareDevice(bool half);
    // does the dense fp16 kernel serve this filter ((C / groups) % 8 == 0, or plain depthwise)?
    bool HalfKernel() const;

    DeviceBuffer weight_dev_, bias_dev_;
    bool device_ready_ = false;
    bool prepared_half_ = false;
};

}  // namespace SimpleInfer

#endif
