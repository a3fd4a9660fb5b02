// layer/functional_conv_2d.h -- F.conv2d whose FILTER IS AN OPERAND (torch semantics, zero padding; no reference counterpart) on the MI355X: one
// launch of si_hip_xcorr_f32 / _f16 (include/si_xcorr.h).  x [N, C, H, W] and w [O, C / groups, KH, KW] are rank-4 tensors, which this project
// stores NHWC: the filter tensor already lies as [O][KH][KW][C / groups], every filter one K-vector of the implicit GEMM, and the kernel reads
// it where it lies -- nothing is packed, at load or per forward.  groups == 1 is the dense form, groups == C == O the depthwise one; every other
// group count is kUnsupport at load.  The bias is absent or a graph constant (the layer keeps an fp32 copy of its own: the kernels' bias is fp32
// under both storage types); a bias that is an activation is kUnsupport.  A following activation is the launch's epilogue.
//
// A filter that is a graph constant never reaches this layer when it has no other reader: pnnx/lower_functional_conv.cpp rewrites the operator
// to nn.Conv2d before layers are created.
//
// The planner pass FuseCrossCorrelations (engine_plan.cpp) turns view -> view -> F.conv2d(groups = N C) -> view, the depthwise cross-correlation
// of the Siamese trackers, into ONE launch in the kernel's per-sample addressing on the operands in front of the views: SetPerSample().
#ifndef SIMPLE_INFER_SRC_LAYER_FUNCTIONAL_CONV_2D_H_
#define SIMPLE_INFER_SRC_LAYER_FUNCTIONAL_CONV_2D_H_

#include "layer.h"
#include "layer_util.h"
#include "si_xcorr.h"

namespace SimpleInfer {

class FunctionalConv2d : public Layer {
public:
    virtual Status Init(const pnnx::Operator* op) override;
    virtual Status Deinit() override;
    virtual Status Validate() override;
    virtual Status Forward(const std::vector<Tensor>& inputs, Tensor& output) override;

    virtual const char* KernelName() const override;
    virtual bool HalfStorageOk(std::string& why) const override;
    virtual double Flops() const override;

    // engine fusion hook: y = act(conv + bias)
    void SetFusion(int act, float act_param = 0.0f) {
        act_ = act;
        act_param_ = act_param;
    }

    // planner hook: x [N, C, H, W] and z [N, C, kh, kw] are the operands in front of the two views, `out` [N, C, Ho, Wo] the one behind the
    // third; filter n meets image n.  false: the shapes are not those of the pattern, and nothing has changed
    bool SetPerSample(TensorNode* x, TensorNode* z, TensorNode* out);
    bool PerSample() const { return per_sample_; }

public:
    int stride_h_ = 1, stride_w_ = 1, dilation_h_ = 1, dilation_w_ = 1, groups_ = 1;
    int pad_h_ = 0, pad_w_ = 0;   // padding=(ph, pw)
    bool same_ = false;           // padding='same': d (K - 1) per axis, the odd one on the far side
    bool has_bias_ = false;
    std::vector<float> bias_;

    int act_ = SI_ACT_NONE;
    float act_param_ = 0.0f;

private:
    // false: the operands are not rank-4 tensors the descriptor can be made of
    bool MakeDesc(const Tensor& x, const Tensor& w, const Tensor& out, SiXcorrDesc& d) const;
    Status Refuse(const std::string& why, Status status = Status::kUnsupport) const;

    bool per_sample_ = false;
    DeviceBuffer bias_dev_;
    bool bias_ready_ = false;
};

}  // namespace SimpleInfer

#endif
