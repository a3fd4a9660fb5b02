// layer/param_activation.h -- the bounded / soft activations (torch semantics; no reference counterpart), one class on
// si_hip_param_act_f32 / _f16 (include/si_act.h), one launch:
//   nn.ReLU6, F.relu6          clamp 0, 6
//   nn.Hardtanh, F.hardtanh    clamp min_val (default -1), max_val (default 1); min_val > max_val is kFail at load, the values logged
//   torch.clamp                clamp min, max; either may be missing or None (-inf / +inf); both None is kUnsupport
//   nn.Softplus, F.softplus    softplus beta (default 1), threshold (default 20)
//   nn.Mish, F.mish            mish
// A numeric parameter may be written as a float or an int; a mistyped one is kFail.
//
// NOT an ActivationLayer, on purpose: FuseEpilogues folds every ActivationLayer into the convolution, transposed convolution or GroupNorm
// in front of it by its ActCode(), and the kernels' si_act (si_hip_internal.h) ends in `default: return v` -- a folded code the kernels do not know would
// drop the activation without a word.  This layer is always a launch of its own; folding ReLU6 / clamp / Mish into the epilogues is the
// named follow-up.
#ifndef SIMPLE_INFER_SRC_LAYER_PARAM_ACTIVATION_H_
#define SIMPLE_INFER_SRC_LAYER_PARAM_ACTIVATION_H_

#include "layer.h"
#include "layer_util.h"
#include "si_act.h"

namespace SimpleInfer {

class ParamActivation : public Layer {
public:
    virtual Status Init(const pnnx::Operator* op) override;
    virtual Status Validate() override;
    virtual Status Forward(const Tensor& input, Tensor& output) override;

    virtual const char* KernelName() const override { return "param_act"; }
    virtual double Flops() const override { return 0.0; }
    // (HalfStorageOk: the base class's -- true for halves in and out, which run the fp16 kernel; a mixed pair at the graph boundary goes
    // through the engine's fp32 fallback, as for Slice and Reduce)

public:
    int op_code_ = SI_PACT_CLAMP;   // SI_PACT_*
    float p0_ = 0.0f, p1_ = 0.0f;   // clamp: lo, hi; softplus: beta, threshold

private:
    bool MakeDesc(const Tensor& input, const Tensor& output, SiParamActDesc& d) const;
};

}  // namespace SimpleInfer

#endif
