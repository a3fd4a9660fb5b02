#include "param_activation.h"

#include <cmath>
#include <cstring>

namespace SimpleInfer {

DEFINE_LAYER_REGISTRY(ParamActivation);

Status ParamActivation::Init(const pnnx::Operator* op) {
    CHECK_STATUS(Layer::Init(op));
    const std::string& t = op->type;
    bool have0 = false, have1 = false;
    if (t == "nn.ReLU6" || t == "F.relu6") {
        op_code_ = SI_PACT_CLAMP;
        p0_ = 0.0f;
        p1_ = 6.0f;
    } else if (t == "nn.Hardtanh" || t == "F.hardtanh") {
        op_code_ = SI_PACT_CLAMP;
        p0_ = -1.0f;
        p1_ = 1.0f;
        CHECK_BOOL(Number(op, "min_val", p0_, have0));
        CHECK_BOOL(Number(op, "max_val", p1_, have1));
        if (!(p0_ <= p1_)) {
            LOG(ERROR) << "ParamActivation::Init fail [" << t << " with min_val " << p0_ << " > max_val " << p1_ << "]";
            return Status::kFail;
        }
    } else if (t == "torch.clamp") {
        op_code_ = SI_PACT_CLAMP;
        p0_ = -INFINITY;
        p1_ = INFINITY;
        CHECK_BOOL(Number(op, "min", p0_, have0));
        CHECK_BOOL(Number(op, "max", p1_, have1));
        if (!have0 && !have1) {
            LOG(ERROR) << "ParamActivation::Init fail [torch.clamp with neither min nor max]";
            return Status::kUnsupport;
        }
        if (std::isnan(p0_) || std::isnan(p1_)) {
            LOG(ERROR) << "ParamActivation::Init fail [torch.clamp with a NaN bound]";
            return Status::kFail;
        }
    } else if (t == "nn.Softplus" || t == "F.softplus") {
        op_code_ = SI_PACT_SOFTPLUS;
        p0_ = 1.0f;
        p1_ = 20.0f;
        CHECK_BOOL(Number(op, "beta", p0_, have0));
        CHECK_BOOL(Number(op, "threshold", p1_, have1));
        if (!std::isfinite(p0_) || p0_ == 0.0f || std::isnan(p1_)) {
            LOG(ERROR) << "ParamActivation::Init fail [" << t << " with beta " << p0_ << ", threshold " << p1_ << "]";
            return Status::kFail;
        }
    } else {   // nn.Mish, F.mish
        op_code_ = SI_PACT_MISH;
        p0_ = p1_ = 0.0f;
    }
    return Status::kSuccess;
}

Status ParamActivation::Validate() {
    CHECK_STATUS(Layer::Validate());
    CHECK_STATUS(ValidateShape(1, 1));
    CHECK_STATUS(ValidateFloatLogged("ParamActivation"));
    const Tensor& in = input_tensor_nodes_[0]->tensor;
    const Tensor& out = output_tensor_nodes_[0]->tensor;
    if (!IsSameShape(in.Shape(), out.Shape())) {
        LOG(ERROR) << "ParamActivation::Validate fail [error input/output shape]";
        return Status::kErrorShape;
    }
    SiParamActDesc d;
    if (!MakeDesc(in, out, d)) return Status::kErrorShape;
    if (0 == strcmp("none", si_hip_param_act_kernel_name(&d, nullptr, nullptr, 0))) {
        LOG(ERROR) << "ParamActivation::Validate fail [the kernels refuse this tensor (element offsets beyond 31 bits)]";
        return Status::kUnsupport;
    }
    return Status::kSuccess;
}

bool ParamActivation::MakeDesc(const Tensor& input, const Tensor& output, SiParamActDesc& d) const {
    size_t pixels = 0, opix = 0;
    int c = 0, oc = 0;
    if (!GetPixelsChannels(input, pixels, c) || !GetPixelsChannels(output, opix, oc) || pixels != opix || c != oc) return false;
    memset(&d, 0, sizeof(d));
    d.op = op_code_;
    d.p0 = p0_;
    d.p1 = p1_;
    d.pixels = pixels;
    d.c = c;
    d.in_ld = input.PixelStride();
    d.out_ld = output.PixelStride();
    return true;
}

Status ParamActivation::Forward(const Tensor& input, Tensor& output) {
    return ForwardDesc(si_hip_param_act_f32, si_hip_param_act_f16, "ParamActivation", input, output, [this](auto&... a) { return MakeDesc(a...); });
}

}  // namespace SimpleInfer
