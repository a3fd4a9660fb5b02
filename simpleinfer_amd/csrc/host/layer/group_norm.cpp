#include "group_norm.h"

#include <cstring>

namespace SimpleInfer {

DEFINE_LAYER_REGISTRY(GroupNorm);

// nn.GroupNorm: num_groups, num_channels, eps, affine (+ weight, bias of shape (C) when affine);
// nn.InstanceNorm2d: num_features, eps, affine, track_running_stats (+ weight, bias when affine).  A missing key is kFail.
Status GroupNorm::Init(const pnnx::Operator* op) {
    CHECK_STATUS(Layer::Init(op));
    CHECK_BOOL(Get(op, "eps", eps_));
    CHECK_BOOL(Get(op, "affine", use_affine_));
    if (op->type == "nn.InstanceNorm2d") {
        CHECK_BOOL(Get(op, "num_features", num_channels_));
        num_groups_ = 0;
        CHECK_BOOL(Get(op, "track_running_stats", track_running_stats_));
    } else {
        CHECK_BOOL(Get(op, "num_groups", num_groups_));
        CHECK_BOOL(Get(op, "num_channels", num_channels_));
        CHECK_BOOL(num_groups_ > 0);
    }
    CHECK_BOOL(num_channels_ > 0 && eps_ >= 0.0f);
    if (use_affine_) {
        CHECK_BOOL(ReadVec(op, "weight", weight_));
        CHECK_BOOL(ReadVec(op, "bias", bias_));
        CHECK_BOOL(weight_.size() == bias_.size());
    }
    params_ready_ = false;
    return Status::kSuccess;
}

Status GroupNorm::Deinit() {
    params_dev_.Free();
    workspace_dev_.Free();
    params_ready_ = false;
    return Status::kSuccess;
}

Status GroupNorm::Validate() {
    CHECK_STATUS(Layer::Validate());
    CHECK_STATUS(ValidateShape(1, 1));
    CHECK_STATUS(ValidateFloatLogged("GroupNorm"));
    if (track_running_stats_) {
        LOG(ERROR) << "GroupNorm::Validate fail [InstanceNorm2d with track_running_stats=True normalises with stored statistics in eval mode: "
                      "that is a BatchNorm, not this kernel]";
        return Status::kUnsupport;
    }
    Dims4 in, out;
    if (!GetDims4(input_tensor_nodes_[0]->tensor, in) || !GetDims4(output_tensor_nodes_[0]->tensor, out)) {
        LOG(ERROR) << "GroupNorm::Validate fail [input and output must be rank-4]";
        return Status::kErrorShape;
    }
    if (!IsSameShape(input_tensor_nodes_[0]->tensor.Shape(), output_tensor_nodes_[0]->tensor.Shape())) {
        LOG(ERROR) << "GroupNorm::Validate fail [error input/output shape]";
        return Status::kErrorShape;
    }
    if (in.c != num_channels_) {
        LOG(ERROR) << "GroupNorm::Validate fail [" << in.c << " channels, the layer was written for " << num_channels_ << "]";
        return Status::kErrorShape;
    }
    if (use_affine_ && weight_.size() != (size_t)in.c) {
        LOG(ERROR) << "GroupNorm::Validate fail [weight / bias of " << weight_.size() << " elements for " << in.c << " channels]";
        return Status::kErrorShape;
    }
    const int groups = num_groups_ > 0 ? num_groups_ : in.c;
    if (in.c % groups != 0) {
        LOG(ERROR) << "GroupNorm::Validate fail [" << in.c << " channels do not divide into " << groups << " groups]";
        return Status::kErrorShape;
    }
    return Status::kSuccess;
}

bool GroupNorm::MakeDesc(const Tensor& input, const Tensor& output, SiGroupNormDesc& d) const {
    Dims4 id, od;
    if (!GetDims4(input, id) || !GetDims4(output, od) || id.c != od.c || id.n != od.n || id.h != od.h || id.w != od.w) return false;
    memset(&d, 0, sizeof(d));
    d.n = id.n; d.h = id.h; d.w = id.w; d.c = id.c;
    d.groups = num_groups_ > 0 ? num_groups_ : id.c;
    d.in_ld = input.PixelStride();
    d.out_ld = output.PixelStride();
    d.eps = eps_;
    d.affine = use_affine_ ? 1 : 0;
    d.act = act_;
    d.act_param = act_param_;
    return true;
}

// gamma / beta once; the workspace whenever the shape asks for more than there is (the engine's first Forward is never captured, and a
// shape change rebuilds the plan: nothing is allocated during a graph capture)
Status GroupNorm::PrepareDevice(const SiGroupNormDesc& d) {
    if (!params_ready_ && use_affine_) {
        std::vector<float> all(weight_);
        all.insert(all.end(), bias_.begin(), bias_.end());
        CHECK_STATUS(CheckHip(params_dev_.Upload(all.data(), all.size() * sizeof(float)), "upload groupnorm weight / bias"));
    }
    params_ready_ = true;
    const size_t need = si_hip_groupnorm_workspace_bytes(&d);
    if (need > workspace_dev_.bytes()) CHECK_STATUS(CheckHip(workspace_dev_.Alloc(need), "groupnorm workspace"));
    return Status::kSuccess;
}

Status GroupNorm::Forward(const Tensor& input, Tensor& output) {
    return RunOnDevice({&input}, {&output}, [this](const std::vector<Tensor>& in, std::vector<Tensor>& out) {
        if (IsHalf(in[0]) != IsHalf(out[0])) return Status::kUnsupport;
        SiGroupNormDesc d;
        if (!MakeDesc(in[0], out[0], d) || d.c != num_channels_) return Status::kErrorShape;
        CHECK_STATUS(PrepareDevice(d));
        const float* gamma = use_affine_ ? params_dev_.As<float>() : nullptr;
        const float* beta = use_affine_ ? gamma + num_channels_ : nullptr;
        if (IsHalf(in[0]))
            return CheckHip(si_hip_groupnorm_f16(&d, in[0].RawData(), gamma, beta, out[0].RawData(), workspace_dev_.As<void>(), Stream()), "GroupNorm");
        return CheckHip(si_hip_groupnorm_f32(&d, in[0].Data<float>(), gamma, beta, out[0].Data<float>(), workspace_dev_.As<void>(), Stream()),
                        "GroupNorm");
    });
}

const char* GroupNorm::KernelName() const {
    return DescKernelName(si_hip_groupnorm_kernel_name, "groupnorm", [this](auto&... a) { return MakeDesc(a...); });
}

// per element: the Welford update (subtract, multiply-add, subtract, multiply-add) and the normalise (subtract, multiply, add)
double GroupNorm::Flops() const {
    if (input_tensor_nodes_.empty()) return 0.0;
    return 9.0 * (double)input_tensor_nodes_[0]->tensor.NumElements();
}

}  // namespace SimpleInfer
