#include "prelu.h"

#include <cstring>

namespace SimpleInfer {

DEFINE_LAYER_REGISTRY(PReLU);

Status PReLU::Init(const pnnx::Operator* op) {
    CHECK_STATUS(Layer::Init(op));
    CHECK_BOOL(Get(op, "num_parameters", num_parameters_));
    CHECK_BOOL(ReadVec(op, "weight", weight_));
    device_ready_ = false;
    return Status::kSuccess;
}

Status PReLU::Deinit() {
    slope_dev_.Free();
    device_ready_ = false;
    return Status::kSuccess;
}

Status PReLU::Validate() {
    CHECK_STATUS(Layer::Validate());
    CHECK_STATUS(ValidateShape(1, 1));
    CHECK_STATUS(ValidateFloatLogged("PReLU"));
    const std::vector<int>& is = input_tensor_nodes_[0]->tensor.Shape();
    if (!IsSameShape(is, output_tensor_nodes_[0]->tensor.Shape())) {
        LOG(ERROR) << "PReLU::Validate fail [error input/output shape]";
        return Status::kErrorShape;
    }
    if (2 != is.size() && 4 != is.size()) {
        LOG(ERROR) << "PReLU::Validate fail [a rank-" << is.size() << " input: ranks 2 and 4 only]";
        return Status::kUnsupport;
    }
    const int c = is.back();   // NHWC / [N, F]: the channels are last
    if ((1 != num_parameters_ && c != num_parameters_) || weight_.size() != (size_t)num_parameters_) {
        LOG(ERROR) << "PReLU::Validate fail [num_parameters " << num_parameters_ << " with " << weight_.size() << " weights for " << c
                   << " channels: 1 or the channel count]";
        return Status::kErrorShape;
    }
    return Status::kSuccess;
}

Status PReLU::PrepareDevice() {
    if (device_ready_) return Status::kSuccess;
    CHECK_BOOL(!weight_.empty());
    CHECK_STATUS(CheckHip(slope_dev_.Upload(weight_.data(), weight_.size() * sizeof(float)), "upload prelu"));
    device_ready_ = true;
    return Status::kSuccess;
}

Status PReLU::Forward(const Tensor& input, Tensor& output) {
    return RunOnDevice({&input}, {&output}, [this](const std::vector<Tensor>& in, std::vector<Tensor>& out) {
        if (IsHalf(in[0]) != IsHalf(out[0])) return Status::kUnsupport;
        CHECK_STATUS(PrepareDevice());
        size_t pixels = 0;
        int c = 0;
        if (!GetPixelsChannels(in[0], pixels, c) || in[0].NumElements() != out[0].NumElements()) return Status::kErrorShape;
        const int count = (int)weight_.size();
        if (1 != count && c != count) return Status::kErrorShape;
        const float* slope = slope_dev_.As<float>();
        if (IsHalf(in[0]))
            return CheckHip(si_hip_prelu_f16(in[0].RawData(), pixels, c, in[0].PixelStride(), slope, count, out[0].RawData(), out[0].PixelStride(), Stream()),
                            "PReLU");
        return CheckHip(si_hip_prelu_f32(in[0].Data<float>(), pixels, c, in[0].PixelStride(), slope, count, out[0].Data<float>(), out[0].PixelStride(),
                                         Stream()),
                        "PReLU");
    });
}

const char* PReLU::KernelName() const {
    if (input_tensor_nodes_.empty() || output_tensor_nodes_.empty()) return "prelu_kernel";
    const Tensor& in = input_tensor_nodes_[0]->tensor;
    const Tensor& out = output_tensor_nodes_[0]->tensor;
    size_t pixels = 0;
    int c = 0;
    if (!GetPixelsChannels(in, pixels, c) || !in.RawData() || !out.RawData()) return "prelu_kernel";
    return si_hip_prelu_kernel_name(in.RawData(), pixels, c, in.PixelStride(), (int)weight_.size(), out.RawData(), out.PixelStride(), IsHalf(in) ? 1 : 0);
}

// per element: the comparison and the multiply
double PReLU::Flops() const {
    if (input_tensor_nodes_.empty()) return 0.0;
    return 2.0 * (double)input_tensor_nodes_[0]->tensor.NumElements();
}

}  // namespace SimpleInfer
