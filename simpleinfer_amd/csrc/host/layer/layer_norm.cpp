#include "layer_norm.h"

#include <cstring>

namespace SimpleInfer {

DEFINE_LAYER_REGISTRY(LayerNorm);

Status LayerNorm::Refuse(const std::string& why, Status status) const {
    LOG(ERROR) << "F.layer_norm [" << (op_ ? op_->name : std::string("-")) << "] refused [" << why << "]";
    return status;
}

Status LayerNorm::ReadConstant(const pnnx::Operator* op, size_t index, const char* what, std::vector<float>& dst) const {
    const pnnx::Operand* r = op->inputs[index];
    const pnnx::Operator* src = r ? r->producer : nullptr;
    if (!src || src->type != "pnnx.Attribute")
        return Refuse(std::string("the ") + what + " is an activation: only an absent " + what + " and a graph constant are served");
    auto data = src->attrs.find("data");
    if (data == src->attrs.end() || data->second.type != 1 || data->second.shape.size() != 1 ||
        data->second.data.size() != (size_t)data->second.shape[0] * sizeof(float))
        return Refuse(std::string("the constant ") + what + " is not a rank-1 fp32 tensor");
    dst.resize(data->second.shape[0]);
    memcpy(dst.data(), data->second.data.data(), data->second.data.size());
    return Status::kSuccess;
}

// A mistyped or missing key is kFail; an activation as weight or bias is kUnsupport; lengths are left for Validate.
Status LayerNorm::Init(const pnnx::Operator* op) {
    CHECK_STATUS(Layer::Init(op));
    normalized_shape_.clear();
    int one = 0;
    if (Get(op, "normalized_shape", one)) normalized_shape_.push_back(one);
    else CHECK_BOOL(Get(op, "normalized_shape", normalized_shape_) && !normalized_shape_.empty());
    eps_ = 1e-5f;
    if (FindParam(op, "eps")) CHECK_BOOL(GetNumber(op, "eps", eps_));
    CHECK_BOOL(eps_ >= 0.0f);
    has_weight_ = has_bias_ = false;
    weight_.clear();
    bias_.clear();
    device_ready_ = false;
    CHECK_BOOL(op->inputs.size() >= 1 && op->inputs.size() <= 3);
    constants_ = (int)op->inputs.size() - 1;
    if (constants_ == 0) {
        // the module form: its own attributes, unless elementwise_affine=False
        bool affine = true;
        if (FindParam(op, "elementwise_affine")) CHECK_BOOL(Get(op, "elementwise_affine", affine));
        if (affine && op->attrs.count("weight")) {
            CHECK_BOOL(ReadVec(op, "weight", weight_));
            has_weight_ = true;
        }
        if (affine && op->attrs.count("bias")) {
            CHECK_BOOL(ReadVec(op, "bias", bias_));
            has_bias_ = true;
        }
        return Status::kSuccess;
    }
    // the function: one operand behind x is the weight, unless the line says weight=None
    const bool first_is_bias = constants_ == 1 && FindParam(op, "weight") && IsNoneOrText(op, "weight");
    if (constants_ == 2 || !first_is_bias) {
        CHECK_STATUS(ReadConstant(op, 1, "weight", weight_));
        has_weight_ = true;
    }
    if (constants_ == 2 || first_is_bias) {
        CHECK_STATUS(ReadConstant(op, (size_t)constants_, "bias", bias_));
        has_bias_ = true;
    }
    return Status::kSuccess;
}

Status LayerNorm::Deinit() {
    weight_dev_.Free();
    bias_dev_.Free();
    device_ready_ = false;
    return Status::kSuccess;
}

Status LayerNorm::Validate() {
    CHECK_STATUS(Layer::Validate());
    CHECK_STATUS(ValidateShape(1 + constants_, 1));
    CHECK_STATUS(ValidateFloatLogged("LayerNorm"));
    const Tensor& in = input_tensor_nodes_[0]->tensor;
    const Tensor& out = output_tensor_nodes_[0]->tensor;
    const std::vector<int>& is = in.Shape();
    if (normalized_shape_.size() != 1)
        return Refuse("normalized_shape " + TupleString(normalized_shape_) + ": the norm over the last dimension alone is served");
    if (is.size() != 2 && is.size() != 3)
        return Refuse("a rank-" + std::to_string(is.size()) + " operand " + ShapeString(is) +
                      ": ranks 2 and 3 are served (a rank-4 tensor is stored NHWC: its last file dimension is not contiguous)");
    if (normalized_shape_[0] != is.back())
        return Refuse("normalized_shape " + TupleString(normalized_shape_) + " on an operand whose last dimension is " + std::to_string(is.back()),
                      Status::kErrorShape);
    if (!IsSameShape(is, out.Shape())) return Refuse("the output is " + ShapeString(out.Shape()) + ", the input " + ShapeString(is), Status::kErrorShape);
    if ((has_weight_ && (int)weight_.size() != is.back()) || (has_bias_ && (int)bias_.size() != is.back()))
        return Refuse("a weight of " + std::to_string(weight_.size()) + " / a bias of " + std::to_string(bias_.size()) + " values for " +
                          std::to_string(is.back()) + " features",
                      Status::kErrorShape);
    SiLayerNormDesc d;
    if (!MakeDesc(in, out, d) || 0 == strcmp("none", si_hip_layernorm_kernel_name(&d, nullptr, nullptr, 0)))
        return Refuse(ShapeString(is) + ": the kernels refuse this tensor (element offsets beyond 31 bits)");
    return Status::kSuccess;
}

bool LayerNorm::MakeDesc(const Tensor& input, const Tensor& output, SiLayerNormDesc& d) const {
    size_t rows = 0, orows = 0;
    int c = 0, oc = 0;
    if (!GetPixelsChannels(input, rows, c) || !GetPixelsChannels(output, orows, oc) || rows != orows || c != oc || rows > 0x7fffffffu) return false;
    memset(&d, 0, sizeof(d));
    d.rows = (int)rows;
    d.c = c;
    d.in_ld = input.PixelStride();
    d.out_ld = output.PixelStride();
    d.eps = eps_;
    return true;
}

Status LayerNorm::Launch(const Tensor& input, Tensor& output) {
    return RunOnDevice({&input}, {&output}, [this](const std::vector<Tensor>& in, std::vector<Tensor>& out) {
        const bool half = IsHalf(in[0]);
        if (IsHalf(out[0]) != half) return Status::kUnsupport;
        SiLayerNormDesc d;
        if (!MakeDesc(in[0], out[0], d)) return Status::kErrorShape;
        if (!device_ready_) {
            if (has_weight_) CHECK_STATUS(CheckHip(weight_dev_.Upload(weight_.data(), weight_.size() * sizeof(float)), "upload weight"));
            if (has_bias_) CHECK_STATUS(CheckHip(bias_dev_.Upload(bias_.data(), bias_.size() * sizeof(float)), "upload bias"));
            device_ready_ = true;
        }
        const float* const gamma = has_weight_ ? weight_dev_.As<float>() : nullptr;
        const float* const beta = has_bias_ ? bias_dev_.As<float>() : nullptr;
        const int rc = half ? si_hip_layernorm_f16(&d, in[0].RawData(), gamma, beta, out[0].RawData(), Stream())
                            : si_hip_layernorm_f32(&d, in[0].Data<float>(), gamma, beta, out[0].Data<float>(), Stream());
        return CheckHip(rc, "LayerNorm");
    });
}

Status LayerNorm::Forward(const Tensor& input, Tensor& output) { return Launch(input, output); }

// (the constants were read at Init: their operands are bound but never launched on)
Status LayerNorm::Forward(const std::vector<Tensor>& inputs, Tensor& output) {
    if (inputs.empty()) return Status::kUnsupport;
    return Launch(inputs[0], output);
}

const char* LayerNorm::KernelName() const {
    return DescKernelName(si_hip_layernorm_kernel_name, "layernorm", [this](auto&... a) { return MakeDesc(a...); });
}

// per element: two additions for the sums, the centring, the square, and up to three operations of the result
double LayerNorm::Flops() const {
    if (input_tensor_nodes_.empty()) return 0.0;
    return 7.0 * (double)input_tensor_nodes_[0]->tensor.NumElements();
}

// one read of x, one write of the output; gamma and beta once per workgroup, from cache
double LayerNorm::Bytes() const {
    if (input_tensor_nodes_.empty() || output_tensor_nodes_.empty()) return 0.0;
    return (double)input_tensor_nodes_[0]->tensor.ByteSize() + (double)output_tensor_nodes_[0]->tensor.ByteSize();
}

bool LayerNorm::HalfStorageOk(std::string& why) const {
    if (input_tensor_nodes_.empty() || output_tensor_nodes_.empty()) return true;
    if (IsHalf(input_tensor_nodes_[0]->tensor) == IsHalf(output_tensor_nodes_[0]->tensor)) return true;
    why = "F.layer_norm reads x and writes the output in one storage type";
    return false;
}

}  // namespace SimpleInfer
