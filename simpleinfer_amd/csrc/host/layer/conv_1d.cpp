#include "conv_1d.h"

#include <algorithm>
#include <cstring>

namespace SimpleInfer {

DEFINE_LAYER_REGISTRY(Conv1d);

namespace {

// a one-element int tuple, as pnnx writes kernel_size / stride / dilation of a 1-d module
bool GetOne(const pnnx::Operator* op, const char* key, int& v) {
    std::vector<int> t;
    if (!Get(op, key, t) || t.size() != 1) return false;
    v = t[0];
    return true;
}

}  // namespace

// pnnx: in_channels, out_channels, kernel_size, stride, padding (an int tuple, `same` or `valid`), dilation, groups, bias, padding_mode;
// weight [Cout][Cin / groups][K], bias [Cout].  A missing key is kFail; what the kernels do not serve is refused by Validate().
Status Conv1d::Init(const pnnx::Operator* op) {
    CHECK_STATUS(Layer::Init(op));
    CHECK_BOOL(Get(op, "in_channels", in_channels_));
    CHECK_BOOL(Get(op, "out_channels", out_channels_));
    CHECK_BOOL(GetOne(op, "kernel_size", kernel_));
    CHECK_BOOL(GetOne(op, "stride", stride_));
    CHECK_BOOL(GetOne(op, "dilation", dilation_));
    CHECK_BOOL(Get(op, "groups", groups_));
    CHECK_BOOL(Get(op, "bias", use_bias_));
    CHECK_BOOL(Get(op, "padding_mode", padding_mode_));
    CHECK_BOOL(in_channels_ > 0 && out_channels_ > 0 && kernel_ > 0 && stride_ > 0 && dilation_ > 0 && groups_ > 0);
    CHECK_BOOL(in_channels_ % groups_ == 0 && out_channels_ % groups_ == 0);
    std::string text;
    same_ = false;
    pad_left_ = pad_right_ = 0;
    if (Get(op, "padding", text)) {
        CHECK_BOOL(text == "same" || text == "valid");
        if (text == "same") {
            same_ = true;
            const long long total = (long long)dilation_ * (kernel_ - 1);
            CHECK_BOOL(total <= 0x7fffffffLL);
            pad_left_ = (int)(total / 2);
            pad_right_ = (int)(total - total / 2);
        }
    } else {
        int p = 0;
        CHECK_BOOL(GetOne(op, "padding", p) && p >= 0);
        pad_left_ = pad_right_ = p;
    }

    CHECK_BOOL(CheckAttr(op, "weight", 1));
    const pnnx::Attribute& w = op->attrs.at("weight");
    CHECK_BOOL(3 == w.shape.size());
    CHECK_BOOL(w.shape[0] == out_channels_ && w.shape[1] == in_channels_ / groups_ && w.shape[2] == kernel_);
    const size_t w_count = (size_t)w.shape[0] * w.shape[1] * w.shape[2];
    CHECK_BOOL(w.data.size() == w_count * sizeof(float));
    weight_.resize(w_count);
    memcpy(weight_.data(), w.data.data(), w.data.size());
    bias_.clear();
    if (use_bias_) CHECK_BOOL(ReadVec(op, "bias", bias_) && bias_.size() == (size_t)out_channels_);
    device_ready_ = false;
    return Status::kSuccess;
}

Status Conv1d::Deinit() {
    weight_dev_.Free();
    bias_dev_.Free();
    device_ready_ = false;
    return Status::kSuccess;
}

Status Conv1d::Validate() {
    CHECK_STATUS(Layer::Validate());
    CHECK_STATUS(ValidateShape(1, 1));
    CHECK_STATUS(ValidateFloatLogged("Conv1d"));
    auto refuse = [&](const char* why) {
        LOG(ERROR) << "Conv1d::Validate fail [" << why << "]";
        return Status::kUnsupport;
    };
    if (padding_mode_ != "zeros") return refuse("padding_mode other than zeros is not served");
    if (same_ && stride_ != 1) return refuse("padding='same' with a stride above 1 (torch refuses it too)");
    const std::vector<int>& in = input_tensor_nodes_[0]->tensor.Shape();
    const std::vector<int>& out = output_tensor_nodes_[0]->tensor.Shape();
    if (in.size() == 2) return refuse("an unbatched rank-2 input [C, L] is not served");
    const long long e = in.size() == 3 ? (long long)in[2] + pad_left_ + pad_right_ - (long long)dilation_ * (kernel_ - 1) - 1 : -1;
    const long long lo = e >= 0 ? e / stride_ + 1 : 0;
    if (in.size() != 3 || out.size() != 3 || in[1] != in_channels_ || out[0] != in[0] || out[1] != out_channels_ || out[2] != lo || lo <= 0) {
        LOG(ERROR) << "Conv1d::Validate fail [output shape " << ShapeString(out) << " for input " << ShapeString(in) << ": expected [N, "
                   << out_channels_ << ", " << lo << "] from [N, " << in_channels_ << ", L]]";
        return Status::kErrorShape;
    }
    // anything else the kernel refuses (sizes beyond its 31-bit offsets, its grid or its LDS): asked for aligned addresses far apart
    SiConv1dDesc d;
    const uintptr_t base = (uintptr_t)1 << 40;
    if (!MakeDesc(input_tensor_nodes_[0]->tensor, output_tensor_nodes_[0]->tensor, d) ||
        0 == strcmp("none", si_hip_conv1d_kernel_name(&d, (const void*)base, (const void*)(base << 1), 0)))
        return refuse("the kernel refuses these sizes: element offsets beyond 31 bits, a grid extent or a tile span beyond its limit");
    return Status::kSuccess;
}

// rows of a rank-3 tensor are PixelStride() elements apart (dense: L), batch items C rows
bool Conv1d::MakeDesc(const Tensor& in, const Tensor& out, SiConv1dDesc& d) const {
    memset(&d, 0, sizeof(d));
    const std::vector<int>& x = in.Shape();
    const std::vector<int>& y = out.Shape();
    if (x.size() != 3 || y.size() != 3 || x[0] != y[0] || x[1] != in_channels_ || y[1] != out_channels_) return false;
    d.n = x[0]; d.c = x[1]; d.l = x[2]; d.oc = y[1]; d.lo = y[2];
    d.k = kernel_; d.stride = stride_; d.dilation = dilation_; d.pad_left = pad_left_; d.groups = groups_;
    d.x_sc = in.PixelStride(); d.x_sn = (long long)d.c * d.x_sc;
    d.y_sc = out.PixelStride(); d.y_sn = (long long)d.oc * d.y_sc;
    d.act = act_;
    d.act_param = act_param_;
    return true;
}

bool Conv1d::HalfKernel() const {
    const bool depthwise = groups_ == in_channels_ && groups_ == out_channels_;
    return depthwise || (in_channels_ / std::max(groups_, 1)) % 8 == 0;
}

// the image of the storage type in use, packed and uploaded once (again when the type changes)
Status Conv1d::PrepareDevice(bool half) {
    if (device_ready_ && half == prepared_half_) return Status::kSuccess;
    device_ready_ = false;
    SiConv1dDesc d;
    memset(&d, 0, sizeof(d));
    d.c = in_channels_; d.oc = out_channels_; d.k = kernel_; d.groups = groups_;
    const size_t bytes = si_hip_conv1d_weight_bytes(&d, half ? 1 : 0);
    if (bytes == 0) {
        LOG(ERROR) << "Conv1d: no " << (half ? "fp16" : "fp32") << " kernel for " << in_channels_ << " -> " << out_channels_ << " channels in " << groups_ << " groups";
        return Status::kUnsupport;
    }
    std::vector<char> img(bytes);
    const int rc = half ? si_hip_conv1d_pack_weights_f16(&d, weight_.data(), img.data())
                        : si_hip_conv1d_pack_weights_f32(&d, weight_.data(), reinterpret_cast<float*>(img.data()));
    CHECK_STATUS(CheckHip(rc, "pack Conv1d weights"));
    CHECK_STATUS(CheckHip(weight_dev_.Upload(img.data(), img.size()), "upload weight"));
    if (use_bias_) CHECK_STATUS(CheckHip(bias_dev_.Upload(bias_.data(), bias_.size() * sizeof(float)), "upload bias"));
    prepared_half_ = half;
    device_ready_ = true;
    return Status::kSuccess;
}

// (the entries take the weight image and the bias between x and y, so the launch is written out instead of going through LaunchDesc)
Status Conv1d::Forward(const Tensor& input, Tensor& output) {
    return RunOnDevice({&input}, {&output}, [this](const std::vector<Tensor>& in, std::vector<Tensor>& out) {
        const bool half = IsHalf(in[0]);
        if (IsHalf(out[0]) != half) return Status::kUnsupport;
        SiConv1dDesc d;
        if (!MakeDesc(in[0], out[0], d)) return Status::kErrorShape;
        CHECK_STATUS(PrepareDevice(half));
        const float* const bias = use_bias_ ? bias_dev_.As<float>() : nullptr;
        const int rc = half ? si_hip_conv1d_f16(&d, in[0].RawData(), weight_dev_.As<void>(), bias, out[0].RawData(), Stream())
                            : si_hip_conv1d_f32(&d, in[0].Data<float>(), weight_dev_.As<float>(), bias, out[0].Data<float>(), Stream());
        return CheckHip(rc, "Conv1d");
    });
}

const char* Conv1d::KernelName() const {
    return DescKernelName<SiConv1dDesc>(
        +[](const SiConv1dDesc* d, const void* x, const void* y, int half) {
            // (before the arena is bound the tensors have no address yet: the name is then asked for aligned ones)
            const uintptr_t base = (uintptr_t)1 << 40;
            return si_hip_conv1d_kernel_name(d, x ? x : (const void*)base, y ? y : (const void*)(base << 1), half);
        },
        "conv1d", [this](const Tensor& in, const Tensor& out, SiConv1dDesc& d) { return MakeDesc(in, out, d); });
}

// 2 N Lo Cout (Cin / groups) K
double Conv1d::Flops() const {
    if (output_tensor_nodes_.empty()) return 0.0;
    return 2.0 * (double)output_tensor_nodes_[0]->tensor.NumElements() * (in_channels_ / std::max(groups_, 1)) * kernel_;
}

double Conv1d::Bytes() const { return Layer::Bytes() + (double)(weight_.size() + bias_.size()) * sizeof(float); }

// The dense fp16 kernel needs (C / groups) % 8 == 0: a layer that breaks the rule runs in fp32 between casts
bool Conv1d::HalfStorageOk(std::string& why) const {
    if (!Layer::HalfStorageOk(why)) return false;
    bool half = false;
    for (auto* n : input_tensor_nodes_) half = half || IsHalf(n->tensor);
    if (half && !HalfKernel()) {
        why = "the fp16 kernel of nn.Conv1d needs (in_channels / groups) % 8 == 0 or a plain depthwise filter";
        return false;
    }
    // (the fp16 LDS image holds fewer positions than the fp32 one: a span the fp16 kernel refuses runs in fp32 too)
    SiConv1dDesc d;
    const uintptr_t base = (uintptr_t)1 << 40;
    if (half && !output_tensor_nodes_.empty() && MakeDesc(input_tensor_nodes_[0]->tensor, output_tensor_nodes_[0]->tensor, d) &&
        0 == strcmp("none", si_hip_conv1d_kernel_name(&d, (const void*)base, (const void*)(base << 1), 1))) {
        why = "the fp16 kernel of nn.Conv1d refuses these sizes (a tile's span beyond its LDS image)";
        return false;
    }
    return true;
}

}  // namespace SimpleInfer
