#include "conv_transpose_2d.h"

#include <algorithm>
#include <cstring>

namespace SimpleInfer {

DEFINE_LAYER_REGISTRY(ConvTranspose2d);

Status ConvTranspose2d::Init(const pnnx::Operator* op) {
    CHECK_STATUS(Layer::Init(op));
    return Init(op->params, op->attrs);
}

// the parameters pnnx writes for torch.nn.ConvTranspose2d (a missing key is kFail, as for Conv2d)
Status ConvTranspose2d::Init(const std::map<std::string, pnnx::Parameter>& params,
                             const std::map<std::string, pnnx::Attribute>& attrs) {
    if (params.count("padding_mode")) {
        CHECK_BOOL(CheckParam(params, "padding_mode", 4));
        if (params.at("padding_mode").s != "zeros") {
            LOG(ERROR) << "ConvTranspose2d::Init fail [unsupport padding mode " << params.at("padding_mode").s << ", torch allows zeros only]";
            return Status::kUnsupport;
        }
    }
    struct IntPair { const char* key; int* a; int* b; };
    const IntPair pairs[] = {{"kernel_size", &kernel_h_, &kernel_w_},
                             {"stride", &stride_h_, &stride_w_},
                             {"padding", &padding_h_, &padding_w_},
                             {"output_padding", &output_padding_h_, &output_padding_w_},
                             {"dilation", &dilation_h_, &dilation_w_}};
    for (const IntPair& p : pairs) {
        CHECK_BOOL(CheckParam(params, p.key, 5));
        const std::vector<int>& v = params.at(p.key).ai;
        CHECK_BOOL(2 == v.size());
        *p.a = v[0];
        *p.b = v[1];
    }
    CHECK_BOOL(CheckParam(params, "groups", 2));
    groups_ = params.at("groups").i;
    CHECK_BOOL(CheckParam(params, "in_channels", 2));
    in_channels_ = params.at("in_channels").i;
    CHECK_BOOL(CheckParam(params, "out_channels", 2));
    out_channels_ = params.at("out_channels").i;
    CHECK_BOOL(groups_ > 0 && in_channels_ > 0 && out_channels_ > 0 && kernel_h_ > 0 && kernel_w_ > 0);
    CHECK_BOOL(stride_h_ > 0 && stride_w_ > 0 && dilation_h_ > 0 && dilation_w_ > 0 && padding_h_ >= 0 && padding_w_ >= 0);
    CHECK_BOOL(output_padding_h_ >= 0 && output_padding_w_ >= 0 && out_channels_ % groups_ == 0);

    // weight [Cin][Cout/groups][kh][kw]
    CHECK_BOOL(CheckAttr(attrs, "weight", 1));
    const pnnx::Attribute& w = attrs.at("weight");
    CHECK_BOOL(4 == w.shape.size());
    CHECK_BOOL(w.shape[0] == in_channels_ && w.shape[1] == out_channels_ / groups_ && w.shape[2] == kernel_h_ && w.shape[3] == kernel_w_);
    const size_t w_count = (size_t)w.shape[0] * w.shape[1] * w.shape[2] * w.shape[3];
    CHECK_BOOL(w.data.size() == w_count * sizeof(float));
    weight_.resize(w_count);
    memcpy(weight_.data(), w.data.data(), w.data.size());

    CHECK_BOOL(CheckParam(params, "bias", 1));
    use_bias_ = params.at("bias").b;
    bias_.clear();
    if (use_bias_) {
        CHECK_BOOL(CheckAttr(attrs, "bias", 1));
        const pnnx::Attribute& b = attrs.at("bias");
        CHECK_BOOL(1 == b.shape.size() && b.shape[0] == out_channels_);
        CHECK_BOOL(b.data.size() == (size_t)out_channels_ * sizeof(float));
        bias_.resize(out_channels_);
        memcpy(bias_.data(), b.data.data(), b.data.size());
    }
    device_ready_ = false;
    return Status::kSuccess;
}

Status ConvTranspose2d::Deinit() {
    weight_dev_.Free();
    bias_dev_.Free();
    device_ready_ = false;
    return Status::kSuccess;
}

Status ConvTranspose2d::Validate() {
    CHECK_STATUS(Layer::Validate());
    CHECK_STATUS(ValidateShape(1, 1));
    CHECK_STATUS(ValidateFloatLogged("ConvTranspose2d"));
    if (groups_ != 1) {
        LOG(ERROR) << "ConvTranspose2d::Validate fail [groups " << groups_ << ": grouped / depthwise transposed convolution is not supported]";
        return Status::kUnsupport;
    }
    if (output_padding_h_ >= std::max(stride_h_, dilation_h_) || output_padding_w_ >= std::max(stride_w_, dilation_w_)) {
        LOG(ERROR) << "ConvTranspose2d::Validate fail [output_padding (" << output_padding_h_ << ", " << output_padding_w_
                   << ") must be smaller than either stride or dilation]";
        return Status::kUnsupport;
    }
    Dims4 in, out;
    if (!GetDims4(input_tensor_nodes_[0]->tensor, in) || !GetDims4(output_tensor_nodes_[0]->tensor, out)) {
        LOG(ERROR) << "ConvTranspose2d::Validate fail [input and output must be rank-4]";
        return Status::kErrorShape;
    }
    const long long oh = (long long)(in.h - 1) * stride_h_ - 2LL * padding_h_ + (long long)dilation_h_ * (kernel_h_ - 1) + output_padding_h_ + 1;
    const long long ow = (long long)(in.w - 1) * stride_w_ - 2LL * padding_w_ + (long long)dilation_w_ * (kernel_w_ - 1) + output_padding_w_ + 1;
    if (in.c != in_channels_ || out.c != out_channels_ || out.n != in.n || out.h != oh || out.w != ow) {
        LOG(ERROR) << "ConvTranspose2d::Validate fail [output shape " << out.n << "x" << out.c << "x" << out.h << "x" << out.w << " for input "
                   << in.n << "x" << in.c << "x" << in.h << "x" << in.w << ": expected " << in.n << "x" << out_channels_ << "x" << oh << "x" << ow
                   << ", in_channels " << in_channels_ << "]";
        return Status::kErrorShape;
    }
    return Status::kSuccess;
}

SiConvTranspose2dDesc ConvTranspose2d::MakeDesc(const Tensor& input, const Tensor& output) const {
    SiConvTranspose2dDesc d;
    memset(&d, 0, sizeof(d));
    Dims4 in, out;
    GetDims4(input, in);
    GetDims4(output, out);
    d.n = in.n; d.ih = in.h; d.iw = in.w; d.ic = in.c; d.in_ld = input.PixelStride();
    d.oh = out.h; d.ow = out.w; d.oc = out.c; d.out_ld = output.PixelStride();
    d.kh = kernel_h_; d.kw = kernel_w_; d.sh = stride_h_; d.sw = stride_w_; d.ph = padding_h_; d.pw = padding_w_;
    d.oph = output_padding_h_; d.opw = output_padding_w_; d.dh = dilation_h_; d.dw = dilation_w_;
    d.groups = groups_;
    d.has_bias = use_bias_ ? 1 : 0;
    d.act = act_;
    d.act_param = act_param_;
    return d;
}

Status ConvTranspose2d::PrepareDevice() {
    if (device_ready_) return Status::kSuccess;
    SiConvTranspose2dDesc d;
    memset(&d, 0, sizeof(d));
    d.ic = in_channels_; d.oc = out_channels_; d.kh = kernel_h_; d.kw = kernel_w_; d.groups = groups_;
    const size_t elems = si_hip_conv_transpose2d_weight_elems(&d);
    if (elems == 0) return Status::kUnsupport;
    std::vector<float> packed(elems);
    CHECK_STATUS(CheckHip(si_hip_conv_transpose2d_pack_weight_host(&d, weight_.data(), packed.data()), "pack transposed-conv weight"));
    CHECK_STATUS(CheckHip(weight_dev_.Upload(packed.data(), packed.size() * sizeof(float)), "upload weight"));
    if (use_bias_) CHECK_STATUS(CheckHip(bias_dev_.Upload(bias_.data(), bias_.size() * sizeof(float)), "upload bias"));
    device_ready_ = true;
    return Status::kSuccess;
}

Status ConvTranspose2d::Forward(const Tensor& input, Tensor& output) {
    return RunOnDevice({&input}, {&output}, [this](const std::vector<Tensor>& in, std::vector<Tensor>& out) {
        if (IsHalf(in[0]) || IsHalf(out[0])) return Status::kUnsupport;   // (fp16 engines run this layer between casts)
        CHECK_STATUS(PrepareDevice());
        const SiConvTranspose2dDesc d = MakeDesc(in[0], out[0]);
        return CheckHip(si_hip_conv_transpose2d_f32(&d, in[0].Data<float>(), weight_dev_.As<float>(), use_bias_ ? bias_dev_.As<float>() : nullptr,
                                                    out[0].Data<float>(), Stream()),
                        "ConvTranspose2d");
    });
}

const char* ConvTranspose2d::KernelName() const {
    if (input_tensor_nodes_.empty() || output_tensor_nodes_.empty()) return "conv_transpose_f32_kernel";
    const Tensor& in = input_tensor_nodes_[0]->tensor;
    const Tensor& out = output_tensor_nodes_[0]->tensor;
    if (in.Shape().size() != 4 || out.Shape().size() != 4) return "conv_transpose_f32_kernel";
    const SiConvTranspose2dDesc d = MakeDesc(in, out);
    return si_hip_conv_transpose2d_kernel_name(&d);
}

// 2 N H W Cin Cout kh kw: every input pixel meets every tap once
double ConvTranspose2d::Flops() const {
    if (input_tensor_nodes_.empty()) return 0.0;
    Dims4 in;
    if (!GetDims4(input_tensor_nodes_[0]->tensor, in)) return 0.0;
    return 2.0 * (double)in.pixels() * in_channels_ * (out_channels_ / std::max(groups_, 1)) * kernel_h_ * kernel_w_;
}

double ConvTranspose2d::Bytes() const {
    return Layer::Bytes() + (double)(weight_.size() + bias_.size()) * sizeof(float);
}

bool ConvTranspose2d::HalfStorageOk(std::string& why) const {
    for (auto* n : input_tensor_nodes_)
        if (IsHalf(n->tensor)) { why = "ConvTranspose2d has an fp32 kernel only"; return false; }
    for (auto* n : output_tensor_nodes_)
        if (IsHalf(n->tensor)) { why = "ConvTranspose2d has an fp32 kernel only"; return false; }
    return true;
}

}  // namespace SimpleInfer
