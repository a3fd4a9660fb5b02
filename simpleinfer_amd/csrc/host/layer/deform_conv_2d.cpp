#include "deform_conv_2d.h"

#include <algorithm>
#include <cstring>

namespace SimpleInfer {

DEFINE_LAYER_REGISTRY(DeformConv2d);

Status DeformConv2d::Init(const pnnx::Operator* op) {
    CHECK_STATUS(Layer::Init(op));
    return Init(op->params, op->attrs);
}

// the parameters pnnx writes for torchvision.ops.DeformConv2d (a missing key is kFail, as for Conv2d)
Status DeformConv2d::Init(const std::map<std::string, pnnx::Parameter>& params, const std::map<std::string, pnnx::Attribute>& attrs) {
    struct IntPair { const char* key; int* a; int* b; };
    const IntPair pairs[] = {{"kernel_size", &kernel_h_, &kernel_w_},
                             {"stride", &stride_h_, &stride_w_},
                             {"padding", &padding_h_, &padding_w_},
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
    CHECK_BOOL(in_channels_ % groups_ == 0 && out_channels_ % groups_ == 0);

    // weight [Cout][Cin/groups][kh][kw]
    CHECK_BOOL(CheckAttr(attrs, "weight", 1));
    const pnnx::Attribute& w = attrs.at("weight");
    CHECK_BOOL(4 == w.shape.size());
    CHECK_BOOL(w.shape[0] == out_channels_ && w.shape[1] == in_channels_ / groups_ && w.shape[2] == kernel_h_ && w.shape[3] == kernel_w_);
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

Status DeformConv2d::Deinit() {
    weight_dev_.Free();
    bias_dev_.Free();
    device_ready_ = false;
    return Status::kSuccess;
}

Status DeformConv2d::Validate() {
    CHECK_STATUS(Layer::Validate());
    CHECK_STATUS(ValidateShape(-1, 1));
    CHECK_STATUS(ValidateFloatLogged("DeformConv2d"));
    const size_t n_in = input_tensor_nodes_.size();
    if (n_in != 2 && n_in != 3) {
        LOG(ERROR) << "DeformConv2d::Validate fail [" << n_in << " inputs: (x, offset) or (x, offset, mask)]";
        return Status::kErrorShape;
    }
    Dims4 in, off, mask, out;
    if (!GetDims4(input_tensor_nodes_[0]->tensor, in) || !GetDims4(input_tensor_nodes_[1]->tensor, off) ||
        (n_in == 3 && !GetDims4(input_tensor_nodes_[2]->tensor, mask)) || !GetDims4(output_tensor_nodes_[0]->tensor, out)) {
        LOG(ERROR) << "DeformConv2d::Validate fail [inputs and output must be rank-4]";
        return Status::kErrorShape;
    }
    const long long eh = (long long)in.h + 2LL * padding_h_ - (long long)dilation_h_ * (kernel_h_ - 1) - 1;
    const long long ew = (long long)in.w + 2LL * padding_w_ - (long long)dilation_w_ * (kernel_w_ - 1) - 1;
    const long long oh = eh >= 0 ? eh / stride_h_ + 1 : 0, ow = ew >= 0 ? ew / stride_w_ + 1 : 0;
    if (in.c != in_channels_ || out.c != out_channels_ || out.n != in.n || out.h != oh || out.w != ow) {
        LOG(ERROR) << "DeformConv2d::Validate fail [output shape " << out.n << "x" << out.c << "x" << out.h << "x" << out.w << " for input " << in.n
                   << "x" << in.c << "x" << in.h << "x" << in.w << ": expected " << in.n << "x" << out_channels_ << "x" << oh << "x" << ow
                   << ", in_channels " << in_channels_ << "]";
        return Status::kErrorShape;
    }
    const int taps = kernel_h_ * kernel_w_;
    if (off.n != in.n || off.h != oh || off.w != ow || off.c % (2 * taps) != 0) {
        LOG(ERROR) << "DeformConv2d::Validate fail [offset shape " << off.n << "x" << off.c << "x" << off.h << "x" << off.w << ": expected " << in.n
                   << "x(a multiple of " << 2 * taps << ")x" << oh << "x" << ow << "]";
        return Status::kErrorShape;
    }
    const int og = off.c / (2 * taps);
    if (in_channels_ % og != 0) {
        LOG(ERROR) << "DeformConv2d::Validate fail [" << off.c << " offset channels are " << og << " offset groups, which do not divide in_channels "
                   << in_channels_ << "]";
        return Status::kErrorShape;
    }
    if (n_in == 3 && (mask.n != in.n || mask.h != oh || mask.w != ow || mask.c != og * taps)) {
        LOG(ERROR) << "DeformConv2d::Validate fail [mask shape " << mask.n << "x" << mask.c << "x" << mask.h << "x" << mask.w << ": expected " << in.n
                   << "x" << og * taps << "x" << oh << "x" << ow << "]";
        return Status::kErrorShape;
    }
    // anything else the kernel refuses (sizes beyond its 31-bit offsets)
    std::vector<const Tensor*> ins;
    for (auto* n : input_tensor_nodes_) ins.push_back(&n->tensor);
    SiDeformConv2dDesc d;
    const uintptr_t base = (uintptr_t)1 << 40, apart = (uintptr_t)1 << 36;   // aligned addresses far apart: the descriptor alone is asked
    if (!MakeDesc(ins, output_tensor_nodes_[0]->tensor, d) ||
        0 == strcmp("none", si_hip_deform_conv2d_kernel_name(&d, (const void*)base, (const void*)(base + apart), (const void*)(base + 2 * apart),
                                                             (const void*)(base + 3 * apart)))) {
        LOG(ERROR) << "DeformConv2d::Validate fail [the kernel refuses these sizes: element offsets beyond 31 bits]";
        return Status::kUnsupport;
    }
    return Status::kSuccess;
}

bool DeformConv2d::MakeDesc(const std::vector<const Tensor*>& in, const Tensor& output, SiDeformConv2dDesc& d) const {
    memset(&d, 0, sizeof(d));
    if (in.size() != 2 && in.size() != 3) return false;
    Dims4 x, off, mask, out;
    if (!GetDims4(*in[0], x) || !GetDims4(*in[1], off) || !GetDims4(output, out)) return false;
    if (in.size() == 3 && !GetDims4(*in[2], mask)) return false;
    const int taps = kernel_h_ * kernel_w_;
    if (taps <= 0 || off.c % (2 * taps) != 0) return false;
    d.n = x.n; d.ih = x.h; d.iw = x.w; d.ic = x.c; d.in_ld = in[0]->PixelStride();
    d.oh = out.h; d.ow = out.w; d.oc = out.c; d.out_ld = output.PixelStride();
    d.off_ld = in[1]->PixelStride();
    d.mask_ld = in.size() == 3 ? in[2]->PixelStride() : 0;
    d.kh = kernel_h_; d.kw = kernel_w_; d.sh = stride_h_; d.sw = stride_w_; d.ph = padding_h_; d.pw = padding_w_;
    d.dh = dilation_h_; d.dw = dilation_w_;
    d.groups = groups_;
    d.offset_groups = off.c / (2 * taps);
    d.has_mask = in.size() == 3 ? 1 : 0;
    d.has_bias = use_bias_ ? 1 : 0;
    d.act = act_;
    d.act_param = act_param_;
    return true;
}

Status DeformConv2d::PrepareDevice() {
    if (device_ready_) return Status::kSuccess;
    SiDeformConv2dDesc d;
    memset(&d, 0, sizeof(d));
    d.ic = in_channels_; d.oc = out_channels_; d.kh = kernel_h_; d.kw = kernel_w_; d.groups = groups_;
    const size_t elems = si_hip_deform_conv2d_weight_elems(&d);
    if (elems == 0) return Status::kUnsupport;
    std::vector<float> packed(elems);
    CHECK_STATUS(CheckHip(si_hip_deform_conv2d_pack_weight_host(&d, weight_.data(), packed.data()), "pack deformable-conv weight"));
    CHECK_STATUS(CheckHip(weight_dev_.Upload(packed.data(), packed.size() * sizeof(float)), "upload weight"));
    if (use_bias_) CHECK_STATUS(CheckHip(bias_dev_.Upload(bias_.data(), bias_.size() * sizeof(float)), "upload bias"));
    device_ready_ = true;
    return Status::kSuccess;
}

Status DeformConv2d::Forward(const std::vector<Tensor>& inputs, Tensor& output) {
    if (inputs.size() != 2 && inputs.size() != 3) return Status::kUnsupport;
    std::vector<const Tensor*> ins;
    for (const Tensor& t : inputs) ins.push_back(&t);
    return RunOnDevice(ins, {&output}, [this](const std::vector<Tensor>& in, std::vector<Tensor>& out) {
        for (const Tensor& t : in)
            if (IsHalf(t)) return Status::kUnsupport;   // (fp16 engines run this layer between casts)
        if (IsHalf(out[0])) return Status::kUnsupport;
        CHECK_STATUS(PrepareDevice());
        std::vector<const Tensor*> p;
        for (const Tensor& t : in) p.push_back(&t);
        SiDeformConv2dDesc d;
        if (!MakeDesc(p, out[0], d)) return Status::kErrorShape;
        return CheckHip(si_hip_deform_conv2d_f32(&d, in[0].Data<float>(), in[1].Data<float>(), in.size() == 3 ? in[2].Data<float>() : nullptr,
                                                 weight_dev_.As<float>(), use_bias_ ? bias_dev_.As<float>() : nullptr, out[0].Data<float>(), Stream()),
                        "DeformConv2d");
    });
}

const char* DeformConv2d::KernelName() const {
    const char* const fallback = "deform_conv_f32_kernel";
    if (input_tensor_nodes_.size() < 2 || output_tensor_nodes_.empty()) return fallback;
    std::vector<const Tensor*> ins;
    for (auto* n : input_tensor_nodes_) ins.push_back(&n->tensor);
    const Tensor& out = output_tensor_nodes_[0]->tensor;
    SiDeformConv2dDesc d;
    if (!MakeDesc(ins, out, d)) return fallback;
    // (before the arena is bound the tensors have no address yet: the name is then asked for aligned ones)
    if (!ins[0]->RawData() || !ins[1]->RawData() || !out.RawData() || (ins.size() == 3 && !ins[2]->RawData())) {
        const uintptr_t base = (uintptr_t)1 << 40, apart = (uintptr_t)1 << 36;
        return si_hip_deform_conv2d_kernel_name(&d, (const void*)base, (const void*)(base + apart), (const void*)(base + 2 * apart),
                                                (const void*)(base + 3 * apart));
    }
    return si_hip_deform_conv2d_kernel_name(&d, ins[0]->RawData(), ins[1]->RawData(), ins.size() == 3 ? ins[2]->RawData() : nullptr, out.RawData());
}

// 2 N Ho Wo Cout (Cin / groups) kh kw
double DeformConv2d::Flops() const {
    if (output_tensor_nodes_.empty()) return 0.0;
    Dims4 out;
    if (!GetDims4(output_tensor_nodes_[0]->tensor, out)) return 0.0;
    return 2.0 * (double)out.pixels() * out_channels_ * (in_channels_ / std::max(groups_, 1)) * kernel_h_ * kernel_w_;
}

double DeformConv2d::Bytes() const {
    return Layer::Bytes() + (double)(weight_.size() + bias_.size()) * sizeof(float);
}

bool DeformConv2d::HalfStorageOk(std::string& why) const {
    for (auto* n : input_tensor_nodes_)
        if (IsHalf(n->tensor)) { why = "DeformConv2d has an fp32 kernel only"; return false; }
    for (auto* n : output_tensor_nodes_)
        if (IsHalf(n->tensor)) { why = "DeformConv2d has an fp32 kernel only"; return false; }
    return true;
}

}  // namespace SimpleInfer
