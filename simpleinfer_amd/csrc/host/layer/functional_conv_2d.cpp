#include "functional_conv_2d.h"

#include <algorithm>
#include <cstring>

namespace SimpleInfer {

DEFINE_LAYER_REGISTRY(FunctionalConv2d);

namespace {

// a two-element int tuple, as pnnx writes stride / padding / dilation of the 2-d function
bool GetTwo(const pnnx::Operator* op, const char* key, int& a, int& b) {
    std::vector<int> t;
    if (!Get(op, key, t) || t.size() != 2) return false;
    a = t[0];
    b = t[1];
    return true;
}

// aligned addresses far apart: the descriptor alone is asked
const void* FarAddress(int k) { return (const void*)(((uintptr_t)1 << 40) + ((uintptr_t)k << 36)); }

}  // namespace

Status FunctionalConv2d::Refuse(const std::string& why, Status status) const {
    LOG(ERROR) << "F.conv2d [" << (op_ ? op_->name : std::string("-")) << "] refused [" << why << "]";
    return status;
}

// pnnx: `F.conv2d name 2 1 x w out bias=None stride=(..) padding=(..)|same|valid dilation=(..) groups=G`, or three inputs x w b and no bias=
// key.  A missing key is kFail; what the kernels do not serve is refused by Validate(), with the reason.
Status FunctionalConv2d::Init(const pnnx::Operator* op) {
    CHECK_STATUS(Layer::Init(op));
    CHECK_BOOL(GetTwo(op, "stride", stride_h_, stride_w_));
    CHECK_BOOL(GetTwo(op, "dilation", dilation_h_, dilation_w_));
    CHECK_BOOL(Get(op, "groups", groups_));
    CHECK_BOOL(stride_h_ > 0 && stride_w_ > 0 && dilation_h_ > 0 && dilation_w_ > 0 && groups_ > 0);
    std::string text;
    same_ = false;
    pad_h_ = pad_w_ = 0;
    if (Get(op, "padding", text)) {
        CHECK_BOOL(text == "same" || text == "valid");
        same_ = text == "same";
    } else {
        CHECK_BOOL(GetTwo(op, "padding", pad_h_, pad_w_) && pad_h_ >= 0 && pad_w_ >= 0);
    }
    CHECK_BOOL(op->inputs.size() == 2 || op->inputs.size() == 3);
    if (op->inputs.size() == 2) CHECK_BOOL(IsNoneOrText(op, "bias"));
    has_bias_ = false;
    bias_.clear();
    bias_ready_ = false;
    per_sample_ = false;
    if (op->inputs.size() == 3) {
        // the kernels' bias is fp32 [O] under both storage types: the layer reads the constant's data itself and keeps a copy of its own
        const pnnx::Operand* b = op->inputs[2];
        const pnnx::Operator* src = b ? b->producer : nullptr;
        if (!src || src->type != "pnnx.Attribute") return Refuse("the bias is an activation: only an absent bias and a graph constant are served");
        auto data = src->attrs.find("data");
        if (data == src->attrs.end() || data->second.type != 1 || data->second.shape.size() != 1 ||
            data->second.data.size() != (size_t)data->second.shape[0] * sizeof(float))
            return Refuse("the constant bias is not a rank-1 fp32 tensor");
        bias_.resize(data->second.shape[0]);
        memcpy(bias_.data(), data->second.data.data(), data->second.data.size());
        has_bias_ = true;
    }
    return Status::kSuccess;
}

Status FunctionalConv2d::Deinit() {
    bias_dev_.Free();
    bias_ready_ = false;
    return Status::kSuccess;
}

bool FunctionalConv2d::SetPerSample(TensorNode* x, TensorNode* z, TensorNode* out) {
    if (!x || !z || !out || per_sample_ || input_tensor_nodes_.size() < 2 || output_tensor_nodes_.size() != 1) return false;
    Dims4 dx, dz, dout, ux, uw, uy;
    if (!GetDims4(x->tensor, dx) || !GetDims4(z->tensor, dz) || !GetDims4(out->tensor, dout)) return false;
    if (!GetDims4(input_tensor_nodes_[0]->tensor, ux) || !GetDims4(input_tensor_nodes_[1]->tensor, uw) || !GetDims4(output_tensor_nodes_[0]->tensor, uy)) return false;
    // the unfused operands: x [1, H, W, N C], w [N C, kh, kw, 1], y [1, Ho, Wo, N C]
    const int nc = dx.n * dx.c;
    if (ux.n != 1 || ux.c != nc || ux.h != dx.h || ux.w != dx.w || groups_ != nc) return false;
    if (uw.n != nc || uw.c != 1 || uw.h != dz.h || uw.w != dz.w || dz.n != dx.n || dz.c != dx.c) return false;
    if (uy.n != 1 || uy.c != nc || dout.n != dx.n || dout.c != dx.c || dout.h != uy.h || dout.w != uy.w) return false;
    if (has_bias_ && dx.n != 1) return false;   // (a bias [N C] holds one value per image and channel: the per-sample launch has one per channel)
    std::vector<TensorNode*> ins = input_tensor_nodes_;
    ins[0] = x;
    ins[1] = z;
    per_sample_ = true;
    SetInputNodes(ins);
    SetOutputNodes({out});
    return true;
}

Status FunctionalConv2d::Validate() {
    CHECK_STATUS(Layer::Validate());
    CHECK_STATUS(ValidateShape(has_bias_ ? 3 : 2, 1));
    CHECK_STATUS(ValidateFloatLogged("FunctionalConv2d"));
    if (same_ && (stride_h_ != 1 || stride_w_ != 1)) return Refuse("padding='same' with a stride above 1 (torch refuses it too)");
    const Tensor& x = input_tensor_nodes_[0]->tensor;
    const Tensor& w = input_tensor_nodes_[1]->tensor;
    const Tensor& out = output_tensor_nodes_[0]->tensor;
    Dims4 dx, dw, dout;
    if (x.Shape().size() != 4) return Refuse("x of rank " + std::to_string(x.Shape().size()) + ": only a batched [N, C, H, W] input is served");
    if (w.Shape().size() != 4 || out.Shape().size() != 4) return Refuse("the filter and the output must be rank-4 tensors");
    if (!GetDims4(x, dx) || !GetDims4(w, dw) || !GetDims4(out, dout)) return Refuse("an operand with an empty dimension", Status::kErrorShape);
    if (per_sample_) {
        if (dw.n != dx.n || dw.c != dx.c || dout.n != dx.n || dout.c != dx.c) return Refuse("per-sample operands that disagree", Status::kErrorShape);
    } else {
        if (groups_ != 1 && !(groups_ == dx.c && groups_ == dw.n && dw.c == 1))
            return Refuse("groups=" + std::to_string(groups_) + " with " + std::to_string(dx.c) + " input channels and " + std::to_string(dw.n) +
                          " filters: a tensor filter is served dense (groups == 1) or depthwise (groups == C == O)");
        if ((long long)dw.c * groups_ != dx.c)
            return Refuse("x has " + std::to_string(dx.c) + " channels, the filter " + std::to_string(dw.c) + " x " + std::to_string(groups_) + " groups",
                          Status::kErrorShape);
        if (dout.n != dx.n || dout.c != dw.n) return Refuse("the output must be [N, O, Ho, Wo]", Status::kErrorShape);
    }
    if (has_bias_ && (int)bias_.size() != dout.c)
        return Refuse("the bias holds " + std::to_string(bias_.size()) + " values for " + std::to_string(dout.c) + " output channels", Status::kErrorShape);
    SiXcorrDesc d;
    if (!MakeDesc(x, w, out, d)) return Refuse("operands the descriptor cannot be made of", Status::kErrorShape);
    // the output extent is torch's
    const long long th = same_ ? (long long)dilation_h_ * (d.kh - 1) : 2LL * pad_h_, tw = same_ ? (long long)dilation_w_ * (d.kw - 1) : 2LL * pad_w_;
    const long long eh = d.h + th - (long long)dilation_h_ * (d.kh - 1) - 1, ew = d.w + tw - (long long)dilation_w_ * (d.kw - 1) - 1;
    const long long ho = eh >= 0 ? eh / stride_h_ + 1 : 0, wo = ew >= 0 ? ew / stride_w_ + 1 : 0;
    if (ho <= 0 || wo <= 0 || d.ho != ho || d.wo != wo)
        return Refuse("output " + ShapeString(out.Shape()) + " (NHWC) for input " + ShapeString(x.Shape()) + " and filter " + ShapeString(w.Shape()) +
                          ": torch's formula gives " + std::to_string(ho) + " x " + std::to_string(wo),
                      Status::kErrorShape);
    // anything else the kernel refuses (sizes beyond its 31-bit offsets or its grid)
    if (0 == strcmp("none", si_hip_xcorr_kernel_name(&d, FarAddress(0), FarAddress(1), FarAddress(2), 0)))
        return Refuse("the kernel refuses these sizes: element offsets beyond 31 bits or a grid extent beyond its limit");
    return Status::kSuccess;
}

// rank-4 tensors are NHWC with the pixels PixelStride() elements apart.  The filter as stored is [O][kh][kw][C / groups]
bool FunctionalConv2d::MakeDesc(const Tensor& x, const Tensor& w, const Tensor& out, SiXcorrDesc& d) const {
    memset(&d, 0, sizeof(d));
    Dims4 dx, dw, dout;
    if (!GetDims4(x, dx) || !GetDims4(w, dw) || !GetDims4(out, dout)) return false;
    d.n = dx.n; d.h = dx.h; d.w = dx.w; d.c = dx.c; d.oc = dout.c; d.ho = dout.h; d.wo = dout.w; d.kh = dw.h; d.kw = dw.w;
    d.stride_h = stride_h_; d.stride_w = stride_w_; d.dilation_h = dilation_h_; d.dilation_w = dilation_w_;
    d.pad_top = same_ ? (int)(((long long)dilation_h_ * (d.kh - 1)) / 2) : pad_h_;
    d.pad_left = same_ ? (int)(((long long)dilation_w_ * (d.kw - 1)) / 2) : pad_w_;
    d.x_sp = x.PixelStride(); d.x_sh = (long long)d.w * d.x_sp; d.x_sn = (long long)d.h * d.x_sh;
    d.y_sp = out.PixelStride(); d.y_sh = (long long)d.wo * d.y_sp; d.y_sn = (long long)d.ho * d.y_sh;
    const long long ld = w.PixelStride();
    d.w_sp = ld; d.w_sh = (long long)d.kw * ld;
    if (per_sample_) {
        // w [N][kh][kw][C]: filter n meets image n
        d.groups = d.c;
        d.per_sample = 1;
        d.w_sn = (long long)d.kh * d.w_sh; d.w_sc = 1;
    } else if (groups_ == 1 && !(d.c == 1 && d.oc == 1)) {
        d.groups = 1;
        d.w_sn = (long long)d.kh * d.w_sh; d.w_sc = 1;
    } else {
        // w [C][kh][kw][1]: the filter of channel c is "image" c of the stored tensor
        d.groups = groups_;
        d.w_sn = 0; d.w_sc = (long long)d.kh * d.w_sh;
    }
    d.act = act_;
    d.act_param = act_param_;
    return true;
}

Status FunctionalConv2d::Forward(const std::vector<Tensor>& inputs, Tensor& output) {
    if (inputs.size() < 2) return Status::kUnsupport;
    return RunOnDevice({&inputs[0], &inputs[1]}, {&output}, [this](const std::vector<Tensor>& in, std::vector<Tensor>& out) {
        const bool half = IsHalf(in[0]);
        if (IsHalf(out[0]) != half || IsHalf(in[1]) != half) return Status::kUnsupport;
        SiXcorrDesc d;
        if (!MakeDesc(in[0], in[1], out[0], d)) return Status::kErrorShape;
        if (has_bias_ && !bias_ready_) {
            CHECK_STATUS(CheckHip(bias_dev_.Upload(bias_.data(), bias_.size() * sizeof(float)), "upload bias"));
            bias_ready_ = true;
        }
        const float* const bias = has_bias_ ? bias_dev_.As<float>() : nullptr;
        const int rc = half ? si_hip_xcorr_f16(&d, in[0].RawData(), in[1].RawData(), bias, out[0].RawData(), Stream())
                            : si_hip_xcorr_f32(&d, in[0].Data<float>(), in[1].Data<float>(), bias, out[0].Data<float>(), Stream());
        return CheckHip(rc, "FunctionalConv2d");
    });
}

const char* FunctionalConv2d::KernelName() const {
    const char* const fallback = "xcorr";
    if (input_tensor_nodes_.size() < 2 || output_tensor_nodes_.size() != 1) return fallback;
    const Tensor& x = input_tensor_nodes_[0]->tensor;
    const Tensor& w = input_tensor_nodes_[1]->tensor;
    const Tensor& out = output_tensor_nodes_[0]->tensor;
    SiXcorrDesc d;
    if (!MakeDesc(x, w, out, d)) return fallback;
    // (before the arena is bound the tensors have no address yet: the name is then asked for aligned ones)
    const bool bound = x.RawData() && w.RawData() && out.RawData();
    return si_hip_xcorr_kernel_name(&d, bound ? x.RawData() : FarAddress(0), bound ? w.RawData() : FarAddress(1), bound ? out.RawData() : FarAddress(2),
                                    IsHalf(x) ? 1 : 0);
}

// 2 N Ho Wo O (C / groups) kh kw
double FunctionalConv2d::Flops() const {
    if (input_tensor_nodes_.size() < 2 || output_tensor_nodes_.empty()) return 0.0;
    Dims4 dw;
    if (!GetDims4(input_tensor_nodes_[1]->tensor, dw)) return 0.0;
    const double per_output = (double)dw.h * dw.w * (per_sample_ ? 1 : dw.c);
    return 2.0 * (double)output_tensor_nodes_[0]->tensor.NumElements() * per_output;
}

// x, w and y share one storage type; the dense fp16 kernel needs C % 8 == 0.  A layer that breaks either rule runs in fp32 between casts
bool FunctionalConv2d::HalfStorageOk(std::string& why) const {
    if (input_tensor_nodes_.size() < 2 || output_tensor_nodes_.empty()) return true;
    const int half = IsHalf(input_tensor_nodes_[0]->tensor) + IsHalf(input_tensor_nodes_[1]->tensor) + IsHalf(output_tensor_nodes_[0]->tensor);
    if (half == 0) return true;
    if (half != 3) {
        why = "F.conv2d reads x and the filter and writes the output in one storage type";
        return false;
    }
    Dims4 dx, dw;
    // (one channel and one filter is the depthwise kernel's: no such rule there)
    if (!per_sample_ && groups_ == 1 && GetDims4(input_tensor_nodes_[0]->tensor, dx) && GetDims4(input_tensor_nodes_[1]->tensor, dw) && dx.c % 8 != 0 &&
        !(dx.c == 1 && dw.n == 1)) {
        why = "the dense fp16 kernel of F.conv2d needs in_channels % 8 == 0";
        return false;
    }
    return true;
}

}  // namespace SimpleInfer
