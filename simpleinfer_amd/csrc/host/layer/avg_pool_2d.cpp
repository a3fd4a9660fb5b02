#include "avg_pool_2d.h"

#include <cstring>

namespace SimpleInfer {

DEFINE_LAYER_REGISTRY(AvgPool2d);

// A missing key is kFail; what the file asks for and this layer does not do is left for Validate (kUnsupport).
Status AvgPool2d::Init(const pnnx::Operator* op) {
    CHECK_STATUS(Layer::Init(op));
    CHECK_BOOL(Get(op, "ceil_mode", ceil_mode_));
    CHECK_BOOL(Get(op, "count_include_pad", count_include_pad_));

    struct IntPair { const char* key; int* a; int* b; };
    const IntPair pairs[] = {{"kernel_size", &kernel_h_, &kernel_w_}, {"stride", &stride_h_, &stride_w_}, {"padding", &padding_h_, &padding_w_}};
    for (const IntPair& p : pairs) {
        std::vector<int> v;
        CHECK_BOOL(Get(op, p.key, v) && 2 == v.size());
        *p.a = v[0];
        *p.b = v[1];
    }
    // an int, or None (type 0)
    CHECK_BOOL(FindParam(op, "divisor_override") != nullptr);
    has_divisor_override_ = false;
    divisor_override_ = 0;
    if (!IsNone(op, "divisor_override")) {
        CHECK_BOOL(Get(op, "divisor_override", divisor_override_));
        has_divisor_override_ = true;
    }
    return Status::kSuccess;
}

int AvgPool2d::OutSize(int i, int k, int s, int p, bool ceil_mode) {
    const long long span = (long long)i + 2LL * p - k;
    if (span < 0 || s < 1) return 0;
    long long o = (ceil_mode ? (span + s - 1) / s : span / s) + 1;
    if (ceil_mode && (o - 1) * s >= (long long)i + p) --o;
    return (int)o;
}

Status AvgPool2d::Validate() {
    CHECK_STATUS(Layer::Validate());
    CHECK_STATUS(ValidateShape(1, 1));
    CHECK_STATUS(ValidateFloatLogged("AvgPool2d"));
    if (kernel_h_ < 1 || kernel_w_ < 1 || stride_h_ < 1 || stride_w_ < 1 || padding_h_ < 0 || padding_w_ < 0) {
        LOG(ERROR) << "AvgPool2d::Validate fail [kernel_size and stride must be positive, padding non-negative]";
        return Status::kFail;
    }
    if (padding_h_ > kernel_h_ / 2 || padding_w_ > kernel_w_ / 2) {
        LOG(ERROR) << "AvgPool2d::Validate fail [padding (" << padding_h_ << ", " << padding_w_ << ") is more than half of kernel_size (" << kernel_h_
                   << ", " << kernel_w_ << ")]";
        return Status::kUnsupport;
    }
    if (has_divisor_override_ && 0 == divisor_override_) {
        LOG(ERROR) << "AvgPool2d::Validate fail [divisor_override must not be 0]";
        return Status::kUnsupport;
    }
    Dims4 in, out;
    if (!GetDims4(input_tensor_nodes_[0]->tensor, in) || !GetDims4(output_tensor_nodes_[0]->tensor, out)) {
        LOG(ERROR) << "AvgPool2d::Validate fail [input and output must be rank-4]";
        return Status::kErrorShape;
    }
    const int oh = OutSize(in.h, kernel_h_, stride_h_, padding_h_, ceil_mode_), ow = OutSize(in.w, kernel_w_, stride_w_, padding_w_, ceil_mode_);
    if (out.n != in.n || out.c != in.c || out.h != oh || out.w != ow) {
        LOG(ERROR) << "AvgPool2d::Validate fail [output shape " << out.n << "x" << out.c << "x" << out.h << "x" << out.w << " for input " << in.n << "x"
                   << in.c << "x" << in.h << "x" << in.w << ", kernel_size (" << kernel_h_ << ", " << kernel_w_ << "), stride (" << stride_h_ << ", "
                   << stride_w_ << "), padding (" << padding_h_ << ", " << padding_w_ << "), ceil_mode " << (ceil_mode_ ? "True" : "False")
                   << ": expected " << in.n << "x" << in.c << "x" << oh << "x" << ow << "]";
        return Status::kErrorShape;
    }
    return Status::kSuccess;
}

bool AvgPool2d::MakeDesc(const Tensor& input, const Tensor& output, SiAvgPool2dDesc& d) const {
    Dims4 id, od;
    if (!GetDims4(input, id) || !GetDims4(output, od) || id.c != od.c || id.n != od.n) return false;
    memset(&d, 0, sizeof(d));
    d.n = id.n; d.ih = id.h; d.iw = id.w; d.c = id.c; d.in_ld = input.PixelStride();
    d.oh = od.h; d.ow = od.w; d.out_ld = output.PixelStride();
    d.kh = kernel_h_; d.kw = kernel_w_; d.sh = stride_h_; d.sw = stride_w_; d.pt = padding_h_; d.pl = padding_w_;
    d.count_include_pad = count_include_pad_ ? 1 : 0;
    d.divisor_override = has_divisor_override_ ? divisor_override_ : 0;
    return true;
}

Status AvgPool2d::Forward(const Tensor& input, Tensor& output) {
    return RunOnDevice({&input}, {&output}, [this](const std::vector<Tensor>& in, std::vector<Tensor>& out) {
        if (has_divisor_override_ && 0 == divisor_override_) return Status::kUnsupport;
        return LaunchDesc(si_hip_avgpool2d_f32, si_hip_avgpool2d_f16, "AvgPool2d", in[0], out[0], [this](auto&... a) { return MakeDesc(a...); });
    });
}

const char* AvgPool2d::KernelName() const {
    return DescKernelName(si_hip_avgpool2d_kernel_name, "avgpool2d_kernel", [this](auto&... a) { return MakeDesc(a...); }, true);
}

}  // namespace SimpleInfer
