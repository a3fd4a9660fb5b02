#include "pixel_shuffle.h"

#include <cstring>

namespace SimpleInfer {

DEFINE_LAYER_REGISTRY(PixelShuffle);

// A missing key is kFail; a factor or a shape the rule does not allow is left for Validate.
Status PixelShuffle::Init(const pnnx::Operator* op) {
    CHECK_STATUS(Layer::Init(op));
    inverse_ = op->type == "nn.PixelUnshuffle" || op->type == "F.pixel_unshuffle";
    const char* key = inverse_ ? "downscale_factor" : "upscale_factor";
    CHECK_BOOL(Get(op, key, factor_));
    return Status::kSuccess;
}

Status PixelShuffle::Validate() {
    CHECK_STATUS(Layer::Validate());
    CHECK_STATUS(ValidateShape(1, 1));
    CHECK_STATUS(ValidateFloatLogged("PixelShuffle"));
    const Tensor& in = input_tensor_nodes_[0]->tensor;
    const Tensor& out = output_tensor_nodes_[0]->tensor;
    Dims4 id, od;
    if (!GetDims4(in, id)) {
        LOG(ERROR) << "PixelShuffle::Validate fail [a rank-" << in.Shape().size() << " input " << ShapeString(in.Shape()) << " (NHWC): rank 4 only]";
        return Status::kUnsupport;
    }
    if (factor_ < 1) {
        LOG(ERROR) << "PixelShuffle::Validate fail [" << (inverse_ ? "downscale_factor " : "upscale_factor ") << factor_ << " is below 1]";
        return Status::kErrorShape;
    }
    const long long r = factor_, rr = r * r;
    bool ok = GetDims4(out, od) && od.n == id.n;
    if (ok && !inverse_) ok = id.c % rr == 0 && od.c == id.c / rr && od.h == id.h * r && od.w == id.w * r;
    if (ok && inverse_) ok = id.h % r == 0 && id.w % r == 0 && od.h == id.h / r && od.w == id.w / r && od.c == id.c * rr;
    if (!ok) {
        LOG(ERROR) << "PixelShuffle::Validate fail [output " << ShapeString(out.Shape()) << " for input " << ShapeString(in.Shape()) << " (NHWC) and "
                   << (inverse_ ? "downscale_factor " : "upscale_factor ") << factor_ << ": the "
                   << (inverse_ ? "height and width must be multiples of the factor and the output [n, h / r, w / r, c r r]"
                                : "channels must be a multiple of r r and the output [n, h r, w r, c / (r r)]")
                   << "]";
        return Status::kErrorShape;
    }
    return Status::kSuccess;
}

bool PixelShuffle::MakeDesc(const Tensor& input, const Tensor& output, SiPixelShuffleDesc& d) const {
    Dims4 id, od;
    if (!GetDims4(input, id) || !GetDims4(output, od) || id.n != od.n) return false;
    memset(&d, 0, sizeof(d));
    d.n = id.n; d.ih = id.h; d.iw = id.w; d.ic = id.c; d.in_ld = input.PixelStride();
    d.oh = od.h; d.ow = od.w; d.oc = od.c; d.out_ld = output.PixelStride();
    d.r = factor_;
    d.inverse = inverse_ ? 1 : 0;
    return true;
}

Status PixelShuffle::Forward(const Tensor& input, Tensor& output) {
    return ForwardDesc(si_hip_pixel_shuffle_f32, si_hip_pixel_shuffle_f16, "PixelShuffle", input, output, [this](auto&... a) { return MakeDesc(a...); });
}

const char* PixelShuffle::KernelName() const {
    return DescKernelName(si_hip_pixel_shuffle_kernel_name, "pixel_shuffle", [this](auto&... a) { return MakeDesc(a...); });
}

}  // namespace SimpleInfer
