#include "upsample.h"

#include <cstdio>
#include <cstdlib>

#include "layer_util.h"
#include "si_hip.h"

namespace SimpleInfer {

DEFINE_LAYER_REGISTRY(Upsample);

namespace {

// The file holds scale_factor as text, the loader as float; torch computed with the double of that text.  The shortest decimal
// that reads back as the same float is that text for every value a model author writes (2, 1.5, 3.7), so its double is torch's.
double AsWritten(float f) {
    char buf[32];
    for (int p = 1; p <= 9; ++p) {
        snprintf(buf, sizeof(buf), "%.*g", p, (double)f);
        if ((float)strtod(buf, nullptr) == f) return strtod(buf, nullptr);
    }
    return (double)f;
}

}  // namespace

Status Upsample::Init(const pnnx::Operator* op) {
    CHECK_STATUS(Layer::Init(op));
    std::string mode;
    CHECK_BOOL(Get(op, "mode", mode));
    if ("nearest" == mode) {
        upsample_mode_ = UpsampleMode::kNearest;
    } else if ("bilinear" == mode) {
        upsample_mode_ = UpsampleMode::kBilinear;
    } else {
        LOG(ERROR) << "Upsample::Init fail [unsupport upsample mode " << mode << "]";
        return Status::kUnsupport;
    }
    // (IsNone is the narrow rule, here and below: "None" as text is a value, which the typed read refuses)
    if (!IsNone(op, "align_corners")) CHECK_BOOL(Get(op, "align_corners", align_corners_));
    if (align_corners_ && UpsampleMode::kNearest == upsample_mode_) {
        LOG(ERROR) << "Upsample::Init fail [align_corners=True is not defined for mode nearest]";
        return Status::kUnsupport;
    }
    if (!IsNone(op, "scale_factor")) {
        const pnnx::Parameter& p = *FindParam(op, "scale_factor");
        std::vector<float> v;
        if (6 == p.type) v = p.af;
        else if (5 == p.type) v.assign(p.ai.begin(), p.ai.end());
        else if (3 == p.type) v = {p.f, p.f};
        else if (2 == p.type) v = {(float)p.i, (float)p.i};
        if (2 != v.size()) {
            LOG(ERROR) << "Upsample::Init fail [" << op->type << " with " << v.size() << " scale factors: rank-4 tensors only]";
            return Status::kUnsupport;
        }
        scale_factor_h_ = v[0];
        scale_factor_w_ = v[1];
        scale_h_ = AsWritten(v[0]);
        scale_w_ = AsWritten(v[1]);
        if (!(scale_h_ > 0.0) || !(scale_w_ > 0.0)) {
            LOG(ERROR) << "Upsample::Init fail [scale_factor must be positive]";
            return Status::kFail;
        }
        has_scale_ = true;
    }
    if (!IsNone(op, "size")) {
        std::vector<int> v;
        CHECK_BOOL(Get(op, "size", v));
        if (2 != v.size()) {
            LOG(ERROR) << "Upsample::Init fail [" << op->type << " with " << v.size() << " sizes: rank-4 tensors only]";
            return Status::kUnsupport;
        }
        CHECK_BOOL(v[0] > 0 && v[1] > 0);
        size_h_ = v[0];
        size_w_ = v[1];
        by_size_ = true;
    }
    // (torch refuses both at once; a file that has both is not one it wrote)
    CHECK_BOOL(has_scale_ != by_size_);
    if (has_scale_ && !IsNone(op, "recompute_scale_factor")) {
        bool recompute = false;
        CHECK_BOOL(Get(op, "recompute_scale_factor", recompute));
        // the output size from the scale factor, then the rule of size=
        if (recompute) by_size_ = true;
    }
    return Status::kSuccess;
}

Status Upsample::Validate() {
    CHECK_STATUS(Layer::Validate());
    CHECK_STATUS(ValidateShape(1, 1));
    CHECK_STATUS(ValidateFloatLogged("Upsample"));
    const bool functional = op_ && (op_->type == "F.interpolate" || op_->type == "F.upsample");
    if (functional && (input_tensor_nodes_[0]->tensor.Shape().size() != 4 || output_tensor_nodes_[0]->tensor.Shape().size() != 4)) {
        LOG(ERROR) << "Upsample::Validate fail [" << op_->type << " on a rank-" << input_tensor_nodes_[0]->tensor.Shape().size()
                   << " tensor: rank 4 only]";
        return Status::kUnsupport;
    }
    if (IsNearestByScale()) return Status::kSuccess;   // the reference's form: its checks, nothing more
    Dims4 in, out;
    if (!GetDims4(input_tensor_nodes_[0]->tensor, in) || !GetDims4(output_tensor_nodes_[0]->tensor, out)) {
        LOG(ERROR) << "Upsample::Validate fail [input and output must be rank-4]";
        return Status::kErrorShape;
    }
    const int oh = has_scale_ ? si_upsample_out_size(in.h, scale_h_) : size_h_;
    const int ow = has_scale_ ? si_upsample_out_size(in.w, scale_w_) : size_w_;
    if (out.n != in.n || out.c != in.c || out.h != oh || out.w != ow) {
        LOG(ERROR) << "Upsample::Validate fail [output shape " << out.n << "x" << out.c << "x" << out.h << "x" << out.w << " for input "
                   << in.n << "x" << in.c << "x" << in.h << "x" << in.w << ": expected " << in.n << "x" << in.c << "x" << oh << "x" << ow;
        if (has_scale_) LOG(ERROR) << "  (floor(in * scale_factor) with scale_factor read as " << scale_h_ << ", " << scale_w_
                                   << ": the shortest decimals of the file's floats)";
        return Status::kErrorShape;
    }
    const int mode = UpsampleMode::kBilinear == upsample_mode_ ? SI_UPSAMPLE_BILINEAR : SI_UPSAMPLE_NEAREST;
    const bool use_scale = has_scale_ && !by_size_;
    if (0 != si_upsample_step(mode, in.h, out.h, align_corners_, use_scale ? scale_h_ : 0.0, &step_h_) ||
        0 != si_upsample_step(mode, in.w, out.w, align_corners_, use_scale ? scale_w_ : 0.0, &step_w_)) {
        LOG(ERROR) << "Upsample::Validate fail [no source step for these sizes]";
        return Status::kErrorShape;
    }
    return Status::kSuccess;
}

bool Upsample::MakeDesc(const Tensor& input, const Tensor& output, SiUpsampleDesc& d) const {
    Dims4 id, od;
    if (!GetDims4(input, id) || !GetDims4(output, od) || id.c != od.c || id.n != od.n) return false;
    d.n = id.n; d.ih = id.h; d.iw = id.w; d.c = id.c; d.in_ld = input.PixelStride();
    d.oh = od.h; d.ow = od.w; d.out_ld = output.PixelStride();
    d.align_corners = align_corners_ ? 1 : 0;
    d.step_h = step_h_;
    d.step_w = step_w_;
    return true;
}

Status Upsample::Forward(const Tensor& input, Tensor& output) {
    return RunOnDevice({&input}, {&output}, [this](const std::vector<Tensor>& in, std::vector<Tensor>& out) {
        Dims4 id, od;
        if (!GetDims4(in[0], id) || !GetDims4(out[0], od) || id.c != od.c || id.n != od.n) return Status::kErrorShape;
        if (IsHalf(in[0]) != IsHalf(out[0])) return Status::kUnsupport;
        if (UpsampleMode::kBilinear == upsample_mode_)
            return LaunchDesc(si_hip_upsample_bilinear_f32, si_hip_upsample_bilinear_f16, "Upsample (bilinear)", in[0], out[0], [this](auto&... a) { return MakeDesc(a...); });
        // nearest: by scale factor the reference's entry point, by size the same kernel with the steps of the sizes
        const bool steps = !IsNearestByScale();
        auto nearest = [&](const float* src, int c, int in_ld, float* dst, int out_ld) {
            return steps ? si_hip_upsample_nearest_steps_f32(src, id.n, id.h, id.w, c, in_ld, step_h_, step_w_, dst, od.h, od.w, out_ld, Stream())
                         : si_hip_upsample_nearest_f32(src, id.n, id.h, id.w, c, in_ld, scale_factor_h_, scale_factor_w_, dst, od.h, od.w, out_ld,
                                                       Stream());
        };
        if (IsHalf(in[0])) {
            // pure data movement: an fp16 tensor is copied as half as many 4-byte words
            if (id.c % 2 || in[0].PixelStride() % 2 || out[0].PixelStride() % 2) return Status::kUnsupport;
            return CheckHip(nearest(static_cast<const float*>(in[0].RawData()), id.c / 2, in[0].PixelStride() / 2,
                                    static_cast<float*>(out[0].RawData()), out[0].PixelStride() / 2),
                            "Upsample");
        }
        return CheckHip(nearest(in[0].Data<float>(), id.c, in[0].PixelStride(), out[0].Data<float>(), out[0].PixelStride()), "Upsample");
    });
}

const char* Upsample::KernelName() const {
    if (UpsampleMode::kBilinear != upsample_mode_) return "upsample_nearest";
    return DescKernelName(si_hip_upsample_bilinear_kernel_name, "upsample_bilinear_kernel", [this](auto&... a) { return MakeDesc(a...); });
}

}  // namespace SimpleInfer
