#include "pad_2d.h"

#include <algorithm>
#include <cstring>

namespace SimpleInfer {

DEFINE_LAYER_REGISTRY(Pad2d);

// A missing required key is kFail; what the file asks for and this layer does not do is remembered for Validate (kUnsupport).
Status Pad2d::Init(const pnnx::Operator* op) {
    CHECK_STATUS(Layer::Init(op));
    unsupported_.clear();
    value_ = 0.0f;
    std::vector<int> pads;
    if (op->type == "F.pad") {
        CHECK_BOOL(Get(op, "pad", pads));
        CHECK_BOOL(!pads.empty() && pads.size() % 2 == 0);
        if (pads.size() > 4) unsupported_ = "F.pad with " + std::to_string(pads.size()) + " entries pads the channels or the batch: the last two dimensions only";
        if (pads.size() == 2) pads.insert(pads.end(), {0, 0});   // W only
        std::string mode;
        CHECK_BOOL(Get(op, "mode", mode));
        if ("constant" == mode) mode_ = SI_PAD_CONSTANT;
        else if ("reflect" == mode) mode_ = SI_PAD_REFLECT;
        else if ("replicate" == mode) mode_ = SI_PAD_REPLICATE;
        else if ("circular" == mode) mode_ = SI_PAD_CIRCULAR;
        else if (unsupported_.empty()) unsupported_ = "unknown F.pad mode " + mode;
        if (!IsNone(op, "value")) CHECK_BOOL(GetNumber(op, "value", value_));   // (IsNone is the narrow rule: "None" as text is a value, which this read refuses)
    } else {
        int all = 0;
        if (Get(op, "padding", all)) {
            pads.assign(4, all);
        } else {
            CHECK_BOOL(Get(op, "padding", pads));
            CHECK_BOOL(pads.size() == 4);
        }
        if (op->type == "nn.ReflectionPad2d") mode_ = SI_PAD_REFLECT;
        else if (op->type == "nn.ReplicationPad2d") mode_ = SI_PAD_REPLICATE;
        else if (op->type == "nn.CircularPad2d") mode_ = SI_PAD_CIRCULAR;
        else mode_ = SI_PAD_CONSTANT;   // nn.ZeroPad2d, nn.ConstantPad2d
        if (op->type == "nn.ConstantPad2d") CHECK_BOOL(GetNumber(op, "value", value_));
    }
    pad_l_ = pads[0]; pad_r_ = pads[1]; pad_t_ = pads[2]; pad_b_ = pads[3];
    return Status::kSuccess;
}

Status Pad2d::Validate() {
    CHECK_STATUS(Layer::Validate());
    CHECK_STATUS(ValidateShape(1, 1));
    CHECK_STATUS(ValidateFloatLogged("Pad2d"));
    if (!unsupported_.empty()) {
        LOG(ERROR) << "Pad2d::Validate fail [" << unsupported_ << "]";
        return Status::kUnsupport;
    }
    Dims4 in, out;
    if (!GetDims4(input_tensor_nodes_[0]->tensor, in) || !GetDims4(output_tensor_nodes_[0]->tensor, out)) {
        LOG(ERROR) << "Pad2d::Validate fail [input and output must be rank-4]";
        return Status::kErrorShape;
    }
    const long long oh = (long long)in.h + pad_t_ + pad_b_, ow = (long long)in.w + pad_l_ + pad_r_;
    if (out.n != in.n || out.c != in.c || out.h != oh || out.w != ow) {
        LOG(ERROR) << "Pad2d::Validate fail [output shape " << out.n << "x" << out.c << "x" << out.h << "x" << out.w << " for input " << in.n << "x"
                   << in.c << "x" << in.h << "x" << in.w << " padded by (" << pad_l_ << ", " << pad_r_ << ", " << pad_t_ << ", " << pad_b_
                   << "): expected " << in.n << "x" << in.c << "x" << oh << "x" << ow << "]";
        return Status::kErrorShape;
    }
    // the limits of include/si_pad.h, per mode
    const char* why = nullptr;
    if (in.w + std::min(pad_l_, 0) + std::min(pad_r_, 0) < 1 || in.h + std::min(pad_t_, 0) + std::min(pad_b_, 0) < 1)
        why = "the negative pads crop the whole input";
    else if (SI_PAD_REFLECT == mode_ && (std::max(pad_l_, pad_r_) >= in.w || std::max(pad_t_, pad_b_) >= in.h))
        why = "a reflect pad must be smaller than the dimension it pads";
    else if (SI_PAD_CIRCULAR == mode_ && std::min(std::min(pad_l_, pad_r_), std::min(pad_t_, pad_b_)) < 0)
        why = "a circular pad must not be negative";
    else if (SI_PAD_CIRCULAR == mode_ && (std::max(pad_l_, pad_r_) > in.w || std::max(pad_t_, pad_b_) > in.h))
        why = "a circular pad must not exceed the dimension it pads";
    if (why) {
        LOG(ERROR) << "Pad2d::Validate fail [" << why << ": input " << in.h << "x" << in.w << ", pads (" << pad_l_ << ", " << pad_r_ << ", " << pad_t_
                   << ", " << pad_b_ << ")]";
        return Status::kUnsupport;
    }
    return Status::kSuccess;
}

// fp16 storage with the caller's fp32 tensor as input (the generators' first layer is a pad): the input is rounded to half into a
// buffer of this layer, then padded in half -- the same bits as padding first and rounding the larger tensor afterwards
bool Pad2d::StagesInput(const Tensor& input, const Tensor& output) { return !IsHalf(input) && IsHalf(output); }

bool Pad2d::MakeDesc(const Tensor& input, const Tensor& output, SiPad2dDesc& d) const {
    Dims4 id, od;
    if (!GetDims4(input, id) || !GetDims4(output, od) || id.c != od.c || id.n != od.n) return false;
    memset(&d, 0, sizeof(d));
    d.n = id.n; d.ih = id.h; d.iw = id.w; d.c = id.c; d.in_ld = StagesInput(input, output) ? id.c : input.PixelStride();
    d.oh = od.h; d.ow = od.w; d.out_ld = output.PixelStride();
    d.pad_l = pad_l_; d.pad_r = pad_r_; d.pad_t = pad_t_; d.pad_b = pad_b_;
    d.mode = mode_;
    d.value = value_;
    return true;
}

Status Pad2d::Forward(const Tensor& input, Tensor& output) {
    return RunOnDevice({&input}, {&output}, [this](const std::vector<Tensor>& in, std::vector<Tensor>& out) {
        // the two plain cases; fp16 in and fp32 out is kUnsupport there (the engine puts a cast step in front of a graph output)
        if (!StagesInput(in[0], out[0]))
            return LaunchDesc(si_hip_pad2d_f32, si_hip_pad2d_f16, "Pad2d", in[0], out[0], [this](auto&... a) { return MakeDesc(a...); });
        SiPad2dDesc d;
        if (!MakeDesc(in[0], out[0], d)) return Status::kErrorShape;
        // (the engine's first Forward is never captured, and a shape change rebuilds the plan: nothing is allocated during a graph capture)
        const size_t pixels = (size_t)d.n * d.ih * d.iw, need = pixels * d.c * 2;
        if (need > staging_dev_.bytes()) CHECK_STATUS(CheckHip(staging_dev_.Alloc(need), "Pad2d input staging"));
        CHECK_STATUS(CheckHip(si_hip_convert_f32_f16(in[0].Data<float>(), pixels, d.c, in[0].PixelStride(), staging_dev_.As<void>(), d.c, Stream()),
                              "Pad2d (fp32 input to half)"));
        return CheckHip(si_hip_pad2d_f16(&d, staging_dev_.As<void>(), out[0].RawData(), Stream()), "Pad2d");
    });
}

const char* Pad2d::KernelName() const {
    SiPad2dDesc d;
    if (input_tensor_nodes_.empty() || output_tensor_nodes_.empty() ||
        !MakeDesc(input_tensor_nodes_[0]->tensor, output_tensor_nodes_[0]->tensor, d))
        return "pad2d_kernel";
    const Tensor& in = input_tensor_nodes_[0]->tensor;
    const Tensor& out = output_tensor_nodes_[0]->tensor;
    // (a staged input lives in a hipMalloc'ed buffer of this layer: aligned as the output's base address is)
    return si_hip_pad2d_kernel_name(&d, StagesInput(in, out) ? nullptr : in.RawData(), out.RawData(), IsHalf(out) ? 1 : 0);
}

Status Pad2d::Deinit() {
    staging_dev_.Free();
    return Status::kSuccess;
}

// fp16 in and out run the fp16 kernel directly, fp32 in and fp16 out through the staged input: no cast pair
bool Pad2d::HalfStorageOk(std::string& why) const {
    if (1 == input_tensor_nodes_.size() && 1 == output_tensor_nodes_.size() &&
        StagesInput(input_tensor_nodes_[0]->tensor, output_tensor_nodes_[0]->tensor))
        return true;
    return Layer::HalfStorageOk(why);
}

}  // namespace SimpleInfer
