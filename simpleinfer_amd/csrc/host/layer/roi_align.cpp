#include "roi_align.h"

#include <algorithm>
#include <cstring>

namespace SimpleInfer {

DEFINE_LAYER_REGISTRY(RoiAlign);

// output_size= an int or a pair; spatial_scale= a float (or an int); sampling_ratio= an int; aligned= a bool.  A missing key or None is
// torchvision's default; a key of another type is kFail.
Status RoiAlign::Init(const pnnx::Operator* op) {
    CHECK_STATUS(Layer::Init(op));
    std::vector<int> size;
    int one = 0;
    if (Get(op, "output_size", one)) size = {one, one};
    else if (!Get(op, "output_size", size) || size.size() != 2) return Status::kFail;
    pooled_h_ = size[0];
    pooled_w_ = size[1];
    bool have = false;
    spatial_scale_ = 1.0f;
    CHECK_BOOL(Number(op, "spatial_scale", spatial_scale_, have));
    sampling_ratio_ = -1;
    CHECK_BOOL(OptionalInt(op, "sampling_ratio", sampling_ratio_, have));
    aligned_ = false;
    if (!IsNoneOrText(op, "aligned")) CHECK_BOOL(Get(op, "aligned", aligned_));
    return Status::kSuccess;
}

Status RoiAlign::Validate() {
    CHECK_STATUS(Layer::Validate());
    const std::string name = op_ ? op_->name : std::string("-");
    if (input_tensor_nodes_.size() > 2 || (op_ && op_->inputs.size() > 2)) {
        LOG(ERROR) << "RoiAlign::Validate fail [" << name << ": the boxes as a list of per-image tensors are not served; one [K,5] tensor "
                   << "whose first column is the image index is]";
        return Status::kUnsupport;
    }
    CHECK_STATUS(ValidateShape(2, 1));
    CHECK_STATUS(ValidateFloatLogged("RoiAlign"));
    const Tensor& x = input_tensor_nodes_[0]->tensor;
    const Tensor& rois = input_tensor_nodes_[1]->tensor;
    const Tensor& out = output_tensor_nodes_[0]->tensor;
    const std::vector<int>& rs = rois.Shape();
    if (rs.size() == 2 && rs[1] == 4) {
        LOG(ERROR) << "RoiAlign::Validate fail [" << name << ": boxes of shape " << TupleString(rs) << " belong to the list form, one tensor per "
                   << "image, which is not served; one [K,5] tensor whose first column is the image index is]";
        return Status::kUnsupport;
    }
    Dims4 dx, dout;
    if (!GetDims4(x, dx) || !GetDims4(out, dout) || rs.size() != 2 || rs[1] != 5 || rs[0] <= 0) {
        LOG(ERROR) << "RoiAlign::Validate fail [" << name << ": input " << TupleString(x.Shape()) << ", boxes " << TupleString(rs) << ", output "
                   << TupleString(out.Shape()) << ": the input must be [N,C,H,W], the boxes [K,5], the output [K,C,ph,pw]]";
        return Status::kErrorShape;
    }
    if (pooled_h_ <= 0 || pooled_w_ <= 0 || dout.n != rs[0] || dout.c != dx.c || dout.h != pooled_h_ || dout.w != pooled_w_) {
        LOG(ERROR) << "RoiAlign::Validate fail [" << name << ": " << rs[0] << " boxes, " << dx.c << " channels, output_size=(" << pooled_h_ << ","
                   << pooled_w_ << "), but the output is " << dout.n << "x" << dout.c << "x" << dout.h << "x" << dout.w << ", not [K,C,ph,pw]]";
        return Status::kErrorShape;
    }
    // anything else the kernel refuses (a sampling_ratio beyond its limit, sizes beyond its 31-bit offsets)
    SiRoiAlignDesc d;
    const uintptr_t base = (uintptr_t)1 << 40, apart = (uintptr_t)1 << 36;   // aligned addresses far apart: the descriptor alone is asked
    if (!MakeDesc(x, rois, out, d) ||
        0 == strcmp("none", si_hip_roi_align_kernel_name(&d, (const void*)base, (const void*)(base + apart), (const void*)(base + 2 * apart), 0))) {
        LOG(ERROR) << "RoiAlign::Validate fail [" << name << ": the kernel refuses this descriptor: sampling_ratio=" << sampling_ratio_
                   << " beyond 256, or element offsets beyond 31 bits]";
        return Status::kUnsupport;
    }
    return Status::kSuccess;
}

bool RoiAlign::MakeDesc(const Tensor& x, const Tensor& rois, const Tensor& out, SiRoiAlignDesc& d) const {
    memset(&d, 0, sizeof(d));
    Dims4 dx, dout;
    const std::vector<int>& rs = rois.Shape();
    if (!GetDims4(x, dx) || !GetDims4(out, dout) || rs.size() != 2 || rs[1] != 5) return false;
    d.n = dx.n; d.c = dx.c; d.h = dx.h; d.w = dx.w;
    d.k = rs[0]; d.ph = dout.h; d.pw = dout.w;
    d.in_ld = x.PixelStride();
    d.out_ld = out.PixelStride();
    d.rois_ld = rois.PixelStride();
    d.sampling_ratio = sampling_ratio_;
    d.aligned = aligned_ ? 1 : 0;
    d.spatial_scale = spatial_scale_;
    return dout.n == d.k && dout.c == d.c;
}

Status RoiAlign::Forward(const std::vector<Tensor>& inputs, Tensor& output) {
    if (inputs.size() != 2) return Status::kUnsupport;
    return RunOnDevice({&inputs[0], &inputs[1]}, {&output}, [this](const std::vector<Tensor>& in, std::vector<Tensor>& out) {
        if (IsHalf(in[0]) != IsHalf(out[0]) || IsHalf(in[1])) return Status::kUnsupport;
        SiRoiAlignDesc d;
        if (!MakeDesc(in[0], in[1], out[0], d)) return Status::kErrorShape;
        const int rc = IsHalf(in[0]) ? si_hip_roi_align_f16(&d, in[0].RawData(), in[1].Data<float>(), out[0].RawData(), Stream())
                                     : si_hip_roi_align_f32(&d, in[0].Data<float>(), in[1].Data<float>(), out[0].Data<float>(), Stream());
        return CheckHip(rc, "RoiAlign");
    });
}

const char* RoiAlign::KernelName() const {
    const char* const fallback = "roi_align_kernel";
    if (input_tensor_nodes_.size() != 2 || output_tensor_nodes_.size() != 1) return fallback;
    const Tensor& x = input_tensor_nodes_[0]->tensor;
    const Tensor& rois = input_tensor_nodes_[1]->tensor;
    const Tensor& out = output_tensor_nodes_[0]->tensor;
    SiRoiAlignDesc d;
    if (!MakeDesc(x, rois, out, d)) return fallback;
    const int half = IsHalf(x) ? 1 : 0;
    // (before the arena is bound the tensors have no address yet: the name is then asked for aligned ones)
    if (!x.RawData() || !rois.RawData() || !out.RawData()) {
        const uintptr_t base = (uintptr_t)1 << 40, apart = (uintptr_t)1 << 36;
        return si_hip_roi_align_kernel_name(&d, (const void*)base, (const void*)(base + apart), (const void*)(base + 2 * apart), half);
    }
    return si_hip_roi_align_kernel_name(&d, x.RawData(), rois.RawData(), out.RawData(), half);
}

double RoiAlign::SamplesPerBin() const { return sampling_ratio_ > 0 ? (double)sampling_ratio_ * sampling_ratio_ : 4.0; }

// per output element and sample four multiplications and four additions, plus the division by the count
double RoiAlign::Flops() const {
    if (output_tensor_nodes_.empty()) return 0.0;
    return (8.0 * SamplesPerBin() + 1.0) * (double)output_tensor_nodes_[0]->tensor.NumElements();
}

// what the launch moves at most: four taps per sample, the boxes, the output
double RoiAlign::Bytes() const {
    if (input_tensor_nodes_.size() != 2 || output_tensor_nodes_.empty()) return Layer::Bytes();
    const Tensor& out = output_tensor_nodes_[0]->tensor;
    const double in_bytes = std::min((double)input_tensor_nodes_[0]->tensor.ByteSize(), 4.0 * SamplesPerBin() * (double)out.ByteSize());
    return in_bytes + (double)input_tensor_nodes_[1]->tensor.ByteSize() + (double)out.ByteSize();
}

bool RoiAlign::HalfStorageOk(std::string& why) const {
    if (input_tensor_nodes_.size() != 2 || output_tensor_nodes_.size() != 1) return Layer::HalfStorageOk(why);
    const bool hx = IsHalf(input_tensor_nodes_[0]->tensor), hr = IsHalf(input_tensor_nodes_[1]->tensor), ho = IsHalf(output_tensor_nodes_[0]->tensor);
    if (hr) {
        why = "RoIAlign reads its boxes as fp32: fp16 cannot hold pixel coordinates";
        return false;
    }
    if (hx != ho) {
        why = "RoIAlign reads x and writes the output in one storage type";
        return false;
    }
    return true;
}

}  // namespace SimpleInfer
