#include "grid_sample.h"

#include <algorithm>
#include <cstring>

namespace SimpleInfer {

DEFINE_LAYER_REGISTRY(GridSample);

// mode= and padding_mode= are strings, align_corners= a bool or None (False).  A missing mode / padding_mode is torch's default; a value
// torch does not have is kFail, one this kernel does not have (bicubic) is left for Validate, which names the reason.
Status GridSample::Init(const pnnx::Operator* op) {
    CHECK_STATUS(Layer::Init(op));
    form_ = GridForm::kStored;
    std::string mode = "bilinear", padding = "zeros";
    if (!IsNoneOrText(op, "mode")) CHECK_BOOL(Get(op, "mode", mode));
    if (!IsNoneOrText(op, "padding_mode")) CHECK_BOOL(Get(op, "padding_mode", padding));
    if (mode == "bilinear") mode_ = SI_GRID_BILINEAR;
    else if (mode == "nearest") mode_ = SI_GRID_NEAREST;
    else if (mode == "bicubic") mode_ = SI_GRID_BICUBIC;
    else return Status::kFail;
    if (padding == "zeros") padding_mode_ = SI_GRID_PAD_ZEROS;
    else if (padding == "border") padding_mode_ = SI_GRID_PAD_BORDER;
    else if (padding == "reflection") padding_mode_ = SI_GRID_PAD_REFLECTION;
    else return Status::kFail;
    align_corners_ = false;
    if (!IsNoneOrText(op, "align_corners")) CHECK_BOOL(Get(op, "align_corners", align_corners_));
    return Status::kSuccess;
}

Status GridSample::Validate() {
    CHECK_STATUS(Layer::Validate());
    CHECK_STATUS(ValidateShape(2, 1));
    CHECK_STATUS(ValidateFloatLogged("GridSample"));
    const std::string name = op_ ? op_->name : std::string("-");
    const Tensor& x = input_tensor_nodes_[0]->tensor;
    const Tensor& g = input_tensor_nodes_[1]->tensor;
    const Tensor& out = output_tensor_nodes_[0]->tensor;
    if (x.Shape().size() == 5 || (form_ == GridForm::kStored && g.Shape().size() == 5)) {
        LOG(ERROR) << "GridSample::Validate fail [" << name << ": 5-D (volumetric) sampling is not served; only [N,C,H,W] inputs are]";
        return Status::kUnsupport;
    }
    if (mode_ == SI_GRID_BICUBIC) {
        LOG(ERROR) << "GridSample::Validate fail [" << name << ": mode=bicubic is not served; bilinear and nearest are]";
        return Status::kUnsupport;
    }
    Dims4 dx, dg, dout;
    const bool theta = form_ == GridForm::kTheta;
    if (!GetDims4(x, dx) || !GetDims4(out, dout) || (!theta && !GetDims4(g, dg))) {
        LOG(ERROR) << "GridSample::Validate fail [" << name << ": the input must be [N,C,H,W], the grid [N,Ho,Wo,2], the output [N,C,Ho,Wo]]";
        return Status::kErrorShape;
    }
    bool ok = dout.n == dx.n && dout.c == dx.c;
    if (theta) {
        const std::vector<int>& ts = g.Shape();
        ok = ok && ts.size() == 3 && ts[0] == dx.n && ts[1] == 2 && ts[2] == 3;
    } else if (form_ == GridForm::kInPlace) {
        // the root [N, 2, Ho, Wo], stored NHWC
        ok = ok && dg.n == dx.n && dg.c == 2 && dg.h == dout.h && dg.w == dout.w;
    } else {
        // the file's [N, Ho, Wo, 2] as this project stores a rank-4 tensor: dimensions (0, 2, 3, 1) = [N][Wo][2][Ho]
        ok = ok && dg.n == dx.n && dg.h == dout.w && dg.w == 2 && dg.c == dout.h;
    }
    if (!ok) {
        LOG(ERROR) << "GridSample::Validate fail [" << name << ": input " << dx.n << "x" << dx.c << "x" << dx.h << "x" << dx.w << ", output " << dout.n
                   << "x" << dout.c << "x" << dout.h << "x" << dout.w << ": the grid must be [N,Ho,Wo,2] and the output [N,C,Ho,Wo]]";
        return Status::kErrorShape;
    }
    // anything else the kernel refuses (sizes beyond its 31-bit offsets)
    SiGridSampleDesc d;
    const uintptr_t base = (uintptr_t)1 << 40, apart = (uintptr_t)1 << 36;   // aligned addresses far apart: the descriptor alone is asked
    if (!MakeDesc(x, g, out, d) ||
        0 == strcmp("none", si_hip_grid_sample_kernel_name(&d, (const void*)base, (const void*)(base + apart), (const void*)(base + 2 * apart), 0))) {
        LOG(ERROR) << "GridSample::Validate fail [" << name << ": the kernel refuses these sizes: element offsets beyond 31 bits]";
        return Status::kUnsupport;
    }
    return Status::kSuccess;
}

bool GridSample::SetGridInPlace(TensorNode* root) {
    if (!root || input_tensor_nodes_.size() != 2 || output_tensor_nodes_.size() != 1) return false;
    Dims4 dr, dout;
    if (!GetDims4(root->tensor, dr) || !GetDims4(output_tensor_nodes_[0]->tensor, dout)) return false;
    if (dr.n != dout.n || dr.h != dout.h || dr.w != dout.w || dr.c != 2) return false;
    SetInputNodes({input_tensor_nodes_[0], root});
    form_ = GridForm::kInPlace;
    return true;
}

bool GridSample::SetTheta(TensorNode* theta) {
    if (!theta || input_tensor_nodes_.size() != 2 || output_tensor_nodes_.size() != 1) return false;
    const std::vector<int>& ts = theta->tensor.Shape();
    const std::vector<int>& os = output_tensor_nodes_[0]->tensor.Shape();
    if (ts.size() != 3 || os.size() != 4 || ts[0] != os[0] || ts[1] != 2 || ts[2] != 3) return false;
    SetInputNodes({input_tensor_nodes_[0], theta});
    form_ = GridForm::kTheta;
    return true;
}

bool GridSample::MakeDesc(const Tensor& x, const Tensor& grid, const Tensor& out, SiGridSampleDesc& d) const {
    memset(&d, 0, sizeof(d));
    Dims4 dx, dout;
    if (!GetDims4(x, dx) || !GetDims4(out, dout)) return false;
    d.n = dx.n; d.c = dx.c; d.h = dx.h; d.w = dx.w; d.ho = dout.h; d.wo = dout.w;
    d.in_ld = x.PixelStride();
    d.out_ld = out.PixelStride();
    d.mode = mode_;
    d.padding_mode = padding_mode_;
    d.align_corners = align_corners_ ? 1 : 0;
    d.spatial_dims = 2;
    if (form_ == GridForm::kTheta) {
        d.grid_source = SI_GRID_THETA;
        return grid.Shape().size() == 3;
    }
    d.grid_source = SI_GRID_TENSOR;
    if (grid.Shape().size() != 4) return false;
    const long long ld = grid.PixelStride();
    if (form_ == GridForm::kInPlace) {
        d.gs_n = (long long)d.ho * d.wo * ld; d.gs_h = (long long)d.wo * ld; d.gs_w = ld; d.gs_k = 1;
    } else {
        d.gs_n = 2LL * d.wo * ld; d.gs_h = 1; d.gs_w = 2 * ld; d.gs_k = ld;
    }
    return true;
}

Status GridSample::Forward(const std::vector<Tensor>& inputs, Tensor& output) {
    if (inputs.size() != 2) return Status::kUnsupport;
    return RunOnDevice({&inputs[0], &inputs[1]}, {&output}, [this](const std::vector<Tensor>& in, std::vector<Tensor>& out) {
        if (IsHalf(in[0]) != IsHalf(out[0]) || IsHalf(in[0]) != IsHalf(in[1])) return Status::kUnsupport;
        SiGridSampleDesc d;
        if (!MakeDesc(in[0], in[1], out[0], d)) return Status::kErrorShape;
        const int rc = IsHalf(in[0]) ? si_hip_grid_sample_f16(&d, in[0].RawData(), in[1].RawData(), out[0].RawData(), Stream())
                                     : si_hip_grid_sample_f32(&d, in[0].Data<float>(), in[1].Data<float>(), out[0].Data<float>(), Stream());
        return CheckHip(rc, "GridSample");
    });
}

const char* GridSample::KernelName() const {
    const char* const fallback = "grid_sample_kernel";
    if (input_tensor_nodes_.size() != 2 || output_tensor_nodes_.size() != 1) return fallback;
    const Tensor& x = input_tensor_nodes_[0]->tensor;
    const Tensor& g = input_tensor_nodes_[1]->tensor;
    const Tensor& out = output_tensor_nodes_[0]->tensor;
    SiGridSampleDesc d;
    if (!MakeDesc(x, g, out, d)) return fallback;
    const int half = IsHalf(x) ? 1 : 0;
    // (before the arena is bound the tensors have no address yet: the name is then asked for aligned ones)
    if (!x.RawData() || !g.RawData() || !out.RawData()) {
        const uintptr_t base = (uintptr_t)1 << 40, apart = (uintptr_t)1 << 36;
        return si_hip_grid_sample_kernel_name(&d, (const void*)base, (const void*)(base + apart), (const void*)(base + 2 * apart), half);
    }
    return si_hip_grid_sample_kernel_name(&d, x.RawData(), g.RawData(), out.RawData(), half);
}

// bilinear: per output element four multiply-adds and a weight product shared by the channels; nearest: none
double GridSample::Flops() const {
    if (output_tensor_nodes_.empty() || mode_ != SI_GRID_BILINEAR) return 0.0;
    return 8.0 * (double)output_tensor_nodes_[0]->tensor.NumElements();
}

// what the launch moves at most: four taps per output element, the coordinates, the output
double GridSample::Bytes() const {
    if (input_tensor_nodes_.size() != 2 || output_tensor_nodes_.empty()) return Layer::Bytes();
    const Tensor& out = output_tensor_nodes_[0]->tensor;
    const double taps = mode_ == SI_GRID_BILINEAR ? 4.0 : 1.0;
    const double in_bytes = std::min((double)input_tensor_nodes_[0]->tensor.ByteSize(), taps * (double)out.ByteSize());
    return in_bytes + (double)input_tensor_nodes_[1]->tensor.ByteSize() + (double)out.ByteSize();
}

bool GridSample::HalfStorageOk(std::string& why) const {
    // native fp32 and fp16 kernels; x, the grid (or theta) and the output share one storage type
    int half = 0, total = 0;
    for (auto* n : input_tensor_nodes_) { half += IsHalf(n->tensor); ++total; }
    for (auto* n : output_tensor_nodes_) { half += IsHalf(n->tensor); ++total; }
    if (half == 0 || half == total) return true;
    why = "F.grid_sample reads x and the grid and writes the output in one storage type";
    return false;
}

}  // namespace SimpleInfer
