#include "lp_norm.h"

#include <cmath>
#include <cstring>

namespace SimpleInfer {

DEFINE_LAYER_REGISTRY(LpNorm);

namespace {

// p as the file has it: 1 / 2 as an int or a float, inf as a float or as the text pnnx writes, "fro"; 0: served, 1: a value this layer
// does not do (`text` says which), -1: a key of another type
int ReadP(const pnnx::Operator* op, int& p, std::string& text) {
    if (IsNoneOrText(op, "p")) {   // (torch's default)
        p = SI_LPNORM_P2;
        return 0;
    }
    int i = 0;
    float f = 0.0f;
    std::string s;
    if (Get(op, "p", i)) {
        text = std::to_string(i);
        f = (float)i;
    } else if (Get(op, "p", f)) {
        text = std::to_string(f);
    } else if (Get(op, "p", s)) {
        text = s;
        if (s == "inf") f = INFINITY;
        else if (s == "fro") f = 2.0f;
        else return 1;
    } else {
        return -1;
    }
    if (f == 1.0f) p = SI_LPNORM_P1;
    else if (f == 2.0f) p = SI_LPNORM_P2;
    else if (std::isinf(f) && f > 0.0f) p = SI_LPNORM_PINF;
    else return 1;
    return 0;
}

}  // namespace

// A mistyped key is kFail; a p other than 1, 2, inf, a missing dim on torch.norm and a dtype other than None are kUnsupport; dims the
// shape does not allow are left for Validate.
Status LpNorm::Init(const pnnx::Operator* op) {
    CHECK_STATUS(Layer::Init(op));
    normalize_ = op->type == "F.normalize";
    dims_.clear();
    axes_ = 0;
    keepdim_ = false;
    eps_ = 0.0f;
    std::string text;
    const int rc = ReadP(op, p_, text);
    CHECK_BOOL(rc >= 0);
    if (rc > 0) {
        LOG(ERROR) << "LpNorm::Init fail [" << op->type << " with p=" << text << ": p = 1, 2 and inf only]";
        return Status::kUnsupport;
    }
    if (normalize_) {
        int dim = 1;
        CHECK_BOOL(Get(op, "dim", dim));
        dims_.push_back(dim);
        eps_ = 1e-12f;
        if (FindParam(op, "eps")) CHECK_BOOL(GetNumber(op, "eps", eps_));
        CHECK_BOOL(eps_ >= 0.0f);
        keepdim_ = true;
        return Status::kSuccess;
    }
    return ReadDimKeepdimDtype("LpNorm", op, dims_, keepdim_);
}

Status LpNorm::Validate() {
    CHECK_STATUS(Layer::Validate());
    CHECK_STATUS(ValidateShape(1, 1));
    CHECK_STATUS(ValidateFloatLogged("LpNorm"));
    const Tensor& in = input_tensor_nodes_[0]->tensor;
    const Tensor& out = output_tensor_nodes_[0]->tensor;
    const std::vector<int>& is = in.Shape();
    const int rank = (int)is.size();
    int id[4];
    if (!NhwcDims(in, id)) {
        LOG(ERROR) << "LpNorm::Validate fail [dim " << TupleString(dims_) << " of a rank-" << rank << " tensor " << ShapeString(is) << ": ranks 2 and 4 only]";
        return Status::kUnsupport;
    }
    CHECK_STATUS(DimsToNhwcMask("LpNorm", dims_, rank, axes_));
    CHECK_STATUS(RefuseChannelMix("LpNorm", dims_, is, axes_));
    // the shape the rule gives, as the engine holds it (NHWC; [N, F]; [N, H, W] and [N, C] for the two served keepdim=False cases)
    std::vector<int> want;
    if (normalize_) {
        want = is;
    } else if (!keepdim_) {
        const bool pixel_norm = rank == 4 && axes_ == 8;         // dim=1: [N, H, W], the [N, H, W, 1] memory
        const bool pool = rank == 4 && axes_ == (2 | 4);         // dims (2, 3): [N, C], the [N, 1, 1, C] memory
        if (!pixel_norm && !pool) {
            LOG(ERROR) << "LpNorm::Validate fail [keepdim=False over dim " << TupleString(dims_) << " of a rank-" << rank
                       << " tensor: only dim 1 and dims (2,3) of a rank-4 tensor drop their axes here (the result is the keepdim result's memory)]";
            return Status::kUnsupport;
        }
        if (pixel_norm) want = {id[0], id[1], id[2]};
        else want = {id[0], id[3]};
    } else {
        want = KeptDimsShape(id, rank, axes_);
    }
    if (!IsSameShape(want, out.Shape())) {
        LOG(ERROR) << "LpNorm::Validate fail [the file's output is " << ShapeString(out.Shape()) << ", the rule gives " << ShapeString(want)
                   << " for dim " << TupleString(dims_) << (normalize_ ? " (normalize)" : keepdim_ ? " keepdim=True" : " keepdim=False") << " of "
                   << ShapeString(is) << " (NHWC)]";
        return Status::kErrorShape;
    }
    SiLpNormDesc d;
    if (!MakeDesc(in, out, d) || 0 == strcmp("none", si_hip_lpnorm_kernel_name(&d, nullptr, nullptr, 0))) {
        LOG(ERROR) << "LpNorm::Validate fail [" << ShapeString(is) << " over dim " << TupleString(dims_) << ": the kernels refuse this tensor (element offsets beyond 31 bits)]";
        return Status::kUnsupport;
    }
    return Status::kSuccess;
}

bool LpNorm::SetNormalize(TensorNode* out) {
    if (normalize_ || dims_.size() != 1 || input_tensor_nodes_.size() != 1 || !out) return false;
    if (!IsSameShape(input_tensor_nodes_[0]->tensor.Shape(), out->tensor.Shape())) return false;
    normalize_ = true;
    eps_ = 0.0f;
    SetOutputNodes({out});
    return true;
}

bool LpNorm::MakeDesc(const Tensor& input, const Tensor& output, SiLpNormDesc& d) const {
    int id[4], axes = 0;
    if (!NhwcDims(input, id) || Status::kSuccess != DimsToNhwcMask("LpNorm", dims_, (int)input.Shape().size(), axes)) return false;
    memset(&d, 0, sizeof(d));
    d.n = id[0]; d.h = id[1]; d.w = id[2]; d.c = id[3];
    d.in_ld = input.PixelStride();
    d.out_ld = output.PixelStride();
    if (output.Shape().size() == 3) {
        // keepdim=False over dim 1: the dense [N, H, W] result is the [N, H, W, 1] memory, one element per pixel
        if (output.PixelStride() != output.Shape().back()) return false;
        d.out_ld = 1;
    }
    d.axes = axes;
    d.p = p_;
    d.normalize = normalize_ ? 1 : 0;
    d.eps = normalize_ ? eps_ : 0.0f;
    size_t want = 1;
    for (int a = 0; a < 4; ++a) want *= (!normalize_ && ((axes >> a) & 1)) ? 1 : (size_t)id[a];
    return output.NumElements() == want;
}

Status LpNorm::Forward(const Tensor& input, Tensor& output) {
    return ForwardDesc(si_hip_lpnorm_f32, si_hip_lpnorm_f16, "LpNorm", input, output, [this](auto&... a) { return MakeDesc(a...); });
}

const char* LpNorm::KernelName() const {
    return DescKernelName(si_hip_lpnorm_kernel_name, "lpnorm", [this](auto&... a) { return MakeDesc(a...); });
}

// per input element one multiplication (or absolute value) and one addition (or selection); normalize adds a division
double LpNorm::Flops() const {
    if (input_tensor_nodes_.empty()) return 0.0;
    return (normalize_ ? 3.0 : 2.0) * (double)input_tensor_nodes_[0]->tensor.NumElements();
}

}  // namespace SimpleInfer
