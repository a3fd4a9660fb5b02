#include "reduce.h"

#include <cstring>

namespace SimpleInfer {

DEFINE_LAYER_REGISTRY(Reduce);

// A mistyped key is kFail; a missing dim, and a dtype other than None, are kUnsupport; dims the shape does not allow are left for Validate.
Status Reduce::Init(const pnnx::Operator* op) {
    CHECK_STATUS(Layer::Init(op));
    op_code_ = op->type == "torch.sum" ? SI_REDUCE_SUM : op->type == "torch.amax" ? SI_REDUCE_AMAX : op->type == "torch.amin" ? SI_REDUCE_AMIN : SI_REDUCE_MEAN;
    dims_.clear();
    axes_ = 0;
    keepdim_ = false;
    return ReadDimKeepdimDtype("Reduce", op, dims_, keepdim_);
}

Status Reduce::Validate() {
    CHECK_STATUS(Layer::Validate());
    CHECK_STATUS(ValidateShape(1, 1));
    CHECK_STATUS(ValidateFloatLogged("Reduce"));
    const Tensor& in = input_tensor_nodes_[0]->tensor;
    const Tensor& out = output_tensor_nodes_[0]->tensor;
    const std::vector<int>& is = in.Shape();
    const int rank = (int)is.size();
    int id[4];
    if (!NhwcDims(in, id)) {
        LOG(ERROR) << "Reduce::Validate fail [dim " << TupleString(dims_) << " of a rank-" << rank << " tensor " << ShapeString(is) << ": ranks 2 and 4 only]";
        return Status::kUnsupport;
    }
    CHECK_STATUS(DimsToNhwcMask("Reduce", dims_, rank, axes_));
    CHECK_STATUS(RefuseChannelMix("Reduce", dims_, is, axes_));
    const bool pool = rank == 4 && axes_ == (SI_REDUCE_AXIS_H | SI_REDUCE_AXIS_W);
    if (!keepdim_ && !pool) {
        LOG(ERROR) << "Reduce::Validate fail [keepdim=False over dim " << TupleString(dims_) << " of a rank-" << rank
                   << " tensor: only dims (2,3) of a rank-4 tensor drop their axes here (the [N, C] result is the [N, 1, 1, C] memory)]";
        return Status::kUnsupport;
    }
    // the shape the rule gives, as the engine holds it (NHWC; [N, F]; [N, C] for the pool without keepdim)
    const std::vector<int> want = keepdim_ ? KeptDimsShape(id, rank, axes_) : std::vector<int>{id[0], id[3]};
    if (!IsSameShape(want, out.Shape())) {
        LOG(ERROR) << "Reduce::Validate fail [the file's output is " << ShapeString(out.Shape()) << ", the rule gives " << ShapeString(want)
                   << " for dim " << TupleString(dims_) << (keepdim_ ? " keepdim=True" : " keepdim=False") << " of " << ShapeString(is) << " (NHWC)]";
        return Status::kErrorShape;
    }
    SiReduceDesc d;
    if (!MakeDesc(in, out, d) || 0 == strcmp("none", si_hip_reduce_kernel_name(&d, nullptr, nullptr, 0))) {
        LOG(ERROR) << "Reduce::Validate fail [" << ShapeString(is) << " over dim " << TupleString(dims_) << ": the kernels refuse this tensor (element offsets beyond 31 bits)]";
        return Status::kUnsupport;
    }
    return Status::kSuccess;
}

bool Reduce::MakeDesc(const Tensor& input, const Tensor& output, SiReduceDesc& d) const {
    int id[4], axes = 0;
    if (!NhwcDims(input, id) || Status::kSuccess != DimsToNhwcMask("Reduce", dims_, (int)input.Shape().size(), axes)) return false;
    memset(&d, 0, sizeof(d));
    d.n = id[0]; d.h = id[1]; d.w = id[2]; d.c = id[3];
    d.in_ld = input.PixelStride();
    d.out_ld = output.PixelStride();
    d.axes = axes;
    d.op = op_code_;
    size_t want = 1;
    for (int a = 0; a < 4; ++a) want *= ((axes >> a) & 1) ? 1 : (size_t)id[a];
    return output.NumElements() == want;
}

Status Reduce::Forward(const Tensor& input, Tensor& output) {
    return ForwardDesc(si_hip_reduce_f32, si_hip_reduce_f16, "Reduce", input, output, [this](auto&... a) { return MakeDesc(a...); });
}

const char* Reduce::KernelName() const {
    return DescKernelName(si_hip_reduce_kernel_name, "reduce", [this](auto&... a) { return MakeDesc(a...); });
}

// one addition or one selection per input element
double Reduce::Flops() const {
    if (input_tensor_nodes_.empty()) return 0.0;
    return (double)input_tensor_nodes_[0]->tensor.NumElements();
}

}  // namespace SimpleInfer
