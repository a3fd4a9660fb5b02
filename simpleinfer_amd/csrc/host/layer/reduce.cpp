#include "reduce.h"

#include <cstring>

#include "softmax.h"

namespace SimpleInfer {

DEFINE_LAYER_REGISTRY(Reduce);

// A mistyped key is kFail; a missing dim, and a dtype other than None, are kUnsupport; dims the shape does not allow are left for Validate.
Status Reduce::Init(const pnnx::Operator* op) {
    CHECK_STATUS(Layer::Init(op));
    op_code_ = op->type == "torch.sum" ? SI_REDUCE_SUM : op->type == "torch.amax" ? SI_REDUCE_AMAX : op->type == "torch.amin" ? SI_REDUCE_AMIN : SI_REDUCE_MEAN;
    dims_.clear();
    axes_ = 0;
    if (IsNone(op, "dim")) {
        LOG(ERROR) << "Reduce::Init fail [" << op->type << " without dim: the reduction to a scalar is not served]";
        return Status::kUnsupport;
    }
    int one = 0;
    if (Get(op, "dim", one)) {
        dims_.push_back(one);
    } else {
        CHECK_BOOL(Get(op, "dim", dims_) && !dims_.empty());
    }
    keepdim_ = false;
    if (FindParam(op, "keepdim")) CHECK_BOOL(Get(op, "keepdim", keepdim_));
    if (!IsNoneOrText(op, "dtype")) {
        LOG(ERROR) << "Reduce::Init fail [" << op->type << " with a dtype: the result has the input's type here]";
        return Status::kUnsupport;
    }
    return Status::kSuccess;
}

Status Reduce::Mask(int rank, int& axes) const {
    axes = 0;
    for (int dim : dims_) {
        const int axis = Softmax::NhwcAxis(dim, rank);
        if (axis < 0) {
            LOG(ERROR) << "Reduce: dim " << dim << " of " << TupleString(dims_) << " is out of range for a rank-" << rank << " tensor";
            return Status::kUnsupport;
        }
        if (axes & (1 << axis)) {
            LOG(ERROR) << "Reduce: dim " << dim << " appears twice in " << TupleString(dims_);
            return Status::kFail;
        }
        axes |= 1 << axis;
    }
    return axes != 0 ? Status::kSuccess : Status::kFail;
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
    CHECK_STATUS(Mask(rank, axes_));
    if ((axes_ & SI_REDUCE_AXIS_C) && axes_ != SI_REDUCE_AXIS_C) {
        LOG(ERROR) << "Reduce::Validate fail [dim " << TupleString(dims_) << " of " << ShapeString(is)
                   << " (NHWC) reduces the channels together with another axis: the channel dim alone, or any of the others]";
        return Status::kUnsupport;
    }
    const bool pool = rank == 4 && axes_ == (SI_REDUCE_AXIS_H | SI_REDUCE_AXIS_W);
    if (!keepdim_ && !pool) {
        LOG(ERROR) << "Reduce::Validate fail [keepdim=False over dim " << TupleString(dims_) << " of a rank-" << rank
                   << " tensor: only dims (2,3) of a rank-4 tensor drop their axes here (the [N, C] result is the [N, 1, 1, C] memory)]";
        return Status::kUnsupport;
    }
    // the shape the rule gives, as the engine holds it (NHWC; [N, F]; [N, C] for the pool without keepdim)
    std::vector<int> want;
    if (!keepdim_) {
        want = {id[0], id[3]};
    } else if (rank == 4) {
        for (int a = 0; a < 4; ++a) want.push_back(((axes_ >> a) & 1) ? 1 : id[a]);
    } else {
        want = {(axes_ & SI_REDUCE_AXIS_N) ? 1 : id[0], (axes_ & SI_REDUCE_AXIS_C) ? 1 : id[3]};
    }
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
    if (!NhwcDims(input, id) || Status::kSuccess != Mask((int)input.Shape().size(), axes)) return false;
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
