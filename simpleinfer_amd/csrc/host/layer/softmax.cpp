#include "softmax.h"

#include <cstring>

namespace SimpleInfer {

DEFINE_LAYER_REGISTRY(Softmax);

// A missing key is kFail; a dim or a rank this layer does not do is left for Validate (kUnsupport).
Status Softmax::Init(const pnnx::Operator* op) {
    CHECK_STATUS(Layer::Init(op));
    log_ = op->type == "nn.LogSoftmax" || op->type == "F.log_softmax";
    if (op->type == "nn.Softmax2d") {
        dim_ = -3;
    } else {
        CHECK_BOOL(Get(op, "dim", dim_));
    }
    axis_ = -1;
    return Status::kSuccess;
}

int Softmax::NhwcAxis(int dim, int rank) { return NhwcAxisOfDim(dim, rank); }

Status Softmax::Validate() {
    CHECK_STATUS(Layer::Validate());
    CHECK_STATUS(ValidateShape(1, 1));
    CHECK_STATUS(ValidateFloatLogged("Softmax"));
    const std::vector<int>& is = input_tensor_nodes_[0]->tensor.Shape();
    if (!IsSameShape(is, output_tensor_nodes_[0]->tensor.Shape())) {
        LOG(ERROR) << "Softmax::Validate fail [error input/output shape]";
        return Status::kErrorShape;
    }
    const int rank = (int)is.size();
    if (2 != rank && 4 != rank) {
        LOG(ERROR) << "Softmax::Validate fail [dim " << dim_ << " of a rank-" << rank << " tensor " << ShapeString(is) << ": ranks 2 and 4 only]";
        return Status::kUnsupport;
    }
    axis_ = NhwcAxis(dim_, rank);
    if (axis_ < 0) {
        LOG(ERROR) << "Softmax::Validate fail [dim " << dim_ << " is out of range for the rank-" << rank << " tensor " << ShapeString(is) << "]";
        return Status::kUnsupport;
    }
    return Status::kSuccess;
}

bool Softmax::MakeDesc(const Tensor& input, const Tensor& output, SiSoftmaxDesc& d) const {
    const std::vector<int>& is = input.Shape();
    if (!IsSameShape(is, output.Shape())) return false;
    const int axis = NhwcAxis(dim_, (int)is.size());
    if (axis < 0) return false;
    memset(&d, 0, sizeof(d));
    int id[4] = {0, 0, 0, 0};
    NhwcDims(input, id);   // (NhwcAxis has refused every rank but 2 and 4)
    d.n = id[0]; d.h = id[1]; d.w = id[2]; d.c = id[3];
    d.in_ld = input.PixelStride();
    d.out_ld = output.PixelStride();
    d.axis = axis;
    d.log = log_ ? 1 : 0;
    return true;
}

Status Softmax::Forward(const Tensor& input, Tensor& output) {
    return ForwardDesc(si_hip_softmax_f32, si_hip_softmax_f16, "Softmax", input, output, [this](auto&... a) { return MakeDesc(a...); });
}

const char* Softmax::KernelName() const {
    return DescKernelName(si_hip_softmax_kernel_name, "softmax", [this](auto&... a) { return MakeDesc(a...); });
}

// per element: the maximum, the subtraction, the exponential, the sum and the scaling (or the second subtraction)
double Softmax::Flops() const {
    if (input_tensor_nodes_.empty()) return 0.0;
    return 5.0 * (double)input_tensor_nodes_[0]->tensor.NumElements();
}

}  // namespace SimpleInfer
