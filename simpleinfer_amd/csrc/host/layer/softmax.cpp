#include "softmax.h"

#include <cstring>
#include <sstream>

namespace SimpleInfer {

DEFINE_LAYER_REGISTRY(Softmax);

// A missing key is kFail; a dim or a rank this layer does not do is left for Validate (kUnsupport).
Status Softmax::Init(const pnnx::Operator* op) {
    CHECK_STATUS(Layer::Init(op));
    log_ = op->type == "nn.LogSoftmax" || op->type == "F.log_softmax";
    if (op->type == "nn.Softmax2d") {
        dim_ = -3;
    } else {
        CHECK_BOOL(CheckParam(op, "dim", 2));
        dim_ = op->params.at("dim").i;
    }
    axis_ = -1;
    return Status::kSuccess;
}

int Softmax::NhwcAxis(int dim, int rank) {
    if (dim < 0) dim += rank;
    if (dim < 0 || dim >= rank) return -1;
    if (2 == rank) return 1 == dim ? 3 : 0;
    if (4 != rank) return -1;
    switch (dim) {   // Cat::NhwcAxis
        case 1: return 3;
        case 2: return 1;
        case 3: return 2;
        default: return 0;
    }
}

static std::string ShapeString(const std::vector<int>& s) {
    std::ostringstream os;
    for (size_t i = 0; i < s.size(); ++i) os << (i ? "x" : "") << s[i];
    return os.str();
}

Status Softmax::Validate() {
    CHECK_STATUS(Layer::Validate());
    CHECK_STATUS(ValidateShape(1, 1));
    if (Status::kSuccess != ValidateFloat()) {
        LOG(ERROR) << "Softmax::Validate fail [unsupport input/output data type]";
        return Status::kUnsupport;
    }
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
    if (2 == is.size()) {
        d.n = is[0]; d.h = 1; d.w = 1; d.c = is[1];
    } else {
        d.n = is[0]; d.h = is[1]; d.w = is[2]; d.c = is[3];
    }
    d.in_ld = input.PixelStride();
    d.out_ld = output.PixelStride();
    d.axis = axis;
    d.log = log_ ? 1 : 0;
    return true;
}

Status Softmax::Forward(const Tensor& input, Tensor& output) {
    return RunOnDevice({&input}, {&output}, [this](const std::vector<Tensor>& in, std::vector<Tensor>& out) {
        if (IsHalf(in[0]) != IsHalf(out[0])) return Status::kUnsupport;
        SiSoftmaxDesc d;
        if (!MakeDesc(in[0], out[0], d)) return Status::kErrorShape;
        if (IsHalf(in[0])) return CheckHip(si_hip_softmax_f16(&d, in[0].RawData(), out[0].RawData(), Stream()), "Softmax");
        return CheckHip(si_hip_softmax_f32(&d, in[0].Data<float>(), out[0].Data<float>(), Stream()), "Softmax");
    });
}

const char* Softmax::KernelName() const {
    SiSoftmaxDesc d;
    if (input_tensor_nodes_.empty() || output_tensor_nodes_.empty() ||
        !MakeDesc(input_tensor_nodes_[0]->tensor, output_tensor_nodes_[0]->tensor, d))
        return "softmax";
    const Tensor& in = input_tensor_nodes_[0]->tensor;
    const Tensor& out = output_tensor_nodes_[0]->tensor;
    return si_hip_softmax_kernel_name(&d, in.RawData(), out.RawData(), IsHalf(in) ? 1 : 0);
}

// per element: the maximum, the subtraction, the exponential, the sum and the scaling (or the second subtraction)
double Softmax::Flops() const {
    if (input_tensor_nodes_.empty()) return 0.0;
    return 5.0 * (double)input_tensor_nodes_[0]->tensor.NumElements();
}

// fp16 in and out run the fp16 kernel directly; a mixed pair does not exist for this layer
bool Softmax::HalfStorageOk(std::string& why) const { return Layer::HalfStorageOk(why); }

}  // namespace SimpleInfer
