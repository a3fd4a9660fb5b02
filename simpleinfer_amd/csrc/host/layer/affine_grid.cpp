#include "affine_grid.h"

#include <cstring>

namespace SimpleInfer {

DEFINE_LAYER_REGISTRY(AffineGrid);

Status AffineGrid::Init(const pnnx::Operator* op) {
    CHECK_STATUS(Layer::Init(op));
    size_.clear();
    CHECK_BOOL(Get(op, "size", size_));
    align_corners_ = false;
    if (!IsNoneOrText(op, "align_corners")) CHECK_BOOL(Get(op, "align_corners", align_corners_));
    return Status::kSuccess;
}

Status AffineGrid::Validate() {
    CHECK_STATUS(Layer::Validate());
    CHECK_STATUS(ValidateShape(1, 1));
    CHECK_STATUS(ValidateFloatLogged("AffineGrid"));
    const std::string name = op_ ? op_->name : std::string("-");
    const Tensor& theta = input_tensor_nodes_[0]->tensor;
    const Tensor& out = output_tensor_nodes_[0]->tensor;
    if (size_.size() == 5 || (theta.Shape().size() == 3 && theta.Shape()[1] == 3 && theta.Shape()[2] == 4)) {
        LOG(ERROR) << "AffineGrid::Validate fail [" << name << ": 3-D affine grids (size of 5 entries, theta [N,3,4]) are not served]";
        return Status::kUnsupport;
    }
    const std::vector<int>& ts = theta.Shape();
    Dims4 dout;   // stored [N][W][2][H]
    if (ts.size() != 3 || ts[1] != 2 || ts[2] != 3 || size_.size() != 4 || !GetDims4(out, dout) || dout.w != 2 || dout.n != ts[0]) {
        LOG(ERROR) << "AffineGrid::Validate fail [" << name << ": theta must be [N,2,3], size= (N,C,H,W) and the output [N,H,W,2]; theta is "
                   << TupleString(ts) << ", size= " << TupleString(size_) << "]";
        return Status::kErrorShape;
    }
    // size= against the output operand; the leading entry follows a re-batch (the engine has rewritten dimension 0 of the operands)
    int size_n = size_[0];
    if (op_ && op_->outputs.size() == 1 && !op_->outputs[0]->shape.empty() && op_->outputs[0]->shape[0] != dout.n && size_n == op_->outputs[0]->shape[0])
        size_n = dout.n;
    if (size_n != dout.n || size_[2] != dout.c || size_[3] != dout.h || size_[1] <= 0) {
        LOG(ERROR) << "AffineGrid::Validate fail [" << name << ": size= " << TupleString(size_) << " does not give the output [" << dout.n << ","
                   << dout.c << "," << dout.h << ",2]]";
        return Status::kErrorShape;
    }
    SiAffineGridDesc d;
    const uintptr_t base = (uintptr_t)1 << 40, apart = (uintptr_t)1 << 36;
    if (!MakeDesc(theta, out, d) || 0 == strcmp("none", si_hip_affine_grid_kernel_name(&d, (const void*)base, (const void*)(base + apart), 0))) {
        LOG(ERROR) << "AffineGrid::Validate fail [" << name << ": the kernel refuses these sizes: element offsets beyond 31 bits]";
        return Status::kUnsupport;
    }
    return Status::kSuccess;
}

bool AffineGrid::MakeDesc(const Tensor& theta, const Tensor& out, SiAffineGridDesc& d) const {
    memset(&d, 0, sizeof(d));
    Dims4 dout;
    if (theta.Shape().size() != 3 || !GetDims4(out, dout) || dout.w != 2) return false;
    d.n = dout.n;
    d.h = dout.c;   // stored [N][W][2][H]
    d.w = dout.h;
    d.out_ld = out.PixelStride();
    d.align_corners = align_corners_ ? 1 : 0;
    return true;
}

Status AffineGrid::Forward(const Tensor& input, Tensor& output) {
    return ForwardDesc(si_hip_affine_grid_f32, si_hip_affine_grid_f16, "AffineGrid", input, output, [this](auto&... a) { return MakeDesc(a...); });
}

const char* AffineGrid::KernelName() const {
    if (input_tensor_nodes_.size() != 1 || output_tensor_nodes_.size() != 1) return "affine_grid_kernel";
    const Tensor& theta = input_tensor_nodes_[0]->tensor;
    const Tensor& out = output_tensor_nodes_[0]->tensor;
    SiAffineGridDesc d;
    if (!MakeDesc(theta, out, d)) return "affine_grid_kernel";
    if (!theta.RawData() || !out.RawData()) return IsHalf(out) ? "affine_grid_kernel<_Float16>" : "affine_grid_kernel<float>";
    return si_hip_affine_grid_kernel_name(&d, theta.RawData(), out.RawData(), IsHalf(out) ? 1 : 0);
}

// two fused multiply-adds per coordinate
double AffineGrid::Flops() const {
    return output_tensor_nodes_.empty() ? 0.0 : 4.0 * (double)output_tensor_nodes_[0]->tensor.NumElements();
}

bool AffineGrid::HalfStorageOk(std::string& why) const {
    // native fp32 and fp16 kernels; theta and the grid share one storage type
    if (input_tensor_nodes_.empty() || output_tensor_nodes_.empty()) return true;
    if (IsHalf(input_tensor_nodes_[0]->tensor) == IsHalf(output_tensor_nodes_[0]->tensor)) return true;
    why = "F.affine_grid reads theta and writes the grid in one storage type";
    return false;
}

}  // namespace SimpleInfer
