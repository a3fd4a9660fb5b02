#include "layout.h"

#include <cstring>

namespace SimpleInfer {

DEFINE_LAYER_REGISTRY(Layout);

// A missing or mistyped key is kFail; values the rule does not allow are left for Validate, which knows the shape.
Status Layout::Init(const pnnx::Operator* op) {
    CHECK_STATUS(Layer::Init(op));
    own_ = LayoutOp();
    chain_.clear();
    final_ = Status::kFail;
    const std::string& t = op->type;
    if (t == "Tensor.permute" || t == "torch.permute") {
        own_.kind = LayoutOp::kPermute;
        CHECK_BOOL(Get(op, "dims", own_.args));
    } else if (t == "Tensor.reshape" || t == "Tensor.view") {
        own_.kind = LayoutOp::kReshape;
        if (op->inputs.size() > 1) return Status::kSuccess;   // (the shape as an operand: Validate refuses it with the reason)
        CHECK_BOOL(Get(op, "shape", own_.args));
    } else if (t == "torch.transpose") {
        own_.kind = LayoutOp::kTranspose;
        int dim0 = 0, dim1 = 0;
        CHECK_BOOL(Get(op, "dim0", dim0) && Get(op, "dim1", dim1));
        own_.args = {dim0, dim1};
    } else if (t == "torch.squeeze" || t == "torch.unsqueeze") {
        own_.kind = t == "torch.squeeze" ? LayoutOp::kSqueeze : LayoutOp::kUnsqueeze;
        int dim = 0;
        CHECK_BOOL(Get(op, "dim", dim));
        own_.args = {dim};
    } else {
        own_.kind = LayoutOp::kIdentity;   // Tensor.contiguous
    }
    return Status::kSuccess;
}

std::vector<int> Layout::FileShape(const Tensor& t) {
    std::vector<int> s = t.Shape();
    const size_t r = s.size();
    if (r > 3) {   // stored (.., H, W, C) -> file (.., C, H, W)
        const int c = s[r - 1];
        s[r - 1] = s[r - 2];
        s[r - 2] = s[r - 3];
        s[r - 3] = c;
    }
    return s;
}

// kSuccess with `final` kUnsupport: a refusal that fusing the operator into a chain may lift
Status Layout::PlanBound(const std::vector<LayoutOp>& ops, const Tensor& in, const Tensor& out, LayoutPlan& plan, Status& final,
                         std::string& why) const {
    const std::vector<int> is = FileShape(in), os = FileShape(out);
    const int ld = in.Shape().size() == 4 ? in.PixelStride() : 0;
    const Status s = PlanLayout(is, ld, ops, &os, plan, why);
    final = s;
    if (s == Status::kUnsupport && plan.late) return Status::kSuccess;
    return s;
}

Status Layout::Validate() {
    CHECK_STATUS(Layer::Validate());
    const std::string name = op_ ? op_->name : std::string("-");
    if (op_ && op_->inputs.size() > 1 && own_.kind == LayoutOp::kReshape) {
        LOG(ERROR) << "Layout::Validate fail [" << name << ": the shape of a " << op_->type << " is a second input operand; only shape= is served]";
        return Status::kUnsupport;
    }
    CHECK_STATUS(ValidateShape(1, 1));
    const Tensor& in = input_tensor_nodes_[0]->tensor;
    const Tensor& out = output_tensor_nodes_[0]->tensor;
    if (Status::kSuccess != ValidateFloat()) {
        LOG(ERROR) << "Layout::Validate fail [" << name << ": fp32 or fp16 operands only]";
        return Status::kUnsupport;
    }
    // re-batch: the engine has rewritten dim 0 of every operand that carried the file's batch; a leading shape= entry follows it
    bool rebatched = false;
    if (chain_.size() <= 1) {
        LayoutOp op = own_;
        if (op_ && op_->inputs.size() == 1 && op_->outputs.size() == 1) {
            const std::vector<int>& fi = op_->inputs[0]->shape;
            const std::vector<int>& fo = op_->outputs[0]->shape;
            int file_batch = 0, batch = 0;
            if (!fi.empty() && !in.Shape().empty() && fi[0] != in.Shape()[0]) file_batch = fi[0], batch = in.Shape()[0];
            if (!fo.empty() && !out.Shape().empty() && fo[0] != out.Shape()[0]) file_batch = fo[0], batch = out.Shape()[0];
            rebatched = file_batch > 0;
            if (rebatched && op.kind == LayoutOp::kReshape && !op.args.empty() && op.args[0] == file_batch) op.args[0] = batch;
        }
        chain_.assign(1, op);
    }
    const Status s = PlanBound(chain_, in, out, plan_, final_, final_why_);
    if (s == Status::kSuccess) return s;
    if (s == Status::kErrorShape && rebatched) {
        LOG(ERROR) << "Layout::Validate fail [" << name << ": " << final_why_ << "; the operator folds the batch into another dimension and is served "
                   << "at the file's batch only]";
        return Status::kUnsupport;
    }
    LOG(ERROR) << "Layout::Validate fail [" << name << ": " << final_why_ << "; input " << TupleString(FileShape(in)) << "]";
    return s;
}

bool Layout::TryChain(TensorNode* root, const std::vector<LayoutOp>& ops) {
    if (!root || output_tensor_nodes_.size() != 1) return false;
    LayoutPlan plan;
    Status final = Status::kFail;
    std::string why;
    if (PlanBound(ops, root->tensor, output_tensor_nodes_[0]->tensor, plan, final, why) != Status::kSuccess || final != Status::kSuccess) return false;
    SetInputNodes({root});
    chain_ = ops;
    plan_ = plan;
    final_ = final;
    final_why_.clear();
    return true;
}

Status Layout::Final() const {
    if (final_ != Status::kSuccess)
        LOG(ERROR) << "Layout [" << (op_ ? op_->name : std::string("-")) << "] cannot be served: " << final_why_;
    return final_;
}

// the launch for the tensors bound now: the plan's nest (re-planned when the input has another pixel stride than at Validate), dense output
bool Layout::Desc(const Tensor& in, const Tensor& out, SiPermuteDesc& d) const {
    if (final_ != Status::kSuccess) return false;
    if (out.Shape().empty() || out.PixelStride() != out.Shape().back()) return false;
    LayoutPlan plan = plan_;
    if (in.Shape().size() == 4 && in.PixelStride() != in.Shape().back()) {   // (planned dense at Validate)
        Status final = Status::kFail;
        std::string why;
        if (PlanBound(chain_, in, out, plan, final, why) != Status::kSuccess || final != Status::kSuccess) return false;
    }
    memset(&d, 0, sizeof(d));
    d.rank = (int)plan.dims.size();
    for (int k = 0; k < d.rank; ++k) {
        d.dims[k] = plan.dims[(size_t)k];
        d.in_stride[k] = plan.in_stride[(size_t)k];
    }
    if (d.rank == 0) {
        d.rank = 1;
        d.dims[0] = 1;
        d.in_stride[0] = 1;
    }
    d.out_ld = d.dims[d.rank - 1];
    d.form = SI_PERMUTE_FORM_AUTO;
    return true;
}

Status Layout::Forward(const Tensor& input, Tensor& output) {
    if (final_ != Status::kSuccess) return Final();
    return RunOnDevice({&input}, {&output}, [this](const std::vector<Tensor>& in, std::vector<Tensor>& out) {
        if (in[0].NumElements() != out[0].NumElements()) return Status::kErrorShape;
        if (IsHalf(in[0]) != IsHalf(out[0])) return Status::kUnsupport;
        // already in place: the engine pointed the output at the input's buffer (EngineImpl::AliasViews)
        if (plan_.view && in[0].RawData() && in[0].RawData() == out[0].RawData()) return Status::kSuccess;
        return LaunchDesc(si_hip_permute_f32, si_hip_permute_f16, "Layout", in[0], out[0], [this](auto&... a) { return Desc(a...); }, Status::kUnsupport);
    });
}

const char* Layout::KernelName() const {
    if (input_tensor_nodes_.size() != 1 || output_tensor_nodes_.size() != 1 || final_ != Status::kSuccess) return "permute";
    const Tensor& in = input_tensor_nodes_[0]->tensor;
    const Tensor& out = output_tensor_nodes_[0]->tensor;
    if (plan_.view && in.RawData() && in.RawData() == out.RawData()) return "view";
    SiPermuteDesc d;
    if (!Desc(in, out, d)) return "permute";
    return si_hip_permute_kernel_name(&d, in.RawData(), out.RawData(), IsHalf(in) ? 1 : 0);
}

}  // namespace SimpleInfer
