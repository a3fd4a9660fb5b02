#include "binary_op.h"

#include "layer_util.h"

#include "si_binary.h"
#include "si_hip.h"

namespace SimpleInfer {

DEFINE_LAYER_REGISTRY(BinaryOp);

Status BinaryOp::Init(const pnnx::Operator* op) {
    CHECK_STATUS(Layer::Init(op));
    int code = 0, scalar_form = 0;
    CHECK_BOOL(Get(op, "0", code));
    switch (code) {
        case 0: case 1: case 2: case 3: case 6: case 7: case 8: case 9: case 10: case 11:
            binary_op_type_ = static_cast<BinaryOpType>(code);
            break;
        default:  // 4 / 5 (max / min) are never emitted by expand_expression
            LOG(ERROR) << "unsupport BinaryOp type [" << code << "]";
            return Status::kUnsupport;
    }
    with_scalar_ = false;
    if (Get(op, "1", scalar_form) && scalar_form != 0) {
        // scalar operand form (expand_expression.cpp:206-236): "1" = with_scalar, "2" = the literal as a float
        CHECK_BOOL(Get(op, "2", scalar_));
        with_scalar_ = true;
    }
    return Status::kSuccess;
}

// The constant form is marked here, when the engine binds the operands: exactly one of the two is a graph constant.  torch right-aligns shapes
// in FILE order, so a constant of lower rank is left-padded with 1s to its partner's rank in file order before the storage rule applies -- the
// node keeps one stored image per rank asked for (tensor_node.h), which the engine fills at LoadModel.
void BinaryOp::SetInputNodes(const std::vector<TensorNode*>& nodes) {
    Layer::SetInputNodes(nodes);
    const_index_ = -1;
    const_image_ = nullptr;
    const_rank_refused_ = const_rank_mismatch_ = false;
    if (with_scalar_ || nodes.size() != 2 || !nodes[0] || !nodes[1]) return;
    // (an fp32 shadow of a constant -- the engine's fallback under fp16 storage -- is an ordinary tensor of the constant's own rank)
    auto from_attribute = [](const TensorNode* n) { return n->operand && n->operand->producer && n->operand->producer->type == "pnnx.Attribute"; };
    const size_t r0 = nodes[0]->tensor.Shape().size(), r1 = nodes[1]->tensor.Shape().size();
    if (nodes[0]->constant == nodes[1]->constant) {
        const_rank_mismatch_ = r0 != r1 && (from_attribute(nodes[0]) || from_attribute(nodes[1]));
        return;
    }
    const int ci = nodes[0]->constant ? 0 : 1;
    TensorNode* c = nodes[ci];
    const size_t rank = ci == 0 ? r1 : r0, crank = ci == 0 ? r0 : r1;
    if (crank > rank) {
        const_rank_mismatch_ = true;   // the constant would promote the tensor: not the constant form, and today's kernels pair equal ranks only
        return;
    }
    const_index_ = ci;
    if (crank == rank) {
        const_image_ = &c->tensor;
        return;
    }
    if (rank > 4) {
        const_rank_refused_ = true;
        return;
    }
    auto it = c->promoted.find((int)rank);
    if (it == c->promoted.end()) {
        std::vector<int> file(rank - crank, 1);
        file.insert(file.end(), c->operand->shape.begin(), c->operand->shape.end());
        std::vector<int> stored = file;
        if (rank > 3) {
            stored[rank - 3] = file[rank - 2];
            stored[rank - 2] = file[rank - 1];
            stored[rank - 1] = file[rank - 3];
        }
        it = c->promoted.emplace((int)rank, Tensor(c->tensor.GetDataType(), stored, MemoryType::kDevice, false)).first;
    }
    const_image_ = &it->second;
}

Status BinaryOp::Validate() {
    CHECK_STATUS(Layer::Validate());
    CHECK_STATUS(ValidateShape(with_scalar_ ? 1 : 2, 1));
    const std::string name = op_ ? op_->name : std::string("-");
    if (const_rank_refused_) {
        LOG(ERROR) << "BinaryOp [" << name << "]: a constant against an operand of rank above 4 is not served";
        return Status::kUnsupport;
    }
    if (const_rank_mismatch_) {
        LOG(ERROR) << "BinaryOp [" << name << "]: a constant and an operand of different ranks are served only where the other operand has the result's shape and storage type";
        return Status::kUnsupport;
    }
    if (const_index_ >= 0) {
        // the constant form needs the other operand to be the whole result; a constant that broadcasts the TENSOR is an ordinary operand of
        // today's kernels, which pair equal ranks only
        SiBinaryDesc d;
        const Tensor& x = input_tensor_nodes_[1 - const_index_]->tensor;
        if (!MakeConstDesc(x, output_tensor_nodes_[0]->tensor, d)) {
            if (const_image_ != &input_tensor_nodes_[const_index_]->tensor) {
                LOG(ERROR) << "BinaryOp [" << name << "]: a constant of lower rank whose partner is not the whole result is not served";
                return Status::kUnsupport;
            }
            const_index_ = -1;
            const_image_ = nullptr;
        }
    }
    return Status::kSuccess;
}

// x and out of one shape, the constant's stored image broadcastable to it: the descriptor of one stage (the second is added by RunConst)
bool BinaryOp::MakeConstDesc(const Tensor& x, const Tensor& out, SiBinaryDesc& d) const {
    if (!const_image_ || x.Shape() != out.Shape() || x.Shape().size() != const_image_->Shape().size() || x.Shape().size() > 4 || x.Shape().empty()) return false;
    const std::vector<int> xs = x.ShapeAs(4), cs = const_image_->ShapeAs(4);
    d = SiBinaryDesc();
    int run = 1;
    for (int i = 3; i >= 0; --i) {
        if (xs[i] <= 0 || (cs[i] != xs[i] && cs[i] != 1)) return false;
        d.d[i] = xs[i];
        d.c0_stride[i] = cs[i] == 1 ? 0 : run;
        run *= cs[i];
    }
    d.x_ld = x.PixelStride();
    d.out_ld = out.PixelStride();
    d.stages = 1;
    const int code = (int)binary_op_type_;
    // the constant on the left: the operand-reversed code (add and mul commute exactly)
    static const int reversed[12] = {0, 7, 2, 8, 4, 5, 9, 1, 3, 6, 11, 10};
    d.op[0] = const_index_ == 0 ? reversed[code] : code;
    return true;
}

bool BinaryOp::CanAbsorb(const BinaryOp& next, const TensorNode* mid) const {
    if (!ConstForm() || !next.ConstForm() || stage2_ || next.stage2_ || &next == this) return false;
    if (next.input_tensor_nodes_.size() != 2 || next.input_tensor_nodes_[1 - next.const_index_] != mid || output_tensor_nodes_.size() != 1 ||
        output_tensor_nodes_[0] != mid || next.output_tensor_nodes_.size() != 1)
        return false;
    const Tensor& x = input_tensor_nodes_[1 - const_index_]->tensor;
    const Tensor& out = next.output_tensor_nodes_[0]->tensor;
    SiBinaryDesc d;
    return x.Shape() == mid->tensor.Shape() && out.Shape() == mid->tensor.Shape() && x.GetDataType() == mid->tensor.GetDataType() &&
           out.GetDataType() == mid->tensor.GetDataType() && const_image_->GetDataType() == next.const_image_->GetDataType() &&
           next.MakeConstDesc(mid->tensor, out, d);
}

Status BinaryOp::RunConst(const Tensor& x, const Tensor& out) const {
    SiBinaryDesc d;
    if (!MakeConstDesc(x, out, d)) return Status::kErrorShape;
    const void* c1 = nullptr;
    if (stage2_) {
        SiBinaryDesc d2;
        if (!stage2_->MakeConstDesc(x, out, d2)) return Status::kErrorShape;
        d.stages = 2;
        d.op[1] = d2.op[0];
        for (int i = 0; i < 4; ++i) d.c1_stride[i] = d2.c0_stride[i];
        c1 = stage2_->const_image_->RawData();
        if (stage2_->const_image_->GetDataType() != const_image_->GetDataType()) return Status::kUnsupport;
    }
    const bool half = IsHalf(x);
    if (IsHalf(out) != half || IsHalf(*const_image_) != half) return Status::kUnsupport;
    const int rc = half ? si_hip_binary_const_f16(&d, x.RawData(), const_image_->RawData(), c1, out.RawData(), Stream())
                        : si_hip_binary_const_f32(&d, x.Data<float>(), static_cast<const float*>(const_image_->RawData()),
                                                  static_cast<const float*>(c1), out.Data<float>(), Stream());
    return CheckHip(rc, "BinaryOp (constant)");
}

Status BinaryOp::Forward() {
    if (!ConstForm()) return Layer::Forward();
    LOG(INFO) << "Forward Layer [" << (op_ ? op_->name : std::string("?")) << "]";
    return RunConst(input_tensor_nodes_[1 - const_index_]->tensor, output_tensor_nodes_[0]->tensor);
}

const char* BinaryOp::KernelName() const {
    if (with_scalar_) return "binary_scalar";
    if (!ConstForm() || input_tensor_nodes_.size() != 2 || output_tensor_nodes_.empty()) return "binary";
    const Tensor& x = input_tensor_nodes_[1 - const_index_]->tensor;
    const Tensor& out = output_tensor_nodes_[0]->tensor;
    SiBinaryDesc d;
    if (!MakeConstDesc(x, out, d) || !x.RawData() || !out.RawData() || !const_image_->RawData()) return stage2_ ? "binary_const x2" : "binary_const";
    if (stage2_) {
        SiBinaryDesc d2;
        if (!stage2_->MakeConstDesc(x, out, d2) || !stage2_->const_image_->RawData()) return "binary_const x2";
        d.stages = 2;
        d.op[1] = d2.op[0];
        for (int i = 0; i < 4; ++i) d.c1_stride[i] = d2.c0_stride[i];
    }
    return si_hip_binary_const_kernel_name(&d, x.RawData(), const_image_->RawData(), stage2_ ? stage2_->const_image_->RawData() : nullptr, out.RawData(),
                                           IsHalf(x) ? 1 : 0);
}

Status BinaryOp::Forward(const Tensor& input, Tensor& output) {
    if (!with_scalar_) return Status::kErrorShape;
    return RunOnDevice({&input}, {&output}, [this](const std::vector<Tensor>& in, std::vector<Tensor>& out) {
        if (IsHalf(in[0]) || IsHalf(out[0])) return Status::kUnsupport;  // fp16 storage: not built for this operator
        size_t pixels = 0, opix = 0;
        int c = 0, oc = 0;
        if (!GetPixelsChannels(in[0], pixels, c) || !GetPixelsChannels(out[0], opix, oc) || pixels != opix || c != oc) return Status::kErrorShape;
        return CheckHip(si_hip_binary_scalar_f32((int)binary_op_type_, in[0].Data<float>(), pixels, c, in[0].PixelStride(), scalar_,
                                                 out[0].Data<float>(), out[0].PixelStride(), Stream()),
                        "BinaryOp (scalar)");
    });
}

Status BinaryOp::Forward(const std::vector<Tensor>& inputs, Tensor& output) {
    if (inputs.size() != 2) return Status::kErrorShape;
    return RunOnDevice({&inputs[0], &inputs[1]}, {&output}, [this](const std::vector<Tensor>& in, std::vector<Tensor>& out) {
        const std::vector<int> a = in[0].ShapeAs(4), b = in[1].ShapeAs(4), o = out[0].ShapeAs(4);
        for (int i = 0; i < 4; ++i)
            if (a[i] <= 0 || b[i] <= 0 || o[i] % a[i] != 0 || o[i] % b[i] != 0) return Status::kErrorShape;
        if (IsHalf(in[0]) || IsHalf(in[1]) || IsHalf(out[0])) {
            // fp16 path: add / mul of same-shape tensors (residual blocks) or with one operand broadcast over H and W (the
            // squeeze-excite scale [N,1,1,C] x [N,H,W,C])
            if (!(IsHalf(in[0]) && IsHalf(in[1]) && IsHalf(out[0]))) return Status::kUnsupport;
            if (binary_op_type_ != BinaryOpType::kAdd && binary_op_type_ != BinaryOpType::kMul) return Status::kUnsupport;
            auto per_image_vector = [&](const std::vector<int>& s) { return s[0] == o[0] && s[1] == 1 && s[2] == 1 && s[3] == o[3]; };
            if (a == o && per_image_vector(b) && b != o)
                return CheckHip(si_hip_binary_bcast_f16((int)binary_op_type_, in[0].RawData(), in[0].PixelStride(), in[1].RawData(), in[1].PixelStride(),
                                                        out[0].RawData(), out[0].PixelStride(), o[0], (size_t)o[1] * o[2], o[3], Stream()),
                                "BinaryOp (broadcast)");
            if (b == o && per_image_vector(a) && a != o)   // add and mul commute
                return CheckHip(si_hip_binary_bcast_f16((int)binary_op_type_, in[1].RawData(), in[1].PixelStride(), in[0].RawData(), in[0].PixelStride(),
                                                        out[0].RawData(), out[0].PixelStride(), o[0], (size_t)o[1] * o[2], o[3], Stream()),
                                "BinaryOp (broadcast)");
            if (a != o || b != o) return Status::kUnsupport;
            return CheckHip(si_hip_binary_same_f16((int)binary_op_type_, in[0].RawData(), in[0].PixelStride(), in[1].RawData(),
                                                   in[1].PixelStride(), out[0].RawData(), out[0].PixelStride(),
                                                   (size_t)o[0] * o[1] * o[2], o[3], Stream()),
                            "BinaryOp");
        }
        return CheckHip(si_hip_binary_f32((int)binary_op_type_, in[0].Data<float>(), a.data(), in[0].PixelStride(),
                                          in[1].Data<float>(), b.data(), in[1].PixelStride(), out[0].Data<float>(),
                                          o.data(), out[0].PixelStride(), Stream()),
                        "BinaryOp");
    });
}

// reference src/layer/binary_op.cpp:96-126
Status BroadcastShape(const std::vector<int>& s0, const std::vector<int>& s1, std::vector<int>& out) {
    if (s0.size() != s1.size()) {
        LOG(ERROR) << "BroadcastShape: different shape size [" << s0.size() << "][" << s1.size() << "]";
        return Status::kUnsupport;
    }
    out.resize(s0.size());
    for (size_t i = 0; i < s0.size(); ++i) {
        if (s0[i] == s1[i] || 1 == s1[i]) {
            out[i] = s0[i];
        } else if (1 == s0[i]) {
            out[i] = s1[i];
        } else {
            LOG(ERROR) << "BroadcastShape: different dim size [" << s0[i] << "][" << s1[i] << "] at dimension [" << i << "]";
            return Status::kUnsupport;
        }
    }
    return Status::kSuccess;
}

bool BinaryOp::HalfStorageOk(std::string& why) const {
    bool any = false, all = true;
    for (auto* n : input_tensor_nodes_) { any = any || IsHalf(n->tensor); all = all && IsHalf(n->tensor); }
    for (auto* n : output_tensor_nodes_) { any = any || IsHalf(n->tensor); all = all && IsHalf(n->tensor); }
    if (!any) return true;
    // the constant form: every code, when the tensor, the constant's image and the result are all half
    if (ConstForm() && all && IsHalf(*const_image_) && (!stage2_ || IsHalf(*stage2_->const_image_))) return true;
    const bool addmul = binary_op_type_ == BinaryOpType::kAdd || binary_op_type_ == BinaryOpType::kMul;
    bool same = !with_scalar_ && input_tensor_nodes_.size() == 2 && output_tensor_nodes_.size() == 1;
    if (same) {
        const std::vector<int>& o = output_tensor_nodes_[0]->tensor.Shape();
        same = input_tensor_nodes_[0]->tensor.Shape() == o && input_tensor_nodes_[1]->tensor.Shape() == o;
    }
    if (all && addmul && same) return true;
    if (all && addmul && !with_scalar_ && input_tensor_nodes_.size() == 2 && output_tensor_nodes_.size() == 1) {
        // one operand a per-image channel vector [N,1,1,C] (squeeze-excite), channels a multiple of 8
        const std::vector<int> a = input_tensor_nodes_[0]->tensor.ShapeAs(4), b = input_tensor_nodes_[1]->tensor.ShapeAs(4);
        const std::vector<int> o = output_tensor_nodes_[0]->tensor.ShapeAs(4);
        auto vec = [&](const std::vector<int>& s) { return s[0] == o[0] && s[1] == 1 && s[2] == 1 && s[3] == o[3]; };
        if (o[3] % 8 == 0 && ((a == o && vec(b)) || (b == o && vec(a)))) return true;
    }
    why = "BinaryOp has fp16 kernels for add / mul of same-shape tensors or with a per-image channel vector only (no scalar form, no sub / div / pow)";
    return false;
}

// The per-image channel vector form under fp16 storage (si_hip_binary_bcast_f16) reads and writes 16-byte vectors only and there is no scalar
// form behind it: its three operands keep rows of whole vectors.  The same-shape and constant forms step by ld element by element.
bool BinaryOp::TakesView(const TensorNode* node, int ld, int off) const {
    if (!node || !IsHalf(node->tensor) || ConstForm() || with_scalar_ || input_tensor_nodes_.size() != 2 || output_tensor_nodes_.size() != 1) return true;
    const TensorNode* const nodes[3] = {input_tensor_nodes_[0], input_tensor_nodes_[1], output_tensor_nodes_[0]};
    if (node != nodes[0] && node != nodes[1] && node != nodes[2]) return true;
    const std::vector<int> o = nodes[2]->tensor.ShapeAs(4);
    if (nodes[0]->tensor.ShapeAs(4) == o && nodes[1]->tensor.ShapeAs(4) == o) return true;   // the same-shape form
    return HalfBroadcastTakesView(ld, off);
}

}  // namespace SimpleInfer
