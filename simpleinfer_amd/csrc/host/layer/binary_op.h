// layer/binary_op.h -- BinaryOp emitted by pnnx::expand_expression, with broadcast by integer factors (reference
// src/layer/binary_op.cpp:11-32, :52-94).  The reference layer has add (code 0) and mul (code 2) only and no scalar form;
// here every code the lowering can emit runs.
#pragma once

#include "layer.h"
#include "layer_util.h"
#include "si_binary.h"
#include "view_rule.h"

namespace SimpleInfer {

class BinaryOp : public Layer {
public:
    virtual Status Init(const pnnx::Operator* op) override;
    virtual void SetInputNodes(const std::vector<TensorNode*>& input_tensor_nodes) override;   // marks the constant form
    virtual Status Validate() override;
    virtual Status Forward() override;
    virtual Status Forward(const std::vector<Tensor>& inputs, Tensor& output) override;
    virtual Status Forward(const Tensor& input, Tensor& output) override;  // the `with_scalar` form: one tensor operand
    virtual bool HalfStorageOk(std::string& why) const override;
    virtual bool TakesView(const TensorNode* node, int ld, int off) const override;
    virtual const char* KernelName() const override;

    // ---- the constant form: exactly one operand is a graph constant (a pnnx.Attribute's output) and the other has the output's shape.  It runs
    // on the constant-operand kernel (include/si_binary.h), in fp32 and under fp16 storage, for all ten codes
    bool ConstForm() const { return const_index_ >= 0 && const_image_ != nullptr; }
    int Stages() const { return stage2_ ? 2 : 1; }
    // `next` is a one-stage constant form that reads `mid`, this layer's output, as its tensor operand, with the same shape and storage type
    bool CanAbsorb(const BinaryOp& next, const TensorNode* mid) const;
    void Absorb(BinaryOp& next) { stage2_ = &next; }   // (the engine then hands this layer next's output node)

public:
    // param "0" as pnnx's expression lowering writes it (reference src/pnnx/expand_expression.cpp:198-216).  The reference layer
    // accepts kAdd and kMul only (src/layer/binary_op.cpp:17-31); the rest is what `x - y`, `x / 2.0`, `2.0 - x`, `x ** 0.5` in an
    // exported model lower to.
    enum class BinaryOpType { kAdd = 0, kSub = 1, kMul = 2, kDiv = 3, kPow = 6, kRSub = 7, kRDiv = 8, kRPow = 9, kAtan2 = 10, kRAtan2 = 11 }
        binary_op_type_ = BinaryOpType::kAdd;
    bool with_scalar_ = false;   // params "1" (expand_expression.cpp:206-236): the other operand is the literal in "2"
    float scalar_ = 0.0f;

private:
    Status RunConst(const Tensor& x, const Tensor& out) const;
    bool MakeConstDesc(const Tensor& x, const Tensor& out, SiBinaryDesc& d) const;
    int const_index_ = -1;                 // which of the two inputs is the constant (-1: none, or both)
    const Tensor* const_image_ = nullptr;  // the constant as stored for the other operand's rank: the node's own tensor, or one of its promoted images
    bool const_rank_refused_ = false;      // the promoted rank would be above 4
    bool const_rank_mismatch_ = false;     // a constant of another rank than its partner that the constant form cannot take
    BinaryOp* stage2_ = nullptr;           // the absorbed second stage (FuseConstStages)
};

// broadcast result shape of two same-rank shapes (reference src/layer/binary_op.cpp:96-126)
Status BroadcastShape(const std::vector<int>& shape0, const std::vector<int>& shape1, std::vector<int>& broadcast_shape);

}  // namespace SimpleInfer
