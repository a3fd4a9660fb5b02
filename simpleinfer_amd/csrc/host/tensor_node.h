// tensor_node.h -- graph operand + the tensor bound to it (reference src/tensor_node.h:9-12)
#pragma once

#include <map>

#include "pnnx/ir.h"
#include "tensor.h"

namespace SimpleInfer {

struct TensorNode {
    pnnx::Operand* operand = nullptr;
    Tensor tensor;
    // a graph constant: the output of a pnnx.Attribute operator.  Its buffer lies outside the arena, is filled once at LoadModel from the
    // operator's `data` and is never written; it has no layer and no step.  `tensor` is the file shape under the storage rule of its rank.
    bool constant = false;
    // ... and the further stored images a consumer asked for (BinaryOp pairing it with an operand of higher rank): the file shape left-padded
    // with 1s to the rank of the key, then the storage rule of THAT rank -- [C,1,1] against [N,C,H,W] is [1,C,1,1], stored [1,1,1,C]
    std::map<int, Tensor> promoted;
};

}  // namespace SimpleInfer
