// batch_rule.h -- is an operator per-image?  The engine cuts a batch into contiguous slabs in three places (option "host_slices", option
// "streams", ShardedEngine) and runs every slab through the same model re-batched to N / G.  That computes what the whole batch computes only
// when no operator of the graph combines images: a softmax over dimension 0, a mean over the batch that is broadcast back, a slice or a
// concatenation along the batch, a view that folds the batch into the channels all load and run at N / G -- and give other numbers.
// The rule below names those operators; every operator type it has no row for counts as batch-mixing, so a type added to the registry is
// served unsplit until it gets one.
//
// Pure: ir.h and param_read.h only, so it is tested without a device (tests/cpp/test_batch_rule.cpp).  Shapes are file-order (NCHW) shapes.
#ifndef SIMPLE_INFER_SRC_BATCH_RULE_H_
#define SIMPLE_INFER_SRC_BATCH_RULE_H_

#include <map>
#include <set>
#include <string>
#include <vector>

#include "pnnx/param_read.h"

namespace SimpleInfer {

// The dimension of `out` that carries the batch when dimension `axis` of the operator's input `in` does (file-order shapes; -1: not known).
// permute / transpose move it by their arguments; for everything else -- reshapes, flatten, and every operator that keeps the leading
// dimensions -- it is the dimension of `out` that holds the traced batch behind the same number of leading elements.
inline int FollowBatchAxis(const pnnx::Operator* op, const std::vector<int>& in, int axis, const std::vector<int>& out, int file_batch) {
    const int ir = (int)in.size(), orank = (int)out.size();
    if (axis < 0 || axis >= ir || in[axis] != file_batch) return -1;
    auto at = [&](int j) { return j >= 0 && j < orank && out[j] == file_batch ? j : -1; };
    auto norm = [&](int d) { return d < 0 ? d + ir : d; };
    if (op->type == "Tensor.permute" || op->type == "torch.permute") {
        std::vector<int> dims;
        if (!Get(op, "dims", dims)) return -1;
        for (int j = 0; j < (int)dims.size(); ++j)
            if (norm(dims[j]) == axis) return at(j);
        return -1;
    }
    if (op->type == "torch.transpose") {
        int d0 = 0, d1 = 0;
        if (!Get(op, "dim0", d0) || !Get(op, "dim1", d1)) return -1;
        d0 = norm(d0); d1 = norm(d1);
        return at(axis == d0 ? d1 : axis == d1 ? d0 : axis);
    }
    long long lead = 1, seen = 1;
    for (int k = 0; k < axis; ++k) lead *= in[k];
    for (int j = 0; j < orank; ++j) {
        if (seen == lead && out[j] == file_batch) return j;
        seen *= out[j];
        if (seen > lead) break;
    }
    return -1;
}

// Graph constants: the output of a pnnx.Attribute operator (a tensor stored in the file), and every output of an operator whose inputs are all
// constants.  A constant is no image of the batch whatever its dimension 0 says: it is never re-batched and never cut into slabs.
inline bool IsAttributeOp(const pnnx::Operator* op) { return op->type == "pnnx.Attribute"; }

inline std::set<const pnnx::Operand*> ConstantOperands(const std::vector<pnnx::Operator*>& ops) {
    std::set<const pnnx::Operand*> constants;
    for (const pnnx::Operator* op : ops) {
        bool all = IsAttributeOp(op);
        if (!all && !op->inputs.empty()) {
            all = true;
            for (const pnnx::Operand* in : op->inputs) all = all && constants.count(in) > 0;
        }
        if (all)
            for (const pnnx::Operand* out : op->outputs) constants.insert(out);
    }
    return constants;
}

// The batch dimension of every operand, followed from the graph inputs (dimension 0 where it holds `file_batch`) through the operators in
// file order; -1: the operand does not carry the batch, or where it does is not known.  A constant (ConstantOperands) has
// -1 even when its dimension 0 equals the traced batch.
inline std::map<const pnnx::Operand*, int> FollowBatchAxes(const std::vector<pnnx::Operator*>& ops, int file_batch) {
    std::map<const pnnx::Operand*, int> batch_axis;
    for (const pnnx::Operator* op : ops) {
        const pnnx::Operand* src = nullptr;
        int axis = -1;
        for (const pnnx::Operand* in : op->inputs) {
            auto it = batch_axis.find(in);
            if (it != batch_axis.end() && it->second >= 0) { src = in; axis = it->second; break; }
        }
        const bool recurrent = op->type == "nn.LSTM" || op->type == "nn.GRU";
        for (const pnnx::Operand* out : op->outputs) {
            if (IsAttributeOp(op)) batch_axis[out] = -1;
            else if (op->inputs.empty()) batch_axis[out] = (!out->shape.empty() && out->shape[0] == file_batch) ? 0 : -1;
            else if (recurrent && src) {
                // y keeps the input's batch dimension; the state outputs [layers * dirs, N, H] carry it in dimension 1 whatever batch_first says
                const int to = out == op->outputs[0] ? axis : 1;
                batch_axis[out] = (out->shape.size() == 3 && to < 3 && out->shape[to] == file_batch) ? to : -1;
            } else batch_axis[out] = src ? FollowBatchAxis(op, src->shape, axis, out->shape, file_batch) : -1;
        }
    }
    return batch_axis;
}

// the batch the file was traced with: dimension 0 of the graph inputs (0: none, or they disagree); a pnnx.Attribute is no graph input
inline int FileBatch(const std::vector<pnnx::Operator*>& ops) {
    int file_batch = 0;
    for (const pnnx::Operator* op : ops) {
        if (!op->inputs.empty() || IsAttributeOp(op)) continue;
        for (const pnnx::Operand* out : op->outputs) {
            if (out->shape.empty() || out->shape[0] <= 0 || (file_batch != 0 && file_batch != out->shape[0])) return 0;
            file_batch = out->shape[0];
        }
    }
    return file_batch;
}

// ---- the rule -------------------------------------------------------------------------------------------------------------------------
// How an operator type treats the batch.  One row per type string of layer_registry.cpp, plus the graph's own pnnx.Input / pnnx.Output.
enum class BatchFamily {
    kUnknown,       // no row: not per-image
    kInput,         // pnnx.Input
    kOutput,        // pnnx.Output: a slab of the batch is a slab of the buffer only when the batch is dimension 0
    kSpatial,       // [N, C, H, W] (or [N, C, L], [N, F]) in and out, computed image by image: the batch must be dimension 0
    kElementwise,   // value by value: any batch dimension, the same one in and out
    kRows,          // over the last dimension (nn.Linear): any batch dimension but the last
    kSoftmax,       // along dim
    kReduce,        // over dim
    kSlice,         // pieces along dim(s)
    kCat,           // along dim
    kBinary,        // broadcasting arithmetic
    kMove,          // permute / transpose: moves the batch dimension, combines nothing
    kReshape,       // reshape / view / flatten / squeeze / unsqueeze / contiguous: per-image while the batch stays a dimension of its own
    kAttention,     // nn.MultiheadAttention: reads the batch from dimension 0 (batch_first) or 1
    kRoi,           // torchvision.ops.RoIAlign / roi_align: boxes [K, 5] that name their image by an index in the data -- never per-image
    kConstant,      // pnnx.Attribute: a tensor of the file, the same for every image -- always per-image
    kRecurrent,     // nn.LSTM / nn.GRU: reads the batch from dimension 0 (batch_first) or 1; y keeps it there, the state outputs carry it in 1
    kXcorr,         // F.conv2d: kSpatial on x while the filter (and bias) are graph constants; with a filter computed from a graph input never per-image
};

// why an operator of the family kRoi is never per-image (also the engine's reason for refusing to re-batch a graph that holds one)
inline const char* RoiBatchReason() {
    return "the boxes name their image by an index in the data: dimension 0 of the output counts boxes, not images";
}

// why F.conv2d with a filter computed from a graph input is never per-image (also the engine's reason for refusing to re-batch such a graph)
inline const char* XcorrBatchReason() {
    return "the filter is computed from a graph input: its dimension 0 counts filters, not images, and every image of x meets every filter";
}

// F.conv2d (kXcorr) whose filter, or bias, is no graph constant; `constants`: ConstantOperands of the graph
inline bool HasTensorFilter(const pnnx::Operator* op, const std::set<const pnnx::Operand*>& constants) {
    if (op->type != "F.conv2d") return false;
    for (size_t i = 1; i < op->inputs.size(); ++i)
        if (!constants.count(op->inputs[i])) return true;
    return op->inputs.size() < 2;
}

inline BatchFamily BatchFamilyOf(const std::string& type) {
    static const std::map<std::string, BatchFamily> table = {
        {"pnnx.Input", BatchFamily::kInput},
        {"pnnx.Output", BatchFamily::kOutput},
        {"pnnx.Attribute", BatchFamily::kConstant},
        {"nn.Conv2d", BatchFamily::kSpatial},
        {"nn.ConvTranspose2d", BatchFamily::kSpatial},
        {"nn.Conv1d", BatchFamily::kSpatial},            // ([N, C, L] in and out, computed item by item: the batch must be dimension 0)
        {"F.conv2d", BatchFamily::kXcorr},               // (x image by image against a CONSTANT filter; a tensor filter is never per-image)
        {"torchvision.ops.DeformConv2d", BatchFamily::kSpatial},   // (offset and mask are per-pixel operands of the same image)
        {"F.grid_sample", BatchFamily::kSpatial},        // (x [N,C,H,W] and the grid [N,Ho,Wo,2] are operands of the same image)
        {"F.affine_grid", BatchFamily::kSpatial},        // (theta [N,2,3] -> grid [N,H,W,2]: the batch is dimension 0 on both sides)
        {"nn.BatchNorm2d", BatchFamily::kSpatial},       // (inference: running statistics, nothing of the batch)
        {"nn.GroupNorm", BatchFamily::kSpatial},
        {"nn.InstanceNorm2d", BatchFamily::kSpatial},
        {"nn.CircularPad2d", BatchFamily::kSpatial},
        {"nn.ConstantPad2d", BatchFamily::kSpatial},
        {"nn.ReflectionPad2d", BatchFamily::kSpatial},
        {"nn.ReplicationPad2d", BatchFamily::kSpatial},
        {"nn.ZeroPad2d", BatchFamily::kSpatial},
        {"F.pad", BatchFamily::kSpatial},
        {"nn.MaxPool2d", BatchFamily::kSpatial},
        {"nn.AvgPool2d", BatchFamily::kSpatial},
        {"F.avg_pool2d", BatchFamily::kSpatial},
        {"nn.AdaptiveAvgPool2d", BatchFamily::kSpatial},
        {"F.adaptive_avg_pool2d", BatchFamily::kSpatial},
        {"nn.Upsample", BatchFamily::kSpatial},
        {"F.interpolate", BatchFamily::kSpatial},
        {"F.upsample", BatchFamily::kSpatial},
        {"nn.PixelShuffle", BatchFamily::kSpatial},
        {"nn.PixelUnshuffle", BatchFamily::kSpatial},
        {"F.pixel_shuffle", BatchFamily::kSpatial},
        {"F.pixel_unshuffle", BatchFamily::kSpatial},
        {"nn.PReLU", BatchFamily::kSpatial},              // (a slope per channel: dimension 1 must not be the batch)
        {"models.yolo.Detect", BatchFamily::kSpatial},
        {"nn.ReLU", BatchFamily::kElementwise},
        {"F.relu", BatchFamily::kElementwise},
        {"nn.SiLU", BatchFamily::kElementwise},
        {"F.silu", BatchFamily::kElementwise},
        {"nn.Sigmoid", BatchFamily::kElementwise},
        {"F.sigmoid", BatchFamily::kElementwise},
        {"nn.Hardsigmoid", BatchFamily::kElementwise},
        {"F.hardsigmoid", BatchFamily::kElementwise},
        {"nn.Hardswish", BatchFamily::kElementwise},
        {"F.hardswish", BatchFamily::kElementwise},
        {"nn.LeakyReLU", BatchFamily::kElementwise},
        {"F.leaky_relu", BatchFamily::kElementwise},
        {"nn.Tanh", BatchFamily::kElementwise},
        {"F.tanh", BatchFamily::kElementwise},
        {"nn.ReLU6", BatchFamily::kElementwise},
        {"F.relu6", BatchFamily::kElementwise},
        {"nn.Hardtanh", BatchFamily::kElementwise},
        {"F.hardtanh", BatchFamily::kElementwise},
        {"torch.clamp", BatchFamily::kElementwise},
        {"nn.Softplus", BatchFamily::kElementwise},
        {"F.softplus", BatchFamily::kElementwise},
        {"nn.Mish", BatchFamily::kElementwise},
        {"F.mish", BatchFamily::kElementwise},
        {"UnaryOp", BatchFamily::kElementwise},
        {"nn.Linear", BatchFamily::kRows},
        {"nn.Softmax", BatchFamily::kSoftmax},
        {"nn.LogSoftmax", BatchFamily::kSoftmax},
        {"nn.Softmax2d", BatchFamily::kSoftmax},
        {"F.softmax", BatchFamily::kSoftmax},
        {"F.log_softmax", BatchFamily::kSoftmax},
        {"F.normalize", BatchFamily::kSoftmax},          // (x / max(norm, eps) along dim: per-image unless dim is the batch)
        {"torch.mean", BatchFamily::kReduce},
        {"torch.sum", BatchFamily::kReduce},
        {"torch.amax", BatchFamily::kReduce},
        {"torch.amin", BatchFamily::kReduce},
        {"torch.norm", BatchFamily::kReduce},            // (the Lp norm over dim: per-image unless a reduced dim is the batch)
        {"torch.chunk", BatchFamily::kSlice},
        {"torch.split", BatchFamily::kSlice},
        {"Tensor.slice", BatchFamily::kSlice},
        {"torch.cat", BatchFamily::kCat},
        {"BinaryOp", BatchFamily::kBinary},
        {"Tensor.permute", BatchFamily::kMove},
        {"torch.permute", BatchFamily::kMove},
        {"torch.transpose", BatchFamily::kMove},
        {"Tensor.reshape", BatchFamily::kReshape},
        {"Tensor.view", BatchFamily::kReshape},
        {"torch.flatten", BatchFamily::kReshape},
        {"torch.squeeze", BatchFamily::kReshape},
        {"torch.unsqueeze", BatchFamily::kReshape},
        {"Tensor.contiguous", BatchFamily::kReshape},
        {"nn.MultiheadAttention", BatchFamily::kAttention},
        {"torchvision.ops.RoIAlign", BatchFamily::kRoi},
        {"torchvision.ops.roi_align", BatchFamily::kRoi},
        {"nn.LSTM", BatchFamily::kRecurrent},
        {"nn.GRU", BatchFamily::kRecurrent},
    };
    auto it = table.find(type);
    return it == table.end() ? BatchFamily::kUnknown : it->second;
}

// an operand as the rule sees it: its file-order shape and the dimension that carries the batch (-1: none, or not known)
struct BatchOperand {
    std::vector<int> shape;
    int axis = -1;
    bool constant = false;   // a graph constant (ConstantOperands): broadcast over the images by design, its axis is -1
};

// Is `op` per-image: does image i of every output depend on image i of the inputs alone, so that the operator re-batched to a slab of the
// batch computes that slab of its outputs?  `in` / `out`: the operator's operands in order; `batch`: the batch the shapes were traced with.
// false: `why` says, in one sentence, what combines images.
inline bool PerImageOperator(const pnnx::Operator* op, const std::vector<BatchOperand>& in, const std::vector<BatchOperand>& out, int batch,
                             std::string& why) {
    why.clear();
    const BatchFamily family = BatchFamilyOf(op->type);
    auto dim_text = [](int d) { return "dimension " + std::to_string(d); };
    if (family == BatchFamily::kUnknown) {
        why = "the batch rule has no row for the operator type " + op->type + ", so nothing is known about how it treats the batch";
        return false;
    }
    if (family == BatchFamily::kInput || family == BatchFamily::kConstant) return true;
    if (family == BatchFamily::kRoi) {
        // whatever the shapes say: K == N is a coincidence, and a slab of the boxes still indexes every image
        why = RoiBatchReason();
        return false;
    }
    if (family == BatchFamily::kXcorr) {
        // dimension 0 of the filter [O, C / g, kh, kw] counts filters.  A constant one meets every image (the right-aligned broadcast check
        // below does not apply to it); one computed from a graph input pairs every image with filters made from every image, whatever the
        // shapes say -- also the depthwise sandwich, whose views fold the batch into the channels
        for (size_t i = 1; i < in.size(); ++i)
            if (!in[i].constant) {
                why = XcorrBatchReason();
                return false;
            }
        if (in.size() < 2) {
            why = XcorrBatchReason();
            return false;
        }
        if (in[0].axis < 0) return true;
        if (in[0].axis != 0) {
            why = "the operator works image by image over dimension 0, but its input carries the batch in " + dim_text(in[0].axis);
            return false;
        }
        for (size_t i = 0; i < out.size(); ++i)
            if (out[i].axis != 0) {
                why = "output " + std::to_string(i) + " does not carry the batch in dimension 0";
                return false;
            }
        return true;
    }
    if (family == BatchFamily::kOutput) {
        for (const BatchOperand& o : in)
            if (o.axis != 0) {
                why = o.axis < 0 ? "the graph output does not carry the batch in a dimension of its own"
                                 : "the graph output carries the batch in " + dim_text(o.axis) + ", so a slab of images is not a slab of the buffer";
                return false;
            }
        return true;
    }
    // the operand the batch is followed from, as FollowBatchAxes does: the first input that carries it
    int first = -1;
    for (size_t i = 0; i < in.size() && first < 0; ++i)
        if (in[i].axis >= 0) first = (int)i;
    if (first < 0) return true;   // no operand carries the batch: whatever lost it is reported there, and nothing is left to combine
    const int axis = in[first].axis;
    const int rank = (int)in[first].shape.size();
    auto norm = [&](int d) { return d < 0 ? d + rank : d; };
    // operands beside it: one without a batch dimension is broadcast over the images (its batch extent is 1 where the other's is N), one
    // that carries the batch elsewhere pairs image i with something that is not image i
    if (batch > 1) {
        for (size_t i = 0; i < in.size(); ++i) {
            if (in[i].constant) {
                // a constant is exempt from both checks below: the same tensor meets every image.  What it must not do is hold one value PER
                // image: an extent above 1 where the other operand (shapes are right-aligned, as torch broadcasts) carries the batch
                const int at = axis - (rank - (int)in[i].shape.size());
                if (at >= 0 && at < (int)in[i].shape.size() && in[i].shape[at] != 1) {
                    why = "the constant input " + std::to_string(i) + " has extent " + std::to_string(in[i].shape[at]) + " along the batch " +
                          dim_text(axis) + " of input " + std::to_string(first) + ": it pairs one slice of itself with each image";
                    return false;
                }
                continue;
            }
            if (in[i].axis < 0) {
                why = "input " + std::to_string(i) + " has no batch dimension while input " + std::to_string(first) + " carries " +
                      std::to_string(batch) + " images: one value is combined with every image";
                return false;
            }
            if (in[i].axis != axis) {
                why = "input " + std::to_string(i) + " carries the batch in " + dim_text(in[i].axis) + ", input " + std::to_string(first) + " in " +
                      dim_text(axis);
                return false;
            }
        }
    }
    switch (family) {
        case BatchFamily::kSpatial:
            if (axis != 0) {
                why = "the operator works image by image over dimension 0, but its input carries the batch in " + dim_text(axis);
                return false;
            }
            break;
        case BatchFamily::kRows:
            if (axis == rank - 1) {
                why = "the operator contracts the last dimension, which is the batch";
                return false;
            }
            break;
        case BatchFamily::kSoftmax: {
            int dim = -3;   // nn.Softmax2d: the channels of a rank-4 tensor
            if (op->type != "nn.Softmax2d" && !Get(op, "dim", dim)) {
                why = "no dim= to compare with the batch dimension";
                return false;
            }
            if (norm(dim) == axis) {
                why = std::string(op->type == "F.normalize" ? "the norm is taken along " : "the softmax runs along ") + dim_text(axis) +
                      ", the batch: it normalises over the images";
                return false;
            }
            break;
        }
        case BatchFamily::kReduce: {
            std::vector<int> dims;
            int one = 0;
            if (IsNone(op, "dim")) {
                why = "the reduction runs over every dimension, the batch among them";
                return false;
            }
            if (Get(op, "dim", one)) dims.push_back(one);
            else if (!Get(op, "dim", dims)) {
                why = "no dim= to compare with the batch dimension";
                return false;
            }
            for (int d : dims)
                if (norm(d) == axis) {
                    why = "the reduction runs over " + dim_text(axis) + ", the batch: its result combines the images";
                    return false;
                }
            break;
        }
        case BatchFamily::kSlice: {
            std::vector<int> dims;
            int one = 0;
            if (Get(op, "dim", one)) dims.push_back(one);
            else if (!Get(op, "dims", dims)) {
                why = "no dim= / dims= to compare with the batch dimension";
                return false;
            }
            for (int d : dims)
                if (norm(d) == axis) {
                    why = "the pieces are cut along " + dim_text(axis) + ", the batch: a piece is a choice of images";
                    return false;
                }
            break;
        }
        case BatchFamily::kCat: {
            int dim = 0;
            if (!Get(op, "dim", dim)) {
                why = "no dim= to compare with the batch dimension";
                return false;
            }
            if (norm(dim) == axis) {
                why = "the concatenation runs along " + dim_text(axis) + ", the batch: it changes which image is where";
                return false;
            }
            break;
        }
        case BatchFamily::kAttention: {
            bool batch_first = false;
            Get(op, "batch_first", batch_first);
            const int want = batch_first ? 0 : 1;
            if (axis != want) {
                why = std::string("nn.MultiheadAttention with batch_first=") + (batch_first ? "True" : "False") + " reads the batch from " +
                      dim_text(want) + ", but its operands carry it in " + dim_text(axis);
                return false;
            }
            break;
        }
        case BatchFamily::kRecurrent: {
            bool batch_first = false;
            Get(op, "batch_first", batch_first);
            const int want = batch_first ? 0 : 1;
            if (axis != want) {
                why = op->type + " with batch_first=" + (batch_first ? "True" : "False") + " reads the batch from " + dim_text(want) +
                      ", but its input carries it in " + dim_text(axis);
                return false;
            }
            break;
        }
        default:   // kElementwise, kBinary, kMove, kReshape: what is left is where the batch ends up, below
            break;
    }
    // ... and the batch must still be a dimension of its own behind the operator: a view that folds it into another dimension (or out of
    // one), a permute whose result does not show it, lose it
    for (size_t i = 0; i < out.size(); ++i) {
        if (out[i].axis < 0) {
            why = "output " + std::to_string(i) + " does not carry the batch in a dimension of its own: it is folded into, or out of, another dimension";
            return false;
        }
        const bool moves = family == BatchFamily::kMove || family == BatchFamily::kReshape || family == BatchFamily::kReduce;
        // (a recurrent operator's state outputs [layers * dirs, N, H] carry the batch in dimension 1 whatever its input does)
        const bool state = family == BatchFamily::kRecurrent && i > 0;
        const int expect = state ? 1 : axis;
        if (!moves && out[i].axis != expect) {
            why = "output " + std::to_string(i) + " carries the batch in " + dim_text(out[i].axis) +
                  (state ? ", a state output in " + dim_text(expect) : ", the input in " + dim_text(axis));
            return false;
        }
    }
    return true;
}

// the operators of a graph (file order) that are not per-image, with the reason
struct BatchMixingEntry {
    std::string layer, type, reason;
};

inline std::vector<BatchMixingEntry> FindBatchMixing(const std::vector<pnnx::Operator*>& ops) {
    std::vector<BatchMixingEntry> found;
    const int file_batch = FileBatch(ops);
    if (file_batch <= 0) {
        // no static batch: such a graph is never split.  The graph inputs of a box head, [N, ...] and [K, 5], disagree whenever K != N: its
        // kRoi operators are listed all the same, so that what the engine logs and refuses does not depend on whether K happens to equal N
        // ... and so are the cross-correlations with a tensor filter: a template of batch 1 beside a search batch of N is such a graph
        const std::set<const pnnx::Operand*> consts = ConstantOperands(ops);
        for (const pnnx::Operator* op : ops) {
            if (BatchFamilyOf(op->type) == BatchFamily::kRoi) found.push_back({op->name, op->type, RoiBatchReason()});
            else if (HasTensorFilter(op, consts)) found.push_back({op->name, op->type, XcorrBatchReason()});
        }
        return found;
    }
    const std::map<const pnnx::Operand*, int> axes = FollowBatchAxes(ops, file_batch);
    const std::set<const pnnx::Operand*> constants = ConstantOperands(ops);
    auto describe = [&](const std::vector<pnnx::Operand*>& operands) {
        std::vector<BatchOperand> v;
        for (const pnnx::Operand* r : operands) {
            BatchOperand b;
            b.shape = r->shape;
            auto it = axes.find(r);
            b.axis = it == axes.end() ? -1 : it->second;
            b.constant = constants.count(r) > 0;
            v.push_back(b);
        }
        return v;
    };
    for (const pnnx::Operator* op : ops) {
        std::string why;
        if (!PerImageOperator(op, describe(op->inputs), describe(op->outputs), file_batch, why)) found.push_back({op->name, op->type, why});
    }
    return found;
}

}  // namespace SimpleInfer

#endif
