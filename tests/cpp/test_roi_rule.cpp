// The batch rule (simpleinfer_amd/csrc/host/batch_rule.h) for torchvision.ops.RoIAlign / torchvision.ops.roi_align: the family kRoi is never
// per-image -- the boxes [K, 5] name their image by an index in the data, and dimension 0 of the output counts boxes.  PerImageOperator on
// the operator alone and FindBatchMixing on hand-built box-head graphs, for both type strings, with K == N by coincidence (the shapes alone
// would say "per-image") and with K != N (the graph inputs disagree in dimension 0, so the graph has no static batch at all).  Stand-alone
// (the header needs pnnx/ir.h and pnnx/param_read.h only); built with -fsanitize=address,undefined by tests/test_roi_cpu.py.
#include <cstdio>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "batch_rule.h"

using namespace SimpleInfer;

static int failures = 0;
#define EXPECT(cond)                                                              \
    do {                                                                          \
        if (!(cond)) {                                                            \
            std::printf("%s:%d: EXPECT(%s) failed\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                           \
        }                                                                         \
    } while (0)

using Ints = std::vector<int>;
using Params = std::vector<std::pair<std::string, pnnx::Parameter>>;

struct Graph {
    std::vector<std::unique_ptr<pnnx::Operator>> own_ops;
    std::vector<std::unique_ptr<pnnx::Operand>> own_operands;
    std::vector<pnnx::Operator*> ops;

    pnnx::Operand* Add(const std::string& type, const std::string& name, std::vector<pnnx::Operand*> ins, Ints out_shape, Params params = {}) {
        own_ops.emplace_back(new pnnx::Operator);
        pnnx::Operator* op = own_ops.back().get();
        op->type = type;
        op->name = name;
        for (auto& kv : params) op->params[kv.first] = kv.second;
        op->inputs = ins;
        for (pnnx::Operand* r : ins) r->consumers.push_back(op);
        ops.push_back(op);
        if (type == "pnnx.Output") return nullptr;
        own_operands.emplace_back(new pnnx::Operand);
        pnnx::Operand* out = own_operands.back().get();
        out->name = name + ".out";
        out->shape = std::move(out_shape);
        out->producer = op;
        op->outputs.push_back(out);
        return out;
    }
};

static std::vector<std::string> Names(const std::vector<BatchMixingEntry>& found) {
    std::vector<std::string> v;
    for (const BatchMixingEntry& m : found) v.push_back(m.layer);
    return v;
}

static BatchOperand Opd(Ints shape, int axis) {
    BatchOperand b;
    b.shape = std::move(shape);
    b.axis = axis;
    return b;
}

static const char* const kReason = "the boxes name their image by an index in the data: dimension 0 of the output counts boxes, not images";

// features [n, 6, 5, 7] and boxes [k, 5] -> conv -> RoIAlign 3x3 -> conv + ReLU -> flatten -> Linear
static void BoxHead(Graph& g, const std::string& type, int n, int k) {
    auto* x = g.Add("pnnx.Input", "feat", {}, {n, 6, 5, 7});
    auto* r = g.Add("pnnx.Input", "rois", {}, {k, 5});
    auto* c = g.Add("nn.Conv2d", "neck", {x}, {n, 6, 5, 7});
    auto* p = g.Add(type, "pool", {c, r}, {k, 6, 3, 3}, {{"output_size", Ints{3, 3}}, {"sampling_ratio", 2}, {"aligned", false}});
    auto* h = g.Add("nn.ReLU", "relu", {g.Add("nn.Conv2d", "head", {p}, {k, 8, 3, 3})}, {k, 8, 3, 3});
    auto* f = g.Add("torch.flatten", "flat", {h}, {k, 72}, {{"start_dim", 1}, {"end_dim", -1}});
    g.Add("pnnx.Output", "out", {g.Add("nn.Linear", "fc", {f}, {k, 4})}, {});
}

int main() {
    using V = std::vector<std::string>;
    for (const char* type : {"torchvision.ops.RoIAlign", "torchvision.ops.roi_align"}) {
        EXPECT(BatchFamilyOf(type) == BatchFamily::kRoi);
        pnnx::Operator op;
        op.type = type;
        op.name = "pool";
        std::string why;
        // K == N == 8, every operand "carrying the batch" in dimension 0: the shapes say per-image, the rule does not
        EXPECT(!PerImageOperator(&op, {Opd({8, 6, 5, 7}, 0), Opd({8, 5}, 0)}, {Opd({8, 6, 3, 3}, 0)}, 8, why) && why == kReason);
        // K != N: the boxes carry no batch
        EXPECT(!PerImageOperator(&op, {Opd({8, 6, 5, 7}, 0), Opd({20, 5}, -1)}, {Opd({20, 6, 3, 3}, -1)}, 8, why) && why == kReason);
        // batch 1, no operand with a batch dimension at all
        EXPECT(!PerImageOperator(&op, {Opd({1, 6, 5, 7}, -1), Opd({3, 5}, -1)}, {Opd({3, 6, 3, 3}, -1)}, 1, why) && why == kReason);
        {   // K == N: the graph has a static batch of 8, and only the pooling is batch-mixing -- what follows it looks per-image from its shapes
            Graph g;
            BoxHead(g, type, 8, 8);
            EXPECT(FileBatch(g.ops) == 8);
            const std::vector<BatchMixingEntry> found = FindBatchMixing(g.ops);
            EXPECT(Names(found) == V{"pool"} && found[0].type == type && found[0].reason == kReason);
        }
        {   // K != N: no static batch, and the pooling is listed all the same
            Graph g;
            BoxHead(g, type, 8, 20);
            EXPECT(FileBatch(g.ops) == 0);
            const std::vector<BatchMixingEntry> found = FindBatchMixing(g.ops);
            EXPECT(Names(found) == V{"pool"} && found[0].type == type && found[0].reason == kReason);
        }
        {   // one image, many boxes
            Graph g;
            BoxHead(g, type, 1, 20);
            EXPECT(Names(FindBatchMixing(g.ops)) == V{"pool"});
        }
    }
    {   // graph inputs that disagree and no box pooling: nothing is listed, as before
        Graph g;
        auto* x = g.Add("pnnx.Input", "in0", {}, {8, 6, 5, 7});
        auto* y = g.Add("pnnx.Input", "in1", {}, {4, 6, 5, 7});
        g.Add("pnnx.Output", "out0", {g.Add("nn.Conv2d", "conv", {x}, {8, 6, 5, 7})}, {});
        g.Add("pnnx.Output", "out1", {y}, {});
        EXPECT(FileBatch(g.ops) == 0 && FindBatchMixing(g.ops).empty());
    }
    {   // a per-image graph stays per-image
        Graph g;
        auto* x = g.Add("pnnx.Input", "in", {}, {8, 6, 5, 7});
        g.Add("pnnx.Output", "out", {g.Add("nn.Conv2d", "conv", {x}, {8, 6, 5, 7})}, {});
        EXPECT(FindBatchMixing(g.ops).empty());
    }
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("roi rule ok\n");
    return 0;
}
