// The batch rule (simpleinfer_amd/csrc/host/batch_rule.h) for nn.Conv1d: a row of the family kSpatial on rank-3 operands [N, C, L].  The
// operator is per-image while the batch is dimension 0 of its input and output; behind a permute that moves the batch into dimension 1 it
// would convolve over the images, and is named with the reason.  PerImageOperator on the operator alone, FollowBatchAxes / FindBatchMixing on
// hand-built graphs (a Conv1d stack, Conv1d -> permute -> GRU, a permute in front of the Conv1d).
// Stand-alone (the header needs pnnx/ir.h and pnnx/param_read.h only); built with -fsanitize=address,undefined by tests/test_conv1d_cpu.py.
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

static bool Has(const std::string& text, const char* part) { return text.find(part) != std::string::npos; }

int main() {
    using V = std::vector<std::string>;
    EXPECT(BatchFamilyOf("nn.Conv1d") == BatchFamily::kSpatial);
    EXPECT(BatchFamilyOf("nn.ConvTranspose1d") == BatchFamily::kUnknown && BatchFamilyOf("F.conv1d") == BatchFamily::kUnknown);
    {
        pnnx::Operator op;
        op.type = "nn.Conv1d";
        op.name = "conv";
        std::string why;
        // [N, C, L] -> [N, OC, Lo]: the batch in dimension 0 on both sides
        EXPECT(PerImageOperator(&op, {Opd({4, 16, 50}, 0)}, {Opd({4, 32, 25}, 0)}, 4, why) && why.empty());
        // the batch in dimension 1 (behind a permute): it would be read as the channels
        EXPECT(!PerImageOperator(&op, {Opd({16, 4, 50}, 1)}, {Opd({32, 4, 25}, 1)}, 4, why));
        EXPECT(Has(why, "image by image over dimension 0") && Has(why, "dimension 1"));
        // ... in dimension 2: it would be convolved over
        EXPECT(!PerImageOperator(&op, {Opd({16, 50, 4}, 2)}, {Opd({32, 25, 4}, 2)}, 4, why) && Has(why, "dimension 2"));
        // an output that lost the batch, or shows it elsewhere
        EXPECT(!PerImageOperator(&op, {Opd({4, 16, 50}, 0)}, {Opd({4, 32, 25}, -1)}, 4, why) && Has(why, "output 0 does not carry the batch"));
        EXPECT(!PerImageOperator(&op, {Opd({4, 16, 50}, 0)}, {Opd({32, 4, 25}, 1)}, 4, why) && Has(why, "output 0 carries the batch in dimension 1"));
        // batch 1: nothing carries it, nothing to combine
        EXPECT(PerImageOperator(&op, {Opd({1, 16, 50}, -1)}, {Opd({1, 32, 25}, -1)}, 1, why));
    }
    {   // a stack of temporal convolutions with a residual add: per-image throughout, also where C or L equal the batch
        for (int c : {16, 4}) {
            Graph g;
            auto* x = g.Add("pnnx.Input", "frames", {}, {4, c, 40});
            auto* a = g.Add("nn.ReLU", "relu", {g.Add("nn.Conv1d", "stem", {x}, {4, 8, 20})}, {4, 8, 20});
            auto* dw = g.Add("nn.Conv1d", "dw", {a}, {4, 8, 20});
            auto* pw = g.Add("nn.Conv1d", "pw", {dw}, {4, 4, 20});
            auto* res = g.Add("nn.Conv1d", "res", {a}, {4, 4, 20});
            auto* sum = g.Add("BinaryOp", "add", {pw, res}, {4, 4, 20});
            g.Add("pnnx.Output", "out", {sum}, {});
            EXPECT(FileBatch(g.ops) == 4);
            const auto axes = FollowBatchAxes(g.ops, 4);
            for (pnnx::Operand* r : {a, dw, pw, res, sum}) EXPECT(axes.at(r) == 0);
            EXPECT(Names(FindBatchMixing(g.ops)).empty());
        }
    }
    {   // Conv1d -> permute(2, 0, 1) -> GRU (seq-first) -> Linear: the convolution sees dimension 0, the recurrent operator dimension 1; only
        // the graph output, which carries the batch in dimension 1, is named
        Graph g;
        auto* x = g.Add("pnnx.Input", "frames", {}, {4, 8, 50});
        auto* c = g.Add("nn.Conv1d", "conv", {x}, {4, 16, 25});
        auto* p = g.Add("Tensor.permute", "perm", {c}, {25, 4, 16}, {{"dims", Ints{2, 0, 1}}});
        auto* y = g.Add("nn.GRU", "gru", {p}, {25, 4, 12}, {{"batch_first", false}, {"bidirectional", false}});
        g.Add("pnnx.Output", "out", {g.Add("nn.Linear", "fc", {y}, {25, 4, 5})}, {});
        const auto axes = FollowBatchAxes(g.ops, 4);
        EXPECT(axes.at(c) == 0 && axes.at(p) == 1 && axes.at(y) == 1);
        EXPECT(Names(FindBatchMixing(g.ops)) == V{"out"});
    }
    {   // a permute IN FRONT of the convolution: [N, T, C] tokens -> permute(1, 2, 0) [T, C, N] -> Conv1d convolves over the images
        Graph g;
        auto* x = g.Add("pnnx.Input", "tokens", {}, {4, 25, 16});
        auto* p = g.Add("Tensor.permute", "perm", {x}, {25, 16, 4}, {{"dims", Ints{1, 2, 0}}});
        auto* c = g.Add("nn.Conv1d", "conv", {p}, {25, 8, 4});
        g.Add("pnnx.Output", "out", {c}, {});
        const auto axes = FollowBatchAxes(g.ops, 4);
        EXPECT(axes.at(p) == 2);
        const auto found = FindBatchMixing(g.ops);
        EXPECT(!found.empty() && found[0].layer == "conv" && Has(found[0].reason, "image by image over dimension 0"));
    }
    {   // ... and the batch in dimension 1 after permute(1, 0, 2): the channels of the convolution would be the images
        Graph g;
        auto* x = g.Add("pnnx.Input", "x", {}, {4, 16, 50});
        auto* p = g.Add("Tensor.permute", "perm", {x}, {16, 4, 50}, {{"dims", Ints{1, 0, 2}}});
        auto* c = g.Add("nn.Conv1d", "conv", {p}, {16, 8, 50});
        g.Add("pnnx.Output", "out", {c}, {});
        EXPECT(FollowBatchAxes(g.ops, 4).at(p) == 1);
        const auto found = FindBatchMixing(g.ops);
        EXPECT(!found.empty() && found[0].layer == "conv" && Has(found[0].reason, "dimension 1"));
    }
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("conv1d rule ok\n");
    return 0;
}
