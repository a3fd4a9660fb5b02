// The batch rule (simpleinfer_amd/csrc/host/batch_rule.h) for F.conv2d, the family kXcorr: against a CONSTANT filter (and bias) the operator
// is kSpatial on x -- per-image while the batch is dimension 0 -- whatever dimension 0 of the filter says; with a filter computed from a graph
// input it is never per-image, the depthwise sandwich of the Siamese trackers included, and the reason says why.  PerImageOperator on the
// operator alone, FollowBatchAxes / ConstantOperands / FindBatchMixing on hand-built graphs.
// Stand-alone (the header needs pnnx/ir.h and pnnx/param_read.h only); built with -fsanitize=address,undefined by tests/test_xcorr_cpu.py.
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

static BatchOperand Opd(Ints shape, int axis, bool constant = false) {
    BatchOperand b;
    b.shape = std::move(shape);
    b.axis = axis;
    b.constant = constant;
    return b;
}

static bool Has(const std::string& text, const char* part) { return text.find(part) != std::string::npos; }

int main() {
    using V = std::vector<std::string>;
    EXPECT(BatchFamilyOf("F.conv2d") == BatchFamily::kXcorr);
    EXPECT(BatchFamilyOf("F.conv1d") == BatchFamily::kUnknown && BatchFamilyOf("F.conv_transpose2d") == BatchFamily::kUnknown &&
           BatchFamilyOf("F.linear") == BatchFamily::kUnknown && BatchFamilyOf("nn.LayerNorm") == BatchFamily::kUnknown);
    const char* const reason = "its dimension 0 counts filters, not images";
    EXPECT(Has(XcorrBatchReason(), reason));
    {
        pnnx::Operator op;
        op.type = "F.conv2d";
        op.name = "xcorr";
        std::string why;
        // a constant filter [O, C, kh, kw], also one whose dimension 0 equals the batch: per-image on x
        EXPECT(PerImageOperator(&op, {Opd({4, 8, 16, 16}, 0), Opd({6, 8, 3, 3}, -1, true)}, {Opd({4, 6, 14, 14}, 0)}, 4, why) && why.empty());
        EXPECT(PerImageOperator(&op, {Opd({4, 8, 16, 16}, 0), Opd({4, 8, 3, 3}, -1, true)}, {Opd({4, 4, 14, 14}, 0)}, 4, why) && why.empty());
        // ... with a constant bias
        EXPECT(PerImageOperator(&op, {Opd({4, 8, 16, 16}, 0), Opd({6, 8, 3, 3}, -1, true), Opd({6}, -1, true)}, {Opd({4, 6, 14, 14}, 0)}, 4, why));
        // the batch elsewhere than dimension 0 of x, or lost behind the operator
        EXPECT(!PerImageOperator(&op, {Opd({8, 4, 16, 16}, 1), Opd({6, 8, 3, 3}, -1, true)}, {Opd({8, 6, 14, 14}, -1)}, 4, why));
        EXPECT(Has(why, "image by image over dimension 0") && Has(why, "dimension 1"));
        EXPECT(!PerImageOperator(&op, {Opd({4, 8, 16, 16}, 0), Opd({6, 8, 3, 3}, -1, true)}, {Opd({4, 6, 14, 14}, -1)}, 4, why));
        EXPECT(Has(why, "output 0 does not carry the batch in dimension 0"));
        // a tensor filter: never, whether it carries the batch (SiamRPN++'s template), has lost it (the up-channel view) or never had it
        EXPECT(!PerImageOperator(&op, {Opd({4, 8, 16, 16}, 0), Opd({4, 8, 5, 5}, 0)}, {Opd({4, 4, 12, 12}, 0)}, 4, why) && Has(why, reason));
        EXPECT(!PerImageOperator(&op, {Opd({4, 8, 16, 16}, 0), Opd({10, 8, 4, 4}, -1)}, {Opd({4, 10, 13, 13}, 0)}, 4, why) && Has(why, reason));
        EXPECT(!PerImageOperator(&op, {Opd({1, 32, 16, 16}, -1), Opd({32, 1, 5, 5}, -1)}, {Opd({1, 32, 12, 12}, -1)}, 4, why) && Has(why, reason));
        // a constant filter with a tensor bias is no constant operator either
        EXPECT(!PerImageOperator(&op, {Opd({4, 8, 16, 16}, 0), Opd({6, 8, 3, 3}, -1, true), Opd({6}, -1)}, {Opd({4, 6, 14, 14}, 0)}, 4, why) && Has(why, reason));
        // batch 1 with a constant filter: nothing carries the batch, nothing to combine
        EXPECT(PerImageOperator(&op, {Opd({1, 8, 16, 16}, -1), Opd({6, 8, 3, 3}, -1, true)}, {Opd({1, 6, 14, 14}, -1)}, 1, why));
    }
    {   // blur-pool: conv -> F.conv2d(x, buffer [C, 1, 3, 3], groups = C) -> conv, the buffer a pnnx.Attribute (C equal to the batch): per-image
        Graph g;
        auto* x = g.Add("pnnx.Input", "image", {}, {4, 3, 16, 16});
        auto* f = g.Add("nn.Conv2d", "stem", {x}, {4, 4, 16, 16});
        auto* k = g.Add("pnnx.Attribute", "blur", {}, {4, 1, 3, 3});
        auto* y = g.Add("F.conv2d", "pool", {f, k}, {4, 4, 8, 8}, {{"groups", 4}});
        g.Add("pnnx.Output", "out", {g.Add("nn.Conv2d", "head", {y}, {4, 2, 8, 8})}, {});
        EXPECT(FileBatch(g.ops) == 4);
        const auto axes = FollowBatchAxes(g.ops, 4);
        EXPECT(axes.at(k) == -1 && axes.at(y) == 0);
        EXPECT(ConstantOperands(g.ops).count(k) == 1 && !HasTensorFilter(g.ops[3], ConstantOperands(g.ops)));
        EXPECT(Names(FindBatchMixing(g.ops)).empty());
    }
    {   // a dynamic head whose kernels are DERIVED from a constant (attribute -> view): still constant, still per-image
        Graph g;
        auto* x = g.Add("pnnx.Input", "image", {}, {4, 3, 16, 16});
        auto* f = g.Add("nn.Conv2d", "feat", {x}, {4, 8, 16, 16});
        auto* k = g.Add("Tensor.view", "kernels", {g.Add("pnnx.Attribute", "bank", {}, {1, 32, 1, 1})}, {4, 8, 1, 1}, {{"shape", Ints{4, 8, 1, 1}}});
        auto* y = g.Add("F.conv2d", "masks", {f, k}, {4, 4, 16, 16}, {{"groups", 1}});
        g.Add("pnnx.Output", "out", {y}, {});
        EXPECT(ConstantOperands(g.ops).count(k) == 1);
        EXPECT(Names(FindBatchMixing(g.ops)).empty());
    }
    {   // SiamFC: the template [1, C, h, w] beside a search batch of 4 -- the graph inputs disagree on the batch, and the operator is listed
        // all the same; at batch 1 on both sides it is listed by the rule
        for (int n : {4, 1}) {
            Graph g;
            auto* z = g.Add("nn.Conv2d", "fz", {g.Add("pnnx.Input", "template", {}, {1, 3, 17, 17})}, {1, 16, 13, 13});
            auto* x = g.Add("nn.Conv2d", "fx", {g.Add("pnnx.Input", "search", {}, {n, 3, 33, 33})}, {n, 16, 29, 29});
            auto* y = g.Add("F.conv2d", "xcorr", {x, z}, {n, 1, 17, 17}, {{"groups", 1}});
            g.Add("pnnx.Output", "out", {y}, {});
            EXPECT(FileBatch(g.ops) == (n == 1 ? 1 : 0));
            const auto found = FindBatchMixing(g.ops);
            EXPECT(Names(found) == V{"xcorr"} && Has(found[0].reason, reason));
        }
    }
    {   // SiamRPN++: the sandwich.  The views fold the batch into the channels (x) and into dimension 0 of the filter (z): the views are named
        // because the batch is no dimension of its own behind them, and the cross-correlation with the rule's reason
        Graph g;
        auto* z = g.Add("nn.Conv2d", "fz", {g.Add("pnnx.Input", "template", {}, {2, 3, 11, 11})}, {2, 8, 7, 7});
        auto* x = g.Add("nn.Conv2d", "fx", {g.Add("pnnx.Input", "search", {}, {2, 3, 19, 19})}, {2, 8, 15, 15});
        auto* xv = g.Add("Tensor.view", "xv", {x}, {1, 16, 15, 15}, {{"shape", Ints{1, 16, 15, 15}}});
        auto* zv = g.Add("Tensor.view", "zv", {z}, {16, 1, 7, 7}, {{"shape", Ints{16, 1, 7, 7}}});
        auto* y = g.Add("F.conv2d", "xcorr", {xv, zv}, {1, 16, 9, 9}, {{"groups", 16}});
        auto* yv = g.Add("Tensor.view", "yv", {y}, {2, 8, 9, 9}, {{"shape", Ints{2, 8, 9, 9}}});
        g.Add("pnnx.Output", "out", {yv}, {});
        EXPECT(FileBatch(g.ops) == 2);
        EXPECT(HasTensorFilter(g.ops[6], ConstantOperands(g.ops)));
        const auto found = FindBatchMixing(g.ops);
        bool listed = false;
        for (const BatchMixingEntry& m : found)
            if (m.layer == "xcorr") listed = Has(m.reason, reason);
        EXPECT(listed && found.size() >= 2);
    }
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("xcorr rule ok\n");
    return 0;
}
