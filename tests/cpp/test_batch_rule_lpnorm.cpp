// The batch rule (simpleinfer_amd/csrc/host/batch_rule.h) for F.normalize (family kSoftmax: per-image unless dim is the batch dimension) and
// torch.norm (family kReduce: per-image unless a reduced dim is the batch, the batch followed through keepdim=False).  PerImageOperator on
// the operator alone -- dim on and off the batch dimension, keepdim both ways, rank 2 and 4 --, FollowBatchAxis through the [N, H, W] result
// of a norm over dim 1 and the unsqueeze behind it, and FindBatchMixing on SuperPoint's written-out descriptor norm.
// Stand-alone (the header needs pnnx/ir.h and pnnx/param_read.h only); built with -fsanitize=address,undefined by tests/test_lpnorm_cpu.py.
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

static pnnx::Operator Op(const char* type, Params params) {
    pnnx::Operator op;
    op.type = type;
    op.name = "op";
    for (auto& kv : params) op.params[kv.first] = kv.second;
    return op;
}

int main() {
    using V = std::vector<std::string>;
    EXPECT(BatchFamilyOf("F.normalize") == BatchFamily::kSoftmax && BatchFamilyOf("torch.norm") == BatchFamily::kReduce);
    EXPECT(BatchFamilyOf("nn.BatchNorm1d") == BatchFamily::kUnknown && BatchFamilyOf("nn.LayerNorm") == BatchFamily::kUnknown &&
           BatchFamilyOf("F.cosine_similarity") == BatchFamily::kUnknown);
    std::string why;
    {   // F.normalize, rank 4 and rank 2: every dim but the batch dimension
        for (int dim : {1, 2, 3, -1, -3}) {
            pnnx::Operator op = Op("F.normalize", {{"dim", dim}, {"eps", 1e-12f}, {"p", 2.0f}});
            EXPECT(PerImageOperator(&op, {Opd({4, 8, 6, 6}, 0)}, {Opd({4, 8, 6, 6}, 0)}, 4, why) && why.empty());
        }
        for (int dim : {0, -4}) {
            pnnx::Operator op = Op("F.normalize", {{"dim", dim}, {"eps", 1e-12f}, {"p", 2.0f}});
            EXPECT(!PerImageOperator(&op, {Opd({4, 8, 6, 6}, 0)}, {Opd({4, 8, 6, 6}, 0)}, 4, why));
            EXPECT(Has(why, "the norm is taken along dimension 0, the batch") && Has(why, "normalises over the images"));
        }
        pnnx::Operator rows = Op("F.normalize", {{"dim", 1}, {"eps", 1e-12f}, {"p", 2.0f}});
        EXPECT(PerImageOperator(&rows, {Opd({4, 24}, 0)}, {Opd({4, 24}, 0)}, 4, why));
        pnnx::Operator cols = Op("F.normalize", {{"dim", -2}, {"eps", 1e-12f}, {"p", 1.0f}});
        EXPECT(!PerImageOperator(&cols, {Opd({4, 24}, 0)}, {Opd({4, 24}, 0)}, 4, why) && Has(why, "dimension 0, the batch"));
        // the batch carried in dimension 1 (behind a transpose): dim = 1 is then the batch
        EXPECT(!PerImageOperator(&rows, {Opd({24, 4}, 1)}, {Opd({24, 4}, 1)}, 4, why) && Has(why, "dimension 1, the batch"));
        pnnx::Operator no_dim = Op("F.normalize", {{"eps", 1e-12f}, {"p", 2.0f}});
        EXPECT(!PerImageOperator(&no_dim, {Opd({4, 24}, 0)}, {Opd({4, 24}, 0)}, 4, why) && Has(why, "no dim="));
        // the softmax's own sentence stays as it was
        pnnx::Operator sm = Op("F.softmax", {{"dim", 0}});
        EXPECT(!PerImageOperator(&sm, {Opd({4, 24}, 0)}, {Opd({4, 24}, 0)}, 4, why) && Has(why, "the softmax runs along dimension 0, the batch"));
    }
    {   // torch.norm: keepdim both ways, an int and an array, rank 4 and rank 2
        pnnx::Operator keep = Op("torch.norm", {{"dim", 1}, {"keepdim", true}, {"p", 2}});
        EXPECT(PerImageOperator(&keep, {Opd({4, 8, 6, 6}, 0)}, {Opd({4, 1, 6, 6}, 0)}, 4, why) && why.empty());
        pnnx::Operator drop = Op("torch.norm", {{"dim", 1}, {"keepdim", false}, {"p", 2}});
        EXPECT(PerImageOperator(&drop, {Opd({4, 8, 6, 6}, 0)}, {Opd({4, 6, 6}, 0)}, 4, why) && why.empty());
        pnnx::Operator pool = Op("torch.norm", {{"dim", Ints{2, 3}}, {"keepdim", false}, {"p", "fro"}});
        EXPECT(PerImageOperator(&pool, {Opd({4, 8, 6, 6}, 0)}, {Opd({4, 8}, 0)}, 4, why) && why.empty());
        pnnx::Operator batch = Op("torch.norm", {{"dim", 0}, {"keepdim", true}, {"p", 1}});
        EXPECT(!PerImageOperator(&batch, {Opd({4, 8, 6, 6}, 0)}, {Opd({1, 8, 6, 6}, -1)}, 4, why));
        EXPECT(Has(why, "the reduction runs over dimension 0, the batch"));
        pnnx::Operator mixed = Op("torch.norm", {{"dim", Ints{-4, 2}}, {"keepdim", true}, {"p", "inf"}});
        EXPECT(!PerImageOperator(&mixed, {Opd({4, 8, 6, 6}, 0)}, {Opd({1, 8, 1, 6}, -1)}, 4, why) && Has(why, "dimension 0, the batch"));
        pnnx::Operator all = Op("torch.norm", {{"keepdim", false}, {"p", 2}});
        EXPECT(!PerImageOperator(&all, {Opd({4, 8, 6, 6}, 0)}, {Opd({}, -1)}, 4, why) && Has(why, "every dimension"));
        pnnx::Operator rows = Op("torch.norm", {{"dim", 1}, {"keepdim", true}, {"p", 2}});
        EXPECT(PerImageOperator(&rows, {Opd({4, 24}, 0)}, {Opd({4, 1}, 0)}, 4, why));
        pnnx::Operator cols = Op("torch.norm", {{"dim", 0}, {"keepdim", true}, {"p", 2}});
        EXPECT(!PerImageOperator(&cols, {Opd({4, 24}, 0)}, {Opd({1, 24}, -1)}, 4, why));
        // a result that lost the batch behind a per-image reduction is reported as such
        EXPECT(!PerImageOperator(&drop, {Opd({4, 8, 6, 6}, 0)}, {Opd({4, 6, 6}, -1)}, 4, why) && Has(why, "does not carry the batch"));
    }
    {   // FollowBatchAxis: through the [N, H, W] result and its unsqueeze, also where another extent equals the batch
        pnnx::Operator drop = Op("torch.norm", {{"dim", 1}, {"keepdim", false}, {"p", 2}});
        EXPECT(FollowBatchAxis(&drop, {4, 8, 6, 6}, 0, {4, 6, 6}, 4) == 0);
        EXPECT(FollowBatchAxis(&drop, {4, 4, 4, 4}, 0, {4, 4, 4}, 4) == 0);
        pnnx::Operator unsq = Op("torch.unsqueeze", {{"dim", 1}});
        EXPECT(FollowBatchAxis(&unsq, {4, 6, 6}, 0, {4, 1, 6, 6}, 4) == 0);
        pnnx::Operator pool = Op("torch.norm", {{"dim", Ints{2, 3}}, {"keepdim", false}, {"p", 2}});
        EXPECT(FollowBatchAxis(&pool, {4, 8, 6, 6}, 0, {4, 8}, 4) == 0);
        pnnx::Operator batch = Op("torch.norm", {{"dim", 0}, {"keepdim", false}, {"p", 2}});
        EXPECT(FollowBatchAxis(&batch, {4, 8, 6, 6}, 0, {8, 6, 6}, 4) == -1);
    }
    {   // SuperPoint's descriptor head, written out: conv -> norm(dim 1, keepdim False) -> unsqueeze(1) -> div; per-image throughout
        Graph g;
        auto* x = g.Add("pnnx.Input", "image", {}, {4, 1, 32, 32});
        auto* d = g.Add("nn.Conv2d", "desc", {x}, {4, 32, 4, 4});
        auto* n = g.Add("torch.norm", "dn", {d}, {4, 4, 4}, {{"dim", 1}, {"keepdim", false}, {"p", 2}});
        auto* u = g.Add("torch.unsqueeze", "dn1", {n}, {4, 1, 4, 4}, {{"dim", 1}});
        auto* q = g.Add("BinaryOp", "div", {d, u}, {4, 32, 4, 4}, {{"0", 3}});
        g.Add("pnnx.Output", "out", {q}, {});
        EXPECT(FileBatch(g.ops) == 4);
        const auto axes = FollowBatchAxes(g.ops, 4);
        EXPECT(axes.at(n) == 0 && axes.at(u) == 0 && axes.at(q) == 0);
        EXPECT(Names(FindBatchMixing(g.ops)).empty());
    }
    {   // an embedding head: Linear -> F.normalize(dim 1) is per-image; normalising over dim 0 is named
        for (int dim : {1, 0}) {
            Graph g;
            auto* x = g.Add("pnnx.Input", "features", {}, {4, 32});
            auto* e = g.Add("nn.Linear", "embed", {x}, {4, 24});
            auto* y = g.Add("F.normalize", "unit", {e}, {4, 24}, {{"dim", dim}, {"eps", 1e-12f}, {"p", 2.0f}});
            g.Add("pnnx.Output", "out", {y}, {});
            EXPECT(Names(FindBatchMixing(g.ops)) == (dim == 1 ? V{} : V{"unit"}));
        }
    }
    {   // a norm over the batch that is broadcast back: the norm is named
        Graph g;
        auto* x = g.Add("pnnx.Input", "image", {}, {4, 8, 6, 6});
        auto* n = g.Add("torch.norm", "over_batch", {x}, {1, 8, 6, 6}, {{"dim", 0}, {"keepdim", true}, {"p", 2}});
        auto* q = g.Add("BinaryOp", "div", {x, n}, {4, 8, 6, 6}, {{"0", 3}});
        g.Add("pnnx.Output", "out", {q}, {});
        const auto found = FindBatchMixing(g.ops);
        EXPECT(!found.empty() && found[0].layer == "over_batch" && Has(found[0].reason, "the batch"));
    }
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("lpnorm rule ok\n");
    return 0;
}
