// The batch rule (simpleinfer_amd/csrc/host/batch_rule.h) for graph constants: a pnnx.Attribute is the family kConstant, always per-image;
// a constant operand is exempt from "has no batch dimension" and "carries the batch elsewhere" in either operand position, while an operand
// without a batch dimension that is NO constant still mixes; FollowBatchAxes gives a constant -1 even when its dimension 0 equals the traced
// batch; FileBatch ignores attributes; an operator whose inputs are all constants has constant outputs; and the one thing a constant must not
// do: hold one value per image.  Stand-alone (the header needs pnnx/ir.h and pnnx/param_read.h only); built with
// -fsanitize=address,undefined by tests/test_const_cpu.py.
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
    std::string why;
    EXPECT(BatchFamilyOf("pnnx.Attribute") == BatchFamily::kConstant);
    EXPECT(!BatchOperand().constant);
    {   // the attribute itself: always per-image, whatever its dimension 0
        pnnx::Operator attr;
        attr.type = "pnnx.Attribute";
        EXPECT(PerImageOperator(&attr, {}, {Opd({1, 8, 1, 1}, -1, true)}, 4, why) && why.empty());
        EXPECT(PerImageOperator(&attr, {}, {Opd({4, 8, 1, 1}, -1, true)}, 4, why) && why.empty());
    }
    pnnx::Operator bin;
    bin.type = "BinaryOp";
    bin.name = "mul_0";
    // a constant in either operand position: per-image -- same rank, lower rank (right-aligned), a scalar [1]
    EXPECT(PerImageOperator(&bin, {Opd({4, 8, 5, 6}, 0), Opd({1, 8, 1, 1}, -1, true)}, {Opd({4, 8, 5, 6}, 0)}, 4, why) && why.empty());
    EXPECT(PerImageOperator(&bin, {Opd({1, 8, 1, 1}, -1, true), Opd({4, 8, 5, 6}, 0)}, {Opd({4, 8, 5, 6}, 0)}, 4, why) && why.empty());
    EXPECT(PerImageOperator(&bin, {Opd({8, 1, 1}, -1, true), Opd({4, 8, 5, 6}, 0)}, {Opd({4, 8, 5, 6}, 0)}, 4, why) && why.empty());
    EXPECT(PerImageOperator(&bin, {Opd({4, 8, 5, 6}, 0), Opd({1}, -1, true)}, {Opd({4, 8, 5, 6}, 0)}, 4, why) && why.empty());
    // tokens: the batch in dimension 1 of [L, N, E] against [L, 1, E]; a constant [L, E] (rank 2) is right-aligned past the batch
    EXPECT(PerImageOperator(&bin, {Opd({16, 4, 32}, 1), Opd({16, 1, 32}, -1, true)}, {Opd({16, 4, 32}, 1)}, 4, why) && why.empty());
    EXPECT(PerImageOperator(&bin, {Opd({4, 16, 32}, 0), Opd({16, 32}, -1, true)}, {Opd({4, 16, 32}, 0)}, 4, why) && why.empty());
    // the SAME shapes without the constant mark: one value is combined with every image, as before
    EXPECT(!PerImageOperator(&bin, {Opd({4, 8, 5, 6}, 0), Opd({1, 8, 1, 1}, -1)}, {Opd({4, 8, 5, 6}, 0)}, 4, why) && Has(why, "input 1 has no batch dimension"));
    EXPECT(!PerImageOperator(&bin, {Opd({1, 8, 1, 1}, -1), Opd({4, 8, 5, 6}, 0)}, {Opd({4, 8, 5, 6}, 0)}, 4, why) && Has(why, "input 0 has no batch dimension"));
    // a non-constant operand that carries the batch elsewhere still mixes, with a constant beside it or not
    EXPECT(!PerImageOperator(&bin, {Opd({4, 4, 32}, 0), Opd({4, 4, 32}, 1)}, {Opd({4, 4, 32}, 0)}, 4, why) && Has(why, "input 1 carries the batch in dimension 1"));
    // a constant whose extent along the batch dimension is the batch: it holds a slice per image, and a slab of the batch would pair slices
    // with the wrong images -- the one case in which a constant operand mixes
    EXPECT(!PerImageOperator(&bin, {Opd({4, 8, 5, 6}, 0), Opd({4, 8, 1, 1}, -1, true)}, {Opd({4, 8, 5, 6}, 0)}, 4, why));
    EXPECT(Has(why, "constant input 1") && Has(why, "extent 4") && Has(why, "batch dimension 0"));
    EXPECT(!PerImageOperator(&bin, {Opd({16, 4, 32}, -1, true), Opd({16, 4, 32}, 1)}, {Opd({16, 4, 32}, 1)}, 4, why) && Has(why, "constant input 0"));
    // ... at batch 1 nothing can be paired wrongly
    EXPECT(PerImageOperator(&bin, {Opd({1, 8, 5, 6}, 0), Opd({1, 8, 5, 6}, -1, true)}, {Opd({1, 8, 5, 6}, 0)}, 1, why));
    // every input a constant: no operand carries the batch, nothing to combine
    EXPECT(PerImageOperator(&bin, {Opd({1, 8, 1, 1}, -1, true), Opd({1, 8, 1, 1}, -1, true)}, {Opd({1, 8, 1, 1}, -1, true)}, 4, why));
    {   // another family reads a constant as an ordinary read-only tensor: its own rule decides (a concat along the channels is per-image)
        pnnx::Operator cat;
        cat.type = "torch.cat";
        cat.params["dim"] = 1;
        EXPECT(PerImageOperator(&cat, {Opd({4, 8, 5, 6}, 0), Opd({1, 2, 5, 6}, -1, true)}, {Opd({4, 10, 5, 6}, 0)}, 4, why));
        cat.params["dim"] = 0;
        EXPECT(!PerImageOperator(&cat, {Opd({4, 8, 5, 6}, 0), Opd({1, 8, 5, 6}, -1, true)}, {Opd({5, 8, 5, 6}, -1)}, 4, why) && Has(why, "concatenation runs along dimension 0"));
    }

    {   // FrozenBatchNorm2d at batch 4: x * scale + shift, the constants [1, C, 1, 1]
        Graph g;
        auto* x = g.Add("pnnx.Input", "image", {}, {4, 3, 8, 8});
        auto* scale = g.Add("pnnx.Attribute", "scale", {}, {1, 8, 1, 1});
        auto* shift = g.Add("pnnx.Attribute", "shift", {}, {1, 8, 1, 1});
        auto* y = g.Add("nn.Conv2d", "conv", {x}, {4, 8, 8, 8});
        auto* m = g.Add("BinaryOp", "mul_0", {y, scale}, {4, 8, 8, 8}, {{"0", 2}});
        auto* a = g.Add("BinaryOp", "add_1", {shift, m}, {4, 8, 8, 8}, {{"0", 0}});
        g.Add("pnnx.Output", "out", {a}, {});
        EXPECT(FileBatch(g.ops) == 4);                       // the attributes [1, ...] do not disagree with the input
        const auto axes = FollowBatchAxes(g.ops, 4);
        EXPECT(axes.at(scale) == -1 && axes.at(shift) == -1 && axes.at(m) == 0 && axes.at(a) == 0);
        const auto constants = ConstantOperands(g.ops);
        EXPECT(constants.count(scale) && constants.count(shift) && !constants.count(x) && !constants.count(m) && !constants.count(a));
        EXPECT(Names(FindBatchMixing(g.ops)) == V{});
    }
    {   // a constant whose dimension 0 equals the traced batch (a [2, 2, H, W] table at batch 2): FileBatch still 2, the axis -1 and not 0 --
        // it is never re-batched -- and the operator that pairs it with the images is named
        Graph g;
        auto* x = g.Add("pnnx.Input", "image", {}, {2, 2, 8, 8});
        auto* table = g.Add("pnnx.Attribute", "table", {}, {2, 2, 8, 8});
        auto* chan = g.Add("pnnx.Attribute", "chan", {}, {2, 1, 1});          // dimension 0 equals the batch, but it is the CHANNELS: right-aligned
        auto* a = g.Add("BinaryOp", "add_0", {x, chan}, {2, 2, 8, 8}, {{"0", 0}});
        auto* b = g.Add("BinaryOp", "add_1", {a, table}, {2, 2, 8, 8}, {{"0", 0}});
        g.Add("pnnx.Output", "out", {b}, {});
        EXPECT(FileBatch(g.ops) == 2);
        const auto axes = FollowBatchAxes(g.ops, 2);
        EXPECT(axes.at(table) == -1 && axes.at(chan) == -1 && axes.at(a) == 0 && axes.at(b) == 0);
        const auto found = FindBatchMixing(g.ops);
        EXPECT(Names(found) == V{"add_1"} && Has(found[0].reason, "constant input 1"));
    }
    {   // attributes alone give no file batch; attributes that disagree with each other and with the input do not spoil it
        Graph g;
        g.Add("pnnx.Attribute", "a", {}, {3, 4});
        EXPECT(FileBatch(g.ops) == 0);
        g.Add("pnnx.Input", "image", {}, {4, 3, 8, 8});
        g.Add("pnnx.Attribute", "b", {}, {7});
        EXPECT(FileBatch(g.ops) == 4);
    }
    {   // operators on constants alone have constant outputs, through a chain; one non-constant input ends it
        Graph g;
        auto* x = g.Add("pnnx.Input", "image", {}, {4, 8, 5, 6});
        auto* c0 = g.Add("pnnx.Attribute", "c0", {}, {4, 8, 1, 1});
        auto* c1 = g.Add("pnnx.Attribute", "c1", {}, {1, 8, 1, 1});
        auto* s = g.Add("BinaryOp", "mul_0", {c0, c1}, {4, 8, 1, 1}, {{"0", 2}});
        auto* e = g.Add("UnaryOp", "exp_1", {s}, {4, 8, 1, 1}, {{"0", 7}});
        auto* y = g.Add("BinaryOp", "add_2", {x, c1}, {4, 8, 5, 6}, {{"0", 0}});
        g.Add("pnnx.Output", "out", {y}, {});
        const auto constants = ConstantOperands(g.ops);
        EXPECT(constants.count(c0) && constants.count(c1) && constants.count(s) && constants.count(e) && !constants.count(y) && !constants.count(x));
        const auto axes = FollowBatchAxes(g.ops, 4);
        EXPECT(axes.at(c0) == -1 && axes.at(s) == -1 && axes.at(e) == -1 && axes.at(y) == 0);
        EXPECT(Names(FindBatchMixing(g.ops)) == V{});
    }
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("const rule ok\n");
    return 0;
}
