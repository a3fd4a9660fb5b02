// The batch rule (simpleinfer_amd/csrc/host/batch_rule.h) for nn.LSTM / nn.GRU: the family kRecurrent reads the batch from dimension 0
// (batch_first) or 1 of its input, y keeps it there and the state outputs [layers * dirs, N, H] carry it in dimension 1.  PerImageOperator on
// the operator alone (both settings, the mismatch reasons, the state outputs) and FollowBatchAxes / FindBatchMixing on hand-built CRNN graphs.
// Stand-alone (the header needs pnnx/ir.h and pnnx/param_read.h only); built with -fsanitize=address,undefined by tests/test_rnn_cpu.py.
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

    // an operator with one output operand per shape of `out_shapes`
    std::vector<pnnx::Operand*> AddN(const std::string& type, const std::string& name, std::vector<pnnx::Operand*> ins, std::vector<Ints> out_shapes,
                                     Params params = {}) {
        own_ops.emplace_back(new pnnx::Operator);
        pnnx::Operator* op = own_ops.back().get();
        op->type = type;
        op->name = name;
        for (auto& kv : params) op->params[kv.first] = kv.second;
        op->inputs = ins;
        for (pnnx::Operand* r : ins) r->consumers.push_back(op);
        ops.push_back(op);
        std::vector<pnnx::Operand*> outs;
        for (size_t i = 0; i < out_shapes.size(); ++i) {
            own_operands.emplace_back(new pnnx::Operand);
            pnnx::Operand* out = own_operands.back().get();
            out->name = name + ".out" + std::to_string(i);
            out->shape = out_shapes[i];
            out->producer = op;
            op->outputs.push_back(out);
            outs.push_back(out);
        }
        return outs;
    }
    pnnx::Operand* Add(const std::string& type, const std::string& name, std::vector<pnnx::Operand*> ins, Ints out_shape, Params params = {}) {
        if (type == "pnnx.Output") {
            AddN(type, name, ins, {}, params);
            return nullptr;
        }
        return AddN(type, name, ins, {std::move(out_shape)}, params)[0];
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

// image [n, 3, 8, 4 t] -> conv -> pool to height 1 -> flatten(2) [n, c, t] -> permute -> recurrent -> Linear; `states`: the state outputs too,
// h_n through a Linear into a second graph output
static std::vector<pnnx::Operand*> Crnn(Graph& g, const std::string& type, int n, int t, bool batch_first, bool states, int layers_dirs = 2) {
    const int c = 8, h = 6;
    auto* x = g.Add("pnnx.Input", "image", {}, {n, 3, 8, 4 * t});
    auto* f = g.Add("nn.MaxPool2d", "pool", {g.Add("nn.Conv2d", "conv", {x}, {n, c, 8, 4 * t})}, {n, c, 1, t});
    auto* fl = g.Add("torch.flatten", "flat", {f}, {n, c, t}, {{"start_dim", 2}, {"end_dim", -1}});
    auto* p = batch_first ? g.Add("Tensor.permute", "perm", {fl}, {n, t, c}, {{"dims", Ints{0, 2, 1}}})
                          : g.Add("Tensor.permute", "perm", {fl}, {t, n, c}, {{"dims", Ints{2, 0, 1}}});
    const Ints y_shape = batch_first ? Ints{n, t, 2 * h} : Ints{t, n, 2 * h};
    std::vector<Ints> shapes = {y_shape};
    if (states)
        for (int i = 0; i < (type == "nn.LSTM" ? 2 : 1); ++i) shapes.push_back({layers_dirs, n, h});
    std::vector<pnnx::Operand*> outs = g.AddN(type, "rec", {p}, shapes, {{"batch_first", batch_first}, {"bidirectional", true}});
    Ints cls = y_shape;
    cls[2] = 5;
    g.Add("pnnx.Output", "out", {g.Add("nn.Linear", "fc", {outs[0]}, cls)}, {});
    if (states) g.Add("pnnx.Output", "out_h", {g.Add("nn.Linear", "fc_h", {outs[1]}, {layers_dirs, n, 5})}, {});
    return outs;
}

int main() {
    using V = std::vector<std::string>;
    for (const char* type : {"nn.LSTM", "nn.GRU"}) {
        const std::string ty = type;
        const bool lstm = ty == "nn.LSTM";
        EXPECT(BatchFamilyOf(type) == BatchFamily::kRecurrent);
        pnnx::Operator op;
        op.type = type;
        op.name = "rec";
        std::string why;
        // seq-first [T, N, I]: the batch in dimension 1, in and out
        op.params["batch_first"] = false;
        EXPECT(PerImageOperator(&op, {Opd({10, 4, 8}, 1)}, {Opd({10, 4, 12}, 1)}, 4, why) && why.empty());
        // ... with the state outputs, which carry it in dimension 1 too
        EXPECT(PerImageOperator(&op, {Opd({10, 4, 8}, 1)}, {Opd({10, 4, 12}, 1), Opd({2, 4, 6}, 1), Opd({2, 4, 6}, 1)}, 4, why) && why.empty());
        // the batch in dimension 0 of a seq-first operator: it would be read as the time
        EXPECT(!PerImageOperator(&op, {Opd({4, 10, 8}, 0)}, {Opd({4, 10, 12}, 0)}, 4, why));
        EXPECT(Has(why, type) && Has(why, "batch_first=False") && Has(why, "reads the batch from dimension 1") && Has(why, "carries it in dimension 0"));
        // y that lost the batch, y that carries it elsewhere, a state output that cannot be followed, one that carries it in dimension 0
        EXPECT(!PerImageOperator(&op, {Opd({10, 4, 8}, 1)}, {Opd({10, 4, 12}, -1)}, 4, why) && Has(why, "output 0 does not carry the batch"));
        EXPECT(!PerImageOperator(&op, {Opd({10, 4, 8}, 1)}, {Opd({4, 10, 12}, 0)}, 4, why) && Has(why, "output 0 carries the batch in dimension 0, the input in dimension 1"));
        EXPECT(!PerImageOperator(&op, {Opd({10, 4, 8}, 1)}, {Opd({10, 4, 12}, 1), Opd({2, 4, 6}, -1)}, 4, why) && Has(why, "output 1 does not carry the batch"));
        EXPECT(!PerImageOperator(&op, {Opd({10, 4, 8}, 1)}, {Opd({10, 4, 12}, 1), Opd({4, 4, 6}, 0)}, 4, why) &&
               Has(why, "output 1 carries the batch in dimension 0, a state output in dimension 1"));
        // batch_first [N, T, I]: dimension 0 for x and y, dimension 1 for the states
        op.params["batch_first"] = true;
        EXPECT(PerImageOperator(&op, {Opd({4, 10, 8}, 0)}, {Opd({4, 10, 12}, 0), Opd({2, 4, 6}, 1)}, 4, why) && why.empty());
        EXPECT(!PerImageOperator(&op, {Opd({10, 4, 8}, 1)}, {Opd({10, 4, 12}, 1)}, 4, why));
        EXPECT(Has(why, "batch_first=True") && Has(why, "reads the batch from dimension 0") && Has(why, "carries it in dimension 1"));
        EXPECT(!PerImageOperator(&op, {Opd({4, 10, 8}, 0)}, {Opd({4, 10, 12}, 0), Opd({2, 4, 6}, 0)}, 4, why) && Has(why, "a state output in dimension 1"));
        // h0 as a second input that carries the batch elsewhere than x does: the common operand check answers
        EXPECT(!PerImageOperator(&op, {Opd({4, 10, 8}, 0), Opd({2, 4, 6}, 1)}, {Opd({4, 10, 12}, 0)}, 4, why) && Has(why, "input 1 carries the batch in dimension 1"));
        // no operand carries the batch (batch 1): nothing to combine
        EXPECT(PerImageOperator(&op, {Opd({10, 1, 8}, -1)}, {Opd({10, 1, 12}, -1)}, 1, why));

        for (bool batch_first : {false, true}) {
            {   // y alone: the whole graph is per-image when the graph output is batch-major, and only the output is named when it is not
                Graph g;
                const auto outs = Crnn(g, type, 4, 10, batch_first, false);
                EXPECT(FileBatch(g.ops) == 4);
                const auto axes = FollowBatchAxes(g.ops, 4);
                EXPECT(axes.at(outs[0]) == (batch_first ? 0 : 1));
                EXPECT(Names(FindBatchMixing(g.ops)) == (batch_first ? V{} : V{"out"}));
            }
            {   // the state outputs are followed into dimension 1 -- also where layers * dirs equals the batch (2 == 2) and where T does
                for (int n : {4, 2}) {
                    Graph g;
                    const auto outs = Crnn(g, type, n, n == 2 ? 2 : 10, batch_first, true);
                    const auto axes = FollowBatchAxes(g.ops, n);
                    EXPECT(axes.at(outs[0]) == (batch_first ? 0 : 1));
                    for (size_t i = 1; i < outs.size(); ++i) EXPECT(axes.at(outs[i]) == 1);
                    EXPECT(outs.size() == (lstm ? 3u : 2u));
                    // the recurrent operator is per-image; the graph outputs that carry the batch in dimension 1 are what is named
                    const V names = Names(FindBatchMixing(g.ops));
                    EXPECT(names == (batch_first ? V{"out_h"} : V{"out", "out_h"}));
                }
            }
        }
        {   // a seq-first operator fed batch-major tokens (the permute is missing): named, with the reason
            Graph g;
            auto* x = g.Add("pnnx.Input", "tokens", {}, {4, 10, 8});
            auto* y = g.AddN(type, "rec", {x}, {{4, 10, 12}}, {{"batch_first", false}, {"bidirectional", true}})[0];
            g.Add("pnnx.Output", "out", {y}, {});
            const auto found = FindBatchMixing(g.ops);
            EXPECT(Names(found) == V{"rec"} && Has(found[0].reason, "reads the batch from dimension 1"));
        }
    }
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("rnn rule ok\n");
    return 0;
}
