// The per-image rule (simpleinfer_amd/csrc/host/batch_rule.h) on a table of (type, parameters, operand shapes and batch axes) -> verdict: one
// per-image and one batch-mixing row for every layer class of layer_registry.cpp, the coincidence cases (C == N under permute(1, 0, 2, 3), an
// [N, N] transpose, a reduction over (2, 3)), FollowBatchAxis on the shapes the engine's re-batch rule relies on, and FindBatchMixing on small
// hand-built graphs.  Arguments: the type strings of the layer registry -- each must have a row in the rule.  Stand-alone (the header needs
// pnnx/ir.h and pnnx/param_read.h only); built with -fsanitize=address,undefined by tests/test_batch_rule_cpu.py.
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

using Params = std::vector<std::pair<std::string, pnnx::Parameter>>;
using Ints = std::vector<int>;

static BatchOperand Opd(Ints shape, int axis) {
    BatchOperand b;
    b.shape = std::move(shape);
    b.axis = axis;
    return b;
}

struct Row {
    const char* what;
    std::string type;
    Params params;
    std::vector<BatchOperand> in, out;
    bool per_image;
    const char* why_has;   // a piece of the reason a batch-mixing verdict must give ("" for per-image rows)
    int batch = 8;         // the batch the shapes were traced with
};

static const int N = 8;
static const Ints X{N, 6, 5, 7};   // the rank-4 operand of most rows
static const Ints T{N, 10};        // the rank-2 one

static Row Same(const char* what, const std::string& type, Params p, const Ints& s, int axis, bool ok, const char* why = "") {
    return Row{what, type, std::move(p), {Opd(s, axis)}, {Opd(s, axis)}, ok, why};
}

static std::vector<Row> Table() {
    const pnnx::Parameter none;
    std::vector<Row> t;
    // ---- Softmax (nn.Softmax / nn.LogSoftmax / nn.Softmax2d / F.softmax / F.log_softmax)
    for (const char* type : {"nn.Softmax", "nn.LogSoftmax", "F.softmax", "F.log_softmax"}) {
        t.push_back(Same("softmax over the channels", type, {{"dim", 1}}, X, 0, true));
        t.push_back(Same("softmax over dim -1", type, {{"dim", -1}}, X, 0, true));
        t.push_back(Same("softmax over the batch, rank 4", type, {{"dim", 0}}, X, 0, false, "softmax runs along dimension 0"));
        t.push_back(Same("softmax over the batch, rank 2, negative dim", type, {{"dim", -2}}, T, 0, false, "softmax runs along dimension 0"));
        t.push_back(Same("softmax over dim 1 of tokens whose batch is dim 1", type, {{"dim", 1}}, Ints{9, N, 4}, 1, false, "dimension 1"));
        t.push_back(Same("softmax without dim=", type, {}, X, 0, false, "no dim="));
    }
    t.push_back(Same("Softmax2d", "nn.Softmax2d", {}, X, 0, true));
    t.push_back(Same("Softmax2d on [C, N, H, W]", "nn.Softmax2d", {}, X, 1, false, "dimension 1"));
    // ---- Reduce (torch.mean / sum / amax / amin)
    for (const char* type : {"torch.mean", "torch.sum", "torch.amax", "torch.amin"}) {
        t.push_back(Row{"reduce over (2, 3): per image", type, {{"dim", Ints{2, 3}}, {"keepdim", false}}, {Opd(X, 0)}, {Opd({N, 6}, 0)}, true, ""});
        t.push_back(Row{"reduce over 1, keepdim", type, {{"dim", 1}, {"keepdim", true}}, {Opd(X, 0)}, {Opd({N, 1, 5, 7}, 0)}, true, ""});
        t.push_back(Row{"reduce over the batch, keepdim", type, {{"dim", 0}, {"keepdim", true}}, {Opd(X, 0)}, {Opd({1, 6, 5, 7}, -1)}, false,
                        "reduction runs over dimension 0"});
        t.push_back(Row{"reduce over (0, 2, 3)", type, {{"dim", Ints{0, 2, 3}}, {"keepdim", true}}, {Opd(X, 0)}, {Opd({1, 6, 1, 1}, -1)}, false,
                        "reduction runs over dimension 0"});
        t.push_back(Row{"reduce over (-4, -1)", type, {{"dim", Ints{-4, -1}}, {"keepdim", true}}, {Opd(X, 0)}, {Opd({1, 6, 5, 1}, -1)}, false,
                        "reduction runs over dimension 0"});
        t.push_back(Row{"reduce over everything (dim=None)", type, {{"dim", none}}, {Opd(X, 0)}, {Opd({1}, -1)}, false, "every dimension"});
    }
    // ---- Slice (torch.chunk / torch.split / Tensor.slice) and Cat
    t.push_back(Row{"chunk on the channels", "torch.chunk", {{"chunks", 2}, {"dim", 1}}, {Opd(X, 0)}, {Opd({N, 3, 5, 7}, 0), Opd({N, 3, 5, 7}, 0)}, true, ""});
    t.push_back(Row{"chunk on the batch", "torch.chunk", {{"chunks", 2}, {"dim", 0}}, {Opd(X, 0)}, {Opd({4, 6, 5, 7}, -1), Opd({4, 6, 5, 7}, -1)}, false,
                    "cut along dimension 0"});
    t.push_back(Row{"split on the width", "torch.split", {{"dim", 3}, {"split_size_or_sections", Ints{3, 4}}}, {Opd(X, 0)},
                    {Opd({N, 6, 5, 3}, 0), Opd({N, 6, 5, 4}, 0)}, true, ""});
    t.push_back(Row{"split on the batch", "torch.split", {{"dim", -4}, {"split_size_or_sections", 4}}, {Opd(X, 0)},
                    {Opd({4, 6, 5, 7}, -1), Opd({4, 6, 5, 7}, -1)}, false, "cut along dimension 0"});
    t.push_back(Row{"slice on the channels", "Tensor.slice", {{"dim", 1}, {"start", 2}, {"end", 5}, {"step", 1}}, {Opd(X, 0)}, {Opd({N, 3, 5, 7}, 0)}, true, ""});
    t.push_back(Row{"slice on the batch", "Tensor.slice", {{"dim", 0}, {"start", 4}, {"end", 8}, {"step", 1}}, {Opd(X, 0)}, {Opd({4, 6, 5, 7}, -1)}, false,
                    "cut along dimension 0"});
    t.push_back(Row{"slice on several axes, the batch not among them", "Tensor.slice",
                    {{"dims", Ints{1, 3}}, {"starts", Ints{0, 1}}, {"ends", Ints{3, 5}}, {"steps", Ints{1, 1}}}, {Opd(X, 0)}, {Opd({N, 3, 5, 4}, 0)}, true, ""});
    t.push_back(Row{"slice on several axes, the batch among them", "Tensor.slice",
                    {{"dims", Ints{0, 1}}, {"starts", Ints{0, 0}}, {"ends", Ints{8, 3}}, {"steps", Ints{2, 1}}}, {Opd(X, 0)}, {Opd({4, 3, 5, 7}, -1)}, false,
                    "cut along dimension 0"});
    t.push_back(Row{"cat on the channels", "torch.cat", {{"dim", 1}}, {Opd(X, 0), Opd(X, 0)}, {Opd({N, 12, 5, 7}, 0)}, true, ""});
    t.push_back(Row{"cat on the batch", "torch.cat", {{"dim", 0}}, {Opd(X, 0), Opd(X, 0)}, {Opd({2 * N, 6, 5, 7}, -1)}, false, "concatenation runs along dimension 0"});
    t.push_back(Row{"cat of a batch-major operand and one without a batch", "torch.cat", {{"dim", 1}}, {Opd(X, 0), Opd({N, 6, 5, 7}, -1)}, {Opd({N, 12, 5, 7}, 0)},
                    false, "input 1 has no batch dimension"});
    // ---- BinaryOp
    t.push_back(Row{"add of two batch-major operands", "BinaryOp", {{"0", 0}}, {Opd(X, 0), Opd(X, 0)}, {Opd(X, 0)}, true, ""});
    t.push_back(Row{"mul with a per-image channel vector", "BinaryOp", {{"0", 2}}, {Opd(X, 0), Opd({N, 6, 1, 1}, 0)}, {Opd(X, 0)}, true, ""});
    t.push_back(Row{"scalar form", "BinaryOp", {{"0", 2}, {"1", 1}, {"2", 0.5f}}, {Opd(X, 0)}, {Opd(X, 0)}, true, ""});
    t.push_back(Row{"sub of a batch mean: extent N against extent 1", "BinaryOp", {{"0", 1}}, {Opd(X, 0), Opd({1, 6, 5, 7}, -1)}, {Opd(X, 0)}, false,
                    "input 1 has no batch dimension"});
    t.push_back(Row{"div by a batch maximum, operands the other way round", "BinaryOp", {{"0", 3}}, {Opd({1, 6, 1, 1}, -1), Opd(X, 0)}, {Opd(X, 0)}, false,
                    "input 0 has no batch dimension"});
    t.push_back(Row{"the same at batch 1: nothing to combine", "BinaryOp", {{"0", 1}}, {Opd({1, 6, 5, 7}, 0), Opd({1, 6, 5, 7}, -1)}, {Opd({1, 6, 5, 7}, 0)}, true, "", 1});
    t.push_back(Row{"add of x and its batch transpose", "BinaryOp", {{"0", 0}}, {Opd({N, N, 5, 7}, 0), Opd({N, N, 5, 7}, 1)}, {Opd({N, N, 5, 7}, 0)}, false,
                    "input 1 carries the batch in dimension 1"});
    t.push_back(Row{"operands that carry no batch at all (behind a reported operator)", "BinaryOp", {{"0", 0}}, {Opd({1, 6, 5, 7}, -1), Opd({1, 6, 5, 7}, -1)},
                    {Opd({1, 6, 5, 7}, -1)}, true, ""});
    // ---- Layout (permute / transpose move the batch; reshape / view / squeeze / unsqueeze / contiguous keep it or fold it) and Flatten
    for (const char* type : {"Tensor.permute", "torch.permute"}) {
        t.push_back(Row{"permute(0, 2, 3, 1)", type, {{"dims", Ints{0, 2, 3, 1}}}, {Opd(X, 0)}, {Opd({N, 5, 7, 6}, 0)}, true, ""});
        t.push_back(Row{"permute(1, 0, 2, 3) with C == N: the batch is dimension 1 behind it", type, {{"dims", Ints{1, 0, 2, 3}}}, {Opd({N, N, 5, 7}, 0)},
                        {Opd({N, N, 5, 7}, 1)}, true, ""});
        t.push_back(Row{"permute(2, 0, 1) to seq-first tokens", type, {{"dims", Ints{2, 0, 1}}}, {Opd({N, 6, 35}, 0)}, {Opd({35, N, 6}, 1)}, true, ""});
        t.push_back(Row{"a permute whose result does not show the batch", type, {{"dims", Ints{1, 0, 2, 3}}}, {Opd(X, 0)}, {Opd({6, N, 5, 7}, -1)}, false,
                        "does not carry the batch"});
    }
    t.push_back(Row{"transpose(1, 2)", "torch.transpose", {{"dim0", 1}, {"dim1", 2}}, {Opd({N, 3, 2, 5, 7}, 0)}, {Opd({N, 2, 3, 5, 7}, 0)}, true, ""});
    t.push_back(Row{"[N, N] transposed: the batch is dimension 1 behind it", "torch.transpose", {{"dim0", 0}, {"dim1", 1}}, {Opd({N, N}, 0)}, {Opd({N, N}, 1)}, true, ""});
    t.push_back(Row{"a transpose that loses track of the batch", "torch.transpose", {{"dim0", 0}, {"dim1", 1}}, {Opd(T, 0)}, {Opd({10, N}, -1)}, false,
                    "does not carry the batch"});
    for (const char* type : {"Tensor.reshape", "Tensor.view"}) {
        t.push_back(Row{"view(N, -1, k)", type, {{"shape", Ints{N, -1, 3}}}, {Opd({N, 5, 7, 6}, 0)}, {Opd({N, 70, 3}, 0)}, true, ""});
        t.push_back(Row{"a view that folds the batch into the channels", type, {{"shape", Ints{1, N * 6, 5, 7}}}, {Opd(X, 0)}, {Opd({1, N * 6, 5, 7}, -1)}, false,
                        "folded into, or out of"});
        t.push_back(Row{"a view that folds the batch out of the channels: the input no longer carries it", type, {{"shape", Ints{N, 6, 5, 7}}},
                        {Opd({1, N * 6, 5, 7}, -1)}, {Opd(X, -1)}, true, ""});
    }
    t.push_back(Row{"flatten(1)", "torch.flatten", {{"start_dim", 1}, {"end_dim", -1}}, {Opd(X, 0)}, {Opd({N, 210}, 0)}, true, ""});
    t.push_back(Row{"flatten(0)", "torch.flatten", {{"start_dim", 0}, {"end_dim", -1}}, {Opd(X, 0)}, {Opd({N * 210}, -1)}, false, "folded into, or out of"});
    t.push_back(Row{"squeeze", "torch.squeeze", {{"dim", 2}}, {Opd({N, 6, 1, 7}, 0)}, {Opd({N, 6, 7}, 0)}, true, ""});
    t.push_back(Row{"squeeze whose result lost the batch", "torch.squeeze", {{"dim", 0}}, {Opd({N, 6, 1, 7}, 0)}, {Opd({N, 6, 1, 7}, -1)}, false, "does not carry the batch"});
    t.push_back(Row{"unsqueeze", "torch.unsqueeze", {{"dim", 0}}, {Opd(T, 0)}, {Opd({1, N, 10}, 1)}, true, ""});
    t.push_back(Row{"unsqueeze whose result lost the batch", "torch.unsqueeze", {{"dim", 0}}, {Opd(T, 0)}, {Opd({1, N, 10}, -1)}, false, "does not carry the batch"});
    t.push_back(Same("contiguous", "Tensor.contiguous", {}, X, 0, true));
    t.push_back(Row{"contiguous whose result lost the batch", "Tensor.contiguous", {}, {Opd(X, 0)}, {Opd(X, -1)}, false, "does not carry the batch"});
    // ---- nn.MultiheadAttention
    t.push_back(Row{"self-attention, batch_first", "nn.MultiheadAttention", {{"batch_first", true}}, {Opd({N, 35, 6}, 0)}, {Opd({N, 35, 6}, 0)}, true, ""});
    t.push_back(Row{"three seq-first operands", "nn.MultiheadAttention", {{"batch_first", false}}, {Opd({35, N, 6}, 1), Opd({35, N, 6}, 1), Opd({35, N, 6}, 1)},
                    {Opd({35, N, 6}, 1)}, true, ""});
    t.push_back(Row{"batch_first=False on batch-major tokens", "nn.MultiheadAttention", {{"batch_first", false}}, {Opd({N, 35, 6}, 0)}, {Opd({N, 35, 6}, 0)}, false,
                    "reads the batch from dimension 1"});
    t.push_back(Row{"batch_first=True on seq-first tokens", "nn.MultiheadAttention", {{"batch_first", true}}, {Opd({35, N, 6}, 1)}, {Opd({35, N, 6}, 1)}, false,
                    "reads the batch from dimension 0"});
    t.push_back(Row{"keys that carry the batch elsewhere than the queries", "nn.MultiheadAttention", {{"batch_first", false}},
                    {Opd({N, N, 6}, 1), Opd({N, N, 6}, 0), Opd({N, N, 6}, 0)}, {Opd({N, N, 6}, 1)}, false, "input 1 carries the batch in dimension 0"});
    // ---- nn.Linear: over the last dimension
    t.push_back(Row{"Linear on [N, F]", "nn.Linear", {}, {Opd(T, 0)}, {Opd({N, 4}, 0)}, true, ""});
    t.push_back(Row{"Linear on seq-first tokens", "nn.Linear", {}, {Opd({35, N, 6}, 1)}, {Opd({35, N, 4}, 1)}, true, ""});
    t.push_back(Row{"Linear over the batch", "nn.Linear", {}, {Opd({10, N}, 1)}, {Opd({10, 4}, -1)}, false, "contracts the last dimension"});
    // ---- the image-by-image layers: the batch is dimension 0 or the layer is not per-image
    for (const char* type : {"nn.Conv2d", "nn.ConvTranspose2d", "nn.BatchNorm2d", "nn.GroupNorm", "nn.InstanceNorm2d", "nn.CircularPad2d", "nn.ConstantPad2d",
                             "nn.ReflectionPad2d", "nn.ReplicationPad2d", "nn.ZeroPad2d", "F.pad", "nn.MaxPool2d", "nn.AvgPool2d", "F.avg_pool2d",
                             "nn.AdaptiveAvgPool2d", "F.adaptive_avg_pool2d", "nn.Upsample", "F.interpolate", "F.upsample", "nn.PixelShuffle",
                             "nn.PixelUnshuffle", "F.pixel_shuffle", "F.pixel_unshuffle", "nn.PReLU"}) {
        t.push_back(Row{"batch-major", type, {}, {Opd({N, N, 5, 7}, 0)}, {Opd({N, N, 5, 7}, 0)}, true, ""});
        t.push_back(Row{"behind permute(1, 0, 2, 3)", type, {}, {Opd({N, N, 5, 7}, 1)}, {Opd({N, N, 5, 7}, 1)}, false, "image by image over dimension 0"});
    }
    t.push_back(Row{"Detect on three levels", "models.yolo.Detect", {}, {Opd({N, 16, 8, 8}, 0), Opd({N, 16, 4, 4}, 0), Opd({N, 16, 2, 2}, 0)}, {Opd({N, 252, 85}, 0)}, true, ""});
    t.push_back(Row{"Detect with a level that has no batch", "models.yolo.Detect", {}, {Opd({N, 16, 8, 8}, 0), Opd({1, 16, 4, 4}, -1), Opd({N, 16, 2, 2}, 0)},
                    {Opd({N, 252, 85}, 0)}, false, "input 1 has no batch dimension"});
    // ---- the element-wise layers: any batch dimension, the same one in and out
    for (const char* type : {"nn.ReLU", "F.relu", "nn.SiLU", "F.silu", "nn.Sigmoid", "F.sigmoid", "nn.Hardsigmoid", "F.hardsigmoid", "nn.Hardswish", "F.hardswish",
                             "nn.LeakyReLU", "F.leaky_relu", "nn.Tanh", "F.tanh", "nn.ReLU6", "F.relu6", "nn.Hardtanh", "F.hardtanh", "torch.clamp", "nn.Softplus",
                             "F.softplus", "nn.Mish", "F.mish", "UnaryOp"}) {
        t.push_back(Same("batch-major", type, {}, X, 0, true));
        t.push_back(Same("seq-first tokens", type, {}, Ints{35, N, 6}, 1, true));
        t.push_back(Row{"a result that shows the batch elsewhere than the input", type, {}, {Opd({N, N, 5, 7}, 0)}, {Opd({N, N, 5, 7}, 1)}, false,
                        "output 0 carries the batch in dimension 1"});
    }
    // ---- the graph's own operators, and types without a row
    t.push_back(Row{"graph input", "pnnx.Input", {}, {}, {Opd(X, 0)}, true, ""});
    t.push_back(Row{"batch-major graph output", "pnnx.Output", {}, {Opd(X, 0)}, {}, true, ""});
    t.push_back(Row{"graph output behind permute(1, 0, 2, 3), C == N", "pnnx.Output", {}, {Opd({N, N, 5, 7}, 1)}, {}, false, "carries the batch in dimension 1"});
    t.push_back(Row{"graph output behind an [N, N] transpose", "pnnx.Output", {}, {Opd({N, N}, 1)}, {}, false, "carries the batch in dimension 1"});
    t.push_back(Row{"graph output that lost the batch", "pnnx.Output", {}, {Opd({1, 6, 5, 7}, -1)}, {}, false, "does not carry the batch"});
    t.push_back(Same("a type the registry does not have", "my.CustomLayer", {}, X, 0, false, "no row for the operator type my.CustomLayer"));
    t.push_back(Same("pnnx.Expression (lowered before the rule sees a graph)", "pnnx.Expression", {}, X, 0, false, "no row"));
    t.push_back(Same("nn.LayerNorm", "nn.LayerNorm", {}, X, 0, false, "no row"));
    return t;
}

// ---- small graphs ------------------------------------------------------------------------------------------------------------------------
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

static void CheckGraphs() {
    using V = std::vector<std::string>;
    {   // conv -> softmax(dim=0) -> conv: the layer between two per-image ones, and only it
        Graph g;
        auto* x = g.Add("pnnx.Input", "in", {}, X);
        auto* a = g.Add("nn.Conv2d", "conv0", {x}, {N, 4, 5, 7});
        auto* s = g.Add("nn.Softmax", "sm", {a}, {N, 4, 5, 7}, {{"dim", 0}});
        auto* c = g.Add("nn.Conv2d", "conv1", {s}, {N, 3, 5, 7});
        g.Add("pnnx.Output", "out", {c}, {});
        EXPECT(Names(FindBatchMixing(g.ops)) == V{"sm"});
    }
    {   // x - mean(x, 0, keepdim): the reduction and the broadcast that brings it back
        Graph g;
        auto* x = g.Add("pnnx.Input", "in", {}, X);
        auto* m = g.Add("torch.mean", "mean", {x}, {1, 6, 5, 7}, {{"dim", 0}, {"keepdim", true}});
        auto* d = g.Add("BinaryOp", "sub", {x, m}, X, {{"0", 1}});
        g.Add("pnnx.Output", "out", {d}, {});
        EXPECT((Names(FindBatchMixing(g.ops)) == V{"mean", "sub"}));
    }
    {   // cat([x[4:8], x[0:4]], 0): both slices, and the output the halves were swapped into
        Graph g;
        auto* x = g.Add("pnnx.Input", "in", {}, X);
        auto* hi = g.Add("Tensor.slice", "hi", {x}, {4, 6, 5, 7}, {{"dim", 0}, {"start", 4}, {"end", 8}, {"step", 1}});
        auto* lo = g.Add("Tensor.slice", "lo", {x}, {4, 6, 5, 7}, {{"dim", 0}, {"start", 0}, {"end", 4}, {"step", 1}});
        auto* c = g.Add("torch.cat", "cat", {hi, lo}, X, {{"dim", 0}});
        g.Add("pnnx.Output", "out", {c}, {});
        EXPECT((Names(FindBatchMixing(g.ops)) == V{"hi", "lo", "out"}));
    }
    {   // permute(1, 0, 2, 3) of [8, 8, H, W] as the graph output: the shapes say batch-major, the rule does not
        Graph g;
        auto* x = g.Add("pnnx.Input", "in", {}, {N, N, 5, 7});
        auto* p = g.Add("Tensor.permute", "perm", {x}, {N, N, 5, 7}, {{"dims", Ints{1, 0, 2, 3}}});
        g.Add("pnnx.Output", "out", {p}, {});
        EXPECT(Names(FindBatchMixing(g.ops)) == V{"out"});
        // ... and permuted back it is per-image again
        Graph h;
        auto* y = h.Add("pnnx.Input", "in", {}, {N, N, 5, 7});
        auto* q = h.Add("Tensor.permute", "perm", {y}, {N, N, 5, 7}, {{"dims", Ints{1, 0, 2, 3}}});
        auto* r = h.Add("nn.ReLU", "relu", {q}, {N, N, 5, 7});
        auto* b = h.Add("Tensor.permute", "back", {r}, {N, N, 5, 7}, {{"dims", Ints{1, 0, 2, 3}}});
        h.Add("pnnx.Output", "out", {b}, {});
        EXPECT(FindBatchMixing(h.ops).empty());
    }
    {   // a view that folds the batch, a per-image operator, a view that unfolds it
        Graph g;
        auto* x = g.Add("pnnx.Input", "in", {}, X);
        auto* f = g.Add("Tensor.view", "fold", {x}, {1, N * 6, 5, 7}, {{"shape", Ints{1, N * 6, 5, 7}}});
        auto* r = g.Add("nn.ReLU", "relu", {f}, {1, N * 6, 5, 7});
        auto* u = g.Add("Tensor.view", "unfold", {r}, X, {{"shape", Ints{N, 6, 5, 7}}});
        g.Add("pnnx.Output", "out", {u}, {});
        EXPECT((Names(FindBatchMixing(g.ops)) == V{"fold", "out"}));
    }
    {   // seq-first attention behind flatten(2) + permute(2, 0, 1), and back: per-image throughout
        Graph g;
        auto* x = g.Add("pnnx.Input", "in", {}, X);
        auto* f = g.Add("torch.flatten", "flat", {x}, {N, 6, 35}, {{"start_dim", 2}, {"end_dim", -1}});
        auto* p = g.Add("Tensor.permute", "perm", {f}, {35, N, 6}, {{"dims", Ints{2, 0, 1}}});
        auto* l = g.Add("nn.Linear", "lin", {p}, {35, N, 6});
        auto* s = g.Add("BinaryOp", "add", {p, l}, {35, N, 6}, {{"0", 0}});
        auto* a = g.Add("nn.MultiheadAttention", "mha", {s, s, s}, {35, N, 6}, {{"batch_first", false}});
        auto* b = g.Add("Tensor.permute", "back", {a}, {N, 6, 35}, {{"dims", Ints{1, 2, 0}}});
        auto* v = g.Add("Tensor.reshape", "resh", {b}, X, {{"shape", Ints{N, 6, 5, 7}}});
        g.Add("pnnx.Output", "out", {v}, {});
        EXPECT(FindBatchMixing(g.ops).empty());
    }
    {   // an operator type without a row, in a graph that is otherwise per-image
        Graph g;
        auto* x = g.Add("pnnx.Input", "in", {}, X);
        auto* y = g.Add("my.CustomLayer", "custom", {x}, X);
        g.Add("pnnx.Output", "out", {y}, {});
        const std::vector<BatchMixingEntry> found = FindBatchMixing(g.ops);
        EXPECT(Names(found) == V{"custom"} && found[0].type == "my.CustomLayer" && found[0].reason.find("no row") != std::string::npos);
    }
    {   // graph inputs that disagree on the batch: nothing is followed (such a graph is never split)
        Graph g;
        auto* x = g.Add("pnnx.Input", "in0", {}, X);
        auto* y = g.Add("pnnx.Input", "in1", {}, {4, 6, 5, 7});
        g.Add("pnnx.Output", "out0", {x}, {});
        g.Add("pnnx.Output", "out1", {y}, {});
        EXPECT(FileBatch(g.ops) == 0 && FindBatchMixing(g.ops).empty());
    }
}

// FollowBatchAxis, the function the re-batch rule and this rule share
static void CheckFollow() {
    pnnx::Operator perm, tr, view, conv;
    perm.type = "Tensor.permute";
    perm.params["dims"] = Ints{1, 0, 2, 3};
    tr.type = "torch.transpose";
    tr.params["dim0"] = 0;
    tr.params["dim1"] = -1;
    view.type = "Tensor.view";
    conv.type = "nn.Conv2d";
    EXPECT(FollowBatchAxis(&perm, {N, N, 5, 7}, 0, {N, N, 5, 7}, N) == 1);     // C == N: the arguments decide, not the sizes
    EXPECT(FollowBatchAxis(&perm, {N, N, 5, 7}, 1, {N, N, 5, 7}, N) == 0);
    EXPECT(FollowBatchAxis(&perm, {N, 6, 5, 7}, 0, {6, N, 5, 7}, N) == 1);
    EXPECT(FollowBatchAxis(&tr, {N, N}, 0, {N, N}, N) == 1);
    EXPECT(FollowBatchAxis(&tr, {N, 10}, 0, {10, N}, N) == 1);
    EXPECT(FollowBatchAxis(&view, {N, 5, 7, 6}, 0, {N, 70, 3}, N) == 0);
    EXPECT(FollowBatchAxis(&view, {N, 6, 5, 7}, 0, {1, N * 6, 5, 7}, N) == -1);   // folded into the channels
    EXPECT(FollowBatchAxis(&view, {N, 6, 5, 7}, 0, {N * 6, 5, 7}, N) == -1);
    EXPECT(FollowBatchAxis(&view, {N, N, 5, 7}, 0, {1, N, N * 5, 7}, N) == 1);     // a leading 1 in front of the batch
    EXPECT(FollowBatchAxis(&view, {35, N, 6}, 1, {35, N, 2, 3}, N) == 1);
    EXPECT(FollowBatchAxis(&view, {N, N, 5, 7}, 1, {N * N, 5, 7}, N) == -1);
    EXPECT(FollowBatchAxis(&conv, {N, 3, 5, 7}, 0, {N, 6, 5, 7}, N) == 0);
    EXPECT(FollowBatchAxis(&conv, {N, 3, 5, 7}, 1, {N, 6, 5, 7}, N) == -1);        // (dimension 1 does not hold the batch)
    EXPECT(FollowBatchAxis(&conv, {N, 3, 5, 7}, -1, {N, 6, 5, 7}, N) == -1);
}

int main(int argc, char** argv) {
    const std::vector<Row> table = Table();
    for (const Row& r : table) {
        pnnx::Operator op;
        op.type = r.type;
        op.name = "op";
        for (auto& kv : r.params) op.params[kv.first] = kv.second;
        std::string why = "stale";
        const bool got = PerImageOperator(&op, r.in, r.out, r.batch, why);
        const bool reason_ok = got ? why.empty() : (!why.empty() && why.find(r.why_has) != std::string::npos && why.find('\n') == std::string::npos);
        if (got != r.per_image || !reason_ok) {
            std::printf("row [%s] %s: per-image %d (want %d), reason [%s] (want a piece [%s])\n", r.type.c_str(), r.what, (int)got, (int)r.per_image, why.c_str(),
                        r.why_has);
            ++failures;
        }
    }
    // both verdicts for every layer class, through the type strings of the table
    for (const char* family_type : {"nn.AdaptiveAvgPool2d", "nn.AvgPool2d", "nn.BatchNorm2d", "BinaryOp", "torch.cat", "nn.Conv2d", "nn.ConvTranspose2d",
                                    "torch.flatten", "nn.GroupNorm", "nn.Hardsigmoid", "nn.Hardswish", "Tensor.permute", "nn.LeakyReLU", "nn.Linear", "nn.MaxPool2d",
                                    "nn.MultiheadAttention", "nn.ZeroPad2d", "nn.ReLU6", "nn.PixelShuffle", "nn.PReLU", "torch.mean", "nn.ReLU", "nn.Sigmoid",
                                    "nn.SiLU", "Tensor.slice", "nn.Softmax", "nn.Tanh", "UnaryOp", "nn.Upsample", "models.yolo.Detect"}) {
        bool yes = false, no = false;
        for (const Row& r : table)
            if (r.type == family_type) (r.per_image ? yes : no) = true;
        if (!yes || !no) {
            std::printf("no %s row for %s\n", yes ? "batch-mixing" : "per-image", family_type);
            ++failures;
        }
    }
    CheckGraphs();
    CheckFollow();
    // every type string of the layer registry has a row
    int registry = 0;
    for (int i = 1; i < argc; ++i, ++registry)
        if (BatchFamilyOf(argv[i]) == BatchFamily::kUnknown) {
            std::printf("the layer registry has [%s], the batch rule has no row for it\n", argv[i]);
            ++failures;
        }
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("batch rule ok: %zu rows, %d registry types\n", table.size(), registry);
    return 0;
}
