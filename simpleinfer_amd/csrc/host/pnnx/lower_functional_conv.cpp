#include "lower_functional_conv.h"

#include <algorithm>

namespace pnnx {

namespace {

// the pnnx.Attribute operator behind `r` when `reader` is its only consumer and its data is an fp32 tensor of rank `rank`, else null
Operator* sole_constant(const Operand* r, const Operator* reader, size_t rank) {
    if (!r || !r->producer || r->producer->type != "pnnx.Attribute" || r->producer->outputs.size() != 1) return nullptr;
    if (r->consumers.size() != 1 || r->consumers[0] != reader) return nullptr;
    auto data = r->producer->attrs.find("data");
    if (data == r->producer->attrs.end() || data->second.type != 1 || data->second.shape.size() != rank || r->shape != data->second.shape) return nullptr;
    size_t elems = 1;
    for (int d : data->second.shape) elems *= d > 0 ? (size_t)d : 0;
    return elems > 0 && data->second.data.size() == elems * sizeof(float) ? r->producer : nullptr;
}

bool pair_of(const Operator* op, const char* key, int& a, int& b) {
    auto it = op->params.find(key);
    if (it == op->params.end() || it->second.type != 5 || it->second.ai.size() != 2) return false;
    a = it->second.ai[0];
    b = it->second.ai[1];
    return true;
}

void drop_constant(Graph& g, Operator* attr) {
    Operand* out = attr->outputs[0];
    g.operands.erase(std::find(g.operands.begin(), g.operands.end(), out));
    delete out;
    g.ops.erase(std::find(g.ops.begin(), g.ops.end(), attr));
    delete attr;
}

bool lower_one(Graph& g, Operator* op) {
    if (op->inputs.size() != 2 && op->inputs.size() != 3) return false;
    if (op->outputs.size() != 1) return false;
    Operator* wa = sole_constant(op->inputs[1], op, 4);
    Operator* ba = op->inputs.size() == 3 ? sole_constant(op->inputs[2], op, 1) : nullptr;
    if (!wa || (op->inputs.size() == 3 && !ba) || wa == ba) return false;
    const Attribute& w = wa->attrs.at("data");
    const Operand* x = op->inputs[0];
    int sh = 0, sw = 0, dh = 0, dw = 0, ph = 0, pw = 0, groups = 0;
    if (!pair_of(op, "stride", sh, sw) || !pair_of(op, "dilation", dh, dw)) return false;
    auto gi = op->params.find("groups");
    if (gi == op->params.end() || gi->second.type != 2) return false;
    groups = gi->second.i;
    const int oc = w.shape[0], cg = w.shape[1], kh = w.shape[2], kw = w.shape[3];
    if (groups <= 0 || oc % groups != 0 || x->shape.size() != 4 || x->shape[1] != cg * groups) return false;
    if (ba && ba->attrs.at("data").shape[0] != oc) return false;
    auto pi = op->params.find("padding");
    if (pi == op->params.end()) return false;
    if (pi->second.type == 4) {
        if (pi->second.s == "same") {
            // nn.Conv2d here pads both sides alike: an odd total stays with the function's own kernels
            const long long th = (long long)dh * (kh - 1), tw = (long long)dw * (kw - 1);
            if (sh != 1 || sw != 1 || th % 2 != 0 || tw % 2 != 0 || th > 0x7fffffffLL || tw > 0x7fffffffLL) return false;
            ph = (int)(th / 2);
            pw = (int)(tw / 2);
        } else if (pi->second.s != "valid") {
            return false;
        }
    } else if (!pair_of(op, "padding", ph, pw)) {
        return false;
    }

    Attribute weight = w, bias;
    if (ba) bias = ba->attrs.at("data");
    op->type = "nn.Conv2d";
    op->params.clear();
    op->params["bias"] = ba != nullptr;
    op->params["dilation"] = std::vector<int>{dh, dw};
    op->params["groups"] = groups;
    op->params["in_channels"] = cg * groups;
    op->params["kernel_size"] = std::vector<int>{kh, kw};
    op->params["out_channels"] = oc;
    op->params["padding"] = std::vector<int>{ph, pw};
    op->params["padding_mode"] = "zeros";
    op->params["stride"] = std::vector<int>{sh, sw};
    op->attrs["weight"] = weight;
    if (ba) op->attrs["bias"] = bias;
    op->inputs.resize(1);
    op->inputnames.clear();
    drop_constant(g, wa);
    if (ba) drop_constant(g, ba);
    return true;
}

}  // namespace

int lower_functional_conv(Graph& graph) {
    int lowered = 0;
    const std::vector<Operator*> ops = graph.ops;   // (lowering removes Attribute operators: walk a copy, look only at what is still there)
    for (Operator* op : ops)
        if (std::find(graph.ops.begin(), graph.ops.end(), op) != graph.ops.end() && op->type == "F.conv2d" && lower_one(graph, op)) ++lowered;
    return lowered;
}

}  // namespace pnnx
