#include "lower_nearest_rows.h"

#include <algorithm>

namespace pnnx {

namespace {

bool is_lookup(const Operator* op) { return op->type == "F.embedding" || op->type == "nn.Embedding"; }

// the fp32 rank-2 data of the pnnx.Attribute behind `r`, else null
const Attribute* constant_table(const Operand* r) {
    if (!r || !r->producer || r->producer->type != "pnnx.Attribute") return nullptr;
    auto data = r->producer->attrs.find("data");
    if (data == r->producer->attrs.end() || data->second.type != 1 || data->second.shape.size() != 2) return nullptr;
    return &data->second;
}

bool norm_is_two(const Operator* cdist) {
    auto p = cdist->params.find("p");
    if (p == cdist->params.end()) return true;   // torch's default
    return (p->second.type == 3 && p->second.f == 2.0f) || (p->second.type == 2 && p->second.i == 2);
}

template <typename T>
void erase_one(std::vector<T*>& from, T* what) {
    auto it = std::find(from.begin(), from.end(), what);
    if (it != from.end()) from.erase(it);
}

// "" and the chain's three operators rewritten into `cdist`, or the condition the chain misses
std::string lower_one(Graph& g, Operator* argmin) {
    if (argmin->inputs.size() != 1 || argmin->outputs.size() != 1) return "takes one operand and gives one";
    Operand* d = argmin->inputs[0];
    Operand* i = argmin->outputs[0];
    Operator* cdist = d->producer;
    if (!cdist || cdist->type != "torch.cdist" || cdist->inputs.size() != 2 || cdist->outputs.size() != 1)
        return "its operand is not the output of torch.cdist: only the argmin of a distance matrix is served";
    auto dim = argmin->params.find("dim");
    if (dim == argmin->params.end() || dim->second.type != 2 || (dim->second.i != -1 && dim->second.i != (int)d->shape.size() - 1))
        return "dim must be the last dimension (the codebook's rows)";
    auto keep = argmin->params.find("keepdim");
    if (keep != argmin->params.end() && !(keep->second.type == 1 && !keep->second.b)) return "keepdim must be False";
    if (!norm_is_two(cdist)) return "torch.cdist [" + cdist->name + "] has p != 2: the fused search is Euclidean";
    if (d->consumers.size() != 1) return "the distances of [" + cdist->name + "] have another reader (or are a graph output): they would have to be written";
    if (i->consumers.size() != 1 || !is_lookup(i->consumers[0]))
        return "the indices must be read by one F.embedding / nn.Embedding and nothing else (not a graph output): the engine has no integer tensors";
    Operator* lookup = i->consumers[0];
    Operand* x2 = cdist->inputs[1];
    const Attribute* codebook = constant_table(x2);
    if (!codebook) return "the second operand of torch.cdist [" + cdist->name + "] is not a rank-2 pnnx.Attribute: the codebook must be a constant";
    if (lookup->outputs.size() != 1) return "[" + lookup->name + "] gives more than one output";
    if (lookup->type == "F.embedding") {
        if (lookup->inputs.size() != 2 || lookup->inputs[0] != i || lookup->inputs[1] != x2)
            return "F.embedding [" + lookup->name + "] reads a different table than torch.cdist [" + cdist->name + "] measured against";
    } else {
        auto w = lookup->attrs.find("weight");
        if (lookup->inputs.size() != 1 || w == lookup->attrs.end() || w->second.type != codebook->type || w->second.shape != codebook->shape ||
            w->second.data != codebook->data)
            return "nn.Embedding [" + lookup->name + "] holds a different table than torch.cdist [" + cdist->name + "] measured against";
    }

    Operand* q = lookup->outputs[0];
    cdist->outputs[0] = q;
    q->producer = cdist;
    cdist->params["nearest_rows"] = 1;
    erase_one(x2->consumers, lookup);   // (F.embedding read the codebook too)
    for (Operand* gone : {d, i}) {
        erase_one(g.operands, gone);
        delete gone;
    }
    for (Operator* gone : {argmin, lookup}) {
        erase_one(g.ops, gone);
        delete gone;
    }
    return "";
}

}  // namespace

int lower_nearest_rows(Graph& graph, std::string* why) {
    int lowered = 0;
    const std::vector<Operator*> ops = graph.ops;   // (lowering removes operators: walk a copy, look only at what is still there)
    for (Operator* op : ops) {
        if (std::find(graph.ops.begin(), graph.ops.end(), op) == graph.ops.end() || op->type != "torch.argmin") continue;
        const std::string name = op->name, miss = lower_one(graph, op);
        if (!miss.empty()) {
            if (why) *why = "torch.argmin [" + name + "]: " + miss;
            return -1;
        }
        ++lowered;
    }
    for (const Operator* op : graph.ops)
        if (is_lookup(op)) {
            if (why) *why = op->type + " [" + op->name + "]: its indices are not the torch.argmin of a torch.cdist against the same table";
            return -1;
        }
    return lowered;
}

}  // namespace pnnx
