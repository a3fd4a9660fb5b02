#include "layout_plan.h"

#include <sstream>

#include "layer/layer_util.h"
#include "si_layout.h"

namespace SimpleInfer {

namespace {

struct Sub {
    long long size, stride;
};
typedef std::vector<Sub> Group;   // one logical dimension: its sub-dimensions, outermost first (none: a dimension of 1)

long long SizeOf(const Group& g) {
    long long n = 1;
    for (const Sub& s : g) n *= s.size;
    return n;
}

std::vector<int> ShapeOf(const std::vector<Group>& g) {
    std::vector<int> s;
    for (const Group& d : g) s.push_back((int)SizeOf(d));
    return s;
}

bool WrapDim(int& dim, int rank) {
    if (dim < 0) dim += rank;
    return dim >= 0 && dim < rank;
}

Status Apply(std::vector<Group>& g, const LayoutOp& op, std::string& why) {
    const int rank = (int)g.size();
    std::ostringstream os;
    switch (op.kind) {
        case LayoutOp::kIdentity: return Status::kSuccess;
        case LayoutOp::kPermute: {
            if ((int)op.args.size() != rank) {
                os << "permute with " << op.args.size() << " dims of a rank-" << rank << " tensor";
                why = os.str();
                return Status::kErrorShape;
            }
            std::vector<Group> out;
            std::vector<bool> seen((size_t)rank, false);
            for (int d : op.args) {
                if (!WrapDim(d, rank) || seen[(size_t)d]) {
                    why = "permute dims are not a permutation of the dimensions";
                    return Status::kErrorShape;
                }
                seen[(size_t)d] = true;
                out.push_back(g[(size_t)d]);
            }
            g.swap(out);
            return Status::kSuccess;
        }
        case LayoutOp::kTranspose: {
            int a = op.args.size() == 2 ? op.args[0] : rank, b = op.args.size() == 2 ? op.args[1] : rank;
            if (!WrapDim(a, rank) || !WrapDim(b, rank)) {
                why = "transpose dims outside the tensor's rank";
                return Status::kErrorShape;
            }
            std::swap(g[(size_t)a], g[(size_t)b]);
            return Status::kSuccess;
        }
        case LayoutOp::kSqueeze: {
            int d = op.args.size() == 1 ? op.args[0] : rank;
            if (!WrapDim(d, rank)) {
                why = "squeeze dim outside the tensor's rank";
                return Status::kErrorShape;
            }
            if (SizeOf(g[(size_t)d]) == 1) g.erase(g.begin() + d);
            return Status::kSuccess;
        }
        case LayoutOp::kUnsqueeze: {
            int d = op.args.size() == 1 ? op.args[0] : rank + 1;
            if (d < 0) d += rank + 1;
            if (d < 0 || d > rank) {
                why = "unsqueeze dim outside the tensor's rank";
                return Status::kErrorShape;
            }
            g.insert(g.begin() + d, Group());
            return Status::kSuccess;
        }
        case LayoutOp::kReshape: {
            long long count = 1, known = 1;
            Group flat;
            for (const Group& d : g)
                for (const Sub& s : d) {
                    count *= s.size;
                    if (s.size == 1) continue;
                    // neighbours that are contiguous with each other (t1 == s2 t2) are ONE run of s1 s2 elements: a boundary may fall anywhere
                    // a divisor of the run allows (a dense [4, 3] -> view(6, 2) moves no byte)
                    if (!flat.empty() && flat.back().stride == s.size * s.stride) {
                        flat.back().size *= s.size;
                        flat.back().stride = s.stride;
                    } else {
                        flat.push_back(s);
                    }
                }
            int hole = -1;
            std::vector<long long> shape;
            for (size_t i = 0; i < op.args.size(); ++i) {
                shape.push_back(op.args[i]);
                if (op.args[i] == -1 && hole < 0) hole = (int)i;
                else if (op.args[i] < 1) {
                    why = "reshape to " + TupleString(op.args) + ": entries are positive, one may be -1";
                    return Status::kErrorShape;
                } else known *= op.args[i];
            }
            if (hole >= 0) {
                if (count % known != 0) {
                    os << "reshape of " << count << " elements to " << TupleString(op.args);
                    why = os.str();
                    return Status::kErrorShape;
                }
                shape[(size_t)hole] = count / known;
                known = count;
            }
            if (known != count || shape.empty()) {
                os << "reshape of " << count << " elements to " << TupleString(op.args);
                why = os.str();
                return Status::kErrorShape;
            }
            std::vector<Group> out;
            size_t at = 0;
            for (long long need : shape) {
                Group d;
                while (need > 1) {
                    Sub& s = flat[at];   // (need > 1 and the counts match: a sub-dimension is left)
                    if (need % s.size == 0) {
                        d.push_back(s);
                        need /= s.size;
                        ++at;
                    } else if (s.size % need == 0) {
                        const long long k = s.size / need;   // the boundary falls inside (s, t): (s / k, t k) goes here, (k, t) stays
                        d.push_back(Sub{need, s.stride * k});
                        s.size = k;
                        need = 1;
                    } else {
                        os << "reshape to " << TupleString(op.args) << ": a boundary falls inside a stored dimension of " << s.size
                           << " that it does not divide (" << need << " elements are wanted there)";
                        why = os.str();
                        return Status::kUnsupport;
                    }
                }
                out.push_back(d);
            }
            g.swap(out);
            return Status::kSuccess;
        }
        default: break;
    }
    why = "unknown layout operator";
    return Status::kFail;
}

}  // namespace

Status PlanLayout(const std::vector<int>& in_shape, int in_ld, const std::vector<LayoutOp>& chain, const std::vector<int>* out_shape,
                  LayoutPlan& plan, std::string& why) {
    plan = LayoutPlan();
    const int rank = (int)in_shape.size();
    if (rank < 1) {
        why = "an input without dimensions";
        return Status::kErrorShape;
    }
    for (int v : in_shape)
        if (v < 1) {
            why = "input shape " + TupleString(in_shape) + " has a non-positive dimension";
            return Status::kErrorShape;
        }
    if (rank > 4) {
        why = "an input of rank " + std::to_string(rank) + " " + TupleString(in_shape) + " would have to exist in memory (rank <= 4 does)";
        plan.late = true;
        return Status::kUnsupport;
    }
    std::vector<Group> g((size_t)rank);
    if (rank == 4) {
        const long long c = in_shape[1], h = in_shape[2], w = in_shape[3], ld = in_ld > 0 ? in_ld : c;
        if (ld < c) {
            why = "a pixel stride below the channel count";
            return Status::kErrorShape;
        }
        g[0].push_back(Sub{in_shape[0], h * w * ld});
        g[1].push_back(Sub{c, 1});
        g[2].push_back(Sub{h, w * ld});
        g[3].push_back(Sub{w, ld});
    } else {
        long long st = 1;
        for (int i = rank - 1; i >= 0; --i) {
            g[(size_t)i].push_back(Sub{in_shape[(size_t)i], st});
            st *= in_shape[(size_t)i];
        }
    }
    for (const LayoutOp& op : chain) {
        const Status s = Apply(g, op, why);
        if (s != Status::kSuccess) return s;
    }
    plan.out_shape = ShapeOf(g);
    if (out_shape && *out_shape != plan.out_shape) {
        why = "the operators give " + TupleString(plan.out_shape) + ", the output operand is " + TupleString(*out_shape);
        return Status::kErrorShape;
    }
    const int orank = (int)g.size();
    if (orank > 4 || orank < 1) {
        why = "an output of rank " + std::to_string(orank) + " " + TupleString(plan.out_shape) + " would have to exist in memory (rank 1..4 does)";
        plan.late = true;
        return Status::kUnsupport;
    }
    std::vector<int> order;
    if (orank == 4) order = {0, 2, 3, 1};
    else
        for (int i = 0; i < orank; ++i) order.push_back(i);
    Group nest;
    for (int d : order)
        for (const Sub& s : g[(size_t)d]) {
            if (s.size == 1) continue;
            if (!nest.empty() && nest.back().stride == s.size * s.stride) {
                nest.back().size *= s.size;
                nest.back().stride = s.stride;
            } else {
                nest.push_back(s);
            }
        }
    for (const Sub& s : nest) {
        plan.dims.push_back((int)s.size);
        plan.in_stride.push_back(s.stride);
    }
    plan.view = nest.empty() || (nest.size() == 1 && nest[0].stride == 1);
    if (nest.size() > 4) {
        why = "the copy is a loop nest of " + std::to_string(nest.size()) + " dimensions (at most 4 are served)";
        plan.late = true;
        return Status::kUnsupport;
    }
    return Status::kSuccess;
}

}  // namespace SimpleInfer

extern "C" int si_layout_plan(int in_rank, const int* in_shape, int in_ld, int n_ops, const int* kinds, const int* nargs, const int* args,
                              int out_rank, const int* out_shape, SiLayoutNest* nest) {
    using namespace SimpleInfer;
    if (!in_shape || !nest || in_rank < 1 || n_ops < 0 || (n_ops > 0 && (!kinds || !nargs)) || out_rank < 0 || (out_rank > 0 && !out_shape))
        return (int)Status::kFail;
    std::vector<LayoutOp> chain;
    const int* at = args;
    for (int k = 0; k < n_ops; ++k) {
        LayoutOp op;
        op.kind = kinds[k];
        if (nargs[k] < 0 || (nargs[k] > 0 && !args)) return (int)Status::kFail;
        op.args.assign(at, at + nargs[k]);
        at += nargs[k];
        chain.push_back(op);
    }
    const std::vector<int> in(in_shape, in_shape + in_rank), out(out_shape, out_shape + out_rank);
    LayoutPlan plan;
    std::string why;
    const Status s = PlanLayout(in, in_ld, chain, out_rank > 0 ? &out : nullptr, plan, why);
    nest->view = plan.view ? 1 : 0;
    nest->rank = (int)plan.dims.size();
    for (int k = 0; k < SI_LAYOUT_MAX_NEST; ++k) {
        nest->dims[k] = k < nest->rank ? plan.dims[(size_t)k] : 0;
        nest->in_stride[k] = k < nest->rank ? plan.in_stride[(size_t)k] : 0;
    }
    return (int)s;
}
