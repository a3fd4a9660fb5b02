// engine_plan.cpp -- the planner half of EngineImpl: the launch order (topological), the fusion passes over it, cast insertion for fp16 storage,
// concat aliasing, Detect's side-stream plan and the lifetimes the activation arena is packed by.  Nothing here launches a kernel.
#include <algorithm>

#include "arena_plan.h"
#include "engine_impl.h"
#include "engine_internal.h"
#include "layer/activation.h"
#include "layer/affine_grid.h"
#include "layer/binary_op.h"
#include "layer/cat.h"
#include "layer/conv_1d.h"
#include "layer/conv_2d.h"
#include "layer/conv_transpose_2d.h"
#include "layer/deform_conv_2d.h"
#include "layer/functional_conv_2d.h"
#include "layer/grid_sample.h"
#include "layer/group_norm.h"
#include "layer/layout.h"
#include "layer/linear.h"
#include "layer/lp_norm.h"
#include "layer/max_pool_2d.h"
#include "layer/output_cast.h"
#include "layer/slice.h"
#include "layer/upsample.h"
#include "layer/yolo_detect.h"

namespace SimpleInfer {

namespace {

// built-in operator types whose kernels honour a pixel stride on inputs and outputs
bool HonoursPixelStride(const std::string& type) {
    static const std::set<std::string> ok = {
        "nn.Conv2d", "nn.ConvTranspose2d", "nn.SiLU", "nn.ReLU", "nn.Sigmoid", "nn.Hardsigmoid", "nn.Hardswish", "nn.LeakyReLU",
        "nn.MaxPool2d", "nn.AdaptiveAvgPool2d", "nn.Upsample", "F.interpolate", "F.upsample", "torch.cat", "BinaryOp", "UnaryOp", "nn.BatchNorm2d",
        "nn.GroupNorm", "nn.InstanceNorm2d", "nn.ReflectionPad2d", "nn.ReplicationPad2d", "nn.ZeroPad2d", "nn.ConstantPad2d", "nn.CircularPad2d",
        "F.pad", "nn.Tanh", "nn.AvgPool2d", "F.avg_pool2d", "F.adaptive_avg_pool2d", "nn.Softmax", "nn.LogSoftmax", "nn.Softmax2d",
        "F.softmax", "F.log_softmax", "nn.PixelShuffle", "nn.PixelUnshuffle", "F.pixel_shuffle", "F.pixel_unshuffle", "nn.PReLU", "torch.flatten",
        "torch.chunk", "torch.split", "Tensor.slice", "torch.mean", "torch.sum", "torch.amax", "torch.amin", "F.normalize", "torch.norm", "nn.ReLU6", "F.relu6",
        "nn.Hardtanh", "F.hardtanh", "torch.clamp", "nn.Softplus", "F.softplus", "nn.Mish", "F.mish", "F.relu", "F.silu", "F.sigmoid", "F.hardsigmoid",
        "F.hardswish", "F.leaky_relu", "F.tanh", "models.yolo.Detect", "torchvision.ops.DeformConv2d", "F.grid_sample", "F.affine_grid", "pnnx.Output"};
    return ok.count(type) > 0;
}

}  // namespace

// ---- schedule ------------------------------------------------------------------------------------
Status EngineImpl::CreatePipeline() {
    // Kahn topological order over layer operators, stable w.r.t. file order (pnnx writes operators
    // in execution order, and expression lowering inserts before the expression op)
    std::vector<Step> order;
    std::set<const pnnx::Operand*> ready;
    for (auto& kv : input_tensor_nodes_) ready.insert(kv.second->operand);
    for (auto& kv : tensor_nodes_)
        if (kv.second->constant) ready.insert(kv.second->operand);   // (a graph constant is there before the first step)
    std::vector<const pnnx::Operator*> pending;
    for (pnnx::Operator* op : graph_->ops)
        if (layers_.count(op->name)) pending.push_back(op);
    while (!pending.empty()) {
        bool progressed = false;
        for (auto it = pending.begin(); it != pending.end();) {
            const pnnx::Operator* op = *it;
            bool ok = true;
            for (pnnx::Operand* r : op->inputs) ok = ok && ready.count(r) > 0;
            if (!ok) {
                ++it;
                continue;
            }
            Step s;
            s.layer = layers_[op->name];
            s.op = op;
            order.push_back(s);
            for (pnnx::Operand* r : op->outputs) ready.insert(r);
            it = pending.erase(it);
            progressed = true;
        }
        if (!progressed) {
            LOG(ERROR) << "graph has a cycle or an operand without producer near [" << pending.front()->name << "]";
            return Status::kFail;
        }
    }

    if (opt_.fuse) {
        CHECK_STATUS(FuseEpilogues(order));
        CHECK_STATUS(FuseSiblingConvs(order));
        CHECK_STATUS(FusePoolChains(order));
        if (opt_.fuse_xcorr) CHECK_STATUS(FuseCrossCorrelations(order));   // (before the chains are composed: the views around the call are still single steps)
        if (opt_.fuse_norm) CHECK_STATUS(FuseNormDivisions(order));   // (before the chains are composed: the unsqueeze behind the norm is still a single step)
        if (opt_.fuse_layout) CHECK_STATUS(FuseLayoutChains(order));
        if (opt_.fuse_layout && opt_.fuse_grid) CHECK_STATUS(FuseGridInPlace(order));   // (after the chains are composed: the run in front of a sampler is one step)
        if (opt_.fuse_grid) CHECK_STATUS(FuseAffineGrids(order));
        if (opt_.fuse_const) CHECK_STATUS(FuseConstStages(order));
        if (opt_.fuse_upsample && opt_.alias_cat) CHECK_STATUS(FuseUpsampleIntoConvs(order));   // (fp16 storage too since round 4)
        if (opt_.fp16 && opt_.fuse_stem) CHECK_STATUS(FuseStemPairs(order));
        if (opt_.fp16 && opt_.fuse_stem > 1) CHECK_STATUS(FuseStemTriples(order));
        if (opt_.fp16 && opt_.fuse_pw) CHECK_STATUS(FuseBottleneckPairs(order));
        if (opt_.fp16 && opt_.fuse_pw > 1 && opt_.alias_cat) CHECK_STATUS(FuseCv3IntoPairs(order));
    }
    // what a layout operator could not decide on its own (a tensor of rank > 4 that exists only inside a fused chain) is decided now
    for (const Step& st : order)
        if (Layout* lay = dynamic_cast<Layout*>(st.layer)) CHECK_STATUS(lay->Final());
    if (opt_.fp16) {
        CHECK_STATUS(InsertOutputCasts(order));
        // every layer is asked NOW whether it has a kernel for the storage types it ended up with.  One that has none (a 3x3 conv
        // whose channel count is not a multiple of 32, UnaryOp ...) runs its fp32 kernel between two casts (round 4); only what
        // even that cannot serve makes LoadModel fail -- at load, with the layer and the reason, never at the first Forward
        CHECK_STATUS(InsertFp32Fallbacks(order));
    }
    plan_ = order;
    if (opt_.alias_split) CHECK_STATUS(AliasSplits());   // (first: a chunk that is a view stays one when its halves also feed a concat)
    if (opt_.alias_view) CHECK_STATUS(AliasViews());
    if (opt_.alias_cat) CHECK_STATUS(AliasConcats());
    ResolveAliases();
    if (opt_.detect_stream) CHECK_STATUS(PlanDetectStream());
    return Status::kSuccess;
}

// Option "detect_stream": a Detect level only needs its own feature map, and the two finer maps are final well before the last
// PAN layer.  Each such level is launched on a second stream right after the step that completes its input (fork: an event on
// the main stream), beside the layers that follow; the Detect step launches the remaining level and joins (the main stream
// waits for the side stream's event).  The output tensor is a graph output with its own allocation, so early writes into it
// touch nothing the arena shares.  Under hipGraph capture the side stream joins the capture through the same events.
Status EngineImpl::PlanDetectStream() {
    for (size_t di = 0; di < plan_.size(); ++di) {
        YoloDetect* det = dynamic_cast<YoloDetect*>(plan_[di].layer);
        if (!det) continue;
        if (det->OutputNodes().size() != 1 || !det->OutputNodes()[0]->operand ||
            !output_tensor_nodes_.count(det->OutputNodes()[0]->operand->name))
            continue;   // only when Detect writes a graph output (own buffer)
        unsigned mask = 0;
        std::vector<int> producer(det->InputNodes().size(), -1);
        for (size_t k = 0; k < det->InputNodes().size(); ++k) {
            TensorNode* n = det->InputNodes()[k];
            if (!n || !n->operand || aliases_.count(n->operand->name)) continue;   // a view into a concat buffer has several writers
            bool aliased_into = false;
            for (auto& kv : aliases_) aliased_into = aliased_into || kv.second.parent == n;
            if (aliased_into) continue;
            for (size_t j = 0; j < di; ++j) {
                std::vector<TensorNode*> outs = plan_[j].layer->OutputNodes();
                if (std::find(outs.begin(), outs.end(), n) != outs.end()) producer[k] = (int)j;
            }
            // Worth a fork / join only for a level with real work (MI355X, YOLOv5s same-box A/B: batch 32 +1.3 %, batch 8 +-0,
            // batch 1 -3 %: two more graph edges against launches of a few microseconds)
            const double level_flops = 2.0 * (double)n->tensor.NumElements() * det->num_elements_;
            if (producer[k] >= 0 && producer[k] + 1 < (int)di && (level_flops >= 4e9 || opt_.detect_stream >= 2)) mask |= 1u << k;   // something runs in between
        }
        if (!mask) continue;
        if (!side_context_) {
            side_context_ = new Context;
            CHECK_STATUS(side_context_->Init(context_->device(), opt_.detect_priority));
            SI_TRY_HIP(si_hip_event_create(&ev_fork_), "event create");
            SI_TRY_HIP(si_hip_event_create(&ev_join_), "event create");
        }
        det->SetEarlyLevels(side_context_, mask);
        for (size_t k = 0; k < producer.size(); ++k)
            if ((mask >> k) & 1u) plan_[producer[k]].detect_levels.push_back((int)k);
        LOG(INFO) << "detect_stream: levels mask " << mask << " of [" << plan_[di].op->name << "] launch on the side stream";
    }
    return Status::kSuccess;
}

// ---- fusion passes -------------------------------------------------------------------------------
// What one pass over the launch order works with: where every operator sits, which steps the pass has retired, and the consumer rules the
// passes share.  Positions stay valid for the whole pass: retired steps leave the order only in Compact().
struct EngineImpl::Pass {
    EngineImpl& e;
    std::vector<Step>& order;
    std::map<const pnnx::Operator*, size_t> index;   // operator -> position in order
    std::vector<bool> removed;

    Pass(EngineImpl& engine, std::vector<Step>& o) : e(engine), order(o), removed(o.size(), false) {
        for (size_t i = 0; i < order.size(); ++i) index[order[i].op] = i;
    }

    // the live step at i as layer type T with pnnx type string `type` (null: any type), else null
    template <class T>
    T* At(size_t i, const char* type = nullptr) const {
        if (removed[i] || (type && order[i].op->type != type)) return nullptr;
        return dynamic_cast<T*>(order[i].layer);
    }

    // the scheduled, live, sole consumer of an operand that is not a graph output, else null.  "Live" (removed[]) is FuseEpilogues' rule; the
    // other callers never looked at removed[] for a consumer and are marked (+live): a no-op there, see each call
    const pnnx::Operator* SoleConsumer(const pnnx::Operand* r) const {
        if (e.output_tensor_nodes_.count(r->name)) return nullptr;
        if (r->consumers.size() != 1) return nullptr;
        const pnnx::Operator* c = r->consumers[0];
        auto it = index.find(c);
        if (it == index.end() || removed[it->second]) return nullptr;  // not a layer, or already absorbed
        return c;
    }
    Layer* LayerOf(const pnnx::Operator* c) const { return order[index.at(c)].layer; }

    // ... that is an nn.Conv2d with a launch of its own (not computed by a sibling conv's): its layer, else null
    Conv2d* SoleConvConsumer(const pnnx::Operand* r) const {
        const pnnx::Operator* c = SoleConsumer(r);
        if (!c || c->type != "nn.Conv2d" || e.sibling_ops_.count(c->name)) return nullptr;
        return dynamic_cast<Conv2d*>(LayerOf(c));
    }

    // step i launches nothing any more (folded into another step's launch); `dead`: an operand that no longer exists with it
    void Retire(size_t i, const pnnx::Operand* dead = nullptr) {
        removed[i] = true;
        e.fused_ops_.insert(order[i].op->name);
        if (dead) e.dead_operands_.insert(dead->name);
    }

    // layer -> act  ==>  one launch, for the layers whose epilogue has the activation only (SetFusion(act, param)): the activation's step is
    // retired (it reads nothing else: the fused launch keeps the layer's slot) and the layer at i writes the activation's output
    template <class L>
    void FuseActivationInto(size_t i, L* layer) {
        if (order[i].op->outputs.size() != 1) return;
        const pnnx::Operand* out = order[i].op->outputs[0];
        const pnnx::Operator* c = SoleConsumer(out);
        ActivationLayer* a = c ? dynamic_cast<ActivationLayer*>(LayerOf(c)) : nullptr;
        if (!a || c->inputs.size() != 1 || c->outputs.size() != 1) return;
        layer->SetFusion(a->ActCode(), a->ActCode() == SI_ACT_LEAKYRELU ? a->ActParam() : 0.0f);
        layer->SetOutputNodes({e.tensor_nodes_[c->outputs[0]->name]});
        Retire(index[c], out);
    }

    void Compact() {
        std::vector<Step> out;
        for (size_t i = 0; i < order.size(); ++i)
            if (!removed[i]) out.push_back(order[i]);
        order.swap(out);
    }
};

// conv -> [act] -> [add residual -> [act]]  ==>  one conv launch.  The fused conv runs at the slot of
// the LAST operator of the chain, so a residual produced between the conv and the add is ready.
Status EngineImpl::FuseEpilogues(std::vector<Step>& order) {
    Pass p(*this, order);
    for (size_t i = 0; i < order.size(); ++i) {
        // transposed conv -> act  ==>  one launch (its epilogue has the activation only: a residual add stays a launch of its own)
        if (ConvTranspose2d* ct = p.At<ConvTranspose2d>(i, "nn.ConvTranspose2d")) {
            p.FuseActivationInto(i, ct);
            continue;
        }
        // deformable conv -> act  ==>  one launch, as for the transposed conv
        if (DeformConv2d* dc = p.At<DeformConv2d>(i, "torchvision.ops.DeformConv2d")) {
            p.FuseActivationInto(i, dc);
            continue;
        }
        // temporal conv -> act  ==>  one launch, as for the transposed conv
        if (Conv1d* c1 = p.At<Conv1d>(i, "nn.Conv1d")) {
            p.FuseActivationInto(i, c1);
            continue;
        }
        // F.conv2d with a tensor filter -> act  ==>  one launch, as for the transposed conv
        if (FunctionalConv2d* fc = p.At<FunctionalConv2d>(i, "F.conv2d")) {
            p.FuseActivationInto(i, fc);
            continue;
        }
        // group / instance norm -> act  ==>  one launch (or the same two): the activation runs in the normalise pass's epilogue
        GroupNorm* gn = p.At<GroupNorm>(i, "nn.GroupNorm");
        if (!gn) gn = p.At<GroupNorm>(i, "nn.InstanceNorm2d");
        if (gn) {
            p.FuseActivationInto(i, gn);
            continue;
        }
        Conv2d* conv = p.At<Conv2d>(i, "nn.Conv2d");
        if (!conv || order[i].op->outputs.size() != 1) continue;

        const pnnx::Operand* cur = order[i].op->outputs[0];
        size_t last = i;
        int act1 = SI_ACT_NONE, act2 = SI_ACT_NONE;
        float act_param = 0.f;
        TensorNode* residual = nullptr;
        std::vector<std::pair<size_t, const pnnx::Operand*>> absorbed;   // the steps folded in, each with the operand it read: dead with it

        auto absorb = [&](const pnnx::Operator* c) {
            last = p.index[c];
            absorbed.push_back(std::make_pair(last, cur));
            cur = c->outputs[0];
        };
        auto try_act = [&](int& slot) {
            const pnnx::Operator* c = p.SoleConsumer(cur);
            if (!c) return;
            ActivationLayer* a = dynamic_cast<ActivationLayer*>(p.LayerOf(c));
            if (!a || c->inputs.size() != 1 || c->outputs.size() != 1) return;
            if (slot != SI_ACT_NONE) return;
            if (a->ActCode() == SI_ACT_LEAKYRELU && (act1 == SI_ACT_LEAKYRELU) && act_param != a->ActParam()) return;
            slot = a->ActCode();
            if (a->ActCode() == SI_ACT_LEAKYRELU) act_param = a->ActParam();
            absorb(c);
        };

        try_act(act1);
        {
            const pnnx::Operator* c = p.SoleConsumer(cur);
            BinaryOp* b = c ? dynamic_cast<BinaryOp*>(p.LayerOf(c)) : nullptr;
            if (b && b->binary_op_type_ == BinaryOp::BinaryOpType::kAdd && c->inputs.size() == 2 && c->outputs.size() == 1 &&
                c->inputs[0] != c->inputs[1]) {
                const pnnx::Operand* other = c->inputs[0] == cur ? c->inputs[1] : c->inputs[0];
                const std::vector<int>& so = tensor_nodes_[c->outputs[0]->name]->tensor.Shape();
                const bool same = IsSameShape(tensor_nodes_[other->name]->tensor.Shape(), so) &&
                                  IsSameShape(tensor_nodes_[cur->name]->tensor.Shape(), so);
                if (same) {
                    residual = tensor_nodes_[other->name];
                    absorb(c);
                    try_act(act2);
                }
            }
        }
        if (absorbed.empty()) continue;

        conv->SetFusion(act1, residual, act2, act_param);
        conv->SetOutputNodes({tensor_nodes_[cur->name]});
        for (auto& a : absorbed) p.Retire(a.first, a.second);
        if (last != i) {   // (the index is not updated: the conv's operator still maps to slot i, which reads as retired from here on)
            order[last] = order[i];
            p.removed[last] = false;
            p.removed[i] = true;
        }
    }
    p.Compact();
    return Status::kSuccess;
}

// BinaryOp(x, c0) -> BinaryOp(., c1), c0 and c1 graph constants (FrozenBatchNorm2d's x * scale + shift): one two-stage launch of the
// constant-operand kernel (include/si_binary.h) at the first operator's slot.  x is read once and the result written once; the kernel rounds
// after each stage exactly as the two launches do, so the bits are those of fuse_const = 0.  The second step is retired and the operand between
// the two is dead.  (Folding the constants into a preceding conv's weights and bias would save the launch altogether but changes rounding: not done.)
Status EngineImpl::FuseConstStages(std::vector<Step>& order) {
    Pass p(*this, order);
    for (size_t i = 0; i < order.size(); ++i) {
        BinaryOp* a = p.At<BinaryOp>(i, "BinaryOp");
        if (!a || !a->ConstForm() || a->Stages() != 1 || order[i].op->outputs.size() != 1) continue;
        const pnnx::Operand* mid = order[i].op->outputs[0];
        const pnnx::Operator* c = p.SoleConsumer(mid);
        BinaryOp* b = c ? dynamic_cast<BinaryOp*>(p.LayerOf(c)) : nullptr;
        if (!b || c->type != "BinaryOp" || c->outputs.size() != 1 || !a->CanAbsorb(*b, tensor_nodes_[mid->name])) continue;
        a->Absorb(*b);
        a->SetOutputNodes({tensor_nodes_[c->outputs[0]->name]});
        p.Retire(p.index[c], mid);
    }
    p.Compact();
    return Status::kSuccess;
}

// Two 1x1 convs reading the same operand with the same geometry (YOLOv5 C3: cv1 and cv2) become one launch with
// twice the output channels and a split destination: the input is read once and the launch has twice the tiles.
Status EngineImpl::FuseSiblingConvs(std::vector<Step>& order) {
    Pass p(*this, order);
    for (size_t i = 0; i < order.size(); ++i) {
        Conv2d* a = p.At<Conv2d>(i, "nn.Conv2d");
        if (!a || a->InputNodes().size() != 1 || a->OutputNodes().size() != 1) continue;
        for (size_t j = i + 1; j < order.size(); ++j) {
            Conv2d* b = p.At<Conv2d>(j, "nn.Conv2d");
            if (!b || b->InputNodes().size() != 1 || b->OutputNodes().size() != 1) continue;
            if (a->InputNodes()[0] != b->InputNodes()[0] || !a->CanFuseSibling(*b)) continue;
            const std::vector<int>& sa = a->OutputNodes()[0]->tensor.Shape();
            const std::vector<int>& sb = b->OutputNodes()[0]->tensor.Shape();
            if (sa.size() != 4 || sb.size() != 4 || sa[0] != sb[0] || sa[1] != sb[1] || sa[2] != sb[2]) continue;
            a->SetSibling(b);
            a->SetOutputNodes({a->OutputNodes()[0], b->OutputNodes()[0]});
            p.removed[j] = true;   // (not Retire: a secondary is recorded in sibling_ops_, which the later passes consult, not in fused_ops_)
            sibling_ops_.insert(order[j].op->name);
            break;
        }
    }
    p.Compact();
    return Status::kSuccess;
}

// SPPF: maxpool5 -> maxpool5 -> maxpool5 (each fed by the previous one, every intermediate also read by the concat)
// ==> one launch at the first pool's slot that reads the input once and writes all three operands.
Status EngineImpl::FusePoolChains(std::vector<Step>& order) {
    Pass p(*this, order);
    auto pool_at = [&](size_t i) -> MaxPool2d* {
        MaxPool2d* m = p.At<MaxPool2d>(i);   // (by layer class alone: this pass never looked at the type string)
        return (m && m->InputNodes().size() == 1 && m->OutputNodes().size() == 1 && m->chain_.empty()) ? m : nullptr;
    };
    auto follower = [&](size_t from, MaxPool2d* head) -> size_t {
        for (size_t j = from + 1; j < order.size(); ++j) {
            MaxPool2d* m = pool_at(j);
            if (m && m->InputNodes()[0] == head->OutputNodes()[0] && head->ChainHead(*m) &&
                IsSameShape(m->OutputNodes()[0]->tensor.Shape(), head->OutputNodes()[0]->tensor.Shape()))
                return j;
        }
        return 0;
    };
    for (size_t i = 0; i < order.size(); ++i) {
        MaxPool2d* a = pool_at(i);
        if (!a || !IsSameShape(a->InputNodes()[0]->tensor.Shape(), a->OutputNodes()[0]->tensor.Shape())) continue;
        const size_t j = follower(i, a);
        if (j == 0) continue;
        MaxPool2d* b = pool_at(j);
        const size_t k = follower(j, b);
        if (k == 0) continue;
        MaxPool2d* c = pool_at(k);
        a->SetChain(b, c);
        a->SetOutputNodes({a->OutputNodes()[0], b->OutputNodes()[0], c->OutputNodes()[0]});
        p.Retire(j);
        p.Retire(k);
    }
    p.Compact();
    return Status::kSuccess;
}

// A maximal run of layout operators (Tensor.permute / reshape / view / torch.transpose / squeeze / unsqueeze / contiguous) in which every
// intermediate has exactly one reader and is not a graph output  ==>  ONE layout step at the last operator's slot that reads the run's root
// input and carries the composed chain (layer/layout.h).  The intermediates never exist in memory, so they may have any rank (the raw YOLOv5
// head's view -> permute -> view passes through rank 5).  A chain the algebra cannot serve as a whole is left as it was.
Status EngineImpl::FuseLayoutChains(std::vector<Step>& order) {
    Pass p(*this, order);
    for (size_t i = 0; i < order.size(); ++i) {
        Layout* head = p.At<Layout>(i);
        if (!head || head->InputNodes().size() != 1 || order[i].op->outputs.size() != 1) continue;
        std::vector<LayoutOp> ops = head->Chain();
        std::vector<size_t> run(1, i);
        for (;;) {
            const pnnx::Operator* c = p.SoleConsumer(order[run.back()].op->outputs[0]);
            Layout* next = c ? dynamic_cast<Layout*>(p.LayerOf(c)) : nullptr;
            if (!next || c->inputs.size() != 1 || c->outputs.size() != 1 || next->InputNodes().size() != 1) break;
            ops.insert(ops.end(), next->Chain().begin(), next->Chain().end());
            run.push_back(p.index[c]);
        }
        if (run.size() < 2) continue;
        Layout* last = dynamic_cast<Layout*>(order[run.back()].layer);
        if (!last->TryChain(head->InputNodes()[0], ops)) continue;
        for (size_t k = 0; k + 1 < run.size(); ++k) p.Retire(run[k], order[run[k]].op->outputs[0]);
    }
    p.Compact();
    return Status::kSuccess;
}

// x.view(1, N C, H, W), z.view(N C, 1, kh, kw) -> F.conv2d(groups = N C) -> .view(N, C, Ho, Wo)  ==>  ONE launch of the depthwise kernel in
// its per-sample addressing (include/si_xcorr.h) on x and z themselves: the depthwise cross-correlation of SiamRPN++, SiamMask, SiamBAN and
// Ocean.  In NHWC storage each of the three views is a transpose launch for N > 1 (the batch is folded into the contiguous axis); the kernel
// instead takes the filter of image n from image n of z, [N][kh][kw][C] as it lies, and writes [N][Ho][Wo][C].  The arithmetic per output
// element is that of the unfused addressing, tap by tap, so the bits are those of fuse_xcorr = 0.  Conditions: each view is a single
// Tensor.view / Tensor.reshape step, every intermediate has one reader and is no graph output, and the shapes are exactly the pattern's
// (FunctionalConv2d::SetPerSample checks them).  The three layout steps are retired, the operands between them are dead.
Status EngineImpl::FuseCrossCorrelations(std::vector<Step>& order) {
    Pass p(*this, order);
    auto view_step = [&](const pnnx::Operator* op) -> Layout* {
        if (!op || (op->type != "Tensor.view" && op->type != "Tensor.reshape") || op->inputs.size() != 1 || op->outputs.size() != 1) return nullptr;
        auto at = p.index.find(op);
        return at == p.index.end() ? nullptr : p.At<Layout>(at->second);
    };
    for (size_t i = 0; i < order.size(); ++i) {
        FunctionalConv2d* fc = p.At<FunctionalConv2d>(i, "F.conv2d");
        const pnnx::Operator* op = order[i].op;
        if (!fc || fc->PerSample() || op->inputs.size() < 2 || op->outputs.size() != 1 || fc->InputNodes().size() != op->inputs.size()) continue;
        const pnnx::Operand* xv = op->inputs[0];
        const pnnx::Operand* zv = op->inputs[1];
        const pnnx::Operand* yv = op->outputs[0];
        if (!xv || !zv || xv == zv || p.SoleConsumer(xv) != op || p.SoleConsumer(zv) != op) continue;
        if (fc->InputNodes()[0] != tensor_nodes_[xv->name] || fc->InputNodes()[1] != tensor_nodes_[zv->name]) continue;
        if (fc->OutputNodes().size() != 1 || fc->OutputNodes()[0] != tensor_nodes_[yv->name]) continue;   // (an absorbed activation: not the pattern)
        const pnnx::Operator* back = p.SoleConsumer(yv);
        Layout* lx = view_step(xv->producer);
        Layout* lz = view_step(zv->producer);
        Layout* ly = view_step(back);
        if (!lx || !lz || !ly) continue;
        TensorNode* x = lx->InputNodes().size() == 1 ? lx->InputNodes()[0] : nullptr;
        TensorNode* z = lz->InputNodes().size() == 1 ? lz->InputNodes()[0] : nullptr;
        TensorNode* out = ly->OutputNodes().size() == 1 ? ly->OutputNodes()[0] : nullptr;
        if (!x || !z || !out || x == z) continue;
        if (x->tensor.GetDataType() != z->tensor.GetDataType() || x->tensor.GetDataType() != out->tensor.GetDataType()) continue;
        if (!fc->SetPerSample(x, z, out)) continue;
        p.Retire(p.index[xv->producer], xv);
        p.Retire(p.index[zv->producer], zv);
        // (the launch keeps the conv's slot: x and z are ready before their views were, and nothing between the conv and the view behind it
        // reads or writes `out`)
        p.Retire(p.index[back], yv);
    }
    p.Compact();
    return Status::kSuccess;
}

// n = torch.norm(x, p, dim = d, keepdim = K) -> [K false: torch.unsqueeze(n, d)] -> BinaryOp div(x, .)  ==>  ONE launch of the Lp-norm kernel
// with normalize = 1, eps = 0 (include/si_lpnorm.h): F.normalize written out, as SuperPoint's descriptor head does.  The kernel divides every
// element by the same float32 norm with the same IEEE division BinaryOp uses, so in fp32 the bits are those of fuse_norm = 0; under fp16
// storage the unfused plan rounds the norm to a half in between and the fused one does not.  Conditions: one reduced dim, the unsqueeze puts
// it back where it was, the division's first operand is the norm's own input and its second the (unsqueezed) norm, and the norm and the
// unsqueezed norm have no other reader and are no graph outputs.  The launch keeps the norm's slot (x is ready there and nothing in between
// touches the quotient); the unsqueeze and the division are retired, the operands between the three are dead and no norm tensor is written.
Status EngineImpl::FuseNormDivisions(std::vector<Step>& order) {
    Pass p(*this, order);
    for (size_t i = 0; i < order.size(); ++i) {
        LpNorm* ln = p.At<LpNorm>(i, "torch.norm");
        const pnnx::Operator* op = order[i].op;
        if (!ln || ln->Normalizes() || ln->dims_.size() != 1 || op->inputs.size() != 1 || op->outputs.size() != 1) continue;
        const pnnx::Operand* x = op->inputs[0];
        const pnnx::Operand* norm = op->outputs[0];
        if (ln->InputNodes().size() != 1 || ln->InputNodes()[0] != tensor_nodes_[x->name]) continue;
        const int rank = (int)ln->InputNodes()[0]->tensor.Shape().size();
        const int dim = ln->dims_[0] < 0 ? ln->dims_[0] + rank : ln->dims_[0];
        const pnnx::Operand* divisor = norm;
        const pnnx::Operator* unsq = nullptr;
        const pnnx::Operator* next = p.SoleConsumer(norm);
        if (!ln->keepdim_) {
            int at = 0;
            if (!next || next->type != "torch.unsqueeze" || next->inputs.size() != 1 || next->outputs.size() != 1 || !p.At<Layout>(p.index[next]) ||
                !Get(next, "dim", at) || (at < 0 ? at + rank : at) != dim)
                continue;
            unsq = next;
            divisor = next->outputs[0];
            next = p.SoleConsumer(divisor);
        }
        BinaryOp* div = next ? dynamic_cast<BinaryOp*>(p.LayerOf(next)) : nullptr;
        if (!div || next->type != "BinaryOp" || div->binary_op_type_ != BinaryOp::BinaryOpType::kDiv || div->with_scalar_ || div->ConstForm() ||
            next->inputs.size() != 2 || next->outputs.size() != 1 || next->inputs[0] != x || next->inputs[1] != divisor)
            continue;
        TensorNode* out = tensor_nodes_[next->outputs[0]->name];
        // (whatever storage types x and the quotient have: the planner's later passes treat the launch as they treat F.normalize in that place)
        if (!out || !ln->SetNormalize(out)) continue;
        if (unsq) p.Retire(p.index[unsq], norm);
        p.Retire(p.index[next], divisor);
        if (!unsq) dead_operands_.insert(norm->name);
    }
    p.Compact();
    return Status::kSuccess;
}

// x.permute(0, 2, 3, 1) -> F.grid_sample(., grid)  ==>  the sampler reads the grid IN PLACE.  A rank-4 tensor is stored as dimensions
// (0, 2, 3, 1), so the logical grid [N, Ho, Wo, 2] behind the permute would be moved into [N][Wo][2][Ho] order by a transpose launch, the two
// coordinates of a pixel Ho elements apart -- while the tensor in front of it, [N, 2, Ho, Wo] stored NHWC, already has torch's dense grid
// bytes.  When the grid operand is written by a layout step (a run composed by FuseLayoutChains, or a single operator) that only the sampler
// reads, that is no graph output, and whose chain from its rank-4 root composes to exactly the permutation (0, 2, 3, 1) (permutes,
// transposes and Tensor.contiguous; anything else leaves the plan alone), the layout step is retired and the sampler is pointed at the root.
Status EngineImpl::FuseGridInPlace(std::vector<Step>& order) {
    Pass p(*this, order);
    for (size_t i = 0; i < order.size(); ++i) {
        GridSample* gs = p.At<GridSample>(i, "F.grid_sample");
        if (!gs || gs->Form() != GridSample::GridForm::kStored || order[i].op->inputs.size() != 2 || gs->InputNodes().size() != 2) continue;
        const pnnx::Operand* grid = order[i].op->inputs[1];
        if (!grid || !grid->producer || tensor_nodes_[grid->name] != gs->InputNodes()[1] || p.SoleConsumer(grid) != order[i].op) continue;
        auto at = p.index.find(grid->producer);
        if (at == p.index.end()) continue;
        Layout* lay = p.At<Layout>(at->second);
        if (!lay || lay->InputNodes().size() != 1 || lay->OutputNodes().size() != 1 || lay->OutputNodes()[0] != gs->InputNodes()[1]) continue;
        TensorNode* root = lay->InputNodes()[0];
        if (root->tensor.Shape().size() != 4) continue;
        int perm[4] = {0, 1, 2, 3};   // perm[j]: the root dimension that result dimension j is
        bool ok = true;
        for (const LayoutOp& op : lay->Chain()) {
            auto norm = [](int d) { return d < 0 ? d + 4 : d; };
            if (op.kind == LayoutOp::kIdentity) continue;
            if (op.kind == LayoutOp::kPermute && op.args.size() == 4) {
                int next[4];
                for (int j = 0; j < 4 && ok; ++j) {
                    const int d = norm(op.args[(size_t)j]);
                    ok = d >= 0 && d < 4;
                    if (ok) next[j] = perm[d];
                }
                for (int j = 0; j < 4 && ok; ++j) perm[j] = next[j];
            } else if (op.kind == LayoutOp::kTranspose && op.args.size() == 2) {
                const int a = norm(op.args[0]), b = norm(op.args[1]);
                ok = a >= 0 && a < 4 && b >= 0 && b < 4;
                if (ok) std::swap(perm[a], perm[b]);
            } else {
                ok = false;
            }
            if (!ok) break;
        }
        if (!ok || perm[0] != 0 || perm[1] != 2 || perm[2] != 3 || perm[3] != 1) continue;
        if (!gs->SetGridInPlace(root)) continue;
        p.Retire(at->second, grid);
    }
    p.Compact();
    return Status::kSuccess;
}

// F.affine_grid(theta) -> F.grid_sample(x, .)  ==>  ONE launch: the sampler computes the coordinates from theta (include/si_grid.h, the theta
// source) and the grid is never written.  Conditions: the grid has the sampler as its only reader and is no graph output, and both operators
// have the same align_corners (the kernel's theta source has one flag; torch warns about the other combination).  Spatial transformer
// networks: Linear -> view(N, 2, 3) -> affine_grid -> grid_sample.
Status EngineImpl::FuseAffineGrids(std::vector<Step>& order) {
    Pass p(*this, order);
    for (size_t i = 0; i < order.size(); ++i) {
        AffineGrid* ag = p.At<AffineGrid>(i, "F.affine_grid");
        if (!ag || ag->InputNodes().size() != 1 || order[i].op->outputs.size() != 1) continue;
        const pnnx::Operand* grid = order[i].op->outputs[0];
        const pnnx::Operator* c = p.SoleConsumer(grid);
        if (!c || c->type != "F.grid_sample" || c->inputs.size() != 2 || c->inputs[1] != grid || c->inputs[0] == grid) continue;
        GridSample* gs = dynamic_cast<GridSample*>(p.LayerOf(c));
        if (!gs || gs->Form() != GridSample::GridForm::kStored || gs->align_corners_ != ag->align_corners_) continue;
        if (gs->InputNodes().size() != 2 || gs->InputNodes()[1] != tensor_nodes_[grid->name]) continue;
        if (!gs->SetTheta(ag->InputNodes()[0])) continue;
        p.Retire(i, grid);
    }
    p.Compact();
    return Status::kSuccess;
}

// nn.Upsample(nearest) -> torch.cat(dim = channels) -> 1x1 convs only  ==>  the upsample launch disappears: every consumer conv
// reads the upsampled channel range from the LOW-RESOLUTION tensor at the nearest-neighbour source pixel (dual-source A rows,
// si_hip_conv2d_upcat_f32), with the reference's index rule (src/layer/upsample.cpp:85-92), so the results are bit-identical to
// the unfused schedule.  YOLOv5s: both upsamples of the PAN top-down path (20x20x256 -> 40x40, 40x40x128 -> 80x80): 131 MB per
// batch-32 forward that are neither written nor read back.  Requires concat aliasing (the cat then has nothing to copy for that
// input) and fp32 storage.
Status EngineImpl::FuseUpsampleIntoConvs(std::vector<Step>& order) {
    Pass p(*this, order);
    for (size_t i = 0; i < order.size(); ++i) {
        Upsample* up = p.At<Upsample>(i, "nn.Upsample");
        if (!up || up->InputNodes().size() != 1 || up->OutputNodes().size() != 1) continue;
        if (!up->IsNearestByScale()) continue;   // (bilinear, size=: the dual-source conv kernels implement the nearest-by-scale index rule only)
        const pnnx::Operand* u = up->OutputNodes()[0]->operand;
        const pnnx::Operator* cat = u ? p.SoleConsumer(u) : nullptr;   // (+live: this pass retires upsamples only, never a cat)
        if (!cat || cat->type != "torch.cat" || cat->outputs.size() != 1) continue;
        Cat* cat_layer = dynamic_cast<Cat*>(p.LayerOf(cat));
        if (!cat_layer || cat_layer->NhwcAxis() != 3) continue;
        const std::vector<int>& us = up->OutputNodes()[0]->tensor.Shape();
        if (us.size() != 4) continue;
        // channel offset of the upsampled tensor inside the concat
        int c0 = 0;
        bool found = false;
        for (const pnnx::Operand* r : cat->inputs) {
            if (r == u) { found = true; break; }
            const std::vector<int>& rs = tensor_nodes_[r->name]->tensor.Shape();
            if (rs.size() != 4) { found = false; break; }
            c0 += rs[3];
        }
        if (!found) continue;
        const pnnx::Operand* co = cat->outputs[0];
        if (output_tensor_nodes_.count(co->name) || co->consumers.empty()) continue;
        // every reader of the concat must be a pointwise conv that can take the dual-source form (a sibling-fused secondary has
        // left the order: its primary reads the same operand)
        std::vector<Conv2d*> readers;
        bool ok = true;
        for (const pnnx::Operator* c : co->consumers) {
            if (!c || c->type != "nn.Conv2d") { ok = false; break; }
            if (sibling_ops_.count(c->name)) continue;
            Conv2d* conv = p.index.count(c) ? dynamic_cast<Conv2d*>(p.LayerOf(c)) : nullptr;
            if (!conv || conv->UpsampledSource() || !conv->CanReadUpsampledFrom(up->InputNodes()[0], c0, up->scale_factor_h_, up->scale_factor_w_)) { ok = false; break; }
            readers.push_back(conv);
        }
        // ... and every sibling-fused secondary must have its primary among them
        for (const pnnx::Operator* c : co->consumers) {
            if (!ok || !c || !sibling_ops_.count(c->name)) continue;
            bool has_primary = false;
            for (Conv2d* r : readers) has_primary = has_primary || (r->Sibling() && r->Sibling()->GetOp() == c);
            ok = has_primary;
        }
        if (!ok || readers.empty()) continue;
        for (Conv2d* r : readers) r->SetUpsampledSource(up->InputNodes()[0], c0, up->scale_factor_h_, up->scale_factor_w_);
        p.Retire(i);
    }
    p.Compact();
    return Status::kSuccess;
}

// fp16 storage (round 4): the RGB stem conv (fp32 image in, 32 half channels out) whose ONLY reader is a 3x3 stride-2 conv over those
// 32 channels -- YOLOv5's conv_0 -> conv_1 -- becomes one launch at the second conv's slot (si_hip_conv2d_stem_s2c32_f16): the
// intermediate (210 MB at batch 32) is computed tile by tile in LDS and never written.  The stem's step leaves the order, its
// operand is never allocated; the kernel is asked NOW, with the bound shapes, whether it takes the pair.
Status EngineImpl::FuseStemPairs(std::vector<Step>& order) {
    Pass p(*this, order);
    for (size_t i = 0; i < order.size(); ++i) {
        Conv2d* stem = p.At<Conv2d>(i, "nn.Conv2d");
        if (!stem || stem->InputNodes().size() != 1 || stem->OutputNodes().size() != 1) continue;
        const pnnx::Operand* img = stem->InputNodes()[0]->operand;
        const pnnx::Operand* mid = stem->OutputNodes()[0]->operand;
        if (!img || !mid || !input_tensor_nodes_.count(img->name)) continue;
        Conv2d* conv = p.SoleConvConsumer(mid);   // (+live: a retired step here reads a graph input, and mid is none)
        if (!conv || !conv->CanFuseStemProducer(*stem)) continue;
        conv->SetStemProducer(stem);
        p.Retire(i, mid);
    }
    p.Compact();
    return Status::kSuccess;
}

// fp16 storage (round 6): the conv that took the stem (FuseStemPairs) and the 1x1 conv over its 64 channels that is its only reader -- with the
// sibling that conv computes as well: YOLOv5's first C3 reads the tensor twice, cv1 and cv2, which FuseSiblingConvs has made ONE conv -- become
// one launch at the 1x1 conv's slot (si_hip_conv2d_stem_s2c32_pw_f16); the 64-channel tensor between them is never allocated.
Status EngineImpl::FuseStemTriples(std::vector<Step>& order) {
    Pass p(*this, order);
    for (size_t i = 0; i < order.size(); ++i) {
        Conv2d* c1 = p.At<Conv2d>(i, "nn.Conv2d");
        if (!c1 || !c1->StemProducer() || c1->OutputNodes().size() != 1) continue;
        const pnnx::Operand* mid = c1->OutputNodes()[0]->operand;
        if (!mid || output_tensor_nodes_.count(mid->name) || mid->consumers.empty()) continue;
        // every reader of `mid` is the same scheduled 1x1 conv or the sibling it computes (several readers: not the sole-consumer rule)
        Conv2d* pw = nullptr;
        bool ok = true;
        for (const pnnx::Operator* c : mid->consumers) {
            if (!c || c->type != "nn.Conv2d") { ok = false; break; }
            if (sibling_ops_.count(c->name)) continue;
            if (!p.index.count(c) || pw) { ok = false; break; }
            pw = dynamic_cast<Conv2d*>(p.LayerOf(c));
        }
        if (!ok || !pw) continue;
        for (const pnnx::Operator* c : mid->consumers)
            if (sibling_ops_.count(c->name) && (!pw->Sibling() || pw->Sibling()->GetOp() != c)) ok = false;
        if (!ok || !pw->CanFuseStemPairProducer(*c1)) continue;
        pw->SetStemPairProducer(c1);
        p.Retire(i, mid);
    }
    p.Compact();
    return Status::kSuccess;
}

// fp16 storage (round 5): conv A (1x1, c -> c, SiLU) whose ONLY consumer is conv B (3x3 s1 p1 over c channels that the slab kernel
// serves, SiLU, optional shortcut) -- the C3 bottleneck's pair -- becomes one launch at B's slot; A's output is never allocated.
Status EngineImpl::FuseBottleneckPairs(std::vector<Step>& order) {
    Pass p(*this, order);
    for (size_t i = 0; i < order.size(); ++i) {
        Conv2d* pw = p.At<Conv2d>(i, "nn.Conv2d");
        if (!pw || pw->InputNodes().size() != 1 || pw->OutputNodes().size() != 1) continue;
        const pnnx::Operand* mid = pw->OutputNodes()[0]->operand;
        if (!mid || sibling_ops_.count(order[i].op->name)) continue;
        Conv2d* conv = p.SoleConvConsumer(mid);   // (+live: the consumer sits behind i in the order, retired steps at or before i)
        if (!conv || !conv->CanFusePointwiseProducer(*pw)) continue;
        conv->SetPointwiseProducer(pw);
        p.Retire(i, mid);
    }
    p.Compact();
    return Status::kSuccess;
}

// fp16 storage (round 6): torch.cat([y, z], channels) -> 1x1 conv (a YOLOv5 C3's closing cv3) where y is the output of a fused bottleneck pair
// (FuseBottleneckPairs) that only the concat reads: the pair, the concat and the conv become ONE launch at the conv's slot
// (si_hip_conv2d_pw_cv3_f16); y and the concat operand are never allocated, z keeps a buffer of its own (nothing aliases into a concat
// that no longer exists).
Status EngineImpl::FuseCv3IntoPairs(std::vector<Step>& order) {
    Pass p(*this, order);
    for (size_t i = 0; i < order.size(); ++i) {
        Cat* cat = p.At<Cat>(i, "torch.cat");
        if (!cat || cat->NhwcAxis() != 3 || order[i].op->inputs.size() != 2 || order[i].op->outputs.size() != 1) continue;
        const pnnx::Operand* y = order[i].op->inputs[0];
        const pnnx::Operand* z = order[i].op->inputs[1];
        const pnnx::Operand* cc = order[i].op->outputs[0];
        if (!y || !z || !cc || y == z || output_tensor_nodes_.count(y->name) || y->consumers.size() != 1) continue;
        // the scheduled step that WRITES y: after the epilogue fusion that is the conv whose output node y's is (y's pnnx producer is then the
        // folded SiLU / add operator, which no longer has a step)
        size_t pi = order.size();
        for (size_t j = 0; j < i && pi == order.size(); ++j)
            if (!p.removed[j])
                for (TensorNode* n : order[j].layer->OutputNodes())
                    if (n && n->operand == y) pi = j;
        if (pi == order.size()) continue;
        Conv2d* pair = dynamic_cast<Conv2d*>(order[pi].layer);
        Conv2d* conv = p.SoleConvConsumer(cc);   // (+live: the consumer sits behind i in the order, retired steps at or before i)
        if (!pair || !conv || !pair->PointwiseProducer() || pair->OutputNodes().size() != 1) continue;
        TensorNode* zn = tensor_nodes_[z->name];
        if (!conv->CanFuseCv3Pair(*pair, zn)) continue;
        conv->SetCv3Pair(pair, zn);
        p.Retire(pi, y);
        p.Retire(i, cc);
    }
    p.Compact();
    return Status::kSuccess;
}

// fp16 storage: graph outputs keep the file's fp32 type.  Conv2d / Linear / Detect write fp32 from their own epilogue;
// any other producer fed by half operands writes a half staging operand instead, and a convert step follows it.
Status EngineImpl::InsertOutputCasts(std::vector<Step>& order) {
    for (auto& kv : output_tensor_nodes_) {
        TensorNode* out = kv.second;
        if (out->tensor.GetDataType() != DataType::kFloat32) continue;
        for (size_t i = 0; i < order.size(); ++i) {
            Layer* layer = order[i].layer;
            std::vector<TensorNode*> outs = layer->OutputNodes();
            auto slot = std::find(outs.begin(), outs.end(), out);
            if (slot == outs.end()) continue;
            if (dynamic_cast<Conv2d*>(layer) || dynamic_cast<Linear*>(layer) || dynamic_cast<YoloDetect*>(layer)) break;
            bool half_in = false;
            for (const TensorNode* in : layer->InputNodes()) half_in = half_in || in->tensor.GetDataType() == DataType::kFloat16;
            if (!half_in) break;

            const std::string staging_name = kv.first + "#f16";
            TensorNode* staging = new TensorNode;
            staging->operand = out->operand;
            staging->tensor = Tensor(DataType::kFloat16, out->tensor.Shape(), MemoryType::kDevice, false);
            tensor_nodes_[staging_name] = staging;
            *slot = staging;
            layer->SetOutputNodes(outs);

            OutputCast* cast = new OutputCast(order[i].op->name);
            layers_[cast->GetOp()->name] = cast;
            cast->SetContext(context_);
            cast->SetInputNodes({staging});
            cast->SetOutputNodes({out});
            CHECK_STATUS(cast->Validate());
            Step s;
            s.layer = cast;
            s.op = cast->GetOp();
            order.insert(order.begin() + i + 1, s);
            break;
        }
    }
    return Status::kSuccess;
}

// fp16 storage, a layer without an fp16 kernel: its half operands get fp32 SHADOW tensors -- a cast step in front of the layer
// for every half tensor it reads (inputs, a fused residual), one behind it for every half tensor it writes -- and the layer runs
// the kernel it has.  What the reference computes in fp32 (src/layer/conv_2d.cpp:94-101 rejects anything else) is then computed
// in fp32 here too; the neighbours keep their fp16 storage.
Status EngineImpl::InsertFp32Fallbacks(std::vector<Step>& order) {
    int serial = 0;
    for (size_t i = 0; i < order.size(); ++i) {
        Layer* layer = order[i].layer;
        std::string why;
        if (layer->HalfStorageOk(why)) continue;
        const std::string lname = order[i].op->name;
        auto refuse = [&](const std::string& more) {
            LOG(ERROR) << "fp16 storage: layer [" << lname << "] (" << order[i].op->type << ") cannot run: " << why << more
                       << "; load the model without the fp16 option";
            return Status::kUnsupport;
        };
        auto shadow_of = [&](TensorNode* n, const char* tag) {
            TensorNode* sh = new TensorNode;
            sh->operand = n->operand;
            sh->tensor = Tensor(DataType::kFloat32, n->tensor.Shape(), MemoryType::kDevice, false);
            tensor_nodes_[(n->operand ? n->operand->name : lname) + "#" + tag + std::to_string(serial++)] = sh;
            return sh;
        };
        std::vector<Step> before, after;
        auto cast_step = [&](TensorNode* from, TensorNode* to, const char* suffix, std::vector<Step>& where) -> Status {
            OutputCast* cast = new OutputCast(lname, (std::string(suffix) + std::to_string(serial++)).c_str());
            layers_[cast->GetOp()->name] = cast;
            cast->SetContext(context_);
            cast->SetInputNodes({from});
            cast->SetOutputNodes({to});
            CHECK_STATUS(cast->Validate());
            Step s;
            s.layer = cast;
            s.op = cast->GetOp();
            where.push_back(s);
            return Status::kSuccess;
        };
        std::map<TensorNode*, TensorNode*> in_shadow;
        std::vector<TensorNode*> ins = layer->InputNodes(), outs = layer->OutputNodes(), extra;
        layer->ExtraReads(extra);
        for (TensorNode*& n : ins) {
            if (n->tensor.GetDataType() != DataType::kFloat16) continue;
            if (!in_shadow.count(n)) {
                in_shadow[n] = shadow_of(n, "f32in");
                CHECK_STATUS(cast_step(n, in_shadow[n], ".in_to_f32.", before));
            }
            n = in_shadow[n];
        }
        for (TensorNode* n : extra) {
            if (n->tensor.GetDataType() != DataType::kFloat16) continue;
            if (!in_shadow.count(n)) {
                in_shadow[n] = shadow_of(n, "f32in");
                CHECK_STATUS(cast_step(n, in_shadow[n], ".in_to_f32.", before));
            }
            if (!layer->ReplaceExtraRead(n, in_shadow[n])) return refuse(" (and its fused extra operand cannot be rebound to an fp32 copy)");
        }
        for (TensorNode*& n : outs) {
            if (n->tensor.GetDataType() != DataType::kFloat16) continue;
            TensorNode* sh = shadow_of(n, "f32out");
            CHECK_STATUS(cast_step(sh, n, ".out_to_f16.", after));
            n = sh;
        }
        layer->SetInputNodes(ins);
        layer->SetOutputNodes(outs);
        std::string still;
        if (Status::kSuccess != layer->Validate() || !layer->HalfStorageOk(still)) return refuse(still.empty() ? "" : " / with fp32 operands: " + still);
        LOG(INFO) << "fp16 storage: layer [" << lname << "] has no fp16 kernel (" << why << "): it runs in fp32 between " << before.size()
                  << " + " << after.size() << " casts";
        order.insert(order.begin() + i + 1, after.begin(), after.end());
        order.insert(order.begin() + i, before.begin(), before.end());
        i += before.size() + after.size();
    }
    return Status::kSuccess;
}

// Fusions and storage decisions are re-asked with the real views, or the view is not made.  Every fusion pass and InsertFp32Fallbacks ran on
// dense strides; the alias passes below are what gives an operand its real row.  Before one of them makes `node` a channel slice (pixel
// stride `ld`, `off` channels into the row), every scheduled step is asked whether its launch takes the operand that way (Layer::TakesView:
// a step that does not touch the node says yes) -- the fused groups answer for their real operand lists (the pair's input, the shortcut, the
// upsampled source, the cv3 form's z).  Views that already hang off `node` (the pieces of a split it feeds) move with it and are asked too.
// A "no" leaves the operand its own buffer, and the concat or split launches the copy it has for that case.
bool EngineImpl::ViewTaken(const TensorNode* node, int ld, int off, const char* into) const {
    for (const Step& s : plan_) {
        if (s.layer->TakesView(node, ld, off)) continue;
        LOG(INFO) << "alias: operand [" << (node->operand ? node->operand->name : std::string("-")) << "] keeps its own buffer: [" << s.op->name
                  << "] (" << s.op->type << ") does not take it at pixel stride " << ld << ", channel offset " << off << " (" << into << ")";
        return false;
    }
    for (const auto& kv : aliases_) {
        if (kv.second.parent != node || kv.second.whole) continue;
        auto it = tensor_nodes_.find(kv.first);
        if (it != tensor_nodes_.end() && it->second != node && !ViewTaken(it->second, ld, off + kv.second.channel_offset, into)) return false;
    }
    return true;
}

// torch.cat on the channel axis: every eligible input operand becomes a view into the concat output
// (same pixel grid, pixel stride = total channels), so its producer writes in place and Cat::Forward
// finds nothing left to copy.
Status EngineImpl::AliasConcats() {
    for (const Step& s : plan_) {
        Cat* cat = dynamic_cast<Cat*>(s.layer);
        if (!cat || s.op->type != "torch.cat" || cat->NhwcAxis() != 3 || s.op->outputs.size() != 1) continue;
        TensorNode* out = cat->OutputNodes()[0];  // the staging operand when an output cast follows
        if (out->tensor.Shape().size() != 4) continue;
        int offset = 0;
        std::set<const pnnx::Operand*> seen;
        for (const pnnx::Operand* r : s.op->inputs) {
            const std::vector<int>& rs = tensor_nodes_[r->name]->tensor.Shape();
            const int c = rs.empty() ? 0 : rs.back();
            bool ok = rs.size() == 4 && !seen.count(r) && !aliases_.count(r->name) &&
                      !input_tensor_nodes_.count(r->name) && !output_tensor_nodes_.count(r->name) && r->producer &&
                      r->producer->type != "torch.cat" && HonoursPixelStride(r->producer->type) &&
                      tensor_nodes_[r->name]->tensor.GetDataType() == out->tensor.GetDataType() &&
                      (offset * ElementSize(out->tensor.GetDataType()) % 16 == 0);
            for (const pnnx::Operator* c2 : r->consumers) ok = ok && c2 && HonoursPixelStride(c2->type);
            // flatten writes dense NCHW and Detect writes rank-3 rows: they never feed a rank-4 cat
            if (ok && (r->producer->type == "torch.flatten" || r->producer->type == "models.yolo.Detect")) ok = false;
            // the deformable conv refuses an output whose extent intersects an input's (include/si_deform.h), which a slice of a concat row
            // that also holds one of its inputs would: its output (also behind a fused activation) keeps a buffer of its own.  The sampler
            // of F.grid_sample has the same rule (include/si_grid.h)
            if (ok)
                for (const Step& w : plan_)
                    if (dynamic_cast<DeformConv2d*>(w.layer) || dynamic_cast<GridSample*>(w.layer))
                        for (TensorNode* n : w.layer->OutputNodes()) ok = ok && n != tensor_nodes_[r->name];
            seen.insert(r);
            // ... and its producer and every reader take it at the concat's row (asked last: the refusal it logs is then the only reason)
            ok = ok && ViewTaken(tensor_nodes_[r->name], out->tensor.Shape().back(), offset, s.op->name.c_str());
            if (ok) {
                Alias a;
                a.parent = out;
                a.channel_offset = offset;
                aliases_[r->name] = a;
            }
            offset += c;
        }
    }
    return Status::kSuccess;
}

// torch.chunk / torch.split / Tensor.slice on the channel axis with step 1: every eligible output becomes a view of the input at its channel
// offset (same pixel grid, the input's pixel stride), so the operator launches nothing for it and Slice::Forward skips it.  The input keeps its
// buffer, which PlanArena keeps alive until the last reader of any view.  Only these three types: no existing plan changes.
Status EngineImpl::AliasSplits() {
    for (const Step& s : plan_) {
        Slice* sl = dynamic_cast<Slice*>(s.layer);
        if (!sl || s.op->inputs.size() != 1 || sl->InputNodes().size() != 1) continue;
        const pnnx::Operand* x = s.op->inputs[0];
        TensorNode* in = sl->InputNodes()[0];
        // (an fp32 fallback rebinds the layer to shadow tensors: those are not the file's operands and nothing aliases them)
        if (!x || tensor_nodes_[x->name] != in || input_tensor_nodes_.count(x->name) || output_tensor_nodes_.count(x->name) || in->constant) continue;
        const std::vector<int>& xs = in->tensor.Shape();
        const std::vector<Slice::Piece>& pieces = sl->Pieces();
        if (xs.size() != 4 || pieces.size() != s.op->outputs.size() || sl->OutputNodes().size() != pieces.size()) continue;
        const int in_dims[4] = {xs[0], xs[1], xs[2], xs[3]};
        // the row the views will have: the input's own, or -- a chunk of a chunk -- that of the buffer the input is already a slice of
        const TensorNode* root = in;
        int root_off = 0;
        for (size_t hops = 0; hops <= aliases_.size() && root->operand; ++hops) {
            auto up = aliases_.find(root->operand->name);
            if (up == aliases_.end() || up->second.whole || tensor_nodes_[up->first] != root || !up->second.parent) break;
            root_off += up->second.channel_offset;
            root = up->second.parent;
        }
        const int root_ld = root->tensor.Shape().empty() ? xs[3] : root->tensor.Shape().back();
        for (size_t i = 0; i < pieces.size(); ++i) {
            const pnnx::Operand* r = s.op->outputs[i];
            TensorNode* out = sl->OutputNodes()[i];
            bool ok = r && tensor_nodes_[r->name] == out && !aliases_.count(r->name) && !output_tensor_nodes_.count(r->name) &&
                      !dead_operands_.count(r->name) && Slice::ChannelRange(pieces[i], in_dims) && out->tensor.Shape().size() == 4 &&
                      out->tensor.GetDataType() == in->tensor.GetDataType() &&
                      ((size_t)pieces[i].start[3] * ElementSize(in->tensor.GetDataType()) % 16 == 0);
            if (ok)
                for (const pnnx::Operator* c : r->consumers) ok = ok && c && HonoursPixelStride(c->type);
            // ... and every reader takes it at that row (a concat that later takes the input asks again, for the views that hang off it too)
            ok = ok && ViewTaken(out, root_ld, root_off + pieces[i].start[3], s.op->name.c_str());
            if (!ok) continue;
            Alias a;
            a.parent = in;
            a.channel_offset = pieces[i].start[3];
            aliases_[r->name] = a;
        }
    }
    return Status::kSuccess;
}

// A layout step whose plan is "view" (conv -> permute(0,2,3,1) -> view(N,-1,K): the bytes the conv wrote, in order): the output becomes an
// alias of the WHOLE input buffer under its own shape, dense, and Layout::Forward finds it in place.  Conditions as in AliasSplits: neither side
// is a graph input or output, the types match, the parent is dense (layout operators are not in HonoursPixelStride, so nothing hands them a
// strided operand).  Otherwise the step is one permute_rows copy.
Status EngineImpl::AliasViews() {
    for (const Step& s : plan_) {
        Layout* lay = dynamic_cast<Layout*>(s.layer);
        if (!lay || !lay->IsView() || lay->InputNodes().size() != 1 || lay->OutputNodes().size() != 1 || s.op->outputs.size() != 1) continue;
        TensorNode* in = lay->InputNodes()[0];
        TensorNode* out = lay->OutputNodes()[0];
        const pnnx::Operand* x = in->operand;
        const pnnx::Operand* r = s.op->outputs[0];
        // (fp32 fallbacks and output casts rebind a layer to shadow / staging tensors: those are not the file's operands and nothing aliases them)
        if (!x || !r || tensor_nodes_[x->name] != in || tensor_nodes_[r->name] != out) continue;
        if (input_tensor_nodes_.count(x->name) || output_tensor_nodes_.count(x->name) || output_tensor_nodes_.count(r->name) || in->constant) continue;
        if (aliases_.count(r->name) || dead_operands_.count(r->name) || dead_operands_.count(x->name)) continue;
        if (in->tensor.GetDataType() != out->tensor.GetDataType() || in->tensor.NumElements() != out->tensor.NumElements()) continue;
        // the parent is dense: it is no channel slice of another buffer (a view of a view is fine: that alias is whole and dense itself) and
        // carries no pixel stride.  Today nothing hands a layout step a strided operand; this holds the rule if that ever changes
        auto up = aliases_.find(x->name);
        if (up != aliases_.end() && !up->second.whole) continue;
        if (in->tensor.Shape().empty() || in->tensor.PixelStride() != in->tensor.Shape().back()) continue;
        Alias a;
        a.parent = in;
        a.whole = true;
        aliases_[r->name] = a;
    }
    return Status::kSuccess;
}

// After the alias passes a parent may itself be an alias (a conv output that feeds a chunk and a concat: the chunk's views hang off an operand
// that lives in the concat buffer; a chunk of a chunk).  Every alias is re-pointed at its ROOT buffer with the summed channel offset, so that
// EnsureArena binds views to allocated memory only and PlanArena's lifetimes count every reader against the buffer that is really read.
void EngineImpl::ResolveAliases() {
    for (auto& kv : aliases_) {
        Alias& a = kv.second;
        for (size_t hops = 0; hops <= aliases_.size() && a.parent && a.parent->operand; ++hops) {
            auto up = aliases_.find(a.parent->operand->name);
            if (up == aliases_.end() || tensor_nodes_[up->first] != a.parent || &up->second == &a) break;
            // (a channel slice of a view keeps the view's rows: the root may be the same bytes under another shape)
            if (up->second.whole && !a.whole && a.ld == 0 && !a.parent->tensor.Shape().empty()) a.ld = a.parent->tensor.Shape().back();
            a.channel_offset += up->second.channel_offset;
            a.parent = up->second.parent;
        }
    }
}

// ---- memory plan ---------------------------------------------------------------------------------
// The intermediates (`nodes`: every live operand that is neither an alias nor a graph input / output) are packed into ONE arena: two buffers
// may overlap in memory iff no launch of the plan needs both -- a buffer lives from the first step that writes it (or any alias into it) to
// the last step that reads it.  Plans only: EnsureArena allocates.
void EngineImpl::PlanArena(const std::vector<TensorNode*>& nodes) {
    std::map<TensorNode*, size_t> buf_of;   // root buffer node -> index in bufs
    std::vector<ArenaBuffer> bufs;
    for (TensorNode* n : nodes) {
        buf_of[n] = bufs.size();
        bufs.push_back(ArenaBuffer{n->tensor.ByteSize(), -1, -1});
    }
    auto touch = [&](TensorNode* n, int step) {
        auto al = n && n->operand ? aliases_.find(n->operand->name) : aliases_.end();
        auto it = buf_of.find(al != aliases_.end() ? al->second.parent : n);   // (an alias lives in its root buffer: a concat output, a split input)
        if (it == buf_of.end()) return;
        ArenaBuffer& b = bufs[it->second];
        if (b.first < 0) b.first = step;
        b.last = step;
    };
    for (size_t i = 0; i < plan_.size(); ++i) {
        Layer* L = plan_[i].layer;
        std::vector<TensorNode*> extra;
        L->ExtraReads(extra);
        for (TensorNode* n : L->InputNodes()) touch(n, (int)i);
        for (TensorNode* n : extra) touch(n, (int)i);
        for (TensorNode* n : L->OutputNodes()) touch(n, (int)i);
    }
    const ArenaLayout layout = PackArena(bufs, (int)plan_.size());
    arena_bytes_ = layout.total;
    arena_plan_.clear();
    for (size_t i = 0; i < nodes.size(); ++i) arena_plan_.push_back(ArenaSlot{nodes[i], layout.offsets[i]});
    arena_plan_bytes_ = layout.total;
    arena_pending_ = true;
    LOG(INFO) << "activation arena: " << layout.total << " bytes for " << bufs.size() << " operands (" << unshared_bytes_ << " without sharing)";
}

}  // namespace SimpleInfer
