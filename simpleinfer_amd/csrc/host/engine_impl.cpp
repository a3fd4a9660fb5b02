#include "engine_impl.h"

#include <exception>

#include <algorithm>

#include "batch_rule.h"
#include "layer/conv_2d.h"
#include "layer/yolo_detect.h"
#include "engine_internal.h"
#include "layer_registry.h"
#include "pnnx/expand_expression.h"

namespace SimpleInfer {

EngineImpl::EngineImpl() {}

EngineImpl::~EngineImpl() { Release(); }

Status EngineImpl::SetOption(const std::string& key, int value) {
    if (key == "device") opt_device_ = value;
    else if (key == "fuse") opt_fuse_ = value != 0;
    else if (key == "alias_cat") opt_alias_cat_ = value != 0;
    else if (key == "alias_split") opt_alias_split_ = value != 0;   // chunk / split / slice outputs on the channel axis as views of the input (default 1)
    else if (key == "fuse_layout") opt_fuse_layout_ = value != 0;   // runs of layout operators as one step (default 1)
    else if (key == "fuse_grid") opt_fuse_grid_ = value != 0;       // F.grid_sample reads its grid in place / from theta (default 1; 0: A/B runs)
    else if (key == "alias_view") opt_alias_view_ = value != 0;     // layout steps that move no byte as views of their input (default 1)
    else if (key == "graph") opt_graph_ = value != 0;
    else if (key == "outputs_to_host") opt_outputs_to_host_ = value != 0;
    else if (key == "fp16") opt_fp16_ = value != 0;
    else if (key == "batch") opt_batch_ = value;  // > 0: re-batch the graph at load (the file bakes its batch into every shape)
    else if (key == "arena") opt_arena_ = value != 0;  // 1 (default): intermediates share one arena by lifetime; 0: one hipMalloc each
    else if (key == "fuse_pw") opt_fuse_pw_ = value;           // fp16: 1 (default) a C3 bottleneck's 1x1 conv computed inside the kernel of its 3x3 conv; 2 ... and the C3's closing conv behind its last 64-channel pair (measured slower: opt-in); 0 off
    else if (key == "fuse_stem") opt_fuse_stem_ = value;       // fp16: 1 RGB stem conv + the 3x3 s2 conv behind it in one launch; 2 (default) ... and the 1x1 conv(s) reading that; 0 off
    else if (key == "fuse_upsample") opt_fuse_upsample_ = value != 0;  // upsample -> cat -> 1x1 conv read at the source (default 1)
    else if (key == "detect_priority") opt_detect_priority_ = value < 0 ? -1 : (value > 0 ? 1 : 0);   // priority of Detect's side stream: -1 low, 0 default, +1 high
    else if (key == "detect_stream") opt_detect_stream_ = value;  // Detect's early levels on a second stream: 0 never, 1 (default) where they have enough work, 2 always
    else if (key == "f32_split") opt_f32_split_ = value != 0;   // fp32 tensors, conv contraction from three fp16 MFMA products (default 0: true fp32)
    // kernel-form choices (SiConvPlan, include/si_hip.h; every form of a family produces the same bits): A/B runs and tests.  Until round 6
    // these were process-global setters / environment switches of the kernel library.
    else if (key == "f32_tile") { opt_plan_.f32_tile = value; opt_plan_set_ = true; }
    else if (key == "wino23_form") { opt_plan_.wino23_form = value; opt_plan_set_ = true; }
    else if (key == "wino23_ocg") { opt_plan_.wino23_ocg = value; opt_plan_set_ = true; }
    else if (key == "f16_tile") { opt_plan_.f16_tile = value; opt_plan_set_ = true; }
    else if (key == "f16_detect_tile") { opt_plan_.f16_detect_tile = value; opt_plan_set_ = true; }
    else if (key == "f16_s2c32") { opt_plan_.f16_s2c32 = value; opt_plan_set_ = true; }
    else if (key == "f16_slab") { opt_plan_.f16_slab = value; opt_plan_set_ = true; }
    else if (key == "f16_slab_w2") { opt_plan_.f16_slab_w2 = value; opt_plan_set_ = true; }
    else if (key == "f16_pw_patch") { opt_plan_.f16_pw_patch = value; opt_plan_set_ = true; }
    else if (key == "split3_bm") { opt_plan_.split3_bm = value; opt_plan_set_ = true; }
    else if (key == "f32_split_policy") opt_f32_split_policy_ = value;   // which layers f32_split takes: 1 round 5's, 2 + sibling-fused / wide 1x1 from K = 256, 3 + dual-source (upsampled) layers, 4 (default) + the RGB stem
    else if (key == "winograd") opt_winograd_ = value;  // 0 off, 1 F(2,3) where faster (default), 2 F(4,3) on those layers
    else if (key == "streams") opt_streams_ = value;  // 2: two half-batch lanes on two streams, 1 (default): one stream
    else if (key == "_fail_slicer") debug_fail_slicer_ = value != 0;  // tests: the sliced pipeline's setup fails half way
    else if (key == "pin_inputs") opt_pin_inputs_ = value != 0;  // host_slices: pin a borrowed input buffer in place (default 0, see engine.h)
    else if (key == "host_slices") opt_host_slices_ = value;  // host tensors in and out: G pipelined batch slices per Forward(), 1 off, 0 (default) auto
    else {
        LOG(ERROR) << "unknown engine option [" << key << "]";
        return Status::kUnsupport;
    }
    return Status::kSuccess;
}

Status EngineImpl::LoadModel(const std::string& parampath, const std::string& binpath) {
    struct Stage {
        const char* name;
        Status (EngineImpl::*fn)();
    };
    {
        Status ret = Release();
        if (Status::kSuccess != ret) {
            LOG(ERROR) << "Release fail";
            return ret;
        }
    }
    {
        Status ret = CreateContext();
        if (Status::kSuccess != ret) {
            LOG(ERROR) << "CreateContext fail";
            Release();
            return ret;
        }
    }
    {
        // The reference's loader can throw on malformed files (std::stoi / map::at); nothing may
        // propagate out of this library (there is a C-ABI on top), so a bad model is a Status.
        Status ret = Status::kFail;
        try {
            ret = CreateGraph(parampath, binpath);
        } catch (const std::exception& ex) {
            LOG(ERROR) << "malformed model file: " << ex.what();
            ret = Status::kFail;
        }
        if (Status::kSuccess != ret) {
            LOG(ERROR) << "CreateGraph fail";
            Release();
            return ret;
        }
    }
    param_path_ = parampath;
    bin_path_ = binpath;
    if (!is_lane_) FindBatchMixingLayers();   // (a lane or the slicer's engine is a re-batched copy of a graph that has passed)
    {
        Status ret = CreateTensorNodes();
        if (Status::kSuccess != ret) {
            LOG(ERROR) << "CreateTensorNodes fail";
            Release();
            return ret;
        }
    }
    int lanes = 1;
    {
        Status ret = PlanLanes(lanes);
        if (Status::kSuccess == ret && lanes > 1) {
            ret = LoadLanes(lanes);
            if (Status::kSuccess == ret) ret = AllocateTensorMemory();   // graph inputs / outputs only: the lanes own the rest
        }
        if (Status::kSuccess != ret) {
            LOG(ERROR) << "lane setup fail";
            Release();
            return ret;
        }
        if (lanes > 1) return Status::kSuccess;
    }
    const Stage stages[] = {{"CreateLayers", &EngineImpl::CreateLayers},
                            {"CreatePipeline", &EngineImpl::CreatePipeline},
                            {"AllocateTensorMemory", &EngineImpl::AllocateTensorMemory}};
    for (const Stage& s : stages) {
        Status ret = Status::kFail;
        try {
            ret = (this->*s.fn)();
        } catch (const std::exception& ex) {
            LOG(ERROR) << s.name << ": " << ex.what();
            ret = Status::kFail;
        }
        if (Status::kSuccess != ret) {
            LOG(ERROR) << s.name << " fail";
            Release();
            return ret;
        }
    }
    return Status::kSuccess;
}

Status EngineImpl::Release() {
    if (context_ && context_->stream()) si_hip_stream_sync(context_->stream());
    CHECK_STATUS(DestroyGraphCache());   // (a captured graph references the lanes' streams and buffers)
    CHECK_STATUS(DestroySlicer());
    slicer_failed_ = false;
    UnpinInputs();
    CHECK_STATUS(DestroyLanes());
    CHECK_STATUS(DeallocateTensorMemory());
    CHECK_STATUS(DestroyPipeline());
    CHECK_STATUS(DestroyLayers());
    CHECK_STATUS(DestroyTensorNodes());
    CHECK_STATUS(DestroyGraph());
    CHECK_STATUS(DestroyContext());
    return Status::kSuccess;
}

Status EngineImpl::CreateContext() {
    context_ = new Context;
    CHECK_STATUS(context_->Init(opt_device_));
    SI_TRY_HIP(si_hip_event_create(&ev_start_), "event create");
    SI_TRY_HIP(si_hip_event_create(&ev_stop_), "event create");
    return Status::kSuccess;
}

Status EngineImpl::DestroyContext() {
    if (ev_start_) si_hip_event_destroy(ev_start_);
    if (ev_stop_) si_hip_event_destroy(ev_stop_);
    if (ev_fork_) si_hip_event_destroy(ev_fork_);
    if (ev_join_) si_hip_event_destroy(ev_join_);
    ev_start_ = ev_stop_ = ev_fork_ = ev_join_ = nullptr;
    delete side_context_;
    side_context_ = nullptr;
    delete context_;
    context_ = nullptr;
    return Status::kSuccess;
}

Status EngineImpl::CreateGraph(const std::string& parampath, const std::string& binpath) {
    graph_ = new pnnx::Graph;
    if (0 != graph_->load(parampath, binpath)) {
        LOG(ERROR) << "load graph fail";
        return Status::kFail;
    }
    pnnx::expand_expression(*graph_);
    return Status::kSuccess;
}

Status EngineImpl::DestroyGraph() {
    delete graph_;
    graph_ = nullptr;
    batch_mixing_.clear();
    mixing_logged_ = false;
    return Status::kSuccess;
}

// The operators of the graph that combine images (batch_rule.h), in file order: what keeps "host_slices", "streams" and ShardedEngine from
// cutting the batch.  A layer type registered at run time (RegisterLayer, also one that replaced a built-in) is one of them: the engine knows
// nothing about such a layer beyond the Layer interface.
void EngineImpl::FindBatchMixingLayers() {
    batch_mixing_ = FindBatchMixing(graph_->ops);
    for (const pnnx::Operator* op : graph_->ops) {
        if (!IsUserRegisteredLayer(op->type)) continue;
        bool listed = false;
        for (const BatchMixingEntry& m : batch_mixing_) listed = listed || m.layer == op->name;
        if (!listed) batch_mixing_.push_back({op->name, op->type, "the layer type was registered at run time, so nothing is known about how it treats the batch"});
    }
}

Status EngineImpl::CreateTensorNodes() {
    // Re-batch (SetOption("batch", N)): a pnnx file carries the batch it was traced with in every operand shape
    // (#0=(N,3,640,640)f32).  Serving another batch is a rewrite of dim 0 wherever it equals the traced batch of
    // the graph input.  (An operator that combines images -- a softmax over dimension 0 -- is then that operator over N images,
    // which is what the model means at batch N; it is cutting ONE batch into pieces that such an operator forbids, batch_rule.h.)
    int file_batch = 0;
    if (opt_batch_ > 0) {
        // a box head: the graph inputs [N, ...] and [K, 5] disagree in dimension 0, and where K == N by coincidence the rewrite below would
        // change the number of boxes with the number of images.  Neither is re-batched
        for (const pnnx::Operator* op : graph_->ops)
            if (BatchFamilyOf(op->type) == BatchFamily::kRoi) {
                LOG(ERROR) << "re-batch: [" << op->name << "] (" << op->type << "): " << RoiBatchReason() << ": served at the file's batch only";
                return Status::kUnsupport;
            }
        for (pnnx::Operand* opd : graph_->operands)
            if (opd->producer && opd->producer->inputs.empty() && !opd->shape.empty()) {
                if (file_batch != 0 && file_batch != opd->shape[0]) {
                    LOG(ERROR) << "re-batch: graph inputs disagree on the batch dimension";
                    return Status::kUnsupport;
                }
                file_batch = opd->shape[0];
            }
        if (file_batch <= 0) {
            LOG(ERROR) << "re-batch: no graph input with a static batch dimension";
            return Status::kUnsupport;
        }
    }
    // ... wherever it equals the traced batch -- except where the graph itself has moved the batch to another dimension: seq-first token
    // tensors [L, N, E] (conv -> flatten(2) -> permute(2, 0, 1) in front of nn.MultiheadAttention) carry it in dimension 1.  The batch
    // dimension of every operand is followed from the graph inputs (dimension 0) through the operators; an operand whose batch sits in a
    // dimension >= 1 has THAT dimension rewritten and dimension 0 left alone, every other operand keeps the rule above.
    std::map<const pnnx::Operand*, int> batch_axis;
    if (file_batch > 0) {
        batch_axis = FollowBatchAxes(graph_->ops, file_batch);   // (batch_rule.h: the rule for the split modes follows the same axes)
        for (const pnnx::Operator* op : graph_->ops) {
            if (op->type == "nn.MultiheadAttention") {
                // the layer reads the batch from dimension 0 (batch_first) or 1 of its operands: the rewrite has to have reached that one
                bool batch_first = false;
                Get(op, "batch_first", batch_first);
                for (const pnnx::Operand* in : op->inputs) {
                    auto it = batch_axis.find(in);
                    if (it == batch_axis.end() || it->second != (batch_first ? 0 : 1)) {
                        LOG(ERROR) << "re-batch: [" << op->name << "] nn.MultiheadAttention with batch_first=" << (batch_first ? "True" : "False")
                                   << " reads the batch from dimension " << (batch_first ? 0 : 1) << " of operand [" << in->name
                                   << "], which the graph does not carry there from a batch-major graph input: served at the file's batch only";
                        return Status::kUnsupport;
                    }
                }
            }
        }
    }
    for (pnnx::Operand* opd : graph_->operands) {
        if (tensor_nodes_.count(opd->name) > 0) {
            LOG(ERROR) << "tensor node [" << opd->name << "] already exists";
            return Status::kFail;
        }
        TensorNode* node = new TensorNode;
        node->operand = opd;

        // file shapes are NCHW; tensors are NHWC: the last three dims C,H,W -> H,W,C for rank >= 4
        std::vector<int> file = opd->shape;
        auto moved = batch_axis.find(opd);
        if (moved != batch_axis.end() && moved->second >= 1) file[moved->second] = opt_batch_;
        else if (file_batch > 0 && !file.empty() && file[0] == file_batch) file[0] = opt_batch_;
        std::vector<int> shape = file;
        const int rank = (int)shape.size();
        if (rank > 3) {
            shape[rank - 3] = file[rank - 2];
            shape[rank - 2] = file[rank - 1];
            shape[rank - 1] = file[rank - 3];
        }
        DataType dt = PnnxToDataType(opd->type);
        // graph inputs: produced by an operator with no inputs (pnnx.Input)
        const bool is_input = opd->producer && opd->producer->inputs.empty();
        // graph outputs: consumed by an operator with no outputs (pnnx.Output)
        bool is_output = false;
        for (pnnx::Operator* c : opd->consumers)
            if (c && c->outputs.empty()) is_output = true;
        // fp16 storage: every internal fp32 activation becomes fp16; the tensors the caller hands over / reads back
        // (Input / Extract) keep the file's type
        if (opt_fp16_ && dt == DataType::kFloat32 && !is_input && !is_output) dt = DataType::kFloat16;
        node->tensor = Tensor(dt, shape, MemoryType::kDevice, false);
        tensor_nodes_[opd->name] = node;
        if (is_input) input_tensor_nodes_[opd->name] = node;
        if (is_output) output_tensor_nodes_[opd->name] = node;
    }
    return Status::kSuccess;
}

Status EngineImpl::DestroyTensorNodes() {
    input_tensor_nodes_.clear();
    output_tensor_nodes_.clear();
    user_inputs_.clear();
    user_outputs_.clear();
    for (auto& kv : tensor_nodes_) delete kv.second;
    tensor_nodes_.clear();
    return Status::kSuccess;
}

Status EngineImpl::CreateLayers() {
    for (pnnx::Operator* op : graph_->ops) {
        if ("pnnx.Input" == op->type || "pnnx.Output" == op->type) continue;
        if (layers_.count(op->name) > 0) {
            LOG(ERROR) << "layer [" << op->name << "] already exists";
            return Status::kFail;
        }
        const LayerRegistryEntry* entry = GetLayerRegistry(op->type);
        if (nullptr == entry) {
            LOG(ERROR) << "layer type [" << op->type << "] not registered";
            return Status::kEmpty;
        }
        Layer* layer = entry->creator();
        if (nullptr == layer) {
            LOG(ERROR) << "create layer [" << op->type << "] fail";
            return Status::kFail;
        }
        layers_[op->name] = layer;  // registered first so a failing Init is still destroyed

        Status ret = layer->Init(op);
        if (Status::kSuccess != ret) {
            LOG(ERROR) << "layer [" << op->name << "] init fail";
            return ret;
        }
        layer->SetContext(context_);
        // f32_split: every conv that may run on the split kernels gets its word of the engine's range-guard flags (pinned host memory the
        // kernels can write; 1024 words: more convs than that simply run unguarded-by-flag on the fp32 kernels)
        auto arm_split = [&](Conv2d& cv, bool on) {
            cv.f32_split_ = on;
            cv.f32_split_level_ = opt_f32_split_policy_;
            if (opt_plan_set_) cv.SetPlan(opt_plan_);
            if (!on) return;
            if (!split_flags_) {
                void* p = nullptr;
                if (si_hip_host_alloc(&p, 1024 * sizeof(unsigned)) != 0 || !p) { cv.f32_split_ = false; return; }
                split_flags_ = static_cast<unsigned*>(p);
                for (int i = 0; i < 1024; ++i) split_flags_[i] = 0u;
            }
            if (split_convs_.size() >= 1024) { cv.f32_split_ = false; return; }
            cv.range_flag_ = split_flags_ + split_convs_.size();
            split_convs_.push_back(&cv);
        };
        if (YoloDetect* yd = dynamic_cast<YoloDetect*>(layer)) {
            yd->fuse_decode_ = opt_fuse_;
            for (Conv2d& cv : yd->conv_2d_layer_) arm_split(cv, opt_f32_split_ && !opt_fp16_ && opt_fuse_);
        }
        if (Conv2d* cv = dynamic_cast<Conv2d*>(layer)) {
            if (!opt_winograd_) cv->algo_ = Conv2d::Algo::kImplicitGemm;
            cv->prefer_wino43_ = opt_winograd_ == 2;
            arm_split(*cv, opt_f32_split_ && !opt_fp16_);
        }

        std::vector<TensorNode*> ins, outs;
        for (pnnx::Operand* r : op->inputs) {
            auto it = tensor_nodes_.find(r->name);
            if (it == tensor_nodes_.end()) {
                LOG(ERROR) << "tensor node [" << r->name << "] not exist";
                return Status::kEmpty;
            }
            ins.push_back(it->second);
        }
        for (pnnx::Operand* r : op->outputs) {
            auto it = tensor_nodes_.find(r->name);
            if (it == tensor_nodes_.end()) {
                LOG(ERROR) << "tensor node [" << r->name << "] not exist";
                return Status::kEmpty;
            }
            outs.push_back(it->second);
        }
        layer->SetInputNodes(ins);
        layer->SetOutputNodes(outs);

        ret = layer->Validate();
        if (Status::kSuccess != ret) {
            LOG(ERROR) << "layer [" << op->name << "] validate fail";
            return ret;
        }
    }
    return Status::kSuccess;
}

Status EngineImpl::DestroyLayers() {
    for (auto& kv : layers_) {
        Layer* layer = kv.second;
        const pnnx::Operator* op = layer->GetOp();
        Status ret = layer->Deinit();
        if (Status::kSuccess != ret) LOG(ERROR) << "layer [" << kv.first << "] deinit fail";
        const LayerRegistryEntry* entry = op ? GetLayerRegistry(op->type) : nullptr;
        if (entry) {
            entry->destroyer(layer);
        } else {
            delete layer;
        }
    }
    layers_.clear();
    split_convs_.clear();
    if (split_flags_) si_hip_host_free(split_flags_);
    split_flags_ = nullptr;
    return Status::kSuccess;
}

// A cached graph exec may still be in flight (ForwardAsync without Sync): wait for the stream before destroying any.
Status EngineImpl::DestroyGraphCache() {
    if (!graph_cache_.empty() && context_ && context_->stream()) si_hip_stream_sync(context_->stream());
    for (auto& g : graph_cache_) si_hip_graph_destroy(g.second);
    graph_cache_.clear();
    return Status::kSuccess;
}

Status EngineImpl::DestroyPipeline() {
    CHECK_STATUS(DestroyGraphCache());
    forward_count_ = 0;
    last_slices_ = 1;
    plan_warm_ = false;
    plan_.clear();
    fused_ops_.clear();
    sibling_ops_.clear();
    dead_operands_.clear();
    aliases_.clear();
    return Status::kSuccess;
}

// ---- memory --------------------------------------------------------------------------------------
Status EngineImpl::AllocateTensorMemory() {
    // 1. Every live operand that is not an alias gets HBM.  The reference mallocs each operand separately and never reuses
    //    (src/engine_impl.cpp:465-482, "TODO" at :466).  Here graph inputs / outputs keep their own buffers (they outlive the
    //    forward), and the intermediates share ONE arena by lifetime (PlanArena, engine_plan.cpp).
    std::vector<TensorNode*> arena_nodes;
    unshared_bytes_ = arena_bytes_ = 0;
    for (auto& kv : tensor_nodes_) {
        const std::string& name = kv.first;
        Tensor& t = kv.second->tensor;
        if (dead_operands_.count(name) || aliases_.count(name)) continue;
        if (!lanes_.empty() && !input_tensor_nodes_.count(name) && !output_tensor_nodes_.count(name)) continue;   // the lanes own the intermediates
        const size_t bytes = t.ByteSize();
        if (bytes == 0) {
            LOG(ERROR) << "operand [" << name << "] has no static shape";
            return Status::kErrorShape;
        }
        const bool io = input_tensor_nodes_.count(name) || output_tensor_nodes_.count(name);
        if (io || !opt_arena_) {
            void* p = nullptr;
            SI_TRY_HIP(si_hip_malloc(&p, bytes), "hipMalloc operand");
            device_allocs_.push_back(p);
            if (input_tensor_nodes_.count(name)) input_buffers_[name] = p;  // staging for host inputs
            if (output_tensor_nodes_.count(name)) own_output_ptrs_[name] = p;
            t.SetView(p, MemoryType::kDevice, 0);
            if (!io) unshared_bytes_ += bytes, arena_bytes_ += bytes;
            continue;
        }
        arena_nodes.push_back(kv.second);
        unshared_bytes_ += bytes;
    }
    if (!arena_nodes.empty()) PlanArena(arena_nodes);
    // An engine whose forwards may all be served by the sliced host pipeline (host outputs, slicing not switched off, not a lane)
    // leaves the arena to the first forward that runs its OWN plan: the slicer has an arena of its own, and this one would be a
    // second, never-touched allocation.  Everyone else allocates now, so LoadModel reports an arena that does not fit.
    const bool defer = arena_pending_ && !is_lane_ && opt_outputs_to_host_ && opt_host_slices_ != 1 && lanes_.empty();
    if (!defer) CHECK_STATUS(EnsureArena());
    // 3. pinned host mirrors for outputs
    if (opt_outputs_to_host_) {
        for (auto& kv : output_tensor_nodes_) {
            void* h = nullptr;
            SI_TRY_HIP(si_hip_host_alloc(&h, kv.second->tensor.ByteSize()), "hipHostMalloc output");
            host_outputs_[kv.first] = h;
        }
    }
    return Status::kSuccess;
}

// allocate the planned arena (once) and point the operands -- and the aliases (concat inputs, split outputs), which hang off them -- into it
Status EngineImpl::EnsureArena() {
    if (arena_pending_) {
        void* arena = nullptr;
        SI_TRY_HIP(si_hip_malloc(&arena, arena_plan_bytes_), "hipMalloc activation arena");
        device_allocs_.push_back(arena);
        for (const ArenaSlot& b : arena_plan_) b.node->tensor.SetView(static_cast<char*>(arena) + b.offset, MemoryType::kDevice, 0);
        arena_pending_ = false;
    }
    if (!aliases_bound_) {
        for (auto& kv : aliases_) {
            Tensor& t = tensor_nodes_[kv.first]->tensor;
            Tensor& parent = kv.second.parent->tensor;
            if (parent.RawData() == nullptr) continue;
            // (the parent is a root buffer -- ResolveAliases -- and a channel slice takes ITS pixel stride; a view of the whole buffer is dense
            // under its own shape, and a slice of such a view has the view's rows)
            t.SetView(static_cast<char*>(parent.RawData()) + (size_t)kv.second.channel_offset * ElementSize(parent.GetDataType()),
                      MemoryType::kDevice, kv.second.whole ? 0 : (kv.second.ld > 0 ? kv.second.ld : parent.PixelStride()));
        }
        aliases_bound_ = true;
    }
    return Status::kSuccess;
}

Status EngineImpl::DeallocateTensorMemory() {
    arena_plan_.clear();
    arena_plan_bytes_ = 0;
    arena_pending_ = false;
    aliases_bound_ = false;
    for (void* p : device_allocs_) si_hip_free(p);
    device_allocs_.clear();
    input_buffers_.clear();
    own_output_ptrs_.clear();
    for (auto& kv : host_outputs_) si_hip_host_free(kv.second);
    host_outputs_.clear();
    for (auto& kv : tensor_nodes_) kv.second->tensor.SetView(nullptr, MemoryType::kDevice, 0);
    return Status::kSuccess;
}


// ---- lanes (option "streams") ---------------------------------------------------------------------
// Two half-batch engines on two streams instead of one full-batch engine on one: while one lane is in a layer's tail (the last,
// partial round of workgroups, the epilogue stores) the other lane's workgroups fill the idle CUs.  Measured on MI355X,
// YOLOv5s batch 32, same box, hipGraph replay: +4.9 % (tools/two_stream_exp.py).  A lane is this model
// re-batched to N / 2 (the "batch" option's rule) that reads and writes slab views of this engine's input and output buffers.
// That is the same computation only for a graph whose every operator is per-image (batch_rule.h; the reference's operators all
// are, SURVEY.md 8e, a softmax or a mean over the batch, a slice along it or a view that folds it is not): then the results are
// bit-identical to the one-stream schedule because no kernel's per-element arithmetic depends on the batch
// (tests/test_gpu_tiles.py, tests/test_gpu_engine.py, tests/test_gpu_batch_split.py).  Any other graph is refused.
// Can the batch be cut into contiguous slabs?  Every graph input and output must be batch-major (dimension 0 = the batch, rank >= 2) ...
bool EngineImpl::BatchMajorIO(int& batch) const {
    batch = 0;
    bool ok = !input_tensor_nodes_.empty() && !output_tensor_nodes_.empty();
    for (auto& kv : input_tensor_nodes_) {
        const std::vector<int>& sh = kv.second->tensor.Shape();
        if (sh.size() < 2 || (batch != 0 && sh[0] != batch)) ok = false;
        else batch = sh[0];
    }
    for (auto& kv : output_tensor_nodes_) {
        const std::vector<int>& sh = kv.second->tensor.Shape();
        if (sh.size() < 2 || sh[0] != batch) ok = false;
    }
    return ok && batch >= 2;
}

// ... and every operator of the graph must be per-image by the rule of batch_rule.h
bool EngineImpl::BatchSplittable(int& batch) const { return BatchMajorIO(batch) && batch_mixing_.empty(); }

std::string EngineImpl::BatchMixingText() const {
    std::string s;
    for (const BatchMixingEntry& m : batch_mixing_) s += (s.empty() ? "[" : "; [") + m.layer + "] (" + m.type + "): " + m.reason;
    return s;
}

Status EngineImpl::PlanLanes(int& lanes) {
    lanes = 1;
    if (is_lane_ || opt_streams_ < 2) return Status::kSuccess;
    int batch = 0;
    const bool ok = BatchSplittable(batch) && batch % 2 == 0;
    if (opt_streams_ >= 2) {
        if (!batch_mixing_.empty()) {
            LOG(ERROR) << "streams=2 runs two half-batch copies of the model, which needs per-image operators; not per-image: " << BatchMixingText();
            return Status::kUnsupport;
        }
        if (!ok) {
            LOG(ERROR) << "streams=2 needs an even batch that is dimension 0 of every graph input and output";
            return Status::kUnsupport;
        }
        lanes = 2;
    }
    return Status::kSuccess;
}

Status EngineImpl::LoadLanes(int lanes) {
    int batch = input_tensor_nodes_.begin()->second->tensor.Shape()[0];
    for (int l = 0; l < lanes; ++l) {
        EngineImpl* lane = new EngineImpl;
        lanes_.push_back(lane);
        lane->is_lane_ = true;
        lane->opt_device_ = context_->device();
        lane->opt_fuse_ = opt_fuse_;
        lane->opt_alias_cat_ = opt_alias_cat_;
        lane->opt_alias_split_ = opt_alias_split_;
        lane->opt_fuse_layout_ = opt_fuse_layout_;
        lane->opt_fuse_grid_ = opt_fuse_grid_;
        lane->opt_alias_view_ = opt_alias_view_;
        lane->opt_fuse_upsample_ = opt_fuse_upsample_;
        lane->opt_fuse_stem_ = opt_fuse_stem_;
        lane->opt_fuse_pw_ = opt_fuse_pw_;
        lane->opt_arena_ = opt_arena_;
        lane->opt_winograd_ = opt_winograd_;
        lane->opt_f32_split_ = opt_f32_split_;
        lane->opt_f32_split_policy_ = opt_f32_split_policy_;
        lane->opt_plan_ = opt_plan_;
        lane->opt_plan_set_ = opt_plan_set_;
        lane->opt_detect_stream_ = opt_detect_stream_;
        lane->opt_detect_priority_ = opt_detect_priority_;
        lane->opt_fp16_ = opt_fp16_;
        lane->opt_graph_ = opt_graph_;        // every lane replays its OWN captured graph on its own stream; this engine only forks / joins
                                              // (one graph holding both branches measured 10 % SLOWER than one stream: profiles/r03_ab_streams.txt)
        lane->opt_outputs_to_host_ = false;   // ... and owns the host mirrors
        lane->opt_streams_ = 1;
        lane->opt_batch_ = batch / lanes;
        CHECK_STATUS(lane->LoadModel(param_path_, bin_path_));
        si_event_t ev = nullptr;
        SI_TRY_HIP(si_hip_event_create(&ev), "event create");
        lane_done_.push_back(ev);
    }
    if (!ev_fork_) SI_TRY_HIP(si_hip_event_create(&ev_fork_), "event create");
    LOG(INFO) << "streams: " << lanes << " lanes of batch " << batch / lanes;
    return Status::kSuccess;
}

Status EngineImpl::DestroyLanes() {
    for (EngineImpl* lane : lanes_) delete lane;
    lanes_.clear();
    for (si_event_t ev : lane_done_) si_hip_event_destroy(ev);
    lane_done_.clear();
    return Status::kSuccess;
}

namespace {
// lane `l` of `n`: the contiguous slab of images [l * N / n, (l + 1) * N / n) of a batch-major tensor, as a non-owning view
Tensor SlabView(const Tensor& t, int l, int n) {
    std::vector<int> shape = t.Shape();
    const size_t rows = t.NumElements() / (size_t)shape.back();   // pixels (rank 4) / rows of the last dimension
    const size_t slab_bytes = rows / (size_t)n * (size_t)t.PixelStride() * ElementSize(t.GetDataType());
    shape[0] /= n;
    Tensor v(t.GetDataType(), shape, MemoryType::kDevice, false);
    v.SetView(static_cast<char*>(t.RawData()) + (size_t)l * slab_bytes, MemoryType::kDevice, t.PixelStride() == t.Shape().back() ? 0 : t.PixelStride());
    return v;
}
}  // namespace

// hand every lane its slab of the (already resolved) input and output tensors of this engine
Status EngineImpl::BindLanes() {
    const int n = (int)lanes_.size();
    for (int l = 0; l < n; ++l) {
        for (auto& kv : input_tensor_nodes_) CHECK_STATUS(lanes_[l]->Input(kv.first, SlabView(kv.second->tensor, l, n)));
        for (auto& kv : output_tensor_nodes_) CHECK_STATUS(lanes_[l]->Output(kv.first, SlabView(kv.second->tensor, l, n)));
    }
    return Status::kSuccess;
}

// fork: every lane's stream waits for this engine's stream (the input upload); join: this stream waits for every lane.  With
// option "graph" every lane replays its own captured graph between the two.
Status EngineImpl::LaunchLanes() {
    si_stream_t stream = context_->stream();
    SI_TRY_HIP(si_hip_event_record(ev_fork_, stream), "event record");
    for (size_t l = 0; l < lanes_.size(); ++l) {
        SI_TRY_HIP(si_hip_stream_wait_event(lanes_[l]->context_->stream(), ev_fork_), "stream wait");
        CHECK_STATUS(lanes_[l]->ForwardAsync());
        lanes_[l]->forward_pending_ = false;   // (the lane's own start / stop events may sit inside a capture: never read)
        SI_TRY_HIP(si_hip_event_record(lane_done_[l], lanes_[l]->context_->stream()), "event record");
    }
    for (size_t l = 0; l < lanes_.size(); ++l) SI_TRY_HIP(si_hip_stream_wait_event(stream, lane_done_[l]), "stream wait");
    return Status::kSuccess;
}

// ---- the reference's host-tensor contract at speed (option "host_slices") -------------------------------------------------
// Engine::Input borrows a HOST tensor that is read at Forward() time and Extract hands back host-visible memory (reference
// src/engine_impl.cpp:522-555, bench/bench_yolo.cpp:20-28).  Done naively that is upload -> compute -> download in series:
// YOLOv5s batch 32 moves 157 MB up and 274 MB down around 4.3 ms of kernels, 12.8 ms per Forward.  Here one synchronous
// Forward() is a three-stage pipeline over G contiguous batch slices: slice g's images go up on an upload stream while slice
// g-1 computes (ONE child engine of batch N / G runs the slices back to back on its own stream: same weights, same arena) and
// slice g-2's output rows come down on a download stream into the pinned mirror Extract() returns.  What is left outside the
// overlap is the first slice's upload and the last slice's download.  A borrowed input buffer that is handed over for a second
// Forward is pinned in place (hipHostRegister) so its uploads run asynchronously at the link rate.  Bit-identical to the
// unsliced schedule for a graph of per-image operators (tests/test_gpu_engine.py::test_host_tensor_pipeline_*,
// tests/test_gpu_batch_split.py).  A graph that holds an operator which combines images (batch_rule.h; a layer type registered at
// run time counts as one) is served unsliced: slices of it would compute something else.  Under auto that is said once at INFO,
// under an explicit host_slices > 1 once as an ERROR, each with the layer and the reason.
int EngineImpl::PlanSlices() const {
    if (is_lane_ || opt_host_slices_ == 1 || !opt_outputs_to_host_ || slicer_failed_) return 1;
    if (!lanes_.empty()) return 1;   // "streams" = 2 was asked for: the lanes serve the engine
    int batch = 0;
    if (!BatchMajorIO(batch)) return 1;
    for (auto& kv : input_tensor_nodes_) {
        auto u = user_inputs_.find(kv.first);
        if (u == user_inputs_.end() || u->second.RawData() == nullptr || u->second.GetMemoryType() == MemoryType::kDevice) return 1;
    }
    if (!user_outputs_.empty()) return 1;   // caller-owned device outputs: not the host contract
    const int slices = SlicesFor(batch);
    if (slices > 1 && !batch_mixing_.empty()) {
        if (!mixing_logged_) {
            if (opt_host_slices_ > 1)
                LOG(ERROR) << "host_slices=" << opt_host_slices_ << " needs per-image operators; serving this engine unsliced.  Not per-image: " << BatchMixingText();
            else
                LOG(INFO) << "host_slices: serving this engine unsliced.  Not per-image: " << BatchMixingText();
            mixing_logged_ = true;
        }
        return 1;
    }
    return slices;
}

// the number of slices a batch-major graph of per-image operators is served with
int EngineImpl::SlicesFor(int batch) const {
    if (opt_host_slices_ > 1) return batch % opt_host_slices_ == 0 ? opt_host_slices_ : 1;
    // auto (MI355X, YOLOv5s 640x640, profiles/r03_host_slices.txt): slices of 8 images from batch 32 on (a batch-8 forward is still
    // at 0.6 of the MFMA ceiling, and 8 images are 39 MB up / 69 MB down -- 0.7 / 1.3 ms of PCIe outside the overlap), slices of 4
    // for batches 8 .. 31 (batch 8: 3.49 -> 2.95 ms per Forward with 2 slices; batch 16: 6.61 -> 4.95 with 4); at most 8 slices
    // (one captured graph per slice under "graph")
    const int per = batch >= 32 ? 8 : 4;
    if (batch < 8 || batch % per != 0) return 1;
    int g = batch / per;
    while (g > 8 && g % 2 == 0) g /= 2;
    return g <= 8 ? g : 1;
}

Status EngineImpl::DestroySlicer() {
    delete slicer_;
    slicer_ = nullptr;
    slices_ = 0;
    for (si_event_t e : ev_up_) si_hip_event_destroy(e);
    for (si_event_t e : ev_done_) si_hip_event_destroy(e);
    ev_up_.clear();
    ev_done_.clear();
    if (ev_down_all_) si_hip_event_destroy(ev_down_all_);
    ev_down_all_ = nullptr;
    delete up_context_;
    delete down_context_;
    up_context_ = down_context_ = nullptr;
    return Status::kSuccess;
}

void EngineImpl::UnpinInputs() {
    for (auto& kv : pinned_inputs_)
        if (kv.second.registered) si_hip_host_unregister(const_cast<void*>(kv.second.ptr));
    pinned_inputs_.clear();
}

// everything the sliced pipeline needs; slices_ is set LAST, so a failure half way leaves nothing that looks usable
Status EngineImpl::SetupSlicer(int slices) {
    CHECK_STATUS(DestroySlicer());
    int batch = 0;
    CHECK_BOOL(BatchSplittable(batch) && batch % slices == 0);
    slicer_ = new EngineImpl;
    slicer_->is_lane_ = true;
    slicer_->opt_device_ = context_->device();
    slicer_->opt_fuse_ = opt_fuse_;
    slicer_->opt_alias_cat_ = opt_alias_cat_;
    slicer_->opt_alias_split_ = opt_alias_split_;
    slicer_->opt_fuse_layout_ = opt_fuse_layout_;
    slicer_->opt_fuse_grid_ = opt_fuse_grid_;
    slicer_->opt_alias_view_ = opt_alias_view_;
    slicer_->opt_fuse_upsample_ = opt_fuse_upsample_;
    slicer_->opt_fuse_stem_ = opt_fuse_stem_;
    slicer_->opt_fuse_pw_ = opt_fuse_pw_;
    slicer_->opt_arena_ = opt_arena_;
    slicer_->opt_winograd_ = opt_winograd_;
    slicer_->opt_f32_split_ = opt_f32_split_;
    slicer_->opt_f32_split_policy_ = opt_f32_split_policy_;
    slicer_->opt_plan_ = opt_plan_;
    slicer_->opt_plan_set_ = opt_plan_set_;
    slicer_->opt_detect_stream_ = opt_detect_stream_;
    slicer_->opt_detect_priority_ = opt_detect_priority_;
    slicer_->opt_fp16_ = opt_fp16_;
    slicer_->opt_graph_ = opt_graph_;          // one captured graph per slice (its I/O pointers key the cache) ...
    slicer_->max_graphs_ = std::max<size_t>(max_graphs_, (size_t)slices);   // ... so the cache holds at least one per slice
    slicer_->opt_outputs_to_host_ = false;
    slicer_->opt_streams_ = 1;
    slicer_->opt_batch_ = batch / slices;
    CHECK_STATUS(slicer_->LoadModel(param_path_, bin_path_));
    up_context_ = new Context;
    CHECK_STATUS(up_context_->Init(context_->device()));
    if (debug_fail_slicer_) return Status::kFail;
    down_context_ = new Context;
    CHECK_STATUS(down_context_->Init(context_->device()));
    ev_up_.assign((size_t)slices, nullptr);
    ev_done_.assign((size_t)slices, nullptr);
    for (auto& e : ev_up_) SI_TRY_HIP(si_hip_event_create(&e), "event create");
    for (auto& e : ev_done_) SI_TRY_HIP(si_hip_event_create(&e), "event create");
    SI_TRY_HIP(si_hip_event_create(&ev_down_all_), "event create");
    if (!ev_fork_) SI_TRY_HIP(si_hip_event_create(&ev_fork_), "event create");
    slices_ = slices;
    LOG(INFO) << "host_slices: " << slices << " pipelined slices of batch " << batch / slices;
    return Status::kSuccess;
}

Status EngineImpl::ForwardSliced(int slices) {
    si_stream_t stream = context_->stream();
    CHECK_BOOL(slicer_ != nullptr && slices_ == slices);
    last_slices_ = slices;
    // the engine's device-side input staging and its own output buffers, whole batch; the slices are views
    for (auto& kv : input_tensor_nodes_) kv.second->tensor.SetView(input_buffers_[kv.first], MemoryType::kDevice, 0);
    CHECK_STATUS(BindOutputs());
    // a borrowed input seen for the second Forward in a row is pinned in place; a different pointer drops the old pin
    for (auto& kv : input_tensor_nodes_) {
        const Tensor& host = user_inputs_[kv.first];
        Pinned& p = pinned_inputs_[kv.first];
        if (p.ptr != host.RawData() || p.bytes != host.ByteSize()) {
            if (p.registered) si_hip_host_unregister(const_cast<void*>(p.ptr));
            p = Pinned();
            p.ptr = host.RawData();
            p.bytes = host.ByteSize();
        }
        // (opt-in, "pin_inputs": a registration outlives this call, so the caller has to keep the buffer mapped until the next
        // Input() / Release -- freeing it after Forward(), which the reference's borrow allows, would leave a stale registration)
        if (opt_pin_inputs_ && ++p.seen == 2 && !p.registered) {
            p.registered = si_hip_host_register(const_cast<void*>(p.ptr), p.bytes) == 0;   // (failure: the uploads stay staged copies)
            if (!p.registered) LOG(INFO) << "host_slices: could not pin the input buffer of [" << kv.first << "]; uploads stay staged";
        }
    }
    SI_TRY_HIP(si_hip_event_record(ev_start_, stream), "event record");
    // the upload stream starts behind whatever this engine's stream still holds (a previous ForwardAsync)
    SI_TRY_HIP(si_hip_event_record(ev_fork_, stream), "event record");
    SI_TRY_HIP(si_hip_stream_wait_event(up_context_->stream(), ev_fork_), "stream wait");
    SI_TRY_HIP(si_hip_stream_wait_event(slicer_->context_->stream(), ev_fork_), "stream wait");
    SI_TRY_HIP(si_hip_stream_wait_event(down_context_->stream(), ev_fork_), "stream wait");
    for (int g = 0; g < slices; ++g) {
        for (auto& kv : input_tensor_nodes_) {
            const Tensor dst = SlabView(kv.second->tensor, g, slices);
            const size_t bytes = dst.ByteSize();
            const char* src = static_cast<const char*>(user_inputs_[kv.first].RawData()) + (size_t)g * bytes;
            SI_TRY_HIP(si_hip_memcpy_h2d(dst.RawData(), src, bytes, up_context_->stream()), "input slice h2d");
            CHECK_STATUS(slicer_->Input(kv.first, dst));
        }
        SI_TRY_HIP(si_hip_event_record(ev_up_[(size_t)g], up_context_->stream()), "event record");
        SI_TRY_HIP(si_hip_stream_wait_event(slicer_->context_->stream(), ev_up_[(size_t)g]), "stream wait");
        for (auto& kv : output_tensor_nodes_) CHECK_STATUS(slicer_->Output(kv.first, SlabView(kv.second->tensor, g, slices)));
        CHECK_STATUS(slicer_->ForwardAsync());
        slicer_->forward_pending_ = false;
        SI_TRY_HIP(si_hip_event_record(ev_done_[(size_t)g], slicer_->context_->stream()), "event record");
        SI_TRY_HIP(si_hip_stream_wait_event(down_context_->stream(), ev_done_[(size_t)g]), "stream wait");
        for (auto& kv : output_tensor_nodes_) {
            const Tensor src = SlabView(kv.second->tensor, g, slices);
            const size_t bytes = src.ByteSize();
            SI_TRY_HIP(si_hip_memcpy_d2h(static_cast<char*>(host_outputs_[kv.first]) + (size_t)g * bytes, src.RawData(), bytes,
                                         down_context_->stream()), "output slice d2h");
        }
    }
    SI_TRY_HIP(si_hip_event_record(ev_down_all_, down_context_->stream()), "event record");
    SI_TRY_HIP(si_hip_stream_wait_event(stream, ev_down_all_), "stream wait");   // Sync() on this engine's stream covers the pipeline
    SI_TRY_HIP(si_hip_event_record(ev_stop_, stream), "event record");
    forward_pending_ = true;
    ++forward_count_;
    return Status::kSuccess;
}

// ---- I/O -----------------------------------------------------------------------------------------
const std::vector<std::string> EngineImpl::InputNames() {
    std::vector<std::string> ret;
    for (auto& kv : input_tensor_nodes_) ret.push_back(kv.first);
    return ret;
}

const std::vector<std::string> EngineImpl::OutputNames() {
    std::vector<std::string> ret;
    for (auto& kv : output_tensor_nodes_) ret.push_back(kv.first);
    return ret;
}

Status EngineImpl::OperandShape(const std::string& name, std::vector<int>& shape) {
    auto it = tensor_nodes_.find(name);
    if (it == tensor_nodes_.end()) return Status::kFail;
    shape = it->second->tensor.Shape();
    return Status::kSuccess;
}

Status EngineImpl::Input(const std::string& name, const Tensor& input) {
    auto it = input_tensor_nodes_.find(name);
    if (it == input_tensor_nodes_.end()) {
        LOG(ERROR) << "tensor [" << name << "] is not an input tensor";
        return Status::kFail;
    }
    if (input.NumElements() != it->second->tensor.NumElements() || input.GetDataType() != it->second->tensor.GetDataType()) {
        LOG(ERROR) << "tensor [" << name << "] does not match the model's input shape / type";
        return Status::kErrorShape;
    }
    // a previously borrowed buffer that was pinned in place (host_slices) is released to its owner NOW: the caller may free it
    // as soon as this returns (reference contract: borrowed until the next Input() / Release, engine_impl.cpp:466-471,528)
    auto pin = pinned_inputs_.find(name);
    if (pin != pinned_inputs_.end() && pin->second.ptr != input.RawData()) {
        if (pin->second.registered) {
            if (up_context_) si_hip_stream_sync(up_context_->stream());
            si_hip_host_unregister(const_cast<void*>(pin->second.ptr));
        }
        pinned_inputs_.erase(pin);
    }
    user_inputs_[name] = input;  // alias: the caller keeps ownership (reference engine_impl.cpp:528)
    return Status::kSuccess;
}

// Output(): the mirror of a device-resident Input() -- the caller provides the HBM buffer an output operand is written
// to (e.g. one of two tensors that are handed to an asynchronous collective while the next Forward runs).  Borrowed
// until the next Output() / Release; a null tensor restores the engine's own buffer.
Status EngineImpl::Output(const std::string& name, const Tensor& output) {
    auto it = output_tensor_nodes_.find(name);
    if (it == output_tensor_nodes_.end()) {
        LOG(ERROR) << "tensor [" << name << "] is not an output tensor";
        return Status::kFail;
    }
    if (nullptr == output.RawData()) {
        user_outputs_.erase(name);
        return Status::kSuccess;
    }
    if (output.GetMemoryType() != MemoryType::kDevice) {
        LOG(ERROR) << "Output(" << name << "): a caller-owned output buffer must be device memory";
        return Status::kUnsupport;
    }
    if (output.NumElements() != it->second->tensor.NumElements() || output.GetDataType() != it->second->tensor.GetDataType()) {
        LOG(ERROR) << "tensor [" << name << "] does not match the model's output shape / type";
        return Status::kErrorShape;
    }
    user_outputs_[name] = output;
    return Status::kSuccess;
}

Status EngineImpl::BindOutputs() {
    for (auto& kv : output_tensor_nodes_) {
        auto u = user_outputs_.find(kv.first);
        void* want = u != user_outputs_.end() ? u->second.RawData() : own_output_ptrs_[kv.first];
        if (want && kv.second->tensor.RawData() != want) kv.second->tensor.SetView(want, MemoryType::kDevice, 0);
    }
    return Status::kSuccess;
}

Status EngineImpl::UploadInputs() {
    for (auto& kv : input_tensor_nodes_) {
        auto u = user_inputs_.find(kv.first);
        if (u == user_inputs_.end() || nullptr == u->second.RawData()) {
            LOG(ERROR) << "input [" << kv.first << "] was not provided";
            return Status::kEmpty;
        }
        Tensor& node_tensor = kv.second->tensor;
        if (u->second.GetMemoryType() == MemoryType::kDevice) {
            // device-resident input: read it in place
            node_tensor.SetView(u->second.RawData(), MemoryType::kDevice, u->second.PixelStride());
        } else {
            void* buf = input_buffers_[kv.first];
            node_tensor.SetView(buf, MemoryType::kDevice, 0);
            SI_TRY_HIP(si_hip_memcpy_h2d(buf, u->second.RawData(), node_tensor.ByteSize(), context_->stream()), "input h2d");
        }
    }
    return Status::kSuccess;
}

Status EngineImpl::LaunchAll() {
    if (!lanes_.empty()) return LaunchLanes();
    YoloDetect* early_detect = nullptr;   // the Detect layer with levels in flight on the side stream
    for (size_t i = 0; i < plan_.size(); ++i) {
        const Step& s = plan_[i];
        Status ret = s.layer->Forward();
        if (Status::kSuccess != ret) {
            LOG(ERROR) << "layer [" << s.op->name << "] forward fail";
            return ret;
        }
        if (side_context_ && early_detect && s.layer == early_detect) {
            // join: everything after Detect (and the end of the forward) waits for the side stream's levels
            SI_TRY_HIP(si_hip_event_record(ev_join_, side_context_->stream()), "event record");
            SI_TRY_HIP(si_hip_stream_wait_event(context_->stream(), ev_join_), "stream wait");
            early_detect = nullptr;
        }
        if (side_context_ && !s.detect_levels.empty()) {
            // fork: the side stream may start once this step is done
            SI_TRY_HIP(si_hip_event_record(ev_fork_, context_->stream()), "event record");
            SI_TRY_HIP(si_hip_stream_wait_event(side_context_->stream(), ev_fork_), "stream wait");
            for (size_t j = i + 1; j < plan_.size() && !early_detect; ++j) {
                YoloDetect* d = dynamic_cast<YoloDetect*>(plan_[j].layer);
                if (d && d->EarlyLevels()) early_detect = d;
            }
            if (!early_detect) return Status::kFail;
            for (int level : s.detect_levels) CHECK_STATUS(early_detect->ForwardLevel(level));
        }
    }
    return Status::kSuccess;
}

Status EngineImpl::Forward() {
    CHECK_STATUS(ForwardAsync());
    return Sync();
}

// Forward() is synchronous by contract (reference engine_impl.cpp:533-544)
Status EngineImpl::Sync() {
    if (nullptr == context_) return Status::kFail;
    SI_TRY_HIP(si_hip_stream_sync(context_->stream()), "stream sync");
    // f32_split range guard: a split kernel that saw an operand leave fp16's range has set its layer's flag (the step's results are then
    // Inf / NaN in that layer's outputs).  The layer goes back to the true-fp32 kernels for this engine's lifetime and the step is re-run, here,
    // on the same inputs -- the caller of Forward() never sees the overflowed step.  (A caller that queued several ForwardAsync() steps gets
    // the LAST one re-run: the guard acts where the engine synchronises.)  At most one round per layer, bounded.
    if (forward_pending_ && !is_lane_) {
        for (int round = 0; round < 8 && TakeSplitTrips(); ++round) {
            ++split_reruns_;
            CHECK_STATUS(ForwardAsync());
            --forward_count_;
            SI_TRY_HIP(si_hip_stream_sync(context_->stream()), "stream sync");
        }
    }
    if (forward_pending_) {
        si_hip_event_elapsed_ms(ev_start_, ev_stop_, &last_forward_ms_);
        forward_pending_ = false;
    }
    return Status::kSuccess;
}

bool EngineImpl::TakeSplitTrips() {
    bool any = false;
    for (size_t i = 0; i < split_convs_.size(); ++i) {
        if (split_flags_ && reinterpret_cast<volatile unsigned*>(split_flags_)[i]) {   // (written by the device into pinned host memory)
            split_flags_[i] = 0u;
            Conv2d* cv = split_convs_[i];
            if (cv->f32_split_) {
                const pnnx::Operator* op = cv->GetOp();
                LOG(WARNING) << "f32_split: an operand of conv [" << (op ? op->name : std::string("(Detect level)")) << "] left fp16's range (|x| >= 65520, or a non-finite value); "
                             << "the layer runs on the true-fp32 kernels from here on and the step is re-run";
                cv->DemoteSplit();
                any = true;
            }
        }
    }
    for (EngineImpl* lane : lanes_) any = lane->TakeSplitTrips() || any;
    if (slicer_) any = slicer_->TakeSplitTrips() || any;
    if (any) {
        // captured graphs hold the split launches, and the demoted layers re-pack their weights at their next launch: eager once
        DestroyGraphCache();
        plan_warm_ = false;
    }
    return any;
}

std::vector<std::string> EngineImpl::SplitDemoted() const {
    std::vector<std::string> out;
    for (Conv2d* cv : split_convs_)
        if (cv->split_demoted_) out.push_back(cv->GetOp() ? cv->GetOp()->name : std::string("detect_level"));
    for (const EngineImpl* lane : lanes_)
        for (auto& n : lane->SplitDemoted()) out.push_back(n);
    if (slicer_)
        for (auto& n : slicer_->SplitDemoted()) out.push_back(n);
    return out;
}

Status EngineImpl::ForwardAsync() {
    if (nullptr == context_ || (plan_.empty() && lanes_.empty())) {
        LOG(ERROR) << "Forward before a successful LoadModel";
        return Status::kFail;
    }
    si_hip_set_device(context_->device());
    si_stream_t stream = context_->stream();
    if (const int slices = PlanSlices(); slices > 1) {
        if (slicer_ != nullptr && slices_ == slices) return ForwardSliced(slices);
        if (Status::kSuccess == SetupSlicer(slices)) return ForwardSliced(slices);
        // (a second arena that does not fit, an operator the re-batch rule cannot serve ...): the unsliced schedule below worked
        // before there was a pipeline and still does; remembered, so the setup is not retried on every Forward
        LOG(ERROR) << "host_slices: could not set up " << slices << " pipelined slices; serving this engine unsliced";
        DestroySlicer();
        slicer_failed_ = true;
    }
    last_slices_ = 1;
    CHECK_STATUS(EnsureArena());
    CHECK_STATUS(UploadInputs());
    CHECK_STATUS(BindOutputs());
    if (!lanes_.empty()) CHECK_STATUS(BindLanes());

    SI_TRY_HIP(si_hip_event_record(ev_start_, stream), "event record");
    if (opt_graph_ && plan_warm_ && lanes_.empty()) {
        // a captured graph bakes pointers in: key the cache on where the device-resident inputs and the outputs are now
        std::vector<void*> key;
        for (auto& kv : input_tensor_nodes_) key.push_back(kv.second->tensor.RawData());
        for (auto& kv : output_tensor_nodes_) key.push_back(kv.second->tensor.RawData());
        si_graph_t exec = nullptr;
        for (size_t i = 0; i < graph_cache_.size(); ++i) {
            if (graph_cache_[i].first == key) {
                exec = graph_cache_[i].second;
                if (i != 0) std::rotate(graph_cache_.begin(), graph_cache_.begin() + i, graph_cache_.begin() + i + 1);  // most recent first
                break;
            }
        }
        if (!exec) {
            SI_TRY_HIP(si_hip_graph_begin_capture(stream), "begin capture");
            Status ret = LaunchAll();
            const int rc = si_hip_graph_end_capture(stream, &exec);
            if (Status::kSuccess != ret || rc != 0) {
                // a launch that could not be captured (a layer fell back to another kernel family at this view and had to re-pack and upload
                // its weights, which a capture forbids -- ADVICE r05): the capture is discarded and this step runs eagerly; the next one captures
                if (exec) si_hip_graph_destroy(exec);
                LOG(WARNING) << "graph: the capture of this step failed; running it eagerly";
                CHECK_STATUS(LaunchAll());
                SI_TRY_HIP(si_hip_event_record(ev_stop_, stream), "event record");
                if (opt_outputs_to_host_) {
                    for (auto& kv : output_tensor_nodes_) {
                        const Tensor& t = kv.second->tensor;
                        SI_TRY_HIP(si_hip_memcpy_d2h(host_outputs_[kv.first], t.RawData(), t.ByteSize(), stream), "output d2h");
                    }
                }
                forward_pending_ = true;
                ++forward_count_;
                return Status::kSuccess;
            }
            if (graph_cache_.size() >= max_graphs_) {
                // the evicted exec may be the one a not-yet-synchronised ForwardAsync() launched: let the stream drain first
                SI_TRY_HIP(si_hip_stream_sync(stream), "stream sync");
                si_hip_graph_destroy(graph_cache_.back().second);
                graph_cache_.pop_back();
            }
            graph_cache_.insert(graph_cache_.begin(), std::make_pair(key, exec));
        }
        SI_TRY_HIP(si_hip_graph_launch(exec, stream), "graph launch");
    } else {
        // the first pass over this engine's own plan is always eager: it uploads weights and sizes scratch buffers (a Forward
        // served by the sliced host pipeline does not count: that ran the slicer's plan)
        CHECK_STATUS(LaunchAll());
        plan_warm_ = true;
    }
    SI_TRY_HIP(si_hip_event_record(ev_stop_, stream), "event record");

    if (opt_outputs_to_host_) {
        for (auto& kv : output_tensor_nodes_) {
            const Tensor& t = kv.second->tensor;
            SI_TRY_HIP(si_hip_memcpy_d2h(host_outputs_[kv.first], t.RawData(), t.ByteSize(), stream), "output d2h");
        }
    }
    forward_pending_ = true;
    ++forward_count_;
    return Status::kSuccess;
}

Status EngineImpl::Extract(const std::string& name, Tensor& output) {
    auto it = output_tensor_nodes_.find(name);
    if (it == output_tensor_nodes_.end()) {
        LOG(ERROR) << "tensor [" << name << "] is not an output tensor";
        return Status::kFail;
    }
    const Tensor& t = it->second->tensor;
    if (opt_outputs_to_host_) {
        output = Tensor(t.GetDataType(), t.Shape(), MemoryType::kHost, false);
        output.SetData(host_outputs_[name], MemoryType::kHost);
    } else {
        output = t;  // non-owning device view
    }
    return Status::kSuccess;
}

Status EngineImpl::Profile(std::vector<LayerProfile>& layers) {
    layers.clear();
    if (nullptr == context_ || (plan_.empty() && lanes_.empty())) return Status::kFail;
    si_stream_t stream = context_->stream();
    CHECK_STATUS(EnsureArena());
    CHECK_STATUS(UploadInputs());
    CHECK_STATUS(BindOutputs());
    if (!lanes_.empty()) {
        // per-launch durations are measured WITHOUT the overlap: one lane after the other, each layer between two events (as
        // Detect's side-stream levels are, below).  A layer appears once per lane, with that lane's FLOPs and bytes.
        CHECK_STATUS(BindLanes());
        SI_TRY_HIP(si_hip_stream_sync(stream), "stream sync");
        for (EngineImpl* lane : lanes_) {
            std::vector<LayerProfile> part;
            CHECK_STATUS(lane->Profile(part));
            layers.insert(layers.end(), part.begin(), part.end());
        }
        return Status::kSuccess;
    }
    std::vector<si_event_t> ev(plan_.size() + 1, nullptr);
    for (auto& e : ev) SI_TRY_HIP(si_hip_event_create(&e), "event create");
    Status ret = Status::kSuccess;
    si_hip_event_record(ev[0], stream);
    // (per-layer timing: Detect runs whole on the main stream here, whatever "detect_stream" says)
    std::vector<std::pair<YoloDetect*, unsigned>> early;
    for (const Step& st : plan_)
        if (YoloDetect* d = dynamic_cast<YoloDetect*>(st.layer))
            if (d->EarlyLevels()) { early.push_back(std::make_pair(d, d->EarlyLevels())); d->SetEarlyLevels(nullptr, 0); }
    for (size_t i = 0; i < plan_.size() && ret == Status::kSuccess; ++i) {
        ret = plan_[i].layer->Forward();
        si_hip_event_record(ev[i + 1], stream);
    }
    si_hip_stream_sync(stream);
    for (auto& e : early) e.first->SetEarlyLevels(side_context_, e.second);
    if (ret == Status::kSuccess) {
        for (size_t i = 0; i < plan_.size(); ++i) {
            LayerProfile p;
            p.name = plan_[i].op->name;
            p.type = plan_[i].op->type;
            p.kernel = plan_[i].layer->KernelName();
            si_hip_event_elapsed_ms(ev[i], ev[i + 1], &p.ms);
            p.flops = plan_[i].layer->Flops();
            p.bytes = plan_[i].layer->Bytes();
            layers.push_back(p);
        }
    }
    for (auto& e : ev) si_hip_event_destroy(e);
    return ret;
}

void* EngineImpl::Stream() { return context_ ? context_->stream() : nullptr; }

std::vector<std::string> EngineImpl::ScheduledOps() const {
    if (!lanes_.empty()) return lanes_[0]->ScheduledOps();
    std::vector<std::string> out;
    for (const Step& s : plan_) out.push_back(s.op->name);
    return out;
}

std::vector<std::string> EngineImpl::FusedOps() const {
    if (!lanes_.empty()) return lanes_[0]->FusedOps();
    std::vector<std::string> out(fused_ops_.begin(), fused_ops_.end());
    out.insert(out.end(), sibling_ops_.begin(), sibling_ops_.end());
    return out;
}

std::vector<std::string> EngineImpl::AliasedOperands() const {
    if (!lanes_.empty()) return lanes_[0]->AliasedOperands();
    std::vector<std::string> out;
    for (auto& kv : aliases_) out.push_back(kv.first);
    return out;
}

}  // namespace SimpleInfer
