#include "engine_impl.h"

#include <exception>

#include <algorithm>

#include "batch_rule.h"
#include "layer/conv_2d.h"
#include "layer/yolo_detect.h"
#include "engine_internal.h"
#include "layer_registry.h"
#include "pnnx/expand_expression.h"
#include "pnnx/lower_functional_conv.h"

namespace SimpleInfer {

EngineImpl::EngineImpl() {}

EngineImpl::~EngineImpl() { Release(); }

Status EngineImpl::SetOption(const std::string& key, int value) {
    if (!opt_.Set(key, value)) {   // (the keys and their rules: engine_options.h)
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
    CHECK_STATUS(context_->Init(opt_.device));
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
    // F.conv2d whose filter and bias are constants of the file with no other reader is nn.Conv2d written as a function: it becomes that
    // operator here, before layers exist and before the batch rule looks at the graph
    pnnx::lower_functional_conv(*graph_);
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
    if (opt_.batch > 0) {
        // a box head: the graph inputs [N, ...] and [K, 5] disagree in dimension 0, and where K == N by coincidence the rewrite below would
        // change the number of boxes with the number of images.  Neither is re-batched
        for (const pnnx::Operator* op : graph_->ops)
            if (BatchFamilyOf(op->type) == BatchFamily::kRoi) {
                LOG(ERROR) << "re-batch: [" << op->name << "] (" << op->type << "): " << RoiBatchReason() << ": served at the file's batch only";
                return Status::kUnsupport;
            }
        // a cross-correlation head: the filter of F.conv2d is computed from a graph input, so dimension 0 of it (and, behind the depthwise
        // sandwich's views, the channels) follows the traced batch in ways the rewrite below does not know.  Not re-batched either
        const std::set<const pnnx::Operand*> consts = ConstantOperands(graph_->ops);
        for (const pnnx::Operator* op : graph_->ops)
            if (HasTensorFilter(op, consts)) {
                LOG(ERROR) << "re-batch: [" << op->name << "] (" << op->type << "): " << XcorrBatchReason() << ": served at the file's batch only";
                return Status::kUnsupport;
            }
        for (pnnx::Operand* opd : graph_->operands)
            if (opd->producer && opd->producer->inputs.empty() && !IsAttributeOp(opd->producer) && !opd->shape.empty()) {
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
            const bool recurrent = BatchFamilyOf(op->type) == BatchFamily::kRecurrent;
            bool batch_first = false;
            Get(op, "batch_first", batch_first);
            if (op->type == "nn.MultiheadAttention" || recurrent) {
                // the layer reads the batch from dimension 0 (batch_first) or 1 of its operands: the rewrite has to have reached that one
                for (const pnnx::Operand* in : op->inputs) {
                    auto it = batch_axis.find(in);
                    if (it == batch_axis.end() || it->second != (batch_first ? 0 : 1)) {
                        LOG(ERROR) << "re-batch: [" << op->name << "] " << op->type << " with batch_first=" << (batch_first ? "True" : "False")
                                   << " reads the batch from dimension " << (batch_first ? 0 : 1) << " of operand [" << in->name
                                   << "], which the graph does not carry there from a batch-major graph input: served at the file's batch only";
                        return Status::kUnsupport;
                    }
                }
            }
            if (recurrent) {
                // ... and every output has to be followed: y in the input's batch dimension, the state outputs [layers * dirs, N, H] in 1.  One
                // that is not would keep the file's batch in its shape while the layer writes the new one
                for (size_t i = 0; i < op->outputs.size(); ++i) {
                    auto it = batch_axis.find(op->outputs[i]);
                    if (it == batch_axis.end() || it->second != (i == 0 && batch_first ? 0 : 1)) {
                        LOG(ERROR) << "re-batch: [" << op->name << "] " << op->type << ": the batch dimension of output " << i << " [" << op->outputs[i]->name
                                   << "] cannot be followed, so its shape would keep the file's batch: served at the file's batch only";
                        return Status::kUnsupport;
                    }
                }
            }
        }
    }
    // graph constants (pnnx.Attribute outputs, and what is computed from constants alone): no image of the batch, never re-batched
    const std::set<const pnnx::Operand*> constants = ConstantOperands(graph_->ops);
    for (const pnnx::Operator* op : graph_->ops) {
        if (!IsAttributeOp(op)) continue;
        auto data = op->attrs.find("data");
        if (op->outputs.size() != 1 || data == op->attrs.end()) {
            LOG(ERROR) << "pnnx.Attribute [" << op->name << "]: no data attribute (or not exactly one output)";
            return Status::kFail;
        }
        if (data->second.type != 1 || op->outputs[0]->type != 1) {
            LOG(ERROR) << "pnnx.Attribute [" << op->name << "]: constants of a type other than f32 are not served";
            return Status::kUnsupport;
        }
        size_t elems = 1;
        for (int d : op->outputs[0]->shape) elems *= d > 0 ? (size_t)d : 0;
        if (op->outputs[0]->shape.empty() || elems == 0 || data->second.shape != op->outputs[0]->shape || data->second.data.size() != elems * sizeof(float)) {
            LOG(ERROR) << "pnnx.Attribute [" << op->name << "]: the data holds " << data->second.data.size() << " bytes, the operand's shape asks for "
                       << elems * sizeof(float);
            return Status::kFail;
        }
        for (const pnnx::Operator* c : op->outputs[0]->consumers)
            if (c && c->outputs.empty()) {
                LOG(ERROR) << "pnnx.Attribute [" << op->name << "]: a constant that is a graph output directly is not served";
                return Status::kUnsupport;
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
        if (moved != batch_axis.end() && moved->second >= 1) file[moved->second] = opt_.batch;
        else if (file_batch > 0 && !file.empty() && file[0] == file_batch && !constants.count(opd)) file[0] = opt_.batch;
        std::vector<int> shape = file;
        const int rank = (int)shape.size();
        if (rank > 3) {
            shape[rank - 3] = file[rank - 2];
            shape[rank - 2] = file[rank - 1];
            shape[rank - 1] = file[rank - 3];
        }
        DataType dt = PnnxToDataType(opd->type);
        // graph inputs: produced by an operator with no inputs (pnnx.Input)
        const bool is_constant = opd->producer && IsAttributeOp(opd->producer);
        const bool is_input = opd->producer && opd->producer->inputs.empty() && !is_constant;
        // graph outputs: consumed by an operator with no outputs (pnnx.Output)
        bool is_output = false;
        for (pnnx::Operator* c : opd->consumers)
            if (c && c->outputs.empty()) is_output = true;
        // fp16 storage: every internal fp32 activation becomes fp16; the tensors the caller hands over / reads back
        // (Input / Extract) keep the file's type
        if (opt_.fp16 && dt == DataType::kFloat32 && !is_input && !is_output) dt = DataType::kFloat16;
        node->tensor = Tensor(dt, shape, MemoryType::kDevice, false);
        node->constant = is_constant;
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
        if ("pnnx.Input" == op->type || "pnnx.Output" == op->type || IsAttributeOp(op)) continue;   // (a constant has no layer and no step)
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
            cv.f32_split_level_ = opt_.f32_split_policy;
            if (opt_.plan_set) cv.SetPlan(opt_.plan);
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
            yd->fuse_decode_ = opt_.fuse;
            for (Conv2d& cv : yd->conv_2d_layer_) arm_split(cv, opt_.f32_split && !opt_.fp16 && opt_.fuse);
        }
        if (Conv2d* cv = dynamic_cast<Conv2d*>(layer)) {
            if (!opt_.winograd) cv->algo_ = Conv2d::Algo::kImplicitGemm;
            cv->prefer_wino43_ = opt_.winograd == 2;
            arm_split(*cv, opt_.f32_split && !opt_.fp16);
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
        if (kv.second->constant) {
            // outside the arena, filled once, never written; an engine that runs as lanes leaves it to them (each loads its own copy)
            if (lanes_.empty()) CHECK_STATUS(UploadConstant(kv.second));
            continue;
        }
        if (dead_operands_.count(name) || aliases_.count(name)) continue;
        if (!lanes_.empty() && !input_tensor_nodes_.count(name) && !output_tensor_nodes_.count(name)) continue;   // the lanes own the intermediates
        const size_t bytes = t.ByteSize();
        if (bytes == 0) {
            LOG(ERROR) << "operand [" << name << "] has no static shape";
            return Status::kErrorShape;
        }
        const bool io = input_tensor_nodes_.count(name) || output_tensor_nodes_.count(name);
        if (io || !opt_.arena) {
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
    const bool defer = arena_pending_ && !is_lane_ && opt_.outputs_to_host && opt_.host_slices != 1 && lanes_.empty();
    if (!defer) CHECK_STATUS(EnsureArena());
    // 3. pinned host mirrors for outputs
    if (opt_.outputs_to_host) {
        for (auto& kv : output_tensor_nodes_) {
            void* h = nullptr;
            SI_TRY_HIP(si_hip_host_alloc(&h, kv.second->tensor.ByteSize()), "hipHostMalloc output");
            host_outputs_[kv.first] = h;
        }
    }
    return Status::kSuccess;
}

// The stored image of a constant: the file's fp32 data of shape `file` under the storage rule of its rank -- rank >= 4 has its last three dims
// C,H,W stored H,W,C; the transpose happens here, on the host, once.
static std::vector<float> StoredImage(const float* src, const std::vector<int>& file) {
    size_t total = 1;
    for (int d : file) total *= (size_t)d;
    std::vector<float> dst(total);
    const size_t r = file.size();
    if (r < 4) {
        std::copy(src, src + total, dst.begin());
        return dst;
    }
    const size_t C = file[r - 3], H = file[r - 2], W = file[r - 1], lead = total / (C * H * W);
    for (size_t l = 0; l < lead; ++l)
        for (size_t c = 0; c < C; ++c)
            for (size_t h = 0; h < H; ++h)
                for (size_t w = 0; w < W; ++w) dst[((l * H + h) * W + w) * C + c] = src[((l * C + c) * H + h) * W + w];
    return dst;
}

// a constant's own buffer and those of its promoted images: allocated, filled from the Attribute's data (under fp16 storage converted to half
// once, round-to-nearest-even), bound
Status EngineImpl::UploadConstant(TensorNode* node) {
    const pnnx::Operator* op = node->operand->producer;
    const pnnx::Attribute& data = op->attrs.at("data");
    const float* src = reinterpret_cast<const float*>(data.data.data());
    const std::vector<int>& file = node->operand->shape;
    auto upload = [&](Tensor& t, int rank) -> Status {
        std::vector<int> padded((size_t)rank - file.size(), 1);
        padded.insert(padded.end(), file.begin(), file.end());
        const std::vector<float> image = StoredImage(src, padded);
        if (image.size() != t.NumElements()) return Status::kErrorShape;
        void* p = nullptr;
        SI_TRY_HIP(si_hip_malloc(&p, t.ByteSize()), "hipMalloc constant");
        device_allocs_.push_back(p);
        if (t.GetDataType() == DataType::kFloat16) {
            std::vector<unsigned short> half(image.size());
            SI_TRY_HIP(si_hip_f32_to_f16_host(image.data(), half.data(), image.size()), "constant to half");
            SI_TRY_HIP(si_hip_memcpy_h2d(p, half.data(), t.ByteSize(), nullptr), "constant h2d");
        } else {
            SI_TRY_HIP(si_hip_memcpy_h2d(p, image.data(), t.ByteSize(), nullptr), "constant h2d");
        }
        SI_TRY_HIP(si_hip_stream_sync(nullptr), "constant h2d sync");
        t.SetView(p, MemoryType::kDevice, 0);
        return Status::kSuccess;
    };
    CHECK_STATUS(upload(node->tensor, (int)file.size()));
    for (auto& kv : node->promoted) CHECK_STATUS(upload(kv.second, kv.first));
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
    for (auto& kv : tensor_nodes_) {
        kv.second->tensor.SetView(nullptr, MemoryType::kDevice, 0);
        for (auto& image : kv.second->promoted) image.second.SetView(nullptr, MemoryType::kDevice, 0);
    }
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
    if (opt_.graph && plan_warm_ && lanes_.empty()) {
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
                return EndForward();
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
    return EndForward();
}

// the end of every ForwardAsync that ran this engine's own plan: the stop event, the outputs on their way to the host mirrors, the step counted
Status EngineImpl::EndForward() {
    si_stream_t stream = context_->stream();
    SI_TRY_HIP(si_hip_event_record(ev_stop_, stream), "event record");
    if (opt_.outputs_to_host) {
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
    if (opt_.outputs_to_host) {
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
