// engine_split.cpp -- the batch-split modes of EngineImpl: half-batch lanes ("streams") and the sliced host pipeline ("host_slices"), on child engines made by NewChild.
#include <algorithm>

#include "engine_impl.h"
#include "engine_internal.h"

namespace SimpleInfer {

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
    if (is_lane_ || opt_.streams < 2) return Status::kSuccess;
    int batch = 0;
    const bool ok = BatchSplittable(batch) && batch % 2 == 0;
    if (opt_.streams >= 2) {
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

// A lane or the sliced pipeline's engine: this model loaded again at `batch` under this engine's options (EngineOptions::ForChild), with a
// graph cache of at least `min_graphs`.  `child` is set before the load, so the caller's DestroyLanes / DestroySlicer owns a child that failed.
Status EngineImpl::NewChild(int batch, size_t min_graphs, EngineImpl*& child) {
    child = new EngineImpl;
    child->is_lane_ = true;
    child->opt_ = opt_.ForChild(context_->device(), batch);
    child->max_graphs_ = std::max(max_graphs_, min_graphs);
    return child->LoadModel(param_path_, bin_path_);
}

Status EngineImpl::LoadLanes(int lanes) {
    int batch = input_tensor_nodes_.begin()->second->tensor.Shape()[0];
    for (int l = 0; l < lanes; ++l) {
        lanes_.push_back(nullptr);   // (stored before the load is checked: a lane that fails to load is still destroyed by DestroyLanes)
        CHECK_STATUS(NewChild(batch / lanes, 0, lanes_.back()));
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
    if (is_lane_ || opt_.host_slices == 1 || !opt_.outputs_to_host || slicer_failed_) return 1;
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
            if (opt_.host_slices > 1)
                LOG(ERROR) << "host_slices=" << opt_.host_slices << " needs per-image operators; serving this engine unsliced.  Not per-image: " << BatchMixingText();
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
    if (opt_.host_slices > 1) return batch % opt_.host_slices == 0 ? opt_.host_slices : 1;
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
    CHECK_STATUS(NewChild(batch / slices, (size_t)slices, slicer_));   // one captured graph per slice (its I/O pointers key the cache): the cache holds at least one per slice
    up_context_ = new Context;
    CHECK_STATUS(up_context_->Init(context_->device()));
    if (opt_.fail_slicer) return Status::kFail;
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
        if (opt_.pin_inputs && ++p.seen == 2 && !p.registered) {
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

}  // namespace SimpleInfer
