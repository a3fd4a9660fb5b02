#include "slice.h"

#include <algorithm>
#include <climits>
#include <cstring>

namespace SimpleInfer {

DEFINE_LAYER_REGISTRY(Slice);

// A missing or mistyped key is kFail; values the rule does not allow are left for Validate, which knows the shape.
Status Slice::Init(const pnnx::Operator* op) {
    CHECK_STATUS(Layer::Init(op));
    int dim = 0;
    dims_.clear(); starts_.clear(); ends_.clear(); steps_.clear(); has_end_.clear(); sections_.clear();
    if (op->type == "torch.chunk") {
        kind_ = Kind::kChunk;
        CHECK_BOOL(Get(op, "chunks", chunks_) && Get(op, "dim", dim));
        dims_.push_back(dim);
        return Status::kSuccess;
    }
    if (op->type == "torch.split") {
        kind_ = Kind::kSplit;
        CHECK_BOOL(Get(op, "dim", dim));
        dims_.push_back(dim);
        const char* key = "split_size_or_sections";
        int size = 0;
        sections_is_list_ = !Get(op, key, size);
        if (!sections_is_list_) sections_.push_back(size);
        CHECK_BOOL(!sections_is_list_ || Get(op, key, sections_));
        return Status::kSuccess;
    }
    kind_ = Kind::kSlice;
    if (FindParam(op, "dims")) {
        CHECK_BOOL(Get(op, "dims", dims_));
        const size_t k = dims_.size();
        auto list = [&](const char* key, std::vector<int>& v, int dflt, std::vector<bool>* have) {
            const bool given = !IsNone(op, key);   // (a list or nothing: the string "None" is refused)
            if (given && !(Get(op, key, v) && v.size() == k)) return false;
            if (!given) v.assign(k, dflt);
            if (have) have->assign(k, given);
            return true;
        };
        CHECK_BOOL(list("starts", starts_, 0, nullptr));
        CHECK_BOOL(list("ends", ends_, INT_MAX, &has_end_));
        CHECK_BOOL(list("steps", steps_, 1, nullptr));
        return Status::kSuccess;
    }
    CHECK_BOOL(Get(op, "dim", dim));
    dims_.push_back(dim);
    int start = 0, end = INT_MAX, step = 1;
    bool have = false, have_end = false;
    CHECK_BOOL(OptionalInt(op, "start", start, have));
    CHECK_BOOL(OptionalInt(op, "end", end, have_end));
    CHECK_BOOL(OptionalInt(op, "step", step, have));
    starts_.push_back(start);
    ends_.push_back(end);
    steps_.push_back(step);
    has_end_.push_back(have_end);
    return Status::kSuccess;
}

bool Slice::ChannelRange(const Piece& p, const int in_dims[4]) {
    for (int a = 0; a < 3; ++a)
        if (p.start[a] != 0 || p.step[a] != 1 || p.dims[a] != in_dims[a]) return false;
    return p.step[3] == 1;
}

// kErrorShape: the parameters do not fit the shape (the log says how); kUnsupport: an axis this rank does not have here
Status Slice::MakePieces(const int in_dims[4], int rank, std::vector<Piece>& pieces) const {
    pieces.clear();
    auto axis_of = [&](int dim, int& axis) {
        if (dim < 0) dim += rank;
        if (dim < 0 || dim >= rank) return false;
        if (rank == 2) {
            axis = 3;
            return dim == 1;
        }
        static const int map[4] = {0, 3, 1, 2};   // NCHW dim -> NHWC axis (Cat::NhwcAxis)
        axis = map[dim];
        return true;
    };
    Piece whole;
    for (int a = 0; a < 4; ++a) whole.dims[a] = in_dims[a];
    if (kind_ != Kind::kSlice) {
        int axis = 0;
        if (!axis_of(dims_[0], axis)) {
            LOG(ERROR) << "Slice: dim " << dims_[0] << " of a rank-" << rank << " tensor (rank 4: every dim, rank 2: dim 1)";
            return Status::kUnsupport;
        }
        const int size = in_dims[axis];
        std::vector<int> lens;
        if (kind_ == Kind::kChunk || !sections_is_list_) {
            const int arg = kind_ == Kind::kChunk ? chunks_ : sections_[0];
            if (arg < 1) {
                LOG(ERROR) << "Slice: " << (kind_ == Kind::kChunk ? "chunks " : "split_size ") << arg << " is below 1";
                return Status::kErrorShape;
            }
            const int each = kind_ == Kind::kChunk ? (size + arg - 1) / arg : arg;   // torch: ceil(size / chunks), a smaller last piece
            for (int at = 0; at < size; at += each) lens.push_back(std::min(each, size - at));
        } else {
            long long sum = 0;
            for (int s : sections_) {
                if (s < 1) {
                    LOG(ERROR) << "Slice: a section of " << s << " elements (an empty result)";
                    return Status::kErrorShape;
                }
                sum += s;
            }
            if (sum != size) {
                LOG(ERROR) << "Slice: the sections sum to " << sum << ", the dimension has " << size;
                return Status::kErrorShape;
            }
            lens = sections_;
        }
        int at = 0;
        for (int len : lens) {
            Piece p = whole;
            p.start[axis] = at;
            p.dims[axis] = len;
            pieces.push_back(p);
            at += len;
        }
        return Status::kSuccess;
    }
    Piece p = whole;
    bool seen[4] = {false, false, false, false};
    for (size_t i = 0; i < dims_.size(); ++i) {
        int axis = 0;
        if (!axis_of(dims_[i], axis) || seen[axis]) {
            LOG(ERROR) << "Slice: dim " << dims_[i] << " of a rank-" << rank << " tensor (rank 4: every dim once, rank 2: dim 1)";
            return Status::kUnsupport;
        }
        seen[axis] = true;
        const long long size = in_dims[axis];
        long long start = starts_[i], end = has_end_[i] ? ends_[i] : size, step = steps_[i];
        if (step < 1) {
            LOG(ERROR) << "Slice: step " << step << " (steps are at least 1)";
            return Status::kErrorShape;
        }
        if (start < 0) start += size;
        if (end < 0) end += size;
        start = std::min(std::max(start, 0LL), size);
        end = std::min(std::max(end, 0LL), size);
        const long long len = end > start ? (end - start + step - 1) / step : 0;
        if (len < 1) {
            LOG(ERROR) << "Slice: [" << starts_[i] << ":" << ends_[i] << ":" << step << "] of a dimension of " << size << " is empty";
            return Status::kErrorShape;
        }
        p.start[axis] = (int)start;
        p.step[axis] = (int)step;
        p.dims[axis] = (int)len;
    }
    pieces.push_back(p);
    return Status::kSuccess;
}

Status Slice::Validate() {
    CHECK_STATUS(Layer::Validate());
    CHECK_STATUS(ValidateShape(1, -1));
    if (output_tensor_nodes_.empty()) {
        LOG(ERROR) << "Slice::Validate fail [no output]";
        return Status::kErrorShape;
    }
    const Tensor& in = input_tensor_nodes_[0]->tensor;
    // fp32 or fp16 storage.  The kernels want the same type on every operand; at the graph boundary of an fp16 engine the types differ
    // (a slice of the caller's fp32 image), which the base class's HalfStorageOk reports and the engine answers with fp32 shadows and casts
    CHECK_STATUS(ValidateFloatLogged("Slice"));
    int id[4];
    const int rank = (int)in.Shape().size();
    if (!NhwcDims(in, id)) {
        LOG(ERROR) << "Slice::Validate fail [a rank-" << rank << " input " << ShapeString(in.Shape()) << " (NHWC): rank 4, or rank 2 on dim 1]";
        return Status::kUnsupport;
    }
    CHECK_STATUS(MakePieces(id, rank, pieces_));
    if (pieces_.size() != output_tensor_nodes_.size()) {
        LOG(ERROR) << "Slice::Validate fail [" << output_tensor_nodes_.size() << " outputs in the file, the rule gives " << pieces_.size()
                   << " for input " << ShapeString(in.Shape()) << " (NHWC)]";
        return Status::kErrorShape;
    }
    for (size_t i = 0; i < pieces_.size(); ++i) {
        const Tensor& out = output_tensor_nodes_[i]->tensor;
        int od[4];
        if ((int)out.Shape().size() != rank || !NhwcDims(out, od)) {
            LOG(ERROR) << "Slice::Validate fail [output " << i << " " << ShapeString(out.Shape()) << " for a rank-" << rank << " input]";
            return Status::kUnsupport;
        }
        if (memcmp(od, pieces_[i].dims, sizeof(od)) != 0) {
            LOG(ERROR) << "Slice::Validate fail [output " << i << " is " << ShapeString(out.Shape()) << " for input " << ShapeString(in.Shape())
                       << " (NHWC); the rule gives " << pieces_[i].dims[0] << "x" << pieces_[i].dims[1] << "x" << pieces_[i].dims[2] << "x"
                       << pieces_[i].dims[3] << "]";
            return Status::kErrorShape;
        }
    }
    return Status::kSuccess;
}

int Slice::Route(const Piece& p, const int in_dims[4], const Tensor& in, const Tensor& out) {
    if (!ChannelRange(p, in_dims)) return 2;
    const char* at = static_cast<const char*>(in.RawData()) + (size_t)p.start[3] * ElementSize(in.GetDataType());
    return (in.RawData() && out.RawData() == at && out.PixelStride() == in.PixelStride()) ? 0 : 1;
}

Status Slice::Run(const Tensor& input, const std::vector<Tensor*>& outputs) {
    if (outputs.size() != pieces_.size()) return Status::kErrorShape;
    return RunOnDevice({&input}, outputs, [this](const std::vector<Tensor>& in, std::vector<Tensor>& out) {
        int id[4];
        if (!NhwcDims(in[0], id)) return Status::kErrorShape;
        const bool half = IsHalf(in[0]);
        std::vector<int> offsets, widths, lds;
        std::vector<void*> dsts;
        for (size_t i = 0; i < out.size(); ++i) {
            if (IsHalf(out[i]) != half) return Status::kUnsupport;
            const Piece& p = pieces_[i];
            const int route = Route(p, id, in[0], out[i]);
            if (route == 0) continue;   // already in place: the engine pointed this output at its channels of our input
            if (route == 1) {
                offsets.push_back(p.start[3]);
                widths.push_back(p.dims[3]);
                lds.push_back(out[i].PixelStride());
                dsts.push_back(out[i].RawData());
                continue;
            }
            CHECK_STATUS(LaunchDesc(si_hip_slice_f32, si_hip_slice_f16, "Slice", in[0], out[i], [&](const Tensor& src, const Tensor& dst, SiSliceDesc& d) {
                memset(&d, 0, sizeof(d));
                d.n = id[0]; d.ih = id[1]; d.iw = id[2]; d.ic = id[3]; d.in_ld = src.PixelStride();
                for (int a = 0; a < 4; ++a) { d.start[a] = p.start[a]; d.step[a] = p.step[a]; }
                d.on = p.dims[0]; d.oh = p.dims[1]; d.ow = p.dims[2]; d.oc = p.dims[3]; d.out_ld = dst.PixelStride();
                return true;
            }));
        }
        if (dsts.empty()) return Status::kSuccess;
        const size_t pixels = (size_t)id[0] * id[1] * id[2];
        const int k = (int)dsts.size();
        const int rc = half ? si_hip_split_channels_f16(in[0].RawData(), pixels, id[3], in[0].PixelStride(), k, offsets.data(), widths.data(),
                                                        dsts.data(), lds.data(), Stream())
                            : si_hip_split_channels_f32(in[0].RawData(), pixels, id[3], in[0].PixelStride(), k, offsets.data(), widths.data(),
                                                        dsts.data(), lds.data(), Stream());
        return CheckHip(rc, "Slice");
    });
}

Status Slice::Forward(const Tensor& input, Tensor& output) { return Run(input, {&output}); }

Status Slice::Forward(const Tensor& input, std::vector<Tensor>& outputs) {
    std::vector<Tensor*> outs;
    for (Tensor& t : outputs) outs.push_back(&t);
    return Run(input, outs);
}

const char* Slice::KernelName() const {
    int id[4];
    if (input_tensor_nodes_.empty() || pieces_.size() != output_tensor_nodes_.size() || !NhwcDims(input_tensor_nodes_[0]->tensor, id)) return "slice";
    bool split = false, slice = false;
    for (size_t i = 0; i < pieces_.size(); ++i) {
        const int route = Route(pieces_[i], id, input_tensor_nodes_[0]->tensor, output_tensor_nodes_[i]->tensor);
        split = split || route == 1;
        slice = slice || route == 2;
    }
    return split ? "split_channels" : (slice ? "slice" : "view");
}

}  // namespace SimpleInfer
