#include "cat.h"

#include "layer_util.h"
#include "si_hip.h"
#include "si_slice.h"

namespace SimpleInfer {

DEFINE_LAYER_REGISTRY(Cat);

Status Cat::Init(const pnnx::Operator* op) {
    CHECK_STATUS(Layer::Init(op));
    CHECK_BOOL(Get(op, "dim", dim_));
    return Status::kSuccess;
}

Status Cat::Validate() {
    CHECK_STATUS(Layer::Validate());
    CHECK_STATUS(ValidateShape(-1, 1));
    if (Status::kSuccess != ValidateFloat()) {
        LOG(ERROR) << "Cat::Validate fail [unsupport data type]";
        return Status::kUnsupport;
    }
    // below rank 4 `dim` is the file's own: checked here, at LoadModel (rank 4 keeps the NCHW remap and its checks in Forward)
    const int rank = output_tensor_nodes_.empty() ? 4 : (int)output_tensor_nodes_[0]->tensor.Shape().size();
    if (rank < 4 && (dim_ < -rank || dim_ >= rank)) {
        LOG(ERROR) << "Cat::Validate fail [dim " << dim_ << " of a rank-" << rank << " tensor]";
        return Status::kErrorShape;
    }
    return Status::kSuccess;
}

int Cat::NhwcAxis() const {
    switch (dim_) {
        case 1: return 3;
        case 2: return 1;
        case 3: return 2;
        default: return dim_;
    }
}

// the output as four dimensions and the concat axis among them: rank 4 is NHWC with NhwcAxis(); rank 3 [N, L, K] is [N, 1, L, K] and rank 2
// [N, F] is [N, 1, 1, F], `dim` being the file's there (no NCHW remap below rank 4; negative: from the end)
static bool Shape4(const Tensor& t, int rank, int s[4]) {
    const std::vector<int>& v = t.Shape();
    if ((int)v.size() != rank) return false;
    s[0] = v[0];
    for (int k = 1; k < 4; ++k) s[k] = k < 5 - rank ? 1 : v[(size_t)(k - (4 - rank))];   // the batch stays in front, the rest is right-aligned
    return s[0] > 0 && s[1] > 0 && s[2] > 0 && s[3] > 0;
}

Status Cat::Forward(const std::vector<Tensor>& inputs, Tensor& output) {
    const int rank = (int)output.Shape().size();
    if (rank < 2 || rank > 4) {
        LOG(ERROR) << "Cat::Forward fail [unsupport output shape]";
        return Status::kUnsupport;
    }
    if (inputs.size() < 2) {
        LOG(ERROR) << "Cat::Forward fail [unsupport inputs size]";
        return Status::kUnsupport;
    }
    int axis = NhwcAxis();
    if (rank < 4) {
        const int dim = dim_ < 0 ? dim_ + rank : dim_;
        if (dim < 0 || dim >= rank) return Status::kUnsupport;
        axis = dim == 0 ? 0 : dim + (4 - rank);
    }
    if (axis < 0 || axis > 3) return Status::kUnsupport;

    std::vector<const Tensor*> ins;
    for (auto& t : inputs) ins.push_back(&t);
    return RunOnDevice(ins, {&output}, [this, axis, rank](const std::vector<Tensor>& in, std::vector<Tensor>& out) {
        int os[4];
        if (!Shape4(out[0], rank, os)) return Status::kErrorShape;
        Dims4 od;
        od.n = os[0]; od.h = os[1]; od.w = os[2]; od.c = os[3];
        int offset = 0;
        int copies = 0;
        const bool half = IsHalf(out[0]);
        // fp16 tensors are copied as 4-byte words (pure data movement) where channel counts / strides / offsets are even
        const int wd = half ? 2 : 1;
        for (const Tensor& t : in) {
            int is[4];
            if (!Shape4(t, rank, is)) return Status::kErrorShape;
            Dims4 id;
            id.n = is[0]; id.h = is[1]; id.w = is[2]; id.c = is[3];
            if (IsHalf(t) != half) return Status::kUnsupport;
            if (axis == 3) {
                char* dst = static_cast<char*>(out[0].RawData()) + (size_t)offset * (half ? 2 : 4);
                // already in place: the engine pointed this input at its slice of our output
                if (t.RawData() != dst || t.PixelStride() != out[0].PixelStride()) {
                    ++copies;
                    if (id.c % wd || t.PixelStride() % wd || out[0].PixelStride() % wd || offset % wd) {
                        // an odd count of halves (the 3-channel Focus slices of an RGB image): 2-byte elements through the split kernel
                        const int first = 0, width = id.c, ld = out[0].PixelStride();
                        void* to = dst;
                        CHECK_STATUS(CheckHip(si_hip_split_channels_f16(t.RawData(), id.pixels(), id.c, t.PixelStride(), 1, &first, &width, &to, &ld,
                                                                        Stream()),
                                              "Cat"));
                        offset += is[axis];
                        continue;
                    }
                    CHECK_STATUS(CheckHip(si_hip_copy_channels_f32(static_cast<const float*>(t.RawData()), id.pixels(), id.c / wd,
                                                                   t.PixelStride() / wd, reinterpret_cast<float*>(dst),
                                                                   out[0].PixelStride() / wd, Stream()),
                                          "Cat"));
                }
            } else {
                ++copies;
                if (t.PixelStride() != id.c || out[0].PixelStride() != od.c) return Status::kUnsupport;
                if (half && id.c % 2 && rank < 4) {   // (rank 4 keeps its refusal below: unchanged behaviour)
                    // an odd count of halves ([N, A, 3] score rows): dense tensors, so the concat is rows of `run` elements laid into rows of
                    // `pitch` -- one destination of the split kernel, 2-byte elements
                    size_t outer = 1;
                    int inner = 1;
                    for (int k = 0; k < axis; ++k) outer *= (size_t)is[k];
                    for (int k = axis + 1; k < 4; ++k) inner *= is[k];
                    const int first = 0, run = is[axis] * inner, pitch = os[axis] * inner;
                    void* to = static_cast<char*>(out[0].RawData()) + (size_t)offset * inner * 2;
                    CHECK_STATUS(CheckHip(si_hip_split_channels_f16(t.RawData(), outer, run, run, 1, &first, &run, &to, &pitch, Stream()), "Cat"));
                } else if (half) {
                    if (id.c % 2) return Status::kUnsupport;
                    int isw[4] = {is[0], is[1], is[2], is[3] / 2}, osw[4] = {os[0], os[1], os[2], os[3] / 2};
                    CHECK_STATUS(CheckHip(si_hip_cat_axis_f32(static_cast<const float*>(t.RawData()), isw,
                                                              static_cast<float*>(out[0].RawData()), osw, axis, offset, Stream()),
                                          "Cat"));
                } else {
                    CHECK_STATUS(CheckHip(si_hip_cat_axis_f32(t.Data<float>(), is, out[0].Data<float>(), os, axis,
                                                              offset, Stream()),
                                          "Cat"));
                }
            }
            offset += is[axis];
        }
        last_copies_ = copies;
        return offset == os[axis] ? Status::kSuccess : Status::kErrorShape;
    });
}

}  // namespace SimpleInfer
