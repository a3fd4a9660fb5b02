// layer_util.h -- small helpers shared by the concrete layers.
#ifndef SIMPLE_INFER_SRC_LAYER_UTIL_H_
#define SIMPLE_INFER_SRC_LAYER_UTIL_H_

#include <cstring>
#include <sstream>
#include <string>
#include <vector>

#include "logger.h"
#include "pnnx/ir.h"
#include "pnnx/param_read.h"
#include "pnnx/pnnx_helper.h"
#include "si_hip.h"
#include "tensor.h"
#include "types.h"

namespace SimpleInfer {

struct Dims4 {
    int n = 0, h = 0, w = 0, c = 0;
    size_t pixels() const { return (size_t)n * h * w; }
};

// NHWC view of a rank-4 tensor
inline bool GetDims4(const Tensor& t, Dims4& d) {
    const std::vector<int>& s = t.Shape();
    if (s.size() != 4) return false;
    d.n = s[0]; d.h = s[1]; d.w = s[2]; d.c = s[3];
    return d.n > 0 && d.h > 0 && d.w > 0 && d.c > 0;
}

// any rank as [pixels, channels]: last dim = channels, the rest folded
inline bool GetPixelsChannels(const Tensor& t, size_t& pixels, int& c) {
    const std::vector<int>& s = t.Shape();
    if (s.empty()) return false;
    c = s.back();
    pixels = 1;
    for (size_t i = 0; i + 1 < s.size(); ++i) pixels *= (size_t)s[i];
    return c > 0 && pixels > 0;
}

// rank 4: NHWC; rank 2 [N, F]: [N, 1, 1, F]; no other rank
static inline bool NhwcDims(const Tensor& t, int d[4]) {
    const std::vector<int>& s = t.Shape();
    if (s.size() != 4 && s.size() != 2) return false;
    const bool r4 = s.size() == 4;
    d[0] = s[0]; d[1] = r4 ? s[1] : 1; d[2] = r4 ? s[2] : 1; d[3] = s.back();
    return d[0] > 0 && d[1] > 0 && d[2] > 0 && d[3] > 0;
}

// "2x3x4" for the log messages; TupleString: "(2,3,4)"
static inline std::string ShapeString(const std::vector<int>& s, const char* sep = "x") {
    std::ostringstream os;
    for (size_t i = 0; i < s.size(); ++i) os << (i ? sep : "") << s[i];
    return os.str();
}
static inline std::string TupleString(const std::vector<int>& s) { return "(" + ShapeString(s, ",") + ")"; }

// ---- reductions over `dim` (Reduce, LpNorm): the file's parameters, the NHWC mask of its dims and the shape the rule gives

// the NHWC axis of an NCHW dim (negative: from the end) of a rank-4 tensor, or of a dim of [N, F]; -1: out of range, or another rank
static inline int NhwcAxisOfDim(int dim, int rank) {
    if (dim < 0) dim += rank;
    if (dim < 0 || dim >= rank) return -1;
    if (2 == rank) return 1 == dim ? 3 : 0;
    if (4 != rank) return -1;
    switch (dim) {   // Cat::NhwcAxis
        case 1: return 3;
        case 2: return 1;
        case 3: return 2;
        default: return 0;
    }
}

// `dim` an int or a non-empty int array, `keepdim` a bool (missing: as it stands), `dtype` None if present.  A mistyped key is kFail; a
// missing dim (the reduction to a scalar) and a dtype are kUnsupport with the reason logged.
static inline Status ReadDimKeepdimDtype(const char* layer, const pnnx::Operator* op, std::vector<int>& dims, bool& keepdim) {
    if (IsNone(op, "dim")) {
        LOG(ERROR) << layer << "::Init fail [" << op->type << " without dim: the reduction to a scalar is not served]";
        return Status::kUnsupport;
    }
    int one = 0;
    dims.clear();
    if (Get(op, "dim", one)) {
        dims.push_back(one);
    } else {
        CHECK_BOOL(Get(op, "dim", dims) && !dims.empty());
    }
    if (FindParam(op, "keepdim")) CHECK_BOOL(Get(op, "keepdim", keepdim));
    if (!IsNoneOrText(op, "dtype")) {
        LOG(ERROR) << layer << "::Init fail [" << op->type << " with a dtype: the result has the input's type here]";
        return Status::kUnsupport;
    }
    return Status::kSuccess;
}

// the mask (bit a: NHWC axis a, SI_REDUCE_AXIS_*) of `dims` on a tensor of this rank; kUnsupport / kFail with the reason logged
static inline Status DimsToNhwcMask(const char* layer, const std::vector<int>& dims, int rank, int& axes) {
    axes = 0;
    for (int dim : dims) {
        const int axis = NhwcAxisOfDim(dim, rank);
        if (axis < 0) {
            LOG(ERROR) << layer << ": dim " << dim << " of " << TupleString(dims) << " is out of range for a rank-" << rank << " tensor";
            return Status::kUnsupport;
        }
        if (axes & (1 << axis)) {
            LOG(ERROR) << layer << ": dim " << dim << " appears twice in " << TupleString(dims);
            return Status::kFail;
        }
        axes |= 1 << axis;
    }
    return axes != 0 ? Status::kSuccess : Status::kFail;
}

// a mask that reduces the channels (bit 3) together with another axis is not served: kUnsupport with the reason logged
static inline Status RefuseChannelMix(const char* layer, const std::vector<int>& dims, const std::vector<int>& shape, int axes) {
    if (!(axes & 8) || axes == 8) return Status::kSuccess;
    LOG(ERROR) << layer << "::Validate fail [dim " << TupleString(dims) << " of " << ShapeString(shape)
               << " (NHWC) reduces the channels together with another axis: the channel dim alone, or any of the others]";
    return Status::kUnsupport;
}

// the keepdim=True shape of a mask as the engine holds it: NHWC for rank 4, [N, F] for rank 2 (id: NhwcDims)
static inline std::vector<int> KeptDimsShape(const int id[4], int rank, int axes) {
    if (rank != 4) return {(axes & 1) ? 1 : id[0], (axes & 8) ? 1 : id[3]};
    std::vector<int> s;
    for (int a = 0; a < 4; ++a) s.push_back(((axes >> a) & 1) ? 1 : id[a]);
    return s;
}

// a rank-1 fp32 attribute (weights, statistics) into a vector
static inline bool ReadVec(const pnnx::Operator* op, const char* key, std::vector<float>& dst) {
    if (!CheckAttr(op, key, 1)) return false;
    const pnnx::Attribute& a = op->attrs.at(key);
    if (1 != a.shape.size() || a.data.size() != (size_t)a.shape[0] * sizeof(float)) return false;
    dst.resize(a.shape[0]);
    memcpy(dst.data(), a.data.data(), a.data.size());
    return true;
}

// HBM buffer for layer parameters (weights, bias, grids): uploaded once, freed with the layer.
class DeviceBuffer {
public:
    DeviceBuffer() {}
    ~DeviceBuffer() { Free(); }
    DeviceBuffer(const DeviceBuffer&) = delete;
    DeviceBuffer& operator=(const DeviceBuffer&) = delete;

    // (re)allocates and copies synchronously; returns a C-ABI code
    int Upload(const void* host, size_t bytes) {
        if (bytes != bytes_ || !ptr_) {
            Free();
            const int rc = si_hip_malloc(&ptr_, bytes);
            if (rc != 0) return rc;
            bytes_ = bytes;
        }
        int rc = si_hip_memcpy_h2d(ptr_, host, bytes, nullptr);
        if (rc != 0) return rc;
        return si_hip_stream_sync(nullptr);
    }
    int Alloc(size_t bytes) {
        Free();
        const int rc = si_hip_malloc(&ptr_, bytes);
        if (rc == 0) bytes_ = bytes;
        return rc;
    }
    void Free() {
        if (ptr_) si_hip_free(ptr_);
        ptr_ = nullptr;
        bytes_ = 0;
    }
    template<typename T>
    T* As() const { return static_cast<T*>(ptr_); }
    size_t bytes() const { return bytes_; }

private:
    void* ptr_ = nullptr;
    size_t bytes_ = 0;
};

}  // namespace SimpleInfer

#endif
