// slice.hip -- torch.chunk / torch.split / Tensor.slice (include/si_slice.h) on NHWC fp32 and fp16 tensors with pixel strides on both
// sides.  Pure data movement: values travel as integer words, nothing here does arithmetic on a value.
//
// Both kernels are grid-stride loops (si_grid_for: at most 2048 workgroups of 256 lanes) over ITEMS of the output, an item being one
// 16-byte channel vector (the vec forms) or one element (the elem forms).  Consecutive lanes take consecutive items of a pixel, then
// consecutive pixels: a wave writes whole runs of the destination and reads runs of the source that are as long as the slice allows.
//
// Strided slice: an item's output pixel is split into (n, h, w) by three 32-bit divisions and mapped to the source pixel
// (n0 + n sn, h0 + h sh, w0 + w sw); the channel is c0 + c sc (sc == 1 in the vec form).
//
// Channel split: up to SI_SPLIT_MAX destinations in one launch.  The items of a pixel are the destinations' channel ranges laid end to end
// (`begin[k]`: where destination k starts in that order, INT_MAX behind the last one); a lane finds its destination with a chain of
// selects over the by-value argument struct -- no branch, no table in memory -- and every input vector that has a destination is read
// exactly once.
//
// Index arithmetic is 32-bit and unsigned: the host refuses tensors whose pixel counts, element offsets or item counts do not fit 31
// bits.  Register table per instantiation: DESIGN.md section 9h.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "si_hip_internal.h"
#include "si_slice.h"

namespace {

constexpr int SL_THREADS = 256;

// the integer word a <T, V> item travels as
template <typename T, int V> struct SlWord { typedef u32x4 type; };
template <> struct SlWord<float, 1> { typedef uint32_t type; };
template <> struct SlWord<_Float16, 1> { typedef uint16_t type; };

// ---- strided slice ------------------------------------------------------------------------------------------------------------
struct SliceArgs {
    const void* in;
    void* out;
    unsigned ih, iw, in_ld;
    unsigned oh, ow, out_ld;
    unsigned per_pixel;          // items of one output pixel: oc / V
    unsigned n0, h0, w0, c0;     // start[], NHWC
    unsigned sn, sh, sw, sc;     // step[]
    unsigned total;              // items of the launch (< 2^31)
};

template <typename T, int V>
__device__ __forceinline__ void slice_body(const SliceArgs& a) {
    typedef typename SlWord<T, V>::type W;
    const T* const in = static_cast<const T*>(a.in);
    T* const out = static_cast<T*>(a.out);
    const size_t stride = (size_t)gridDim.x * SL_THREADS;
    for (size_t it = (size_t)blockIdx.x * SL_THREADS + threadIdx.x; it < a.total; it += stride) {
        const unsigned i = (unsigned)it;
        const unsigned p = i / a.per_pixel, v = i - p * a.per_pixel;
        const unsigned row = p / a.ow, w = p - row * a.ow;
        const unsigned n = row / a.oh, h = row - n * a.oh;
        const unsigned sp = ((a.n0 + n * a.sn) * a.ih + a.h0 + h * a.sh) * a.iw + a.w0 + w * a.sw;
        const unsigned sc = V > 1 ? a.c0 + v * V : a.c0 + v * a.sc;
        *reinterpret_cast<W*>(out + p * a.out_ld + v * V) = *reinterpret_cast<const W*>(in + sp * a.in_ld + sc);
    }
}

template <typename T, int V>
__global__ __launch_bounds__(SL_THREADS) void slice_vec(SliceArgs a) { slice_body<T, V>(a); }

template <typename T>
__global__ __launch_bounds__(SL_THREADS) void slice_elem(SliceArgs a) { slice_body<T, 1>(a); }

// ---- channel split ------------------------------------------------------------------------------------------------------------
struct SplitArgs {
    const void* in;
    void* out[SI_SPLIT_MAX];
    int begin[SI_SPLIT_MAX];     // first item of destination k among a pixel's items; INT_MAX for k >= the launch's count
    unsigned off[SI_SPLIT_MAX];  // its first input channel
    unsigned ld[SI_SPLIT_MAX];
    unsigned in_ld;
    unsigned per_pixel;          // items of one pixel: sum of the widths / V
    unsigned total;              // pixels * per_pixel (< 2^31)
};

template <typename T, int V>
__device__ __forceinline__ void split_body(const SplitArgs& a) {
    typedef typename SlWord<T, V>::type W;
    const T* const in = static_cast<const T*>(a.in);
    const size_t stride = (size_t)gridDim.x * SL_THREADS;
    for (size_t it = (size_t)blockIdx.x * SL_THREADS + threadIdx.x; it < a.total; it += stride) {
        const unsigned i = (unsigned)it;
        const unsigned p = i / a.per_pixel;
        const int j = (int)(i - p * a.per_pixel);
        T* dst = static_cast<T*>(a.out[0]);
        unsigned ld = a.ld[0], off = a.off[0];
        int b = 0;
#pragma unroll
        for (int k = 1; k < SI_SPLIT_MAX; ++k) {
            const bool ge = j >= a.begin[k];
            dst = ge ? static_cast<T*>(a.out[k]) : dst;
            ld = ge ? a.ld[k] : ld;
            off = ge ? a.off[k] : off;
            b = ge ? a.begin[k] : b;
        }
        const unsigned c = (unsigned)(j - b) * V;
        *reinterpret_cast<W*>(dst + p * ld + c) = *reinterpret_cast<const W*>(in + p * a.in_ld + off + c);
    }
}

template <typename T, int V>
__global__ __launch_bounds__(SL_THREADS) void split_vec(SplitArgs a) { split_body<T, V>(a); }

template <typename T>
__global__ __launch_bounds__(SL_THREADS) void split_elem(SplitArgs a) { split_body<T, 1>(a); }

// ---- host -----------------------------------------------------------------------------------------------------------------

// everything that can be decided without a device: SI_E_BADARG / SI_E_UNSUPPORTED / 0
int check_slice(const SiSliceDesc* d) {
    if (!d) return SI_E_BADARG;
    if (d->n <= 0 || d->ih <= 0 || d->iw <= 0 || d->ic <= 0 || d->on <= 0 || d->oh <= 0 || d->ow <= 0 || d->oc <= 0) return SI_E_BADARG;
    if (d->in_ld < d->ic || d->out_ld < d->oc) return SI_E_BADARG;
    const int in_dims[4] = {d->n, d->ih, d->iw, d->ic}, out_dims[4] = {d->on, d->oh, d->ow, d->oc};
    for (int a = 0; a < 4; ++a) {
        if (d->step[a] < 1 || d->start[a] < 0) return SI_E_BADARG;
        if ((int64_t)d->start[a] + (int64_t)(out_dims[a] - 1) * d->step[a] >= (int64_t)in_dims[a]) return SI_E_BADARG;
    }
    if (d->n > 65535) return SI_E_UNSUPPORTED;
    const uint64_t in_rows = (uint64_t)d->n * d->ih, out_rows = (uint64_t)d->on * d->oh;   // < 2^47
    if (in_rows > SI_INDEX_LIMIT || out_rows > SI_INDEX_LIMIT) return SI_E_UNSUPPORTED;
    const uint64_t in_pix = in_rows * d->iw, out_pix = out_rows * d->ow;                    // < 2^62
    if (in_pix > SI_INDEX_LIMIT || out_pix > SI_INDEX_LIMIT) return SI_E_UNSUPPORTED;
    if (in_pix * (uint64_t)d->in_ld > SI_INDEX_LIMIT || out_pix * (uint64_t)d->out_ld > SI_INDEX_LIMIT) return SI_E_UNSUPPORTED;
    return 0;
}

// 16-byte channel vectors when the channel step, the channel start, the width, both strides and both pointers allow it
template <typename T>
bool slice_is_vec(const SiSliceDesc* d, const void* src, const void* dst) {
    constexpr int V = (int)(16 / sizeof(T));
    return d->step[3] == 1 && d->start[3] % V == 0 && d->oc % V == 0 && d->in_ld % V == 0 && d->out_ld % V == 0 && si_aligned_to(src, 16) &&
           si_aligned_to(dst, 16);
}

template <typename T>
int run_slice(const SiSliceDesc* d, const void* src, void* dst, si_stream_t stream) {
    const int rc = check_slice(d);
    if (rc != 0) return rc;
    if (!src || !dst) return SI_E_BADARG;
    constexpr int V = (int)(16 / sizeof(T));
    const bool vec = slice_is_vec<T>(d, src, dst);
    SliceArgs a;
    a.in = src;
    a.out = dst;
    a.ih = d->ih; a.iw = d->iw; a.in_ld = d->in_ld;
    a.oh = d->oh; a.ow = d->ow; a.out_ld = d->out_ld;
    a.per_pixel = vec ? d->oc / V : d->oc;
    a.n0 = d->start[0]; a.h0 = d->start[1]; a.w0 = d->start[2]; a.c0 = d->start[3];
    a.sn = d->step[0]; a.sh = d->step[1]; a.sw = d->step[2]; a.sc = d->step[3];
    const size_t total = (size_t)d->on * d->oh * d->ow * a.per_pixel;   // <= out_pix * out_ld: fits 31 bits
    a.total = (unsigned)total;
    const dim3 grid(si_grid_for(total, SL_THREADS));
    if (vec) hipLaunchKernelGGL((slice_vec<T, V>), grid, dim3(SL_THREADS), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL((slice_elem<T>), grid, dim3(SL_THREADS), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int check_split(const void* src, size_t pixels, int c, int in_ld, int k, const int* offsets, const int* widths, void* const* dsts,
                const int* out_lds) {
    if (!src || !offsets || !widths || !dsts || !out_lds) return SI_E_BADARG;
    if (pixels == 0 || c <= 0 || in_ld < c || k < 1) return SI_E_BADARG;
    for (int i = 0; i < k; ++i) {
        if (!dsts[i] || widths[i] < 1 || offsets[i] < 0 || (int64_t)offsets[i] + widths[i] > (int64_t)c || out_lds[i] < widths[i]) return SI_E_BADARG;
    }
    if (pixels > SI_INDEX_LIMIT || (uint64_t)pixels * (uint64_t)in_ld > SI_INDEX_LIMIT) return SI_E_UNSUPPORTED;
    for (int i0 = 0; i0 < k; i0 += SI_SPLIT_MAX) {
        uint64_t per_pixel = 0;
        for (int i = i0; i < k && i < i0 + SI_SPLIT_MAX; ++i) {
            if ((uint64_t)pixels * (uint64_t)out_lds[i] > SI_INDEX_LIMIT) return SI_E_UNSUPPORTED;
            per_pixel += (uint64_t)widths[i];
        }
        if ((uint64_t)pixels * per_pixel > SI_INDEX_LIMIT) return SI_E_UNSUPPORTED;   // one launch's items
    }
    return 0;
}

// one rule over ALL destinations: a split is either all vectors or all elements
template <typename T>
bool split_is_vec(const void* src, int in_ld, int k, const int* offsets, const int* widths, void* const* dsts, const int* out_lds) {
    constexpr int V = (int)(16 / sizeof(T));
    if (in_ld % V != 0 || !si_aligned_to(src, 16)) return false;
    for (int i = 0; i < k; ++i)
        if (offsets[i] % V != 0 || widths[i] % V != 0 || out_lds[i] % V != 0 || !si_aligned_to(dsts[i], 16)) return false;
    return true;
}

template <typename T>
int run_split(const void* src, size_t pixels, int c, int in_ld, int k, const int* offsets, const int* widths, void* const* dsts,
              const int* out_lds, si_stream_t stream) {
    const int rc = check_split(src, pixels, c, in_ld, k, offsets, widths, dsts, out_lds);
    if (rc != 0) return rc;
    constexpr int V = (int)(16 / sizeof(T));
    const bool vec = split_is_vec<T>(src, in_ld, k, offsets, widths, dsts, out_lds);
    const int v = vec ? V : 1;
    for (int i0 = 0; i0 < k; i0 += SI_SPLIT_MAX) {
        const int cnt = k - i0 < SI_SPLIT_MAX ? k - i0 : SI_SPLIT_MAX;
        SplitArgs a;
        a.in = src;
        a.in_ld = in_ld;
        int items = 0;
        for (int j = 0; j < SI_SPLIT_MAX; ++j) {
            const int i = i0 + (j < cnt ? j : 0);   // (the slots behind the last destination repeat the first one and are never selected)
            a.out[j] = dsts[i];
            a.off[j] = offsets[i];
            a.ld[j] = out_lds[i];
            a.begin[j] = j < cnt ? items : INT_MAX;
            if (j < cnt) items += widths[i] / v;
        }
        a.per_pixel = items;
        const size_t total = pixels * (size_t)items;
        a.total = (unsigned)total;
        const dim3 grid(si_grid_for(total, SL_THREADS));
        if (vec) hipLaunchKernelGGL((split_vec<T, V>), grid, dim3(SL_THREADS), 0, (hipStream_t)stream, a);
        else hipLaunchKernelGGL((split_elem<T>), grid, dim3(SL_THREADS), 0, (hipStream_t)stream, a);
        const int e = (int)hipGetLastError();
        if (e != 0) return e;
    }
    return 0;
}

}  // namespace

extern "C" {

int si_hip_slice_f32(const SiSliceDesc* d, const void* src, void* dst, si_stream_t stream) { return run_slice<float>(d, src, dst, stream); }

int si_hip_slice_f16(const SiSliceDesc* d, const void* src, void* dst, si_stream_t stream) { return run_slice<_Float16>(d, src, dst, stream); }

const char* si_hip_slice_kernel_name(const SiSliceDesc* d, const void* src, const void* dst, int half) {
    if (check_slice(d) != 0) return "none";
    if (half) return slice_is_vec<_Float16>(d, src, dst) ? "slice_vec<_Float16, 8>" : "slice_elem<_Float16>";
    return slice_is_vec<float>(d, src, dst) ? "slice_vec<float, 4>" : "slice_elem<float>";
}

int si_hip_split_channels_f32(const void* src, size_t pixels, int c, int in_ld, int k, const int* offsets, const int* widths,
                              void* const* dsts, const int* out_lds, si_stream_t stream) {
    return run_split<float>(src, pixels, c, in_ld, k, offsets, widths, dsts, out_lds, stream);
}

int si_hip_split_channels_f16(const void* src, size_t pixels, int c, int in_ld, int k, const int* offsets, const int* widths,
                              void* const* dsts, const int* out_lds, si_stream_t stream) {
    return run_split<_Float16>(src, pixels, c, in_ld, k, offsets, widths, dsts, out_lds, stream);
}

const char* si_hip_split_channels_kernel_name(const void* src, size_t pixels, int c, int in_ld, int k, const int* offsets,
                                              const int* widths, void* const* dsts, const int* out_lds, int half) {
    if (check_split(src, pixels, c, in_ld, k, offsets, widths, dsts, out_lds) != 0) return "none";
    if (half) return split_is_vec<_Float16>(src, in_ld, k, offsets, widths, dsts, out_lds) ? "split_vec<_Float16, 8>" : "split_elem<_Float16>";
    return split_is_vec<float>(src, in_ld, k, offsets, widths, dsts, out_lds) ? "split_vec<float, 4>" : "split_elem<float>";
}

}  // extern "C"
