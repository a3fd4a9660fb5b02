// prelu.hip -- nn.PReLU (include/si_superres.h): y = x > 0 ? x : slope[ch] * x on [pixels, c] fp32 and fp16 tensors with pixel strides on
// both sides; the slopes are an fp32 vector of 1 or c elements.  torch's CPU formula: -0.0 and NaN take the multiply.  fp32
// arithmetic; a half result is rounded once, at the store.
//
// One item is one channel vector of one pixel (16 bytes, or one element in the scalar form); consecutive lanes take consecutive
// vectors of a pixel, then consecutive pixels; the grid is capped and strides over the rest.  Item indices and element offsets
// are 32-bit: the host refuses tensors whose offsets do not fit 31 bits.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "si_hip_internal.h"
#include "si_superres.h"

namespace {

constexpr int PRELU_THREADS = 256;

template <typename T, int VW>
__global__ __launch_bounds__(PRELU_THREADS) void prelu_kernel(const T* in, unsigned items, int cv, int in_ld, const float* __restrict__ slope,
                                                              int per_channel, T* out, int out_ld) {
    typedef si_vec<T, VW> Vec;
    const float shared = slope[0];
    for (unsigned item = blockIdx.x * PRELU_THREADS + threadIdx.x; item < items; item += gridDim.x * PRELU_THREADS) {   // (items < 2^31)
        const int pix = (int)(item / (unsigned)cv), v = (int)item - pix * cv;
        if constexpr (VW == 1) {
            const float x = (float)in[pix * in_ld + v];
            const float s = per_channel ? slope[v] : shared;
            out[pix * out_ld + v] = si_store_cast<T>(x > 0.0f ? x : s * x);
        } else {
            const Vec x = *reinterpret_cast<const Vec*>(in + pix * in_ld + v * VW);
            Vec y;
#pragma unroll
            for (int t = 0; t < VW; ++t) {
                const float xf = (float)x[t];
                const float s = per_channel ? slope[v * VW + t] : shared;
                y[t] = si_store_cast<T>(xf > 0.0f ? xf : s * xf);
            }
            *reinterpret_cast<Vec*>(out + pix * out_ld + v * VW) = y;
        }
    }
}

// SI_E_BADARG / SI_E_UNSUPPORTED / 0, without a device
int check_args(const void* in, size_t pixels, int c, int in_ld, int slope_count, const void* out, int out_ld) {
    if (!in || !out || pixels == 0 || c <= 0 || in_ld < c || out_ld < c) return SI_E_BADARG;
    if (slope_count != 1 && slope_count != c) return SI_E_BADARG;
    if (pixels > SI_INDEX_LIMIT || pixels * (uint64_t)in_ld > SI_INDEX_LIMIT || pixels * (uint64_t)out_ld > SI_INDEX_LIMIT) return SI_E_UNSUPPORTED;
    return 0;
}

template <typename T>
int run(const T* in, size_t pixels, int c, int in_ld, const float* slope, int slope_count, T* out, int out_ld, si_stream_t stream) {
    const int rc = check_args(in, pixels, c, in_ld, slope_count, out, out_ld);
    if (rc != 0) return rc;
    if (!slope) return SI_E_BADARG;
    constexpr int full = (int)(16 / sizeof(T));
    hipStream_t s = (hipStream_t)stream;
    const int per_channel = slope_count == c && c > 1 ? 1 : 0;
    if (si_vector_width<T>(c, in_ld, out_ld, in, out) == full) {
        const int cv = c / full;
        const unsigned items = (unsigned)pixels * (unsigned)cv;
        hipLaunchKernelGGL((prelu_kernel<T, full>), dim3(si_grid_for((size_t)items)), dim3(PRELU_THREADS), 0, s, in, items, cv, in_ld, slope,
                           per_channel, out, out_ld);
    } else {
        const unsigned items = (unsigned)pixels * (unsigned)c;
        hipLaunchKernelGGL((prelu_kernel<T, 1>), dim3(si_grid_for((size_t)items)), dim3(PRELU_THREADS), 0, s, in, items, c, in_ld, slope,
                           per_channel, out, out_ld);
    }
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int si_hip_prelu_f32(const float* in, size_t pixels, int c, int in_ld, const float* slope, int slope_count, float* out, int out_ld,
                     si_stream_t stream) {
    return run<float>(in, pixels, c, in_ld, slope, slope_count, out, out_ld, stream);
}

int si_hip_prelu_f16(const void* in, size_t pixels, int c, int in_ld, const float* slope, int slope_count, void* out, int out_ld,
                     si_stream_t stream) {
    return run<_Float16>(static_cast<const _Float16*>(in), pixels, c, in_ld, slope, slope_count, static_cast<_Float16*>(out), out_ld, stream);
}

const char* si_hip_prelu_kernel_name(const void* in, size_t pixels, int c, int in_ld, int slope_count, const void* out, int out_ld, int half) {
    if (check_args(in, pixels, c, in_ld, slope_count, out, out_ld) != 0) return "none";
    if (half) return si_vector_width<_Float16>(c, in_ld, out_ld, in, out) > 1 ? "prelu_kernel<_Float16, 8>" : "prelu_kernel<_Float16, 1>";
    return si_vector_width<float>(c, in_ld, out_ld, in, out) > 1 ? "prelu_kernel<float, 4>" : "prelu_kernel<float, 1>";
}

}  // extern "C"
