// activation_param.hip -- clamp / softplus / mish (include/si_act.h) on fp32 and fp16 [pixels, c] tensors with pixel strides on both sides.
// Arithmetic, special values, the arms and the refusals: the header.  The model is activation_kernel of ops.hip: one lane per
// 16-byte channel vector (or single element), consecutive lanes on consecutive addresses, a grid-stride loop under si_grid_for.  What
// differs: the operator is a template parameter, so a lane runs straight-line code of one operator, and the two parameters are kernel
// arguments.  Element offsets are 32-bit: the host refuses tensors whose offsets do not fit 31 bits, and an item index plus one grid
// (2048 x 256) stays below 2^32.  No LDS, no scratch.  Register table per instantiation: DESIGN.md 9j.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "si_act.h"
#include "si_hip_internal.h"

#pragma clang fp contract(off)

namespace {

constexpr int PA_THREADS = 256;

// log1p(e) for 0 <= e <= 1 (a NaN comes out).  u = 1 + e rounds; d = (u - 1) - e is that rounding error, exactly (u - 1 is exact for
// 1 <= u <= 2, and so is the difference of two values that close), and log(1 + e) = log(u - d) = log(u) - d / u up to (d / u)^2 < 2^-48.
// Where e is below half an ulp of 1, u is 1 and the result is e itself.  The quotient is a correction of at most 2^-24, so the
// reciprocal instruction serves it.  The library's log1pf is a double-float evaluation of about 115 instructions; this is about 20.
__device__ __forceinline__ float pa_log1p_unit(float e) {
    const float u = 1.0f + e;
    const float d = (u - 1.0f) - e;
    return logf(u) - d * __builtin_amdgcn_rcpf(u);
}

template <int OP>
__device__ __forceinline__ float pa_apply(float x, float p0, float p1) {
    if constexpr (OP == SI_PACT_CLAMP) {
        const float y = x < p0 ? p0 : x;
        return y > p1 ? p1 : y;
    } else if constexpr (OP == SI_PACT_SOFTPLUS) {
        const float z = p0 * x;
        if (z > p1) return x;
        // max(z, 0) + log1p(exp(-|z|)): a NaN leaves the first term 0 and comes out of the second
        return ((z > 0.0f ? z : 0.0f) + pa_log1p_unit(expf(-fabsf(z)))) / p0;
    } else {
        if (x > (float)SI_PACT_MISH_CUT) return x;
        const float e = expf(x);            // (a NaN fails the test above and comes out of the product below)
        const float n = e * (e + 2.0f);
        return x * (n / (n + 2.0f));
    }
}

// items = pixels * cv, cv = items (vectors of VW elements, or elements) per pixel; in_ld / out_ld in elements
template <int OP, typename T, int VW>
__global__ __launch_bounds__(PA_THREADS) void param_act_kernel(float p0, float p1, const T* __restrict__ in, unsigned items, unsigned cv,
                                                                unsigned in_ld, T* __restrict__ out, unsigned out_ld) {
    const unsigned step = gridDim.x * PA_THREADS;
    for (unsigned i = blockIdx.x * PA_THREADS + threadIdx.x; i < items; i += step) {
        const unsigned p = i / cv;
        const unsigned ch = (i - p * cv) * VW;
        float v[VW];
        si_load_vec<T, VW>(in + (p * in_ld + ch), v);
#pragma unroll
        for (int e = 0; e < VW; ++e) v[e] = pa_apply<OP>(v[e], p0, p1);
        si_store_vec<T, VW>(out + (p * out_ld + ch), v);
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------
// everything that can be decided without a device or a pointer: SI_E_BADARG / SI_E_UNSUPPORTED / 0
int check_desc(const SiParamActDesc* d) {
    if (!d) return SI_E_BADARG;
    if (d->pixels == 0 || d->c <= 0 || d->in_ld < d->c || d->out_ld < d->c) return SI_E_BADARG;
    switch (d->op) {
        case SI_PACT_CLAMP:
            if (std::isnan(d->p0) || std::isnan(d->p1)) return SI_E_BADARG;
            break;
        case SI_PACT_SOFTPLUS:
            if (!std::isfinite(d->p0) || d->p0 == 0.0f || std::isnan(d->p1)) return SI_E_BADARG;
            break;
        case SI_PACT_MISH: break;
        default: return SI_E_BADARG;
    }
    // offsets, and with them the item counts (at most one item per element, c <= ld)
    const uint64_t ld = (uint64_t)(d->in_ld > d->out_ld ? d->in_ld : d->out_ld);
    if ((uint64_t)d->pixels > SI_INDEX_LIMIT || (uint64_t)d->pixels * ld > SI_INDEX_LIMIT) return SI_E_UNSUPPORTED;
    return 0;
}

// do the two views share an element?  (the strided-window rule of si_views.h)
bool views_overlap(const SiParamActDesc* d, const void* in, const void* out, size_t esize) {
    return si_strided_windows_overlap(in, (uint64_t)d->pixels, (uint64_t)d->in_ld, (uint64_t)d->c, out, (uint64_t)d->pixels, (uint64_t)d->out_ld,
                                      (uint64_t)d->c, esize);
}

enum Arm { kDense, kVector, kElement };

template <typename T>
Arm arm_of(const SiParamActDesc* d, const void* in, const void* out) {
    const int full = (int)(16 / sizeof(T));
    if (!si_aligned_to(in, 16) || !si_aligned_to(out, 16)) return kElement;
    // a dense tensor is one long row: lets odd channel counts (e.g. 3) still take the 16-byte path
    if (d->in_ld == d->c && d->out_ld == d->c && (d->pixels * (size_t)d->c) % (size_t)full == 0) return kDense;
    return (d->c % full == 0 && d->in_ld % full == 0 && d->out_ld % full == 0) ? kVector : kElement;
}

template <int OP, typename T>
int launch(const SiParamActDesc* d, const T* in, T* out, hipStream_t s) {
    constexpr int full = (int)(16 / sizeof(T));
    const Arm arm = arm_of<T>(d, in, out);
    if (arm == kElement) {
        const unsigned items = (unsigned)(d->pixels * (size_t)d->c);
        hipLaunchKernelGGL((param_act_kernel<OP, T, 1>), dim3(si_grid_for(items, PA_THREADS)), dim3(PA_THREADS), 0, s, d->p0, d->p1, in, items,
                           (unsigned)d->c, (unsigned)d->in_ld, out, (unsigned)d->out_ld);
    } else {
        const unsigned items = (unsigned)(d->pixels * (size_t)d->c / full);
        // dense: one pixel of `items` vectors (the strides are never used); vector: c / full vectors per pixel
        const unsigned cv = arm == kDense ? items : (unsigned)(d->c / full);
        hipLaunchKernelGGL((param_act_kernel<OP, T, full>), dim3(si_grid_for(items, PA_THREADS)), dim3(PA_THREADS), 0, s, d->p0, d->p1, in, items, cv,
                           (unsigned)d->in_ld, out, (unsigned)d->out_ld);
    }
    return (int)hipGetLastError();
}

template <typename T>
int run(const SiParamActDesc* d, const T* in, T* out, si_stream_t stream) {
    const int rc = check_desc(d);
    if (rc != 0) return rc;
    if (!in || !out) return SI_E_BADARG;
    if (views_overlap(d, in, out, sizeof(T))) return SI_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    switch (d->op) {
        case SI_PACT_CLAMP: return launch<SI_PACT_CLAMP, T>(d, in, out, s);
        case SI_PACT_SOFTPLUS: return launch<SI_PACT_SOFTPLUS, T>(d, in, out, s);
        default: return launch<SI_PACT_MISH, T>(d, in, out, s);
    }
}

}  // namespace

extern "C" {

int si_hip_param_act_f32(const SiParamActDesc* d, const float* in, float* out, si_stream_t stream) { return run<float>(d, in, out, stream); }

int si_hip_param_act_f16(const SiParamActDesc* d, const void* in, void* out, si_stream_t stream) {
    return run<_Float16>(d, static_cast<const _Float16*>(in), static_cast<_Float16*>(out), stream);
}

const char* si_hip_param_act_kernel_name(const SiParamActDesc* d, const void* in, const void* out, int half) {
    if (check_desc(d) != 0) return "none";
    static const char* const names[3][4] = {
        {"param_act_kernel<clamp, float, 4>", "param_act_kernel<clamp, float, 1>", "param_act_kernel<clamp, _Float16, 8>",
         "param_act_kernel<clamp, _Float16, 1>"},
        {"param_act_kernel<softplus, float, 4>", "param_act_kernel<softplus, float, 1>", "param_act_kernel<softplus, _Float16, 8>",
         "param_act_kernel<softplus, _Float16, 1>"},
        {"param_act_kernel<mish, float, 4>", "param_act_kernel<mish, float, 1>", "param_act_kernel<mish, _Float16, 8>",
         "param_act_kernel<mish, _Float16, 1>"},
    };
    const bool vec = (half ? arm_of<_Float16>(d, in, out) : arm_of<float>(d, in, out)) != kElement;
    return names[d->op][(half ? 2 : 0) + (vec ? 0 : 1)];
}

}  // extern "C"
