// binary_const.hip -- arithmetic of an activation against one or two graph constants (include/si_binary.h):
// out = stage1(stage0(x, c0), c1) on fp32 and fp16 views with pixel strides on both sides.  HBM-bound: x is read once and out written once
// whatever the number of stages; the constants are small next to x and come from the caches.
//
// Work item: one lane-wide piece (16 bytes of x, or one element in the scalar arm) of one run d[3].  Consecutive lanes take consecutive
// pieces of a run, then consecutive pixels: a wave reads and writes whole stretches of rows.
//   chan   a lane's place in the run never changes: the grid's working lanes are a multiple of the pieces per run, so a lane loads its piece
//          of the constants ONCE into registers (at most 2 x 8 values, statically indexed: no scratch, no LDS -- the run is not shared
//          between lanes in any way a wave could exploit, consecutive lanes already read consecutive addresses of it) and then only walks
//          over pixels: no index arithmetic in the loop beyond one add.
//   pixel  item -> (pixel, piece) and pixel -> (i0, i1, i2) by magic division (si_magic.h); one scalar of each constant per item.
//   full   the same decomposition; the constant's piece is one 16-byte load where its strides and pointer allow, single elements otherwise.
// Element offsets are 32-bit: the host (binary_plan.h) refuses operands whose offsets do not fit 31 bits.
//
// No contraction: a two-stage x * scale + shift must round as the two launches it replaces.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include <cstdint>

#include "binary_plan.h"
#include "si_binary.h"
#include "si_hip_internal.h"

namespace {

using si_binary_plan::kChan;
using si_binary_plan::kFull;
using si_binary_plan::kPixel;
using si_binary_plan::kThreads;
using si_binary_plan::Plan;

struct BcArgs {
    const void* x;
    void* out;
    const void* c[2];
    int op[2];
    int stages;
    int cs[2][4];        // constant strides
    int cvec[2];         // full form: vector reads of this constant
    int cv;              // pieces per run
    int d1, d2;
    unsigned m_cv, m_d1, m_d2;
    int x_ld, out_ld;
    unsigned pixels, items;
    unsigned lanes, pixel_step;   // chan form
};

// a stage's result as the storage type holds it: fp16 rounds here, once per stage
template <typename T>
__device__ __forceinline__ float bc_round(float v) {
    if constexpr (sizeof(T) == 2) return (float)si_store_cast<T>(v);
    else return v;
}

// (the stores below are si_store_vec<T, VW, /*exact=*/true>: bc_round already rounded every stage to T, so a plain cast stores it)

// One stage on a lane's piece.  The formulas are those of ops.hip's binary_apply: IEEE division, the library's powf / atan2f.  The code is
// chosen once per piece, not per element: it is uniform over the launch, and a switch inside the element loop costs a chain of scalar
// branches for every element (8 halves x 2 stages per piece).
template <typename T, int VW>
__device__ __forceinline__ void bc_stage(int op, float (&v)[VW], const float (&c)[VW]) {
#define BC_EACH(expr)                           \
    _Pragma("unroll") for (int j = 0; j < VW; ++j) { \
        const float x = v[j], y = c[j];         \
        v[j] = bc_round<T>(expr);               \
    }                                           \
    break
    switch (op) {
        case 0: BC_EACH(x + y);
        case 1: BC_EACH(x - y);
        case 2: BC_EACH(x * y);
        case 3: BC_EACH(x / y);
        case 6: BC_EACH(powf(x, y));
        case 7: BC_EACH(y - x);
        case 8: BC_EACH(y / x);
        case 9: BC_EACH(powf(y, x));
        case 10: BC_EACH(atan2f(x, y));
        case 11: BC_EACH(atan2f(y, x));
        default: break;
    }
#undef BC_EACH
}

template <typename T, int VW, int FORM>
__global__ __launch_bounds__(kThreads) void binary_const_kernel(BcArgs a) {
    const T* const x = static_cast<const T*>(a.x);
    T* const out = static_cast<T*>(a.out);
    const T* const c0 = static_cast<const T*>(a.c[0]);
    const T* const c1 = static_cast<const T*>(a.c[1]);   // null with one stage: never dereferenced
    const bool two = a.stages == 2;
    const unsigned g = blockIdx.x * (unsigned)kThreads + threadIdx.x;
    if constexpr (FORM == kChan) {
        if (g >= a.lanes) return;
        int piece;
        const int p0 = si_fast_divmod((int)g, a.cv, a.m_cv, piece);
        const int e0 = piece * VW;   // first element of this lane's piece
        float k0[VW], k1[VW];
        if (VW > 1 && a.cvec[0]) {
            si_load_vec<T, VW>(c0 + e0, k0);
        } else {
#pragma unroll
            for (int j = 0; j < VW; ++j) k0[j] = (float)c0[(e0 + j) * a.cs[0][3]];
        }
        if (two && VW > 1 && a.cvec[1]) {
            si_load_vec<T, VW>(c1 + e0, k1);
        } else {
#pragma unroll
            for (int j = 0; j < VW; ++j) k1[j] = two ? (float)c1[(e0 + j) * a.cs[1][3]] : 0.0f;
        }
        for (unsigned p = (unsigned)p0; p < a.pixels; p += a.pixel_step) {
            float v[VW];
            si_load_vec<T, VW>(x + p * (unsigned)a.x_ld + e0, v);
            bc_stage<T, VW>(a.op[0], v, k0);
            if (two) bc_stage<T, VW>(a.op[1], v, k1);
            si_store_vec<T, VW, /*exact=*/true>(out + p * (unsigned)a.out_ld + e0, v);
        }
    } else {
        const unsigned step = gridDim.x * (unsigned)kThreads;
        for (unsigned i = g; i < a.items; i += step) {
            int piece, i1, i2;
            const int p = si_fast_divmod((int)i, a.cv, a.m_cv, piece);
            const int e0 = piece * VW;
            const int t = si_fast_divmod(p, a.d2, a.m_d2, i2);
            const int i0 = si_fast_divmod(t, a.d1, a.m_d1, i1);
            float v[VW];
            si_load_vec<T, VW>(x + (unsigned)p * (unsigned)a.x_ld + e0, v);
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                if (s == 1 && !two) break;
                const T* const c = (s == 0 ? c0 : c1) + (i0 * a.cs[s][0] + i1 * a.cs[s][1] + i2 * a.cs[s][2]);
                float k[VW];
                if constexpr (FORM == kPixel) {
                    const float ks = (float)c[0];
#pragma unroll
                    for (int j = 0; j < VW; ++j) k[j] = ks;
                } else {
                    if (VW > 1 && a.cvec[s]) {
                        si_load_vec<T, VW>(c + e0, k);
                    } else {
#pragma unroll
                        for (int j = 0; j < VW; ++j) k[j] = (float)c[(e0 + j) * a.cs[s][3]];
                    }
                }
                bc_stage<T, VW>(a.op[s], v, k);
            }
            si_store_vec<T, VW, /*exact=*/true>(out + (unsigned)p * (unsigned)a.out_ld + e0, v);
        }
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------
template <typename T, int VW, int FORM>
int launch(const BcArgs& a, unsigned blocks, hipStream_t stream) {
    hipLaunchKernelGGL((binary_const_kernel<T, VW, FORM>), dim3(blocks), dim3(kThreads), 0, stream, a);
    return (int)hipGetLastError();
}

template <typename T, int VW>
int launch_form(const BcArgs& a, const Plan& p, hipStream_t stream) {
    switch (p.form) {
        case kChan: return launch<T, VW, kChan>(a, p.blocks, stream);
        case kPixel: return launch<T, VW, kPixel>(a, p.blocks, stream);
        default: return launch<T, VW, kFull>(a, p.blocks, stream);
    }
}

template <typename T>
int run(const SiBinaryDesc* d, const T* x, const T* c0, const T* c1, T* out, si_stream_t stream) {
    Plan p;
    const int rc = si_binary_plan::MakePlan(d, x, c0, c1, out, (int)sizeof(T), p);
    if (rc != 0) return rc;
    BcArgs a;
    a.x = x;
    a.out = out;
    a.c[0] = c0;
    a.c[1] = d->stages == 2 ? c1 : nullptr;
    a.stages = d->stages;
    for (int s = 0; s < 2; ++s) {
        a.op[s] = s < d->stages ? d->op[s] : 0;
        a.cvec[s] = s < d->stages ? p.cvec[s] : 0;
        for (int i = 0; i < 4; ++i) a.cs[s][i] = s < d->stages ? si_binary_plan::Strides(d, s)[i] : 0;
    }
    a.cv = p.cv;
    a.d1 = d->d[1];
    a.d2 = d->d[2];
    a.m_cv = si_magic(p.cv);
    a.m_d1 = si_magic(d->d[1]);
    a.m_d2 = si_magic(d->d[2]);
    a.x_ld = d->x_ld;
    a.out_ld = d->out_ld;
    a.pixels = p.pixels;
    a.items = p.items;
    a.lanes = p.lanes;
    a.pixel_step = p.pixel_step;
    hipStream_t s = (hipStream_t)stream;
    constexpr int full = (int)(16 / sizeof(T));
    return p.vw == full ? launch_form<T, full>(a, p, s) : launch_form<T, 1>(a, p, s);
}

}  // namespace

extern "C" {

int si_hip_binary_const_f32(const SiBinaryDesc* d, const float* x, const float* c0, const float* c1, float* out, si_stream_t stream) {
    return run<float>(d, x, c0, c1, out, stream);
}

int si_hip_binary_const_f16(const SiBinaryDesc* d, const void* x, const void* c0, const void* c1, void* out, si_stream_t stream) {
    return run<_Float16>(d, static_cast<const _Float16*>(x), static_cast<const _Float16*>(c0), static_cast<const _Float16*>(c1),
                         static_cast<_Float16*>(out), stream);
}

const char* si_hip_binary_const_kernel_name(const SiBinaryDesc* d, const void* x, const void* c0, const void* c1, const void* out, int half) {
    Plan p;
    if (si_binary_plan::MakePlan(d, x, c0, c1, out, half ? 2 : 4, p) != 0) return "none";
    static const char* const names[2][2][3] = {
        {{"binary_const_kernel<float, 1, chan>", "binary_const_kernel<float, 1, pixel>", "binary_const_kernel<float, 1, full>"},
         {"binary_const_kernel<float, 4, chan>", "binary_const_kernel<float, 4, pixel>", "binary_const_kernel<float, 4, full>"}},
        {{"binary_const_kernel<_Float16, 1, chan>", "binary_const_kernel<_Float16, 1, pixel>", "binary_const_kernel<_Float16, 1, full>"},
         {"binary_const_kernel<_Float16, 8, chan>", "binary_const_kernel<_Float16, 8, pixel>", "binary_const_kernel<_Float16, 8, full>"}}};
    return names[half ? 1 : 0][p.vw > 1 ? 1 : 0][p.form];
}

}  // extern "C"
