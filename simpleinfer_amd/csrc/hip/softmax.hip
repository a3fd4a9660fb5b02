// softmax.hip -- softmax / log_softmax along one axis (include/si_softmax.h) on NHWC fp32 and fp16 tensors with pixel strides on both
// sides.  Arithmetic, special values and the refusals: the header.  This is the project's max / exponential-sum reduction.
//
// Contiguous axis (axis 3), a ROW = the c channels of one pixel, seen as cv items (16-byte vectors, or single elements):
//   group         L = 2^k <= 64 lanes per row (L = the power of two at or above cv / 4 -- cv / 2 for half vectors --, so a lane has up to
//                 four items of a short row), 256 / L rows per workgroup.  Lane j keeps items j, j + L, ... (at most 16 floats) in registers.  The maximum and the
//                 sum are butterflies over the xor offsets below L: lanes of other rows never enter.
//   block         one workgroup per row, thread t keeps items t, t + 256, ... (at most 16 floats).  Butterflies per wave, then the four
//                 wave values from LDS, combined in index order by every thread.
//   block_online  one workgroup per row; thread t runs (m, s) <- (max(m, x), s exp(m - m') + exp(x - m')) over items t, t + 256, ...;
//                 the row's maximum M as above, every s is rescaled by exp(m - M) and the sum taken as above; the row is read again.
// Strided axis (0, 1, 2): the tensor is [outer][A][inner pixels][c]; an ITEM = (outer, inner pixel, channel vector), one lane each,
// consecutive lanes take consecutive channel vectors and then consecutive inner pixels: a wave reads whole runs of pixels at every
// position of the axis.  Every channel of the vector is a reduction of its own, serial in the lane: nothing crosses lanes.
//   strided         A <= SI_SOFTMAX_STRIDED_REG_A: the A vectors stay in registers.
//   strided_online  the recurrence above per channel, then a second walk.
//
// A recurrence whose running maximum is still -inf adds nothing (exp of -inf - -inf would be NaN): such a row, or share of a row,
// carries s = 0 until a finite element arrives; a row of only -inf ends as NaN through x - m at the store, as torch's does.
// fmaxf skips NaNs: a NaN reaches the row through exp(NaN - m) in the sum.
//
// Element offsets are 32-bit: the host refuses tensors whose offsets do not fit 31 bits.  Register table per instantiation: DESIGN.md 9f.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "si_hip_internal.h"
#include "si_softmax.h"

#pragma clang fp contract(off)

namespace {

constexpr int SM_THREADS = 256;
constexpr int SM_WAVES = SM_THREADS / 64;
constexpr int SM_LANE_ELEMS = SI_ROW_LANE_ELEMS;   // floats of a row that a lane of the group / block forms keeps
constexpr int SM_GROUP_ITEMS = 4;   // items per lane that size a group

static_assert(SI_SOFTMAX_GROUP_MAX_C == 64 * SM_LANE_ELEMS && SI_SOFTMAX_BLOCK_MAX_C == SM_THREADS * SM_LANE_ELEMS, "thresholds follow the register tile");

struct SmArgs {
    const void* in;
    void* out;
    int rows;          // axis 3: pixels
    int cv;            // items (channel vectors) per pixel
    int in_ld, out_ld;
    int log;
    int lg;            // group form: log2 of the lanes per row
    int A, inner;      // strided forms: positions of the axis; pixels between two positions (and per outer index)
    int items;         // strided forms: outer * inner * cv
};

// the reference point of a recurrence: its maximum, or 0 while that is still -inf
__device__ __forceinline__ float sm_ref(float m) { return m == -INFINITY ? 0.0f : m; }

// the result from d = x - m (log) or e = exp(x - m): `k` is log(s) or 1 / s
__device__ __forceinline__ float sm_finish(int log, float v, float k) { return log ? v - k : v * k; }
__device__ __forceinline__ float sm_row_const(int log, float s) { return log ? __logf(s) : __builtin_amdgcn_rcpf(s); }

// the maximum is SiMaxNum (fmaxf skips a NaN, on purpose: above), the sum SiSum; both are commutative, so every lane of a team and every
// thread of a workgroup ends with the same bits
template <bool BLOCK, typename Op>
__device__ __forceinline__ float sm_combine(float v, int lanes, float* part) {
    return BLOCK ? si_block<Op, SM_WAVES>(v, part) : si_team<Op>(v, lanes);
}

// the register-resident row: BLOCK = one workgroup per row, else a group of 1 << a.lg lanes per row
template <typename T, int VW, bool BLOCK>
__device__ __forceinline__ void sm_row_in_registers(const SmArgs& a) {
    using Tile = SiRowTile<T, VW, SM_THREADS, BLOCK>;
    __shared__ float part_m[SM_WAVES], part_s[SM_WAVES];
    const Tile tile(a.lg);
    typename Tile::Regs v;
    const int row = (int)blockIdx.x * tile.rows_per_block + tile.sub;
    const bool live = row < a.rows;
    const T* const in = static_cast<const T*>(a.in) + (live ? row : 0) * a.in_ld;
    const int log = a.log;
    float m = tile.load_row(v, in, live, a.cv, -INFINITY, [](float m, float x) { return SiMaxNum::apply(m, x); });
    m = sm_combine<BLOCK, SiMaxNum>(m, tile.L, part_m);
    float s = tile.update_row(v, live, a.cv, 0.0f, [=](float s, float& x) {
        const float d = x - m;
        const float ex = __expf(d);
        x = log ? d : ex;
        return s + ex;
    });
    s = sm_combine<BLOCK, SiSum>(s, tile.L, part_s);
    if (!live) return;
    const float k = sm_row_const(log, s);
    tile.store_row(v, static_cast<T*>(a.out) + row * a.out_ld, a.cv, [=](float x) { return sm_finish(log, x, k); });
}

template <typename T, int VW>
__global__ __launch_bounds__(SM_THREADS) void softmax_group_kernel(SmArgs a) { sm_row_in_registers<T, VW, false>(a); }

template <typename T, int VW>
__global__ __launch_bounds__(SM_THREADS) void softmax_block_kernel(SmArgs a) { sm_row_in_registers<T, VW, true>(a); }

template <typename T, int VW>
__global__ __launch_bounds__(SM_THREADS) void softmax_block_online_kernel(SmArgs a) {
    __shared__ float part_m[SM_WAVES], part_s[SM_WAVES];
    const int tid = (int)threadIdx.x;
    const int row = (int)blockIdx.x;
    const T* const in = static_cast<const T*>(a.in) + row * a.in_ld;
    float m = -INFINITY, s = 0.0f;
    for (int item = tid; item < a.cv; item += SM_THREADS) {
        float x[VW];
        si_load_vec<T, VW>(in + item * VW, x);
        float mn = m;
#pragma unroll
        for (int e = 0; e < VW; ++e) mn = fmaxf(mn, x[e]);
        const float ref = sm_ref(mn);
        s = s * __expf(m - ref);
#pragma unroll
        for (int e = 0; e < VW; ++e) s += __expf(x[e] - ref);
        m = mn;
    }
    const float M = si_block<SiMaxNum, SM_WAVES>(m, part_m);
    s = s * __expf(m - sm_ref(M));
    s = si_block<SiSum, SM_WAVES>(s, part_s);
    const float k = sm_row_const(a.log, s);
    T* const out = static_cast<T*>(a.out) + row * a.out_ld;
    for (int item = tid; item < a.cv; item += SM_THREADS) {
        float x[VW];
        si_load_vec<T, VW>(in + item * VW, x);
#pragma unroll
        for (int e = 0; e < VW; ++e) {
            const float d = x[e] - M;
            x[e] = sm_finish(a.log, a.log ? d : __expf(d), k);
        }
        si_store_vec<T, VW>(out + item * VW, x);
    }
}

// one lane per item; the axis has a.A positions, a.inner pixels apart
template <typename T, int VW, bool ONLINE>
__device__ __forceinline__ void sm_strided(const SmArgs& a) {
    const int item = (int)blockIdx.x * SM_THREADS + (int)threadIdx.x;
    if (item >= a.items) return;
    const int pix = item / a.cv;
    const int cvec = item - pix * a.cv;
    const int o = pix / a.inner;
    const int first = o * a.A * a.inner + (pix - o * a.inner);   // the pixel at position 0
    const T* const in = static_cast<const T*>(a.in) + first * a.in_ld + cvec * VW;
    T* const out = static_cast<T*>(a.out) + first * a.out_ld + cvec * VW;
    const int in_step = a.inner * a.in_ld, out_step = a.inner * a.out_ld;
    float m[VW], s[VW];
#pragma unroll
    for (int e = 0; e < VW; ++e) {
        m[e] = -INFINITY;
        s[e] = 0.0f;
    }
    if constexpr (!ONLINE) {
        constexpr int RA = SI_SOFTMAX_STRIDED_REG_A;
        float v[RA][VW];
#pragma unroll
        for (int p = 0; p < RA; ++p) {
            if (p < a.A) {
                si_load_vec<T, VW>(in + p * in_step, v[p]);
#pragma unroll
                for (int e = 0; e < VW; ++e) m[e] = fmaxf(m[e], v[p][e]);
            }
        }
#pragma unroll
        for (int p = 0; p < RA; ++p) {
            if (p < a.A) {
#pragma unroll
                for (int e = 0; e < VW; ++e) {
                    const float d = v[p][e] - m[e];
                    const float ex = __expf(d);
                    s[e] += ex;
                    v[p][e] = a.log ? d : ex;
                }
            }
        }
#pragma unroll
        for (int e = 0; e < VW; ++e) s[e] = sm_row_const(a.log, s[e]);
#pragma unroll
        for (int p = 0; p < RA; ++p) {
            if (p < a.A) {
#pragma unroll
                for (int e = 0; e < VW; ++e) v[p][e] = sm_finish(a.log, v[p][e], s[e]);
                si_store_vec<T, VW>(out + p * out_step, v[p]);
            }
        }
    } else {
        for (int p = 0; p < a.A; ++p) {
            float x[VW];
            si_load_vec<T, VW>(in + p * in_step, x);
#pragma unroll
            for (int e = 0; e < VW; ++e) {
                const float mn = fmaxf(m[e], x[e]);
                const float ref = sm_ref(mn);
                s[e] = s[e] * __expf(m[e] - ref) + __expf(x[e] - ref);
                m[e] = mn;
            }
        }
#pragma unroll
        for (int e = 0; e < VW; ++e) s[e] = sm_row_const(a.log, s[e]);
        for (int p = 0; p < a.A; ++p) {
            float x[VW];
            si_load_vec<T, VW>(in + p * in_step, x);
#pragma unroll
            for (int e = 0; e < VW; ++e) {
                const float d = x[e] - m[e];
                x[e] = sm_finish(a.log, a.log ? d : __expf(d), s[e]);
            }
            si_store_vec<T, VW>(out + p * out_step, x);
        }
    }
}

template <typename T, int VW>
__global__ __launch_bounds__(SM_THREADS) void softmax_strided_kernel(SmArgs a) { sm_strided<T, VW, false>(a); }

template <typename T, int VW>
__global__ __launch_bounds__(SM_THREADS) void softmax_strided_online_kernel(SmArgs a) { sm_strided<T, VW, true>(a); }

// ---- host -----------------------------------------------------------------------------------------------------------------
// everything that can be decided without a device: SI_E_BADARG / SI_E_UNSUPPORTED / 0
int check_desc(const SiSoftmaxDesc* d) {
    if (!d) return SI_E_BADARG;
    if (d->axis < 0 || d->axis > 3 || (d->log != 0 && d->log != 1)) return SI_E_BADARG;
    return si_check_reduce_views(d->n, d->h, d->w, d->c, d->in_ld, d->out_ld, si_masked_pixels(d->n, d->h, d->w, 0), d->c);
}

enum Form { kGroup, kBlock, kBlockOnline, kStrided, kStridedOnline };

int axis_len(const SiSoftmaxDesc* d) { return d->axis == 0 ? d->n : d->axis == 1 ? d->h : d->axis == 2 ? d->w : d->c; }

// a function of the shape, never of n (axis != 0) or the row count
Form form_of(const SiSoftmaxDesc* d) {
    if (d->axis == 3) return d->c <= SI_SOFTMAX_GROUP_MAX_C ? kGroup : d->c <= SI_SOFTMAX_BLOCK_MAX_C ? kBlock : kBlockOnline;
    return axis_len(d) <= SI_SOFTMAX_STRIDED_REG_A ? kStrided : kStridedOnline;
}

template <typename T>
int vector_width(const SiSoftmaxDesc* d, const void* in, const void* out) { return si_vector_width<T>(d->c, d->in_ld, d->out_ld, in, out); }

template <typename T, int VW>
int launch(const SiSoftmaxDesc* d, const T* in, T* out, hipStream_t stream) {
    SmArgs a;
    a.in = in;
    a.out = out;
    a.rows = d->n * d->h * d->w;
    a.cv = d->c / VW;
    a.in_ld = d->in_ld;
    a.out_ld = d->out_ld;
    a.log = d->log;
    a.lg = 0;
    a.A = axis_len(d);
    a.inner = d->axis == 0 ? d->h * d->w : d->axis == 1 ? d->w : 1;
    a.items = 0;
    const dim3 block(SM_THREADS);
    switch (form_of(d)) {
        case kGroup: {
            // lanes per row: the power of two at or above cv / per, at most 64 (then up to SM_LANE_ELEMS / VW items per lane)
            constexpr int per = SM_LANE_ELEMS / VW < SM_GROUP_ITEMS ? SM_LANE_ELEMS / VW : SM_GROUP_ITEMS;
            a.lg = si_group_lg(a.cv, per);
            const int rows_per_block = SM_THREADS >> a.lg;
            hipLaunchKernelGGL((softmax_group_kernel<T, VW>), dim3((unsigned)((a.rows + rows_per_block - 1) / rows_per_block)), block, 0, stream, a);
            break;
        }
        case kBlock:
            hipLaunchKernelGGL((softmax_block_kernel<T, VW>), dim3((unsigned)a.rows), block, 0, stream, a);
            break;
        case kBlockOnline:
            hipLaunchKernelGGL((softmax_block_online_kernel<T, VW>), dim3((unsigned)a.rows), block, 0, stream, a);
            break;
        case kStrided:
        case kStridedOnline: {
            a.items = (a.rows / a.A) * a.cv;   // outer * inner * cv
            const dim3 grid(((unsigned)a.items + SM_THREADS - 1) / SM_THREADS);
            if (form_of(d) == kStrided)
                hipLaunchKernelGGL((softmax_strided_kernel<T, VW>), grid, block, 0, stream, a);
            else
                hipLaunchKernelGGL((softmax_strided_online_kernel<T, VW>), grid, block, 0, stream, a);
            break;
        }
    }
    return (int)hipGetLastError();
}

template <typename T>
int run(const SiSoftmaxDesc* d, const T* in, T* out, si_stream_t stream) {
    const int rc = check_desc(d);
    if (rc != 0) return rc;
    if (!in || !out) return SI_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    constexpr int full = (int)(16 / sizeof(T));
    return vector_width<T>(d, in, out) == full ? launch<T, full>(d, in, out, s) : launch<T, 1>(d, in, out, s);
}

}  // namespace

extern "C" {

int si_hip_softmax_f32(const SiSoftmaxDesc* d, const float* in, float* out, si_stream_t stream) { return run<float>(d, in, out, stream); }

int si_hip_softmax_f16(const SiSoftmaxDesc* d, const void* in, void* out, si_stream_t stream) {
    return run<_Float16>(d, static_cast<const _Float16*>(in), static_cast<_Float16*>(out), stream);
}

const char* si_hip_softmax_kernel_name(const SiSoftmaxDesc* d, const void* in, const void* out, int half) {
    if (check_desc(d) != 0) return "none";
    static const char* const names[5][4] = {SI_KERNEL_NAMES("softmax_group_kernel"), SI_KERNEL_NAMES("softmax_block_kernel"),
                                            SI_KERNEL_NAMES("softmax_block_online_kernel"), SI_KERNEL_NAMES("softmax_strided_kernel"),
                                            SI_KERNEL_NAMES("softmax_strided_online_kernel")};
    const bool vec = (half ? vector_width<_Float16>(d, in, out) : vector_width<float>(d, in, out)) > 1;
    return names[form_of(d)][si_kernel_name_index(half != 0, vec)];
}

}  // extern "C"
