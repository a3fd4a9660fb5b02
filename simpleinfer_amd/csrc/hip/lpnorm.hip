// lpnorm.hip -- torch.norm (p = 1, 2, inf) over axes of an NHWC tensor and F.normalize along one axis (include/si_lpnorm.h) on fp32 and
// fp16 tensors with pixel strides on both sides.  Arithmetic, special values, the order of additions, the forms and the refusals: the
// header.  The masks and their folding into levels, the combines and the register-resident row are the reduction commons
// (si_reduce_plan.h, si_reduce_dev.h).
//
// One float32 accumulator per set, starting at +0.  An element enters as |x| (p = 1, inf) or as x * x rounded on its own (p = 2); sums
// add, p = inf runs the NaN-keeping maximum (SiMaxNan).  The square root is taken once, after the last combination.  normalize
// divides every element by d = norm < eps ? eps : norm with the IEEE division.
//
// Every kernel is a grid-stride loop under the usual cap (si_grid_for); a set is computed by one lane, one group or one workgroup in an
// order that does not know the grid.  Element offsets are 32-bit: the host refuses tensors whose offsets do not fit 31 bits.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "si_hip_internal.h"
#include "si_lpnorm.h"

#pragma clang fp contract(off)

namespace {

constexpr int LN_THREADS = 256;
constexpr int LN_WAVES = LN_THREADS / 64;
constexpr int LN_LANE_ELEMS = SI_ROW_LANE_ELEMS;   // floats of a row that a lane of the register-resident row forms keeps
constexpr int LN_GROUP_ITEMS = 4;   // items per lane that size a group
constexpr int LN_REG_R = SI_LPNORM_COL_REG_POSITIONS;

static_assert(SI_LPNORM_GROUP_MAX_C == 64 * LN_LANE_ELEMS && SI_LPNORM_BLOCK_MAX_C == LN_THREADS * LN_LANE_ELEMS, "thresholds follow the register tile");

struct LnArgs {
    const void* in;
    void* out;
    int in_ld, out_ld;
    int cv;              // items (channel vectors) per pixel
    int p, normalize;
    float eps;
    int rows, lg;        // row forms: pixels; group: log2 of the lanes per row
    int items;           // col_lane: kept pixels * cv
    SiLevelArgs lv;      // col forms: the kept pixels and the positions of the mask
};

template <bool MAX>
__device__ __forceinline__ float ln_combine(float a, float b) { return SiSumOrMaxNan<MAX>::apply(a, b); }

// an element on its way in
__device__ __forceinline__ float ln_prep(int p, float x) { return p == SI_LPNORM_P2 ? x * x : fabsf(x); }

__device__ __forceinline__ float ln_finish(int p, float acc) { return p == SI_LPNORM_P2 ? sqrtf(acc) : acc; }

// the divisor of a set: max(norm, eps) as torch's clamp_min (a NaN norm stays)
__device__ __forceinline__ float ln_divisor(const LnArgs& a, float norm) { return norm < a.eps ? a.eps : norm; }

// the register-resident row: BLOCK = one workgroup per row, else a group of 1 << a.lg lanes per row
template <typename T, int VW, bool BLOCK, bool MAX>
__device__ __forceinline__ void ln_row_in_registers(const LnArgs& a, float* part) {
    using Tile = SiRowTile<T, VW, LN_THREADS, BLOCK>;
    using Op = SiSumOrMaxNan<MAX>;
    const Tile tile(a.lg);
    typename Tile::Regs v;
    const unsigned rows_per_block = (unsigned)tile.rows_per_block;
    // (the trip count is the same for every lane of the workgroup: all of them take part in every exchange)
    for (unsigned base = (unsigned)blockIdx.x * rows_per_block; base < (unsigned)a.rows; base += (unsigned)gridDim.x * rows_per_block) {
        const unsigned row = base + (unsigned)tile.sub;
        const bool live = row < (unsigned)a.rows;
        const T* const in = static_cast<const T*>(a.in) + (size_t)(live ? row : 0u) * (unsigned)a.in_ld;
        const int p = a.p;
        float acc = tile.load_row(v, in, live, a.cv, 0.0f, [=](float sum, float x) { return Op::apply(sum, ln_prep(p, x)); });
        if constexpr (BLOCK) acc = si_block<Op, LN_WAVES>(acc, part);
        else acc = si_team<Op>(acc, tile.L);
        if (live) {
            const float norm = ln_finish(a.p, acc);
            T* const out = static_cast<T*>(a.out) + (size_t)row * (unsigned)a.out_ld;
            if (!a.normalize) {
                if (tile.j == 0) out[0] = si_store_cast<T>(norm);
            } else {
                const float d = ln_divisor(a, norm);
                tile.store_row(v, out, a.cv, [=](float x) { return x / d; });
            }
        }
        if constexpr (BLOCK) __syncthreads();
    }
}

template <typename T, int VW>
__global__ __launch_bounds__(LN_THREADS) void lpnorm_row_group_kernel(LnArgs a) {
    if (a.p == SI_LPNORM_PINF)
        ln_row_in_registers<T, VW, false, true>(a, nullptr);
    else
        ln_row_in_registers<T, VW, false, false>(a, nullptr);
}

template <typename T, int VW>
__global__ __launch_bounds__(LN_THREADS) void lpnorm_row_block_kernel(LnArgs a) {
    __shared__ float part[LN_WAVES];
    if (a.p == SI_LPNORM_PINF)
        ln_row_in_registers<T, VW, true, true>(a, part);
    else
        ln_row_in_registers<T, VW, true, false>(a, part);
}

template <typename T, int VW, bool MAX>
__device__ __forceinline__ void ln_row_2pass(const LnArgs& a, float* part) {
    const int tid = (int)threadIdx.x;
    for (unsigned row = (unsigned)blockIdx.x; row < (unsigned)a.rows; row += (unsigned)gridDim.x) {
        const T* const in = static_cast<const T*>(a.in) + (size_t)row * (unsigned)a.in_ld;
        T* const out = static_cast<T*>(a.out) + (size_t)row * (unsigned)a.out_ld;
        float acc = 0.0f;
        for (int item = tid; item < a.cv; item += LN_THREADS) {
            float x[VW];
            si_load_vec<T, VW>(in + item * VW, x);
#pragma unroll
            for (int e = 0; e < VW; ++e) acc = ln_combine<MAX>(acc, ln_prep(a.p, x[e]));
        }
        const float norm = ln_finish(a.p, si_block<SiSumOrMaxNan<MAX>, LN_WAVES>(acc, part));
        if (!a.normalize) {
            if (tid == 0) out[0] = si_store_cast<T>(norm);
        } else {
            const float d = ln_divisor(a, norm);
            for (int item = tid; item < a.cv; item += LN_THREADS) {
                float x[VW];
                si_load_vec<T, VW>(in + item * VW, x);
#pragma unroll
                for (int e = 0; e < VW; ++e) x[e] = x[e] / d;
                si_store_vec<T, VW>(out + item * VW, x);
            }
        }
        __syncthreads();
    }
}

template <typename T, int VW>
__global__ __launch_bounds__(LN_THREADS) void lpnorm_row_block_2pass_kernel(LnArgs a) {
    __shared__ float part[LN_WAVES];
    if (a.p == SI_LPNORM_PINF)
        ln_row_2pass<T, VW, true>(a, part);
    else
        ln_row_2pass<T, VW, false>(a, part);
}

// One lane per item.  REG: normalize over one axis of at most LN_REG_R positions, kept in registers; else the lane walks its positions
// (two levels, outer first) and, with normalize, walks them again.
template <typename T, int VW, bool REG, bool MAX>
__device__ __forceinline__ void ln_col_lane(const LnArgs& a) {
    const T* const in = static_cast<const T*>(a.in);
    T* const out = static_cast<T*>(a.out);
    const unsigned in_ld = (unsigned)a.in_ld, out_ld = (unsigned)a.out_ld;
    for (unsigned item = (unsigned)blockIdx.x * LN_THREADS + threadIdx.x; item < (unsigned)a.items; item += (unsigned)gridDim.x * LN_THREADS) {
        const unsigned kp = item / (unsigned)a.cv;
        const unsigned c0 = (item - kp * (unsigned)a.cv) * VW;
        const unsigned k0 = kp / (unsigned)a.lv.K1;
        const unsigned k1 = kp - k0 * (unsigned)a.lv.K1;
        const unsigned pix0 = k0 * (unsigned)a.lv.ks0 + k1 * (unsigned)a.lv.ks1;   // the pixel of position 0
        float acc[VW];
#pragma unroll
        for (int e = 0; e < VW; ++e) acc[e] = 0.0f;
        if constexpr (REG) {
            // (one reduced axis: position r is r * rs1 pixels further)
            float v[LN_REG_R][VW];
#pragma unroll
            for (int r = 0; r < LN_REG_R; ++r) {
                if (r < a.lv.R) {
                    si_load_vec<T, VW>(in + (size_t)(pix0 + (unsigned)(r * a.lv.rs1)) * in_ld + c0, v[r]);
#pragma unroll
                    for (int e = 0; e < VW; ++e) acc[e] = ln_combine<MAX>(acc[e], ln_prep(a.p, v[r][e]));
                }
            }
#pragma unroll
            for (int e = 0; e < VW; ++e) acc[e] = ln_divisor(a, ln_finish(a.p, acc[e]));
#pragma unroll
            for (int r = 0; r < LN_REG_R; ++r) {
                if (r < a.lv.R) {
#pragma unroll
                    for (int e = 0; e < VW; ++e) v[r][e] = v[r][e] / acc[e];
                    si_store_vec<T, VW>(out + (size_t)(pix0 + (unsigned)(r * a.lv.rs1)) * out_ld + c0, v[r]);
                }
            }
        } else {
            SiLevelWalk pix(a.lv, 1u, pix0, 0);
            for (int r = 0; r < a.lv.R; ++r, pix.next()) {
                float x[VW];
                si_load_vec<T, VW>(in + (size_t)pix.off * in_ld + c0, x);
#pragma unroll
                for (int e = 0; e < VW; ++e) acc[e] = ln_combine<MAX>(acc[e], ln_prep(a.p, x[e]));
            }
#pragma unroll
            for (int e = 0; e < VW; ++e) acc[e] = ln_finish(a.p, acc[e]);
            if (!a.normalize) {
                si_store_vec<T, VW>(out + (size_t)kp * out_ld + c0, acc);
            } else {
#pragma unroll
                for (int e = 0; e < VW; ++e) acc[e] = ln_divisor(a, acc[e]);
                pix = SiLevelWalk(a.lv, 1u, pix0, 0);
                for (int r = 0; r < a.lv.R; ++r, pix.next()) {
                    float x[VW];
                    si_load_vec<T, VW>(in + (size_t)pix.off * in_ld + c0, x);
#pragma unroll
                    for (int e = 0; e < VW; ++e) x[e] = x[e] / acc[e];
                    si_store_vec<T, VW>(out + (size_t)pix.off * out_ld + c0, x);
                }
            }
        }
    }
}

template <typename T, int VW>
__global__ __launch_bounds__(LN_THREADS) void lpnorm_col_lane_kernel(LnArgs a) {
    if (a.p == SI_LPNORM_PINF)
        ln_col_lane<T, VW, false, true>(a);
    else
        ln_col_lane<T, VW, false, false>(a);
}

template <typename T, int VW>
__global__ __launch_bounds__(LN_THREADS) void lpnorm_col_lane_reg_kernel(LnArgs a) {
    if (a.p == SI_LPNORM_PINF)
        ln_col_lane<T, VW, true, true>(a);
    else
        ln_col_lane<T, VW, true, false>(a);
}

// ---- host -----------------------------------------------------------------------------------------------------------------
int out_channels(const SiLpNormDesc* d) { return (d->normalize || !(d->axes & SI_AXIS_C)) ? d->c : 1; }

uint64_t out_pixels(const SiLpNormDesc* d) { return si_masked_pixels(d->n, d->h, d->w, d->normalize ? 0 : d->axes); }

// everything that can be decided without a device or a pointer: SI_E_BADARG / SI_E_UNSUPPORTED / 0
int check_desc(const SiLpNormDesc* d) {
    if (!d) return SI_E_BADARG;
    if (d->axes < 1 || d->axes > 15 || d->p < SI_LPNORM_P1 || d->p > SI_LPNORM_PINF) return SI_E_BADARG;
    if (d->normalize != 0 && d->normalize != 1) return SI_E_BADARG;
    if (!(d->eps >= 0.0f)) return SI_E_BADARG;   // (negative, or NaN)
    if (d->normalize && (d->axes & (d->axes - 1)) != 0) return SI_E_BADARG;
    // (every SI_E_BADARG before the mask refusal, and that one an SI_E_UNSUPPORTED like the limits: each descriptor keeps its code)
    const int rc = si_check_reduce_views(d->n, d->h, d->w, d->c, d->in_ld, d->out_ld, out_pixels(d), out_channels(d));
    if (rc != 0) return rc;
    if ((d->axes & SI_AXIS_C) && (d->axes & SI_AXIS_SPATIAL)) return SI_E_UNSUPPORTED;
    return 0;
}

enum Form { kRowGroup, kRowBlock, kRowBlock2Pass, kColLane, kColLaneReg };

// a function of the descriptor; n enters through the positions only, that is only when it is reduced
Form form_of(const SiLpNormDesc* d) {
    if (d->axes == SI_AXIS_C) return d->c <= SI_LPNORM_GROUP_MAX_C ? kRowGroup : d->c <= SI_LPNORM_BLOCK_MAX_C ? kRowBlock : kRowBlock2Pass;
    return (d->normalize && si_fold_levels(d->n, d->h, d->w, d->axes).positions <= (uint64_t)SI_LPNORM_COL_REG_POSITIONS) ? kColLaneReg : kColLane;
}

// 16-byte channel vectors when c, the strides and the pointers allow it (the row forms that store one element per pixel: their output
// does not enter); single elements otherwise
template <typename T>
int vector_width(const SiLpNormDesc* d, const void* in, const void* out) {
    if (d->axes == SI_AXIS_C && !d->normalize) return si_vector_width<T>(d->c, d->in_ld, d->in_ld, in, in);
    return si_vector_width<T>(d->c, d->in_ld, d->out_ld, in, out);
}

template <typename T, int VW>
int launch(const SiLpNormDesc* d, const T* in, T* out, hipStream_t stream) {
    LnArgs a = {};
    a.in = in;
    a.out = out;
    a.in_ld = d->in_ld;
    a.out_ld = d->out_ld;
    a.cv = d->c / VW;
    a.p = d->p;
    a.normalize = d->normalize;
    a.eps = d->eps;
    const Form form = form_of(d);
    const dim3 block(LN_THREADS);
    if (form == kRowGroup || form == kRowBlock || form == kRowBlock2Pass) {
        a.rows = d->n * d->h * d->w;
        if (form == kRowGroup) {
            // lanes per row: the power of two at or above cv / per, at most 64 (then up to LN_LANE_ELEMS / VW items per lane)
            constexpr int per = LN_LANE_ELEMS / VW < LN_GROUP_ITEMS ? LN_LANE_ELEMS / VW : LN_GROUP_ITEMS;
            a.lg = si_group_lg(a.cv, per);
            const dim3 grid(si_grid_for((size_t)a.rows << a.lg, LN_THREADS));
            hipLaunchKernelGGL((lpnorm_row_group_kernel<T, VW>), grid, block, 0, stream, a);
        } else {
            const dim3 grid(si_grid_for((size_t)a.rows, 1));
            if (form == kRowBlock)
                hipLaunchKernelGGL((lpnorm_row_block_kernel<T, VW>), grid, block, 0, stream, a);
            else
                hipLaunchKernelGGL((lpnorm_row_block_2pass_kernel<T, VW>), grid, block, 0, stream, a);
        }
        return (int)hipGetLastError();
    }
    const SiLevels lv = si_fold_levels(d->n, d->h, d->w, d->axes);
    a.lv = si_level_args(lv);
    a.items = lv.kept[0][0] * lv.kept[1][0] * a.cv;
    const dim3 grid(si_grid_for((size_t)a.items, LN_THREADS));
    if (form == kColLaneReg)
        hipLaunchKernelGGL((lpnorm_col_lane_reg_kernel<T, VW>), grid, block, 0, stream, a);
    else
        hipLaunchKernelGGL((lpnorm_col_lane_kernel<T, VW>), grid, block, 0, stream, a);
    return (int)hipGetLastError();
}

template <typename T>
int run(const SiLpNormDesc* d, const T* in, T* out, si_stream_t stream) {
    const int rc = check_desc(d);
    if (rc == SI_E_BADARG) return rc;
    if (!in || !out) return SI_E_BADARG;
    if (rc != 0) return rc;
    // do the two views share an element?  (the strided-window rule of si_views.h)
    const uint64_t pix = (uint64_t)d->n * d->h * d->w;
    if (si_strided_windows_overlap(in, pix, (uint64_t)d->in_ld, (uint64_t)d->c, out, out_pixels(d), (uint64_t)d->out_ld, (uint64_t)out_channels(d),
                                   sizeof(T)))
        return SI_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    constexpr int full = (int)(16 / sizeof(T));
    return vector_width<T>(d, in, out) == full ? launch<T, full>(d, in, out, s) : launch<T, 1>(d, in, out, s);
}

}  // namespace

extern "C" {

int si_hip_lpnorm_f32(const SiLpNormDesc* d, const float* in, float* out, si_stream_t stream) { return run<float>(d, in, out, stream); }

int si_hip_lpnorm_f16(const SiLpNormDesc* d, const void* in, void* out, si_stream_t stream) {
    return run<_Float16>(d, static_cast<const _Float16*>(in), static_cast<_Float16*>(out), stream);
}

const char* si_hip_lpnorm_kernel_name(const SiLpNormDesc* d, const void* in, const void* out, int half) {
    if (check_desc(d) != 0) return "none";
    static const char* const names[5][4] = {SI_KERNEL_NAMES("lpnorm_row_group_kernel"), SI_KERNEL_NAMES("lpnorm_row_block_kernel"),
                                            SI_KERNEL_NAMES("lpnorm_row_block_2pass_kernel"), SI_KERNEL_NAMES("lpnorm_col_lane_kernel"),
                                            SI_KERNEL_NAMES("lpnorm_col_lane_reg_kernel")};
    const bool vec = (half ? vector_width<_Float16>(d, in, out) : vector_width<float>(d, in, out)) > 1;
    return names[form_of(d)][si_kernel_name_index(half != 0, vec)];
}

}  // extern "C"
