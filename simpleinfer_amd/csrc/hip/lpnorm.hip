// lpnorm.hip -- torch.norm (p = 1, 2, inf) over axes of an NHWC tensor and F.normalize along one axis (include/si_lpnorm.h) on fp32 and
// fp16 tensors with pixel strides on both sides.  Arithmetic, special values, the order of additions, the forms and the refusals: the
// header.  reduce.hip is the model for the masks and their folding into levels, softmax.hip for the register-resident row.
//
// One float32 accumulator per set, starting at +0.  An element enters as |x| (p = 1, inf) or as x * x rounded on its own (p = 2); sums
// add, p = inf runs the NaN-keeping maximum of reduce.hip.  The square root is taken once, after the last combination.  normalize
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
constexpr int LN_LANE_ELEMS = 16;   // floats of a row that a lane of the register-resident row forms keeps
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
    int K1, ks0, ks1;    // kept pixel kp starts at input pixel (kp / K1) * ks0 + (kp % K1) * ks1
    int R, R1, rs0, rs1; // position r is (r / R1) * rs0 + (r % R1) * rs1 pixels further
};

template <bool MAX>
__device__ __forceinline__ float ln_combine(float a, float b) {
    if constexpr (MAX) return (a != a || a > b) ? a : b;
    return a + b;
}

// an element on its way in
__device__ __forceinline__ float ln_prep(int p, float x) { return p == SI_LPNORM_P2 ? x * x : fabsf(x); }

__device__ __forceinline__ float ln_finish(int p, float acc) { return p == SI_LPNORM_P2 ? sqrtf(acc) : acc; }

// the divisor of a set: max(norm, eps) as torch's clamp_min (a NaN norm stays)
__device__ __forceinline__ float ln_divisor(const LnArgs& a, float norm) { return norm < a.eps ? a.eps : norm; }

// butterfly over the xor offsets below `lanes` (a power of two <= 64): lane j's value becomes v[j] (+) v[j ^ off] at every step
template <bool MAX>
__device__ __forceinline__ float ln_team(float v, int lanes) {
    for (int off = lanes >> 1; off > 0; off >>= 1) v = ln_combine<MAX>(v, __shfl_xor(v, off, 64));
    return v;
}

// the whole workgroup: per wave as above, then the wave values in index order (every thread reads all of them).  The caller
// synchronises before `part` is written again.
template <bool MAX>
__device__ __forceinline__ float ln_block(float v, float* part) {
    v = ln_team<MAX>(v, 64);
    if (((int)threadIdx.x & 63) == 0) part[(int)threadIdx.x >> 6] = v;
    __syncthreads();
    float r = part[0];
#pragma unroll
    for (int w = 1; w < LN_WAVES; ++w) r = ln_combine<MAX>(r, part[w]);
    return r;
}

// the register-resident row: BLOCK = one workgroup per row, else a group of 1 << a.lg lanes per row
template <typename T, int VW, bool BLOCK, bool MAX>
__device__ __forceinline__ void ln_row_in_registers(const LnArgs& a, float* part) {
    constexpr int ITEMS = LN_LANE_ELEMS / VW;
    const int tid = (int)threadIdx.x;
    const int L = BLOCK ? LN_THREADS : (1 << a.lg);
    const int j = BLOCK ? tid : (tid & (L - 1));
    const unsigned rows_per_block = BLOCK ? 1u : (unsigned)(LN_THREADS >> a.lg);
    const unsigned sub = BLOCK ? 0u : (unsigned)(tid >> a.lg);
    // (the trip count is the same for every lane of the workgroup: all of them take part in every exchange)
    for (unsigned base = (unsigned)blockIdx.x * rows_per_block; base < (unsigned)a.rows; base += (unsigned)gridDim.x * rows_per_block) {
        const unsigned row = base + sub;
        const bool live = row < (unsigned)a.rows;   // (a dead row's lanes load and store nothing)
        const T* const in = static_cast<const T*>(a.in) + (size_t)(live ? row : 0u) * (unsigned)a.in_ld;
        float v[ITEMS][VW];
        float acc = 0.0f;
#pragma unroll
        for (int i = 0; i < ITEMS; ++i) {
            const int item = i * L + j;
            if (live && item < a.cv) {
                si_load_vec<T, VW>(in + item * VW, v[i]);
#pragma unroll
                for (int e = 0; e < VW; ++e) acc = ln_combine<MAX>(acc, ln_prep(a.p, v[i][e]));
            } else {
#pragma unroll
                for (int e = 0; e < VW; ++e) v[i][e] = 0.0f;
            }
        }
        if constexpr (BLOCK) acc = ln_block<MAX>(acc, part);
        else acc = ln_team<MAX>(acc, L);
        if (live) {
            const float norm = ln_finish(a.p, acc);
            T* const out = static_cast<T*>(a.out) + (size_t)row * (unsigned)a.out_ld;
            if (!a.normalize) {
                if (j == 0) out[0] = si_store_cast<T>(norm);
            } else {
                const float d = ln_divisor(a, norm);
#pragma unroll
                for (int i = 0; i < ITEMS; ++i) {
                    const int item = i * L + j;
                    if (item < a.cv) {
#pragma unroll
                        for (int e = 0; e < VW; ++e) v[i][e] = v[i][e] / d;
                        si_store_vec<T, VW>(out + item * VW, v[i]);
                    }
                }
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
        const float norm = ln_finish(a.p, ln_block<MAX>(acc, part));
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
        const unsigned k0 = kp / (unsigned)a.K1;
        const unsigned k1 = kp - k0 * (unsigned)a.K1;
        const unsigned pix0 = k0 * (unsigned)a.ks0 + k1 * (unsigned)a.ks1;   // the pixel of position 0
        float acc[VW];
#pragma unroll
        for (int e = 0; e < VW; ++e) acc[e] = 0.0f;
        if constexpr (REG) {
            // (one reduced axis: position r is r * rs1 pixels further)
            float v[LN_REG_R][VW];
#pragma unroll
            for (int r = 0; r < LN_REG_R; ++r) {
                if (r < a.R) {
                    si_load_vec<T, VW>(in + (size_t)(pix0 + (unsigned)(r * a.rs1)) * in_ld + c0, v[r]);
#pragma unroll
                    for (int e = 0; e < VW; ++e) acc[e] = ln_combine<MAX>(acc[e], ln_prep(a.p, v[r][e]));
                }
            }
#pragma unroll
            for (int e = 0; e < VW; ++e) acc[e] = ln_divisor(a, ln_finish(a.p, acc[e]));
#pragma unroll
            for (int r = 0; r < LN_REG_R; ++r) {
                if (r < a.R) {
#pragma unroll
                    for (int e = 0; e < VW; ++e) v[r][e] = v[r][e] / acc[e];
                    si_store_vec<T, VW>(out + (size_t)(pix0 + (unsigned)(r * a.rs1)) * out_ld + c0, v[r]);
                }
            }
        } else {
            // Pixel indices are unsigned: the step past the last position may wrap, and is unused.
            const unsigned step = (unsigned)a.rs1;
            const unsigned wrap = (unsigned)(a.rs0 - a.R1 * a.rs1);
            unsigned pix = pix0;
            int r1 = 0;
            for (int r = 0; r < a.R; ++r) {
                float x[VW];
                si_load_vec<T, VW>(in + (size_t)pix * in_ld + c0, x);
#pragma unroll
                for (int e = 0; e < VW; ++e) acc[e] = ln_combine<MAX>(acc[e], ln_prep(a.p, x[e]));
                pix += step;
                if (++r1 == a.R1) {
                    r1 = 0;
                    pix += wrap;
                }
            }
#pragma unroll
            for (int e = 0; e < VW; ++e) acc[e] = ln_finish(a.p, acc[e]);
            if (!a.normalize) {
                si_store_vec<T, VW>(out + (size_t)kp * out_ld + c0, acc);
            } else {
#pragma unroll
                for (int e = 0; e < VW; ++e) acc[e] = ln_divisor(a, acc[e]);
                pix = pix0;
                r1 = 0;
                for (int r = 0; r < a.R; ++r) {
                    float x[VW];
                    si_load_vec<T, VW>(in + (size_t)pix * in_ld + c0, x);
#pragma unroll
                    for (int e = 0; e < VW; ++e) x[e] = x[e] / acc[e];
                    si_store_vec<T, VW>(out + (size_t)pix * out_ld + c0, x);
                    pix += step;
                    if (++r1 == a.R1) {
                        r1 = 0;
                        pix += wrap;
                    }
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
constexpr int kAxisN = 1, kAxisH = 2, kAxisW = 4, kAxisC = 8;   // SI_REDUCE_AXIS_*
constexpr int kSpatial = kAxisN | kAxisH | kAxisW;

int out_channels(const SiLpNormDesc* d) { return (d->normalize || !(d->axes & kAxisC)) ? d->c : 1; }

uint64_t out_pixels(const SiLpNormDesc* d) {
    if (d->normalize) return (uint64_t)d->n * (uint64_t)d->h * (uint64_t)d->w;
    return (uint64_t)((d->axes & kAxisN) ? 1 : d->n) * (uint64_t)((d->axes & kAxisH) ? 1 : d->h) * (uint64_t)((d->axes & kAxisW) ? 1 : d->w);
}

// everything that can be decided without a device or a pointer: SI_E_BADARG / SI_E_UNSUPPORTED / 0
int check_desc(const SiLpNormDesc* d) {
    if (!d) return SI_E_BADARG;
    if (d->n <= 0 || d->h <= 0 || d->w <= 0 || d->c <= 0) return SI_E_BADARG;
    if (d->axes < 1 || d->axes > 15 || d->p < SI_LPNORM_P1 || d->p > SI_LPNORM_PINF) return SI_E_BADARG;
    if (d->normalize != 0 && d->normalize != 1) return SI_E_BADARG;
    if (!(d->eps >= 0.0f)) return SI_E_BADARG;   // (negative, or NaN)
    if (d->normalize && (d->axes & (d->axes - 1)) != 0) return SI_E_BADARG;
    if (d->in_ld < d->c || d->out_ld < out_channels(d)) return SI_E_BADARG;
    if ((d->axes & kAxisC) && (d->axes & kSpatial)) return SI_E_UNSUPPORTED;
    const uint64_t rows = (uint64_t)d->n * (uint64_t)d->h;   // < 2^62
    if (rows > SI_INDEX_LIMIT || rows * (uint64_t)d->w > SI_INDEX_LIMIT) return SI_E_UNSUPPORTED;
    const uint64_t pix = rows * (uint64_t)d->w;
    // offsets, and with them the item counts: at most one lane per element (c <= ld)
    if (pix * (uint64_t)d->in_ld > SI_INDEX_LIMIT || out_pixels(d) * (uint64_t)d->out_ld > SI_INDEX_LIMIT) return SI_E_UNSUPPORTED;
    return 0;
}

enum Form { kRowGroup, kRowBlock, kRowBlock2Pass, kColLane, kColLaneReg };

// the three spatial axes folded into kept and reduced levels of (count, pixel stride), outer first (reduce.hip's folding)
struct Levels {
    int kept[2][2] = {{1, 0}, {1, 0}};
    int red[2][2] = {{1, 0}, {1, 0}};
    uint64_t positions = 1;   // the product of the reduced extents
};

Levels levels_of(const SiLpNormDesc* d) {
    Levels lv;
    const int ext[3] = {d->n, d->h, d->w};
    const int stride[3] = {d->h * d->w, d->w, 1};
    int nk = 0, nr = 0;
    int kept[3][2], red[3][2];
    for (int a = 0; a < 3; ++a) {
        const bool reduced = (d->axes >> a) & 1;
        if (reduced) lv.positions *= (uint64_t)ext[a];
        if (ext[a] == 1) continue;
        int(*list)[2] = reduced ? red : kept;
        int& cnt = reduced ? nr : nk;
        if (cnt > 0 && list[cnt - 1][1] == ext[a] * stride[a]) {   // the level above is a run of this one
            list[cnt - 1][0] *= ext[a];
            list[cnt - 1][1] = stride[a];
        } else {
            list[cnt][0] = ext[a];
            list[cnt][1] = stride[a];
            ++cnt;
        }
    }
    // (three levels of one kind would need the other kind between each pair: there are three axes, so at most two)
    for (int i = 0; i < nk; ++i) { lv.kept[2 - nk + i][0] = kept[i][0]; lv.kept[2 - nk + i][1] = kept[i][1]; }
    for (int i = 0; i < nr; ++i) { lv.red[2 - nr + i][0] = red[i][0]; lv.red[2 - nr + i][1] = red[i][1]; }
    return lv;
}

// a function of the descriptor; n enters through the positions only, that is only when it is reduced
Form form_of(const SiLpNormDesc* d) {
    if (d->axes == kAxisC) return d->c <= SI_LPNORM_GROUP_MAX_C ? kRowGroup : d->c <= SI_LPNORM_BLOCK_MAX_C ? kRowBlock : kRowBlock2Pass;
    return (d->normalize && levels_of(d).positions <= (uint64_t)SI_LPNORM_COL_REG_POSITIONS) ? kColLaneReg : kColLane;
}

// 16-byte channel vectors when c, the strides and the pointers allow it (the row forms that store one element per pixel: their output
// does not enter); single elements otherwise
template <typename T>
int vector_width(const SiLpNormDesc* d, const void* in, const void* out) {
    if (d->axes == kAxisC && !d->normalize) return si_vector_width<T>(d->c, d->in_ld, d->in_ld, in, in);
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
    a.K1 = a.R1 = a.R = 1;
    const Form form = form_of(d);
    const dim3 block(LN_THREADS);
    if (form == kRowGroup || form == kRowBlock || form == kRowBlock2Pass) {
        a.rows = d->n * d->h * d->w;
        if (form == kRowGroup) {
            // lanes per row: the power of two at or above cv / per, at most 64 (then up to LN_LANE_ELEMS / VW items per lane)
            constexpr int per = LN_LANE_ELEMS / VW < LN_GROUP_ITEMS ? LN_LANE_ELEMS / VW : LN_GROUP_ITEMS;
            while ((1 << a.lg) < 64 && (1 << a.lg) * per < a.cv) ++a.lg;
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
    const Levels lv = levels_of(d);
    a.K1 = lv.kept[1][0];
    a.ks0 = lv.kept[0][1];
    a.ks1 = lv.kept[1][1];
    a.R = (int)lv.positions;
    a.R1 = lv.red[1][0];
    a.rs0 = lv.red[0][1];
    a.rs1 = lv.red[1][1];
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
    static const char* const names[5][4] = {
        {"lpnorm_row_group_kernel<float, 4>", "lpnorm_row_group_kernel<float, 1>", "lpnorm_row_group_kernel<_Float16, 8>",
         "lpnorm_row_group_kernel<_Float16, 1>"},
        {"lpnorm_row_block_kernel<float, 4>", "lpnorm_row_block_kernel<float, 1>", "lpnorm_row_block_kernel<_Float16, 8>",
         "lpnorm_row_block_kernel<_Float16, 1>"},
        {"lpnorm_row_block_2pass_kernel<float, 4>", "lpnorm_row_block_2pass_kernel<float, 1>", "lpnorm_row_block_2pass_kernel<_Float16, 8>",
         "lpnorm_row_block_2pass_kernel<_Float16, 1>"},
        {"lpnorm_col_lane_kernel<float, 4>", "lpnorm_col_lane_kernel<float, 1>", "lpnorm_col_lane_kernel<_Float16, 8>",
         "lpnorm_col_lane_kernel<_Float16, 1>"},
        {"lpnorm_col_lane_reg_kernel<float, 4>", "lpnorm_col_lane_reg_kernel<float, 1>", "lpnorm_col_lane_reg_kernel<_Float16, 8>",
         "lpnorm_col_lane_reg_kernel<_Float16, 1>"},
    };
    const bool vec = (half ? vector_width<_Float16>(d, in, out) : vector_width<float>(d, in, out)) > 1;
    return names[form_of(d)][(half ? 2 : 0) + (vec ? 0 : 1)];
}

}  // extern "C"
