// reduce.hip -- sum / mean / amax / amin over axes of an NHWC tensor (include/si_reduce.h) on fp32 and fp16 tensors with pixel strides on
// both sides.  Arithmetic, special values, the forms and the refusals: the header.  This is the project's plain reduction; the fixed
// order of its combinations, the fold of the mask and the position walk are the reduction commons (si_reduce_dev.h, si_reduce_plan.h).
//
// One accumulator per result, float32.  sum / mean add; amax / amin run ONE selection, the NaN-keeping maximum (SiMaxNan of
// si_reduce_dev.h: a NaN on either side comes out; fmaxf would drop it),
// amin being -max(-x): negation is exact and keeps a NaN a NaN.  The identity of an empty share is 0 (sum) or -inf (max).
//
// Channel axis (axes == 8), a ROW = the c channels of one pixel, seen as cv items (16-byte vectors, or single elements); the elements of
// an item enter the accumulator in channel order:
//   row_group  L = 2^k <= 64 lanes per row (the power of two at or above cv / 4, as softmax.hip sizes its groups), 256 / L rows per
//              workgroup; lane j takes items j, j + L, ...; a butterfly over the xor offsets below L; lane 0 of the group stores.
//   row_block  one workgroup per row, thread t takes items t, t + 256, ...; butterflies per wave, then the four wave values from LDS in
//              index order (si_block); thread 0 stores.
// Axes within {n, h, w}: the host folds the three axes into at most two KEPT levels and two REDUCED levels of (count, pixel stride) --
// neighbouring axes of one kind merge (h and w reduced are one run of h * w pixels), extents of 1 drop out; only {n, w} around a kept h
// (or kept around a reduced h) needs both levels.  An ITEM = (kept pixel, channel vector); every channel of the vector is a reduction
// of its own, nothing crosses lanes in col_lane:
//   col_lane   one lane per item, consecutive lanes take consecutive channel vectors and then consecutive kept pixels; the lane walks
//              the positions r = 0 .. R-1 (outer level first: increasing (n, h, w)).
//   col_coop   SI_REDUCE_COOP_SLOTS items per workgroup, SI_REDUCE_COOP_PARTS threads each: part g walks positions [g * chunk,
//              min(R, (g + 1) * chunk)), chunk = ceil(R / parts); the partials go to LDS and one thread per (item, channel) combines
//              those of the ceil(R / chunk) non-empty parts in the order g = 0, 1, ... and stores its element.
//
// Element offsets are 32-bit: the host refuses tensors whose offsets do not fit 31 bits.  Register table per instantiation: DESIGN.md 9i.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "si_hip_internal.h"
#include "si_reduce.h"

#pragma clang fp contract(off)

namespace {

constexpr int RD_THREADS = 256;
constexpr int RD_WAVES = RD_THREADS / 64;
constexpr int RD_GROUP_ITEMS = 4;   // items per lane that size a group
constexpr int RD_COOP_THREADS = SI_REDUCE_COOP_PARTS * SI_REDUCE_COOP_SLOTS;

static_assert(RD_COOP_THREADS <= 1024 && RD_COOP_THREADS % 64 == 0, "col_coop is one workgroup of whole waves");
static_assert(SI_REDUCE_COOP_SLOTS * 8 <= RD_COOP_THREADS, "one thread per (slot, channel) combines the partials");

struct RdArgs {
    const void* in;
    void* out;
    int in_ld, out_ld;
    int cv;              // items (channel vectors) per pixel
    int op;
    float count;         // mean: (float)positions
    int rows, lg;        // row forms: pixels; group: log2 of the lanes per row
    int items;           // col forms: kept pixels * cv
    SiLevelArgs lv;      // col forms: the kept pixels and the positions of the mask
    int chunk, parts;    // col_coop: positions per part, non-empty parts
};

template <bool MAX>
__device__ __forceinline__ float rd_identity() { return MAX ? -INFINITY : 0.0f; }

template <bool MAX>
__device__ __forceinline__ float rd_combine(float a, float b) { return SiSumOrMaxNan<MAX>::apply(a, b); }

// an element on its way in: amin runs as the maximum of the negated values
template <bool MAX>
__device__ __forceinline__ float rd_prep(int op, float x) { return (MAX && op == SI_REDUCE_AMIN) ? -x : x; }

template <bool MAX>
__device__ __forceinline__ float rd_finish(const RdArgs& a, float acc) {
    if constexpr (MAX) return a.op == SI_REDUCE_AMIN ? -acc : acc;
    return a.op == SI_REDUCE_MEAN ? acc / a.count : acc;
}

// BLOCK = one workgroup per row, else a group of 1 << a.lg lanes per row
template <typename T, int VW, bool BLOCK, bool MAX>
__device__ __forceinline__ void rd_row(const RdArgs& a, float* part) {
    const SiRowTile<T, VW, RD_THREADS, BLOCK> tile(a.lg);   // (its geometry alone: the row is streamed, not kept)
    const int L = tile.L, j = tile.j;
    const int row = (int)blockIdx.x * tile.rows_per_block + tile.sub;
    const bool live = row < a.rows;   // (a dead row's lanes load and store nothing but take part in every exchange)
    const T* const in = static_cast<const T*>(a.in) + (live ? row : 0) * a.in_ld;
    float acc = rd_identity<MAX>();
    if (live) {
        for (int item = j; item < a.cv; item += L) {
            float v[VW];
            si_load_vec<T, VW>(in + item * VW, v);
#pragma unroll
            for (int e = 0; e < VW; ++e) acc = rd_combine<MAX>(acc, rd_prep<MAX>(a.op, v[e]));
        }
    }
    if constexpr (BLOCK) {
        acc = si_block<SiSumOrMaxNan<MAX>, RD_WAVES>(acc, part);
        if (j != 0) return;
    } else {
        acc = si_team<SiSumOrMaxNan<MAX>>(acc, L);   // (lane 0 of the team is the one whose value is used)
        if (!live || j != 0) return;
    }
    static_cast<T*>(a.out)[row * a.out_ld] = si_store_cast<T>(rd_finish<MAX>(a, acc));
}

template <typename T, int VW>
__global__ __launch_bounds__(RD_THREADS) void reduce_row_group_kernel(RdArgs a) {
    if (a.op >= SI_REDUCE_AMAX)
        rd_row<T, VW, false, true>(a, nullptr);
    else
        rd_row<T, VW, false, false>(a, nullptr);
}

template <typename T, int VW>
__global__ __launch_bounds__(RD_THREADS) void reduce_row_block_kernel(RdArgs a) {
    __shared__ float part[RD_WAVES];
    if (a.op >= SI_REDUCE_AMAX)
        rd_row<T, VW, true, true>(a, part);
    else
        rd_row<T, VW, true, false>(a, part);
}

// the element offset of an item's first position, and where its result goes
template <int VW>
__device__ __forceinline__ void rd_item(const RdArgs& a, int item, unsigned& in_off, unsigned& out_off) {
    const int kp = item / a.cv;
    const int cvec = item - kp * a.cv;
    const int k0 = kp / a.lv.K1;
    const int k1 = kp - k0 * a.lv.K1;
    in_off = (unsigned)(k0 * a.lv.ks0 + k1 * a.lv.ks1) * (unsigned)a.in_ld + (unsigned)(cvec * VW);
    out_off = (unsigned)kp * (unsigned)a.out_ld + (unsigned)(cvec * VW);
}

// positions [start, end) of one item into acc, in order (element offsets: the walk counts in pixel strides)
template <typename T, int VW, bool MAX>
__device__ __forceinline__ void rd_walk(const RdArgs& a, const T* in, unsigned off0, int start, int end, float (&acc)[VW]) {
    SiLevelWalk walk(a.lv, (unsigned)a.in_ld, off0, start);
#pragma unroll 4
    for (int r = start; r < end; ++r, walk.next()) {
        float v[VW];
        si_load_vec<T, VW>(in + walk.off, v);
#pragma unroll
        for (int e = 0; e < VW; ++e) acc[e] = rd_combine<MAX>(acc[e], rd_prep<MAX>(a.op, v[e]));
    }
}

template <typename T, int VW, bool MAX>
__device__ __forceinline__ void rd_col_lane(const RdArgs& a) {
    const int item = (int)blockIdx.x * RD_THREADS + (int)threadIdx.x;
    if (item >= a.items) return;
    unsigned in_off, out_off;
    rd_item<VW>(a, item, in_off, out_off);
    float acc[VW];
#pragma unroll
    for (int e = 0; e < VW; ++e) acc[e] = rd_identity<MAX>();
    rd_walk<T, VW, MAX>(a, static_cast<const T*>(a.in), in_off, 0, a.lv.R, acc);
#pragma unroll
    for (int e = 0; e < VW; ++e) acc[e] = rd_finish<MAX>(a, acc[e]);
    si_store_vec<T, VW>(static_cast<T*>(a.out) + out_off, acc);
}

template <typename T, int VW>
__global__ __launch_bounds__(RD_THREADS) void reduce_col_lane_kernel(RdArgs a) {
    if (a.op >= SI_REDUCE_AMAX)
        rd_col_lane<T, VW, true>(a);
    else
        rd_col_lane<T, VW, false>(a);
}

template <typename T, int VW, bool MAX>
__device__ __forceinline__ void rd_col_coop(const RdArgs& a, float* part) {
    constexpr int S = SI_REDUCE_COOP_SLOTS;
    const int tid = (int)threadIdx.x;
    const int slot = tid % S, g = tid / S;
    const int item = (int)blockIdx.x * S + slot;
    float acc[VW];
#pragma unroll
    for (int e = 0; e < VW; ++e) acc[e] = rd_identity<MAX>();
    if (item < a.items && g < a.parts) {
        unsigned in_off, out_off;
        rd_item<VW>(a, item, in_off, out_off);
        const int start = g * a.chunk;
        const int end = start + a.chunk < a.lv.R ? start + a.chunk : a.lv.R;
        rd_walk<T, VW, MAX>(a, static_cast<const T*>(a.in), in_off, start, end, acc);
    }
#pragma unroll
    for (int e = 0; e < VW; ++e) part[tid * VW + e] = acc[e];   // [g][slot][e]
    __syncthreads();
    if (tid >= S * VW) return;
    const int slot2 = tid / VW, e2 = tid - slot2 * VW;
    const int item2 = (int)blockIdx.x * S + slot2;
    if (item2 >= a.items) return;
    float r = part[tid];   // g = 0
    for (int p = 1; p < a.parts; ++p) r = rd_combine<MAX>(r, part[p * (S * VW) + tid]);
    unsigned in_off, out_off;
    rd_item<VW>(a, item2, in_off, out_off);
    static_cast<T*>(a.out)[out_off + (unsigned)e2] = si_store_cast<T>(rd_finish<MAX>(a, r));
}

template <typename T, int VW>
__global__ __launch_bounds__(RD_COOP_THREADS) void reduce_col_coop_kernel(RdArgs a) {
    __shared__ float part[RD_COOP_THREADS * VW];
    if (a.op >= SI_REDUCE_AMAX)
        rd_col_coop<T, VW, true>(a, part);
    else
        rd_col_coop<T, VW, false>(a, part);
}

// ---- host -----------------------------------------------------------------------------------------------------------------
static_assert(SI_REDUCE_AXIS_N == SI_AXIS_N && SI_REDUCE_AXIS_H == SI_AXIS_H && SI_REDUCE_AXIS_W == SI_AXIS_W && SI_REDUCE_AXIS_C == SI_AXIS_C,
              "si_reduce_plan.h folds the header's mask");

int out_channels(const SiReduceDesc* d) { return (d->axes & SI_AXIS_C) ? 1 : d->c; }

// everything that can be decided without a device or a pointer: SI_E_BADARG / SI_E_UNSUPPORTED / 0
int check_desc(const SiReduceDesc* d) {
    if (!d) return SI_E_BADARG;
    if (d->axes < 1 || d->axes > 15 || d->op < SI_REDUCE_SUM || d->op > SI_REDUCE_AMIN) return SI_E_BADARG;
    // (every SI_E_BADARG before the mask refusal, and that one an SI_E_UNSUPPORTED like the limits: each descriptor keeps its code)
    const int rc = si_check_reduce_views(d->n, d->h, d->w, d->c, d->in_ld, d->out_ld, si_masked_pixels(d->n, d->h, d->w, d->axes), out_channels(d));
    if (rc != 0) return rc;
    if ((d->axes & SI_AXIS_C) && (d->axes & SI_AXIS_SPATIAL)) return SI_E_UNSUPPORTED;
    return 0;
}

// do the two views share an element?  (the strided-window rule of si_views.h)
bool views_overlap(const SiReduceDesc* d, const void* in, const void* out, size_t esize) {
    const uint64_t pix = (uint64_t)d->n * d->h * d->w;
    return si_strided_windows_overlap(in, pix, (uint64_t)d->in_ld, (uint64_t)d->c, out, si_masked_pixels(d->n, d->h, d->w, d->axes),
                                      (uint64_t)d->out_ld, (uint64_t)out_channels(d), esize);
}

enum Form { kRowGroup, kRowBlock, kColLane, kColCoop };

// a function of the descriptor; n enters through the positions only, that is only when it is reduced
Form form_of(const SiReduceDesc* d) {
    if (d->axes == SI_REDUCE_AXIS_C) return d->c <= SI_REDUCE_GROUP_MAX_C ? kRowGroup : kRowBlock;
    const SiLevels lv = si_fold_levels(d->n, d->h, d->w, d->axes);
    const uint64_t outputs_per_image = si_masked_pixels(1, d->h, d->w, d->axes) * (uint64_t)d->c;   // kept h x kept w x c
    const int force = SI_ENV_INT("SI_REDUCE_FORCE_COL", 0);   // experiment build only: 1 col_lane, 2 col_coop
    if (force == 1) return kColLane;
    if (force == 2) return kColCoop;
    return (lv.positions >= SI_REDUCE_COOP_MIN_POSITIONS && outputs_per_image <= SI_REDUCE_COOP_MAX_OUTPUTS) ? kColCoop : kColLane;
}

// 16-byte channel vectors when c, the strides and the pointers allow it (the row forms store single elements: their output does not
// enter); single elements otherwise
template <typename T>
int vector_width(const SiReduceDesc* d, const void* in, const void* out) {
    if (d->axes == SI_AXIS_C) return si_vector_width<T>(d->c, d->in_ld, d->in_ld, in, in);
    return si_vector_width<T>(d->c, d->in_ld, d->out_ld, in, out);
}

template <typename T, int VW>
int launch(const SiReduceDesc* d, const T* in, T* out, hipStream_t stream) {
    RdArgs a = {};
    a.in = in;
    a.out = out;
    a.in_ld = d->in_ld;
    a.out_ld = d->out_ld;
    a.cv = d->c / VW;
    a.op = d->op;
    a.chunk = a.parts = 1;
    const Form form = form_of(d);
    if (form == kRowGroup || form == kRowBlock) {
        a.rows = d->n * d->h * d->w;
        a.count = (float)d->c;
        if (form == kRowBlock) {
            hipLaunchKernelGGL((reduce_row_block_kernel<T, VW>), dim3((unsigned)a.rows), dim3(RD_THREADS), 0, stream, a);
        } else {
            // lanes per row: the power of two at or above cv / RD_GROUP_ITEMS, at most 64
            a.lg = si_group_lg(a.cv, RD_GROUP_ITEMS);
            const int rows_per_block = RD_THREADS >> a.lg;
            hipLaunchKernelGGL((reduce_row_group_kernel<T, VW>), dim3((unsigned)((a.rows + rows_per_block - 1) / rows_per_block)), dim3(RD_THREADS), 0,
                               stream, a);
        }
        return (int)hipGetLastError();
    }
    const SiLevels lv = si_fold_levels(d->n, d->h, d->w, d->axes);
    a.lv = si_level_args(lv);
    a.count = (float)lv.positions;
    a.items = lv.kept[0][0] * lv.kept[1][0] * a.cv;
    if (form == kColLane) {
        hipLaunchKernelGGL((reduce_col_lane_kernel<T, VW>), dim3(((unsigned)a.items + RD_THREADS - 1) / RD_THREADS), dim3(RD_THREADS), 0, stream, a);
    } else {
        a.chunk = (a.lv.R + SI_REDUCE_COOP_PARTS - 1) / SI_REDUCE_COOP_PARTS;
        a.parts = (a.lv.R + a.chunk - 1) / a.chunk;
        hipLaunchKernelGGL((reduce_col_coop_kernel<T, VW>), dim3(((unsigned)a.items + SI_REDUCE_COOP_SLOTS - 1) / SI_REDUCE_COOP_SLOTS),
                           dim3(RD_COOP_THREADS), 0, stream, a);
    }
    return (int)hipGetLastError();
}

template <typename T>
int run(const SiReduceDesc* d, const T* in, T* out, si_stream_t stream) {
    const int rc = check_desc(d);
    if (rc != 0) return rc;
    if (!in || !out) return SI_E_BADARG;
    if (views_overlap(d, in, out, sizeof(T))) return SI_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    constexpr int full = (int)(16 / sizeof(T));
    return vector_width<T>(d, in, out) == full ? launch<T, full>(d, in, out, s) : launch<T, 1>(d, in, out, s);
}

}  // namespace

extern "C" {

int si_hip_reduce_f32(const SiReduceDesc* d, const float* in, float* out, si_stream_t stream) { return run<float>(d, in, out, stream); }

int si_hip_reduce_f16(const SiReduceDesc* d, const void* in, void* out, si_stream_t stream) {
    return run<_Float16>(d, static_cast<const _Float16*>(in), static_cast<_Float16*>(out), stream);
}

const char* si_hip_reduce_kernel_name(const SiReduceDesc* d, const void* in, const void* out, int half) {
    if (check_desc(d) != 0) return "none";
    static const char* const names[4][4] = {SI_KERNEL_NAMES("reduce_row_group_kernel"), SI_KERNEL_NAMES("reduce_row_block_kernel"),
                                            SI_KERNEL_NAMES("reduce_col_lane_kernel"), SI_KERNEL_NAMES("reduce_col_coop_kernel")};
    const bool vec = (half ? vector_width<_Float16>(d, in, out) : vector_width<float>(d, in, out)) > 1;
    return names[form_of(d)][si_kernel_name_index(half != 0, vec)];
}

}  // extern "C"
