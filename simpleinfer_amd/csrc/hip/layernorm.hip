// layernorm.hip -- F.layer_norm over the last axis (include/si_layernorm.h) on fp32 and fp16 rows with row strides on both sides.
// Arithmetic, special values, the order of additions, the forms and the refusals: the header.  The lane butterfly, the workgroup combine
// and the register-resident row are the reduction commons (si_reduce_dev.h), called as softmax.hip and lpnorm.hip call them.
//
// What is this file's own: the row makes TWO trips through the combine without leaving the registers (the sum, then the squares of the
// values centred in place), and a lane's gamma / beta items are loaded once, before the grid-stride loop over the rows -- a lane owns
// the same items of every row it visits.
//
// Every kernel is a grid-stride loop under the usual cap (si_grid_for).  Element offsets are 32-bit: the host refuses views whose
// offsets do not fit 31 bits.  Register table per instantiation: DESIGN.md 9x.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "si_hip_internal.h"
#include "si_layernorm.h"

namespace {

constexpr int LY_THREADS = 256;
constexpr int LY_WAVES = LY_THREADS / 64;
constexpr int LY_LANE_ELEMS = SI_ROW_LANE_ELEMS;   // floats of a row that a lane keeps
constexpr int LY_GROUP_ITEMS = 4;                  // items per lane that size a group

static_assert(SI_LAYERNORM_GROUP_MAX_C == 64 * LY_LANE_ELEMS && SI_LAYERNORM_BLOCK_MAX_C == LY_THREADS * LY_LANE_ELEMS,
              "thresholds follow the register tile");

struct LyArgs {
    const void* in;
    void* out;
    const float* gamma;   // c floats, or null
    const float* beta;
    int in_ld, out_ld;
    int cv;               // items (channel vectors) per row
    int rows, lg;         // group form: log2 of the lanes per row
    float cf, eps;        // (float)c
};

__device__ __forceinline__ float ly_rstd(const LyArgs& a, float sq) { return 1.0f / sqrtf(sq / a.cf + a.eps); }

// ((d * rstd) * gamma) + beta; hg / hb: is there a gamma / a beta (the same for every lane of the launch)
__device__ __forceinline__ float ly_affine(float d, float rstd, bool hg, float g, bool hb, float b) {
    float y = d * rstd;
    if (hg) y = y * g;
    if (hb) y = y + b;
    return y;
}

// the items of `p` (gamma or beta) that lane j of L owns, in the layout of SiRowTile's registers; 0 beyond the row and for a null p
template <int ITEMS, int VW>
__device__ __forceinline__ void ly_lane_params(const float* p, int L, int j, int cv, float (&r)[ITEMS][VW]) {
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
        const int item = i * L + j;
        const bool have = p != nullptr && item < cv;
#pragma unroll
        for (int e = 0; e < VW; ++e) r[i][e] = have ? p[item * VW + e] : 0.0f;
    }
}

// the register-resident row: BLOCK = one workgroup per row, else a group of 1 << a.lg lanes per row
template <typename T, int VW, bool BLOCK>
__device__ __forceinline__ void ly_row_in_registers(const LyArgs& a, float* part) {
    using Tile = SiRowTile<T, VW, LY_THREADS, BLOCK>;
    const Tile tile(a.lg);
    const bool hg = a.gamma != nullptr, hb = a.beta != nullptr;
    // this lane's gamma / beta: the same items in every row of the loop below
    float g[Tile::ITEMS][VW], b[Tile::ITEMS][VW];
    ly_lane_params<Tile::ITEMS, VW>(a.gamma, tile.L, tile.j, a.cv, g);
    ly_lane_params<Tile::ITEMS, VW>(a.beta, tile.L, tile.j, a.cv, b);
    typename Tile::Regs v;
    const unsigned rows_per_block = (unsigned)tile.rows_per_block;
    // (the trip count is the same for every lane of the workgroup: all of them take part in every exchange)
    for (unsigned base = (unsigned)blockIdx.x * rows_per_block; base < (unsigned)a.rows; base += (unsigned)gridDim.x * rows_per_block) {
        const unsigned row = base + (unsigned)tile.sub;
        const bool live = row < (unsigned)a.rows;
        const T* const in = static_cast<const T*>(a.in) + (size_t)(live ? row : 0u) * (unsigned)a.in_ld;
        float sum = tile.load_row(v, in, live, a.cv, 0.0f, [](float s, float x) { return s + x; });
        if constexpr (BLOCK) {
            sum = si_block<SiSum, LY_WAVES>(sum, part);
            __syncthreads();   // (part is written again below)
        } else {
            sum = si_team<SiSum>(sum, tile.L);
        }
        const float mean = sum / a.cf;
        // centre in place, add the squares of what now stands in the registers
        float sq = tile.update_row(v, live, a.cv, 0.0f, [=](float s, float& x) {
            x = x - mean;
            return s + x * x;
        });
        if constexpr (BLOCK) sq = si_block<SiSum, LY_WAVES>(sq, part);
        else sq = si_team<SiSum>(sq, tile.L);
        if (live) {
            const float rstd = ly_rstd(a, sq);
            float (&d)[Tile::ITEMS][VW] = Tile::items(v);
#pragma unroll
            for (int i = 0; i < Tile::ITEMS; ++i) {
#pragma unroll
                for (int e = 0; e < VW; ++e) d[i][e] = ly_affine(d[i][e], rstd, hg, g[i][e], hb, b[i][e]);
            }
            T* const out = static_cast<T*>(a.out) + (size_t)row * (unsigned)a.out_ld;
            tile.store_row(v, out, a.cv, [](float y) { return y; });
        }
        if constexpr (BLOCK) __syncthreads();
    }
}

template <typename T, int VW>
__global__ __launch_bounds__(LY_THREADS) void layernorm_row_group_kernel(LyArgs a) {
    ly_row_in_registers<T, VW, false>(a, nullptr);
}

template <typename T, int VW>
__global__ __launch_bounds__(LY_THREADS) void layernorm_row_block_kernel(LyArgs a) {
    __shared__ float part[LY_WAVES];
    ly_row_in_registers<T, VW, true>(a, part);
}

// longer rows: thread t adds items t, t + 256, ... (the order of the block form), three reads of the row
template <typename T, int VW>
__global__ __launch_bounds__(LY_THREADS) void layernorm_row_block_3pass_kernel(LyArgs a) {
    __shared__ float part[LY_WAVES];
    const int tid = (int)threadIdx.x;
    const bool hg = a.gamma != nullptr, hb = a.beta != nullptr;
    for (unsigned row = (unsigned)blockIdx.x; row < (unsigned)a.rows; row += (unsigned)gridDim.x) {
        const T* const in = static_cast<const T*>(a.in) + (size_t)row * (unsigned)a.in_ld;
        T* const out = static_cast<T*>(a.out) + (size_t)row * (unsigned)a.out_ld;
        float sum = 0.0f;
        for (int item = tid; item < a.cv; item += LY_THREADS) {
            float x[VW];
            si_load_vec<T, VW>(in + item * VW, x);
#pragma unroll
            for (int e = 0; e < VW; ++e) sum = sum + x[e];
        }
        const float mean = si_block<SiSum, LY_WAVES>(sum, part) / a.cf;
        __syncthreads();
        float sq = 0.0f;
        for (int item = tid; item < a.cv; item += LY_THREADS) {
            float x[VW];
            si_load_vec<T, VW>(in + item * VW, x);
#pragma unroll
            for (int e = 0; e < VW; ++e) {
                const float d = x[e] - mean;
                sq = sq + d * d;
            }
        }
        const float rstd = ly_rstd(a, si_block<SiSum, LY_WAVES>(sq, part));
        for (int item = tid; item < a.cv; item += LY_THREADS) {
            float x[VW];
            si_load_vec<T, VW>(in + item * VW, x);
#pragma unroll
            for (int e = 0; e < VW; ++e)
                x[e] = ly_affine(x[e] - mean, rstd, hg, hg ? a.gamma[item * VW + e] : 0.0f, hb, hb ? a.beta[item * VW + e] : 0.0f);
            si_store_vec<T, VW>(out + item * VW, x);
        }
        __syncthreads();
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------
// everything that can be decided without a device or a pointer: SI_E_BADARG / SI_E_UNSUPPORTED / 0
int check_desc(const SiLayerNormDesc* d) {
    if (!d) return SI_E_BADARG;
    if (!(d->eps >= 0.0f)) return SI_E_BADARG;   // (negative, or NaN)
    return si_check_reduce_views(d->rows, 1, 1, d->c, d->in_ld, d->out_ld, (uint64_t)(d->rows > 0 ? d->rows : 0), d->c);
}

enum Form { kRowGroup, kRowBlock, kRowBlock3Pass };

Form form_of(const SiLayerNormDesc* d) {
    return d->c <= SI_LAYERNORM_GROUP_MAX_C ? kRowGroup : d->c <= SI_LAYERNORM_BLOCK_MAX_C ? kRowBlock : kRowBlock3Pass;
}

template <typename T>
int vector_width(const SiLayerNormDesc* d, const void* in, const void* out) {
    return si_vector_width<T>(d->c, d->in_ld, d->out_ld, in, out);
}

template <typename T, int VW>
int launch(const SiLayerNormDesc* d, const T* in, const float* gamma, const float* beta, T* out, hipStream_t stream) {
    LyArgs a = {};
    a.in = in;
    a.out = out;
    a.gamma = gamma;
    a.beta = beta;
    a.in_ld = d->in_ld;
    a.out_ld = d->out_ld;
    a.cv = d->c / VW;
    a.rows = d->rows;
    a.cf = (float)d->c;
    a.eps = d->eps;
    const Form form = form_of(d);
    const dim3 block(LY_THREADS);
    if (form == kRowGroup) {
        // lanes per row: the power of two at or above cv / per, at most 64 (then up to LY_LANE_ELEMS / VW items per lane)
        constexpr int per = LY_LANE_ELEMS / VW < LY_GROUP_ITEMS ? LY_LANE_ELEMS / VW : LY_GROUP_ITEMS;
        a.lg = si_group_lg(a.cv, per);
        const dim3 grid(si_grid_for((size_t)a.rows << a.lg, LY_THREADS));
        hipLaunchKernelGGL((layernorm_row_group_kernel<T, VW>), grid, block, 0, stream, a);
    } else {
        const dim3 grid(si_grid_for((size_t)a.rows, 1));
        if (form == kRowBlock)
            hipLaunchKernelGGL((layernorm_row_block_kernel<T, VW>), grid, block, 0, stream, a);
        else
            hipLaunchKernelGGL((layernorm_row_block_3pass_kernel<T, VW>), grid, block, 0, stream, a);
    }
    return (int)hipGetLastError();
}

template <typename T>
int run(const SiLayerNormDesc* d, const T* in, const float* gamma, const float* beta, T* out, si_stream_t stream) {
    const int rc = check_desc(d);
    if (rc == SI_E_BADARG) return rc;
    if (!in || !out) return SI_E_BADARG;
    if (rc != 0) return rc;
    // do the two views share an element?  (the strided-window rule of si_views.h)
    if (si_strided_windows_overlap(in, (uint64_t)d->rows, (uint64_t)d->in_ld, (uint64_t)d->c, out, (uint64_t)d->rows, (uint64_t)d->out_ld,
                                   (uint64_t)d->c, sizeof(T)))
        return SI_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    constexpr int full = (int)(16 / sizeof(T));
    return vector_width<T>(d, in, out) == full ? launch<T, full>(d, in, gamma, beta, out, s) : launch<T, 1>(d, in, gamma, beta, out, s);
}

}  // namespace

extern "C" {

int si_hip_layernorm_f32(const SiLayerNormDesc* d, const float* in, const float* gamma, const float* beta, float* out, si_stream_t stream) {
    return run<float>(d, in, gamma, beta, out, stream);
}

int si_hip_layernorm_f16(const SiLayerNormDesc* d, const void* in, const float* gamma, const float* beta, void* out, si_stream_t stream) {
    return run<_Float16>(d, static_cast<const _Float16*>(in), gamma, beta, static_cast<_Float16*>(out), stream);
}

const char* si_hip_layernorm_kernel_name(const SiLayerNormDesc* d, const void* in, const void* out, int half) {
    if (check_desc(d) != 0) return "none";
    static const char* const names[3][4] = {SI_KERNEL_NAMES("layernorm_row_group_kernel"), SI_KERNEL_NAMES("layernorm_row_block_kernel"),
                                            SI_KERNEL_NAMES("layernorm_row_block_3pass_kernel")};
    const bool vec = (half ? vector_width<_Float16>(d, in, out) : vector_width<float>(d, in, out)) > 1;
    return names[form_of(d)][si_kernel_name_index(half != 0, vec)];
}

}  // extern "C"
