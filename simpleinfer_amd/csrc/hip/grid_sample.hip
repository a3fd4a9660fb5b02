// grid_sample.hip -- F.grid_sample (4-D; bilinear and nearest; zeros, border and reflection padding; align_corners both ways) and
// F.affine_grid on NHWC fp32 and fp16 tensors (include/si_grid.h).  torch semantics; no reference counterpart.
//
// The rule (include/si_grid.h states it in full; this file is compiled with contraction off and writes every fused operation out, so the
// vector arms, the three grid sources and both storage types produce the same bits):
//     unnormalise   align_corners: p = ((g + 1) * 0.5f) * (size - 1)       otherwise: p = ((g + 1) * size - 1) * 0.5f        (torch's order)
//     border        p = fminf(fmaxf(p, 0), size - 1)
//     reflection    torch's reflect_coordinates about [0, size - 1] (align_corners) or [-0.5, size - 0.5], flips counted in float, then the clip
//     NaN           a coordinate that is still NaN gives NaN in every channel of the pixel
//     bilinear      taps floor / floor + 1; acc = 0, then acc = fmaf(weight, value, acc) for the taps inside the image in the order nw, ne, sw, se
//                   (a tap inside is multiplied also by a weight of 0; a tap outside is neither read nor added)
//     nearest       nearbyintf, half to even
//     integers      formed from a float clamped to [-2, size]
//     affine grid   base (2 j + 1 - W) / W or 2 j / (W - 1) - 1;  g = fmaf(t0, xb, fmaf(t1, yb, t2))
//
// Shape of the sampler: a gather bound by HBM / L2 -- one read of the taps, one write of the output.  A lane owns ONE channel vector of one
// output pixel; channel vectors run fastest across lanes, so a wave reads each tap of a pixel as one contiguous stretch and the lanes of a
// pixel share its two coordinates (one 8-byte load when the grid is dense in k: the "pair" source; the lanes of a pixel hit the same line).
// The four taps' loads are issued before the first is used.  The grid (si_grid_for) is capped and strides over the items.  32-bit index
// arithmetic: the host refuses what does not fit 31 bits.  No LDS, no scratch, no atomics, no workspace.
//
// -Rpass-analysis=kernel-resource-usage (gfx950, -O3), all twenty instantiations: scratch 0, LDS 0, 8 waves / SIMD except
// <_Float16, 8, theta> (70 VGPRs, 7 waves).  VGPRs, strided | pair | theta:
//     grid_sample_kernel<float, 4, .>     48 | 48 | 52        <float, 1, .>       38 | 38 | 42
//     <_Float16, 8, .>                    64 | 64 | 70        <_Float16, 4, .>    48 | 48 | 52
//     <_Float16, 2, .>                    40 | 40 | 44        <_Float16, 1, .>    38 | 38 | 42
//     affine_grid_kernel<float> 22, <_Float16> 20
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "si_grid.h"
#include "si_hip_internal.h"

// no implicit contraction anywhere in this file: every fused multiply-add below is written out
#pragma clang fp contract(off)

namespace {

template <typename T, int VW> struct VecOf;
template <> struct VecOf<float, 4> { typedef f32x4 type; };
template <> struct VecOf<float, 2> { typedef f32x2 type; };
template <> struct VecOf<float, 1> { typedef float type; };
template <> struct VecOf<_Float16, 8> { typedef f16x8 type; };
template <> struct VecOf<_Float16, 4> { typedef f16x4 type; };
template <> struct VecOf<_Float16, 2> { typedef f16x2 type; };
template <> struct VecOf<_Float16, 1> { typedef _Float16 type; };

constexpr int GRID_THREADS = 256;
constexpr int SRC_STRIDED = 0, SRC_PAIR = 1, SRC_THETA = 2;

struct GridArgs {
    const void* x;
    const void* grid;   // the grid, or theta
    void* out;
    int c, h, w, ho, wo;
    int cv;             // channel vectors per pixel
    int in_ld, out_ld;
    int mode, pad, ac;
    unsigned items;     // n ho wo cv
    int gs_n, gs_h, gs_w, gs_k;
};

template <typename T, int VW>
__device__ __forceinline__ void load_vec(const T* p, float (&v)[VW]) {
    typedef typename VecOf<T, VW>::type V;
    if constexpr (VW == 1) {
        v[0] = (float)*p;
    } else {
        const V r = *reinterpret_cast<const V*>(p);
#pragma unroll
        for (int i = 0; i < VW; ++i) v[i] = (float)r[i];
    }
}

template <typename T, int VW>
__device__ __forceinline__ void store_vec(T* p, const float (&v)[VW]) {
    typedef typename VecOf<T, VW>::type V;
    if constexpr (VW == 1) {
        *p = si_store_cast<T>(v[0]);
    } else {
        V r;
#pragma unroll
        for (int i = 0; i < VW; ++i) r[i] = si_store_cast<T>(v[i]);
        *reinterpret_cast<V*>(p) = r;
    }
}

// F.affine_grid's base coordinate of index j on an axis of `size`
__device__ __forceinline__ float affine_base(int j, int size, bool ac) {
    if (ac) return size > 1 ? __fdiv_rn((float)(2 * j), (float)(size - 1)) - 1.0f : 0.0f;
    return __fdiv_rn((float)(2 * j + 1 - size), (float)size);
}

// ... and the two coordinates of pixel (i, j) of image `img` from theta [n][2][3]
template <typename T>
__device__ __forceinline__ void affine_coords(const T* theta, int img, int i, int j, int h, int w, bool ac, float& gx, float& gy) {
    const T* const t = theta + img * 6;
    const float xb = affine_base(j, w, ac), yb = affine_base(i, h, ac);
    gx = __fmaf_rn((float)t[0], xb, __fmaf_rn((float)t[1], yb, (float)t[2]));
    gy = __fmaf_rn((float)t[3], xb, __fmaf_rn((float)t[4], yb, (float)t[5]));
}

// grid value -> pixel coordinate on an axis of `size`, padding applied
__device__ __forceinline__ float source_coord(float g, int size, int pad, bool ac) {
    const float fs = (float)size;
    float p = ac ? ((g + 1.0f) * 0.5f) * (fs - 1.0f) : ((g + 1.0f) * fs - 1.0f) * 0.5f;
    if (pad == SI_GRID_PAD_ZEROS) return p;
    if (pad == SI_GRID_PAD_REFLECTION) {
        const float lo = ac ? 0.0f : -0.5f, span = ac ? fs - 1.0f : fs;
        if (span == 0.0f) {
            p = 0.0f;
        } else {
            const float a = fabsf(p - lo);
            const float e = fmodf(a, span);
            const float f = floorf(__fdiv_rn(a, span));
            const bool even = f - 2.0f * floorf(f * 0.5f) == 0.0f;
            p = even ? e + lo : span - e + lo;
        }
    }
    return fminf(fmaxf(p, 0.0f), fs - 1.0f);   // (fmaxf drops a NaN operand: NaN becomes 0)
}

// a float that is an integer, +-Inf or huge -> int, clamped to [-2, size] first: both -2 and size have both taps outside the image
__device__ __forceinline__ int tap_index(float f, int size) { return (int)fminf(fmaxf(f, -2.0f), (float)size); }

// The workgroups that share an XCD (the dispatcher is observed to deal consecutive workgroups round the eight XCDs; nothing depends on it)
// take one consecutive run of the pass's items: neighbouring pixels share taps, and the run's source rows then stay in that XCD's L2
// instead of every XCD reading every row.  A bijection of [0, nwg) for every nwg.
__device__ __forceinline__ unsigned xcd_block(unsigned orig, unsigned nwg) {
    const unsigned q = nwg >> 3, r = nwg & 7u, x = orig & 7u;
    return (x < r ? x * (q + 1u) : r * (q + 1u) + (x - r) * q) + (orig >> 3);
}

template <typename T, int VW, int SRC>
__global__ __launch_bounds__(GRID_THREADS) void grid_sample_kernel(const GridArgs a) {
    const T* const x = static_cast<const T*>(a.x);
    const T* const grid = static_cast<const T*>(a.grid);
    T* const out = static_cast<T*>(a.out);
    const bool ac = a.ac != 0;
    const unsigned cv = (unsigned)a.cv, wo = (unsigned)a.wo, ho = (unsigned)a.ho;
    for (unsigned item = xcd_block(blockIdx.x, gridDim.x) * GRID_THREADS + threadIdx.x; item < a.items; item += gridDim.x * GRID_THREADS) {
        const unsigned pix = item / cv;
        const unsigned ch = (item - pix * cv) * VW;
        const unsigned row = pix / wo;
        const unsigned ox = pix - row * wo;
        const unsigned img = row / ho;
        const unsigned oy = row - img * ho;
        float gx, gy;
        if constexpr (SRC == SRC_THETA) {
            affine_coords<T>(grid, (int)img, (int)oy, (int)ox, a.ho, a.wo, ac, gx, gy);
        } else {
            const T* const g = grid + img * (unsigned)a.gs_n + oy * (unsigned)a.gs_h + ox * (unsigned)a.gs_w;
            if constexpr (SRC == SRC_PAIR) {
                const typename VecOf<T, 2>::type p = *reinterpret_cast<const typename VecOf<T, 2>::type*>(g);
                gx = (float)p[0];
                gy = (float)p[1];
            } else {
                gx = (float)g[0];
                gy = (float)g[a.gs_k];
            }
        }
        const float px = source_coord(gx, a.w, a.pad, ac);
        const float py = source_coord(gy, a.h, a.pad, ac);
        const T* const xi = x + img * (unsigned)(a.h * a.w) * (unsigned)a.in_ld + ch;
        float acc[VW];
#pragma unroll
        for (int i = 0; i < VW; ++i) acc[i] = 0.0f;
        if (px != px || py != py) {
#pragma unroll
            for (int i = 0; i < VW; ++i) acc[i] = __builtin_nanf("");
        } else if (a.mode == SI_GRID_NEAREST) {
            const int xn = tap_index(rintf(px), a.w), yn = tap_index(rintf(py), a.h);
            if ((unsigned)xn < (unsigned)a.w && (unsigned)yn < (unsigned)a.h) load_vec<T, VW>(xi + (unsigned)(yn * a.w + xn) * (unsigned)a.in_ld, acc);
        } else {
            const float x0f = floorf(px), y0f = floorf(py);
            const float wx1 = px - x0f, wx0 = (x0f + 1.0f) - px;
            const float wy1 = py - y0f, wy0 = (y0f + 1.0f) - py;
            const int x0 = tap_index(x0f, a.w), y0 = tap_index(y0f, a.h);
            const float wgt[4] = {wx0 * wy0, wx1 * wy0, wx0 * wy1, wx1 * wy1};
            bool in[4];
            float v[4][VW];
            // the four loads first, each under its own range test; then the chain
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int xx = x0 + (t & 1), yy = y0 + (t >> 1);
                in[t] = (unsigned)xx < (unsigned)a.w && (unsigned)yy < (unsigned)a.h;
#pragma unroll
                for (int i = 0; i < VW; ++i) v[t][i] = 0.0f;
                if (in[t]) load_vec<T, VW>(xi + (unsigned)(yy * a.w + xx) * (unsigned)a.in_ld, v[t]);
            }
#pragma unroll
            for (int t = 0; t < 4; ++t) {
#pragma unroll
                for (int i = 0; i < VW; ++i) acc[i] = in[t] ? __fmaf_rn(wgt[t], v[t][i], acc[i]) : acc[i];
            }
        }
        store_vec<T, VW>(out + pix * (unsigned)a.out_ld + ch, acc);
    }
}

// out [n][w][2][h], rows out_ld apart: one lane per element, h fastest
template <typename T>
__global__ __launch_bounds__(GRID_THREADS) void affine_grid_kernel(const T* __restrict__ theta, T* __restrict__ out, int h, int w, int out_ld, int ac,
                                                                   unsigned items) {
    for (unsigned item = blockIdx.x * GRID_THREADS + threadIdx.x; item < items; item += gridDim.x * GRID_THREADS) {
        const unsigned row = item / (unsigned)h;   // (img w + j) 2 + k
        const unsigned i = item - row * (unsigned)h;
        const unsigned k = row & 1u;
        const unsigned col = row >> 1;
        const unsigned img = col / (unsigned)w;
        const unsigned j = col - img * (unsigned)w;
        float gx, gy;
        affine_coords<T>(theta, (int)img, (int)i, (int)j, h, w, ac != 0, gx, gy);
        out[row * (unsigned)out_ld + i] = si_store_cast<T>(k ? gy : gx);
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------
constexpr int SIZE_LIMIT = 1 << 24;   // image sizes are used as floats: exact up to here

// the descriptor with its defaults filled in (a pixel stride of 0 is dense)
SiGridSampleDesc normalised(const SiGridSampleDesc* d) {
    SiGridSampleDesc r = *d;
    if (r.in_ld == 0) r.in_ld = r.c;
    if (r.out_ld == 0) r.out_ld = r.c;
    if (r.spatial_dims == 0) r.spatial_dims = 2;
    return r;
}

uint64_t grid_extent(const SiGridSampleDesc& d) {
    if (d.grid_source == SI_GRID_THETA) return (uint64_t)d.n * 6;
    const uint64_t limit = SI_INDEX_LIMIT;
    if ((uint64_t)d.gs_n > limit || (uint64_t)d.gs_h > limit || (uint64_t)d.gs_w > limit || (uint64_t)d.gs_k > limit) return 0;
    const uint64_t e = (uint64_t)(d.n - 1) * d.gs_n + (uint64_t)(d.ho - 1) * d.gs_h + (uint64_t)(d.wo - 1) * d.gs_w + (uint64_t)d.gs_k + 1;
    return e > limit ? 0 : e;
}

// everything that can be decided from the descriptor alone: SI_E_BADARG / SI_E_UNSUPPORTED / 0.  `d` is normalised.
int check_desc(const SiGridSampleDesc& d) {
    if (d.n <= 0 || d.c <= 0 || d.h <= 0 || d.w <= 0 || d.ho <= 0 || d.wo <= 0) return SI_E_BADARG;
    if (d.in_ld < d.c || d.out_ld < d.c) return SI_E_BADARG;
    if (d.mode < SI_GRID_BILINEAR || d.mode > SI_GRID_BICUBIC) return SI_E_BADARG;
    if (d.padding_mode < SI_GRID_PAD_ZEROS || d.padding_mode > SI_GRID_PAD_REFLECTION) return SI_E_BADARG;
    if (d.grid_source != SI_GRID_TENSOR && d.grid_source != SI_GRID_THETA) return SI_E_BADARG;
    if (d.spatial_dims != 2 && d.spatial_dims != 3) return SI_E_BADARG;
    if (d.grid_source == SI_GRID_TENSOR && (d.gs_n < 0 || d.gs_h < 0 || d.gs_w < 0 || d.gs_k < 0)) return SI_E_BADARG;
    if (d.mode == SI_GRID_BICUBIC || d.spatial_dims == 3) return SI_E_UNSUPPORTED;
    if (d.h > SIZE_LIMIT || d.w > SIZE_LIMIT || d.ho > SIZE_LIMIT || d.wo > SIZE_LIMIT) return SI_E_UNSUPPORTED;
    if (!si_view_extent(d.n, d.h, d.w, d.in_ld, d.c) || !si_view_extent(d.n, d.ho, d.wo, d.out_ld, d.c) || !grid_extent(d)) return SI_E_UNSUPPORTED;
    return 0;
}

int check_call(const SiGridSampleDesc& d, const void* x, const void* grid, const void* out, size_t es) {
    const int rc = check_desc(d);
    if (rc != 0) return rc;
    if (!x || !grid || !out) return SI_E_BADARG;
    const uint64_t out_bytes = si_view_extent(d.n, d.ho, d.wo, d.out_ld, d.c) * es;
    if (si_ranges_overlap(out, out_bytes, x, si_view_extent(d.n, d.h, d.w, d.in_ld, d.c) * es) || si_ranges_overlap(out, out_bytes, grid, grid_extent(d) * es))
        return SI_E_BADARG;
    return 0;
}

// widest channel vector (in elements) that c, both strides and both base pointers allow
template <typename T>
int vec_width(const SiGridSampleDesc& d, const void* x, const void* out) {
    const int widths[] = {(int)(16 / sizeof(T)), (int)(8 / sizeof(T)), (int)(4 / sizeof(T))};
    for (int w : widths) {
        if (w <= 1 || (sizeof(T) == 4 && w == 2)) continue;   // (fp32: 4 | 1)
        const size_t bytes = w * sizeof(T);
        if (d.c % w == 0 && d.in_ld % w == 0 && d.out_ld % w == 0 && si_aligned_to(x, bytes) && si_aligned_to(out, bytes)) return w;
    }
    return 1;
}

template <typename T>
int grid_src(const SiGridSampleDesc& d, const void* grid) {
    if (d.grid_source == SI_GRID_THETA) return SRC_THETA;
    const bool pair = d.gs_k == 1 && d.gs_n % 2 == 0 && d.gs_h % 2 == 0 && d.gs_w % 2 == 0 && si_aligned_to(grid, 2 * sizeof(T));
    return pair ? SRC_PAIR : SRC_STRIDED;
}

template <typename T, int VW, int SRC>
int launch(const SiGridSampleDesc& d, const void* x, const void* grid, void* out, hipStream_t stream) {
    GridArgs a;
    a.x = x; a.grid = grid; a.out = out;
    a.c = d.c; a.h = d.h; a.w = d.w; a.ho = d.ho; a.wo = d.wo;
    a.cv = d.c / VW;
    a.in_ld = d.in_ld; a.out_ld = d.out_ld;
    a.mode = d.mode; a.pad = d.padding_mode; a.ac = d.align_corners ? 1 : 0;
    a.items = (unsigned)((uint64_t)d.n * d.ho * d.wo * (uint64_t)a.cv);
    a.gs_n = (int)d.gs_n; a.gs_h = (int)d.gs_h; a.gs_w = (int)d.gs_w; a.gs_k = (int)d.gs_k;
    hipLaunchKernelGGL((grid_sample_kernel<T, VW, SRC>), dim3(si_grid_for(a.items, GRID_THREADS)), dim3(GRID_THREADS), 0, stream, a);
    return (int)hipGetLastError();
}

template <typename T, int VW>
int launch_src(int src, const SiGridSampleDesc& d, const void* x, const void* grid, void* out, hipStream_t stream) {
    switch (src) {
        case SRC_PAIR: return launch<T, VW, SRC_PAIR>(d, x, grid, out, stream);
        case SRC_THETA: return launch<T, VW, SRC_THETA>(d, x, grid, out, stream);
        default: return launch<T, VW, SRC_STRIDED>(d, x, grid, out, stream);
    }
}

template <typename T>
int run(const SiGridSampleDesc* desc, const void* x, const void* grid, void* out, si_stream_t stream) {
    if (!desc) return SI_E_BADARG;
    const SiGridSampleDesc d = normalised(desc);
    const int rc = check_call(d, x, grid, out, sizeof(T));
    if (rc != 0) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int src = grid_src<T>(d, grid);
    const int vw = vec_width<T>(d, x, out);
    if constexpr (sizeof(T) == 4) {
        return vw == 4 ? launch_src<T, 4>(src, d, x, grid, out, s) : launch_src<T, 1>(src, d, x, grid, out, s);
    } else {
        switch (vw) {
            case 8: return launch_src<T, 8>(src, d, x, grid, out, s);
            case 4: return launch_src<T, 4>(src, d, x, grid, out, s);
            case 2: return launch_src<T, 2>(src, d, x, grid, out, s);
            default: return launch_src<T, 1>(src, d, x, grid, out, s);
        }
    }
}

// ---- affine grid
int check_affine(const SiAffineGridDesc* d, const void* theta, const void* out, size_t es, int& out_ld) {
    if (!d) return SI_E_BADARG;
    if (d->n <= 0 || d->h <= 0 || d->w <= 0) return SI_E_BADARG;
    out_ld = d->out_ld == 0 ? d->h : d->out_ld;
    if (out_ld < d->h) return SI_E_BADARG;
    if (d->h > SIZE_LIMIT || d->w > SIZE_LIMIT) return SI_E_UNSUPPORTED;
    const uint64_t extent = si_view_extent(d->n, d->w, 2, out_ld, d->h);
    if (!extent || (uint64_t)d->n * 6 > SI_INDEX_LIMIT) return SI_E_UNSUPPORTED;
    if (!theta || !out) return SI_E_BADARG;
    if (si_ranges_overlap(out, extent * es, theta, (uint64_t)d->n * 6 * es)) return SI_E_BADARG;
    return 0;
}

template <typename T>
int run_affine(const SiAffineGridDesc* d, const void* theta, void* out, si_stream_t stream) {
    int out_ld = 0;
    const int rc = check_affine(d, theta, out, sizeof(T), out_ld);
    if (rc != 0) return rc;
    const unsigned items = (unsigned)((uint64_t)d->n * d->w * 2 * d->h);
    hipLaunchKernelGGL(affine_grid_kernel<T>, dim3(si_grid_for(items, GRID_THREADS)), dim3(GRID_THREADS), 0, (hipStream_t)stream,
                       static_cast<const T*>(theta), static_cast<T*>(out), d->h, d->w, out_ld, d->align_corners ? 1 : 0, items);
    return (int)hipGetLastError();
}

const char* const NAMES_F32[2][3] = {
    {"grid_sample_kernel<float, 4, strided>", "grid_sample_kernel<float, 4, pair>", "grid_sample_kernel<float, 4, theta>"},
    {"grid_sample_kernel<float, 1, strided>", "grid_sample_kernel<float, 1, pair>", "grid_sample_kernel<float, 1, theta>"}};
const char* const NAMES_F16[4][3] = {
    {"grid_sample_kernel<_Float16, 8, strided>", "grid_sample_kernel<_Float16, 8, pair>", "grid_sample_kernel<_Float16, 8, theta>"},
    {"grid_sample_kernel<_Float16, 4, strided>", "grid_sample_kernel<_Float16, 4, pair>", "grid_sample_kernel<_Float16, 4, theta>"},
    {"grid_sample_kernel<_Float16, 2, strided>", "grid_sample_kernel<_Float16, 2, pair>", "grid_sample_kernel<_Float16, 2, theta>"},
    {"grid_sample_kernel<_Float16, 1, strided>", "grid_sample_kernel<_Float16, 1, pair>", "grid_sample_kernel<_Float16, 1, theta>"}};

}  // namespace

extern "C" {

int si_hip_grid_sample_f32(const SiGridSampleDesc* d, const float* x, const float* grid_or_theta, float* out, si_stream_t stream) {
    return run<float>(d, x, grid_or_theta, out, stream);
}

int si_hip_grid_sample_f16(const SiGridSampleDesc* d, const void* x, const void* grid_or_theta, void* out, si_stream_t stream) {
    return run<_Float16>(d, x, grid_or_theta, out, stream);
}

const char* si_hip_grid_sample_kernel_name(const SiGridSampleDesc* desc, const void* x, const void* grid_or_theta, const void* out, int half) {
    if (!desc) return "none";
    const SiGridSampleDesc d = normalised(desc);
    if (check_call(d, x, grid_or_theta, out, half ? 2 : 4) != 0) return "none";
    if (!half) return NAMES_F32[vec_width<float>(d, x, out) == 4 ? 0 : 1][grid_src<float>(d, grid_or_theta)];
    const int vw = vec_width<_Float16>(d, x, out);
    return NAMES_F16[vw == 8 ? 0 : vw == 4 ? 1 : vw == 2 ? 2 : 3][grid_src<_Float16>(d, grid_or_theta)];
}

int si_hip_affine_grid_f32(const SiAffineGridDesc* d, const float* theta, float* out, si_stream_t stream) {
    return run_affine<float>(d, theta, out, stream);
}

int si_hip_affine_grid_f16(const SiAffineGridDesc* d, const void* theta, void* out, si_stream_t stream) {
    return run_affine<_Float16>(d, theta, out, stream);
}

const char* si_hip_affine_grid_kernel_name(const SiAffineGridDesc* d, const void* theta, const void* out, int half) {
    int out_ld = 0;
    if (check_affine(d, theta, out, half ? 2 : 4, out_ld) != 0) return "none";
    return half ? "affine_grid_kernel<_Float16>" : "affine_grid_kernel<float>";
}

}  // extern "C"
