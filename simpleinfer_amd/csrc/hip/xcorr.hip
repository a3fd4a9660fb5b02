// xcorr.hip -- the cross-correlation kernels of F.conv2d with a tensor filter (include/si_xcorr.h).  Forms, reduction orders, contract and
// refusals: the header.  Form choice, extents, view rules, the grid and the 31-bit checks: xcorr_plan.h.
//
// Dense.  A workgroup of four waves owns 64 output pixels x 64 filters of one image; wave w owns pixels 16 w .. 16 w + 15 of the tile and
// all 64 filters as four 16-row MFMA tiles, one accumulator each (four independent chains; with fewer than 49 filters the launch is the
// instance with as many tiles as they need, one for O = 1 .. 16).  With lane = 16 g + x (g = 0..3, x = 0..15) one MFMA step is one tap (ky, kx) of one channel group:
//     A  the filters: lane holds w[o = 16 tile + x][ky][kx][channels 16 q + 4 g + 0..3] (fp32: four MFMA steps, step j taking element j)
//        or channels 32 q + 8 g + 0..7 (fp16: one step), 16 bytes read from the filter tensor where it lies -- the tensor changes every
//        forward, so there is no image to pack it into
//     B  the input: lane holds x[n][oy sh - pt + ky dh][ox sw - pl + kx dw][the same channels] of ITS pixel, a real zero when the tap lies
//        outside the image (never read)
// The C/D map puts the PIXEL on x and filter 4 g + r in register r: a lane stores four consecutive channels of one NHWC pixel at once.
// A fragment is one 16-byte read where the view is aligned; the element path loads the same elements one by one, in the same order.
//
// Depthwise.  One item = 16 bytes of consecutive channels of one output pixel; a lane walks the taps in ascending (ky, kx) order with one
// fmaf per tap and channel, skipping the taps outside the image.  The three vector decisions (x, w, y) are independent: in the unfused
// addressing the taps of a channel are kh kw ld apart in w, which is the element path for w while x and y keep their 16-byte accesses.
//
// One integer division per lane (output pixel -> row, column) and one per depthwise item; none in a loop.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <type_traits>

#include "si_hip_internal.h"
#include "si_xcorr.h"
#include "xcorr_plan.h"

#pragma clang fp contract(off)

namespace {

namespace plan = si_xcorr_plan;

constexpr int XC_THREADS = plan::kThreads;
static_assert(plan::kBlockPix == plan::kWavePix * (XC_THREADS / 64), "a wave owns 16 output pixels");

struct XcorrArgs {
    const void* x;
    const void* w;
    const float* bias;
    void* y;
    int h, w_in, c, oc, ho, wo, kh, kw, sh, sw, dh, dw, pt, pl;
    int npix, runs;
    int x_sn, x_sh, x_sp, w_sn, w_sh, w_sp, w_sc, y_sn, y_sh, y_sp;
    int x_vec, w_vec, y_vec;
    int act;
    float act_param;
};

__device__ __forceinline__ f32x4 xc_mma(float w, float b, f32x4 acc) { return __builtin_amdgcn_mfma_f32_16x16x4f32(w, b, acc, 0, 0, 0); }
__device__ __forceinline__ f32x4 xc_mma(f16x8 w, f16x8 b, f32x4 acc) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(w, b, acc, 0, 0, 0); }

// A lane's fragment of one channel block: CH_LANE consecutive channels starting at `c`, 16 bytes of the storage type.  The load itself is
// unconditional -- a fragment that is not live reads element 0 of its view, which always exists, and is then replaced by zeros -- so that the
// loads of several blocks can be in flight before the first MFMA needs one; what lies outside the image or beyond the channels is never read.
// `vec`: one 16-byte read; else the same elements one by one (any alignment, any channel stride, a ragged last block).
__device__ __forceinline__ f32x4 xc_frag(const float* p, int off, int c, int sc, int cmax, bool live, bool vec) {
    f32x4 v;
    if (vec) {
        v = *reinterpret_cast<const f32x4*>(p + (live ? off + c : 0));
        if (!live) v = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool lj = live && c + j < cmax;
            const float e = p[lj ? off + (c + j) * sc : 0];
            v[j] = lj ? e : 0.0f;
        }
    }
    return v;
}
__device__ __forceinline__ f16x8 xc_frag(const _Float16* p, int off, int c, int sc, int /*cmax*/, bool live, bool vec) {
    f16x8 v;
    if (vec) {
        v = *reinterpret_cast<const f16x8*>(p + (live ? off + c : 0));
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = p[live ? off + (c + j) * sc : 0];   // (c % 8 == 0: the 8 channels are in or out together)
    }
    if (!live) v = f16x8{0, 0, 0, 0, 0, 0, 0, 0};
    return v;
}

// one channel block into an accumulator: fp16 is ONE 16x16x32 step; fp32 four 16x16x4 steps, step j holding element j of every lane's
// fragment -- channels 4 g + j, g = 0..3, of the block of 16
__device__ __forceinline__ f32x4 xc_block(f32x4 w, f32x4 b, f32x4 acc) {
#pragma unroll
    for (int j = 0; j < 4; ++j) acc = xc_mma(w[j], b[j], acc);
    return acc;
}
__device__ __forceinline__ f32x4 xc_block(f16x8 w, f16x8 b, f32x4 acc) { return xc_mma(w, b, acc); }

// VEC: x and w are both read in 16-byte fragments; TILES: the filter tiles a wave keeps accumulators for (the host asks for no more than the
// filters need: O = 1 .. 16 is one tile).  Both are compile-time so that the block loop is straight-line code.
template <typename T, bool VEC, int TILES>
__global__ __launch_bounds__(XC_THREADS) void xcorr_dense_kernel(XcorrArgs a) {
    constexpr bool HALF = sizeof(T) == 2;
    constexpr int CH_BLOCK = HALF ? plan::kChanF16 : plan::kChanF32;   // channels of one block: a fragment of every lane group
    constexpr int CH_LANE = HALF ? 8 : 4;                              // ... of one lane's fragment

    const int tid = (int)threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int xl = lane & 15, g = lane >> 4;
    const int pix = (int)blockIdx.x * plan::kBlockPix + wave * plan::kWavePix + xl;
    const bool pix_live = pix < a.npix;
    const int oy = pix_live ? pix / a.wo : 0;
    const int ox = pix_live ? pix - oy * a.wo : 0;
    const int o0 = (int)blockIdx.y * plan::kTileOc * TILES;
    const int n = (int)blockIdx.z;

    const T* const xn = static_cast<const T*>(a.x) + n * a.x_sn;
    const T* const wb = static_cast<const T*>(a.w);
    int wo_[TILES];   // this lane's filter of tile t: its element offset, 0 (never dereferenced as live) beyond the filters
    bool wl[TILES];
    f32x4 acc[TILES];
#pragma unroll
    for (int t = 0; t < TILES; ++t) {
        const int o = o0 + plan::kTileOc * t + xl;
        wl[t] = o < a.oc;
        wo_[t] = wl[t] ? o * a.w_sn : 0;
        acc[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    }

    const int iy0 = oy * a.sh - a.pt, ix0 = ox * a.sw - a.pl;
    const int blocks = (a.c + CH_BLOCK - 1) / CH_BLOCK;
    const int cl0 = CH_LANE * g;
    for (int ky = 0; ky < a.kh; ++ky) {
        const int iy = iy0 + ky * a.dh;
        for (int kx = 0; kx < a.kw; ++kx) {
            const int ix = ix0 + kx * a.dw;
            const bool inb = pix_live && iy >= 0 && iy < a.h && ix >= 0 && ix < a.w_in;
            const int xoff = inb ? iy * a.x_sh + ix * a.x_sp : 0;
            const int woff = ky * a.w_sh + kx * a.w_sp;
            // two blocks per round, the fragments of both requested before the first MFMA (a run-time trip count is not unrolled for us)
            typedef decltype(xc_frag(xn, 0, 0, 1, 0, false, false)) Frag;
            int q = 0;
            for (; q + 2 <= blocks; q += 2) {
                Frag b[2], wfr[2][TILES];
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int c = CH_BLOCK * (q + u) + cl0;
                    const bool cl = c < a.c;
                    b[u] = xc_frag(xn, xoff, c, 1, a.c, inb && cl, VEC);
#pragma unroll
                    for (int t = 0; t < TILES; ++t) wfr[u][t] = xc_frag(wb, wo_[t] + woff, c, a.w_sc, a.c, wl[t] && cl, VEC);
                }
#pragma unroll
                for (int u = 0; u < 2; ++u)
#pragma unroll
                    for (int t = 0; t < TILES; ++t) acc[t] = xc_block(wfr[u][t], b[u], acc[t]);
            }
            if (q < blocks) {
                const int c = CH_BLOCK * q + cl0;
                const bool cl = c < a.c;
                const Frag b = xc_frag(xn, xoff, c, 1, a.c, inb && cl, VEC);
                Frag wfr[TILES];
#pragma unroll
                for (int t = 0; t < TILES; ++t) wfr[t] = xc_frag(wb, wo_[t] + woff, c, a.w_sc, a.c, wl[t] && cl, VEC);
#pragma unroll
                for (int t = 0; t < TILES; ++t) acc[t] = xc_block(wfr[t], b, acc[t]);
            }
        }
    }

    // epilogue: register r of accumulator t is filter o0 + 16 t + 4 g + r at this lane's pixel
    if (!pix_live) return;
    T* const yp = static_cast<T*>(a.y) + n * a.y_sn + oy * a.y_sh + ox * a.y_sp;
#pragma unroll
    for (int t = 0; t < TILES; ++t) {
        const int ob = o0 + plan::kTileOc * t + 4 * g;
        if (ob >= a.oc) continue;
        T out[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float bv = (a.bias && ob + r < a.oc) ? a.bias[ob + r] : 0.0f;
            out[r] = si_store_cast<T>(si_act(a.act, acc[t][r] + bv, a.act_param));
        }
        if (a.y_vec && ob + 3 < a.oc) {
            typedef T V4 __attribute__((ext_vector_type(4)));
            *reinterpret_cast<V4*>(yp + ob) = V4{out[0], out[1], out[2], out[3]};
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (ob + r < a.oc) yp[ob + r] = out[r];
        }
    }
}

template <typename T>
__global__ __launch_bounds__(XC_THREADS) void xcorr_depthwise_kernel(XcorrArgs a) {
    constexpr int R = 16 / (int)sizeof(T);   // channels of an item: 16 bytes of the storage type
    typedef T VR __attribute__((ext_vector_type(R)));
    const unsigned item = blockIdx.x * (unsigned)XC_THREADS + threadIdx.x;
    if (item >= (unsigned)a.npix * (unsigned)a.runs) return;
    const int pix = (int)(item / (unsigned)a.runs);
    const int c0 = ((int)item - pix * a.runs) * R;
    const int oy = pix / a.wo, ox = pix - oy * a.wo;
    const int n = (int)blockIdx.z;
    const int live = min(R, a.c - c0);
    const bool whole = live == R;
    const bool xv = a.x_vec && whole, wv = a.w_vec && whole, yv = a.y_vec && whole;

    const T* const xn = static_cast<const T*>(a.x) + n * a.x_sn + c0;
    const T* const wn = static_cast<const T*>(a.w) + n * a.w_sn + c0 * a.w_sc;
    float acc[R];
#pragma unroll
    for (int j = 0; j < R; ++j) acc[j] = 0.0f;

    const int iy0 = oy * a.sh - a.pt, ix0 = ox * a.sw - a.pl;
    for (int ky = 0; ky < a.kh; ++ky) {
        const int iy = iy0 + ky * a.dh;
        if (iy < 0 || iy >= a.h) continue;
        for (int kx = 0; kx < a.kw; ++kx) {
            const int ix = ix0 + kx * a.dw;
            if (ix < 0 || ix >= a.w_in) continue;
            const T* const xp = xn + iy * a.x_sh + ix * a.x_sp;
            const T* const wp = wn + ky * a.w_sh + kx * a.w_sp;
            float xf[R], wfl[R];
            if (xv) {
                const VR v = *reinterpret_cast<const VR*>(xp);
#pragma unroll
                for (int j = 0; j < R; ++j) xf[j] = (float)v[j];
            } else {
#pragma unroll
                for (int j = 0; j < R; ++j) xf[j] = j < live ? (float)xp[j] : 0.0f;
            }
            if (wv) {
                const VR v = *reinterpret_cast<const VR*>(wp);
#pragma unroll
                for (int j = 0; j < R; ++j) wfl[j] = (float)v[j];
            } else {
#pragma unroll
                for (int j = 0; j < R; ++j) wfl[j] = j < live ? (float)wp[j * a.w_sc] : 0.0f;
            }
#pragma unroll
            for (int j = 0; j < R; ++j) acc[j] = fmaf(xf[j], wfl[j], acc[j]);
        }
    }

    T out[R];
#pragma unroll
    for (int j = 0; j < R; ++j) {
        const float bv = (a.bias && j < live) ? a.bias[c0 + j] : 0.0f;
        out[j] = si_store_cast<T>(si_act(a.act, acc[j] + bv, a.act_param));
    }
    T* const yp = static_cast<T*>(a.y) + n * a.y_sn + oy * a.y_sh + ox * a.y_sp + c0;
    if (yv) {
        VR v;
#pragma unroll
        for (int j = 0; j < R; ++j) v[j] = out[j];
        *reinterpret_cast<VR*>(yp) = v;
    } else {
#pragma unroll
        for (int j = 0; j < R; ++j)
            if (j < live) yp[j] = out[j];
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------
plan::Shape shape_of(const SiXcorrDesc* d) {
    plan::Shape s;
    s.n = d->n; s.h = d->h; s.w = d->w; s.c = d->c; s.oc = d->oc; s.ho = d->ho; s.wo = d->wo; s.kh = d->kh; s.kw = d->kw;
    s.stride_h = d->stride_h; s.stride_w = d->stride_w; s.dilation_h = d->dilation_h; s.dilation_w = d->dilation_w;
    s.pad_top = d->pad_top; s.pad_left = d->pad_left; s.groups = d->groups;
    s.per_sample = d->per_sample != 0 ? 1 : 0;
    return s;
}

// the filter view's extent: dense [oc][kh][kw][c]; depthwise [kh][kw][c], per-sample [n][kh][kw][c] with the image stride w_sn
uint64_t filter_extent(const SiXcorrDesc* d, plan::Form form) {
    const int lead = form == plan::kDense ? d->oc : d->per_sample ? d->n : 1;
    return plan::ViewExtent(lead, d->kh, d->kw, d->c, d->w_sn, d->w_sh, d->w_sp, d->w_sc);
}

// everything that can be decided without a device and without the pointers: SI_E_BADARG / SI_E_UNSUPPORTED / 0
int check_desc(const SiXcorrDesc* d, bool half) {
    if (!d) return SI_E_BADARG;
    const plan::Shape s = shape_of(d);
    if (!plan::Positive(s)) return SI_E_BADARG;
    if (!plan::ExtentsOk(s)) return SI_E_BADARG;
    if (d->x_sn < 0 || d->x_sh < 0 || d->x_sp < 0 || d->w_sn < 0 || d->w_sh < 0 || d->w_sp < 0 || d->w_sc < 0) return SI_E_BADARG;
    if (!plan::NestedStrides(d->n, d->ho, d->wo, d->oc, d->y_sn, d->y_sh, d->y_sp)) return SI_E_BADARG;
    const plan::Form form = plan::FormOf(s);
    if (form == plan::kNone) return SI_E_UNSUPPORTED;
    if (half && !plan::HalfOk(s)) return SI_E_UNSUPPORTED;
    if (plan::ViewExtent(d->n, d->h, d->w, d->c, d->x_sn, d->x_sh, d->x_sp, 1) == 0) return SI_E_UNSUPPORTED;
    if (plan::ViewExtent(d->n, d->ho, d->wo, d->oc, d->y_sn, d->y_sh, d->y_sp, 1) == 0) return SI_E_UNSUPPORTED;
    if (filter_extent(d, form) == 0) return SI_E_UNSUPPORTED;
    plan::Grid grid;
    if (!plan::MakeGrid(s, half, grid) || !plan::PositionsFit(s)) return SI_E_UNSUPPORTED;
    return 0;
}

int check_ptrs(const SiXcorrDesc* d, const void* x, const void* w, const float* bias, const void* y, bool half) {
    if (!x || !w || !y) return SI_E_BADARG;
    const uint64_t es = half ? 2 : 4;
    const uint64_t y_bytes = plan::ViewExtent(d->n, d->ho, d->wo, d->oc, d->y_sn, d->y_sh, d->y_sp, 1) * es;
    const uint64_t x_bytes = plan::ViewExtent(d->n, d->h, d->w, d->c, d->x_sn, d->x_sh, d->x_sp, 1) * es;
    if (si_ranges_overlap(y, y_bytes, x, x_bytes)) return SI_E_BADARG;
    if (si_ranges_overlap(y, y_bytes, w, filter_extent(d, plan::FormOf(shape_of(d))) * es)) return SI_E_BADARG;
    if (bias && si_ranges_overlap(y, y_bytes, bias, (uint64_t)d->oc * 4)) return SI_E_BADARG;
    if (!si_aligned_to(x, es) || !si_aligned_to(y, es) || !si_aligned_to(w, es) || (bias && !si_aligned_to(bias, 4))) return SI_E_UNSUPPORTED;
    return 0;
}

// do the start and the strides of a view keep every access of `elems` consecutive elements aligned to elems * es bytes?
bool vector_view(const void* p, size_t es, int elems, long long s0, long long s1, long long s2) {
    return si_aligned_to(p, es * elems) && s0 % elems == 0 && s1 % elems == 0 && s2 % elems == 0;
}

template <typename T, bool VEC>
void launch_dense_tiles(int tiles, dim3 grid, hipStream_t st, const XcorrArgs& a) {
    switch (tiles) {
        case 1: hipLaunchKernelGGL((xcorr_dense_kernel<T, VEC, 1>), grid, dim3(XC_THREADS), 0, st, a); break;
        case 2: hipLaunchKernelGGL((xcorr_dense_kernel<T, VEC, 2>), grid, dim3(XC_THREADS), 0, st, a); break;
        case 3: hipLaunchKernelGGL((xcorr_dense_kernel<T, VEC, 3>), grid, dim3(XC_THREADS), 0, st, a); break;
        default: hipLaunchKernelGGL((xcorr_dense_kernel<T, VEC, plan::kWaveTiles>), grid, dim3(XC_THREADS), 0, st, a); break;
    }
}

template <typename T>
void launch_dense(bool vec, int tiles, dim3 grid, hipStream_t st, const XcorrArgs& a) {
    if (vec) launch_dense_tiles<T, true>(tiles, grid, st, a);
    else launch_dense_tiles<T, false>(tiles, grid, st, a);
}

template <typename T>
int run(const SiXcorrDesc* d, const void* x, const void* w, const float* bias, void* y, si_stream_t stream) {
    constexpr bool half = sizeof(T) == 2;
    int rc = check_desc(d, half);
    if (rc != 0) return rc;
    rc = check_ptrs(d, x, w, bias, y, half);
    if (rc != 0) return rc;
    const plan::Shape s = shape_of(d);
    const plan::Form form = plan::FormOf(s);
    plan::Grid grid;
    plan::MakeGrid(s, half, grid);
    XcorrArgs a;
    memset(&a, 0, sizeof(a));
    a.x = x; a.w = w; a.bias = bias; a.y = y;
    a.h = d->h; a.w_in = d->w; a.c = d->c; a.oc = d->oc; a.ho = d->ho; a.wo = d->wo; a.kh = d->kh; a.kw = d->kw;
    a.sh = d->stride_h; a.sw = d->stride_w; a.dh = d->dilation_h; a.dw = d->dilation_w; a.pt = d->pad_top; a.pl = d->pad_left;
    a.npix = (int)plan::OutPixels(s);
    a.runs = plan::DwChanRuns(s, half);
    a.x_sn = (int)d->x_sn; a.x_sh = (int)d->x_sh; a.x_sp = (int)d->x_sp;
    a.w_sn = (form == plan::kDense || d->per_sample) ? (int)d->w_sn : 0;   // (depthwise with shared filters: no image stride)
    a.w_sh = (int)d->w_sh; a.w_sp = (int)d->w_sp; a.w_sc = (int)d->w_sc;
    a.y_sn = (int)d->y_sn; a.y_sh = (int)d->y_sh; a.y_sp = (int)d->y_sp;
    a.act = d->act; a.act_param = d->act_param;
    hipStream_t st = (hipStream_t)stream;
    const dim3 g3(grid.x, grid.y, grid.z);
    if (form == plan::kDepthwise) {
        const int r = plan::DwRun(half);
        a.x_vec = vector_view(x, sizeof(T), r, d->x_sn, d->x_sh, d->x_sp) ? 1 : 0;
        a.w_vec = (d->w_sc == 1 && vector_view(w, sizeof(T), r, a.w_sn, d->w_sh, d->w_sp)) ? 1 : 0;
        a.y_vec = vector_view(y, sizeof(T), r, d->y_sn, d->y_sh, d->y_sp) ? 1 : 0;
        hipLaunchKernelGGL((xcorr_depthwise_kernel<T>), g3, dim3(XC_THREADS), 0, st, a);
    } else {
        // a fragment is 16 bytes of consecutive channels (4 floats / 8 halves): one read where the view allows it
        const int r = half ? 8 : 4;
        a.x_vec = (d->c % r == 0 && vector_view(x, sizeof(T), r, d->x_sn, d->x_sh, d->x_sp)) ? 1 : 0;
        a.w_vec = (d->c % r == 0 && d->w_sc == 1 && vector_view(w, sizeof(T), r, d->w_sn, d->w_sh, d->w_sp)) ? 1 : 0;
        a.y_vec = vector_view(y, sizeof(T), 4, d->y_sn, d->y_sh, d->y_sp) ? 1 : 0;
        launch_dense<T>(a.x_vec && a.w_vec, plan::WaveTiles(s), g3, st, a);
    }
    SI_HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" {

int si_hip_xcorr_f32(const SiXcorrDesc* d, const float* x, const float* w, const float* bias, float* y, si_stream_t stream) {
    return run<float>(d, x, w, bias, y, stream);
}

int si_hip_xcorr_f16(const SiXcorrDesc* d, const void* x, const void* w, const float* bias, void* y, si_stream_t stream) {
    return run<_Float16>(d, x, w, bias, y, stream);
}

const char* si_hip_xcorr_kernel_name(const SiXcorrDesc* d, const void* x, const void* w, const void* y, int half) {
    if (check_desc(d, half != 0) != 0 || !x || !w || !y) return "none";
    const size_t es = half ? 2 : 4;
    if (!si_aligned_to(x, es) || !si_aligned_to(w, es) || !si_aligned_to(y, es)) return "none";
    static const char* const names[2][2] = {{"xcorr_dense_kernel<float>", "xcorr_depthwise_kernel<float>"},
                                            {"xcorr_dense_kernel<_Float16>", "xcorr_depthwise_kernel<_Float16>"}};
    return names[half ? 1 : 0][plan::FormOf(shape_of(d)) == plan::kDepthwise ? 1 : 0];
}

}  // extern "C"
