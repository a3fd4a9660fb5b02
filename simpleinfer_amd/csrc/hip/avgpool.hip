// avgpool.hip -- the window means (include/si_pool.h): nn.AvgPool2d / F.avg_pool2d and the general case of nn.AdaptiveAvgPool2d on NHWC
// fp32 and fp16 tensors with pixel strides on both sides.  Rule, accepted set and the arithmetic contract: the header.
//
// Windowed form (largest window below SI_AVGPOOL_COOP_TAPS taps): one lane per item, an item being one channel vector of one output pixel
// (16 bytes, or one element in the scalar form).  Consecutive lanes take consecutive channel vectors of a pixel, then consecutive pixels
// (the layout of pad2d.hip): a wave reads whole runs of an input row.  blockIdx = (items of the image, image).  A lane maps its item once
// (two 32-bit divisions), computes its window and divisor once and adds the taps row by row, left to right, from +0.0f.
//
// Cooperative form (larger windows): a workgroup of 256 threads owns one output pixel and CW consecutive channel vectors; thread =
// (group g, lane), lane -> channel vector (a tap's CW vectors are one contiguous run), the G = 256 / CW groups stride over the window's
// taps in row-major order.  Partials meet in LDS as [g][lane] and lane's owner (g == 0) adds them in the order g = 0 .. G - 1: the order
// of every addition is a function of the window's extents and of G, which the vector width fixes.  blockIdx = (output pixel, channel
// chunk, image).
//
// Element offsets are 32-bit: the host refuses tensors whose offsets do not fit 31 bits.  Register table per instantiation: DESIGN.md 9e.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "si_hip_internal.h"
#include "si_pool.h"

#pragma clang fp contract(off)

namespace {

constexpr int AP_THREADS = 256;

struct AvgArgs {
    const void* in;
    void* out;
    int ih, iw, oh, ow;
    int cv;            // items (channel vectors) per pixel
    int in_ld, out_ld;
    int kh, kw, sh, sw, pt, pl;
    int adaptive, count_include_pad, divisor_override;
    int items;         // oh * ow * cv (windowed form)
};

// one axis: output j of size-i input -> clipped window [lo, hi) and the padded extent
struct AxisWin { int lo, hi, padded; };

__device__ __forceinline__ AxisWin axis_window(int j, int i, int o, int k, int s, int p, int adaptive) {
    AxisWin w;
    if (adaptive) {
        w.lo = (j * i) / o;
        w.hi = ((j + 1) * i + o - 1) / o;
        w.padded = w.hi - w.lo;
    } else {
        const int a = j * s - p;
        const int b = min(a + k, i + p);
        w.padded = b - a;
        w.lo = max(a, 0);
        w.hi = min(b, i);
    }
    return w;
}

__device__ __forceinline__ float window_divisor(const AvgArgs& a, const AxisWin& y, const AxisWin& x) {
    if (a.divisor_override != 0) return (float)a.divisor_override;
    if (a.count_include_pad && !a.adaptive) return (float)(y.padded * x.padded);
    return (float)((y.hi - y.lo) * (x.hi - x.lo));
}

// an item of VW elements of T in memory, widened to float lanes
template <typename T, int VW> struct Item;
template <> struct Item<float, 4> {
    static __device__ __forceinline__ void add(float (&acc)[4], const float* p) {
        const f32x4 w = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] += w[e];
    }
    static __device__ __forceinline__ void store(float* p, const float (&v)[4]) {
        f32x4 w;
#pragma unroll
        for (int e = 0; e < 4; ++e) w[e] = v[e];
        *reinterpret_cast<f32x4*>(p) = w;
    }
};
template <> struct Item<float, 1> {
    static __device__ __forceinline__ void add(float (&acc)[1], const float* p) { acc[0] += *p; }
    static __device__ __forceinline__ void store(float* p, const float (&v)[1]) { *p = v[0]; }
};
template <> struct Item<_Float16, 8> {
    static __device__ __forceinline__ void add(float (&acc)[8], const _Float16* p) {
        const f16x8 w = *reinterpret_cast<const f16x8*>(p);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] += (float)w[e];
    }
    static __device__ __forceinline__ void store(_Float16* p, const float (&v)[8]) {
        f16x8 w;
#pragma unroll
        for (int e = 0; e < 8; ++e) w[e] = si_store_cast<_Float16>(v[e]);
        *reinterpret_cast<f16x8*>(p) = w;
    }
};
template <> struct Item<_Float16, 1> {
    static __device__ __forceinline__ void add(float (&acc)[1], const _Float16* p) { acc[0] += (float)*p; }
    static __device__ __forceinline__ void store(_Float16* p, const float (&v)[1]) { *p = si_store_cast<_Float16>(v[0]); }
};

template <typename T, int VW>
__global__ __launch_bounds__(AP_THREADS) void avgpool2d_window_kernel(AvgArgs a) {
    const int item = (int)blockIdx.x * AP_THREADS + (int)threadIdx.x;
    if (item >= a.items) return;
    const int pix = item / a.cv;
    const int v = item - pix * a.cv;
    const int oy = pix / a.ow;
    const int ox = pix - oy * a.ow;
    const int img = (int)blockIdx.y;
    const AxisWin wy = axis_window(oy, a.ih, a.oh, a.kh, a.sh, a.pt, a.adaptive);
    const AxisWin wx = axis_window(ox, a.iw, a.ow, a.kw, a.sw, a.pl, a.adaptive);
    const float div = window_divisor(a, wy, wx);
    const T* const in = static_cast<const T*>(a.in) + v * VW;
    float acc[VW];
#pragma unroll
    for (int e = 0; e < VW; ++e) acc[e] = 0.0f;
    for (int y = wy.lo; y < wy.hi; ++y) {
        const T* row = in + ((img * a.ih + y) * a.iw + wx.lo) * a.in_ld;
#pragma unroll 4
        for (int x = wx.lo; x < wx.hi; ++x, row += a.in_ld) Item<T, VW>::add(acc, row);
    }
#pragma unroll
    for (int e = 0; e < VW; ++e) acc[e] = acc[e] / div;
    Item<T, VW>::store(static_cast<T*>(a.out) + ((img * a.oh + oy) * a.ow + ox) * a.out_ld + v * VW, acc);
}

// lanes per tap (channel vectors of one chunk) by vector width: 16 x 16 bytes of floats, 8 x 16 bytes of halves, 64 single elements
template <typename T, int VW> struct CoopShape { static constexpr int CW = 64; };
template <> struct CoopShape<float, 4> { static constexpr int CW = 16; };
template <> struct CoopShape<_Float16, 8> { static constexpr int CW = 8; };

template <typename T, int VW>
__global__ __launch_bounds__(AP_THREADS) void avgpool2d_coop_kernel(AvgArgs a) {
    constexpr int CW = CoopShape<T, VW>::CW;
    constexpr int G = AP_THREADS / CW;
    __shared__ float part[G][CW][VW];
    const int lane = (int)threadIdx.x % CW;
    const int g = (int)threadIdx.x / CW;
    const int pix = (int)blockIdx.x;
    const int oy = pix / a.ow;
    const int ox = pix - oy * a.ow;
    const int v = (int)blockIdx.y * CW + lane;
    const int img = (int)blockIdx.z;
    const AxisWin wy = axis_window(oy, a.ih, a.oh, a.kh, a.sh, a.pt, a.adaptive);
    const AxisWin wx = axis_window(ox, a.iw, a.ow, a.kw, a.sw, a.pl, a.adaptive);
    const int ww = max(wx.hi - wx.lo, 1);   // (never empty on the accepted set; the divisions below stay defined whatever happens)
    const int taps = max(wy.hi - wy.lo, 0) * max(wx.hi - wx.lo, 0);
    float acc[VW];
#pragma unroll
    for (int e = 0; e < VW; ++e) acc[e] = 0.0f;
    if (v < a.cv) {
        const T* const in = static_cast<const T*>(a.in) + ((img * a.ih + wy.lo) * a.iw + wx.lo) * a.in_ld + v * VW;
        // tap t = ty * ww + tx; a group steps G taps: (dy, dx) rows and columns, one carry
        const int dy = G / ww, dx = G - dy * ww;
        int ty = g / ww, tx = g - ty * ww;
        for (int t = g; t < taps; t += G) {
            Item<T, VW>::add(acc, in + (ty * a.iw + tx) * a.in_ld);
            ty += dy;
            tx += dx;
            if (tx >= ww) {
                tx -= ww;
                ++ty;
            }
        }
    }
#pragma unroll
    for (int e = 0; e < VW; ++e) part[g][lane][e] = acc[e];
    __syncthreads();
    if (g == 0 && v < a.cv) {
        const float div = window_divisor(a, wy, wx);
        float sum[VW];
#pragma unroll
        for (int e = 0; e < VW; ++e) sum[e] = part[0][lane][e];
        for (int k = 1; k < G; ++k) {
#pragma unroll
            for (int e = 0; e < VW; ++e) sum[e] += part[k][lane][e];
        }
#pragma unroll
        for (int e = 0; e < VW; ++e) sum[e] = sum[e] / div;
        Item<T, VW>::store(static_cast<T*>(a.out) + ((img * a.oh + oy) * a.ow + ox) * a.out_ld + v * VW, sum);
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------
// the rule's output size with either rounding; 0: `o` is neither
bool out_size_ok(int64_t i, int64_t k, int64_t s, int64_t p, int64_t o) {
    const int64_t span = i + 2 * p - k;
    if (span < 0) return false;
    const int64_t fl = span / s + 1;
    int64_t ce = (span + s - 1) / s + 1;
    if ((ce - 1) * s >= i + p) --ce;
    return o == fl || o == ce;
}

// the largest clipped extent of an axis over its o windows, in closed form.
// windowed: f(a) = min(a + k, i) - max(a, 0) with a = j s - p rises up to a = 0 and does not rise after it: the largest value is at
// one of the two windows around a = 0.  adaptive: i = q o + r; every window has q taps (r = 0), q + 1 or q + 2, and q + 2 occurs iff r does
// not divide o.
int64_t max_extent(int64_t i, int64_t o, int64_t k, int64_t s, int64_t p, bool adaptive) {
    if (adaptive) {
        const int64_t q = i / o, r = i % o;
        return q + (r == 0 ? 0 : (o % r == 0 ? 1 : 2));
    }
    int64_t best = 0;
    for (int64_t jj = p / s; jj <= p / s + 1; ++jj) {
        const int64_t j = jj < o ? jj : o - 1;   // (fewer windows than that: the last one is the nearest)
        const int64_t a = j * s - p;
        const int64_t b = (a + k < i + p ? a + k : i + p);
        const int64_t ext = (b < i ? b : i) - (a > 0 ? a : 0);
        if (ext > best) best = ext;
    }
    return best;
}

// everything that can be decided without a device: SI_E_BADARG / SI_E_UNSUPPORTED / 0
int check_desc(const SiAvgPool2dDesc* d) {
    if (!d) return SI_E_BADARG;
    if (d->n <= 0 || d->ih <= 0 || d->iw <= 0 || d->c <= 0 || d->oh <= 0 || d->ow <= 0) return SI_E_BADARG;
    if (d->in_ld < d->c || d->out_ld < d->c) return SI_E_BADARG;
    if (!d->adaptive) {
        if (d->kh < 1 || d->kw < 1 || d->sh < 1 || d->sw < 1 || d->pt < 0 || d->pl < 0) return SI_E_BADARG;
        if (d->pt > d->kh / 2 || d->pl > d->kw / 2) return SI_E_UNSUPPORTED;
        if (!out_size_ok(d->ih, d->kh, d->sh, d->pt, d->oh) || !out_size_ok(d->iw, d->kw, d->sw, d->pl, d->ow)) return SI_E_BADARG;
    } else {
        // (j + 1) * i + o - 1 is computed in 32 bits on the device
        if ((uint64_t)d->ih * d->oh + (uint64_t)d->oh > SI_INDEX_LIMIT || (uint64_t)d->iw * d->ow + (uint64_t)d->ow > SI_INDEX_LIMIT) return SI_E_UNSUPPORTED;
    }
    if (d->n > 65535) return SI_E_UNSUPPORTED;
    const uint64_t in_rows = (uint64_t)d->n * d->ih, out_rows = (uint64_t)d->n * d->oh;   // < 2^47
    if (in_rows > SI_INDEX_LIMIT || out_rows > SI_INDEX_LIMIT) return SI_E_UNSUPPORTED;
    const uint64_t in_pix = in_rows * d->iw, out_pix = out_rows * d->ow;                    // < 2^62
    if (in_pix > SI_INDEX_LIMIT || out_pix > SI_INDEX_LIMIT) return SI_E_UNSUPPORTED;
    if (in_pix * (uint64_t)d->in_ld > SI_INDEX_LIMIT || out_pix * (uint64_t)d->out_ld > SI_INDEX_LIMIT) return SI_E_UNSUPPORTED;
    // the windowed form's item count and the cooperative form's chunk count (c <= ld: both fit once the offsets do)
    if ((uint64_t)d->oh * d->ow * (uint64_t)d->c > SI_INDEX_LIMIT) return SI_E_UNSUPPORTED;
    return 0;
}

// the tap count of the launch's largest window decides the form: a function of the shape, never of n
bool cooperative(const SiAvgPool2dDesc* d) {
    const int64_t taps = max_extent(d->ih, d->oh, d->kh, d->sh, d->pt, d->adaptive != 0) * max_extent(d->iw, d->ow, d->kw, d->sw, d->pl, d->adaptive != 0);
    return taps >= (int64_t)SI_ENV_INT("SI_AVGPOOL_COOP_TAPS", SI_AVGPOOL_COOP_TAPS);
}

template <typename T>
int vector_width(const SiAvgPool2dDesc* d, const void* in, const void* out) { return si_vector_width<T>(d->c, d->in_ld, d->out_ld, in, out); }

template <typename T, int VW>
int launch(const SiAvgPool2dDesc* d, const T* in, T* out, hipStream_t stream) {
    AvgArgs a;
    a.in = in;
    a.out = out;
    a.ih = d->ih; a.iw = d->iw; a.oh = d->oh; a.ow = d->ow;
    a.cv = d->c / VW;
    a.in_ld = d->in_ld;
    a.out_ld = d->out_ld;
    a.kh = d->kh; a.kw = d->kw; a.sh = d->sh; a.sw = d->sw; a.pt = d->pt; a.pl = d->pl;
    a.adaptive = d->adaptive ? 1 : 0;
    a.count_include_pad = d->count_include_pad ? 1 : 0;
    a.divisor_override = d->divisor_override;
    a.items = d->oh * d->ow * a.cv;
    if (cooperative(d)) {
        constexpr int CW = CoopShape<T, VW>::CW;
        const unsigned chunks = ((unsigned)a.cv + CW - 1) / CW;
        if (chunks > 65535u) return SI_E_UNSUPPORTED;
        const dim3 grid((unsigned)(d->oh * d->ow), chunks, (unsigned)d->n);
        hipLaunchKernelGGL((avgpool2d_coop_kernel<T, VW>), grid, dim3(AP_THREADS), 0, stream, a);
    } else {
        const dim3 grid(((unsigned)a.items + AP_THREADS - 1) / AP_THREADS, (unsigned)d->n);
        hipLaunchKernelGGL((avgpool2d_window_kernel<T, VW>), grid, dim3(AP_THREADS), 0, stream, a);
    }
    return (int)hipGetLastError();
}

template <typename T>
int run(const SiAvgPool2dDesc* d, const T* in, T* out, si_stream_t stream) {
    const int rc = check_desc(d);
    if (rc != 0) return rc;
    if (!in || !out) return SI_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    constexpr int full = (int)(16 / sizeof(T));
    return vector_width<T>(d, in, out) == full ? launch<T, full>(d, in, out, s) : launch<T, 1>(d, in, out, s);
}

}  // namespace

extern "C" {

int si_hip_avgpool2d_f32(const SiAvgPool2dDesc* d, const float* in, float* out, si_stream_t stream) { return run<float>(d, in, out, stream); }

int si_hip_avgpool2d_f16(const SiAvgPool2dDesc* d, const void* in, void* out, si_stream_t stream) {
    return run<_Float16>(d, static_cast<const _Float16*>(in), static_cast<_Float16*>(out), stream);
}

const char* si_hip_avgpool2d_kernel_name(const SiAvgPool2dDesc* d, const void* in, const void* out, int half) {
    if (check_desc(d) != 0) return "none";
    const bool vec = (half ? vector_width<_Float16>(d, in, out) : vector_width<float>(d, in, out)) > 1;
    if (cooperative(d)) {
        if (half) return vec ? "avgpool2d_coop_kernel<_Float16, 8>" : "avgpool2d_coop_kernel<_Float16, 1>";
        return vec ? "avgpool2d_coop_kernel<float, 4>" : "avgpool2d_coop_kernel<float, 1>";
    }
    if (half) return vec ? "avgpool2d_window_kernel<_Float16, 8>" : "avgpool2d_window_kernel<_Float16, 1>";
    return vec ? "avgpool2d_window_kernel<float, 4>" : "avgpool2d_window_kernel<float, 1>";
}

}  // extern "C"
