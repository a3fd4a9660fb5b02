// roi_align.hip -- torchvision.ops.RoIAlign / roi_align on NHWC fp32 and fp16 feature maps with fp32 boxes (include/si_roi.h).  The
// semantics of torchvision's CPU kernel; no reference counterpart.
//
// The rule (include/si_roi.h states it in full; this file is compiled with contraction off, so the vector arms and both storage types
// produce the same bits):
//     per roi       sw = x1 * scale - o ... ; rw = ew - sw (fmaxf(rw, 1) without `aligned`); bw = rw / pw; gw = ratio > 0 ? ratio : ceilf(rw / pw)
//     per sample    x = sw + j * bw + (ix + 0.5f) * bw / gw; outside [-1, w]: nothing; fmaxf(x, 0); xl = (int)x, clamped at w - 1; lx, hx = 1 - lx
//     accumulate    acc = acc + (((w1 * v1 + w2 * v2) + w3 * v3) + w4 * v4), iy outer, ix inner;  result acc / count, one rounding at the store
//     invalid roi   NaN in every element, nothing read
// What decides a loop length or a conversion to int is in roi_interval.h, shared with a CPU test program: the count of samples is clamped in
// float, and each axis loop runs over the interval of indices whose samples can lie in [-1, size] -- at most 2 size + 8 trips per axis and
// bin whatever the box holds.
//
// Shape: a gather bound by HBM / L2.  A lane owns ONE channel vector of one output bin (r, i, j); channel vectors run fastest across lanes,
// so a wave reads each tap as one contiguous stretch and the lanes of a bin share the roi's five floats (ordinary loads: the lanes of a bin
// hit the same line).  The four taps' loads of a sample are issued before the first is used.  The grid (si_grid_for) is capped and strides
// over the items, one consecutive run per XCD.  32-bit index arithmetic: the host refuses what does not fit 31 bits.  No LDS, no scratch,
// no atomics, no workspace.
//
// -Rpass-analysis=kernel-resource-usage (gfx950, -O3), all six instantiations: scratch 0, LDS 0.  VGPRs:
//     roi_align_kernel<float, 4> 68    <float, 1> 56    <_Float16, 8> 86    <_Float16, 4> 70    <_Float16, 2> 60    <_Float16, 1> 55
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "si_hip_internal.h"
#include "si_roi.h"

// no implicit contraction anywhere in this file: the rule has no fused multiply-add
#pragma clang fp contract(off)

#include "roi_interval.h"

namespace {

template <typename T, int VW> struct VecOf;
template <> struct VecOf<float, 4> { typedef f32x4 type; };
template <> struct VecOf<float, 1> { typedef float type; };
template <> struct VecOf<_Float16, 8> { typedef f16x8 type; };
template <> struct VecOf<_Float16, 4> { typedef f16x4 type; };
template <> struct VecOf<_Float16, 2> { typedef f16x2 type; };
template <> struct VecOf<_Float16, 1> { typedef _Float16 type; };

constexpr int ROI_THREADS = 256;

struct RoiArgs {
    const void* x;
    const float* rois;
    void* out;
    int n, h, w, ph, pw;
    int cv;             // channel vectors per pixel
    int in_ld, out_ld, rois_ld;
    int ratio, aligned;
    float scale;
    unsigned items;     // k ph pw cv
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

// the two taps and weights of an inside coordinate on an axis of `size`
__device__ __forceinline__ void axis_taps(float y, int size, int& lo, int& hi, float& l, float& h) {
    y = fmaxf(y, 0.0f);
    lo = (int)y;   // (y is in [0, size] here, size <= 2^24)
    if (lo >= size - 1) {
        lo = hi = size - 1;
        y = (float)lo;
    } else {
        hi = lo + 1;
    }
    l = y - (float)lo;
    h = 1.0f - l;
}

// The workgroups that share an XCD take one consecutive run of the pass's items (grid_sample.hip: neighbouring bins share taps, and the
// run's source rows then stay in that XCD's L2).  A bijection of [0, nwg) for every nwg; nothing depends on how workgroups are dealt.
__device__ __forceinline__ unsigned xcd_block(unsigned orig, unsigned nwg) {
    const unsigned q = nwg >> 3, r = nwg & 7u, x = orig & 7u;
    return (x < r ? x * (q + 1u) : r * (q + 1u) + (x - r) * q) + (orig >> 3);
}

template <typename T, int VW>
__global__ __launch_bounds__(ROI_THREADS) void roi_align_kernel(const RoiArgs a) {
    const T* const x = static_cast<const T*>(a.x);
    T* const out = static_cast<T*>(a.out);
    const unsigned cv = (unsigned)a.cv, pw = (unsigned)a.pw, ph = (unsigned)a.ph;
    for (unsigned item = xcd_block(blockIdx.x, gridDim.x) * ROI_THREADS + threadIdx.x; item < a.items; item += gridDim.x * ROI_THREADS) {
        const unsigned bin = item / cv;
        const unsigned ch = (item - bin * cv) * VW;
        const unsigned row = bin / pw;
        const unsigned j = bin - row * pw;
        const unsigned r = row / ph;
        const unsigned i = row - r * ph;
        const float* const rp = a.rois + r * (unsigned)a.rois_ld;
        const float roi[5] = {rp[0], rp[1], rp[2], rp[3], rp[4]};
        const SiRoiBox b = si_roi_setup(roi, a.n, a.ph, a.pw, a.scale, a.ratio, a.aligned);
        T* const o = out + bin * (unsigned)a.out_ld + ch;
        float acc[VW];
        if (!b.valid) {
#pragma unroll
            for (int e = 0; e < VW; ++e) acc[e] = __builtin_nanf("");
            store_vec<T, VW>(o, acc);
            continue;
        }
#pragma unroll
        for (int e = 0; e < VW; ++e) acc[e] = 0.0f;
        const T* const xi = x + (unsigned)b.img * (unsigned)(a.h * a.w) * (unsigned)a.in_ld + ch;
        int ylo, yhi, xlo, xhi;
        si_roi_axis_interval(b.sh, b.bh, (int)i, b.gh, b.ghf, a.h, ylo, yhi);
        si_roi_axis_interval(b.sw, b.bw, (int)j, b.gw, b.gwf, a.w, xlo, xhi);
        for (int iy = ylo; iy < yhi; ++iy) {
            const float y = si_roi_sample(b.sh, b.bh, (int)i, iy, b.ghf);
            if (si_roi_outside(y, a.h)) continue;
            int yl, yh;
            float ly, hy;
            axis_taps(y, a.h, yl, yh, ly, hy);
            const T* const row_l = xi + (unsigned)(yl * a.w) * (unsigned)a.in_ld;
            const T* const row_h = xi + (unsigned)(yh * a.w) * (unsigned)a.in_ld;
            for (int ix = xlo; ix < xhi; ++ix) {
                const float xx = si_roi_sample(b.sw, b.bw, (int)j, ix, b.gwf);
                if (si_roi_outside(xx, a.w)) continue;
                int xl, xh;
                float lx, hx;
                axis_taps(xx, a.w, xl, xh, lx, hx);
                const float w1 = hy * hx, w2 = hy * lx, w3 = ly * hx, w4 = ly * lx;
                float v1[VW], v2[VW], v3[VW], v4[VW];
                load_vec<T, VW>(row_l + (unsigned)xl * (unsigned)a.in_ld, v1);
                load_vec<T, VW>(row_l + (unsigned)xh * (unsigned)a.in_ld, v2);
                load_vec<T, VW>(row_h + (unsigned)xl * (unsigned)a.in_ld, v3);
                load_vec<T, VW>(row_h + (unsigned)xh * (unsigned)a.in_ld, v4);
#pragma unroll
                for (int e = 0; e < VW; ++e) {
                    float t = w1 * v1[e];
                    t = t + w2 * v2[e];
                    t = t + w3 * v3[e];
                    t = t + w4 * v4[e];
                    acc[e] = acc[e] + t;
                }
            }
        }
#pragma unroll
        for (int e = 0; e < VW; ++e) acc[e] = __fdiv_rn(acc[e], b.count);
        store_vec<T, VW>(o, acc);
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------
constexpr int SIZE_LIMIT = 1 << 24;   // map sizes are used as floats: exact up to here

// the descriptor with its defaults filled in (a stride of 0 is dense)
SiRoiAlignDesc normalised(const SiRoiAlignDesc* d) {
    SiRoiAlignDesc r = *d;
    if (r.in_ld == 0) r.in_ld = r.c;
    if (r.out_ld == 0) r.out_ld = r.c;
    if (r.rois_ld == 0) r.rois_ld = 5;
    return r;
}

// everything that can be decided from the descriptor alone: SI_E_BADARG / SI_E_UNSUPPORTED / 0.  `d` is normalised.
int check_desc(const SiRoiAlignDesc& d) {
    if (d.n <= 0 || d.c <= 0 || d.h <= 0 || d.w <= 0 || d.k <= 0 || d.ph <= 0 || d.pw <= 0) return SI_E_BADARG;
    if (d.in_ld < d.c || d.out_ld < d.c || d.rois_ld < 5) return SI_E_BADARG;
    if (d.h > SIZE_LIMIT || d.w > SIZE_LIMIT || d.ph > SIZE_LIMIT || d.pw > SIZE_LIMIT) return SI_E_UNSUPPORTED;
    if (d.sampling_ratio > SI_ROI_RATIO_LIMIT) return SI_E_UNSUPPORTED;
    if (!si_view_extent(d.n, d.h, d.w, d.in_ld, d.c) || !si_view_extent(d.k, d.ph, d.pw, d.out_ld, d.c) || !si_view_extent(1, 1, d.k, d.rois_ld, 5))
        return SI_E_UNSUPPORTED;
    return 0;
}

int check_call(const SiRoiAlignDesc& d, const void* x, const void* rois, const void* out, size_t es) {
    const int rc = check_desc(d);
    if (rc != 0) return rc;
    if (!x || !rois || !out) return SI_E_BADARG;
    const uint64_t out_bytes = si_view_extent(d.k, d.ph, d.pw, d.out_ld, d.c) * es;
    if (si_ranges_overlap(out, out_bytes, x, si_view_extent(d.n, d.h, d.w, d.in_ld, d.c) * es) ||
        si_ranges_overlap(out, out_bytes, rois, si_view_extent(1, 1, d.k, d.rois_ld, 5) * sizeof(float)))
        return SI_E_BADARG;
    return 0;
}

// widest channel vector (in elements) that c, both strides and both base pointers allow
template <typename T>
int vec_width(const SiRoiAlignDesc& d, const void* x, const void* out) {
    const int widths[] = {(int)(16 / sizeof(T)), (int)(8 / sizeof(T)), (int)(4 / sizeof(T))};
    for (int w : widths) {
        if (w <= 1 || (sizeof(T) == 4 && w == 2)) continue;   // (fp32: 4 | 1)
        const size_t bytes = w * sizeof(T);
        if (d.c % w == 0 && d.in_ld % w == 0 && d.out_ld % w == 0 && si_aligned_to(x, bytes) && si_aligned_to(out, bytes)) return w;
    }
    return 1;
}

template <typename T, int VW>
int launch(const SiRoiAlignDesc& d, const void* x, const float* rois, void* out, hipStream_t stream) {
    RoiArgs a;
    a.x = x; a.rois = rois; a.out = out;
    a.n = d.n; a.h = d.h; a.w = d.w; a.ph = d.ph; a.pw = d.pw;
    a.cv = d.c / VW;
    a.in_ld = d.in_ld; a.out_ld = d.out_ld; a.rois_ld = d.rois_ld;
    a.ratio = d.sampling_ratio; a.aligned = d.aligned ? 1 : 0;
    a.scale = d.spatial_scale;
    a.items = (unsigned)((uint64_t)d.k * d.ph * d.pw * (uint64_t)a.cv);
    hipLaunchKernelGGL((roi_align_kernel<T, VW>), dim3(si_grid_for(a.items, ROI_THREADS)), dim3(ROI_THREADS), 0, stream, a);
    return (int)hipGetLastError();
}

template <typename T>
int run(const SiRoiAlignDesc* desc, const void* x, const float* rois, void* out, si_stream_t stream) {
    if (!desc) return SI_E_BADARG;
    const SiRoiAlignDesc d = normalised(desc);
    const int rc = check_call(d, x, rois, out, sizeof(T));
    if (rc != 0) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int vw = vec_width<T>(d, x, out);
    if constexpr (sizeof(T) == 4) {
        return vw == 4 ? launch<T, 4>(d, x, rois, out, s) : launch<T, 1>(d, x, rois, out, s);
    } else {
        switch (vw) {
            case 8: return launch<T, 8>(d, x, rois, out, s);
            case 4: return launch<T, 4>(d, x, rois, out, s);
            case 2: return launch<T, 2>(d, x, rois, out, s);
            default: return launch<T, 1>(d, x, rois, out, s);
        }
    }
}

}  // namespace

extern "C" {

int si_hip_roi_align_f32(const SiRoiAlignDesc* d, const float* x, const float* rois, float* out, si_stream_t stream) {
    return run<float>(d, x, rois, out, stream);
}

int si_hip_roi_align_f16(const SiRoiAlignDesc* d, const void* x, const float* rois, void* out, si_stream_t stream) {
    return run<_Float16>(d, x, rois, out, stream);
}

const char* si_hip_roi_align_kernel_name(const SiRoiAlignDesc* desc, const void* x, const void* rois, const void* out, int half) {
    if (!desc) return "none";
    const SiRoiAlignDesc d = normalised(desc);
    if (check_call(d, x, rois, out, half ? 2 : 4) != 0) return "none";
    if (!half) return vec_width<float>(d, x, out) == 4 ? "roi_align_kernel<float, 4>" : "roi_align_kernel<float, 1>";
    const int vw = vec_width<_Float16>(d, x, out);
    return vw == 8   ? "roi_align_kernel<_Float16, 8>"
           : vw == 4 ? "roi_align_kernel<_Float16, 4>"
           : vw == 2 ? "roi_align_kernel<_Float16, 2>"
                     : "roi_align_kernel<_Float16, 1>";
}

}  // extern "C"
