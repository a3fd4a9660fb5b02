// upsample_bilinear.hip -- bilinear nn.Upsample / F.interpolate (torch's rule, align_corners both ways) on NHWC fp32 and fp16
// tensors, and the segmentation label map (argmax over classes of the bilinear upsample, the upsampled logits never written).
//
// One rule for everything in this file (include/si_hip.h, "Upsample"): per axis a float32 step `s`, formed on the HOST
// (si_upsample_step), and per destination index d
//     align_corners:  src = s * (float)d                       otherwise:  src = max(0, fmaf(s, (float)d + 0.5f, -0.5f))
//     i0 = min((int)src, in - 1),  i1 = i0 + (i0 < in - 1),  l1 = src - (float)i0,  l0 = 1 - l1
//     out = l0h * (l0w * v00 + l1w * v01) + l1h * (l0w * v10 + l1w * v11)
// blended in fp32 whatever the storage type, with the fused multiply-adds written out (the file is compiled with contraction
// off), so the copy kernel, the label map and every vector width produce the same bits.
//
// Shape of the copy kernel: HBM-bound, one read of the input and one write of the output.  A lane owns ONE (x, channel vector)
// column of the output for the rows of its workgroup's band: the column's taps and weights are computed once, the row's taps and
// weights are wave-uniform, and the loop over the band's rows holds four loads, the blend and one store.  x and channel run fastest
// across lanes, so a wave reads two contiguous stretches of two source rows and writes one contiguous stretch of the output row;
// the overlapping taps of neighbouring pixels and rows meet in L1 / L2.  No LDS, no scratch, no atomics.
// -Rpass-analysis=kernel-resource-usage, all eight instantiations: scratch 0, LDS 0, 8 waves / SIMD; VGPRs <float, 4> 34, <float, 1> 19,
// <_Float16, 8 | 4 | 2 | 1> 60 | 36 | 23 | 18, segment_labels <float> 26, <_Float16> 24 (profiles/upsample_bilinear_56fe1c1.txt, section 4).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "si_hip.h"
#include "si_hip_internal.h"

// no implicit contraction anywhere in this file: every fused multiply-add below is written out
#pragma clang fp contract(off)

namespace {

template <typename T, int VW> struct VecOf;
template <> struct VecOf<float, 4> { typedef f32x4 type; };
template <> struct VecOf<float, 1> { typedef float type; };
template <> struct VecOf<_Float16, 8> { typedef f16x8 type; };
template <> struct VecOf<_Float16, 4> { typedef f16x4 type; };
template <> struct VecOf<_Float16, 2> { typedef f16x2 type; };
template <> struct VecOf<_Float16, 1> { typedef _Float16 type; };

struct Tap {
    int i0, i1;
    float l0, l1;
};

// source taps and weights of destination index d on one axis
__device__ __forceinline__ Tap tap_of(int d, int in, float step, bool align_corners) {
    const float src = align_corners ? step * (float)d : fmaxf(0.0f, __fmaf_rn(step, (float)d + 0.5f, -0.5f));
    Tap t;
    t.i0 = min((int)src, in - 1);
    t.i1 = t.i0 + (t.i0 < in - 1 ? 1 : 0);
    t.l1 = src - (float)t.i0;
    t.l0 = 1.0f - t.l1;
    return t;
}

// the blend, in this order and with these fused operations everywhere
__device__ __forceinline__ float blend(float v00, float v01, float v10, float v11, float l0w, float l1w, float l0h, float l1h) {
    const float top = __fmaf_rn(l0w, v00, l1w * v01);
    const float bot = __fmaf_rn(l0w, v10, l1w * v11);
    return __fmaf_rn(l0h, top, l1h * bot);
}

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

// the horizontal half of the blend for one source row: l0w * v[x0] + l1w * v[x1]
template <typename T, int VW>
__device__ __forceinline__ void blend_row(const T* row, unsigned off0, unsigned off1, float l0w, float l1w, float (&h)[VW]) {
    float v0[VW], v1[VW];
    load_vec<T, VW>(row + off0, v0);
    load_vec<T, VW>(row + off1, v1);
#pragma unroll
    for (int i = 0; i < VW; ++i) h[i] = __fmaf_rn(l0w, v0[i], l1w * v1[i]);
}

// grid: (column blocks, row bands, images); block 256.  Column index = x * (c / VW) + channel vector.
// The horizontally blended values of the two source rows stay in registers from one output row to the next: when upsampling,
// consecutive output rows share one or both source rows (x2: ~1.25 source rows per output row instead of 2), and which row is
// needed is the same for every lane, so the reuse is a wave-uniform branch.  Same operations per output element as blend().
template <typename T, int VW>
__global__ __launch_bounds__(256) void upsample_bilinear_kernel(const T* __restrict__ in, T* __restrict__ out, const SiUpsampleDesc d,
                                                                int rows_per_band) {
    const unsigned cv = (unsigned)d.c / VW;
    const unsigned col = blockIdx.x * 256u + threadIdx.x;
    if (col >= (unsigned)d.ow * cv) return;
    const unsigned x = col / cv;
    const unsigned ch = (col - x * cv) * VW;
    const bool ac = d.align_corners != 0;
    const Tap tw = tap_of((int)x, d.iw, d.step_w, ac);
    const unsigned img = blockIdx.z;
    const T* const src = in + (size_t)img * d.ih * d.iw * d.in_ld + ch;
    const unsigned off0 = (unsigned)tw.i0 * d.in_ld, off1 = (unsigned)tw.i1 * d.in_ld;
    const int y0 = blockIdx.y * rows_per_band;
    const int y1 = min(y0 + rows_per_band, d.oh);
    T* o = out + ((size_t)img * d.oh + y0) * d.ow * d.out_ld + (size_t)x * d.out_ld + ch;
    const unsigned in_row = (unsigned)d.iw * d.in_ld, out_row = (unsigned)d.ow * d.out_ld;
    int have0 = -1, have1 = -1;   // the source rows whose horizontal blends h0 / h1 hold
    float h0[VW], h1[VW];
#pragma unroll
    for (int i = 0; i < VW; ++i) h0[i] = h1[i] = 0.0f;
    for (int y = y0; y < y1; ++y, o += out_row) {
        const Tap th = tap_of(y, d.ih, d.step_h, ac);
        float n0[VW], n1[VW], r[VW];
        if (th.i0 == have0) {
#pragma unroll
            for (int i = 0; i < VW; ++i) n0[i] = h0[i];
        } else if (th.i0 == have1) {
#pragma unroll
            for (int i = 0; i < VW; ++i) n0[i] = h1[i];
        } else {
            blend_row<T, VW>(src + (size_t)th.i0 * in_row, off0, off1, tw.l0, tw.l1, n0);
        }
        if (th.i1 == th.i0) {
#pragma unroll
            for (int i = 0; i < VW; ++i) n1[i] = n0[i];
        } else if (th.i1 == have1) {
#pragma unroll
            for (int i = 0; i < VW; ++i) n1[i] = h1[i];
        } else if (th.i1 == have0) {
#pragma unroll
            for (int i = 0; i < VW; ++i) n1[i] = h0[i];
        } else {
            blend_row<T, VW>(src + (size_t)th.i1 * in_row, off0, off1, tw.l0, tw.l1, n1);
        }
#pragma unroll
        for (int i = 0; i < VW; ++i) {
            h0[i] = n0[i];
            h1[i] = n1[i];
            r[i] = __fmaf_rn(th.l0, n0[i], th.l1 * n1[i]);
        }
        have0 = th.i0;
        have1 = th.i1;
        store_vec<T, VW>(o, r);
    }
}

// label map: one lane per output pixel, x fastest; grid (x blocks, oh, n).  The four source pixels' channel rows are walked
// together; strictly-greater keeps the lowest class index on a tie.
template <typename T>
__global__ __launch_bounds__(256) void segment_labels_kernel(const T* __restrict__ in, unsigned char* __restrict__ labels,
                                                             const SiUpsampleDesc d) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= d.ow) return;
    const int y = blockIdx.y, img = blockIdx.z;
    const bool ac = d.align_corners != 0;
    const Tap tw = tap_of(x, d.iw, d.step_w, ac);
    const Tap th = tap_of(y, d.ih, d.step_h, ac);
    const T* const base = in + (size_t)img * d.ih * d.iw * d.in_ld;
    const T* const p00 = base + ((size_t)th.i0 * d.iw + tw.i0) * d.in_ld;
    const T* const p01 = base + ((size_t)th.i0 * d.iw + tw.i1) * d.in_ld;
    const T* const p10 = base + ((size_t)th.i1 * d.iw + tw.i0) * d.in_ld;
    const T* const p11 = base + ((size_t)th.i1 * d.iw + tw.i1) * d.in_ld;
    float best = blend((float)p00[0], (float)p01[0], (float)p10[0], (float)p11[0], tw.l0, tw.l1, th.l0, th.l1);
    int arg = 0;
    for (int c = 1; c < d.c; ++c) {
        const float v = blend((float)p00[c], (float)p01[c], (float)p10[c], (float)p11[c], tw.l0, tw.l1, th.l0, th.l1);
        if (v > best) {
            best = v;
            arg = c;
        }
    }
    labels[((size_t)img * d.oh + y) * d.ow + x] = (unsigned char)arg;
}

// everything that can be decided without a device: SI_E_BADARG / SI_E_UNSUPPORTED / 0
int check_desc(const SiUpsampleDesc* d, bool out_is_labels) {
    if (!d) return SI_E_BADARG;
    if (d->n <= 0 || d->ih <= 0 || d->iw <= 0 || d->c <= 0 || d->oh <= 0 || d->ow <= 0) return SI_E_BADARG;
    if (d->in_ld < d->c || (!out_is_labels && d->out_ld < d->c)) return SI_E_BADARG;
    if (!std::isfinite(d->step_h) || !std::isfinite(d->step_w) || d->step_h < 0.0f || d->step_w < 0.0f) return SI_E_BADARG;
    if ((uint64_t)d->n * d->ih * d->iw * (uint64_t)d->in_ld > SI_INDEX_LIMIT) return SI_E_UNSUPPORTED;
    if ((uint64_t)d->n * d->oh * d->ow * (uint64_t)(out_is_labels ? 1 : d->out_ld) > SI_INDEX_LIMIT) return SI_E_UNSUPPORTED;
    if (d->n > 65535) return SI_E_UNSUPPORTED;
    if (out_is_labels && (d->c > 256 || d->oh > 65535)) return SI_E_UNSUPPORTED;
    return 0;
}

// widest channel vector (in elements) that c, both strides and both base pointers allow
template <typename T>
int vec_width(const SiUpsampleDesc* d, const void* in, const void* out) {
    const int widths[] = {(int)(16 / sizeof(T)), (int)(8 / sizeof(T)), (int)(4 / sizeof(T))};
    for (int w : widths) {
        if (w <= 1) break;
        const size_t bytes = w * sizeof(T);
        if (d->c % w == 0 && d->in_ld % w == 0 && d->out_ld % w == 0 && si_aligned_to(in, bytes) && si_aligned_to(out, bytes)) return w;
    }
    return 1;
}

template <typename T, int VW>
int launch(const SiUpsampleDesc* d, const T* in, T* out, hipStream_t stream) {
    const unsigned cols = (unsigned)d->ow * (unsigned)(d->c / VW);
    const unsigned col_blocks = (cols + 255u) / 256u;
    // rows per band: the more rows, the more source rows are reused from registers (x2: 9 source rows per 16 output rows against
    // 2 per row); as many, up to 16, as leave ~4 workgroups per CU.  The sweep behind the two constants (rows 1 .. 16 forced on the
    // decoder and head shapes at batch 8) is in profiles/upsample_bilinear_56fe1c1.txt, section 3.
    int rows = 16;
    while (rows > 1 && (uint64_t)col_blocks * ((d->oh + rows - 1) / rows) * d->n < 1024u) rows /= 2;
    const int forced = SI_ENV_INT("SI_UPSAMPLE_ROWS", 0);   // (experiment build only: sweeps)
    if (forced > 0) rows = forced;
    const unsigned bands = (unsigned)((d->oh + rows - 1) / rows);
    if (bands > 65535u) return SI_E_UNSUPPORTED;
    hipLaunchKernelGGL((upsample_bilinear_kernel<T, VW>), dim3(col_blocks, bands, (unsigned)d->n), dim3(256), 0, stream, in, out, *d, rows);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int si_upsample_out_size(int in, double scale_factor) {
    if (in <= 0 || !(scale_factor > 0.0) || !std::isfinite(scale_factor)) return SI_E_BADARG;
    const double o = std::floor((double)in * scale_factor);
    if (o < 1.0 || o > 2147483647.0) return SI_E_BADARG;
    return (int)o;
}

int si_upsample_step(int mode, int in, int out, int align_corners, double scale_factor, float* step) {
    if (!step || in <= 0 || out <= 0 || (mode != SI_UPSAMPLE_NEAREST && mode != SI_UPSAMPLE_BILINEAR)) return SI_E_BADARG;
    if (scale_factor != 0.0 && (!(scale_factor > 0.0) || !std::isfinite(scale_factor))) return SI_E_BADARG;
    if (align_corners) {
        if (mode == SI_UPSAMPLE_NEAREST) return SI_E_BADARG;   // (torch refuses it too)
        *step = out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.0f;
    } else if (scale_factor > 0.0) {
        *step = (float)(1.0 / scale_factor);
    } else {
        *step = (float)in / (float)out;
    }
    return 0;
}

int si_hip_upsample_bilinear_f32(const SiUpsampleDesc* d, const float* in, float* out, si_stream_t stream) {
    const int rc = check_desc(d, false);
    if (rc != 0) return rc;
    if (!in || !out) return SI_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    return vec_width<float>(d, in, out) == 4 ? launch<float, 4>(d, in, out, s) : launch<float, 1>(d, in, out, s);
}

int si_hip_upsample_bilinear_f16(const SiUpsampleDesc* d, const void* in, void* out, si_stream_t stream) {
    const int rc = check_desc(d, false);
    if (rc != 0) return rc;
    if (!in || !out) return SI_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    const _Float16* i = static_cast<const _Float16*>(in);
    _Float16* o = static_cast<_Float16*>(out);
    switch (vec_width<_Float16>(d, in, out)) {
        case 8: return launch<_Float16, 8>(d, i, o, s);
        case 4: return launch<_Float16, 4>(d, i, o, s);
        case 2: return launch<_Float16, 2>(d, i, o, s);
        default: return launch<_Float16, 1>(d, i, o, s);
    }
}

const char* si_hip_upsample_bilinear_kernel_name(const SiUpsampleDesc* d, const void* in, const void* out, int half) {
    if (check_desc(d, false) != 0) return "none";
    if (!half) return vec_width<float>(d, in, out) == 4 ? "upsample_bilinear_kernel<float, 4>" : "upsample_bilinear_kernel<float, 1>";
    switch (vec_width<_Float16>(d, in, out)) {
        case 8: return "upsample_bilinear_kernel<_Float16, 8>";
        case 4: return "upsample_bilinear_kernel<_Float16, 4>";
        case 2: return "upsample_bilinear_kernel<_Float16, 2>";
        default: return "upsample_bilinear_kernel<_Float16, 1>";
    }
}

int si_hip_segment_labels_f32(const SiUpsampleDesc* d, const float* logits, unsigned char* labels, si_stream_t stream) {
    const int rc = check_desc(d, true);
    if (rc != 0) return rc;
    if (!logits || !labels) return SI_E_BADARG;
    hipLaunchKernelGGL(segment_labels_kernel<float>, dim3((d->ow + 255) / 256, d->oh, d->n), dim3(256), 0, (hipStream_t)stream, logits, labels, *d);
    return (int)hipGetLastError();
}

int si_hip_segment_labels_f16(const SiUpsampleDesc* d, const void* logits, unsigned char* labels, si_stream_t stream) {
    const int rc = check_desc(d, true);
    if (rc != 0) return rc;
    if (!logits || !labels) return SI_E_BADARG;
    hipLaunchKernelGGL(segment_labels_kernel<_Float16>, dim3((d->ow + 255) / 256, d->oh, d->n), dim3(256), 0, (hipStream_t)stream,
                       static_cast<const _Float16*>(logits), labels, *d);
    return (int)hipGetLastError();
}

}  // extern "C"
