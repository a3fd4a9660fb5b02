// pixel_shuffle.hip -- nn.PixelShuffle / nn.PixelUnshuffle (include/si_superres.h) on NHWC fp32 and fp16 tensors with pixel strides on
// both sides.  Pure data movement: values travel as integer words, nothing here does arithmetic on a value.
//
// Two tensors, whichever way the data goes: the DEEP one [n, h, w, D = C r r] and the WIDE one [n, h r, w r, C].  Element
// k = c r r + i r + j of deep pixel (h, w) is element c of wide pixel (h r + i, w r + j).
//
// Element form: one lane per OUTPUT element, 256 consecutive elements of an output row per workgroup: whole stores, strided loads.
//
// LDS form: a workgroup takes a run of P deep pixels of one row (blockIdx = (run, deep row, image)) and the r wide rows of
// P r pixels under it.  It reads its source side with 16-byte loads into an LDS image [p][q = i r + j][c], waits, and writes its
// destination side with 16-byte stores.  In that image the wide side's channel vectors are contiguous (one ds_read / ds_write of
// 16 bytes when C is a multiple of the vector, element by element otherwise) and the deep side always goes element by element:
// lane l of a deep vector holds channels k .. k + V - 1 and puts (takes) them at q C + c, which for consecutive lanes is
// consecutive c in the layers that matter (256 -> 64 at r = 2: a lane's four floats are one c and the four q), so neither side
// has a bank conflict worth the name.  A run is a flat array on each side -- P D elements of the deep row, P r C of each wide
// row -- cut into 16-byte vectors; a dense tensor whose channel count is no multiple of the vector (C = 3) is read and written
// with vectors that straddle pixels.  Index arithmetic inside a run is 32-bit with multiply-high divisions (exact below
// 2^32 / divisor; a run has at most 8192 elements).  Element offsets are 32-bit: the host refuses tensors whose offsets do not
// fit 31 bits.
//
// Register table per instantiation: DESIGN.md section 9g.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "si_hip_internal.h"
#include "si_superres.h"

namespace {

constexpr int PS_THREADS = 256;
constexpr int PS_LDS_BYTES = 16 * 1024;   // per workgroup: a budget (8 workgroups of 256 lanes fit a CU beside it), not a measured optimum
#ifndef SI_PS_UNROLL
#define SI_PS_UNROLL 2
#endif
constexpr int PS_UNROLL = SI_PS_UNROLL;   // 16-byte loads a lane issues before it touches LDS (2: at most 63 VGPRs, 8 waves / SIMD; 4: 116 and 4)

template <typename T> struct PsElem { typedef uint32_t type; };
template <> struct PsElem<_Float16> { typedef uint16_t type; };

struct PsArgs {
    const void* in;
    void* out;
    int deep_h, deep_w;     // of the deep tensor
    int C, r, rr, D;        // D = C * rr
    int deep_ld, wide_ld;
    int inverse;            // 0: deep -> wide, 1: wide -> deep
    int P;                  // deep pixels per run (LDS form), a multiple of 8
    unsigned m_D, m_rr, m_C, m_r;   // floor(2^32 / d) + 1
};

// x / d for x * d < 2^32 (d >= 2; m = floor(2^32 / d) + 1)
__device__ __forceinline__ int ps_div(int x, unsigned m) { return (int)__umulhi((unsigned)x, m); }

template <typename E>
__device__ __forceinline__ E ps_get(const u32x4& v, int t) {
    if constexpr (sizeof(E) == 4) return v[t];
    else return (E)(v[t >> 1] >> ((t & 1) * 16));
}

// (v starts as zeros)
template <typename E>
__device__ __forceinline__ void ps_put(u32x4& v, int t, E x) {
    if constexpr (sizeof(E) == 4) v[t] = x;
    else v[t >> 1] |= (unsigned)x << ((t & 1) * 16);
}

// ---- element form ------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(PS_THREADS) void pixel_shuffle_elem(PsArgs a) {
    typedef typename PsElem<T>::type E;
    const E* const in = static_cast<const E*>(a.in);
    E* const out = static_cast<E*>(a.out);
    const int img = (int)blockIdx.z;
    const int wide_h = a.deep_h * a.r, wide_w = a.deep_w * a.r;
    const int oc = a.inverse ? a.D : a.C, ow = a.inverse ? a.deep_w : wide_w, oh = a.inverse ? a.deep_h : wide_h;
    const int out_ld = a.inverse ? a.deep_ld : a.wide_ld;
    const int item = (int)blockIdx.x * PS_THREADS + (int)threadIdx.x;
    if (item >= ow * oc) return;
    const int ox = item / oc, k = item - ox * oc;
    if (!a.inverse) {
        const int w = ox / a.r, j = ox - w * a.r;
        const int col = w * a.deep_ld + k * a.rr + j;
        for (int oy = (int)blockIdx.y; oy < oh; oy += (int)gridDim.y) {
            const int h = oy / a.r, i = oy - h * a.r;   // (the same in every lane)
            out[((img * oh + oy) * ow + ox) * out_ld + k] = in[(img * a.deep_h + h) * a.deep_w * a.deep_ld + col + i * a.r];
        }
    } else {
        const int c = k / a.rr, q = k - c * a.rr, i = q / a.r, j = q - i * a.r;
        const int col = (ox * a.r + j) * a.wide_ld + c;
        for (int oy = (int)blockIdx.y; oy < oh; oy += (int)gridDim.y)
            out[((img * oh + oy) * ow + ox) * out_ld + k] = in[(img * wide_h + oy * a.r + i) * wide_w * a.wide_ld + col];
    }
}

// ---- LDS form ----------------------------------------------------------------------------------------------------------------
// where vector v of a run of the deep row starts: the global offset from the run's first element, and the pixel / channel it
// starts at
struct PsDeepPos { int off, pD, c, q; };

__device__ __forceinline__ PsDeepPos ps_deep_pos(const PsArgs& a, int e) {
    PsDeepPos s;
    const int p = ps_div(e, a.m_D), k = e - p * a.D;
    s.off = p * a.deep_ld + k;
    s.pD = p * a.D;
    s.c = ps_div(k, a.m_rr);
    s.q = k - s.c * a.rr;
    return s;
}

// the LDS index of the position, which then moves on by one element of the deep row
__device__ __forceinline__ int ps_deep_step(const PsArgs& a, PsDeepPos& s) {
    const int idx = s.pD + s.q * a.C + s.c;
    if (++s.q == a.rr) {
        s.q = 0;
        if (++s.c == a.C) {
            s.c = 0;
            s.pD += a.D;
        }
    }
    return idx;
}

// the same for a run of a wide row (row i of the r rows enters through qC = i r C)
struct PsWidePos { int off, wD, jC, c; };

__device__ __forceinline__ PsWidePos ps_wide_pos(const PsArgs& a, int e) {
    PsWidePos s;
    const int x = a.C == 1 ? e : ps_div(e, a.m_C);
    s.c = e - x * a.C;
    s.off = x * a.wide_ld + s.c;
    const int wl = ps_div(x, a.m_r);
    s.wD = wl * a.D;
    s.jC = (x - wl * a.r) * a.C;
    return s;
}

__device__ __forceinline__ int ps_wide_step(const PsArgs& a, PsWidePos& s, int iC, int rC) {
    const int idx = s.wD + iC + s.jC + s.c;
    if (++s.c == a.C) {
        s.c = 0;
        s.jC += a.C;
        if (s.jC == rC) {
            s.jC = 0;
            s.wD += a.D;
        }
    }
    return idx;
}

template <typename T, int WV>
__global__ __launch_bounds__(PS_THREADS) void pixel_shuffle_lds(PsArgs a) {
    typedef typename PsElem<T>::type E;
    constexpr int VW = (int)(16 / sizeof(T));
    __shared__ u32x4 image[PS_LDS_BYTES / 16];
    E* const lds = reinterpret_cast<E*>(image);
    const int tid = (int)threadIdx.x, img = (int)blockIdx.z;
    const int w0 = (int)blockIdx.x * a.P;
    const int np = min(a.P, a.deep_w - w0);
    const int wide_w = a.deep_w * a.r, rC = a.r * a.C;
    const int deep_vecs = np * a.D / VW, wide_vecs = np * rC / VW;   // exact: the host's conditions
    const E* const in = static_cast<const E*>(a.in);
    E* const out = static_cast<E*>(a.out);
    for (int h = (int)blockIdx.y; h < a.deep_h; h += (int)gridDim.y) {
        const int deep0 = ((img * a.deep_h + h) * a.deep_w + w0) * a.deep_ld;
        const int wide0 = ((img * a.deep_h + h) * a.r * wide_w + w0 * a.r) * a.wide_ld;   // row i: + i * wide_w * wide_ld
        if (!a.inverse) {
            // the deep run -> LDS, element by element
            for (int v0 = tid; v0 < deep_vecs; v0 += PS_UNROLL * PS_THREADS) {
                u32x4 val[PS_UNROLL];
                PsDeepPos pos[PS_UNROLL];
#pragma unroll
                for (int u = 0; u < PS_UNROLL; ++u) {
                    const int v = v0 + u * PS_THREADS;
                    if (v < deep_vecs) {
                        pos[u] = ps_deep_pos(a, v * VW);
                        val[u] = *reinterpret_cast<const u32x4*>(in + deep0 + pos[u].off);
                    }
                }
#pragma unroll
                for (int u = 0; u < PS_UNROLL; ++u) {
                    if (v0 + u * PS_THREADS < deep_vecs) {
#pragma unroll
                        for (int t = 0; t < VW; ++t) lds[ps_deep_step(a, pos[u])] = ps_get<E>(val[u], t);
                    }
                }
            }
            __syncthreads();
            // LDS -> the r wide runs
            for (int i = 0; i < a.r; ++i) {
                E* const row = out + wide0 + i * wide_w * a.wide_ld;
                const int iC = i * rC;
                for (int v = tid; v < wide_vecs; v += PS_THREADS) {
                    PsWidePos pos = ps_wide_pos(a, v * VW);
                    const int off = pos.off;
                    u32x4 val = {0u, 0u, 0u, 0u};
                    if constexpr (WV == VW) {
                        val = *reinterpret_cast<const u32x4*>(lds + pos.wD + iC + pos.jC + pos.c);
                    } else {
#pragma unroll
                        for (int t = 0; t < VW; ++t) ps_put<E>(val, t, lds[ps_wide_step(a, pos, iC, rC)]);
                    }
                    *reinterpret_cast<u32x4*>(row + off) = val;
                }
            }
        } else {
            // the r wide runs -> LDS
            for (int i = 0; i < a.r; ++i) {
                const E* const row = in + wide0 + i * wide_w * a.wide_ld;
                const int iC = i * rC;
                for (int v0 = tid; v0 < wide_vecs; v0 += PS_UNROLL * PS_THREADS) {
                    u32x4 val[PS_UNROLL];
                    PsWidePos pos[PS_UNROLL];
#pragma unroll
                    for (int u = 0; u < PS_UNROLL; ++u) {
                        const int v = v0 + u * PS_THREADS;
                        if (v < wide_vecs) {
                            pos[u] = ps_wide_pos(a, v * VW);
                            val[u] = *reinterpret_cast<const u32x4*>(row + pos[u].off);
                        }
                    }
#pragma unroll
                    for (int u = 0; u < PS_UNROLL; ++u) {
                        if (v0 + u * PS_THREADS < wide_vecs) {
                            if constexpr (WV == VW) {
                                *reinterpret_cast<u32x4*>(lds + pos[u].wD + iC + pos[u].jC + pos[u].c) = val[u];
                            } else {
#pragma unroll
                                for (int t = 0; t < VW; ++t) lds[ps_wide_step(a, pos[u], iC, rC)] = ps_get<E>(val[u], t);
                            }
                        }
                    }
                }
            }
            __syncthreads();
            // LDS -> the deep run, element by element
            for (int v = tid; v < deep_vecs; v += PS_THREADS) {
                PsDeepPos pos = ps_deep_pos(a, v * VW);
                const int off = pos.off;
                u32x4 val = {0u, 0u, 0u, 0u};
#pragma unroll
                for (int t = 0; t < VW; ++t) ps_put<E>(val, t, lds[ps_deep_step(a, pos)]);
                *reinterpret_cast<u32x4*>(out + deep0 + off) = val;
            }
        }
        __syncthreads();   // the image is reused by the next row
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------
// everything that can be decided without a device: SI_E_BADARG / SI_E_UNSUPPORTED / 0
int check_desc(const SiPixelShuffleDesc* d) {
    if (!d) return SI_E_BADARG;
    if (d->n <= 0 || d->ih <= 0 || d->iw <= 0 || d->ic <= 0 || d->oh <= 0 || d->ow <= 0 || d->oc <= 0 || d->r < 1) return SI_E_BADARG;
    if (d->in_ld < d->ic || d->out_ld < d->oc) return SI_E_BADARG;
    const int64_t r = d->r, rr = r * r;
    if (!d->inverse) {
        if ((int64_t)d->oc * rr != d->ic || (int64_t)d->ih * r != d->oh || (int64_t)d->iw * r != d->ow) return SI_E_BADARG;
    } else {
        if (d->ih % r != 0 || d->iw % r != 0) return SI_E_BADARG;
        if ((int64_t)d->ic * rr != d->oc || (int64_t)d->oh * r != d->ih || (int64_t)d->ow * r != d->iw) return SI_E_BADARG;
    }
    if (d->n > 65535) return SI_E_UNSUPPORTED;
    const uint64_t in_rows = (uint64_t)d->n * d->ih, out_rows = (uint64_t)d->n * d->oh;   // < 2^47
    if (in_rows > SI_INDEX_LIMIT || out_rows > SI_INDEX_LIMIT) return SI_E_UNSUPPORTED;
    const uint64_t in_pix = in_rows * d->iw, out_pix = out_rows * d->ow;                    // < 2^62
    if (in_pix > SI_INDEX_LIMIT || out_pix > SI_INDEX_LIMIT) return SI_E_UNSUPPORTED;
    if (in_pix * (uint64_t)d->in_ld > SI_INDEX_LIMIT || out_pix * (uint64_t)d->out_ld > SI_INDEX_LIMIT) return SI_E_UNSUPPORTED;
    return 0;
}

// one side of the LDS form: 16-byte vectors inside the pixels, or a dense tensor whose rows are whole vectors
inline bool side_ok(int c, int ld, int w, int vw) { return (c % vw == 0 && ld % vw == 0) || (ld == c && ((int64_t)w * c) % vw == 0); }

// 0: the element form; 1: the LDS form gathering single elements on the wide side; VW: the LDS form with channel vectors
template <typename T>
int lds_form(const SiPixelShuffleDesc* d, const void* in, const void* out) {
    constexpr int VW = (int)(16 / sizeof(T));
    const int D = d->inverse ? d->oc : d->ic, C = d->inverse ? d->ic : d->oc;
    const int deep_ld = d->inverse ? d->out_ld : d->in_ld, wide_ld = d->inverse ? d->in_ld : d->out_ld;
    const int deep_w = d->inverse ? d->ow : d->iw, wide_w = d->inverse ? d->iw : d->ow;
    if (d->r < 2 || !si_aligned_to(in, 16) || !si_aligned_to(out, 16)) return 0;
    if ((size_t)D * sizeof(T) * 8 > (size_t)PS_LDS_BYTES) return 0;   // a run is at least 8 pixels
    if (!side_ok(D, deep_ld, deep_w, VW) || !side_ok(C, wide_ld, wide_w, VW)) return 0;
    return C % VW == 0 ? VW : 1;
}

inline unsigned magic(int d) { return d < 2 ? 0u : (unsigned)(0x100000000ull / (unsigned)d) + 1u; }

template <typename T>
int run(const SiPixelShuffleDesc* d, const T* in, T* out, si_stream_t stream) {
    const int rc = check_desc(d);
    if (rc != 0) return rc;
    if (!in || !out) return SI_E_BADARG;
    constexpr int VW = (int)(16 / sizeof(T));
    PsArgs a;
    a.in = in;
    a.out = out;
    a.inverse = d->inverse ? 1 : 0;
    a.r = d->r;
    a.rr = d->r * d->r;
    a.deep_h = a.inverse ? d->oh : d->ih;
    a.deep_w = a.inverse ? d->ow : d->iw;
    a.C = a.inverse ? d->ic : d->oc;
    a.D = a.inverse ? d->oc : d->ic;
    a.deep_ld = a.inverse ? d->out_ld : d->in_ld;
    a.wide_ld = a.inverse ? d->in_ld : d->out_ld;
    a.P = 0;
    a.m_D = magic(a.D); a.m_rr = magic(a.rr); a.m_C = magic(a.C); a.m_r = magic(a.r);
    hipStream_t s = (hipStream_t)stream;
    const int form = lds_form<T>(d, in, out);
    if (form == 0) {
        unsigned rows = (unsigned)d->oh;
        if (rows > 65535u) rows = 65535u;
        const dim3 grid(((unsigned)d->ow * (unsigned)d->oc + PS_THREADS - 1) / PS_THREADS, rows, (unsigned)d->n);
        hipLaunchKernelGGL((pixel_shuffle_elem<T>), grid, dim3(PS_THREADS), 0, s, a);
        return (int)hipGetLastError();
    }
    int P = (int)((size_t)PS_LDS_BYTES / ((size_t)a.D * sizeof(T))) / 8 * 8;   // >= 8: lds_form
    const int w8 = (a.deep_w + 7) / 8 * 8;
    a.P = P < w8 ? P : w8;
    unsigned rows = (unsigned)a.deep_h;
    if (rows > 65535u) rows = 65535u;
    const dim3 grid(((unsigned)a.deep_w + a.P - 1) / a.P, rows, (unsigned)d->n);
    if (form == VW) hipLaunchKernelGGL((pixel_shuffle_lds<T, VW>), grid, dim3(PS_THREADS), 0, s, a);
    else hipLaunchKernelGGL((pixel_shuffle_lds<T, 1>), grid, dim3(PS_THREADS), 0, s, a);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int si_hip_pixel_shuffle_f32(const SiPixelShuffleDesc* d, const float* in, float* out, si_stream_t stream) { return run<float>(d, in, out, stream); }

int si_hip_pixel_shuffle_f16(const SiPixelShuffleDesc* d, const void* in, void* out, si_stream_t stream) {
    return run<_Float16>(d, static_cast<const _Float16*>(in), static_cast<_Float16*>(out), stream);
}

const char* si_hip_pixel_shuffle_kernel_name(const SiPixelShuffleDesc* d, const void* in, const void* out, int half) {
    if (check_desc(d) != 0) return "none";
    if (half) {
        const int f = lds_form<_Float16>(d, in, out);
        return f == 0 ? "pixel_shuffle_elem<_Float16>" : (f == 1 ? "pixel_shuffle_lds<_Float16, 1>" : "pixel_shuffle_lds<_Float16, 8>");
    }
    const int f = lds_form<float>(d, in, out);
    return f == 0 ? "pixel_shuffle_elem<float>" : (f == 1 ? "pixel_shuffle_lds<float, 1>" : "pixel_shuffle_lds<float, 4>");
}

}  // extern "C"
