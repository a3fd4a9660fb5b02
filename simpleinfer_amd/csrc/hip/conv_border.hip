// conv_border.hip -- the border-mapped convolution of nn.Conv2d(padding_mode = reflect | replicate | circular) (include/si_border.h).
// The rule, the work split, the LDS layout with its bank arithmetic, the reduction order, the contract and the refusals: the header.
//
// A workgroup of four waves owns TH x TW = 4 x 16 output pixels x up to 64 filters of one image.  Phases:
//   1. tables   ymap[PH], xmap[positions], kpos[kw] into LDS: the mapped source row of every patch row, the mapped source column of every
//               patch column POSITION (phase-major: column p at (p mod sw) CW + p / sw), the position of each kx's first column
//   2. per chunk of KC = 32 input channels, between two barriers: every thread carries one 16-byte vector slot of a pixel and walks the
//      patch pixels 256 / (vectors per pixel) at a time -- global -> registers -> LDS through the tables; then every tap (ky, kx) reads
//      its B fragment (16 bytes of consecutive channels of the lane's pixel) from the patch at row w sh + ky dh, position kpos[kx] + x,
//      and its A fragments (the same channels of filter 16 t + x) from the weight image in global memory
//   3. epilogue in registers: bias, act1, residual, act2; a lane holds four consecutive output channels of one pixel (si_mma_dev.h's
//      pixel-on-x tile, shared with xcorr.hip: si_pix16_filters, si_frag16, si_pix16_store)
// With lane = 16 g + x (g = 0..3, x = 0..15): fp32 fragments hold channels 16 q + 4 g + 0..3 of block q (four 16x16x4 steps, step j
// taking element j), fp16 fragments channels 8 g + 0..7 of the chunk (one 16x16x32 step).  One integer division per thread (its first patch
// pixel -> row, position) and one per workgroup (tile -> tile row, tile column), none in a loop; the tables need kw + sw more.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "si_border.h"
#include "si_hip_internal.h"

#pragma clang fp contract(off)

namespace {

constexpr int BD_THREADS = 256;
constexpr int BD_TILE_OC = 16;
static_assert(SI_BORDER_TH == BD_THREADS / 64, "a wave owns one row of the tile");
static_assert(SI_BORDER_TW == 16 && SI_BORDER_OC == 4 * BD_TILE_OC && SI_BORDER_KC == 32, "the lane maps below");
static_assert(((SI_BORDER_KC + SI_BORDER_PAD_F32) * 4 / 16) % 2 == 1 && ((SI_BORDER_KC + SI_BORDER_PAD_F16) * 2 / 16) % 2 == 1,
              "an odd pixel pitch in 16-byte slots: the header's bank arithmetic");

// the one map: compares and adds.  Inside the preconditions the result is a row / column of the image; outside them it is whatever one
// fold gives (the callers clamp or refuse)
__host__ __device__ inline int border_map(int mode, int i, int n) {
    if (mode == SI_PAD_REFLECT) return i < 0 ? -i : (i > n - 1 ? 2 * (n - 1) - i : i);
    if (mode == SI_PAD_CIRCULAR) return i < 0 ? i + n : (i > n - 1 ? i - n : i);
    return i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
}
__host__ __device__ inline int clamp_index(int i, int n) { return i < 0 ? 0 : (i > n - 1 ? n - 1 : i); }

struct BorderArgs {
    const void* x;
    const void* w;
    const float* bias;
    const void* res;
    void* y;
    int ih, iw, ic, in_ld, oh, ow, oc, out_ld, res_ld;
    int kh, kw, sh, sw, dh, dw, pt, pl, mode;
    int icp;             // channels of a tap in the weight image
    int th;              // live rows of the tile: 4, 2 or 1
    int ph, cw, npos;    // patch rows; positions of one phase; positions of a row (sw cw)
    int tiles_x;
    int x_sn, x_sh, y_sn, r_sn;
    int x_vec, y_vec;
    int act1, act2;
    float act_param;
};

template <typename T, int TILES>
__global__ __launch_bounds__(BD_THREADS) void conv_border_kernel(BorderArgs a) {
    constexpr bool HALF = sizeof(T) == 2;
    constexpr int VE = 16 / (int)sizeof(T);                                               // elements of a 16-byte vector
    constexpr int PITCH = SI_BORDER_KC + (HALF ? SI_BORDER_PAD_F16 : SI_BORDER_PAD_F32);  // elements between two staged pixels
    constexpr int VPP = SI_BORDER_KC / VE;                                                // vectors of a staged pixel
    constexpr int STEP = BD_THREADS / VPP;                                                // patch pixels staged per round
    typedef si_vec<T, VE> Vec;

    extern __shared__ __attribute__((aligned(16))) unsigned char bd_lds[];
    T* const patch = reinterpret_cast<T*>(bd_lds);
    int* const ymap = reinterpret_cast<int*>(bd_lds + (size_t)a.ph * a.npos * PITCH * sizeof(T));
    int* const xmap = ymap + a.ph;
    int* const kpos = xmap + a.npos;

    const int tid = (int)threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int xl = lane & 15, g = lane >> 4;
    const int tile_y = (int)blockIdx.x / a.tiles_x;
    const int tile_x = (int)blockIdx.x - tile_y * a.tiles_x;
    const int oy0 = tile_y * a.th, ox0 = tile_x * SI_BORDER_TW;
    const int o0 = (int)blockIdx.y * SI_BORDER_OC;
    const int n = (int)blockIdx.z;

    // ---- 1. tables.  A row / column that only dead outputs of a ragged tile read lies beyond one fold: clamped into the image
    for (int r = tid; r < a.ph; r += BD_THREADS) ymap[r] = clamp_index(border_map(a.mode, oy0 * a.sh - a.pt + r, a.ih), a.ih);
    for (int phase = 0; phase < a.sw; ++phase)
        for (int q = tid; q < a.cw; q += BD_THREADS)
            xmap[phase * a.cw + q] = clamp_index(border_map(a.mode, ox0 * a.sw - a.pl + q * a.sw + phase, a.iw), a.iw);
    for (int kx = tid; kx < a.kw; kx += BD_THREADS) {
        const int off = kx * a.dw, q = off / a.sw;
        kpos[kx] = (off - q * a.sw) * a.cw + q;
    }

    // this thread's staging walk: vector slot v of the patch pixels first, first + STEP, ... (row, position kept by adds)
    const int v = tid % VPP, first = tid / VPP;
    const int r0 = first / a.npos, j0 = first - r0 * a.npos;
    const int step_r = STEP / a.npos, step_j = STEP - step_r * a.npos;

    const T* const xn = static_cast<const T*>(a.x) + n * a.x_sn;
    const T* const wb = static_cast<const T*>(a.w);
    const int taps = a.kh * a.kw;
    int wo_[TILES];
    bool wl[TILES];
    f32x4 acc[TILES];
    si_pix16_filters(o0 + xl, a.oc, taps, a.icp, wo_, wl, acc);
    const bool wave_live = wave < a.th;

    for (int c0 = 0; c0 < a.ic; c0 += SI_BORDER_KC) {
        __syncthreads();   // the tables are written / the previous chunk's fragments are read
        // ---- 2a. stage the chunk: every pixel exists in the image; the zeros are the channels beyond ic
        {
            const int c = c0 + v * VE;
            int r = r0, j = j0;
            while (r < a.ph) {
                const T* const src = xn + ymap[r] * a.x_sh + xmap[j] * a.in_ld;
                Vec val;
                if (a.x_vec) {
                    val = *reinterpret_cast<const Vec*>(src + (c < a.ic ? c : 0));   // (ic % VE == 0: a vector is inside or beyond)
                    if (c >= a.ic) {
#pragma unroll
                        for (int e = 0; e < VE; ++e) val[e] = (T)0;
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < VE; ++e) {
                        const bool le = c + e < a.ic;
                        const T el = src[le ? c + e : 0];
                        val[e] = le ? el : (T)0;
                    }
                }
                *reinterpret_cast<Vec*>(patch + (r * a.npos + j) * PITCH + v * VE) = val;
                j += step_j;
                r += step_r;
                if (j >= a.npos) {
                    j -= a.npos;
                    ++r;
                }
            }
        }
        __syncthreads();
        // ---- 2b. the taps of the chunk, ascending
        if (wave_live) {
            for (int ky = 0; ky < a.kh; ++ky) {
                const T* const prow = patch + (wave * a.sh + ky * a.dh) * a.npos * PITCH;
                for (int kx = 0; kx < a.kw; ++kx) {
                    const T* const pp = prow + (kpos[kx] + xl) * PITCH;
                    const int woff = (ky * a.kw + kx) * a.icp + c0;
                    if constexpr (HALF) {
                        const int cl = 8 * g;
                        const f16x8 b = *reinterpret_cast<const f16x8*>(pp + cl);
                        const bool live_c = c0 + cl < a.icp;
                        f16x8 wf[TILES];
#pragma unroll
                        for (int t = 0; t < TILES; ++t) wf[t] = si_frag16(wb, wo_[t] + woff + cl, wl[t] && live_c);
#pragma unroll
                        for (int t = 0; t < TILES; ++t) acc[t] = si_mma16_block(wf[t], b, acc[t]);
                    } else {
#pragma unroll
                        for (int q = 0; q < SI_BORDER_KC / 16; ++q) {
                            if (c0 + 16 * q >= a.ic) break;   // (a block of zeros on both sides)
                            const int cl = 16 * q + 4 * g;
                            const f32x4 b = *reinterpret_cast<const f32x4*>(pp + cl);
                            const bool live_c = c0 + cl < a.icp;
                            f32x4 wf[TILES];
#pragma unroll
                            for (int t = 0; t < TILES; ++t) wf[t] = si_frag16(wb, wo_[t] + woff + cl, wl[t] && live_c);
#pragma unroll
                            for (int t = 0; t < TILES; ++t)   // (si_mma16_block, written out: through the helper <float, 4> takes 4 more AGPRs and loses a wave)
#pragma unroll
                                for (int j = 0; j < 4; ++j) acc[t] = si_mma16(wf[t][j], b[j], acc[t]);
                        }
                    }
                }
            }
        }
    }

    // ---- 3. epilogue (si_pix16_store): register r of accumulator t is filter o0 + 16 t + 4 g + r at this lane's pixel
    const int oy = oy0 + wave, ox = ox0 + xl;
    if (!wave_live || oy >= a.oh || ox >= a.ow) return;
    const int pix = oy * a.ow + ox;
    T* const yp = static_cast<T*>(a.y) + n * a.y_sn + pix * a.out_ld;
    const T* const rp = a.res ? static_cast<const T*>(a.res) + n * a.r_sn + pix * a.res_ld : nullptr;
    si_pix16_store<T, TILES, true>(yp, rp, a.bias, acc, o0 + 4 * g, a.oc, a.y_vec != 0, a.act1, a.act2, a.act_param);
}

// ---- host -----------------------------------------------------------------------------------------------------------------
constexpr uint64_t kGridLimitYZ = 65535;

struct Geometry {
    int th, ph, cw, npos;
    size_t lds;
};

inline int icp_of(const SiBorderConvDesc* d, bool half) {
    const int ve = half ? 8 : 4;
    return (d->ic + ve - 1) / ve * ve;
}

// torch's output extent for the pad p on both sides, or 0
inline int64_t out_extent(int64_t l, int64_t p, int64_t k, int64_t s, int64_t dil) {
    const int64_t e = l + 2 * p - dil * (k - 1) - 1;
    return e < 0 ? 0 : e / s + 1;
}

// the largest live row count whose patch and tables fit LDS
bool geometry_of(const SiBorderConvDesc* d, bool half, Geometry& g) {
    const uint64_t pitch_bytes = half ? (SI_BORDER_KC + SI_BORDER_PAD_F16) * 2 : (SI_BORDER_KC + SI_BORDER_PAD_F32) * 4;
    const uint64_t pw = (uint64_t)(SI_BORDER_TW - 1) * d->sw + (uint64_t)(d->kw - 1) * d->dw + 1;
    const uint64_t cw = (pw + d->sw - 1) / d->sw, npos = cw * d->sw;
    for (int th = SI_BORDER_TH; th >= 1; th /= 2) {
        const uint64_t ph = (uint64_t)(th - 1) * d->sh + (uint64_t)(d->kh - 1) * d->dh + 1;
        const uint64_t bytes = ph * npos * pitch_bytes + 4 * (ph + npos + (uint64_t)d->kw);
        if (ph <= SI_INDEX_LIMIT && npos <= SI_INDEX_LIMIT && bytes <= (uint64_t)SI_BORDER_LDS_BYTES) {
            g.th = th; g.ph = (int)ph; g.cw = (int)cw; g.npos = (int)npos; g.lds = (size_t)bytes;
            return true;
        }
    }
    return false;
}

int pad_limit(int mode, int n) { return mode == SI_PAD_REFLECT ? n - 1 : (mode == SI_PAD_CIRCULAR ? n : INT32_MAX); }

// everything that can be decided without a device and without the pointers: SI_E_BADARG / SI_E_UNSUPPORTED / 0
int check_desc(const SiBorderConvDesc* d, bool half) {
    if (!d) return SI_E_BADARG;
    if (d->n <= 0 || d->ih <= 0 || d->iw <= 0 || d->ic <= 0 || d->oh <= 0 || d->ow <= 0 || d->oc <= 0 || d->kh <= 0 || d->kw <= 0 || d->sh <= 0 ||
        d->sw <= 0 || d->dh <= 0 || d->dw <= 0 || d->groups <= 0 || d->pt < 0 || d->pl < 0)
        return SI_E_BADARG;
    if (d->in_ld < d->ic || d->out_ld < d->oc || (d->has_residual && d->res_ld < d->oc)) return SI_E_BADARG;
    if (d->mode != SI_PAD_REFLECT && d->mode != SI_PAD_REPLICATE && d->mode != SI_PAD_CIRCULAR) return SI_E_BADARG;
    if (out_extent(d->ih, d->pt, d->kh, d->sh, d->dh) != d->oh || out_extent(d->iw, d->pl, d->kw, d->sw, d->dw) != d->ow) return SI_E_BADARG;
    if (d->pt > pad_limit(d->mode, d->ih) || d->pl > pad_limit(d->mode, d->iw)) return SI_E_UNSUPPORTED;
    if (d->groups != 1 || (half && d->ic % 8 != 0)) return SI_E_UNSUPPORTED;
    if (si_view_extent(d->n, d->ih, d->iw, d->in_ld, d->ic) == 0 || si_view_extent(d->n, d->oh, d->ow, d->out_ld, d->oc) == 0) return SI_E_UNSUPPORTED;
    if (d->has_residual && si_view_extent(d->n, d->oh, d->ow, d->res_ld, d->oc) == 0) return SI_E_UNSUPPORTED;
    if ((uint64_t)d->oc * d->kh * d->kw * (uint64_t)icp_of(d, half) > SI_INDEX_LIMIT) return SI_E_UNSUPPORTED;
    // the device forms o s - p + k d, and tile origins rounded up, in 32 bits
    if ((uint64_t)(d->oh + SI_BORDER_TH) * d->sh + (uint64_t)d->kh * d->dh + d->pt > SI_INDEX_LIMIT ||
        (uint64_t)(d->ow + SI_BORDER_TW) * d->sw + (uint64_t)d->kw * d->dw + d->pl > SI_INDEX_LIMIT)
        return SI_E_UNSUPPORTED;
    Geometry g;
    if (!geometry_of(d, half, g)) return SI_E_UNSUPPORTED;
    const uint64_t tiles = (uint64_t)((d->ow + SI_BORDER_TW - 1) / SI_BORDER_TW) * (uint64_t)((d->oh + g.th - 1) / g.th);
    if (tiles > SI_INDEX_LIMIT || (uint64_t)((d->oc + SI_BORDER_OC - 1) / SI_BORDER_OC) > kGridLimitYZ || (uint64_t)d->n > kGridLimitYZ)
        return SI_E_UNSUPPORTED;
    return 0;
}

int check_ptrs(const SiBorderConvDesc* d, const void* x, const void* w, const float* bias, const void* res, const void* y, bool half) {
    if (!x || !w || !y || (d->has_bias && !bias) || (d->has_residual && !res)) return SI_E_BADARG;
    const uint64_t es = half ? 2 : 4;
    const uint64_t y_bytes = si_view_extent(d->n, d->oh, d->ow, d->out_ld, d->oc) * es;
    if (si_ranges_overlap(y, y_bytes, x, si_view_extent(d->n, d->ih, d->iw, d->in_ld, d->ic) * es)) return SI_E_BADARG;
    if (si_ranges_overlap(y, y_bytes, w, (uint64_t)d->oc * d->kh * d->kw * icp_of(d, half) * es)) return SI_E_BADARG;
    if (d->has_bias && si_ranges_overlap(y, y_bytes, bias, (uint64_t)d->oc * 4)) return SI_E_BADARG;
    if (!si_aligned_to(x, es) || !si_aligned_to(y, es) || (d->has_residual && !si_aligned_to(res, es)) || (d->has_bias && !si_aligned_to(bias, 4)))
        return SI_E_UNSUPPORTED;
    if (!si_aligned_to(w, 16)) return SI_E_UNSUPPORTED;   // (a fragment of the image is one 16-byte read)
    return 0;
}

template <typename T>
void launch_tiles(int tiles, dim3 grid, size_t lds, hipStream_t st, const BorderArgs& a) {
    switch (tiles) {
        case 1: hipLaunchKernelGGL((conv_border_kernel<T, 1>), grid, dim3(BD_THREADS), lds, st, a); break;
        case 2: hipLaunchKernelGGL((conv_border_kernel<T, 2>), grid, dim3(BD_THREADS), lds, st, a); break;
        case 3: hipLaunchKernelGGL((conv_border_kernel<T, 3>), grid, dim3(BD_THREADS), lds, st, a); break;
        default: hipLaunchKernelGGL((conv_border_kernel<T, 4>), grid, dim3(BD_THREADS), lds, st, a); break;
    }
}

template <typename T>
int run(const SiBorderConvDesc* d, const void* x, const void* w, const float* bias, const void* res, void* y, si_stream_t stream) {
    constexpr bool half = sizeof(T) == 2;
    int rc = check_desc(d, half);
    if (rc != 0) return rc;
    rc = check_ptrs(d, x, w, bias, res, y, half);
    if (rc != 0) return rc;
    Geometry g;
    geometry_of(d, half, g);
    BorderArgs a;
    memset(&a, 0, sizeof(a));
    a.x = x; a.w = w; a.bias = d->has_bias ? bias : nullptr; a.res = d->has_residual ? res : nullptr; a.y = y;
    a.ih = d->ih; a.iw = d->iw; a.ic = d->ic; a.in_ld = d->in_ld; a.oh = d->oh; a.ow = d->ow; a.oc = d->oc; a.out_ld = d->out_ld; a.res_ld = d->res_ld;
    a.kh = d->kh; a.kw = d->kw; a.sh = d->sh; a.sw = d->sw; a.dh = d->dh; a.dw = d->dw; a.pt = d->pt; a.pl = d->pl; a.mode = d->mode;
    a.icp = icp_of(d, half);
    a.th = g.th; a.ph = g.ph; a.cw = g.cw; a.npos = g.npos;
    a.tiles_x = (d->ow + SI_BORDER_TW - 1) / SI_BORDER_TW;
    a.x_sh = d->iw * d->in_ld;
    a.x_sn = d->ih * a.x_sh;
    a.y_sn = d->oh * d->ow * d->out_ld;
    a.r_sn = d->oh * d->ow * d->res_ld;
    const int ve = half ? 8 : 4;
    a.x_vec = (d->ic % ve == 0 && d->in_ld % ve == 0 && si_aligned_to(x, 16)) ? 1 : 0;
    a.y_vec = (d->out_ld % 4 == 0 && si_aligned_to(y, 4 * sizeof(T))) ? 1 : 0;
    a.act1 = d->act1; a.act2 = d->act2; a.act_param = d->act_param;
    const int oc_tiles = (d->oc + BD_TILE_OC - 1) / BD_TILE_OC;
    const dim3 grid((unsigned)(a.tiles_x * ((d->oh + g.th - 1) / g.th)), (unsigned)((d->oc + SI_BORDER_OC - 1) / SI_BORDER_OC), (unsigned)d->n);
    launch_tiles<T>(oc_tiles < 4 ? oc_tiles : 4, grid, g.lds, (hipStream_t)stream, a);
    SI_HIP_TRY(hipGetLastError());
    return 0;
}

template <typename T>
void pack(const SiBorderConvDesc* d, const float* w_oihw, T* image, int icp) {
    for (int o = 0; o < d->oc; ++o)
        for (int ky = 0; ky < d->kh; ++ky)
            for (int kx = 0; kx < d->kw; ++kx)
                for (int c = 0; c < icp; ++c) {
                    const float v = c < d->ic ? w_oihw[(((size_t)o * d->ic + c) * d->kh + ky) * d->kw + kx] : 0.0f;
                    image[(((size_t)o * d->kh + ky) * d->kw + kx) * icp + c] = (T)v;
                }
}

bool pack_shape_ok(const SiBorderConvDesc* d, bool half) {
    return d && d->ic > 0 && d->oc > 0 && d->kh > 0 && d->kw > 0 && d->groups == 1 && (!half || d->ic % 8 == 0) &&
           (uint64_t)d->oc * d->kh * d->kw * (uint64_t)icp_of(d, half) <= SI_INDEX_LIMIT;
}

}  // namespace

extern "C" {

int si_hip_conv2d_border_supported(const SiBorderConvDesc* d, int half) { return check_desc(d, half != 0) == 0 ? 1 : 0; }

size_t si_hip_conv2d_border_weight_elems(const SiBorderConvDesc* d, int half) {
    if (!pack_shape_ok(d, half != 0)) return 0;
    return (size_t)d->oc * d->kh * d->kw * icp_of(d, half != 0);
}

int si_hip_conv2d_border_pack_weight_host(const SiBorderConvDesc* d, const float* w_oihw, void* w_packed, int half) {
    if (!d || !w_oihw || !w_packed) return SI_E_BADARG;
    if (!pack_shape_ok(d, half != 0)) return SI_E_UNSUPPORTED;
    if (half) pack<_Float16>(d, w_oihw, static_cast<_Float16*>(w_packed), icp_of(d, true));
    else pack<float>(d, w_oihw, static_cast<float*>(w_packed), icp_of(d, false));
    return 0;
}

int si_hip_conv2d_border_f32(const SiBorderConvDesc* d, const float* in, const float* w_packed, const float* bias, const float* residual,
                             float* out, si_stream_t stream) {
    return run<float>(d, in, w_packed, bias, residual, out, stream);
}

int si_hip_conv2d_border_f16(const SiBorderConvDesc* d, const void* in, const void* w_packed, const float* bias, const void* residual,
                             void* out, si_stream_t stream) {
    return run<_Float16>(d, in, w_packed, bias, residual, out, stream);
}

const char* si_hip_conv2d_border_kernel_name(const SiBorderConvDesc* d, const void* in, const void* out, int half) {
    if (check_desc(d, half != 0) != 0 || !in || !out) return "none";
    const size_t es = half ? 2 : 4;
    if (!si_aligned_to(in, es) || !si_aligned_to(out, es)) return "none";
    return half ? "conv_border_kernel<_Float16>" : "conv_border_kernel<float>";
}

int si_hip_conv2d_border_source_index(int mode, int i, int n) {
    if (n <= 0) return SI_BORDER_REFUSED;
    if (mode == SI_PAD_REFLECT ? (i < -(n - 1) || i > 2 * (n - 1)) : mode == SI_PAD_CIRCULAR ? (i < -n || i > 2 * n - 1) : mode != SI_PAD_REPLICATE)
        return SI_BORDER_REFUSED;
    return border_map(mode, i, n);
}

}  // extern "C"
