// deform_conv.hip -- torchvision.ops.deform_conv2d (DCNv1 / DCNv2; the rule: include/si_deform.h) on the gfx950 fp32 matrix cores
// (v_mfma_f32_32x32x2_f32: exact fp32, k-ordered fma chain, as conv_igemm.hip and conv_transpose.hip).
//
// An implicit GEMM per weight group: M = n * oh * ow output pixels, N = oc / groups, K = kh * kw * cgp (tap-major, the channels of the weight
// group inside, cgp = ic / groups rounded up to 4 and zero filled in the weight image).  The B operand is conv_transpose.hip's: rows of the
// packed weight [tap][oc][cgp].  The A operand is produced by the gather: for a tile row (an output pixel), a tap and an offset group the
// two offsets and the mask give a sampling record -- four corner element offsets (or "absent") and four weights -- and every 4-channel
// vector of that (row, tap) is four corner loads, the blend in the order of the rule, the mask multiply, and a 16-byte LDS store.  The eight
// threads that share a row each make the record from the offsets (which sit in L1 after the first of them) and keep it in registers for the
// K-tiles of that tap; nothing is staged in LDS.
//
// Tile: conv_transpose.hip's -- 64 x 64 per workgroup, four waves as 2 x 2, one 32x32 accumulator per wave, one LDS stage ([row][32 + 4]),
// the next K-tile's gather in flight during the MFMAs, the same XCD-aware tile mapping; the weight group is blockIdx.z.  Output-stationary:
// exactly one lane computes and stores each output element, once -- no workspace, no atomics, the same bits from run to run.
#include <hip/hip_runtime.h>

#include <cstdint>

// No contraction: the coordinate add, the blend, the mask multiply, bias add and activation round as written in every instantiation.
#pragma clang fp contract(off)

#include "si_deform.h"
#include "si_hip_internal.h"

namespace {

constexpr int DC_BM = 64, DC_BN = 64, DC_BK = 32, DC_LDL = DC_BK + 4;

struct DcArgs {
    const float* in;
    const float* off;
    const float* mask;   // null: DCNv1
    const float* w;
    const float* bias;
    float* out;
    int n, ih, iw, ic, in_ld;
    int oh, ow, oc, out_ld, off_ld, mask_ld;
    int kh, kw, sh, sw, ph, pw, dh, dw;
    int cg, cgp, cog, cpo;   // ic / groups, that rounded up to 4, oc / groups, ic / offset_groups
    int m_tiles, n_tiles;
    int act;
    float act_param;
};

// C/D map of the 32x32 tile: col = lane & 31 (GEMM column), row = Mma<32>::row(e) + 4 * (lane >> 5).
// rows[]: the output pixel of each of the workgroup's 64 rows (-1 past M); o: this lane's output channel.
template <int ACT>
__device__ __forceinline__ void dc_store(const DcArgs& a, const f32x16& acc, const int* rows, int row0, bool live, int o) {
    if (!live) return;
    const float bv = a.bias ? a.bias[o] : 0.0f;
    float* const ob = a.out + o;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int pix = rows[row0 + Mma<32>::row(e)];
        if (pix >= 0) ob[(size_t)pix * a.out_ld] = si_act<ACT>(acc[e] + bv, a.act_param);
    }
}

// The sampling record of one (output pixel, tap, offset group).  kind: 0 the sample is 0, 1 the blend, 2 NaN.  o0 .. o3: the element offset of
// each corner's pixel (channel 0), -1 for a corner outside the image; w0 .. w3: the corner weights; m: the mask value (1 without a mask).
struct DcRecord {
    int kind;
    int o0, o1, o2, o3;
    f32x4 w;   // w0 .. w3
    float m;
};

// pix: the output pixel (its index into offset / mask), img: its image, (by, bx): ho * sh - ph + i * dh and the like, ch: the tap's channel
// og * taps + t of the mask (the offsets sit at 2 ch and 2 ch + 1)
__device__ __forceinline__ DcRecord dc_record(const DcArgs& a, int pix, int img, int by, int bx, int ch) {
    DcRecord r;
    const float* const po = a.off + (size_t)pix * a.off_ld + 2 * ch;
    const float y = (float)by + po[0];
    const float x = (float)bx + po[1];
    r.m = a.mask ? a.mask[(size_t)pix * a.mask_ld + ch] : 1.0f;
    const bool nan = y != y || x != x;
    const bool inside = y > -1.0f && y < (float)a.ih && x > -1.0f && x < (float)a.iw;   // (false for a NaN and for +-Inf)
    r.kind = nan ? 2 : (inside ? 1 : 0);
    // in range: -1 < y < ih, so floor(y) is in [-1, ih - 1] and converts exactly; out of range nothing below is used
    const float ys = inside ? y : 0.0f, xs = inside ? x : 0.0f;
    const float fy = floorf(ys), fx = floorf(xs);
    const int hl = (int)fy, wl = (int)fx;
    const float lh = ys - fy, lw = xs - fx;
    const float hh = 1.0f - lh, hw = 1.0f - lw;
    r.w.x = hh * hw; r.w.y = hh * lw; r.w.z = lh * hw; r.w.w = lh * lw;
    const bool t_ok = inside && hl >= 0, b_ok = inside && hl + 1 <= a.ih - 1, l_ok = wl >= 0, r_ok = wl + 1 <= a.iw - 1;
    const int base = ((img * a.ih + hl) * a.iw + wl) * a.in_ld;   // (only ever used through a corner that is inside)
    r.o0 = t_ok && l_ok ? base : -1;
    r.o1 = t_ok && r_ok ? base + a.in_ld : -1;
    r.o2 = b_ok && l_ok ? base + a.iw * a.in_ld : -1;
    r.o3 = b_ok && r_ok ? base + (a.iw + 1) * a.in_ld : -1;
    return r;
}

__device__ __forceinline__ float dc_nan() { return __builtin_nanf(""); }

// one channel of the blend, in the order of the rule; an absent corner contributes exactly 0 and is not read
__device__ __forceinline__ float dc_sample1(const DcArgs& a, const DcRecord& r, int c) {
    const float t0 = r.o0 >= 0 ? r.w.x * a.in[r.o0 + c] : 0.0f;
    const float t1 = r.o1 >= 0 ? r.w.y * a.in[r.o1 + c] : 0.0f;
    const float t2 = r.o2 >= 0 ? r.w.z * a.in[r.o2 + c] : 0.0f;
    const float t3 = r.o3 >= 0 ? r.w.w * a.in[r.o3 + c] : 0.0f;
    const float v = r.m * (((t0 + t1) + t2) + t3);
    return r.kind == 2 ? dc_nan() : (r.kind == 1 ? v : 0.0f);
}

__device__ __forceinline__ f32x4 dc_corner4(const DcArgs& a, int o, float w, int c) {
    f32x4 t = {0.f, 0.f, 0.f, 0.f};
    if (o >= 0) t = w * *reinterpret_cast<const f32x4*>(a.in + o + c);
    return t;
}

// four channels of one offset group
__device__ __forceinline__ f32x4 dc_sample4(const DcArgs& a, const DcRecord& r, int c) {
    const int kind = r.kind;
    const f32x4 t0 = dc_corner4(a, r.o0, r.w.x, c);
    const f32x4 t1 = dc_corner4(a, r.o1, r.w.y, c);
    const f32x4 t2 = dc_corner4(a, r.o2, r.w.z, c);
    const f32x4 t3 = dc_corner4(a, r.o3, r.w.w, c);
    const f32x4 b = r.m * (((t0 + t1) + t2) + t3);
    const float f = kind == 2 ? dc_nan() : 0.0f;
    f32x4 v;
    v.x = kind == 1 ? b.x : f;
    v.y = kind == 1 ? b.y : f;
    v.z = kind == 1 ? b.z : f;
    v.w = kind == 1 ? b.w : f;
    return v;
}

template <bool VEC_A>
__global__ __launch_bounds__(256) void deform_conv_f32_kernel(const DcArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[(DC_BM + DC_BN) * DC_LDL];
    __shared__ int rows[DC_BM];

    // tile mapping as conv_igemm.hip: the n_tiles workgroups that share one A panel get the same blockIdx % 8 (same XCD / L2)
    const int per_chunk = 8 * a.n_tiles;
    const int chunk = (int)blockIdx.x / per_chunk;
    const int r = (int)blockIdx.x - chunk * per_chunk;
    const int m_tile = chunk * 8 + (r & 7);
    const int n_tile = r >> 3;
    if (m_tile >= a.m_tiles) return;

    const int g = blockIdx.z;   // weight group
    const int opix = a.oh * a.ow;
    const int M = a.n * opix;
    const int m0 = m_tile * DC_BM;
    const int n0 = n_tile * DC_BN;
    const int taps = a.kh * a.kw;
    const int K = taps * a.cgp;

    const int tid = threadIdx.x;
    const int kv = tid & 7;   // 4-wide K vector of the 32-wide K-tile
    const int r0 = tid >> 3;  // base row 0..31

    if (tid < DC_BM) rows[tid] = m0 + tid < M ? m0 + tid : -1;

    // ---- per-thread A rows (fixed for the whole K loop)
    int a_pix[2], a_img[2], a_by[2], a_bx[2];
    bool a_ok[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int m = m0 + r0 + 32 * q;
        a_ok[q] = m < M;
        const int mm = a_ok[q] ? m : 0;
        const int img = mm / opix;
        const int rem = mm - img * opix;
        const int ho = rem / a.ow;
        a_pix[q] = mm;
        a_img[q] = img;
        a_by[q] = ho * a.sh - a.ph;
        a_bx[q] = (rem - ho * a.ow) * a.sw - a.pw;
    }

    // VEC_A: the records of this thread's two rows for the (tap, offset group) it met last.  A thread's channel vector walks the channels of one
    // tap over cgp / 32 K-tiles, so with 128 channels a record serves four tiles (the same values as recomputing it: the same arithmetic)
    DcRecord rec0 = {}, rec1 = {};
    int rec_ch = -1;
    f32x4 pa[2], pb[2];
    auto load_tile = [&](int kt) {
        const int k = kt * DC_BK + kv * 4;
        const bool kvalid = k < K;
        const int t = kvalid ? k / a.cgp : 0;
        const int c = k - t * a.cgp;      // channel inside the weight group
        const int ti = t / a.kw;
        const int tj = t - ti * a.kw;
        const int cglob = g * a.cg + c;   // channel of x
        if (VEC_A && kvalid && c < a.cg) {
            // cg % 4 == 0 and cpo % 4 == 0: the four channels exist and share an offset group
            const int ch = (cglob / a.cpo) * taps + t;
            if (ch != rec_ch) {   // (a row past M has pixel 0: its record is made and never used)
                rec0 = dc_record(a, a_pix[0], a_img[0], a_by[0] + ti * a.dh, a_bx[0] + tj * a.dw, ch);
                rec1 = dc_record(a, a_pix[1], a_img[1], a_by[1] + ti * a.dh, a_bx[1] + tj * a.dw, ch);
                rec_ch = ch;
            }
        }
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (kvalid && a_ok[q] && c < a.cg) {
                const int by = a_by[q] + ti * a.dh, bx = a_bx[q] + tj * a.dw;
                if (VEC_A) {
                    v = dc_sample4(a, q == 0 ? rec0 : rec1, cglob);
                } else {
                    int og = cglob / a.cpo;
                    DcRecord rec = dc_record(a, a_pix[q], a_img[q], by, bx, og * taps + t);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        if (c + e >= a.cg) break;
                        const int oge = (cglob + e) / a.cpo;
                        if (oge != og) {   // the vector straddles two offset groups
                            og = oge;
                            rec = dc_record(a, a_pix[q], a_img[q], by, bx, og * taps + t);
                        }
                        v[e] = dc_sample1(a, rec, cglob + e);
                    }
                }
            }
            pa[q] = v;
        }
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int col = n0 + r0 + 32 * q;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (kvalid && col < a.cog) v = *reinterpret_cast<const f32x4*>(a.w + ((size_t)t * a.oc + g * a.cog + col) * a.cgp + c);
            pb[q] = v;
        }
    };

    const int wave = tid >> 6, lane = tid & 63;
    const int wm = wave >> 1, wn = wave & 1;
    const int l31 = lane & 31, lh = lane >> 5;

    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.0f;

    const int nk = (K + DC_BK - 1) / DC_BK;
    load_tile(0);   // (K >= 4: nk >= 1)
    for (int kt = 0; kt < nk; ++kt) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            *reinterpret_cast<f32x4*>(lds + (r0 + 32 * q) * DC_LDL + kv * 4) = pa[q];
            *reinterpret_cast<f32x4*>(lds + (DC_BM + r0 + 32 * q) * DC_LDL + kv * 4) = pb[q];
        }
        __syncthreads();
        if (kt + 1 < nk) load_tile(kt + 1);   // in flight during the MFMAs
        const float* As = lds + (wm * 32 + l31) * DC_LDL + lh * 4;
        const float* Bs = lds + (DC_BM + wn * 32 + l31) * DC_LDL + lh * 4;
#pragma unroll
        for (int p = 0; p < DC_BK / 16; ++p) {
            f32x4 fa[2], fb[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                fa[h] = *reinterpret_cast<const f32x4*>(As + p * 16 + h * 8);
                fb[h] = *reinterpret_cast<const f32x4*>(Bs + p * 16 + h * 8);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int h = 0; h < 2; ++h) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[h][j], fb[h][j], acc, 0, 0, 0);
        }
        __syncthreads();
    }

    // ---- epilogue
    const int col = n0 + wn * 32 + l31;
    const bool live = col < a.cog;
    const int o = g * a.cog + col;
    const int row0 = wm * 32 + 4 * lh;
    switch (a.act) {
        case SI_ACT_RELU: dc_store<SI_ACT_RELU>(a, acc, rows, row0, live, o); break;
        case SI_ACT_SILU: dc_store<SI_ACT_SILU>(a, acc, rows, row0, live, o); break;
        case SI_ACT_SIGMOID: dc_store<SI_ACT_SIGMOID>(a, acc, rows, row0, live, o); break;
        case SI_ACT_HARDSIGMOID: dc_store<SI_ACT_HARDSIGMOID>(a, acc, rows, row0, live, o); break;
        case SI_ACT_HARDSWISH: dc_store<SI_ACT_HARDSWISH>(a, acc, rows, row0, live, o); break;
        case SI_ACT_LEAKYRELU: dc_store<SI_ACT_LEAKYRELU>(a, acc, rows, row0, live, o); break;
        default: dc_store<SI_ACT_NONE>(a, acc, rows, row0, live, o); break;
    }
}

int dc_cgp(const SiDeformConv2dDesc* d) { return (d->ic / d->groups + 3) & ~3; }

// what the weight functions need of the descriptor
bool dc_weight_ok(const SiDeformConv2dDesc* d) {
    return d && d->ic > 0 && d->oc > 0 && d->kh > 0 && d->kw > 0 && d->groups > 0 && d->ic % d->groups == 0 && d->oc % d->groups == 0;
}

// 0, or why the descriptor is refused (checked before any device call)
int dc_check(const SiDeformConv2dDesc* d) {
    if (!d) return SI_E_BADARG;
    if (d->n <= 0 || d->ih <= 0 || d->iw <= 0 || d->ic <= 0 || d->oc <= 0 || d->oh <= 0 || d->ow <= 0) return SI_E_BADARG;
    if (d->kh <= 0 || d->kw <= 0 || d->sh <= 0 || d->sw <= 0 || d->dh <= 0 || d->dw <= 0 || d->ph < 0 || d->pw < 0) return SI_E_BADARG;
    if (d->groups <= 0 || d->offset_groups <= 0) return SI_E_BADARG;
    if (d->ic % d->groups != 0 || d->oc % d->groups != 0 || d->ic % d->offset_groups != 0) return SI_E_BADARG;
    const long long taps = (long long)d->kh * d->kw;
    const long long off_c = 2LL * d->offset_groups * taps, mask_c = (long long)d->offset_groups * taps;
    if (d->in_ld < d->ic || d->out_ld < d->oc || d->off_ld < off_c || (d->has_mask && d->mask_ld < mask_c)) return SI_E_BADARG;
    const long long eh = (long long)d->ih + 2LL * d->ph - (long long)d->dh * (d->kh - 1) - 1;
    const long long ew = (long long)d->iw + 2LL * d->pw - (long long)d->dw * (d->kw - 1) - 1;
    if (eh < 0 || ew < 0 || eh / d->sh + 1 != d->oh || ew / d->sw + 1 != d->ow) return SI_E_BADARG;
    if (d->act < SI_ACT_NONE || d->act > SI_ACT_LEAKYRELU) return SI_E_UNSUPPORTED;
    // element offsets are 32-bit in the kernel
    const long long ipix = (long long)d->n * d->ih * d->iw, opix = (long long)d->n * d->oh * d->ow;
    if (ipix > (long long)SI_INDEX_LIMIT || opix > (long long)SI_INDEX_LIMIT) return SI_E_UNSUPPORTED;
    if (ipix * d->in_ld > (long long)SI_INDEX_LIMIT || opix * d->out_ld > (long long)SI_INDEX_LIMIT || opix * d->off_ld > (long long)SI_INDEX_LIMIT ||
        (d->has_mask && opix * d->mask_ld > (long long)SI_INDEX_LIMIT))
        return SI_E_UNSUPPORTED;
    if (taps * d->oc * dc_cgp(d) > (long long)SI_INDEX_LIMIT) return SI_E_UNSUPPORTED;
    const long long m_tiles = (opix + DC_BM - 1) / DC_BM, n_tiles = (d->oc / d->groups + DC_BN - 1) / DC_BN;
    if ((m_tiles + 7) / 8 * 8 * n_tiles > (long long)SI_INDEX_LIMIT || d->groups > 65535) return SI_E_UNSUPPORTED;
    return 0;
}

// the pointers: null, and `out` intersecting an input
int dc_check_ptrs(const SiDeformConv2dDesc* d, const void* x, const void* offset, const void* mask, const void* out) {
    if (!x || !offset || !out || (d->has_mask && !mask)) return SI_E_BADARG;
    const uint64_t ipix = (uint64_t)d->n * d->ih * d->iw, opix = (uint64_t)d->n * d->oh * d->ow;
    const uint64_t taps = (uint64_t)d->kh * d->kw;
    auto extent = [](uint64_t pixels, uint64_t ld, uint64_t c) { return ((pixels - 1) * ld + c) * sizeof(float); };
    const uint64_t out_bytes = extent(opix, d->out_ld, d->oc);
    const void* const in[3] = {x, offset, d->has_mask ? mask : nullptr};
    const uint64_t bytes[3] = {extent(ipix, d->in_ld, d->ic), extent(opix, d->off_ld, 2 * d->offset_groups * taps),
                               d->has_mask ? extent(opix, d->mask_ld, d->offset_groups * taps) : 0};
    for (int i = 0; i < 3; ++i)
        if (in[i] && si_ranges_overlap(in[i], bytes[i], out, out_bytes)) return SI_E_BADARG;
    return 0;
}

bool dc_vec(const SiDeformConv2dDesc* d, const void* x) {
    return d->ic % 4 == 0 && d->in_ld % 4 == 0 && (d->ic / d->groups) % 4 == 0 && (d->ic / d->offset_groups) % 4 == 0 &&
           si_aligned_to(x, 16);
}

}  // namespace

extern "C" size_t si_hip_deform_conv2d_weight_elems(const SiDeformConv2dDesc* d) {
    if (!dc_weight_ok(d)) return 0;
    return (size_t)d->kh * d->kw * d->oc * dc_cgp(d);
}

extern "C" int si_hip_deform_conv2d_pack_weight_host(const SiDeformConv2dDesc* d, const float* w_oihw, float* w_packed) {
    if (!dc_weight_ok(d) || !w_oihw || !w_packed) return SI_E_BADARG;
    const int cg = d->ic / d->groups, cgp = dc_cgp(d), taps = d->kh * d->kw;
    // [oc][cg][kh][kw] -> [kh][kw][oc][cgp]
    for (int t = 0; t < taps; ++t)
        for (int o = 0; o < d->oc; ++o) {
            float* dst = w_packed + ((size_t)t * d->oc + o) * cgp;
            for (int c = 0; c < cgp; ++c) dst[c] = c < cg ? w_oihw[((size_t)o * cg + c) * taps + t] : 0.0f;
        }
    return 0;
}

extern "C" const char* si_hip_deform_conv2d_kernel_name(const SiDeformConv2dDesc* d, const void* x, const void* offset, const void* mask,
                                                        const void* out) {
    if (dc_check(d) != 0 || dc_check_ptrs(d, x, offset, mask, out) != 0) return "none";
    return dc_vec(d, x) ? "deform_conv_f32_kernel<true>" : "deform_conv_f32_kernel<false>";
}

extern "C" int si_hip_deform_conv2d_f32(const SiDeformConv2dDesc* d, const float* x, const float* offset, const float* mask, const float* w_packed,
                                        const float* bias, float* out, si_stream_t stream) {
    if (const int rc = dc_check(d)) return rc;
    if (const int rc = dc_check_ptrs(d, x, offset, mask, out)) return rc;
    if (!w_packed || (d->has_bias && !bias)) return SI_E_BADARG;
    if (!si_aligned_to(w_packed, 16)) return SI_E_BADARG;
    DcArgs a{};
    a.in = x; a.off = offset; a.mask = d->has_mask ? mask : nullptr; a.w = w_packed; a.bias = d->has_bias ? bias : nullptr; a.out = out;
    a.n = d->n; a.ih = d->ih; a.iw = d->iw; a.ic = d->ic; a.in_ld = d->in_ld;
    a.oh = d->oh; a.ow = d->ow; a.oc = d->oc; a.out_ld = d->out_ld; a.off_ld = d->off_ld; a.mask_ld = d->mask_ld;
    a.kh = d->kh; a.kw = d->kw; a.sh = d->sh; a.sw = d->sw; a.ph = d->ph; a.pw = d->pw; a.dh = d->dh; a.dw = d->dw;
    a.cg = d->ic / d->groups; a.cgp = dc_cgp(d); a.cog = d->oc / d->groups; a.cpo = d->ic / d->offset_groups;
    a.act = d->act; a.act_param = d->act_param;
    const long long opix = (long long)d->n * d->oh * d->ow;
    a.m_tiles = (int)((opix + DC_BM - 1) / DC_BM);
    a.n_tiles = (a.cog + DC_BN - 1) / DC_BN;
    const long long gx_blocks = (long long)((a.m_tiles + 7) / 8) * 8 * a.n_tiles;
    const dim3 grid((unsigned)gx_blocks, 1, (unsigned)d->groups);
    hipStream_t s = (hipStream_t)stream;
    if (dc_vec(d, x)) hipLaunchKernelGGL((deform_conv_f32_kernel<true>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((deform_conv_f32_kernel<false>), grid, dim3(256), 0, s, a);
    return (int)hipGetLastError();
}
