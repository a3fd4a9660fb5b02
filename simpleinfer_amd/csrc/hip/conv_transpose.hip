// conv_transpose.hip -- nn.ConvTranspose2d (torch semantics, groups = 1) on the gfx950 fp32 matrix cores
// (v_mfma_f32_32x32x2_f32: exact fp32, k-ordered fma chain, as conv_igemm.hip).
//
//   out[n, oy, ox, oc] = act( bias[oc] + sum_{ky,kx,ic} x[n, iy, ix, ic] * W[ic, oc, ky, kx] )
//   over every (iy, ix, ky, kx) with oy = iy*sh - ph + ky*dh, ox = ix*sw - pw + kx*dw.
//
// Gather form, output-stationary: exactly one lane computes and stores each output element, once -- no atomics, no
// zero-fill pass, no col2im scatter-add, so the result is the same from run to run and the launch is safe in a captured
// graph.  Sub-pixel phases: the output pixels with (oy mod sh, ox mod sw) = (ry, rx) all see the same taps,
//   ky in {ky0(ry) + t * step_y},  step_y = sh / gcd(sh, dh),  iy = oy / sh + off0(ry) - t * (dh / gcd(sh, dh))
// (and likewise along x), so every phase is a dense stride-1 implicit GEMM: M = the phase's output pixels, N = Cout,
// K = |taps| * Cin (tap-major, channels inside).  All phases run in one launch (blockIdx.z); a phase without a tap
// (k < s) has K = 0 and stores act(bias).
//
// The one-tap case (kh = sh, kw = sw, no padding, dilation 1, no output padding -- U-Net's 2x2 stride-2 up-conv) has its
// own path: each output pixel has exactly one tap, so the layer is ONE GEMM [N*H*W, Cin] x [Cin, sh*sw*Cout] whose
// column j = (tap, oc) is stored to output pixel (y*sh + ky, x*sw + kx) -- a pixel-shuffle store.
//
// Weights: [kh][kw][oc][icp] (icp = Cin rounded up to 4, zero filled), re-laid once on the host; for the one-tap path
// that is exactly the [sh*sw*Cout][icp] B matrix.
//
// Tile: 64 x 64 per workgroup, four waves as 2 x 2, one 32x32 accumulator per wave, one LDS stage ([row][32 + 4]: 18 KB,
// so many workgroups share a CU) with the next K-tile's global loads in flight during the MFMAs -- the form
// conv_igemm.hip measured fastest for the fp32 MFMA (its 64x64 one-stage tiles).  Fragment reads: one ds_read_b128 per
// lane of A[row][16p + 8h + 4(lane>>5) .. +3]; MFMA j of that group takes element j from A and B alike (a K permutation
// inside the tile, the same products).
#include <hip/hip_runtime.h>

#include <cstdint>

// No contraction: bias add and activation round as written in every instantiation.
#pragma clang fp contract(off)

#include "si_hip.h"
#include "si_hip_internal.h"

namespace {

constexpr int CT_BM = 64, CT_BN = 64, CT_BK = 32, CT_LDL = CT_BK + 4;

struct CtArgs {
    const float* in;
    const float* w;
    const float* bias;
    float* out;
    int n, ih, iw, ic, icp, in_ld;
    int oh, ow, oc, out_ld;
    int kh, kw, sh, sw, ph, pw, dh, dw;
    int step_y, step_x, dly, dlx;   // tap stride inside a phase and the matching input-row step (see the file comment)
    int ncols;                      // GEMM columns: sh*sw*oc (one-tap) or oc
    int m_tiles, n_tiles;
    int act;
    float act_param;
};

// C/D map of the 32x32 tile: col = lane & 31 (GEMM column), row = Mma<32>::row(e) + 4 * (lane >> 5).
// rows[]: the output pixel of each of the workgroup's 64 rows (-1 past M); col_pix: the pixel offset of this lane's
// column (the one-tap path's ky * ow + kx, else 0); o: its output channel.
template <int ACT>
__device__ __forceinline__ void ct_store(const CtArgs& a, const f32x16& acc, const int* rows, int row0, bool live, int o, int col_pix) {
    if (!live) return;
    const float bv = a.bias ? a.bias[o] : 0.0f;
    float* const ob = a.out + o;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int pix = rows[row0 + Mma<32>::row(e)];
        if (pix >= 0) ob[(size_t)(pix + col_pix) * a.out_ld] = si_act<ACT>(acc[e] + bv, a.act_param);
    }
}

template <bool ONE_TAP, bool VEC_A>
__global__ __launch_bounds__(256) void conv_transpose_f32_kernel(const CtArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[(CT_BM + CT_BN) * CT_LDL];
    __shared__ int rows[CT_BM];

    // tile mapping as conv_igemm.hip: the n_tiles workgroups that share one A panel get the same blockIdx % 8 (same XCD / L2)
    const int per_chunk = 8 * a.n_tiles;
    const int chunk = (int)blockIdx.x / per_chunk;
    const int r = (int)blockIdx.x - chunk * per_chunk;
    const int m_tile = chunk * 8 + (r & 7);
    const int n_tile = r >> 3;
    if (m_tile >= a.m_tiles) return;

    // ---- this workgroup's phase (wave-uniform scalar arithmetic)
    const int phase = blockIdx.z;
    const int ry = ONE_TAP ? 0 : phase / a.sw;
    const int rx = ONE_TAP ? 0 : phase - ry * a.sw;
    int prow, pcol, nty = 1, ntx = 1, ky0 = 0, kx0 = 0, offy0 = 0, offx0 = 0;
    if (ONE_TAP) {
        prow = a.ih;
        pcol = a.iw;
    } else {
        prow = ry < a.oh ? (a.oh - ry + a.sh - 1) / a.sh : 0;
        pcol = rx < a.ow ? (a.ow - rx + a.sw - 1) / a.sw : 0;
        // first tap of the phase: the smallest ky with (ry + ph - ky*dh) = 0 (mod sh); the rest follow every step_y
        nty = 0;
        for (int ky = 0; ky < a.step_y && ky < a.kh; ++ky) {
            const int v = ry + a.ph - ky * a.dh;
            if (((v % a.sh) + a.sh) % a.sh == 0) {
                ky0 = ky;
                offy0 = v / a.sh;   // exact
                nty = (a.kh - 1 - ky) / a.step_y + 1;
                break;
            }
        }
        ntx = 0;
        for (int kx = 0; kx < a.step_x && kx < a.kw; ++kx) {
            const int v = rx + a.pw - kx * a.dw;
            if (((v % a.sw) + a.sw) % a.sw == 0) {
                kx0 = kx;
                offx0 = v / a.sw;
                ntx = (a.kw - 1 - kx) / a.step_x + 1;
                break;
            }
        }
    }
    const int M = a.n * prow * pcol;
    const int m0 = m_tile * CT_BM;
    if (m0 >= M) return;
    const int n0 = n_tile * CT_BN;
    const int K = nty * ntx * a.icp;

    const int tid = threadIdx.x;
    const int kv = tid & 7;   // 4-wide K vector of the 32-wide K-tile
    const int r0 = tid >> 3;  // base row 0..31

    // ---- output pixel of each tile row
    if (tid < CT_BM) {
        const int m = m0 + tid;
        int pix = -1;
        if (m < M) {
            const int img = m / (prow * pcol);
            const int rem = m - img * prow * pcol;
            const int j = rem / pcol;
            const int i = rem - j * pcol;
            pix = ONE_TAP ? (img * a.oh + j * a.sh) * a.ow + i * a.sw : (img * a.oh + ry + a.sh * j) * a.ow + rx + a.sw * i;
        }
        rows[tid] = pix;
    }

    // ---- per-thread A rows (fixed for the whole K loop)
    int a_img[2], a_j[2], a_i[2];
    bool a_ok[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int m = m0 + r0 + 32 * q;
        a_ok[q] = m < M;
        const int mm = a_ok[q] ? m : 0;
        const int img = mm / (prow * pcol);
        const int rem = mm - img * prow * pcol;
        a_img[q] = img;
        a_j[q] = rem / pcol;
        a_i[q] = rem - a_j[q] * pcol;
    }

    f32x4 pa[2], pb[2];
    auto load_tile = [&](int kt) {
        const int k = kt * CT_BK + kv * 4;
        const bool kvalid = k < K;
        int t = 0, c = k;
        if (!ONE_TAP) {
            t = k / a.icp;
            c = k - t * a.icp;
        }
        const int ty = t / (ntx > 0 ? ntx : 1);
        const int tx = t - ty * ntx;
        const int dy = offy0 - ty * a.dly, dx = offx0 - tx * a.dlx;
        const int wtap = ONE_TAP ? 0 : (ky0 + ty * a.step_y) * a.kw + (kx0 + tx * a.step_x);
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int y = a_j[q] + dy, x = a_i[q] + dx;
            const bool ok = kvalid && a_ok[q] && c < a.ic && (ONE_TAP || ((unsigned)y < (unsigned)a.ih && (unsigned)x < (unsigned)a.iw));
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (ok) {
                const float* p = a.in + (size_t)((a_img[q] * a.ih + y) * a.iw + x) * a.in_ld + c;
                if (VEC_A) {
                    v = *reinterpret_cast<const f32x4*>(p);
                } else {
                    v.x = p[0];
                    if (c + 1 < a.ic) v.y = p[1];
                    if (c + 2 < a.ic) v.z = p[2];
                    if (c + 3 < a.ic) v.w = p[3];
                }
            }
            pa[q] = v;
        }
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int col = n0 + r0 + 32 * q;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (kvalid && col < a.ncols) v = *reinterpret_cast<const f32x4*>(a.w + ((size_t)wtap * a.oc + col) * a.icp + c);
            pb[q] = v;
        }
    };

    const int wave = tid >> 6, lane = tid & 63;
    const int wm = wave >> 1, wn = wave & 1;
    const int l31 = lane & 31, lh = lane >> 5;

    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.0f;

    const int nk = (K + CT_BK - 1) / CT_BK;
    if (nk > 0) load_tile(0);
    for (int kt = 0; kt < nk; ++kt) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            *reinterpret_cast<f32x4*>(lds + (r0 + 32 * q) * CT_LDL + kv * 4) = pa[q];
            *reinterpret_cast<f32x4*>(lds + (CT_BM + r0 + 32 * q) * CT_LDL + kv * 4) = pb[q];
        }
        __syncthreads();
        if (kt + 1 < nk) load_tile(kt + 1);   // in flight during the MFMAs
        const float* As = lds + (wm * 32 + l31) * CT_LDL + lh * 4;
        const float* Bs = lds + (CT_BM + wn * 32 + l31) * CT_LDL + lh * 4;
#pragma unroll
        for (int p = 0; p < CT_BK / 16; ++p) {
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
    if (nk == 0) __syncthreads();   // (rows[] is read below)

    // ---- epilogue
    const int col = n0 + wn * 32 + l31;
    const bool live = col < a.ncols;
    int o = col, col_pix = 0;
    if (ONE_TAP && live) {
        const int tap = col / a.oc;
        o = col - tap * a.oc;
        const int ky = tap / a.sw;
        col_pix = ky * a.ow + (tap - ky * a.sw);
    }
    const int row0 = wm * 32 + 4 * lh;
    switch (a.act) {
        case SI_ACT_RELU: ct_store<SI_ACT_RELU>(a, acc, rows, row0, live, o, col_pix); break;
        case SI_ACT_SILU: ct_store<SI_ACT_SILU>(a, acc, rows, row0, live, o, col_pix); break;
        case SI_ACT_SIGMOID: ct_store<SI_ACT_SIGMOID>(a, acc, rows, row0, live, o, col_pix); break;
        case SI_ACT_HARDSIGMOID: ct_store<SI_ACT_HARDSIGMOID>(a, acc, rows, row0, live, o, col_pix); break;
        case SI_ACT_HARDSWISH: ct_store<SI_ACT_HARDSWISH>(a, acc, rows, row0, live, o, col_pix); break;
        case SI_ACT_LEAKYRELU: ct_store<SI_ACT_LEAKYRELU>(a, acc, rows, row0, live, o, col_pix); break;
        default: ct_store<SI_ACT_NONE>(a, acc, rows, row0, live, o, col_pix); break;
    }
}

int ct_gcd(int x, int y) {
    while (y) {
        const int t = x % y;
        x = y;
        y = t;
    }
    return x;
}

int ct_icp(const SiConvTranspose2dDesc* d) { return (d->ic + 3) & ~3; }

bool ct_one_tap(const SiConvTranspose2dDesc* d) {
    return d->kh == d->sh && d->kw == d->sw && d->ph == 0 && d->pw == 0 && d->dh == 1 && d->dw == 1 && d->oph == 0 && d->opw == 0;
}

// 0, or why the descriptor is refused (checked before any device call)
int ct_check(const SiConvTranspose2dDesc* d) {
    if (!d) return SI_E_BADARG;
    if (d->n <= 0 || d->ih <= 0 || d->iw <= 0 || d->ic <= 0 || d->oc <= 0 || d->in_ld < d->ic || d->out_ld < d->oc) return SI_E_BADARG;
    if (d->kh <= 0 || d->kw <= 0 || d->sh <= 0 || d->sw <= 0 || d->dh <= 0 || d->dw <= 0 || d->ph < 0 || d->pw < 0 || d->oph < 0 || d->opw < 0)
        return SI_E_BADARG;
    if (d->groups != 1) return SI_E_UNSUPPORTED;
    // torch's rule: output padding smaller than either stride or dilation
    if (d->oph >= (d->sh > d->dh ? d->sh : d->dh) || d->opw >= (d->sw > d->dw ? d->sw : d->dw)) return SI_E_BADARG;
    const long long oh = (long long)(d->ih - 1) * d->sh - 2LL * d->ph + (long long)d->dh * (d->kh - 1) + d->oph + 1;
    const long long ow = (long long)(d->iw - 1) * d->sw - 2LL * d->pw + (long long)d->dw * (d->kw - 1) + d->opw + 1;
    if (oh != d->oh || ow != d->ow || oh <= 0 || ow <= 0) return SI_E_BADARG;
    if (d->act < SI_ACT_NONE || d->act > SI_ACT_LEAKYRELU) return SI_E_UNSUPPORTED;
    // pixel indices are 32-bit in the kernel
    if ((long long)d->n * d->oh * d->ow >= (1LL << 31) || (long long)d->n * d->ih * d->iw >= (1LL << 31)) return SI_E_UNSUPPORTED;
    if ((long long)d->kh * d->kw * d->oc * ct_icp(d) >= (1LL << 31)) return SI_E_UNSUPPORTED;
    return 0;
}

}  // namespace

extern "C" size_t si_hip_conv_transpose2d_weight_elems(const SiConvTranspose2dDesc* d) {
    if (!d || d->groups != 1 || d->ic <= 0 || d->oc <= 0 || d->kh <= 0 || d->kw <= 0) return 0;
    return (size_t)d->kh * d->kw * d->oc * ct_icp(d);
}

extern "C" int si_hip_conv_transpose2d_pack_weight_host(const SiConvTranspose2dDesc* d, const float* w_iohw, float* w_packed) {
    if (!d || !w_iohw || !w_packed) return SI_E_BADARG;
    if (d->groups != 1) return SI_E_UNSUPPORTED;
    if (d->ic <= 0 || d->oc <= 0 || d->kh <= 0 || d->kw <= 0) return SI_E_BADARG;
    const int icp = ct_icp(d), taps = d->kh * d->kw;
    // [ic][oc][kh][kw] -> [kh][kw][oc][icp]
    for (int t = 0; t < taps; ++t)
        for (int o = 0; o < d->oc; ++o) {
            float* dst = w_packed + ((size_t)t * d->oc + o) * icp;
            for (int c = 0; c < icp; ++c) dst[c] = c < d->ic ? w_iohw[((size_t)c * d->oc + o) * taps + t] : 0.0f;
        }
    return 0;
}

extern "C" const char* si_hip_conv_transpose2d_kernel_name(const SiConvTranspose2dDesc* d) {
    if (!d) return "";
    const bool vec = d->ic % 4 == 0 && d->in_ld % 4 == 0;   // (and a 16-byte aligned input: the engine's tensors are)
    if (ct_one_tap(d)) return vec ? "conv_transpose_f32_kernel<true, true>" : "conv_transpose_f32_kernel<true, false>";
    return vec ? "conv_transpose_f32_kernel<false, true>" : "conv_transpose_f32_kernel<false, false>";
}

extern "C" int si_hip_conv_transpose2d_f32(const SiConvTranspose2dDesc* d, const float* in, const float* w_packed, const float* bias, float* out,
                                           si_stream_t stream) {
    if (const int rc = ct_check(d)) return rc;
    if (!in || !w_packed || !out || (d->has_bias && !bias)) return SI_E_BADARG;
    if (!si_aligned_to(w_packed, 16)) return SI_E_BADARG;
    CtArgs a{};
    a.in = in; a.w = w_packed; a.bias = d->has_bias ? bias : nullptr; a.out = out;
    a.n = d->n; a.ih = d->ih; a.iw = d->iw; a.ic = d->ic; a.icp = ct_icp(d); a.in_ld = d->in_ld;
    a.oh = d->oh; a.ow = d->ow; a.oc = d->oc; a.out_ld = d->out_ld;
    a.kh = d->kh; a.kw = d->kw; a.sh = d->sh; a.sw = d->sw; a.ph = d->ph; a.pw = d->pw; a.dh = d->dh; a.dw = d->dw;
    const int gy = ct_gcd(d->sh, d->dh), gx = ct_gcd(d->sw, d->dw);
    a.step_y = d->sh / gy; a.dly = d->dh / gy;
    a.step_x = d->sw / gx; a.dlx = d->dw / gx;
    a.act = d->act; a.act_param = d->act_param;
    const bool one = ct_one_tap(d);
    long long mmax;
    int phases;
    if (one) {
        a.ncols = d->sh * d->sw * d->oc;
        mmax = (long long)d->n * d->ih * d->iw;
        phases = 1;
    } else {
        a.ncols = d->oc;
        mmax = (long long)d->n * ((d->oh + d->sh - 1) / d->sh) * ((d->ow + d->sw - 1) / d->sw);
        phases = d->sh * d->sw;
    }
    a.m_tiles = (int)((mmax + CT_BM - 1) / CT_BM);
    a.n_tiles = (a.ncols + CT_BN - 1) / CT_BN;
    const long long gx_blocks = (long long)((a.m_tiles + 7) / 8) * 8 * a.n_tiles;
    if (gx_blocks >= (1LL << 31) || phases > 65535) return SI_E_UNSUPPORTED;
    const bool vec = d->ic % 4 == 0 && d->in_ld % 4 == 0 && si_aligned_to(in, 16);
    const dim3 grid((unsigned)gx_blocks, 1, (unsigned)phases);
    hipStream_t s = (hipStream_t)stream;
    if (one) {
        if (vec) hipLaunchKernelGGL((conv_transpose_f32_kernel<true, true>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((conv_transpose_f32_kernel<true, false>), grid, dim3(256), 0, s, a);
    } else {
        if (vec) hipLaunchKernelGGL((conv_transpose_f32_kernel<false, true>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((conv_transpose_f32_kernel<false, false>), grid, dim3(256), 0, s, a);
    }
    return (int)hipGetLastError();
}
