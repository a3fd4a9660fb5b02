// groupnorm.hip -- nn.GroupNorm / nn.InstanceNorm2d in eval mode (include/si_norm.h) on NHWC fp32 and fp16 tensors with pixel
// strides on both sides.  The statistics come from the activation itself, per image and group, on every forward: this is the
// project's reduction kernel.
//
//   mean, var over the h * w * cg elements of (n, g);   y = act((x - mean) * (rsqrt(var + eps) * gamma[ch]) + beta[ch])
//
// Work unit: a TILE = a range of pixels of one image x a chunk of WHOLE groups (channels [g0 * cg, (g0 + gn) * cg), the chunk
// length a multiple of the channel vector), one workgroup of 256 threads per tile.  Thread t owns channel vector tv = t % VPB
// and pixel lane pl = t / VPB (VPB = vectors per pixel of the chunk, at most 256; PL = min(256 / VPB, 64) pixel lanes) and
// walks the pixels pl, pl + PL, ... of the tile.  A vector may straddle a group boundary (cg = 3): statistics are kept PER
// CHANNEL until step 3, so every channel lands in its own group.
//
//   1. per lane and channel: Welford's update over the lane's pixels (fp32; count, mean, M2)
//   2. per channel: the PL lane partials -- two runs of equal counts, each as in step 3, then Chan's formula  (LDS, one thread per channel)
//   3. per group: the cg channel partials (equal counts) as mean-of-means + sum of M2 + count * deviations^2, a team of
//      2^k <= 64 lanes per group, partner exchange by __shfl_xor                                          (fixed butterfly)
//   4. two-launch form only: the S slice partials of a group (staged in LDS by the apply pass's prologue), again equal counts but
//      for the last slice: the same team reduction, then Chan's formula with the last slice
// Every tree is a function of (h, w, c, groups, vector width) alone -- not of n, not of the grid: image i of a batch has the
// bits of the same image run alone, two launches agree, nothing is atomic.  None of the steps forms E[x^2] - E[x]^2.
//
// Forms (gn_plan): ONE LAUNCH when a unit of whole groups is at most 8192 elements (h * w * lcm(cg, 8) <= 8192): the tile is the
// whole image x a bundle of groups, the input vectors stay in LDS between steps 1-3 and the store -- one read, one write.
// Otherwise TWO LAUNCHES: groupnorm_stats_kernel over (slice, chunk, image) writes (mean, M2) per (image, slice, group) to the
// workspace, groupnorm_apply_kernel over the same grid runs step 4 for its chunk's groups and normalises its tile.  The slice
// count comes from h * w alone (at most 32: an apply workgroup reads slices x groups-of-its-chunk partials from L2).
//
// Register / occupancy table per instantiation: DESIGN.md section 9c.
#include <hip/hip_runtime.h>

#include <cstdint>

// (x - mean) * scale + beta and the activations round as written in every instantiation
#pragma clang fp contract(off)

#include "si_hip_internal.h"
#include "si_norm.h"

namespace {

constexpr int GN_THREADS = 256;
constexpr int GN_MAX_PL = 64;          // pixel lanes per channel vector: bounds the serial sums of step 2
constexpr int GN_SLAB_ELEMS = 8192;    // one-launch form: elements of a tile kept in LDS
constexpr int GN_MAX_GROUP_C = 4096;   // widest unit of whole groups (per-channel partials live in LDS)
constexpr int GN_MAX_SLICES = 32;

template <typename T>
struct GnArgs {
    const T* in;
    T* out;
    const float* gamma;
    const float* beta;
    float2* ws;   // [n][S][G] (mean, M2); two-launch form only
    int P, c, cg, G, in_ld, out_ld;
    float eps;
    int act;
    float act_param;
    int S, SP;    // slices per image and pixels per slice (one-launch form: 1, P)
    int gc;       // groups per chunk
    int cc4;      // channels of a full chunk, rounded up to 4: the LDS layout's stride
};

struct GnTile {
    int p0, npix;         // pixel range of the image
    int g0, gn, c0, ccn;  // groups / channels of the chunk
    int cvc, vpb, pl_n;   // vectors per pixel, vectors per pass, pixel lanes
    int tv, pl;           // this thread's vector (within a pass) and pixel lane
};

template <typename T, int VW>
__device__ __forceinline__ GnTile gn_tile(const GnArgs<T>& a, int slice, int chunk) {
    GnTile t;
    t.p0 = slice * a.SP;
    t.npix = min(a.SP, a.P - t.p0);
    t.g0 = chunk * a.gc;
    t.gn = min(a.gc, a.G - t.g0);
    t.c0 = t.g0 * a.cg;
    t.ccn = t.gn * a.cg;
    t.cvc = t.ccn / VW;
    t.vpb = min(t.cvc, GN_THREADS);
    t.pl_n = min(GN_THREADS / t.vpb, GN_MAX_PL);
    t.tv = (int)threadIdx.x % t.vpb;
    t.pl = (int)threadIdx.x / t.vpb;
    return t;
}

// Chan's formula: (na, ma, qa) <- (na, ma, qa) + (nb, mb, qb); an empty b changes nothing
__device__ __forceinline__ void gn_merge(float& na, float& ma, float& qa, float nb, float mb, float qb) {
    if (nb > 0.0f) {
        const float nab = na + nb;
        const float r = nb / nab;
        const float d = mb - ma;
        ma = ma + d * r;
        qa = qa + qb + (d * d) * (na * r);
        na = nab;
    }
}

// k >= 1 partials of the SAME count m, get(i) = (mean_i, M2_i), combined by lane j of a team of tpg lanes: the mean of the
// means (summed as differences to the first one: no cancellation against a large common offset) and
// M2 = sum M2_i + m * sum (mean_i - mean)^2.  One partial comes back bit for bit.
template <typename Get>
__device__ __forceinline__ float2 gn_combine_equal(Get get, int k, float m, int j, int tpg) {
    const float pivot = get(0).x;
    float s = 0.0f;
    for (int i = j; i < k; i += tpg) s += get(i).x - pivot;
    s = si_team<SiSum>(s, tpg);
    const float mu = pivot + s / (float)k;
    float q = 0.0f;
    for (int i = j; i < k; i += tpg) {
        const float2 e = get(i);
        const float d = e.x - mu;
        q += e.y + m * (d * d);
    }
    q = si_team<SiSum>(q, tpg);
    return make_float2(mu, q);
}

// lanes per team for gn groups: as many as 256 threads give every group at once, a power of two in [1, 64]
__device__ __forceinline__ int gn_team_size(int gn) {
    int tpg = 64;
    while (tpg > 1 && tpg * gn > GN_THREADS) tpg >>= 1;
    return tpg;
}

// LDS layout (floats): part_mean[256 * VW] | part_m2[256 * VW] | chan_mean[cc4] | chan_m2[cc4] | grp[2 * gc] | slab cache
template <int VW>
__device__ __forceinline__ float* gn_lds_chan(float* lds) { return lds + 2 * GN_THREADS * VW; }
template <int VW>
__device__ __forceinline__ float* gn_lds_grp(float* lds, int cc4) { return lds + 2 * GN_THREADS * VW + 2 * cc4; }

// steps 1-3 for one tile: grp[2 * gl] = mean, grp[2 * gl + 1] = M2 of the tile's pixels x group g0 + gl.  CACHE: every vector read
// is also kept at cache[pixel * cvc + vector] in its storage type.
template <typename T, int VW, bool CACHE>
__device__ __forceinline__ void gn_tile_stats(const GnArgs<T>& a, const GnTile& t, const T* img, float* lds, T* cache) {
    float* const part_mean = lds;
    float* const part_m2 = lds + GN_THREADS * VW;
    float* const chan_mean = gn_lds_chan<VW>(lds);
    float* const chan_m2 = chan_mean + a.cc4;
    float* const grp = gn_lds_grp<VW>(lds, a.cc4);
    const int tid = threadIdx.x;

    for (int vb = 0; vb < t.cvc; vb += t.vpb) {
        const int v = vb + t.tv;
        const bool lane_live = t.pl < t.pl_n;
        float mean[VW], m2[VW];
#pragma unroll
        for (int i = 0; i < VW; ++i) mean[i] = m2[i] = 0.0f;
        if (lane_live && v < t.cvc) {
            const T* src = img + (size_t)(t.p0 + t.pl) * a.in_ld + t.c0 + v * VW;
            const size_t step = (size_t)t.pl_n * a.in_ld;
            float k = 0.0f;
#pragma unroll 4
            for (int p = t.pl; p < t.npix; p += t.pl_n, src += step) {
                float x[VW];
                si_load_vec<T, VW>(src, x);
                if constexpr (CACHE) {
                    if constexpr (VW == 1) cache[p * t.cvc + v] = *src;
                    else si_store_vec<T, VW>(cache + (size_t)(p * t.cvc + v) * VW, x);   // (exact: x came from T)
                }
                k += 1.0f;
                const float inv = k == 1.0f ? 1.0f : __builtin_amdgcn_rcpf(k);   // (1 ulp: the mean moves by delta * 2^-24 at most)
#pragma unroll
                for (int i = 0; i < VW; ++i) {
                    const float d = x[i] - mean[i];
                    mean[i] = mean[i] + d * inv;
                    m2[i] = m2[i] + d * (x[i] - mean[i]);
                }
            }
        }
        if (lane_live) {
#pragma unroll
            for (int i = 0; i < VW; ++i) {
                part_mean[(t.pl * t.vpb + t.tv) * VW + i] = mean[i];
                part_m2[(t.pl * t.vpb + t.tv) * VW + i] = m2[i];
            }
        }
        __syncthreads();
        // step 2: one thread per channel of this pass.  Lanes [0, hi_n) saw full + 1 pixels, lanes [hi_n, PL) saw full: two runs of
        // equal counts (sums only, no division per lane), then Chan's formula between the two
        const int pass_c = min(t.vpb, t.cvc - vb) * VW;
        const int full = t.npix / t.pl_n, hi_n = t.npix % t.pl_n, stride = t.vpb * VW;
        for (int cl = tid; cl < pass_c; cl += GN_THREADS) {
            const float* const pm = part_mean + cl;
            const float* const pq = part_m2 + cl;
            float na = 0.0f, ma = 0.0f, qa = 0.0f;
            if (hi_n > 0) {
                const float2 r = gn_combine_equal([&](int i) { return make_float2(pm[i * stride], pq[i * stride]); }, hi_n, (float)(full + 1), 0, 1);
                na = (float)(hi_n * (full + 1));
                ma = r.x;
                qa = r.y;
            }
            if (full > 0) {
                const float2 r = gn_combine_equal([&](int i) { return make_float2(pm[(hi_n + i) * stride], pq[(hi_n + i) * stride]); },
                                                  t.pl_n - hi_n, (float)full, 0, 1);
                gn_merge(na, ma, qa, (float)((t.pl_n - hi_n) * full), r.x, r.y);
            }
            chan_mean[vb * VW + cl] = ma;
            chan_m2[vb * VW + cl] = qa;
        }
        __syncthreads();
    }
    // step 3: every channel of the tile has npix elements
    const int tpg = gn_team_size(t.gn);
    const int teams = GN_THREADS / tpg;
    const int team = tid / tpg, j = tid % tpg;
    for (int k0 = 0; k0 < t.gn; k0 += teams) {
        const int gl = k0 + team;
        const int gr = gl < t.gn ? gl : 0;   // (a team without a group computes group 0 again and drops it: the exchange needs every lane)
        const float* cm = chan_mean + gr * a.cg;
        const float* cq = chan_m2 + gr * a.cg;
        const float2 r = gn_combine_equal([&](int i) { return make_float2(cm[i], cq[i]); }, a.cg, (float)t.npix, j, tpg);
        if (gl < t.gn && j == 0) {
            grp[2 * gl] = r.x;
            grp[2 * gl + 1] = r.y;
        }
    }
    __syncthreads();
}

// the normalise / activation / store loop of one tile; grp[2 * gl] = mean, grp[2 * gl + 1] = rstd
template <typename T, int VW, bool CACHE>
__device__ __forceinline__ void gn_tile_apply(const GnArgs<T>& a, const GnTile& t, const T* img_in, T* img_out, const float* grp, const T* cache) {
    for (int vb = 0; vb < t.cvc; vb += t.vpb) {
        const int v = vb + t.tv;
        if (t.pl >= t.pl_n || v >= t.cvc) continue;
        float mu[VW], sc[VW], be[VW];
#pragma unroll
        for (int i = 0; i < VW; ++i) {
            const int cl = v * VW + i;
            const int gl = cl / a.cg;
            mu[i] = grp[2 * gl];
            sc[i] = a.gamma ? grp[2 * gl + 1] * a.gamma[t.c0 + cl] : grp[2 * gl + 1];
            be[i] = a.beta ? a.beta[t.c0 + cl] : 0.0f;
        }
        const T* src = img_in + (size_t)(t.p0 + t.pl) * a.in_ld + t.c0 + v * VW;
        T* dst = img_out + (size_t)(t.p0 + t.pl) * a.out_ld + t.c0 + v * VW;
        const size_t in_step = (size_t)t.pl_n * a.in_ld, out_step = (size_t)t.pl_n * a.out_ld;
        for (int p = t.pl; p < t.npix; p += t.pl_n, src += in_step, dst += out_step) {
            float x[VW], y[VW];
            if constexpr (CACHE) si_load_vec<T, VW>(cache + (size_t)(p * t.cvc + v) * VW, x);
            else si_load_vec<T, VW>(src, x);
#pragma unroll
            for (int i = 0; i < VW; ++i) y[i] = si_act(a.act, (x[i] - mu[i]) * sc[i] + be[i], a.act_param);
            si_store_vec<T, VW>(dst, y);
        }
    }
}

// grid: (slices, chunks, images)
template <typename T, int VW>
__global__ __launch_bounds__(GN_THREADS) void groupnorm_stats_kernel(const GnArgs<T> a) {
    extern __shared__ __attribute__((aligned(16))) float gn_lds[];
    const GnTile t = gn_tile<T, VW>(a, blockIdx.x, blockIdx.y);
    const int img = blockIdx.z;
    gn_tile_stats<T, VW, false>(a, t, a.in + (size_t)img * a.P * a.in_ld, gn_lds, nullptr);
    const float* grp = gn_lds_grp<VW>(gn_lds, a.cc4);
    float2* const ws = a.ws + ((size_t)img * a.S + blockIdx.x) * a.G + t.g0;
    for (int gl = threadIdx.x; gl < t.gn; gl += GN_THREADS) ws[gl] = make_float2(grp[2 * gl], grp[2 * gl + 1]);
}

// grid: (slices, chunks, images), the tiles of the statistics pass.  Prologue (step 4): slices 0 .. S-2 hold SP * cg elements each,
// the last one the rest.
template <typename T, int VW>
__global__ __launch_bounds__(GN_THREADS) void groupnorm_apply_kernel(const GnArgs<T> a) {
    extern __shared__ __attribute__((aligned(16))) float gn_lds[];
    const GnTile t = gn_tile<T, VW>(a, blockIdx.x, blockIdx.y);
    const int img = blockIdx.z, tid = threadIdx.x;
    float* const grp = gn_lds;
    // the chunk's partials, every slice, fetched from L2 once: stage[s * gn + gl]
    float2* const stage = reinterpret_cast<float2*>(gn_lds + ((size_t)2 * a.gc + 3) / 4 * 4);
    const float2* const ws = a.ws + (size_t)img * a.S * a.G + t.g0;
    for (int idx = tid; idx < a.S * t.gn; idx += GN_THREADS) {
        const int sl = idx / t.gn;
        stage[idx] = ws[(size_t)sl * a.G + (idx - sl * t.gn)];
    }
    __syncthreads();
    const int tpg = gn_team_size(t.gn);
    const int teams = GN_THREADS / tpg;
    const int team = tid / tpg, j = tid % tpg;
    const float m_full = (float)a.SP * (float)a.cg;
    const float m_last = (float)(a.P - (a.S - 1) * a.SP) * (float)a.cg;
    for (int k0 = 0; k0 < t.gn; k0 += teams) {
        const int gl = k0 + team;
        const int gr = gl < t.gn ? gl : 0;
        const float2 last = stage[(a.S - 1) * t.gn + gr];
        float na = 0.0f, ma = 0.0f, qa = 0.0f;
        if (a.S > 1) {
            const float2 r = gn_combine_equal([&](int i) { return stage[i * t.gn + gr]; }, a.S - 1, m_full, j, tpg);
            na = m_full * (float)(a.S - 1);
            ma = r.x;
            qa = r.y;
            gn_merge(na, ma, qa, m_last, last.x, last.y);
        } else {
            na = m_last;
            ma = last.x;
            qa = last.y;
        }
        if (gl < t.gn && j == 0) {
            grp[2 * gl] = ma;
            grp[2 * gl + 1] = 1.0f / sqrtf(qa / na + a.eps);
        }
    }
    __syncthreads();
    gn_tile_apply<T, VW, false>(a, t, a.in + (size_t)img * a.P * a.in_ld, a.out + (size_t)img * a.P * a.out_ld, grp, nullptr);
}

// one launch; grid: (1, bundles of groups, images)
template <typename T, int VW>
__global__ __launch_bounds__(GN_THREADS) void groupnorm_slab_kernel(const GnArgs<T> a, int cache_off) {
    extern __shared__ __attribute__((aligned(16))) float gn_lds[];
    const GnTile t = gn_tile<T, VW>(a, 0, blockIdx.y);
    const int img = blockIdx.z;
    T* const cache = reinterpret_cast<T*>(gn_lds + cache_off);
    const T* const img_in = a.in + (size_t)img * a.P * a.in_ld;
    gn_tile_stats<T, VW, true>(a, t, img_in, gn_lds, cache);
    float* const grp = gn_lds_grp<VW>(gn_lds, a.cc4);
    const float count = (float)a.P * (float)a.cg;
    for (int gl = threadIdx.x; gl < t.gn; gl += GN_THREADS) grp[2 * gl + 1] = 1.0f / sqrtf(grp[2 * gl + 1] / count + a.eps);
    __syncthreads();
    gn_tile_apply<T, VW, true>(a, t, img_in, a.out + (size_t)img * a.P * a.out_ld, grp, cache);
}

// ---- host -----------------------------------------------------------------------------------------------------------------
int gcd_int(int a, int b) {
    while (b) {
        const int r = a % b;
        a = b;
        b = r;
    }
    return a;
}

// everything that can be decided without a device: SI_E_BADARG / SI_E_UNSUPPORTED / 0
int check_desc(const SiGroupNormDesc* d) {
    if (!d) return SI_E_BADARG;
    if (d->n <= 0 || d->h <= 0 || d->w <= 0 || d->c <= 0) return SI_E_BADARG;
    if (d->groups <= 0 || d->c % d->groups != 0) return SI_E_BADARG;
    if (d->in_ld < d->c || d->out_ld < d->c) return SI_E_BADARG;
    if (d->act < SI_ACT_NONE || d->act > SI_ACT_LEAKYRELU) return SI_E_BADARG;
    if (!(d->eps >= 0.0f)) return SI_E_BADARG;
    const uint64_t pixels = (uint64_t)d->n * d->h * d->w;
    if (pixels > SI_INDEX_LIMIT) return SI_E_UNSUPPORTED;
    if (pixels * (uint64_t)d->in_ld > SI_INDEX_LIMIT || pixels * (uint64_t)d->out_ld > SI_INDEX_LIMIT) return SI_E_UNSUPPORTED;
    if (d->n > 65535) return SI_E_UNSUPPORTED;
    if (d->c / d->groups > GN_MAX_GROUP_C) return SI_E_UNSUPPORTED;
    return 0;
}

struct GnPlan {
    int vw;       // channel vector in elements: 16 bytes' worth, or 1
    bool slab;    // one launch
    int S, SP;    // slices and pixels per slice
    int gc;       // groups per chunk
    int chunks;
    int cc4;
};

// the form is a function of the SHAPE (the workspace query has no pointers): one launch when h * w * lcm(cg, 8) <= 8192 -- a unit of
// whole groups that is a whole number of vectors, for every vector width
bool slab_form(const SiGroupNormDesc* d) {
    if (SI_ENV_INT("SI_GROUPNORM_FORM", 0) == 2) return false;   // (experiment build only: the two-launch form on every shape, for A/B runs)
    const int cg = d->c / d->groups;
    const uint64_t unit8 = (uint64_t)cg / gcd_int(cg, 8) * 8;
    return (uint64_t)d->h * d->w * unit8 <= (uint64_t)GN_SLAB_ELEMS;
}

// slices of the two-launch form, from the pixel count alone: ~256 pixels each, at most 32 slices
void slices_of(int P, int& S, int& SP) {
    S = (P + 255) / 256;
    if (S > GN_MAX_SLICES) S = GN_MAX_SLICES;
    SP = (P + S - 1) / S;
    S = (P + SP - 1) / SP;
}

template <typename T>
int make_plan(const SiGroupNormDesc* d, const void* in, const void* out, GnPlan& pl) {
    const int full = (int)(16 / sizeof(T));
    const int cg = d->c / d->groups;
    const int P = d->h * d->w;
    pl.vw = 1;
    if (d->c % full == 0 && d->in_ld % full == 0 && d->out_ld % full == 0 && si_aligned_to(in, 16) && si_aligned_to(out, 16) &&
        (uint64_t)cg / gcd_int(cg, full) * full <= (uint64_t)GN_MAX_GROUP_C)
        pl.vw = full;
    const int unit = pl.vw / gcd_int(cg, pl.vw);   // groups per whole number of vectors
    const int unit_c = unit * cg;
    pl.slab = slab_form(d);
    int target_c;   // channels per chunk aimed at
    if (pl.slab) {
        pl.S = 1;
        pl.SP = P;
        target_c = GN_SLAB_ELEMS / P;
        if (target_c > 32 * pl.vw) target_c = 32 * pl.vw;
    } else {
        slices_of(P, pl.S, pl.SP);
        // eight vectors (128 contiguous bytes) per pixel; at most 32 channels -- four half vectors: twice the tiles and pixel lanes,
        // half the walk -- where the slice count is capped and a slice is longer than 256 pixels (both widths and ~128-pixel slices
        // measured at batch 8: profiles/groupnorm_01a5c12.txt, section 3)
        target_c = 8 * pl.vw;
        if (pl.SP > 256 && target_c > 32) target_c = 32;
    }
    int units = target_c / unit_c;
    if (units < 1) units = 1;
    pl.gc = units * unit;
    if (pl.gc > d->groups) pl.gc = d->groups;
    pl.chunks = (d->groups + pl.gc - 1) / pl.gc;
    if (pl.chunks > 65535) return SI_E_UNSUPPORTED;
    pl.cc4 = (pl.gc * cg + 3) / 4 * 4;
    return 0;
}

size_t lds_floats(const GnPlan& pl) { return (size_t)2 * GN_THREADS * pl.vw + 2 * (size_t)pl.cc4 + ((size_t)2 * pl.gc + 3) / 4 * 4; }

template <typename T, int VW>
int launch(const SiGroupNormDesc* d, const GnPlan& pl, const T* in, const float* gamma, const float* beta, T* out, void* workspace, hipStream_t stream) {
    GnArgs<T> a;
    a.in = in;
    a.out = out;
    a.gamma = d->affine ? gamma : nullptr;
    a.beta = d->affine ? beta : nullptr;
    a.ws = static_cast<float2*>(workspace);
    a.P = d->h * d->w;
    a.c = d->c;
    a.cg = d->c / d->groups;
    a.G = d->groups;
    a.in_ld = d->in_ld;
    a.out_ld = d->out_ld;
    a.eps = d->eps;
    a.act = d->act;
    a.act_param = d->act_param;
    a.S = pl.S;
    a.SP = pl.SP;
    a.gc = pl.gc;
    a.cc4 = pl.cc4;
    const dim3 grid((unsigned)pl.S, (unsigned)pl.chunks, (unsigned)d->n);
    const size_t stat_lds = lds_floats(pl) * sizeof(float);
    if (pl.slab) {
        const size_t lds = stat_lds + (size_t)a.P * pl.gc * a.cg * sizeof(T);
        SI_HIP_TRY(si_allow_dynamic_lds(groupnorm_slab_kernel<T, VW>, lds));
        hipLaunchKernelGGL((groupnorm_slab_kernel<T, VW>), grid, dim3(GN_THREADS), lds, stream, a, (int)lds_floats(pl));
        return (int)hipGetLastError();
    }
    SI_HIP_TRY(si_allow_dynamic_lds(groupnorm_stats_kernel<T, VW>, stat_lds));
    hipLaunchKernelGGL((groupnorm_stats_kernel<T, VW>), grid, dim3(GN_THREADS), stat_lds, stream, a);
    SI_HIP_TRY(hipGetLastError());
    const size_t apply_lds = (((size_t)2 * pl.gc + 3) / 4 * 4 + (size_t)2 * pl.S * pl.gc) * sizeof(float);   // grp | the staged partials
    SI_HIP_TRY(si_allow_dynamic_lds(groupnorm_apply_kernel<T, VW>, apply_lds));
    hipLaunchKernelGGL((groupnorm_apply_kernel<T, VW>), grid, dim3(GN_THREADS), apply_lds, stream, a);
    return (int)hipGetLastError();
}

template <typename T>
int run(const SiGroupNormDesc* d, const T* in, const float* gamma, const float* beta, T* out, void* workspace, si_stream_t stream) {
    const int rc = check_desc(d);
    if (rc != 0) return rc;
    if (!in || !out) return SI_E_BADARG;
    if (d->affine && (!gamma || !beta)) return SI_E_BADARG;
    GnPlan pl;
    const int prc = make_plan<T>(d, in, out, pl);
    if (prc != 0) return prc;
    if (!pl.slab && !workspace) return SI_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    constexpr int full = (int)(16 / sizeof(T));
    return pl.vw == full ? launch<T, full>(d, pl, in, gamma, beta, out, workspace, s) : launch<T, 1>(d, pl, in, gamma, beta, out, workspace, s);
}

}  // namespace

extern "C" {

size_t si_hip_groupnorm_workspace_bytes(const SiGroupNormDesc* d) {
    if (check_desc(d) != 0 || slab_form(d)) return 0;
    int S, SP;
    slices_of(d->h * d->w, S, SP);
    return (size_t)d->n * S * d->groups * sizeof(float2);
}

int si_hip_groupnorm_f32(const SiGroupNormDesc* d, const float* in, const float* gamma, const float* beta, float* out, void* workspace,
                         si_stream_t stream) {
    return run<float>(d, in, gamma, beta, out, workspace, stream);
}

int si_hip_groupnorm_f16(const SiGroupNormDesc* d, const void* in, const float* gamma, const float* beta, void* out, void* workspace,
                         si_stream_t stream) {
    return run<_Float16>(d, static_cast<const _Float16*>(in), gamma, beta, static_cast<_Float16*>(out), workspace, stream);
}

const char* si_hip_groupnorm_kernel_name(const SiGroupNormDesc* d, const void* in, const void* out, int half) {
    if (check_desc(d) != 0) return "none";
    GnPlan pl;
    if ((half ? make_plan<_Float16>(d, in, out, pl) : make_plan<float>(d, in, out, pl)) != 0) return "none";
    const bool vec = pl.vw > 1;
    if (pl.slab) {
        if (half) return vec ? "groupnorm_slab_kernel<_Float16, 8>" : "groupnorm_slab_kernel<_Float16, 1>";
        return vec ? "groupnorm_slab_kernel<float, 4>" : "groupnorm_slab_kernel<float, 1>";
    }
    if (half)
        return vec ? "groupnorm_stats_kernel<_Float16, 8> + groupnorm_apply_kernel<_Float16, 8>"
                   : "groupnorm_stats_kernel<_Float16, 1> + groupnorm_apply_kernel<_Float16, 1>";
    return vec ? "groupnorm_stats_kernel<float, 4> + groupnorm_apply_kernel<float, 4>"
               : "groupnorm_stats_kernel<float, 1> + groupnorm_apply_kernel<float, 1>";
}

}  // extern "C"
