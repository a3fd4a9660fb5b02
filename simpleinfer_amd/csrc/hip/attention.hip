// attention.hip -- fused scaled dot-product attention (include/si_attention.h): O = softmax(scale * Q K^T) V per (batch, head), one launch,
// no workspace, no atomics.  Views, contract, special values and the refusals: the header.
//
// A workgroup of four waves owns one (batch, head, block of 64 queries); wave w owns query rows 16w .. 16w + 15 of the block.  K and V are
// walked in tiles of 64 keys; the four waves stage a tile in LDS together and read it as MFMA operands.  With lane = 16 g + x (g = 0..3,
// x = 0..15) a wave computes, per tile,
//     S^T = K Q^T    four 16-key x 16-query products (sub-tiles t = 0..3).  K is the A operand from LDS, Q^T the B operand from registers
//                    (loaded once per workgroup).  The C/D map of the 16x16 MFMA puts the QUERY on x and key 16 t + 4 g + r in register r
//                    of sub-tile t: a lane holds 16 scores of ONE query.
//     softmax        the row maximum is a maximum over the lane's 16 registers and two butterflies (xor 16, xor 32) over the four lanes of
//                    a query; m' = max(m, tile maximum), alpha = exp2(c (m - m')), p = exp2(c (s - m')), l = l * alpha + sum p with l kept
//                    per lane (its four lanes are added once, by the same butterflies, before the store); O is scaled by alpha.  c is
//                    |scale| log2(e); s is the score times the sign of the scale.
//     O^T += V^T P^T the query stays on x, so P^T is already the B operand: the k-step (t, r) takes key 16 t + 4 g + r from lane group g,
//                    which is the value the lane holds in register r of sub-tile t (fp16: the k-step u = 0, 1 takes the eight values of
//                    sub-tiles 2u and 2u + 1, rounded to halves).  V^T is the A operand from LDS.  O^T has the query on x and head-dim
//                    column 16 c + 4 g + r in register r of chunk c: a lane stores runs of four neighbouring columns.
// Nothing of S or P touches LDS.  The key order inside a product is a permutation of 0 .. 63, the same in every launch.
//
// LDS images, both refilled per tile behind a barrier; rows of keys beyond lk and columns beyond d are written as zeros, never loaded:
//   fp32  K [64 keys][DP + 2], V [64 keys][DP + 4] floats.  ds_read_b32 serves a wave as two halves of 32 lanes over 32 banks.  The K read of
//         a half is 16 keys x 2 neighbouring columns: with a pitch of DP + 2 (= 2 mod 32 for DP >= 32; 18 for DP = 16, where 18 k mod 32
//         runs through the 16 even banks) key k starts at bank 2 k plus a constant, so the 32 lanes take 32 banks.  The V read of a half
//         is 2 keys four rows apart x 16 neighbouring columns: 4 (DP + 4) = 16 mod 32 puts the second key's columns on the other 16 banks.
//   fp16  K as [DP / 8 chunks][64 keys][8 halves]: a lane reads 16 bytes (ds_read_b128), chunk 4 s + g of key 16 t + x in k-step s.  The
//         chunk pitch is 1 KiB = four bank rows, so the 16-byte slot of a lane is x mod 16 whatever g is, and each of the instruction's
//         four 16-lane groups (which mix two values of g) covers the 16 slots of a bank row once: no padding needed.
//         V transposed as [DP / 16 chunks c][k-step u][g][16 columns][8 keys]: the eight keys of (u, g) in operand order, one 16-byte
//         read per lane, slots by x as above.  The transposition is paid at the staging store (eight 2-byte stores per 16 bytes loaded).
//
// Offsets are 32-bit: the host refuses views whose offsets do not fit 31 bits.  Register / LDS table per instantiation: DESIGN.md 9m.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <type_traits>

#include "si_attention.h"
#include "si_hip_internal.h"

#pragma clang fp contract(off)

namespace {

constexpr int AT_THREADS = 256;
constexpr int AT_BQ = SI_ATTENTION_BLOCK_Q;
constexpr int AT_TK = SI_ATTENTION_TILE_K;
static_assert(AT_BQ == 16 * (AT_THREADS / 64) && AT_TK == 64, "a wave owns 16 queries; a key tile is four 16-key sub-tiles");

struct AtArgs {
    const void *q, *k, *v;
    void* o;
    int heads, lq, lk, d, qblocks;
    int q_sb, q_ss, k_sb, k_ss, v_sb, v_ss, o_sb, o_ss;
    float sgn, ca;   // scale * log2(e) as its sign (+-1) and its magnitude
};

template <typename T, int DP>
constexpr size_t at_lds_bytes() {
    return sizeof(T) == 4 ? (size_t)AT_TK * ((DP + 2) + (DP + 4)) * 4 : (size_t)2 * AT_TK * DP * 2;
}

template <typename T, int DP>
__global__ __launch_bounds__(AT_THREADS) void attention_kernel(AtArgs a) {
    constexpr bool HALF = sizeof(T) == 2;
    constexpr int KP = DP + 2, VP = DP + 4;   // fp32 image pitches
    constexpr int NC = DP / 16;               // chunks of 16 output columns
    constexpr int QR = HALF ? DP / 32 : DP / 4;   // k-steps of the first product = Q operand registers (f16x8 / float)
    extern __shared__ __attribute__((aligned(16))) unsigned char at_smem[];

    const int tid = (int)threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int x = lane & 15, g = lane >> 4;
    int bid = (int)blockIdx.x;
    const int qb = bid % a.qblocks;
    bid /= a.qblocks;
    const int h = bid % a.heads;
    const int b = bid / a.heads;
    const int hd = h * a.d;

    const T* const qp = static_cast<const T*>(a.q) + b * a.q_sb + hd;
    const T* const kp = static_cast<const T*>(a.k) + b * a.k_sb + hd;
    const T* const vp = static_cast<const T*>(a.v) + b * a.v_sb + hd;
    T* const op = static_cast<T*>(a.o) + b * a.o_sb + hd;

    const int q0 = qb * AT_BQ + wave * 16;
    const bool wave_live = q0 < a.lq;   // (a wave without query rows stages tiles and meets the barriers, nothing else)
    const int query = q0 + x;
    const bool q_live = query < a.lq;

    // Q^T as the B operand: fp32 B[k = g][col x] = Q[query][4 s + g]; fp16 B[k = 8 g + j][col x] = Q[query][32 s + 8 g + j]
    typedef typename std::conditional<HALF, f16x8, float>::type QFrag;
    QFrag qf[QR];
#pragma unroll
    for (int s = 0; s < QR; ++s) {
        if constexpr (HALF) {
            const int col = 32 * s + 8 * g;
            f16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
            qf[s] = (q_live && col < a.d) ? *reinterpret_cast<const f16x8*>(qp + query * a.q_ss + col) : z;
        } else {
            const int col = 4 * s + g;
            qf[s] = (q_live && col < a.d) ? qp[query * a.q_ss + col] : 0.0f;
        }
    }

    f32x4 oacc[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) oacc[c] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    float m = -INFINITY, l = 0.0f;

    for (int k0 = 0; k0 < a.lk; k0 += AT_TK) {
        const int rem = a.lk - k0;   // keys of this tile and beyond, >= 1
        __syncthreads();             // the previous tile's reads are done
        if constexpr (HALF) {
            f16x8* const kimg = reinterpret_cast<f16x8*>(at_smem);
            _Float16* const vimg = reinterpret_cast<_Float16*>(at_smem) + AT_TK * DP;
            constexpr int CH = DP / 8;
            for (int idx = tid; idx < AT_TK * CH; idx += AT_THREADS) {
                const int ch = idx % CH, row = idx / CH;
                const bool live = row < rem && ch * 8 < a.d;
                f16x8 kv = {0, 0, 0, 0, 0, 0, 0, 0}, vv = {0, 0, 0, 0, 0, 0, 0, 0};
                if (live) {
                    kv = *reinterpret_cast<const f16x8*>(kp + (k0 + row) * a.k_ss + ch * 8);
                    vv = *reinterpret_cast<const f16x8*>(vp + (k0 + row) * a.v_ss + ch * 8);
                }
                kimg[ch * AT_TK + row] = kv;
                // key row = 16 t + 4 gg + r is element j = 4 (t & 1) + r of k-step u = t >> 1, lane group gg
                const int t = row >> 4, gg = (row >> 2) & 3, r = row & 3;
                const int u = t >> 1, j = 4 * (t & 1) + r;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int col = ch * 8 + e;
                    vimg[((((col >> 4) * 2 + u) * 4 + gg) * 16 + (col & 15)) * 8 + j] = vv[e];
                }
            }
        } else {
            float* const kimg = reinterpret_cast<float*>(at_smem);
            float* const vimg = kimg + AT_TK * KP;
            for (int idx = tid; idx < AT_TK * DP; idx += AT_THREADS) {
                const int col = idx % DP, row = idx / DP;
                const bool live = row < rem && col < a.d;
                float kv = 0.0f, vv = 0.0f;
                if (live) {
                    kv = kp[(k0 + row) * a.k_ss + col];
                    vv = vp[(k0 + row) * a.v_ss + col];
                }
                kimg[row * KP + col] = kv;
                vimg[row * VP + col] = vv;
            }
        }
        __syncthreads();
        if (!wave_live) continue;

        // ---- S^T = K Q^T: sub-tile t, register r = key 16 t + 4 g + r, query x
        f32x4 sc[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            sc[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            if (16 * t < rem) {   // (a sub-tile without keys is skipped: wave-uniform)
                if constexpr (HALF) {
                    const f16x8* const kimg = reinterpret_cast<const f16x8*>(at_smem);
#pragma unroll
                    for (int s = 0; s < QR; ++s)
                        sc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kimg[(4 * s + g) * AT_TK + 16 * t + x], qf[s], sc[t], 0, 0, 0);
                } else {
                    const float* const kimg = reinterpret_cast<const float*>(at_smem);
#pragma unroll
                    for (int s = 0; s < QR; ++s)
                        sc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(kimg[(16 * t + x) * KP + 4 * s + g], qf[s], sc[t], 0, 0, 0);
                }
            }
        }

        // ---- online softmax of the lane's 16 scores.  The maximum is taken of the raw scores (times the sign of the scale) and subtracted
        // BEFORE the one multiply by |scale| log2(e): the difference of two nearby scores is exact, so a weight keeps its relative precision
        // however large the scores are, and the largest score gives exactly exp2(0) = 1.  Keys beyond lk: p = 0 by a select.
        float tmax = -INFINITY;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float s = sc[t][r] * a.sgn;
                sc[t][r] = s;
                tmax = fmaxf(tmax, (16 * t + 4 * g + r < rem) ? s : -INFINITY);   // (fmaxf skips a NaN: it reaches the row through exp2 below)
            }
        tmax = fmaxf(tmax, __shfl_xor(tmax, 16, 64));
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
        const float mn = fmaxf(m, tmax);
        const float ref = mn == -INFINITY ? 0.0f : mn;   // (a row of only NaN scores keeps m = -inf: no inf - inf)
        const float alpha = m == -INFINITY ? 0.0f : __builtin_amdgcn_exp2f((m - ref) * a.ca);
        m = mn;
        float psum = 0.0f;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float p = (16 * t + 4 * g + r < rem) ? __builtin_amdgcn_exp2f((sc[t][r] - ref) * a.ca) : 0.0f;
                if constexpr (HALF) p = (float)(_Float16)p;   // the value the second product uses
                sc[t][r] = p;
                psum += p;
            }
        l = l * alpha + psum;
#pragma unroll
        for (int c = 0; c < NC; ++c) oacc[c] *= alpha;

        // ---- O^T += V^T P^T
        if constexpr (HALF) {
            const f16x8* const vimg = reinterpret_cast<const f16x8*>(at_smem) + AT_TK * DP / 8;
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                if (32 * u < rem) {
                    f16x8 pk;
#pragma unroll
                    for (int j = 0; j < 8; ++j) pk[j] = (_Float16)sc[2 * u + (j >> 2)][j & 3];
#pragma unroll
                    for (int c = 0; c < NC; ++c)
                        oacc[c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vimg[((c * 2 + u) * 4 + g) * 16 + x], pk, oacc[c], 0, 0, 0);
                }
            }
        } else {
            const float* const vimg = reinterpret_cast<const float*>(at_smem) + AT_TK * KP;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                if (16 * t < rem) {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
#pragma unroll
                        for (int c = 0; c < NC; ++c)
                            oacc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(vimg[(16 * t + 4 * g + r) * VP + 16 * c + x], sc[t][r], oacc[c], 0, 0, 0);
                }
            }
        }
    }

    if (!wave_live) return;
    // the row sum: the four lanes of a query, same bits in all four (+ is commutative: both partners of an exchange form the same value)
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    if (!q_live) return;
    T* const orow = op + query * a.o_ss;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const int col = 16 * c + 4 * g;
        if constexpr (HALF) {
            if (col < a.d) {   // d % 8 == 0: the four columns are inside together
                f16x4 hv;
#pragma unroll
                for (int r = 0; r < 4; ++r) hv[r] = si_store_cast<_Float16>(oacc[c][r] / l);
                *reinterpret_cast<f16x4*>(orow + col) = hv;
            }
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (col + r < a.d) orow[col + r] = oacc[c][r] / l;
        }
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------
// one past the last element offset of a view, or 0 when it does not fit 31 bits
uint64_t view_extent(const SiAttentionDesc* d, long long sb, long long ss, int len) {
    const uint64_t last = (uint64_t)(d->batch - 1) * (uint64_t)sb + (uint64_t)(len - 1) * (uint64_t)ss + (uint64_t)d->heads * (uint64_t)d->d - 1;
    // (each product is below 2^31 * 2^63: check the factors before trusting the sum)
    if ((uint64_t)sb > SI_INDEX_LIMIT || (uint64_t)ss > SI_INDEX_LIMIT) return 0;
    return last > SI_INDEX_LIMIT ? 0 : last + 1;
}

// everything that can be decided without a device and without the pointers: SI_E_BADARG / SI_E_UNSUPPORTED / 0
int check_desc(const SiAttentionDesc* d) {
    if (!d) return SI_E_BADARG;
    if (d->batch <= 0 || d->heads <= 0 || d->lq <= 0 || d->lk <= 0 || d->d <= 0) return SI_E_BADARG;
    const long long sb[4] = {d->q_sb, d->k_sb, d->v_sb, d->o_sb}, ss[4] = {d->q_ss, d->k_ss, d->v_ss, d->o_ss};
    const long long row = (long long)d->heads * (long long)d->d;
    for (int i = 0; i < 4; ++i) {
        if (sb[i] < 0 || ss[i] < 0) return SI_E_BADARG;
        if (ss[i] < row) return SI_E_BADARG;
    }
    if (d->batch > 1 && d->o_sb < row) return SI_E_BADARG;
    // the output rows of different (batch item, token) pairs must not share an element: one index has to step over the whole other one
    if (d->batch > 1 && d->lq > 1 && d->o_sb < (long long)(d->lq - 1) * d->o_ss + row && d->o_ss < (long long)(d->batch - 1) * d->o_sb + row)
        return SI_E_BADARG;
    if (d->d > SI_ATTENTION_MAX_D) return SI_E_UNSUPPORTED;
    for (int i = 0; i < 4; ++i)
        if (view_extent(d, sb[i], ss[i], (i == 0 || i == 3) ? d->lq : d->lk) == 0) return SI_E_UNSUPPORTED;
    const uint64_t blocks = (uint64_t)d->batch * (uint64_t)d->heads * (uint64_t)((d->lq + AT_BQ - 1) / AT_BQ);
    if (blocks > SI_INDEX_LIMIT) return SI_E_UNSUPPORTED;
    return 0;
}

// the pointers: null, overlap (SI_E_BADARG), and the fp16 alignment rule (SI_E_UNSUPPORTED)
int check_ptrs(const SiAttentionDesc* d, const void* q, const void* k, const void* v, const void* o, bool half) {
    if (!q || !k || !v || !o) return SI_E_BADARG;
    const size_t es = half ? 2 : 4;
    const uint64_t o_bytes = view_extent(d, d->o_sb, d->o_ss, d->lq) * es;
    const void* const in[3] = {q, k, v};
    const long long sb[3] = {d->q_sb, d->k_sb, d->v_sb}, ss[3] = {d->q_ss, d->k_ss, d->v_ss};
    for (int i = 0; i < 3; ++i)
        if (si_ranges_overlap(in[i], view_extent(d, sb[i], ss[i], i == 0 ? d->lq : d->lk) * es, o, o_bytes)) return SI_E_BADARG;
    if (half) {
        if (d->d % 8 != 0) return SI_E_UNSUPPORTED;
        const long long st[8] = {d->q_sb, d->q_ss, d->k_sb, d->k_ss, d->v_sb, d->v_ss, d->o_sb, d->o_ss};
        for (int i = 0; i < 8; ++i)
            if (st[i] % 8 != 0) return SI_E_UNSUPPORTED;
        if (!si_aligned_to(q, 16) || !si_aligned_to(k, 16) || !si_aligned_to(v, 16) || !si_aligned_to(o, 16)) return SI_E_UNSUPPORTED;
    }
    return 0;
}

// the padded head dim of the instantiation: a function of d and the type alone
int padded_d(int d, bool half) {
    const int lo = half ? 32 : 16;
    int dp = lo;
    while (dp < d) dp *= 2;
    return dp;
}

template <typename T, int DP>
int launch(const AtArgs& a, unsigned blocks, hipStream_t stream) {
    constexpr size_t lds = at_lds_bytes<T, DP>();
    SI_HIP_TRY(si_allow_dynamic_lds(attention_kernel<T, DP>, lds));
    hipLaunchKernelGGL((attention_kernel<T, DP>), dim3(blocks), dim3(AT_THREADS), lds, stream, a);
    return (int)hipGetLastError();
}

template <typename T>
int run(const SiAttentionDesc* d, const void* q, const void* k, const void* v, void* o, si_stream_t stream) {
    constexpr bool half = sizeof(T) == 2;
    int rc = check_desc(d);
    if (rc != 0) return rc;
    rc = check_ptrs(d, q, k, v, o, half);
    if (rc != 0) return rc;
    AtArgs a;
    a.q = q; a.k = k; a.v = v; a.o = o;
    a.heads = d->heads; a.lq = d->lq; a.lk = d->lk; a.d = d->d;
    a.qblocks = (d->lq + AT_BQ - 1) / AT_BQ;
    a.q_sb = (int)d->q_sb; a.q_ss = (int)d->q_ss;
    a.k_sb = (int)d->k_sb; a.k_ss = (int)d->k_ss;
    a.v_sb = (int)d->v_sb; a.v_ss = (int)d->v_ss;
    a.o_sb = (int)d->o_sb; a.o_ss = (int)d->o_ss;
    const float c = d->scale * 1.44269504088896340736f;
    a.sgn = c < 0.0f ? -1.0f : 1.0f;
    a.ca = fabsf(c);
    const unsigned blocks = (unsigned)(d->batch * d->heads * a.qblocks);
    hipStream_t s = (hipStream_t)stream;
    switch (padded_d(d->d, half)) {
        case 16:
            if constexpr (!half) return launch<T, 16>(a, blocks, s);
            break;
        case 32: return launch<T, 32>(a, blocks, s);
        case 64: return launch<T, 64>(a, blocks, s);
        case 128: return launch<T, 128>(a, blocks, s);
        default: break;
    }
    return SI_E_UNSUPPORTED;
}

}  // namespace

extern "C" {

int si_hip_attention_f32(const SiAttentionDesc* d, const float* q, const float* k, const float* v, float* o, si_stream_t stream) {
    return run<float>(d, q, k, v, o, stream);
}

int si_hip_attention_f16(const SiAttentionDesc* d, const void* q, const void* k, const void* v, void* o, si_stream_t stream) {
    return run<_Float16>(d, q, k, v, o, stream);
}

const char* si_hip_attention_kernel_name(const SiAttentionDesc* d, const void* q, const void* k, const void* v, const void* o, int half) {
    if (check_desc(d) != 0 || check_ptrs(d, q, k, v, o, half != 0) != 0) return "none";
    static const char* const names[2][4] = {
        {"attention_kernel<float, 16>", "attention_kernel<float, 32>", "attention_kernel<float, 64>", "attention_kernel<float, 128>"},
        {"none", "attention_kernel<_Float16, 32>", "attention_kernel<_Float16, 64>", "attention_kernel<_Float16, 128>"},
    };
    const int dp = padded_d(d->d, half != 0);
    return names[half ? 1 : 0][dp == 16 ? 0 : dp == 32 ? 1 : dp == 64 ? 2 : 3];
}

}  // extern "C"
