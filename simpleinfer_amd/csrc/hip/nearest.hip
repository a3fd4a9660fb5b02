// nearest.hip -- the fused nearest-row search (include/si_nearest.h): per row of x1 the nearest (and second nearest) row of x2, its
// distance and the row itself, without the p x r matrix of torch.cdist.
//
//   nearest_kernel<T, VEC, K>    a workgroup owns 64 rows of x1 and walks the 64-column tiles of its share of r.  Per tile the A . B^T
//                                product is cdist_mm_kernel's, instruction for instruction (the 64 x 64 x 32 core of si_mma_dev.h for fp32,
//                                si_mma16 on K-tiles of 64 halves for fp16, the squared norms on the staging path); the epilogue folds the
//                                accumulators into a per-lane running (best, second best) per row, in registers, as the online softmax
//                                of attention.hip keeps its running maximum.  Nothing of a score tile reaches LDS or memory.
//   nearest_combine_kernel<T>    with more than one split: one thread per row combines the splits' pairs from the workspace.
//
// Both finish through nr_finish: idx, sqrtf of the winners, and the copy of the winning rows of x2.  The order rule is a total order on
// (key, column), so no combine depends on its order; nothing here may be contracted.
#include <hip/hip_runtime.h>

#include <cstdint>

#pragma clang fp contract(off)

#include "si_hip.h"
#include "si_hip_internal.h"
#include "si_nearest.h"

#include "cdist_dev.h"
#include "nearest_plan.h"

namespace {

namespace plan = si_nearest_plan;

constexpr unsigned NR_NONE = 0xffffffffu;   // the key of "no candidate yet"; its column is NR_NOCOL
constexpr int NR_NOCOL = 0x7fffffff;

struct NrArgs {
    const void* x1;
    const void* x2;
    int* idx;
    float* dist;
    void* rows;
    u32x2* ws;                  // [B][p][splits][k] of (key, column)
    int batch, p, r, m, k;
    int x1_ld, x2_ld, rows_ld;
    int x1_sb, x2_sb, rows_sb;  // x1_sb / x2_sb: 0 for a broadcast operand
    int splits, tiles_per_split, r_tiles;
    int rows_vec;               // the winning rows travel as 16-byte vectors
};

// the comparison key of one pair of rows: cdist_mm_kernel's s, then its order-preserving integer image with NaN in front
__device__ __forceinline__ unsigned nr_key(float n1, float n2, float acc) {
    float s = (n1 + n2) - 2.0f * acc;
    s = s < 0.0f ? 0.0f : s;
    return s != s ? 0u : __float_as_uint(s) + 1u;
}
__device__ __forceinline__ float nr_dist(unsigned key) { return key == 0u ? __uint_as_float(0x7fc00000u) : sqrtf(__uint_as_float(key - 1u)); }

// a row's running best K candidates
template <int K>
struct NrTop {
    unsigned key[K];
    int col[K];
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int i = 0; i < K; ++i) { key[i] = NR_NONE; col[i] = NR_NOCOL; }
    }
    // a candidate whose column is above every column this lane has seen: a strict < keeps the lower column
    __device__ __forceinline__ void push_ascending(unsigned k, int c) {
        if (K == 2) {
            const bool second = k < key[K - 1];
            key[K - 1] = second ? k : key[K - 1];
            col[K - 1] = second ? c : col[K - 1];
        }
        if (k < key[0]) {
            if (K == 2) { key[K - 1] = key[0]; col[K - 1] = col[0]; }
            key[0] = k;
            col[0] = c;
        }
    }
    // any candidate: (key, column) lexicographically
    __device__ __forceinline__ void push(unsigned k, int c) {
        if (K == 2) {
            const bool second = k < key[K - 1] || (k == key[K - 1] && c < col[K - 1]);
            key[K - 1] = second ? k : key[K - 1];
            col[K - 1] = second ? c : col[K - 1];
        }
        if (k < key[0] || (k == key[0] && c < col[0])) {
            if (K == 2) { key[K - 1] = key[0]; col[K - 1] = col[0]; }
            key[0] = k;
            col[0] = c;
        }
    }
    // the lane `mask` away holds the same row over other columns: both take the best K of the union
    __device__ __forceinline__ void meet(int mask) {
        unsigned ok[K];
        int oc[K];
#pragma unroll
        for (int i = 0; i < K; ++i) {
            ok[i] = (unsigned)__shfl_xor((int)key[i], mask);
            oc[i] = __shfl_xor(col[i], mask);
        }
#pragma unroll
        for (int i = 0; i < K; ++i) push(ok[i], oc[i]);
    }
};

// What every workgroup ends with: thread t < 64 holds the final candidates of row m0 + t of batch item b.  idx and dist by that thread;
// then the 256 threads copy the 64 winning rows of x2.  `win`: 64 ints of LDS.
template <typename T>
__device__ __forceinline__ void nr_finish(const NrArgs& a, int b, int m0, int tid, const unsigned (&key)[2], const int (&col)[2], int* win) {
    typedef typename CdMm<T>::item_t item_t;
    constexpr int VW = CdMm<T>::VW;
    if (tid < plan::kTile && m0 + tid < a.p) {
        const size_t o = ((size_t)b * a.p + m0 + tid) * a.k;
        for (int i = 0; i < a.k; ++i) {
            if (a.idx) a.idx[o + i] = col[i];
            if (a.dist) a.dist[o + i] = nr_dist(key[i]);
        }
    }
    if (!a.rows) return;
    // (a row always has a candidate, r >= 1; the comparison keeps the copy inside x2 whatever a workspace held)
    if (tid < plan::kTile) win[tid] = (unsigned)col[0] < (unsigned)a.r ? col[0] : 0;
    __syncthreads();
    const T* const x2 = static_cast<const T*>(a.x2) + (size_t)b * a.x2_sb;
    T* const rows = static_cast<T*>(a.rows) + (size_t)b * a.rows_sb;
    const int per_row = a.rows_vec ? a.m / VW : a.m;
    for (int i = tid; i < plan::kTile * per_row; i += 256) {
        const int rl = i / per_row, e = i - rl * per_row;
        if (m0 + rl >= a.p) break;
        const T* const src = x2 + (size_t)win[rl] * a.x2_ld;
        T* const dst = rows + (size_t)(m0 + rl) * a.rows_ld;
        if (a.rows_vec) *reinterpret_cast<item_t*>(dst + e * VW) = *reinterpret_cast<const item_t*>(src + e * VW);
        else dst[e] = src[e];
    }
    __syncthreads();   // (the next batch item writes win)
}

template <typename T, bool VEC, int K>
__global__ __launch_bounds__(256) void nearest_kernel(const NrArgs a) {
    typedef CdMm<T> G;
    typedef typename G::item_t item_t;
    constexpr bool HALF = sizeof(T) == 2;
    constexpr int NR = HALF ? 8 : 16;   // rows a lane holds
    __shared__ __attribute__((aligned(16))) T lds[G::LDS_ELEMS];
    __shared__ float norms[SI_G64_BM + SI_G64_BN];   // n1 of the panel's 64 rows, then n2 of the tile's 64 columns
    __shared__ unsigned red_key[2][SI_G64_BM][K];    // [wn]: what the lanes of a wave found for a row
    __shared__ int red_col[2][SI_G64_BM][K];
    __shared__ int win[SI_G64_BM];

    const int p_tile = (int)blockIdx.x / a.splits, sp = (int)blockIdx.x - p_tile * a.splits;
    const int m0 = p_tile * SI_G64_BM;
    const int t0 = sp * a.tiles_per_split;
    const int t1 = t0 + a.tiles_per_split < a.r_tiles ? t0 + a.tiles_per_split : a.r_tiles;   // (t0 >= t1: a split without columns)
    const int tid = threadIdx.x;
    const SiG64Stage st = si_g64_stage(tid);
    const int kv = st.kv, r0 = st.r0;
    const SiG64Lane ln = si_g64_lane(tid);
    const int l15 = tid & 15, g4 = (tid & 63) >> 4;   // the 16 x 16 step's lane maps (fp16)
    const int nk = (a.m + G::BK - 1) / G::BK;

    for (int b = blockIdx.z; b < a.batch; b += gridDim.z) {
        const T* const x1 = static_cast<const T*>(a.x1) + (size_t)b * a.x1_sb;
        const T* const x2 = static_cast<const T*>(a.x2) + (size_t)b * a.x2_sb;

        NrTop<K> top[NR];
#pragma unroll
        for (int e = 0; e < NR; ++e) top[e].clear();

        for (int ct = t0; ct < t1; ++ct) {
            const int n0 = ct * SI_G64_BN;
            const bool first = ct == t0;   // n1 does not depend on the column tile: it is added up on the first one
            item_t pa[2], pb[2];
            auto load_tile = [&](int kt) {
                const int k = kt * G::BK + kv * G::VW;
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    pa[q] = cd_load_item<T, VEC>(x1, m0 + r0 + 32 * q, a.p, a.x1_ld, k, a.m);
                    pb[q] = cd_load_item<T, VEC>(x2, n0 + r0 + 32 * q, a.r, a.x2_ld, k, a.m);
                }
            };

            float qa[2] = {0.0f, 0.0f}, qb[2] = {0.0f, 0.0f};   // this thread's partial squared norms of the rows it stages
            f32x16 acc32;
            f32x4 acc16[2][2];
#pragma unroll
            for (int e = 0; e < 16; ++e) acc32[e] = 0.0f;
#pragma unroll
            for (int e = 0; e < 4; ++e) acc16[e >> 1][e & 1] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

            load_tile(0);
            for (int kt = 0; kt < nk; ++kt) {
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    *reinterpret_cast<item_t*>(lds + (r0 + 32 * q) * G::LDL + kv * G::VW) = pa[q];
                    *reinterpret_cast<item_t*>(lds + (SI_G64_BM + r0 + 32 * q) * G::LDL + kv * G::VW) = pb[q];
                    if (first) qa[q] = cd_add_squares<item_t, G::VW>(qa[q], pa[q]);
                    qb[q] = cd_add_squares<item_t, G::VW>(qb[q], pb[q]);
                }
                __syncthreads();
                if (kt + 1 < nk) load_tile(kt + 1);   // in flight during the MFMAs
                if constexpr (!HALF) {
                    si_g64_mma(lds, ln, acc32);
                } else {
                    // two steps of 32 k; lane (l15, g4) reads the 8 halves k = 32 s + 8 g4 .. + 7 of rows 16 t + l15 of the wave's 32 x 32
                    const T* const As = lds + (ln.wm * 32 + l15) * G::LDL + g4 * 8;
                    const T* const Bs = lds + (SI_G64_BM + ln.wn * 32 + l15) * G::LDL + g4 * 8;
#pragma unroll
                    for (int s = 0; s < G::BK / 32; ++s) {
                        f16x8 fa[2], fb[2];
#pragma unroll
                        for (int t = 0; t < 2; ++t) {
                            fa[t] = *reinterpret_cast<const f16x8*>(As + t * 16 * G::LDL + s * 32);
                            fb[t] = *reinterpret_cast<const f16x8*>(Bs + t * 16 * G::LDL + s * 32);
                        }
#pragma unroll
                        for (int ti = 0; ti < 2; ++ti)
#pragma unroll
                            for (int tj = 0; tj < 2; ++tj) acc16[ti][tj] = si_mma16(fa[ti], fb[tj], acc16[ti][tj]);
                    }
                }
                __syncthreads();
            }

            // ---- the norms: the eight partials of a row side by side in LDS (the staging image is free), then one thread per row, in order
            float* const part = reinterpret_cast<float*>(lds);   // [128 rows][8]
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                if (first) part[(r0 + 32 * q) * 8 + kv] = qa[q];
                part[(SI_G64_BM + r0 + 32 * q) * 8 + kv] = qb[q];
            }
            __syncthreads();
            if (tid < SI_G64_BM + SI_G64_BN && (first || tid >= SI_G64_BM)) {
                float n = part[tid * 8];
#pragma unroll
                for (int v = 1; v < 8; ++v) n = n + part[tid * 8 + v];
                norms[tid] = n;
            }
            __syncthreads();

            // ---- the fold: a lane's columns come in ascending order, tile after tile
            if constexpr (!HALF) {
                const int col = ln.col(n0);
                if (col < a.r) {
                    const float n2 = norms[SI_G64_BM + col - n0];
#pragma unroll
                    for (int e = 0; e < 16; ++e) top[e].push_ascending(nr_key(norms[ln.row0() + Mma<32>::row(e)], n2, acc32[e]), col);
                }
            } else {
#pragma unroll
                for (int tj = 0; tj < 2; ++tj) {
                    const int cl = ln.wn * 32 + tj * 16 + l15;
                    if (n0 + cl >= a.r) continue;
                    const float n2 = norms[SI_G64_BM + cl];
#pragma unroll
                    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            top[ti * 4 + e].push_ascending(nr_key(norms[ln.wm * 32 + ti * 16 + 4 * g4 + Mma<16>::row(e)], n2, acc16[ti][tj][e]), n0 + cl);
                }
            }
            __syncthreads();   // (the next tile stages into the image the norms were read from, and rewrites n2)
        }

        // ---- the lanes of a wave that share a row (32 under fp32, 16 under fp16: the low bits of the lane), then the two waves wn
#pragma unroll
        for (int mask = 1; mask < (HALF ? 16 : 32); mask <<= 1)
#pragma unroll
            for (int e = 0; e < NR; ++e) top[e].meet(mask);
        if ((HALF ? l15 : ln.l31) == 0) {
#pragma unroll
            for (int e = 0; e < NR; ++e) {
                const int rl = HALF ? ln.wm * 32 + (e >> 2) * 16 + 4 * g4 + Mma<16>::row(e & 3) : ln.row0() + Mma<32>::row(e);
#pragma unroll
                for (int i = 0; i < K; ++i) {
                    red_key[ln.wn][rl][i] = top[e].key[i];
                    red_col[ln.wn][rl][i] = top[e].col[i];
                }
            }
        }
        __syncthreads();
        unsigned key[2] = {NR_NONE, NR_NONE};
        int col[2] = {NR_NOCOL, NR_NOCOL};
        if (tid < SI_G64_BM) {
            NrTop<K> fin;
            fin.clear();
#pragma unroll
            for (int w = 0; w < 2; ++w)
#pragma unroll
                for (int i = 0; i < K; ++i) fin.push(red_key[w][tid][i], red_col[w][tid][i]);
#pragma unroll
            for (int i = 0; i < K; ++i) { key[i] = fin.key[i]; col[i] = fin.col[i]; }
        }
        if (a.splits == 1) {
            nr_finish<T>(a, b, m0, tid, key, col, win);
        } else {
            if (tid < SI_G64_BM && m0 + tid < a.p) {
                u32x2* const w = a.ws + (((size_t)b * a.p + m0 + tid) * a.splits + sp) * K;
#pragma unroll
                for (int i = 0; i < K; ++i) w[i] = u32x2{key[i], (unsigned)col[i]};
            }
            __syncthreads();   // (the next batch item writes red_key / red_col)
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void nearest_combine_kernel(const NrArgs a) {
    __shared__ int win[plan::kTile];
    const int m0 = (int)blockIdx.x * plan::kTile, tid = threadIdx.x;
    for (int b = blockIdx.z; b < a.batch; b += gridDim.z) {
        NrTop<2> fin;
        fin.clear();
        if (tid < plan::kTile && m0 + tid < a.p) {
            const u32x2* const w = a.ws + ((size_t)b * a.p + m0 + tid) * a.splits * a.k;
            for (int i = 0; i < a.splits * a.k; ++i) fin.push(w[i][0], (int)w[i][1]);
        }
        nr_finish<T>(a, b, m0, tid, fin.key, fin.col, win);
    }
}

// ---- host
template <typename T>
uint64_t nr_bytes(int items, int rows, int width, int sb, int ld) {
    return plan::OperandExtent(items, rows, width, sb, ld) * sizeof(T);
}

// SI_E_BADARG first; rows, idx, dist may be null (not all of them)
template <typename T>
int nr_refusal(const SiNearestDesc* d, const void* x1, const void* x2, const int* idx, const float* dist, const void* rows) {
    constexpr bool HALF = sizeof(T) == 2;
    if (!d || !x1 || !x2) return SI_E_BADARG;
    const int rc = plan::Check(*d, HALF);
    if (rc == SI_E_BADARG) return rc;
    const int B = plan::Batch(*d);
    const uint64_t b1 = nr_bytes<T>(d->b1, d->p, d->m, d->x1_sb, d->x1_ld), b2 = nr_bytes<T>(d->b2, d->r, d->m, d->x2_sb, d->x2_ld);
    const uint64_t small = (uint64_t)B * (uint64_t)d->p * (uint64_t)d->k * 4u;
    const void* const outs[3] = {idx, dist, rows};
    const uint64_t sizes[3] = {small, small, nr_bytes<T>(B, d->p, d->m, d->rows_sb, d->rows_ld)};
    for (int i = 0; i < 3; ++i) {
        if (!outs[i]) continue;
        if (si_ranges_overlap(outs[i], sizes[i], x1, b1) || si_ranges_overlap(outs[i], sizes[i], x2, b2)) return SI_E_BADARG;
        for (int j = 0; j < i; ++j)
            if (outs[j] && si_ranges_overlap(outs[i], sizes[i], outs[j], sizes[j])) return SI_E_BADARG;
    }
    if (rc) return rc;
    if (HALF && (!si_aligned_to(x1, 16) || !si_aligned_to(x2, 16) || (rows && !si_aligned_to(rows, 16)))) return SI_E_UNSUPPORTED;
    return 0;
}

template <typename T>
bool nr_vector(const SiNearestDesc* d, const void* x1, const void* x2) {
    return plan::Vector(*d, (int)(16 / sizeof(T)), si_aligned_to(x1, 16), si_aligned_to(x2, 16));
}

template <typename T, bool VEC>
void nr_launch_k(int k, dim3 grid, hipStream_t s, const NrArgs& a) {
    if (k == 2) hipLaunchKernelGGL((nearest_kernel<T, VEC, 2>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((nearest_kernel<T, VEC, 1>), grid, dim3(256), 0, s, a);
}

template <typename T>
int nr_launch(const SiNearestDesc* d, const void* x1, const void* x2, int* idx, float* dist, void* rows, void* workspace, size_t workspace_bytes,
              si_stream_t stream) {
    if (!idx && !dist && !rows) return SI_E_BADARG;
    if (const int rc = nr_refusal<T>(d, x1, x2, idx, dist, rows)) return rc;
    const plan::Grid g = plan::MakeGrid(*d);
    if (g.splits > 1) {
        const uint64_t need = plan::WorkspaceBytes(*d, g.splits);
        if (!workspace || !si_aligned_to(workspace, 8) || workspace_bytes < need) return SI_E_BADARG;
        // the pairs written there must not land on an operand or an output
        const int B = plan::Batch(*d);
        const uint64_t small = (uint64_t)B * (uint64_t)d->p * (uint64_t)d->k * 4u;
        const void* const others[5] = {x1, x2, idx, dist, rows};
        const uint64_t sizes[5] = {nr_bytes<T>(d->b1, d->p, d->m, d->x1_sb, d->x1_ld), nr_bytes<T>(d->b2, d->r, d->m, d->x2_sb, d->x2_ld), small, small,
                                   nr_bytes<T>(B, d->p, d->m, d->rows_sb, d->rows_ld)};
        for (int i = 0; i < 5; ++i)
            if (others[i] && si_ranges_overlap(workspace, need, others[i], sizes[i])) return SI_E_BADARG;
    }
    NrArgs a{};
    a.x1 = x1; a.x2 = x2; a.idx = idx; a.dist = dist; a.rows = rows; a.ws = static_cast<u32x2*>(workspace);
    a.batch = plan::Batch(*d); a.p = d->p; a.r = d->r; a.m = d->m; a.k = d->k;
    a.x1_ld = d->x1_ld; a.x2_ld = d->x2_ld; a.rows_ld = d->rows_ld;
    a.x1_sb = d->b1 > 1 ? d->x1_sb : 0; a.x2_sb = d->b2 > 1 ? d->x2_sb : 0; a.rows_sb = a.batch > 1 ? d->rows_sb : 0;
    a.splits = g.splits; a.tiles_per_split = g.tiles_per_split; a.r_tiles = g.r_tiles;
    a.rows_vec = rows && plan::RowsVector(*d, (int)(16 / sizeof(T)), si_aligned_to(x2, 16), si_aligned_to(rows, 16)) ? 1 : 0;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(g.x, 1, g.z);
    if constexpr (sizeof(T) == 2) {
        nr_launch_k<T, true>(d->k, grid, s, a);
    } else {
        if (nr_vector<T>(d, x1, x2)) nr_launch_k<T, true>(d->k, grid, s, a);
        else nr_launch_k<T, false>(d->k, grid, s, a);
    }
    if (g.splits > 1) hipLaunchKernelGGL((nearest_combine_kernel<T>), dim3(g.combine_x, 1, g.z), dim3(256), 0, s, a);
    return (int)hipGetLastError();
}

template <typename T>
const char* nr_name(const SiNearestDesc* d, const void* x1, const void* x2, const void* rows) {
    static const char* const names[3][2] = {{"nearest_kernel<float, true, 1>", "nearest_kernel<float, true, 2>"},
                                            {"nearest_kernel<float, false, 1>", "nearest_kernel<float, false, 2>"},
                                            {"nearest_kernel<_Float16, true, 1>", "nearest_kernel<_Float16, true, 2>"}};
    if (nr_refusal<T>(d, x1, x2, nullptr, nullptr, rows) != 0) return "none";
    const int row = sizeof(T) == 2 ? 2 : (nr_vector<T>(d, x1, x2) ? 0 : 1);
    return names[row][d->k - 1];
}

}  // namespace

extern "C" {

size_t si_hip_nearest_workspace_bytes(const SiNearestDesc* d) {
    if (!d || plan::Check(*d, false) != 0) return 0;
    return plan::WorkspaceBytes(*d, plan::Splits(*d));
}

int si_hip_nearest_f32(const SiNearestDesc* d, const float* x1, const float* x2, int* idx, float* dist, float* rows, void* workspace,
                       size_t workspace_bytes, si_stream_t stream) {
    return nr_launch<float>(d, x1, x2, idx, dist, rows, workspace, workspace_bytes, stream);
}

int si_hip_nearest_f16(const SiNearestDesc* d, const void* x1, const void* x2, int* idx, float* dist, void* rows, void* workspace,
                       size_t workspace_bytes, si_stream_t stream) {
    return nr_launch<_Float16>(d, x1, x2, idx, dist, rows, workspace, workspace_bytes, stream);
}

const char* si_hip_nearest_kernel_name(const SiNearestDesc* d, const void* x1, const void* x2, const void* rows, int half) {
    return half ? nr_name<_Float16>(d, x1, x2, rows) : nr_name<float>(d, x1, x2, rows);
}

}  // extern "C"
