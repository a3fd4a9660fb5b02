// cdist.hip -- torch.cdist (include/si_cdist.h): out[b, i, j] = || x1[b, i, :] - x2[b, j, :] ||_norm for every pair of rows.
//
//   cdist_mm_kernel<T, VEC>       norm 2 as sqrt(n1[i] + n2[j] - 2 x1[i] . x2[j]) on the matrix cores: the product is an A . B^T GEMM with both
//                                 operands [row][k], the form the 64 x 64 core of si_mma_dev.h was written for.  fp32 takes that core as it is
//                                 (si_g64_stage / si_g64_lane / si_g64_mma, v_mfma_f32_32x32x2_f32); fp16 keeps its tile and its staging map on
//                                 K-tiles of 64 halves and runs si_mma16 (v_mfma_f32_16x16x32_f16), 2 x 2 accumulators of 16 x 16 per wave.
//                                 The squared row norms ride on the staging: the thread that puts a K vector of a row into LDS adds its
//                                 squares to a private accumulator; the eight staging threads of a row meet in LDS after the K loop.
//   cdist_direct_kernel<T, NORM>  the difference form on the vector ALU, 4 x 4 outputs per lane from an LDS image of 32 k at a time.
//
// Both: a workgroup owns a 64 x 64 tile of out for one batch item (blockIdx.z, looping when B > 65535), tiles numbered by si_g64_tile so that
// the tiles along r sharing a panel of x1 land on one XCD.  A lane stores one element at a time with the lane on the column.  The order of
// every addition is stated in the header; nothing here may be contracted.
#include <hip/hip_runtime.h>

#include <cstdint>

#pragma clang fp contract(off)

#include "si_cdist.h"
#include "si_hip.h"
#include "si_hip_internal.h"

#include "cdist_dev.h"
#include "cdist_plan.h"

namespace {

namespace plan = si_cdist_plan;

struct CdArgs {
    const void* x1;
    const void* x2;
    void* out;
    int batch, p, r, m;
    int x1_ld, x2_ld, out_ld;
    int x1_sb, x2_sb, out_sb;   // x1_sb / x2_sb: 0 for a broadcast operand
    int p_tiles, r_tiles;
};

// the epilogue of one output: contraction is off, so the sum, the difference and the root round as written; a NaN passes the clamp
__device__ __forceinline__ float cd_mm_result(float n1, float n2, float acc) {
    float s = (n1 + n2) - 2.0f * acc;
    s = s < 0.0f ? 0.0f : s;
    return sqrtf(s);
}

template <typename T, bool VEC>
__global__ __launch_bounds__(256) void cdist_mm_kernel(const CdArgs a) {
    typedef CdMm<T> G;
    typedef typename G::item_t item_t;
    constexpr bool HALF = sizeof(T) == 2;
    __shared__ __attribute__((aligned(16))) T lds[G::LDS_ELEMS];
    __shared__ float norms[SI_G64_BM + SI_G64_BN];   // n1 of the tile's 64 rows, then n2 of its 64 columns

    const SiG64Tile tile = si_g64_tile(a.p_tiles, a.r_tiles);
    if (tile.none) return;
    const int m0 = tile.m_tile * SI_G64_BM, n0 = tile.n_tile * SI_G64_BN;
    const int tid = threadIdx.x;
    const SiG64Stage st = si_g64_stage(tid);
    const int kv = st.kv, r0 = st.r0;
    const SiG64Lane ln = si_g64_lane(tid);
    const int l15 = tid & 15, g4 = (tid & 63) >> 4;   // the 16 x 16 step's lane maps (fp16)
    const int nk = (a.m + G::BK - 1) / G::BK;

    for (int b = blockIdx.z; b < a.batch; b += gridDim.z) {
        const T* const x1 = static_cast<const T*>(a.x1) + (size_t)b * a.x1_sb;
        const T* const x2 = static_cast<const T*>(a.x2) + (size_t)b * a.x2_sb;
        T* const out = static_cast<T*>(a.out) + (size_t)b * a.out_sb;

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
                qa[q] = cd_add_squares<item_t, G::VW>(qa[q], pa[q]);
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
            part[(r0 + 32 * q) * 8 + kv] = qa[q];
            part[(SI_G64_BM + r0 + 32 * q) * 8 + kv] = qb[q];
        }
        __syncthreads();
        if (tid < SI_G64_BM + SI_G64_BN) {
            float n = part[tid * 8];
#pragma unroll
            for (int v = 1; v < 8; ++v) n = n + part[tid * 8 + v];
            norms[tid] = n;
        }
        __syncthreads();

        // ---- epilogue: the lane on the column, one element per store
        if constexpr (!HALF) {
            const int col = ln.col(n0);
            if (col < a.r) {
                const float n2 = norms[SI_G64_BM + col - n0];
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int rl = ln.row0() + Mma<32>::row(e);
                    if (m0 + rl < a.p) out[(size_t)(m0 + rl) * a.out_ld + col] = si_store_cast<T>(cd_mm_result(norms[rl], n2, acc32[e]));
                }
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
                    for (int e = 0; e < 4; ++e) {
                        const int rl = ln.wm * 32 + ti * 16 + 4 * g4 + Mma<16>::row(e);
                        if (m0 + rl < a.p) out[(size_t)(m0 + rl) * a.out_ld + n0 + cl] = si_store_cast<T>(cd_mm_result(norms[rl], n2, acc16[ti][tj][e]));
                    }
            }
        }
        __syncthreads();   // (the next batch item stages into the image the norms were read from)
    }
}

// ---- the difference form
constexpr int CD_DK = 32, CD_DLD = CD_DK + 1;   // k per chunk; the row pitch in words (odd: 16 rows at one k lie in 16 banks)

template <int NORM>
__device__ __forceinline__ float cd_direct_step(float acc, float av, float bv) {
    const float d = fabsf(av - bv);
    if (NORM == SI_CDIST_NORM_1) return acc + d;
    if (NORM == SI_CDIST_NORM_INF) return (d > acc || d != d) ? d : acc;
    return acc + d * d;
}

template <typename T, int NORM>
__global__ __launch_bounds__(256) void cdist_direct_kernel(const CdArgs a) {
    __shared__ float As[plan::kTile * CD_DLD];
    __shared__ float Bs[plan::kTile * CD_DLD];

    const SiG64Tile tile = si_g64_tile(a.p_tiles, a.r_tiles);
    if (tile.none) return;
    const int m0 = tile.m_tile * plan::kTile, n0 = tile.n_tile * plan::kTile;
    const int tid = threadIdx.x;
    const int tx = tid & 15, ty = tid >> 4;   // outputs: rows 4 ty + i, columns tx + 16 j
    const int sk = tid & 31, sr = tid >> 5;   // staging: element sk of rows sr + 8 i of the chunk

    for (int b = blockIdx.z; b < a.batch; b += gridDim.z) {
        const T* const x1 = static_cast<const T*>(a.x1) + (size_t)b * a.x1_sb;
        const T* const x2 = static_cast<const T*>(a.x2) + (size_t)b * a.x2_sb;
        T* const out = static_cast<T*>(a.out) + (size_t)b * a.out_sb;

        float acc[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = 0.0f;

        for (int k0 = 0; k0 < a.m; k0 += CD_DK) {
            // a row or a k that does not exist is staged as 0 on both sides: |0 - 0| changes no accumulator
            const bool kin = k0 + sk < a.m;
#pragma unroll
            for (int i = 0; i < plan::kTile / 8; ++i) {
                const int row = sr + 8 * i;
                As[row * CD_DLD + sk] = (kin && m0 + row < a.p) ? (float)x1[(size_t)(m0 + row) * a.x1_ld + k0 + sk] : 0.0f;
                Bs[row * CD_DLD + sk] = (kin && n0 + row < a.r) ? (float)x2[(size_t)(n0 + row) * a.x2_ld + k0 + sk] : 0.0f;
            }
            __syncthreads();
            const int kn = a.m - k0 < CD_DK ? a.m - k0 : CD_DK;
            for (int k = 0; k < kn; ++k) {
                float av[4], bv[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    av[i] = As[(4 * ty + i) * CD_DLD + k];
                    bv[i] = Bs[(tx + 16 * i) * CD_DLD + k];
                }
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[i][j] = cd_direct_step<NORM>(acc[i][j], av[i], bv[j]);
            }
            __syncthreads();
        }

#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = m0 + 4 * ty + i;
            if (row >= a.p) continue;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int col = n0 + tx + 16 * j;
                if (col < a.r) out[(size_t)row * a.out_ld + col] = si_store_cast<T>(NORM == SI_CDIST_NORM_2 ? sqrtf(acc[i][j]) : acc[i][j]);
            }
        }
    }
}

// ---- host
template <typename T>
int cd_refusal(const SiCdistDesc* d, const void* x1, const void* x2, const void* out) {
    if (!d || !x1 || !x2 || !out) return SI_E_BADARG;
    const int rc = plan::Check(*d);
    if (rc == SI_E_BADARG) return rc;
    // (the extents of a descriptor refused as unsupported may be beyond 31 bits: the overlap is looked at all the same, in 64 bits)
    if (plan::Overlaps(*d, (uintptr_t)x1, (uintptr_t)x2, (uintptr_t)out, sizeof(T))) return SI_E_BADARG;
    return rc;
}

template <typename T>
bool cd_vector(const SiCdistDesc* d, const void* x1, const void* x2) {
    return plan::Vector(*d, (int)(16 / sizeof(T)), (uintptr_t)x1, (uintptr_t)x2);
}

template <typename T>
int cd_launch(const SiCdistDesc* d, const void* x1, const void* x2, void* out, si_stream_t stream) {
    if (const int rc = cd_refusal<T>(d, x1, x2, out)) return rc;
    const plan::Grid g = plan::MakeGrid(*d);
    CdArgs a{};
    a.x1 = x1; a.x2 = x2; a.out = out;
    a.batch = plan::Batch(*d); a.p = d->p; a.r = d->r; a.m = d->m;
    a.x1_ld = d->x1_ld; a.x2_ld = d->x2_ld; a.out_ld = d->out_ld;
    a.x1_sb = d->b1 > 1 ? d->x1_sb : 0; a.x2_sb = d->b2 > 1 ? d->x2_sb : 0; a.out_sb = a.batch > 1 ? d->out_sb : 0;
    a.p_tiles = g.p_tiles; a.r_tiles = g.r_tiles;
    const dim3 grid(g.x, 1, g.z), block(256);
    hipStream_t s = (hipStream_t)stream;
    if (plan::FormOf(*d) == plan::kMm) {
        if (cd_vector<T>(d, x1, x2)) hipLaunchKernelGGL((cdist_mm_kernel<T, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((cdist_mm_kernel<T, false>), grid, block, 0, s, a);
    } else if (d->norm == SI_CDIST_NORM_1) {
        hipLaunchKernelGGL((cdist_direct_kernel<T, SI_CDIST_NORM_1>), grid, block, 0, s, a);
    } else if (d->norm == SI_CDIST_NORM_2) {
        hipLaunchKernelGGL((cdist_direct_kernel<T, SI_CDIST_NORM_2>), grid, block, 0, s, a);
    } else {
        hipLaunchKernelGGL((cdist_direct_kernel<T, SI_CDIST_NORM_INF>), grid, block, 0, s, a);
    }
    return (int)hipGetLastError();
}

template <typename T>
const char* cd_name(const SiCdistDesc* d, const void* x1, const void* x2, const void* out) {
    static const char* const names[2][5] = {
        {"cdist_mm_kernel<float, true>", "cdist_mm_kernel<float, false>", "cdist_direct_kernel<float, 1>", "cdist_direct_kernel<float, 2>",
         "cdist_direct_kernel<float, 3>"},
        {"cdist_mm_kernel<_Float16, true>", "cdist_mm_kernel<_Float16, false>", "cdist_direct_kernel<_Float16, 1>", "cdist_direct_kernel<_Float16, 2>",
         "cdist_direct_kernel<_Float16, 3>"}};
    if (cd_refusal<T>(d, x1, x2, out) != 0) return "none";
    const char* const* row = names[sizeof(T) == 2 ? 1 : 0];
    if (plan::FormOf(*d) == plan::kMm) return row[cd_vector<T>(d, x1, x2) ? 0 : 1];
    return row[1 + d->norm];
}

}  // namespace

extern "C" {

int si_hip_cdist_f32(const SiCdistDesc* d, const float* x1, const float* x2, float* out, si_stream_t stream) {
    return cd_launch<float>(d, x1, x2, out, stream);
}

int si_hip_cdist_f16(const SiCdistDesc* d, const void* x1, const void* x2, void* out, si_stream_t stream) {
    return cd_launch<_Float16>(d, x1, x2, out, stream);
}

const char* si_hip_cdist_kernel_name(const SiCdistDesc* d, const void* x1, const void* x2, const void* out, int half) {
    return half ? cd_name<_Float16>(d, x1, x2, out) : cd_name<float>(d, x1, x2, out);
}

}  // extern "C"
