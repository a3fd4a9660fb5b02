// rnn.hip -- the recurrent step kernel of nn.LSTM / nn.GRU (include/si_rnn.h): t launches per layer, one per time step of both directions,
// and the small state-output launch.  Stages, views, contract and refusals: the header.  Grid, sizes and 31-bit checks: rnn_plan.h.
//
// A workgroup of four waves owns (direction, 16 batch rows, 64 hidden units); wave w owns units 16 w .. 16 w + 15 of the block for ALL gates.
// With lane = 16 g + x (g = 0..3, x = 0..15) a wave computes per gate q
//     P_q^T = W_q H^T    16 units x 16 batch rows.  W_q (rows q H + unit of W_hh) is the A operand, read from the packed image in lane order
//                        (one coalesced 256-byte / 1-KiB load per k step and gate, from L2, requested 8 / 4 k steps ahead of their MFMAs);
//                        H^T is the B operand from the LDS tile of h_{t-1}, loaded once per k step and used by all G gates.
// The C/D map puts the BATCH ROW on x and unit 4 g + r in register r: a lane holds the G pre-activations of four neighbouring units of one
// batch item, adds the projected gates, applies the cell and stores four neighbouring elements of y (and of c).  The k order is 0 .. K - 1.
//
// LDS tile of h_{t-1}, zero where the row is beyond batch or k beyond H (never loaded):
//   fp32  [padded k][17] floats: the operand read of k step s is (4 s + g) * 17 + x; the staging store of neighbouring k is 17 words apart.
//   fp16  [padded k / 8][16 rows][8 halves]: a lane reads 16 bytes, chunk 4 s + g of row x: the 64 lanes read one contiguous KiB.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <type_traits>

#include "rnn_plan.h"
#include "si_hip_internal.h"
#include "si_rnn.h"

#pragma clang fp contract(off)

namespace {

namespace plan = si_rnn_plan;

constexpr int RNN_THREADS = 256;
static_assert(plan::kBlockUnits == plan::kWaveUnits * (RNN_THREADS / 64), "a wave owns 16 units");
static_assert(SI_RNN_TILE_ROWS == plan::kTileRows && SI_RNN_BLOCK_UNITS == plan::kBlockUnits && SI_RNN_MAX_HIDDEN == plan::kMaxHidden, "header and plan agree");

struct RnnArgs {
    const void* gates;
    const void* whh;
    const float* bhn;
    void* y;
    float* c;
    int t, n, h, step;
    int kp, unit_tiles, row_tiles, unit_blocks;
    int g_st, g_sb, y_st, y_sb;
};

// the forms of nn.Sigmoid (ops.hip) and nn.Tanh (UnaryOp 16)
__device__ __forceinline__ float rnn_tanh(float v) { return tanhf(v); }

// four neighbouring elements from `u` on, as floats: halves by one 8-byte load (H % 8 == 0: in or out together), floats one by one
template <typename T>
__device__ __forceinline__ void load4(const T* p, int u, int h, float (&v)[4]) {
    if constexpr (sizeof(T) == 2) {
        f16x4 t = {0, 0, 0, 0};
        if (u < h) t = *reinterpret_cast<const f16x4*>(p + u);
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = (float)t[r];
    } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = (u + r < h) ? p[u + r] : 0.0f;
    }
}

__device__ __forceinline__ f32x4 rnn_mma(float w, float h, f32x4 acc) { return __builtin_amdgcn_mfma_f32_16x16x4f32(w, h, acc, 0, 0, 0); }
__device__ __forceinline__ f32x4 rnn_mma(f16x8 w, f16x8 h, f32x4 acc) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(w, h, acc, 0, 0, 0); }

template <typename T>
__device__ __forceinline__ void store4(T* p, int u, int h, const float (&v)[4]) {
    if constexpr (sizeof(T) == 2) {
        if (u < h) {
            f16x4 t;
#pragma unroll
            for (int r = 0; r < 4; ++r) t[r] = si_store_cast<_Float16>(v[r]);
            *reinterpret_cast<f16x4*>(p + u) = t;
        }
    } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (u + r < h) p[u + r] = v[r];
    }
}

template <typename T, int G>
__global__ __launch_bounds__(RNN_THREADS) void rnn_step_kernel(RnnArgs a) {
    constexpr bool HALF = sizeof(T) == 2;
    constexpr bool LSTM = G == 4;
    extern __shared__ __attribute__((aligned(16))) unsigned char rnn_smem[];

    const int tid = (int)threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int x = lane & 15, g = lane >> 4;
    int bid = (int)blockIdx.x;
    const int ub = bid % a.unit_blocks;
    bid /= a.unit_blocks;
    const int rt = bid % a.row_tiles;
    const int dir = bid / a.row_tiles;

    const int time = dir ? a.t - 1 - a.step : a.step;
    const int prev = dir ? time + 1 : time - 1;
    const bool first = a.step == 0;
    const int b0 = rt * plan::kTileRows;
    const int tile = ub * (RNN_THREADS / 64) + wave;   // the wave's unit tile
    const int u0 = tile * plan::kWaveUnits;
    const bool wave_live = u0 < a.h;                   // (a wave without units stages the tile and meets the barrier, nothing else)

    T* const yd = static_cast<T*>(a.y) + dir * a.h;

    // this lane's share of the epilogue: batch item b, units u .. u + 3.  Its operands are requested BEFORE the product, so that their
    // latency passes behind the staging and the MFMA loop instead of in front of the cell arithmetic
    const int b = b0 + x;
    const int u = u0 + 4 * g;
    const bool lane_live = wave_live && b < a.n && u < a.h;
    float pre[G][4], cv[4] = {0.0f, 0.0f, 0.0f, 0.0f}, hprev[4] = {0.0f, 0.0f, 0.0f, 0.0f}, bn[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int q = 0; q < G; ++q)
#pragma unroll
        for (int r = 0; r < 4; ++r) pre[q][r] = 0.0f;
    if (lane_live) {
        const T* const gp = static_cast<const T*>(a.gates) + time * a.g_st + b * a.g_sb + dir * (G * a.h);
#pragma unroll
        for (int q = 0; q < G; ++q) load4<T>(gp + q * a.h, u, a.h, pre[q]);
        if constexpr (LSTM) {
            if (!first) load4<float>(a.c + (dir * a.n + b) * a.h, u, a.h, cv);
        } else {
            if (!first) load4<T>(yd + prev * a.y_st + b * a.y_sb, u, a.h, hprev);
            if (a.bhn) load4<float>(a.bhn + dir * a.h, u, a.h, bn);
        }
    }

    f32x4 acc[G];
#pragma unroll
    for (int q = 0; q < G; ++q) acc[q] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    if (!first) {
        const T* const hp = yd + prev * a.y_st;
        if constexpr (HALF) {
            f16x8* const img = reinterpret_cast<f16x8*>(rnn_smem);
            const int chunks = a.kp / 8;
            for (int idx = tid; idx < plan::kTileRows * chunks; idx += RNN_THREADS) {
                const int ch = idx % chunks, row = idx / chunks;
                f16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
                if (b0 + row < a.n && ch * 8 < a.h) v = *reinterpret_cast<const f16x8*>(hp + (b0 + row) * a.y_sb + ch * 8);
                img[ch * plan::kTileRows + row] = v;
            }
        } else {
            float* const img = reinterpret_cast<float*>(rnn_smem);
            for (int idx = tid; idx < plan::kTileRows * a.kp; idx += RNN_THREADS) {
                const int k = idx % a.kp, row = idx / a.kp;
                float v = 0.0f;
                if (b0 + row < a.n && k < a.h) v = hp[(b0 + row) * a.y_sb + k];
                img[k * (plan::kTileRows + 1) + row] = v;
            }
        }
        __syncthreads();
        if (wave_live) {
            // k steps in ascending order, U at a time: the U * G operand loads of a group are all requested before its first MFMA (one wave
            // per SIMD: with a load in front of every MFMA the loop ran at one L2 round trip per k step)
            typedef typename std::conditional<HALF, f16x8, float>::type Frag;
            constexpr int U = HALF ? 4 : 8;
            constexpr int PITCH = HALF ? plan::kTileRows : plan::kTileRows + 1;   // operand elements between two k groups of the h tile
            const Frag* const img = reinterpret_cast<const Frag*>(rnn_smem) + g * PITCH + x;
            const int ks = a.kp / (HALF ? 32 : 4);
            const Frag* wp = static_cast<const Frag*>(a.whh) + ((dir * a.unit_tiles + tile) * ks) * (G * 64) + lane;
            int s = 0;
            for (; s + U <= ks; s += U, wp += U * G * 64) {
                Frag wv[U][G], hb[U];
#pragma unroll
                for (int j = 0; j < U; ++j) {
#pragma unroll
                    for (int q = 0; q < G; ++q) wv[j][q] = wp[(j * G + q) * 64];
                    hb[j] = img[4 * (s + j) * PITCH];
                }
#pragma unroll
                for (int j = 0; j < U; ++j)
#pragma unroll
                    for (int q = 0; q < G; ++q) acc[q] = rnn_mma(wv[j][q], hb[j], acc[q]);
            }
            for (; s < ks; ++s, wp += G * 64) {
                const Frag hb = img[4 * s * PITCH];
#pragma unroll
                for (int q = 0; q < G; ++q) acc[q] = rnn_mma(wp[q * 64], hb, acc[q]);
            }
        }
    }

    if (!lane_live) return;
#pragma unroll
    for (int q = 0; q < G; ++q)
        if (LSTM || q < 2) {   // (the GRU's n keeps its product apart: r multiplies it)
#pragma unroll
            for (int r = 0; r < 4; ++r) pre[q][r] = pre[q][r] + acc[q][r];
        }

    float hv[4];
    if constexpr (LSTM) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float ig = si_sigmoid_fast(pre[0][r]), fg = si_sigmoid_fast(pre[1][r]), gg = rnn_tanh(pre[2][r]), og = si_sigmoid_fast(pre[3][r]);
            cv[r] = fg * cv[r] + ig * gg;
            hv[r] = og * rnn_tanh(cv[r]);
        }
        store4<float>(a.c + (dir * a.n + b) * a.h, u, a.h, cv);
    } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float rg = si_sigmoid_fast(pre[0][r]), zg = si_sigmoid_fast(pre[1][r]);
            const float ng = rnn_tanh(pre[2][r] + rg * (acc[2][r] + bn[r]));
            hv[r] = (1.0f - zg) * ng + zg * hprev[r];
        }
    }
    store4<T>(yd + time * a.y_st + b * a.y_sb, u, a.h, hv);
}

struct StateArgs {
    const void* y;
    const float* c;
    void *hn, *cn;
    int t, n, h, dirs, y_st, y_sb;
};

// h_n[d, b, u] = y[d ? 0 : t - 1, b, d H + u]; c_n = c rounded to the storage type
template <typename T>
__global__ __launch_bounds__(256) void rnn_state_kernel(StateArgs a) {
    const unsigned total = (unsigned)(a.dirs * a.n * a.h);   // (below 2^31: an unsigned index plus the grid's stride does not wrap)
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int u = (int)(i % (unsigned)a.h), b = (int)((i / (unsigned)a.h) % (unsigned)a.n), d = (int)(i / (unsigned)(a.h * a.n));
        if (a.hn) static_cast<T*>(a.hn)[i] = static_cast<const T*>(a.y)[(d ? 0 : a.t - 1) * a.y_st + b * a.y_sb + d * a.h + u];
        if (a.cn) static_cast<T*>(a.cn)[i] = si_store_cast<T>(a.c[i]);
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------
// everything that can be decided without a device and without the pointers: SI_E_BADARG / SI_E_UNSUPPORTED / 0
int check_desc(const SiRnnDesc* d, bool half) {
    if (!d) return SI_E_BADARG;
    const int G = plan::Gates(d->cell);
    if (G == 0) return SI_E_BADARG;
    if (d->t <= 0 || d->batch <= 0 || d->input <= 0 || d->hidden <= 0 || d->dirs < 1 || d->dirs > 2) return SI_E_BADARG;
    if (d->step0 < 0 || d->step0 > d->t) return SI_E_BADARG;
    if (d->hidden > plan::kMaxHidden) return SI_E_UNSUPPORTED;
    const long long gw = (long long)d->dirs * G * d->hidden, yw = (long long)d->dirs * d->hidden;
    const long long st[3] = {d->x_st, d->g_st, d->y_st}, sb[3] = {d->x_sb, d->g_sb, d->y_sb}, width[3] = {d->input, gw, yw};
    for (int i = 0; i < 3; ++i)
        if (st[i] < width[i] || sb[i] < width[i]) return SI_E_BADARG;
    for (int i = 0; i < 3; ++i)
        if (plan::ViewExtent(d->t, d->batch, st[i], sb[i], width[i]) == 0) return SI_E_UNSUPPORTED;
    if (!plan::RowsDisjoint(d->t, d->batch, d->y_st, d->y_sb, yw)) return SI_E_BADARG;
    plan::Grid grid;
    if (!plan::MakeGrid(d->batch, d->hidden, d->dirs, grid)) return SI_E_UNSUPPORTED;
    const uint64_t img = plan::WhhImageElems(d->cell, d->hidden, d->dirs, half), state = plan::StateElems(d->batch, d->hidden, d->dirs);
    if (img == 0 || img > plan::kIndexLimit || state > plan::kIndexLimit) return SI_E_UNSUPPORTED;
    if (half) {
        if (d->hidden % 8 != 0 || d->input % 8 != 0) return SI_E_UNSUPPORTED;
        for (int i = 0; i < 3; ++i)
            if (st[i] % 8 != 0 || sb[i] % 8 != 0) return SI_E_UNSUPPORTED;
    }
    return 0;
}

// the pointers of the layer entries: null, overlap (SI_E_BADARG), the fp16 alignment rule (SI_E_UNSUPPORTED)
int check_ptrs(const SiRnnDesc* d, const void* gates, const void* whh, const void* y, const float* c, const void* hn, const void* cn, bool half) {
    const bool lstm = d->cell == SI_RNN_LSTM;
    if (!gates || !whh || !y || (lstm && !c) || (!lstm && cn)) return SI_E_BADARG;
    const uint64_t es = half ? 2 : 4;
    const int G = plan::Gates(d->cell);
    const uint64_t y_bytes = plan::ViewExtent(d->t, d->batch, d->y_st, d->y_sb, (long long)d->dirs * d->hidden) * es;
    const uint64_t g_bytes = plan::ViewExtent(d->t, d->batch, d->g_st, d->g_sb, (long long)d->dirs * G * d->hidden) * es;
    const uint64_t state = plan::StateElems(d->batch, d->hidden, d->dirs);
    if (si_ranges_overlap(y, y_bytes, gates, g_bytes)) return SI_E_BADARG;
    if (si_ranges_overlap(y, y_bytes, whh, plan::WhhImageElems(d->cell, d->hidden, d->dirs, half) * es)) return SI_E_BADARG;
    if (lstm && si_ranges_overlap(y, y_bytes, c, state * 4)) return SI_E_BADARG;
    if (hn && si_ranges_overlap(y, y_bytes, hn, state * es)) return SI_E_BADARG;
    if (cn && si_ranges_overlap(y, y_bytes, cn, state * es)) return SI_E_BADARG;
    if (half && (!si_aligned_to(gates, 16) || !si_aligned_to(whh, 16) || !si_aligned_to(y, 16) || (hn && !si_aligned_to(hn, 16)) ||
                 (cn && !si_aligned_to(cn, 16))))
        return SI_E_UNSUPPORTED;
    return 0;
}

template <typename T, int G>
int launch_steps(const SiRnnDesc* d, RnnArgs a, hipStream_t stream) {
    constexpr bool half = sizeof(T) == 2;
    const size_t lds = (size_t)plan::LdsBytes(d->hidden, half);
    SI_HIP_TRY(si_allow_dynamic_lds(rnn_step_kernel<T, G>, lds));
    plan::Grid grid;
    plan::MakeGrid(d->batch, d->hidden, d->dirs, grid);
    for (int s = d->step0; s < d->t; ++s) {
        a.step = s;
        hipLaunchKernelGGL((rnn_step_kernel<T, G>), dim3((unsigned)grid.blocks), dim3(RNN_THREADS), lds, stream, a);
        SI_HIP_TRY(hipGetLastError());
    }
    return 0;
}

template <typename T>
int run(const SiRnnDesc* d, const void* gates, const void* whh, const float* bhn, void* y, float* c, void* hn, void* cn, si_stream_t stream) {
    constexpr bool half = sizeof(T) == 2;
    int rc = check_desc(d, half);
    if (rc != 0) return rc;
    rc = check_ptrs(d, gates, whh, y, c, hn, cn, half);
    if (rc != 0) return rc;
    plan::Grid grid;
    plan::MakeGrid(d->batch, d->hidden, d->dirs, grid);
    RnnArgs a;
    a.gates = gates; a.whh = whh; a.bhn = bhn; a.y = y; a.c = c;
    a.t = d->t; a.n = d->batch; a.h = d->hidden; a.step = 0;
    a.kp = plan::PaddedK(d->hidden, half);
    a.unit_tiles = plan::UnitTiles(d->hidden);
    a.row_tiles = (int)grid.row_tiles; a.unit_blocks = (int)grid.unit_blocks;
    a.g_st = (int)d->g_st; a.g_sb = (int)d->g_sb; a.y_st = (int)d->y_st; a.y_sb = (int)d->y_sb;
    hipStream_t s = (hipStream_t)stream;
    rc = d->cell == SI_RNN_LSTM ? launch_steps<T, 4>(d, a, s) : launch_steps<T, 3>(d, a, s);
    if (rc != 0) return rc;
    if (hn || cn) {
        StateArgs sa;
        sa.y = y; sa.c = c; sa.hn = hn; sa.cn = cn;
        sa.t = d->t; sa.n = d->batch; sa.h = d->hidden; sa.dirs = d->dirs; sa.y_st = a.y_st; sa.y_sb = a.y_sb;
        const size_t total = (size_t)plan::StateElems(d->batch, d->hidden, d->dirs);
        hipLaunchKernelGGL((rnn_state_kernel<T>), dim3(si_grid_for(total)), dim3(256), 0, s, sa);
        SI_HIP_TRY(hipGetLastError());
    }
    return 0;
}

// W_hh [dirs][G H][H] fp32 -> [dirs][unit tile][k step][gate][lane] operand elements: lane 16 g + x holds row (gate H + 16 tile + x) of W_hh
// at k = 4 s + g (fp32) or k = 32 s + 8 g + 0..7 (fp16); rows beyond H and k beyond H are zeros
template <typename T>
int pack_whh(const SiRnnDesc* d, const float* w, T* image) {
    constexpr bool half = sizeof(T) == 2;
    const int rc = check_desc(d, half);
    if (rc != 0) return rc;
    if (!w || !image) return SI_E_BADARG;
    const int G = plan::Gates(d->cell), H = d->hidden, per = half ? 8 : 1;
    const int ks = plan::PaddedK(H, half) / plan::KStep(half);
    for (int dir = 0; dir < d->dirs; ++dir)
        for (int tile = 0; tile < plan::UnitTiles(H); ++tile)
            for (int s = 0; s < ks; ++s)
                for (int q = 0; q < G; ++q)
                    for (int lane = 0; lane < 64; ++lane) {
                        const int x = lane & 15, g = lane >> 4;
                        const int unit = tile * plan::kWaveUnits + x;
                        T* const dst = image + plan::WhhImageIndex(d->cell, H, half, dir, tile, s, q, lane) * per;
                        for (int j = 0; j < per; ++j) {
                            const int k = half ? 32 * s + 8 * g + j : 4 * s + g;
                            const float v = (unit < H && k < H) ? w[((size_t)dir * G * H + (size_t)q * H + unit) * H + k] : 0.0f;
                            dst[j] = (T)v;
                        }
                    }
    return 0;
}

}  // namespace

extern "C" {

int si_hip_rnn_layer_f32(const SiRnnDesc* d, const float* gates, const float* whh, const float* b_hn, float* y, float* c, float* h_n, float* c_n,
                         si_stream_t stream) {
    return run<float>(d, gates, whh, b_hn, y, c, h_n, c_n, stream);
}

int si_hip_rnn_layer_f16(const SiRnnDesc* d, const void* gates, const void* whh, const float* b_hn, void* y, float* c, void* h_n, void* c_n,
                         si_stream_t stream) {
    return run<_Float16>(d, gates, whh, b_hn, y, c, h_n, c_n, stream);
}

size_t si_hip_rnn_workspace_bytes(const SiRnnDesc* d, int which, int half) {
    if (check_desc(d, half != 0) != 0) return 0;
    const size_t es = half ? 2 : 4;
    switch (which) {
        case SI_RNN_WS_GATES: return (size_t)plan::DenseGateElems(d->cell, d->t, d->batch, d->hidden, d->dirs) * es;
        case SI_RNN_WS_STATE: return d->cell == SI_RNN_LSTM ? (size_t)plan::StateElems(d->batch, d->hidden, d->dirs) * 4 : 0;
        case SI_RNN_WS_WHH: return (size_t)plan::WhhImageElems(d->cell, d->hidden, d->dirs, half != 0) * es;
        default: return 0;
    }
}

int si_hip_rnn_pack_whh_f32(const SiRnnDesc* d, const float* w_hh, float* image) { return pack_whh<float>(d, w_hh, image); }

int si_hip_rnn_pack_whh_f16(const SiRnnDesc* d, const float* w_hh, void* image) { return pack_whh<_Float16>(d, w_hh, static_cast<_Float16*>(image)); }

const char* si_hip_rnn_kernel_name(const SiRnnDesc* d, const void* gates, const void* y, int half) {
    if (check_desc(d, half != 0) != 0 || !gates || !y) return "none";
    if (half && (!si_aligned_to(gates, 16) || !si_aligned_to(y, 16))) return "none";
    static const char* const names[2][2] = {{"rnn_step_kernel<float, 4>", "rnn_step_kernel<float, 3>"},
                                            {"rnn_step_kernel<_Float16, 4>", "rnn_step_kernel<_Float16, 3>"}};
    return names[half ? 1 : 0][d->cell == SI_RNN_LSTM ? 0 : 1];
}

}  // extern "C"
