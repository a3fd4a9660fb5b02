// conv1d.hip -- the temporal convolution kernels of nn.Conv1d (include/si_conv1d.h).  Forms, reduction orders, contract and refusals: the
// header.  Form choice, spans, LDS sizes, image indices, the grid and the 31-bit checks: conv1d_plan.h.
//
// Dense.  A workgroup of four waves owns 64 output channels x 64 output positions of one batch item and one group; wave w owns channels
// 16 w .. 16 w + 15 of the block and all 64 positions as four 16-column MFMA tiles, one accumulator each (four independent chains).  With
// lane = 16 g + x (g = 0..3, x = 0..15) one MFMA step is one tap k of one channel group:
//     A  the filters: lane holds w[oc = 16 tile + x][channel 4 q + g][k] (fp32) or channels 32 q + 8 g + 0..7 (fp16), read from the packed
//        image in lane order -- one coalesced 256-byte / 1-KiB load per step, requested for a group of 8 / 4 steps before the group's first MFMA
//     B  the input: lane holds x[channel ..][(pos0 + 16 j + x) s - pl + k d] from the LDS image of the workgroup's span
// The C/D map puts the POSITION on x and channel 4 g + r in register r: every register stores a run of 16 contiguous positions of one row.
//
// LDS image of the span (tile - 1) s + (K - 1) d + 1, real zeros where the position is outside [0, L) or the channel beyond the group:
//   fp32  [channel of the chunk][pitch] floats, pitch = 16 mod 32: the 32 lanes of a half-wave (two channel rows of 16 consecutive positions
//         at stride 1) read 32 different banks.  A chunk is up to 32 channels; chunks are walked in ascending order between two barriers.
//   fp16  [position][chunk + 8] halves: the 128, 64 or 32 channels of the chunk and 8 halves of padding, transposed while it is staged (rows
//         are read from global memory along L, element by element, whatever their alignment; a lane writes the 8 channels of one position
//         as one 16-byte operand); an operand is one 16-byte read.
//
// Depthwise.  A workgroup of four waves owns four (n, c) rows x 256 positions; a wave stages its row's span and its K taps as floats, a lane
// produces four consecutive outputs with one fmaf per tap, taps ascending.  At stride 1 and dilation 1 a staged position is read once for
// the four outputs it belongs to.
//
// No integer division by a runtime value: the grid is 3-D (position tile; channel block, group or row block; batch item).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <type_traits>

#include "conv1d_plan.h"
#include "si_conv1d.h"
#include "si_hip_internal.h"

#pragma clang fp contract(off)

namespace {

namespace plan = si_conv1d_plan;

constexpr int C1_THREADS = 256;
static_assert(plan::kBlockOc == plan::kTileOc * (C1_THREADS / 64), "a wave owns 16 output channels");
static_assert(plan::kDwRows == C1_THREADS / 64 && plan::kDwPos == 64 * plan::kDwRun, "a wave owns one depthwise row");

struct Conv1dArgs {
    const void* x;
    const void* w;
    const float* bias;
    void* y;
    int c, l, oc, lo, k, stride, dilation, pad_left;
    int cg, ocg, oc_tiles, chan_steps, grouped, oc_blocks;
    int chunk, pitch, span;
    int x_sn, x_sc, y_sn, y_sc;
    int act;
    float act_param;
};

__device__ __forceinline__ f32x4 c1_mma(float w, float b, f32x4 acc) { return __builtin_amdgcn_mfma_f32_16x16x4f32(w, b, acc, 0, 0, 0); }
__device__ __forceinline__ f32x4 c1_mma(f16x8 w, f16x8 b, f32x4 acc) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(w, b, acc, 0, 0, 0); }

template <typename T>
__global__ __launch_bounds__(C1_THREADS) void conv1d_dense_kernel(Conv1dArgs a) {
    constexpr bool HALF = sizeof(T) == 2;
    typedef typename std::conditional<HALF, f16x8, float>::type Frag;
    constexpr int CH_STEP = HALF ? plan::kChanF16 : plan::kChanF32;   // channels of one MFMA step
    constexpr int U = HALF ? 4 : 8;                                   // steps whose A operands are requested together
    extern __shared__ __attribute__((aligned(16))) unsigned char c1_smem[];

    const int tid = (int)threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int x = lane & 15, g = lane >> 4;
    const int lo0 = (int)blockIdx.x * plan::kTilePos;
    const int group = a.grouped ? (int)blockIdx.y : 0;
    const int ocb0 = a.grouped ? 0 : (int)blockIdx.y;
    const int n = (int)blockIdx.z;

    const T* const xg = static_cast<const T*>(a.x) + n * a.x_sn + group * a.cg * a.x_sc;
    const int li0 = lo0 * a.stride - a.pad_left;   // the input position of LDS position 0
    const int chunk = a.chunk;                     // fp32: a multiple of 4 up to 32; fp16: 32, 64 or 128
    const int row8 = (chunk + plan::kRowPadF16) / 8;   // fp16: 16-byte operands in one position's row of the image

    for (int ob = 0; ob < a.oc_blocks; ++ob) {
        const int tile = (ocb0 + ob) * (C1_THREADS / 64) + wave;   // the wave's tile of 16 output channels inside the group
        const bool wave_live = tile < a.oc_tiles;
        f32x4 acc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        const Frag* const wt = static_cast<const Frag*>(a.w) + (size_t)((group * a.oc_tiles + (wave_live ? tile : 0)) * a.chan_steps) * a.k * 64 + lane;

        for (int c0 = 0; c0 < a.cg; c0 += chunk) {
            __syncthreads();   // (the previous chunk's reads are over)
            if constexpr (HALF) {
                // a lane owns a position, a wave 8 channels at a time: 8 rows of global memory are read along L (128 contiguous bytes per
                // row and instruction) and the 8 halves of one position are written as ONE 16-byte operand of the transposed image
                f16x8* const img = reinterpret_cast<f16x8*>(c1_smem);
                for (int c8 = wave; c8 < chunk / 8; c8 += C1_THREADS / 64) {
                    const bool ch_live = c0 + 8 * c8 < a.cg;   // (cg % 8 == 0: the 8 channels are in or out together)
                    const T* const rows = xg + (ch_live ? (c0 + 8 * c8) * a.x_sc : 0);
                    for (int p = lane; p < a.span; p += 64) {
                        const int li = li0 + p;
                        f16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
                        if (ch_live && li >= 0 && li < a.l) {
#pragma unroll
                            for (int j = 0; j < 8; ++j) v[j] = rows[j * a.x_sc + li];
                        }
                        img[p * row8 + c8] = v;
                    }
                }
            } else {
                float* const img = reinterpret_cast<float*>(c1_smem);
                for (int cl = wave; cl < chunk; cl += C1_THREADS / 64) {
                    const bool ch_live = c0 + cl < a.cg;
                    const T* const row = xg + (ch_live ? (c0 + cl) * a.x_sc : 0);
                    for (int p = lane; p < a.span; p += 64) {
                        const int li = li0 + p;
                        float v = 0.0f;
                        if (ch_live && li >= 0 && li < a.l) v = row[li];
                        img[cl * a.pitch + p] = v;
                    }
                }
            }
            __syncthreads();
            if (!wave_live) continue;

            // this lane's B operand of column tile j at tap k of channel step q (relative to the chunk), in Frag elements
            const Frag* bp;
            int col_step, tap_step, q_step;
            if constexpr (HALF) {
                bp = reinterpret_cast<const Frag*>(c1_smem) + (x * a.stride) * row8 + g;
                col_step = 16 * a.stride * row8;
                tap_step = a.dilation * row8;
                q_step = plan::kChanF16 / 8;
            } else {
                bp = reinterpret_cast<const Frag*>(c1_smem) + g * a.pitch + x * a.stride;
                col_step = 16 * a.stride;
                tap_step = a.dilation;
                q_step = plan::kChanF32 * a.pitch;
            }
            // the steps of the chunk in one ascending run: channel step q, then tap k.  Their A operands lie one behind the other in the
            // image; the U operands of a group are all requested before its first MFMA
            const int q0 = c0 / CH_STEP;
            const int q_end = min((c0 + chunk) / CH_STEP, a.chan_steps);
            const int total = (q_end - q0) * a.k;
            const Frag* const wp = wt + (size_t)q0 * a.k * 64;
            int k = 0, boff = 0, s = 0;
            for (; s + U <= total; s += U) {
                Frag wv[U];
                int bo[U];
#pragma unroll
                for (int u = 0; u < U; ++u) wv[u] = wp[(s + u) * 64];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    bo[u] = boff;
                    boff += tap_step;
                    if (++k == a.k) {
                        k = 0;
                        boff += q_step - a.k * tap_step;
                    }
                }
#pragma unroll
                for (int u = 0; u < U; ++u)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[j] = c1_mma(wv[u], bp[bo[u] + j * col_step], acc[j]);
            }
            for (; s < total; ++s) {
                const Frag wv = wp[s * 64];
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] = c1_mma(wv, bp[boff + j * col_step], acc[j]);
                boff += tap_step;
                if (++k == a.k) {
                    k = 0;
                    boff += q_step - a.k * tap_step;
                }
            }
        }

        // epilogue: register r of accumulator j is channel 16 tile + 4 g + r at position lo0 + 16 j + x
        if (wave_live) {
            T* const yg = static_cast<T*>(a.y) + n * a.y_sn + group * a.ocg * a.y_sc;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int o = tile * plan::kTileOc + 4 * g + r;
                if (o >= a.ocg) continue;
                const float bv = a.bias ? a.bias[group * a.ocg + o] : 0.0f;
                T* const yr = yg + o * a.y_sc;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int lo = lo0 + 16 * j + x;
                    if (lo < a.lo) yr[lo] = si_store_cast<T>(si_act(a.act, acc[j][r] + bv, a.act_param));
                }
            }
        }
    }
}

template <typename T>
__global__ __launch_bounds__(C1_THREADS) void conv1d_depthwise_kernel(Conv1dArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char c1_smem[];
    const int tid = (int)threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int lo0 = (int)blockIdx.x * plan::kDwPos;
    const int c = (int)blockIdx.y * plan::kDwRows + wave;
    const int n = (int)blockIdx.z;
    const bool live = c < a.c;   // (a wave without a row meets the barrier, nothing else)

    // per wave: the row's span, then its K taps, as floats
    float* const img = reinterpret_cast<float*>(c1_smem) + wave * (a.span + a.k);
    float* const wl = img + a.span;
    const int li0 = lo0 * a.stride - a.pad_left;
    if (live) {
        const T* const row = static_cast<const T*>(a.x) + n * a.x_sn + c * a.x_sc;
        for (int p = lane; p < a.span; p += 64) {
            const int li = li0 + p;
            float v = 0.0f;
            if (li >= 0 && li < a.l) v = (float)row[li];
            img[p] = v;
        }
        const T* const wr = static_cast<const T*>(a.w) + c * a.k;
        for (int k = lane; k < a.k; k += 64) wl[k] = (float)wr[k];
    }
    __syncthreads();
    if (!live) return;

    float acc[plan::kDwRun];
#pragma unroll
    for (int r = 0; r < plan::kDwRun; ++r) acc[r] = 0.0f;
    // positions of the tile beyond lo read inside the staged span all the same: the span is that of the whole tile
    const float* const bp = img + lane * plan::kDwRun * a.stride;
    if (a.stride == 1 && a.dilation == 1) {
        // the four windows of a lane overlap in all but three positions: position t of the lane's span is read ONCE and meets tap t - r of
        // output r; the taps slide through four registers.  Every output still sums its taps in ascending order, one fmaf each, and a tap
        // outside 0 .. K - 1 is skipped, not multiplied by zero (the value it would meet may be a NaN of another output's window)
        static_assert(plan::kDwRun == 4, "four sliding taps");
        float w0 = 0.0f, w1 = 0.0f, w2 = 0.0f, w3 = 0.0f;
        for (int t = 0; t < a.k + 3; ++t) {
            w3 = w2; w2 = w1; w1 = w0;
            w0 = t < a.k ? wl[t] : 0.0f;
            const float v = bp[t];
            if (t < a.k) acc[0] = fmaf(w0, v, acc[0]);
            if (t >= 1 && t - 1 < a.k) acc[1] = fmaf(w1, v, acc[1]);
            if (t >= 2 && t - 2 < a.k) acc[2] = fmaf(w2, v, acc[2]);
            if (t >= 3) acc[3] = fmaf(w3, v, acc[3]);
        }
    } else {
        for (int k = 0; k < a.k; ++k) {
            const float wv = wl[k];
#pragma unroll
            for (int r = 0; r < plan::kDwRun; ++r) acc[r] = fmaf(wv, bp[r * a.stride + k * a.dilation], acc[r]);
        }
    }
    const float bv = a.bias ? a.bias[c] : 0.0f;
    T* const yr = static_cast<T*>(a.y) + n * a.y_sn + c * a.y_sc;
#pragma unroll
    for (int r = 0; r < plan::kDwRun; ++r) {
        const int lo = lo0 + lane * plan::kDwRun + r;
        if (lo < a.lo) yr[lo] = si_store_cast<T>(si_act(a.act, acc[r] + bv, a.act_param));
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------
plan::Shape shape_of(const SiConv1dDesc* d) {
    plan::Shape s;
    s.n = d->n; s.c = d->c; s.l = d->l; s.oc = d->oc; s.lo = d->lo; s.k = d->k;
    s.stride = d->stride; s.dilation = d->dilation; s.pad_left = d->pad_left; s.groups = d->groups;
    return s;
}

// the filter alone (c, oc, k, groups): what the image functions look at
plan::Shape filter_of(const SiConv1dDesc* d) {
    plan::Shape s;
    s.n = s.l = s.lo = s.stride = s.dilation = 1;
    s.pad_left = 0;
    s.c = d->c; s.oc = d->oc; s.k = d->k; s.groups = d->groups;
    return s;
}

int check_filter(const SiConv1dDesc* d, bool half) {
    if (!d) return SI_E_BADARG;
    const plan::Shape s = filter_of(d);
    if (!plan::Positive(s) || !plan::GroupsDivide(s)) return SI_E_BADARG;
    if (half && !plan::HalfOk(s)) return SI_E_UNSUPPORTED;
    const uint64_t elems = plan::WeightElems(s, half);
    if (elems == 0 || elems > plan::kIndexLimit) return SI_E_UNSUPPORTED;
    return 0;
}

// everything that can be decided without a device and without the pointers: SI_E_BADARG / SI_E_UNSUPPORTED / 0
int check_desc(const SiConv1dDesc* d, bool half) {
    if (!d) return SI_E_BADARG;
    const plan::Shape s = shape_of(d);
    if (!plan::Positive(s) || !plan::GroupsDivide(s)) return SI_E_BADARG;
    if (plan::ImpliedRightPad(s) < 0) return SI_E_BADARG;
    if (!plan::StridesOk(d->n, d->c, d->x_sn, d->x_sc, d->l) || !plan::StridesOk(d->n, d->oc, d->y_sn, d->y_sc, d->lo)) return SI_E_BADARG;
    const int rc = check_filter(d, half);
    if (rc != 0) return rc;
    if (plan::ViewExtent(d->n, d->c, d->x_sn, d->x_sc, d->l) == 0 || plan::ViewExtent(d->n, d->oc, d->y_sn, d->y_sc, d->lo) == 0) return SI_E_UNSUPPORTED;
    plan::Grid grid;
    if (!plan::MakeGrid(s, grid)) return SI_E_UNSUPPORTED;
    if (plan::LdsBytes(s, half) == 0 || !plan::PositionsFit(s)) return SI_E_UNSUPPORTED;
    return 0;
}

int check_ptrs(const SiConv1dDesc* d, const void* x, const void* w, const float* bias, const void* y, bool half) {
    if (!x || !w || !y) return SI_E_BADARG;
    const uint64_t es = half ? 2 : 4;
    const uint64_t y_bytes = plan::ViewExtent(d->n, d->oc, d->y_sn, d->y_sc, d->lo) * es;
    const uint64_t x_bytes = plan::ViewExtent(d->n, d->c, d->x_sn, d->x_sc, d->l) * es;
    if (si_ranges_overlap(y, y_bytes, x, x_bytes)) return SI_E_BADARG;
    if (si_ranges_overlap(y, y_bytes, w, plan::WeightElems(filter_of(d), half) * es)) return SI_E_BADARG;
    if (bias && si_ranges_overlap(y, y_bytes, bias, (uint64_t)d->oc * 4)) return SI_E_BADARG;
    if (half && plan::FormOf(shape_of(d)) == plan::kDense && !si_aligned_to(w, 16)) return SI_E_UNSUPPORTED;
    if (!si_aligned_to(x, es) || !si_aligned_to(y, es) || !si_aligned_to(w, es)) return SI_E_UNSUPPORTED;
    return 0;
}

template <typename T>
int run(const SiConv1dDesc* d, const void* x, const void* w, const float* bias, void* y, si_stream_t stream) {
    constexpr bool half = sizeof(T) == 2;
    int rc = check_desc(d, half);
    if (rc != 0) return rc;
    rc = check_ptrs(d, x, w, bias, y, half);
    if (rc != 0) return rc;
    const plan::Shape s = shape_of(d);
    const plan::Form form = plan::FormOf(s);
    plan::Grid grid;
    plan::MakeGrid(s, grid);
    Conv1dArgs a;
    memset(&a, 0, sizeof(a));
    a.x = x; a.w = w; a.bias = bias; a.y = y;
    a.c = d->c; a.l = d->l; a.oc = d->oc; a.lo = d->lo; a.k = d->k; a.stride = d->stride; a.dilation = d->dilation; a.pad_left = d->pad_left;
    a.cg = plan::Cg(s); a.ocg = plan::Ocg(s); a.oc_tiles = plan::OcTiles(s); a.chan_steps = plan::ChanSteps(s, half);
    a.grouped = d->groups > 1 ? 1 : 0;
    a.oc_blocks = grid.oc_blocks_per_wg;
    a.x_sn = (int)d->x_sn; a.x_sc = (int)d->x_sc; a.y_sn = (int)d->y_sn; a.y_sc = (int)d->y_sc;
    a.act = d->act; a.act_param = d->act_param;
    const size_t lds = (size_t)plan::LdsBytes(s, half);
    hipStream_t st = (hipStream_t)stream;
    const dim3 g3(grid.x, grid.y, grid.z);
    if (form == plan::kDepthwise) {
        a.span = (int)plan::Span(s, plan::kDwPos);
        hipLaunchKernelGGL((conv1d_depthwise_kernel<T>), g3, dim3(C1_THREADS), lds, st, a);
    } else {
        a.span = (int)plan::Span(s, plan::kTilePos);
        a.pitch = (int)plan::PitchF32((uint64_t)a.span);
        a.chunk = half ? plan::ChunkF16(s) : plan::ChunkF32(s);
        hipLaunchKernelGGL((conv1d_dense_kernel<T>), g3, dim3(C1_THREADS), lds, st, a);
    }
    SI_HIP_TRY(hipGetLastError());
    return 0;
}

// dense: w [oc][cg][k] fp32 -> [group][oc tile][channel step q][tap][lane] operand elements: lane 16 g + x holds filter (16 tile + x) of the
// group at channel 4 q + g (fp32) or channels 32 q + 8 g + 0..7 (fp16); filters beyond the group's and channels beyond cg are zeros.
// depthwise: the filters [c][k] as they are, rounded to the storage type
template <typename T>
int pack_weights(const SiConv1dDesc* d, const float* w, T* image) {
    constexpr bool half = sizeof(T) == 2;
    const int rc = check_filter(d, half);
    if (rc != 0) return rc;
    if (!w || !image) return SI_E_BADARG;
    const plan::Shape s = filter_of(d);
    if (plan::FormOf(s) == plan::kDepthwise) {
        for (size_t i = 0; i < (size_t)s.c * s.k; ++i) image[i] = (T)w[i];
        return 0;
    }
    const int cg = plan::Cg(s), ocg = plan::Ocg(s), per = half ? 8 : 1;
    for (int grp = 0; grp < s.groups; ++grp)
        for (int tile = 0; tile < plan::OcTiles(s); ++tile)
            for (int q = 0; q < plan::ChanSteps(s, half); ++q)
                for (int k = 0; k < s.k; ++k)
                    for (int lane = 0; lane < 64; ++lane) {
                        const int x = lane & 15, g = lane >> 4;
                        const int o = tile * plan::kTileOc + x;
                        T* const dst = image + plan::WeightIndex(s, half, grp, tile, q, k, lane) * per;
                        for (int j = 0; j < per; ++j) {
                            const int c = half ? plan::kChanF16 * q + 8 * g + j : plan::kChanF32 * q + g;
                            const float v = (o < ocg && c < cg) ? w[((size_t)(grp * ocg + o) * cg + c) * s.k + k] : 0.0f;
                            dst[j] = (T)v;
                        }
                    }
    return 0;
}

}  // namespace

extern "C" {

int si_hip_conv1d_f32(const SiConv1dDesc* d, const float* x, const float* weights, const float* bias, float* y, si_stream_t stream) {
    return run<float>(d, x, weights, bias, y, stream);
}

int si_hip_conv1d_f16(const SiConv1dDesc* d, const void* x, const void* weights, const float* bias, void* y, si_stream_t stream) {
    return run<_Float16>(d, x, weights, bias, y, stream);
}

size_t si_hip_conv1d_weight_bytes(const SiConv1dDesc* d, int half) {
    if (check_filter(d, half != 0) != 0) return 0;
    return (size_t)plan::WeightElems(filter_of(d), half != 0) * (half ? 2 : 4);
}

int si_hip_conv1d_pack_weights_f32(const SiConv1dDesc* d, const float* w, float* image) { return pack_weights<float>(d, w, image); }

int si_hip_conv1d_pack_weights_f16(const SiConv1dDesc* d, const float* w, void* image) {
    return pack_weights<_Float16>(d, w, static_cast<_Float16*>(image));
}

const char* si_hip_conv1d_kernel_name(const SiConv1dDesc* d, const void* x, const void* y, int half) {
    if (check_desc(d, half != 0) != 0 || !x || !y) return "none";
    const size_t es = half ? 2 : 4;
    if (!si_aligned_to(x, es) || !si_aligned_to(y, es)) return "none";
    static const char* const names[2][2] = {{"conv1d_dense_kernel<float>", "conv1d_depthwise_kernel<float>"},
                                            {"conv1d_dense_kernel<_Float16>", "conv1d_depthwise_kernel<_Float16>"}};
    return names[half ? 1 : 0][plan::FormOf(shape_of(d)) == plan::kDepthwise ? 1 : 0];
}

}  // extern "C"
