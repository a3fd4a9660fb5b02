// detect_topk.hip -- NMS-free detection post-processing (include/si_topk.h): the max_det best candidates of an image's score matrix by
// (score descending, flat index ascending), selected on the device and written as si_hip_detect_postprocess_f32 writes its detections.
//
// The work is a radix SELECT, not a sort of everything.  A score s > prob_threshold becomes the order-preserving integer `key` (-0.0 folded
// onto +0.0 first), and three histogram / select pairs over its bits 31..21, 20..10 and 9..0 find the threshold key T = the take-th largest
// key, take = min(candidates, max_det), with gt = #{key > T} < take and need = take - gt keys equal to T still to store.  Then
//   topk_collect_kernel        keys > T take slots [0, gt) by atomic add (the final sort restores their order); keys == T are counted per chunk
//   topk_collect_ties_kernel   chunk by chunk in flat-index order the equal keys get ranks; rank < need stores into slot gt + rank
//   topk_sort_write_kernel     bitonic sort of the take keys {key, ~f} in LDS, then dets / src_rows / net_boxes / extras
// Every pass uses one chunking: a workgroup owns kChunkRows = 256 consecutive rows of one image, a lane owns a row and walks its classes in
// ascending order, so a lane's candidates are consecutive flat indices and the lanes of a chunk follow one another in that order.
// SI_DETECT_CHANNELS: lane l reads pred[(4 + c) * ld + r0 + l], neighbouring lanes neighbouring addresses, nothing staged.  SI_DETECT_ROWS:
// slabs of 32 classes x 256 rows go through LDS (pitch 33 words: the lanes of a wave, rows apart, hit different banks), loaded with 128-byte
// runs along the rows of pred.  No launch waits on another workgroup; the order of the launches on the stream does that job.
//
// Compare and index work only; the box arithmetic is detect_post.h's, shared with postprocess.hip.
#include "si_topk.h"
#include "si_hip_internal.h"
#include "detect_topk_plan.h"
#include "detect_post.h"

#pragma clang fp contract(off)

namespace {

namespace plan = si_topk_plan;
constexpr int T = plan::kThreads;
constexpr int SLAB = plan::kSlabClasses, PITCH = SLAB + 1;
static_assert(plan::kChunkRows == T, "a lane owns a row of its chunk");

struct TopkArgs {
    const float* pred;
    long long image_ld;
    int rows, ld, classes, extra, box_format, multi_label, max_det;
    float threshold;
};

struct TopkWs {
    unsigned long long* keys;   // [n][max_det]
    unsigned* hist;             // [n][kLevels][kBins]
    unsigned* slot;             // [n]
    unsigned* state;            // [n][kStateWords]
    unsigned* ties;             // [n][chunks]
};

// order-preserving map float -> u32 (larger float <=> larger integer) with the two zeros on one key
__device__ __forceinline__ unsigned topk_key(float s) {
    const unsigned u = __float_as_uint(s == 0.0f ? 0.0f : s);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// f(c, score) for every class c of this lane's row, ascending.  Every thread of the workgroup calls it (SI_DETECT_ROWS has barriers inside);
// lanes behind the chunk's last row get no call.
template <int LAYOUT, class F>
__device__ __forceinline__ void topk_walk(const TopkArgs& a, const float* __restrict__ img, int r0, int nrows, float* stage, F&& f) {
    const bool live = (int)threadIdx.x < nrows;
    if (LAYOUT == plan::kChannels) {
        if (!live) return;
        const float* p = img + (size_t)4 * (size_t)a.ld + (size_t)(r0 + (int)threadIdx.x);
#pragma unroll 4
        for (int c = 0; c < a.classes; ++c) f(c, p[(size_t)c * (size_t)a.ld]);
    } else {
        const float* src = img + (size_t)r0 * (size_t)a.ld + 4;
        for (int c0 = 0; c0 < a.classes; c0 += SLAB) {
            const int w = min(SLAB, a.classes - c0);
            __syncthreads();    // the slab before this one has been walked
            if (w == SLAB) {
                for (int i = threadIdx.x; i < nrows * SLAB; i += T) stage[(i >> 5) * PITCH + (i & 31)] = src[(size_t)(i >> 5) * (size_t)a.ld + c0 + (i & 31)];
            } else {
                for (int i = threadIdx.x; i < nrows * w; i += T) {
                    const int r = i / w, c = i - r * w;
                    stage[r * PITCH + c] = src[(size_t)r * (size_t)a.ld + c0 + c];
                }
            }
            __syncthreads();
            if (live)
                for (int c = 0; c < w; ++c) f(c0 + c, stage[threadIdx.x * PITCH + c]);
        }
    }
}
static_assert(SLAB == 32, "the slab loader's shifts");

// g(c, key) for every kept candidate of this lane's row in flat-index order: c its class (multi_label) or the row's first-maximum label
template <int LAYOUT, class G>
__device__ __forceinline__ void topk_candidates(const TopkArgs& a, const float* __restrict__ img, int r0, int nrows, float* stage, G&& g) {
    if (a.multi_label) {
        topk_walk<LAYOUT>(a, img, r0, nrows, stage, [&](int c, float s) {
            if (s > a.threshold) g(c, topk_key(s));
        });
    } else {
        int label = -1;
        float best = -3.402823466e+38f;  // -FLT_MAX
        topk_walk<LAYOUT>(a, img, r0, nrows, stage, [&](int c, float s) {
            if (s > best) {
                best = s;
                label = c;
            }
        });
        if ((int)threadIdx.x < nrows && best > a.threshold) g(label, topk_key(best));
    }
}

__device__ __forceinline__ unsigned topk_flat(const TopkArgs& a, int row, int c) {
    return a.multi_label ? (unsigned)row * (unsigned)a.classes + (unsigned)c : (unsigned)row;
}
__device__ __forceinline__ unsigned long long topk_sort_key(unsigned key, unsigned flat) {
    return ((unsigned long long)key << 32) | (unsigned long long)(0xffffffffu - flat);   // larger sorts first: score down, flat index up
}

// ---- 0. clear the histograms and the slot counters (a kernel, not a memset: the sequence is replayed from captured graphs) -------------------
__global__ __launch_bounds__(T) void topk_clear_kernel(unsigned* __restrict__ words, size_t count) {
    for (size_t i = (size_t)blockIdx.x * T + threadIdx.x; i < count; i += (size_t)gridDim.x * T) words[i] = 0u;
}

// ---- 1. histogram of one level's bits, of the kept keys under the prefix found so far ---------------------------------------------------------
// A lane gathers runs of one bin in a register before it touches LDS: neighbouring classes of a row mostly share their leading bits, and
// same-address LDS atomics of a wave are served one after another.
template <int LAYOUT, int LEVEL>
__global__ __launch_bounds__(T) void topk_hist_kernel(const TopkArgs a, const TopkWs ws) {
    constexpr int SHIFT = plan::LevelShift(LEVEL), NB = 1 << plan::LevelBits(LEVEL);
    __shared__ unsigned h[NB];
    __shared__ float stage[LAYOUT == plan::kRows ? T * PITCH : 1];
    const int b = blockIdx.y, r0 = plan::kChunkRows * (int)blockIdx.x;
    const int nrows = min(plan::kChunkRows, a.rows - r0);
    const unsigned* st = ws.state + (size_t)b * plan::kStateWords;
    unsigned prefix = 0;
    if constexpr (LEVEL > 0) {
        if (st[plan::kTake] == 0u) return;    // nothing to store: workgroup-uniform
        prefix = st[plan::kPrefix] >> (SHIFT + plan::LevelBits(LEVEL));
    }
    for (int i = threadIdx.x; i < NB; i += T) h[i] = 0u;
    __syncthreads();
    unsigned run_bin = 0u, run = 0u;
    topk_candidates<LAYOUT>(a, a.pred + (size_t)b * (size_t)a.image_ld, r0, nrows, stage, [&](int, unsigned key) {
        if constexpr (LEVEL > 0) {
            if ((key >> (SHIFT + plan::LevelBits(LEVEL))) != prefix) return;
        }
        const unsigned bin = (key >> SHIFT) & (unsigned)(NB - 1);
        if (bin != run_bin && run != 0u) {
            atomicAdd(&h[run_bin], run);
            run = 0u;
        }
        run_bin = bin;
        ++run;
    });
    if (run != 0u) atomicAdd(&h[run_bin], run);
    __syncthreads();
    unsigned* gh = ws.hist + ((size_t)b * plan::kLevels + LEVEL) * plan::kBins;
    for (int i = threadIdx.x; i < NB; i += T) {
        const unsigned v = h[i];
        if (v != 0u) atomicAdd(&gh[i], v);    // integer adds commute: the totals do not depend on the order
    }
}

// ---- 2. the bin in which the count from the top reaches what is still wanted -----------------------------------------------------------------
template <int LEVEL>
__global__ __launch_bounds__(T) void topk_select_kernel(const TopkWs ws, int max_det) {
    constexpr int SHIFT = plan::LevelShift(LEVEL), NB = 1 << plan::LevelBits(LEVEL), PER = NB / T;
    __shared__ unsigned part[T];
    const int b = blockIdx.x, t = threadIdx.x;
    unsigned* st = ws.state + (size_t)b * plan::kStateWords;
    const unsigned* gh = ws.hist + ((size_t)b * plan::kLevels + LEVEL) * plan::kBins;
    unsigned take = 0u, prefix = 0u, above = 0u;
    if constexpr (LEVEL > 0) {
        take = st[plan::kTake];
        prefix = st[plan::kPrefix];
        above = st[plan::kAbove];
        if (take == 0u) return;
    }
    unsigned v[PER], sum = 0u;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        v[j] = gh[t * PER + j];
        sum += v[j];
    }
    part[t] = sum;
    __syncthreads();
    for (int off = 1; off < T; off <<= 1) {     // inclusive suffix scan: part[t] = the counts of threads t .. T - 1
        const unsigned x = t + off < T ? part[t + off] : 0u;
        __syncthreads();
        part[t] += x;
        __syncthreads();
    }
    if constexpr (LEVEL == 0) {
        const unsigned total = part[0];
        take = total < (unsigned)max_det ? total : (unsigned)max_det;
        if (t == 0) {
            st[plan::kTotal] = total;
            st[plan::kTake] = take;
        }
        if (take == 0u) return;     // kPrefix and kAbove are read by nobody then
    }
    const unsigned want = take - above;         // >= 1, and at most the keys under the prefix
    unsigned cum = part[t] - sum;               // keys in the bins of the threads above this one
#pragma unroll
    for (int j = PER - 1; j >= 0; --j) {
        if (cum < want && cum + v[j] >= want) {     // exactly one bin of one thread
            st[plan::kPrefix] = prefix | ((unsigned)(t * PER + j) << SHIFT);
            st[plan::kAbove] = above + cum;
        }
        cum += v[j];
    }
}

// ---- 3. keys above T, and the count of keys equal to T in this chunk -------------------------------------------------------------------------
template <int LAYOUT>
__global__ __launch_bounds__(T) void topk_collect_kernel(const TopkArgs a, const TopkWs ws, int chunks) {
    __shared__ float stage[LAYOUT == plan::kRows ? T * PITCH : 1];
    __shared__ unsigned equal;
    const int b = blockIdx.y, r0 = plan::kChunkRows * (int)blockIdx.x;
    const int nrows = min(plan::kChunkRows, a.rows - r0);
    const unsigned* st = ws.state + (size_t)b * plan::kStateWords;
    if (st[plan::kTake] == 0u) return;
    const unsigned tkey = st[plan::kPrefix];
    if (threadIdx.x == 0) equal = 0u;
    __syncthreads();
    unsigned long long* keys = ws.keys + (size_t)b * (size_t)a.max_det;
    const int row = r0 + (int)threadIdx.x;
    unsigned eq = 0u;
    topk_candidates<LAYOUT>(a, a.pred + (size_t)b * (size_t)a.image_ld, r0, nrows, stage, [&](int c, unsigned key) {
        if (key > tkey) {
            const unsigned slot = atomicAdd(&ws.slot[b], 1u);      // fewer than take such keys exist
            if (slot < (unsigned)a.max_det) keys[slot] = topk_sort_key(key, topk_flat(a, row, c));
        } else if (key == tkey) {
            ++eq;
        }
    });
    if (eq != 0u) atomicAdd(&equal, eq);
    __syncthreads();
    if (threadIdx.x == 0) ws.ties[(size_t)b * chunks + blockIdx.x] = equal;
}

// exclusive prefix of v over the workgroup's threads in thread order: shuffles inside a wave, the wave totals through LDS
__device__ __forceinline__ unsigned topk_block_exclusive_scan(unsigned v, unsigned* wave_sum /* [T / 64] */) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned up = __shfl_up(inc, o);
        if (lane >= o) inc += up;
    }
    if (lane == 63) wave_sum[wave] = inc;
    __syncthreads();
    unsigned before = 0u;
    for (int w = 0; w < wave; ++w) before += wave_sum[w];
    return before + inc - v;
}

// ---- 4. the `need` lowest flat indices among the keys equal to T ------------------------------------------------------------------------------
// rank of an equal key = equal keys in the chunks before this one + in the rows of this chunk before its own + in its row before its class.
// The first sum is taken by every workgroup for itself over at most `chunk` words; a chunk without equal keys, or whose first rank is
// already `need` or more, returns before it reads a score.
template <int LAYOUT>
__global__ __launch_bounds__(T) void topk_collect_ties_kernel(const TopkArgs a, const TopkWs ws, int chunks) {
    __shared__ float stage[LAYOUT == plan::kRows ? T * PITCH : 1];
    __shared__ unsigned before_chunk;
    __shared__ unsigned wave_sum[T / 64];
    const int b = blockIdx.y, chunk = blockIdx.x, r0 = plan::kChunkRows * chunk;
    const int nrows = min(plan::kChunkRows, a.rows - r0);
    const unsigned* st = ws.state + (size_t)b * plan::kStateWords;
    const unsigned take = st[plan::kTake];
    if (take == 0u) return;
    const unsigned tkey = st[plan::kPrefix], gt = st[plan::kAbove], need = take - gt;
    const unsigned* ties = ws.ties + (size_t)b * chunks;
    if (ties[chunk] == 0u) return;
    if (threadIdx.x == 0) before_chunk = 0u;
    __syncthreads();
    unsigned part = 0u;
    for (int i = threadIdx.x; i < chunk; i += T) part += ties[i];
    if (part != 0u) atomicAdd(&before_chunk, part);
    __syncthreads();
    const unsigned base = before_chunk;
    if (base >= need) return;
    const float* img = a.pred + (size_t)b * (size_t)a.image_ld;
    unsigned eq = 0u;
    topk_candidates<LAYOUT>(a, img, r0, nrows, stage, [&](int, unsigned key) { eq += key == tkey ? 1u : 0u; });
    unsigned rank = base + topk_block_exclusive_scan(eq, wave_sum);
    unsigned long long* keys = ws.keys + (size_t)b * (size_t)a.max_det;
    const int row = r0 + (int)threadIdx.x;
    topk_candidates<LAYOUT>(a, img, r0, nrows, stage, [&](int c, unsigned key) {
        if (key != tkey) return;
        if (rank < need && gt + rank < (unsigned)a.max_det) keys[gt + rank] = topk_sort_key(key, topk_flat(a, row, c));
        ++rank;
    });
}

// ---- 5. sort the stored keys, write every output ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(T) void topk_sort_write_kernel(const TopkArgs a, const TopkWs ws, int layout, const float* __restrict__ adjust,
                                                            float* __restrict__ dets, int* __restrict__ counts, int* __restrict__ src_rows,
                                                            float* __restrict__ net_boxes, unsigned* __restrict__ extras) {
    __shared__ unsigned long long k[plan::kMaxDet];
    __shared__ int row_of[plan::kMaxDet];
    const int b = blockIdx.x, t = threadIdx.x;
    const unsigned* st = ws.state + (size_t)b * plan::kStateWords;
    if (t == 0) counts[b] = (int)st[plan::kTotal];
    const int take = min((int)st[plan::kTake], plan::kMaxDet);
    if (take == 0) return;
    int P = 1;
    while (P < take) P <<= 1;
    const unsigned long long* keys = ws.keys + (size_t)b * (size_t)a.max_det;
    for (int i = t; i < P; i += T) k[i] = i < take ? keys[i] : 0ull;      // no stored key is 0: its high word would be a NaN's
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1) {
        for (int j = size >> 1; j > 0; j >>= 1) {
            for (int i = t; i < P; i += T) {
                const int o = i ^ j;
                if (o > i) {
                    const unsigned long long x = k[i], y = k[o];
                    const bool down = (i & size) == 0;
                    if (down ? x < y : x > y) {
                        k[i] = y;
                        k[o] = x;
                    }
                }
            }
            __syncthreads();
        }
    }
    const float* img = a.pred + (size_t)b * (size_t)a.image_ld;
    const size_t ld = (size_t)a.ld;
    auto at = [&](int row, int e) { return layout == plan::kRows ? img[(size_t)row * ld + e] : img[(size_t)e * ld + row]; };
    const si_post::PostAdjust adj = si_post::post_adjust(adjust, b);
    for (int d = t; d < take; d += T) {
        const unsigned flat = 0xffffffffu - (unsigned)(k[d] & 0xffffffffull);
        const int row = (int)(a.multi_label ? flat / (unsigned)a.classes : flat);
        if ((unsigned)row >= (unsigned)a.rows) {    // cannot happen with the keys the collect kernels store; never follow one that is not theirs
            row_of[d] = 0;
            continue;
        }
        int label;
        float confidence;
        if (a.multi_label) {
            label = (int)(flat - (unsigned)row * (unsigned)a.classes);
            confidence = at(row, 4 + label);
        } else {
            label = -1;
            confidence = -3.402823466e+38f;  // -FLT_MAX
            for (int c = 0; c < a.classes; ++c) {
                const float s = at(row, 4 + c);
                if (s > confidence) {
                    confidence = s;
                    label = c;
                }
            }
        }
        const float4 box = si_post::post_box(at(row, 0), at(row, 1), at(row, 2), at(row, 3), a.box_format);
        const size_t o = (size_t)b * (size_t)a.max_det + d;
        si_post::post_store_det(dets + o * 6, box, adj, confidence, (float)label);
        if (src_rows) src_rows[o] = row;
        if (net_boxes) {
            float* nb = net_boxes + o * 4;
            nb[0] = box.x; nb[1] = box.y; nb[2] = box.z; nb[3] = box.w;
        }
        row_of[d] = row;
    }
    if (!extras || a.extra <= 0) return;
    __syncthreads();
    const unsigned* bits = reinterpret_cast<const unsigned*>(img);
    unsigned* dst = extras + (size_t)b * (size_t)a.max_det * (size_t)a.extra;
    const int first = 4 + a.classes;
    for (size_t i = t; i < (size_t)take * (size_t)a.extra; i += T) {
        const size_t d = i / (size_t)a.extra;
        const size_t e = (size_t)first + (i - d * (size_t)a.extra);
        const size_t row = (size_t)row_of[d];
        dst[i] = layout == plan::kRows ? bits[row * ld + e] : bits[e * ld + row];
    }
}

plan::Shape topk_shape(const SiDetectTopkDesc* d) {
    plan::Shape v;
    v.n = d->n; v.rows = d->rows; v.classes = d->classes; v.extra = d->extra; v.layout = d->layout; v.ld = d->ld; v.image_ld = d->image_ld;
    v.box_format = d->box_format; v.multi_label = d->multi_label; v.max_det = d->max_det;
    return v;
}

template <int LAYOUT>
int topk_launch(const TopkArgs& a, const TopkWs& ws, size_t zero_words, int n, int chunks, const float* adjust, const SiDetectPostOut* out,
                hipStream_t s) {
    const dim3 grid(chunks, n), block(T);
    const unsigned clear_blocks = si_grid_for(zero_words);
    hipLaunchKernelGGL(topk_clear_kernel, dim3(clear_blocks > 1024u ? 1024u : clear_blocks), block, 0, s, ws.hist, zero_words);
    hipLaunchKernelGGL((topk_hist_kernel<LAYOUT, 0>), grid, block, 0, s, a, ws);
    hipLaunchKernelGGL(topk_select_kernel<0>, dim3(n), block, 0, s, ws, a.max_det);
    hipLaunchKernelGGL((topk_hist_kernel<LAYOUT, 1>), grid, block, 0, s, a, ws);
    hipLaunchKernelGGL(topk_select_kernel<1>, dim3(n), block, 0, s, ws, a.max_det);
    hipLaunchKernelGGL((topk_hist_kernel<LAYOUT, 2>), grid, block, 0, s, a, ws);
    hipLaunchKernelGGL(topk_select_kernel<2>, dim3(n), block, 0, s, ws, a.max_det);
    hipLaunchKernelGGL(topk_collect_kernel<LAYOUT>, grid, block, 0, s, a, ws, chunks);
    hipLaunchKernelGGL(topk_collect_ties_kernel<LAYOUT>, grid, block, 0, s, a, ws, chunks);
    hipLaunchKernelGGL(topk_sort_write_kernel, dim3(n), block, 0, s, a, ws, LAYOUT, adjust, out->dets, out->counts, out->src_rows, out->net_boxes,
                       (unsigned*)out->extras);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

size_t si_hip_detect_topk_workspace_bytes(const SiDetectTopkDesc* d) { return d ? plan::WorkspaceBytes(topk_shape(d)) : 0; }

const char* si_hip_detect_topk_kernel_name(const SiDetectTopkDesc* d, const void* pred) {
    if (!d || !pred || (reinterpret_cast<uintptr_t>(pred) & 3) != 0 || plan::StatusOf(topk_shape(d)) != plan::kOk) return "none";
    return d->layout == plan::kRows ? "topk_hist_kernel<SI_DETECT_ROWS>" : "topk_hist_kernel<SI_DETECT_CHANNELS>";
}

int si_hip_detect_topk_postprocess_f32(const SiDetectTopkDesc* d, const float* pred, const float* adjust, const SiDetectPostOut* out,
                                       void* workspace, size_t workspace_bytes, si_stream_t stream) {
    if (!d || !pred || !out || !out->counts || !workspace) return SI_E_BADARG;
    if ((reinterpret_cast<uintptr_t>(pred) & 3) != 0) return SI_E_BADARG;
    const plan::Shape v = topk_shape(d);
    const int rc = plan::StatusOf(v);
    if (rc != plan::kOk) return rc == plan::kBadArg ? SI_E_BADARG : SI_E_UNSUPPORTED;
    if (d->max_det > 0 && !out->dets) return SI_E_BADARG;
    const plan::Workspace w = plan::LayoutOf(d->n, d->rows, d->max_det);
    if (workspace_bytes < w.total) return SI_E_BADARG;
    char* base = (char*)workspace;
    const TopkWs ws{(unsigned long long*)(base + w.offset[plan::kKeys]), (unsigned*)(base + w.offset[plan::kHist]),
                    (unsigned*)(base + w.offset[plan::kSlot]), (unsigned*)(base + w.offset[plan::kStateRegion]),
                    (unsigned*)(base + w.offset[plan::kTies])};
    const TopkArgs a{pred, d->image_ld, d->rows, d->ld, d->classes, d->extra, d->box_format, d->multi_label, d->max_det, d->prob_threshold};
    const int chunks = plan::Chunks(d->rows);
    return d->layout == plan::kRows ? topk_launch<plan::kRows>(a, ws, w.zero_words, d->n, chunks, adjust, out, (hipStream_t)stream)
                                    : topk_launch<plan::kChannels>(a, ws, w.zero_words, d->n, chunks, adjust, out, (hipStream_t)stream);
}

}  // extern "C"
