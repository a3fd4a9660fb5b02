// detect_obb.hip -- oriented-box post-processing (include/si_obb.h): behind the filter and the rank sort of postprocess.hip (the same kernels,
// launched through detect_post.h), rotated NMS by ProbIoU in its matrix form -- a candidate goes when ANY earlier candidate of its label
// overlaps it, dropped or not -- and the compaction into 7-wide rows.
//
// The matrix form has no dependency chain, so the suppression is a triangular all-pairs pass spread over the whole chip: one lane owns
// candidate i and keeps its record in registers, the records of the earlier candidates come by in LDS tiles that the workgroup stages with
// coalesced 16-byte loads, and every lane of a wave reads the same record at the same time (an LDS broadcast: no bank conflicts).  Everything
// that belongs to one box alone (the covariance terms, the clamped determinant) is computed once per candidate by the record kernel; the
// threshold is moved onto the Bhattacharyya distance, so a pair costs one reciprocal pair, one square root and one logarithm and no exp.
//
// The pair arithmetic is the header's, operation by operation: contraction is off.
#include "si_obb.h"
#include "si_hip_internal.h"
#include "detect_post.h"
#include "obb_plan.h"

#pragma clang fp contract(off)

namespace {

namespace oplan = si_obb_plan;
namespace plan = si_detect_plan;
using si_post::PostWs;

constexpr int OBB_T = oplan::kThreads;
constexpr int OBB_TILE = oplan::kTile;
constexpr float OBB_EPS = 1e-7f;

struct ObbWs {
    float4* rec;    // [n][rows][2]: {cx, cy, A, B}, {C, det, label bits, 0}
    float4* raw;    // [n][rows]: {w, h, angle, confidence}
    int* keep;      // [n][rows]
};

struct ObbSrc {
    const float* pred;
    long long image_ld;
    int rows, ld, layout;
    int angle_e;    // element index of the angle inside a row
};

// ---- 1. records ------------------------------------------------------------------------------------------------------------------------------
// One lane per sorted candidate: the five raw elements of its prediction row (found through srow; both layouts read in place, nothing between
// rows is touched), the covariance terms of the box, and the raw size / angle / confidence for the store.
__global__ __launch_bounds__(OBB_T) void obb_record_kernel(ObbSrc a, PostWs ws, ObbWs ow) {
    const int b = blockIdx.y;
    const int count = ws.count[b];
    const int i = blockIdx.x * OBB_T + threadIdx.x;
    if (i >= count) return;
    const size_t at = (size_t)b * a.rows + i;
    const size_t row = (size_t)ws.srow[at];
    const size_t es = a.layout == plan::kRows ? 1 : (size_t)a.ld;     // element stride, row stride
    const size_t rs = a.layout == plan::kRows ? (size_t)a.ld : 1;
    const float* p = a.pred + (size_t)b * (size_t)a.image_ld + row * rs;
    const float cx = p[0], cy = p[es], w = p[2 * es], h = p[3 * es], angle = p[(size_t)a.angle_e * es];
    const float va = w * w / 12.0f, vb = h * h / 12.0f;
    const float c = cosf(angle), s = sinf(angle);
    const float c2 = c * c, s2 = s * s;
    const float A = va * c2 + vb * s2;
    const float B = va * s2 + vb * c2;
    const float C = ((va - vb) * c) * s;
    float det = A * B - C * C;
    det = det < 0.0f ? 0.0f : det;       // clamp_(0): a NaN stays
    ow.rec[2 * at] = make_float4(cx, cy, A, B);
    ow.rec[2 * at + 1] = make_float4(C, det, __int_as_float(ws.slabel[at]), 0.0f);
    ow.raw[at] = make_float4(w, h, angle, ws.sprob[at]);
}

// ---- 2. triangular suppression -----------------------------------------------------------------------------------------------------------------
// grid (ceil(rows / 256), n); a workgroup beyond count[b] returns at once, the others visit only the tiles that start before their last
// candidate, and a wave only the records before ITS last candidate.  The j loop is wave-uniform; `j < i` and the label test are selects.  A
// wave whose lanes are all dead skips the rest of a tile (checked every 32 records); the barriers stay workgroup-uniform.
__global__ __launch_bounds__(OBB_T) void obb_suppress_kernel(int rows, float bd_max, int agnostic, PostWs ws, ObbWs ow) {
    __shared__ float4 tile[2 * OBB_TILE];
    const int b = blockIdx.y;
    const int count = ws.count[b];
    const int i0 = blockIdx.x * OBB_T;
    if (i0 >= count) return;
    const size_t base = (size_t)b * rows;
    const int i = i0 + (int)threadIdx.x;
    const bool valid = i < count;
    const int iend = min(count, i0 + OBB_T);                                         // one past this workgroup's last candidate
    const int wlast = min(iend - 1, i0 + (int)(threadIdx.x | 63));                   // this wave's last candidate (wave-uniform)
    float4 m0 = make_float4(0.f, 0.f, 0.f, 0.f), m1 = m0;
    if (valid) {
        m0 = ow.rec[2 * (base + i)];
        m1 = ow.rec[2 * (base + i) + 1];
    }
    const float x2 = m0.x, y2 = m0.y, A2 = m0.z, B2 = m0.w, C2 = m1.x, det2 = m1.y;
    const int lab2 = __float_as_int(m1.z);
    bool dead = !valid;
    const float4* src = ow.rec + 2 * base;
    for (int t0 = 0; t0 < iend - 1; t0 += OBB_TILE) {
        const int tn = min(OBB_TILE, iend - 1 - t0);                                 // records j < iend - 1 are all anyone here needs
        __syncthreads();
        for (int k = threadIdx.x; k < 2 * tn; k += OBB_T) tile[k] = src[2 * (size_t)t0 + k];
        __syncthreads();
        const int jn = min(tn, wlast - t0);
        for (int j0 = 0; j0 < jn; j0 += 32) {
            if (__builtin_amdgcn_ballot_w64(!dead) == 0ull) break;                   // wave-uniform
            const int je = min(j0 + 32, jn);
#pragma unroll 4
            for (int j = j0; j < je; ++j) {
                const float4 r0 = tile[2 * j], r1 = tile[2 * j + 1];
                const float x1 = r0.x, y1 = r0.y;
                const float sA = r0.z + A2, sB = r0.w + B2, sC = r1.x + C2;
                const float D = sA * sB - sC * sC;
                const float dx = x1 - x2, dy = y1 - y2;
                const float r = __builtin_amdgcn_rcpf(D + OBB_EPS);
                const float t12 = (0.25f * (sA * (dy * dy) + sB * (dx * dx)) + 0.5f * ((sC * (x2 - x1)) * dy)) * r;
                const float q = D * __builtin_amdgcn_rcpf(4.0f * __builtin_amdgcn_sqrtf(r1.y * det2) + OBB_EPS) + OBB_EPS;
                const float t3 = 0.5f * (__builtin_amdgcn_logf(q) * 0.693147180559945f);
                float bd = t12 + t3;
                bd = bd < OBB_EPS ? OBB_EPS : bd;                                    // the lower clamp; a NaN stays
                const bool hit = !(bd > bd_max);
                const bool mine = (t0 + j < i) & ((agnostic != 0) | (__float_as_int(r1.z) == lab2));
                dead |= hit & mine;
            }
        }
    }
    if (valid) ow.keep[base + i] = dead ? 0 : 1;
}

// ---- 3. compaction -----------------------------------------------------------------------------------------------------------------------------
// keep flags (by confidence rank) -> dense 7-wide rows in the confidence order, counts, src_rows, and drow for the payload gather.  One
// workgroup per image; ballot + prefix over the four waves, as yolo_compact_kernel.
__global__ __launch_bounds__(256) void obb_compact_kernel(int rows, const float* __restrict__ adjust, float* __restrict__ obbs,
                                                          int* __restrict__ counts, int* __restrict__ src_rows, int* __restrict__ drow, int max_det,
                                                          PostWs ws, ObbWs ow) {
    __shared__ int wsum[4];
    const int b = blockIdx.x;
    const int count = ws.count[b];
    const size_t base = (size_t)b * rows;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const bool adj = adjust != nullptr;
    float pad_l = 0.0f, pad_t = 0.0f, scale = 1.0f;
    if (adj) {
        pad_l = adjust[b * 5 + 0];
        pad_t = adjust[b * 5 + 1];
        scale = adjust[b * 5 + 2];
    }
    int total = 0;
    for (int g0 = 0; g0 < count; g0 += 256) {
        const int g = g0 + threadIdx.x;
        const bool f = g < count && ow.keep[base + g] != 0;
        const unsigned long long m = __ballot(f);
        __syncthreads();
        if (lane == 0) wsum[wave] = __popcll(m);
        __syncthreads();
        int pos = total + __popcll(m & ((1ull << lane) - 1ull));
        for (int w = 0; w < wave; ++w) pos += wsum[w];
        total += wsum[0] + wsum[1] + wsum[2] + wsum[3];
        if (f && pos < max_det) {
            const float4 r0 = ow.rec[2 * (base + g)];
            const float4 raw = ow.raw[base + g];
            float cx = r0.x, cy = r0.y, w = raw.x, h = raw.y;
            if (adj) {
                cx = (cx - pad_l) / scale;
                cy = (cy - pad_t) / scale;
                w = w / scale;
                h = h / scale;
            }
            float* d = obbs + ((size_t)b * max_det + pos) * 7;
            d[0] = cx; d[1] = cy; d[2] = w; d[3] = h;
            d[4] = raw.z;
            d[5] = raw.w;
            d[6] = (float)ws.slabel[base + g];
            if (src_rows || drow) {
                const int row = ws.srow[base + g];
                if (drow) drow[base + pos] = row;
                if (src_rows) src_rows[(size_t)b * max_det + pos] = row;
            }
        }
    }
    if (threadIdx.x == 0) counts[b] = total;
}

oplan::Shape obb_shape(const SiDetectObbDesc* d) {
    oplan::Shape v;
    v.post.n = d->n; v.post.rows = d->rows; v.post.classes = d->classes; v.post.objectness = d->objectness; v.post.extra = d->extra;
    v.post.layout = d->layout; v.post.ld = d->ld; v.post.image_ld = d->image_ld; v.post.box_format = plan::kCxCyWh; v.post.agnostic = d->agnostic;
    v.post.max_det = d->max_det;
    v.angle_off = d->angle_off;
    v.nms_threshold = d->nms_threshold;
    return v;
}

}  // namespace

extern "C" {

size_t si_hip_detect_obb_postprocess_workspace_bytes(const SiDetectObbDesc* d) { return d ? oplan::WorkspaceBytes(obb_shape(d)) : 0; }

int si_hip_detect_obb_postprocess_f32(const SiDetectObbDesc* d, const float* pred, const float* adjust, const SiDetectObbOut* out, void* workspace,
                                      size_t workspace_bytes, si_stream_t stream) {
    if (!d || !pred || !out || !out->counts || !workspace) return SI_E_BADARG;
    if ((reinterpret_cast<uintptr_t>(pred) & 3) != 0) return SI_E_BADARG;
    const oplan::Shape v = obb_shape(d);
    const int rc = oplan::StatusOf(v);
    if (rc != plan::kOk) return rc == plan::kBadArg ? SI_E_BADARG : SI_E_UNSUPPORTED;
    if (d->max_det > 0 && !out->obbs) return SI_E_BADARG;
    const int nbins = (int)plan::Bins(v.post);
    const oplan::Workspace w = oplan::Layout(d->n, d->rows, nbins);
    if (workspace_bytes < w.total) return SI_E_BADARG;
    char* base = (char*)workspace;
    PostWs ws;
    post_ws_bind(d->n, d->rows, nbins, true, base, &ws);
    ObbWs ow{(float4*)(base + w.offset[oplan::kRecord]), (float4*)(base + w.offset[oplan::kRaw]), (int*)(base + w.offset[oplan::kKeep])};
    hipStream_t s = (hipStream_t)stream;
    const si_post::FilterArgs filter{pred, d->image_ld, d->rows, d->ld, d->classes, d->objectness, plan::kCxCyWh, d->prob_threshold};
    const int fr = si_post::front_launch(filter, d->n, d->layout, ws, s);
    if (fr != 0) return fr;
    // iou >= thr  <=>  bd <= -log(1 + eps - (1 - thr)^2): formed once, in double
    const double one_minus = 1.0 - (double)d->nms_threshold;
    const float bd_max = (float)-log(1.0 + 1e-7 - one_minus * one_minus);
    const dim3 grid((d->rows + OBB_T - 1) / OBB_T, d->n);
    const ObbSrc src{pred, d->image_ld, d->rows, d->ld, d->layout, (int)oplan::AngleElement(v)};
    hipLaunchKernelGGL(obb_record_kernel, grid, dim3(OBB_T), 0, s, src, ws, ow);
    hipLaunchKernelGGL(obb_suppress_kernel, grid, dim3(OBB_T), 0, s, d->rows, bd_max, d->agnostic, ws, ow);
    const bool gather = out->extras && d->max_det > 0;
    hipLaunchKernelGGL(obb_compact_kernel, dim3(d->n), dim3(256), 0, s, d->rows, adjust, out->obbs, out->counts, out->src_rows,
                       gather ? ws.drow : nullptr, d->max_det, ws, ow);
    if (gather)
        return si_post::gather_launch(filter, d->n, d->layout, (int)plan::Scan(v.post), d->extra, out->counts, d->max_det, ws.drow, out->extras, s);
    return (int)hipGetLastError();
}

}  // extern "C"
