// detect_post.h -- what the translation units of the detection post-processing share (not part of the C-ABI): the bound workspace, the
// filter's arguments, and the two launch sequences every entry goes through -- clear + filter + sort in front, the payload gather behind.
// postprocess.hip defines them (the kernels live there); detect_obb.hip runs its own suppression between the two.  The box and un-letterbox
// arithmetic of an output row is stated here once, for postprocess.hip and detect_topk.hip.
#ifndef SI_DETECT_POST_H_
#define SI_DETECT_POST_H_

#include <hip/hip_runtime.h>

#include "detect_plan.h"

namespace si_post {

namespace plan = si_detect_plan;

// The regions, their order and their sizes: detect_plan.h (Layout).  srow / drow exist in the general entry's layout alone and are
// null for si_hip_yolo_postprocess_f32, whose byte count is what it always was.
struct PostWs {
    int* count;
    int* bin_count;
    int* keep;
    int nbins;
    size_t zero_bytes;
    float4* gbox;
    int* grank;
    unsigned long long* key;
    float4* box;
    int* label;
    float4* sbox;
    int* slabel;
    float* sprob;
    float4* pbox;
    int* plabel;
    float* parea;
    int* srow;   // prediction row of each candidate in the confidence order
    int* drow;   // prediction row of each stored detection: what the payload gather reads
};

inline size_t post_ws_bind(int n, int cap, int nbins, bool general, char* base, PostWs* ws) {
    const plan::Workspace w = plan::Layout(n, cap, nbins, general);
    auto at = [&](int r) { return w.bytes[r] ? base + w.offset[r] : nullptr; };
    ws->count = (int*)at(plan::kCount);
    ws->bin_count = (int*)at(plan::kBinCount);
    ws->keep = (int*)at(plan::kKeep);
    ws->nbins = nbins;
    ws->zero_bytes = w.zero_bytes;
    ws->gbox = (float4*)at(plan::kGbox);
    ws->grank = (int*)at(plan::kGrank);
    ws->key = (unsigned long long*)at(plan::kKey);
    ws->box = (float4*)at(plan::kBox);
    ws->label = (int*)at(plan::kLabel);
    ws->sbox = (float4*)at(plan::kSbox);
    ws->slabel = (int*)at(plan::kSlabel);
    ws->sprob = (float*)at(plan::kSprob);
    ws->pbox = (float4*)at(plan::kPbox);
    ws->plabel = (int*)at(plan::kPlabel);
    ws->parea = (float*)at(plan::kParea);
    ws->srow = (int*)at(plan::kSrow);
    ws->drow = (int*)at(plan::kDrow);
    return w.total;
}

struct FilterArgs {
    const float* pred;
    long long image_ld;
    int rows, ld;
    int classes, objectness, box_format;
    float prob_threshold;
};

// ---- the box arithmetic every entry shares (postprocess.hip, detect_topk.hip) ------------------------------------------------------------------
// Results are held to the reference bit for bit, so contraction is off inside each function, whatever the including file says.

// a row's four raw box elements -> {x0, y0, w, h} in network coordinates
__device__ __forceinline__ float4 post_box(float r0, float r1, float r2, float r3, int box_format) {
#pragma clang fp contract(off)
    float x0, y0, x1, y1;
    if (box_format == plan::kCxCyWh) {
        x0 = r0 - r2 * 0.5f; y0 = r1 - r3 * 0.5f;
        x1 = r0 + r2 * 0.5f; y1 = r1 + r3 * 0.5f;
    } else {
        x0 = r0; y0 = r1; x1 = r2; y1 = r3;
    }
    return make_float4(x0, y0, x1 - x0, y1 - y0);
}

// the reference's clip, (std::max)(lower, (std::min)(n, upper)) (test_yolo.cpp:188-191), spelled out: std::min(a, b) is `b < a ? b : a`,
// std::max(a, b) is `a < b ? b : a`, each its FIRST argument when the compare is false.  So a NaN coordinate clips to lo (fmaxf / fminf
// sent it to hi) and -0.0 to +0.0 (geometry with adjust holds both).
__device__ __forceinline__ float clipf(float v, float lo, float hi) {
    const float m = hi < v ? hi : v;
    return lo < m ? m : lo;
}

// image b's row of `adjust` ({pad_l, pad_t, scale, width, height}); on == false without one
struct PostAdjust {
    bool on;
    float pad_l, pad_t, scale, xmax, ymax;
};
__device__ __forceinline__ PostAdjust post_adjust(const float* __restrict__ adjust, int b) {
#pragma clang fp contract(off)
    PostAdjust a{adjust != nullptr, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f};
    if (a.on) {
        a.pad_l = adjust[b * 5 + 0];
        a.pad_t = adjust[b * 5 + 1];
        a.scale = adjust[b * 5 + 2];
        a.xmax = adjust[b * 5 + 3] - 1.0f;
        a.ymax = adjust[b * 5 + 4] - 1.0f;
    }
    return a;
}

// one output row {x, y, w, h, confidence, label}: the network box un-letterboxed and clipped when there is an `adjust`
__device__ __forceinline__ void post_store_det(float* __restrict__ d, const float4 box, const PostAdjust& a, float prob, float label) {
#pragma clang fp contract(off)
    float x0 = box.x, y0 = box.y, x1 = box.x + box.z, y1 = box.y + box.w;
    if (a.on) {
        x0 = clipf((x0 - a.pad_l) / a.scale, 0.0f, a.xmax);
        y0 = clipf((y0 - a.pad_t) / a.scale, 0.0f, a.ymax);
        x1 = clipf((x1 - a.pad_l) / a.scale, 0.0f, a.xmax);
        y1 = clipf((y1 - a.pad_t) / a.scale, 0.0f, a.ymax);
    }
    d[0] = x0; d[1] = y0;
    d[2] = a.on ? x1 - x0 : box.z;
    d[3] = a.on ? y1 - y0 : box.w;
    d[4] = prob;
    d[5] = label;
}

// clear the counters, filter (the layout's kernel), rank sort: afterwards ws.count[b] candidates of image b stand in the confidence order in
// sbox / slabel / sprob / srow
__attribute__((visibility("hidden"))) int front_launch(const FilterArgs& filter, int n, int layout, const PostWs& ws, hipStream_t s);

// extras[b][d][k] = element (first + k) of prediction row drow[b][d], for d < min(counts[b], max_det); behind the kernel that wrote both
__attribute__((visibility("hidden"))) int gather_launch(const FilterArgs& filter, int n, int layout, int first, int extra, const int* counts,
                                                        int max_det, const int* drow, float* extras, hipStream_t s);

}  // namespace si_post

#endif  // SI_DETECT_POST_H_
