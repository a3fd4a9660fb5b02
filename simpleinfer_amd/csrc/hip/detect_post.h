// detect_post.h -- what the translation units of the detection post-processing share (not part of the C-ABI): the bound workspace, the
// filter's arguments, and the two launch sequences every entry goes through -- clear + filter + sort in front, the payload gather behind.
// postprocess.hip defines them (the kernels live there); detect_obb.hip runs its own suppression between the two.
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

// clear the counters, filter (the layout's kernel), rank sort: afterwards ws.count[b] candidates of image b stand in the confidence order in
// sbox / slabel / sprob / srow
__attribute__((visibility("hidden"))) int front_launch(const FilterArgs& filter, int n, int layout, const PostWs& ws, hipStream_t s);

// extras[b][d][k] = element (first + k) of prediction row drow[b][d], for d < min(counts[b], max_det); behind the kernel that wrote both
__attribute__((visibility("hidden"))) int gather_launch(const FilterArgs& filter, int n, int layout, int first, int extra, const int* counts,
                                                        int max_det, const int* drow, float* extras, hipStream_t s);

}  // namespace si_post

#endif  // SI_DETECT_POST_H_
