// si_reduce_plan.h -- the host side that the reduction files (softmax.hip, reduce.hip, lpnorm.hip) share: the axis mask, its fold into
// levels, the output pixel count under a mask, the lanes-per-row rule, the front half of a descriptor check and the spelling of a kernel's
// four instantiations.  Pure: plain C++, so the rules are exercised without a device (tests/cpp/test_reduce_plan.cpp).  A kernel file
// defines none of these for itself ("Device commons").
#ifndef SI_REDUCE_PLAN_H_
#define SI_REDUCE_PLAN_H_

#include <cstdint>

#include "si_views.h"

// the NHWC axis mask of a reduction: SI_REDUCE_AXIS_* of include/si_reduce.h, which include/si_lpnorm.h shares (reduce.hip asserts it)
constexpr int SI_AXIS_N = 1, SI_AXIS_H = 2, SI_AXIS_W = 4, SI_AXIS_C = 8;
constexpr int SI_AXIS_SPATIAL = SI_AXIS_N | SI_AXIS_H | SI_AXIS_W;

// the two refusals of a descriptor check: SI_E_BADARG and SI_E_UNSUPPORTED of the C-ABI (si_hip_internal.h asserts it)
constexpr int SI_PLAN_BADARG = -1, SI_PLAN_UNSUPPORTED = -2;

// The three spatial axes folded into at most two KEPT and two REDUCED levels of (count, pixel stride), outer first: neighbouring axes of
// one kind merge (h and w reduced are one run of h * w pixels), extents of 1 drop out, an unused level is (1, 0).  Kept pixel kp starts at
// input pixel (kp / kept[1][0]) * kept[0][1] + (kp % kept[1][0]) * kept[1][1]; position r lies (r / red[1][0]) * red[0][1] +
// (r % red[1][0]) * red[1][1] pixels further: kept pixels and positions both count in increasing (n, h, w).
struct SiLevels {
    int kept[2][2] = {{1, 0}, {1, 0}};
    int red[2][2] = {{1, 0}, {1, 0}};
    uint64_t positions = 1;   // the product of the reduced extents
};

static inline SiLevels si_fold_levels(int n, int h, int w, int axes) {
    SiLevels lv;
    const int ext[3] = {n, h, w};
    const int stride[3] = {h * w, w, 1};
    int nk = 0, nr = 0;
    int kept[3][2], red[3][2];
    for (int a = 0; a < 3; ++a) {
        const bool reduced = (axes >> a) & 1;
        if (reduced) lv.positions *= (uint64_t)ext[a];
        if (ext[a] == 1) continue;
        int(*list)[2] = reduced ? red : kept;
        int& cnt = reduced ? nr : nk;
        if (cnt > 0 && list[cnt - 1][1] == ext[a] * stride[a]) {   // the level above is a run of this one
            list[cnt - 1][0] *= ext[a];
            list[cnt - 1][1] = stride[a];
        } else {
            list[cnt][0] = ext[a];
            list[cnt][1] = stride[a];
            ++cnt;
        }
    }
    // (three levels of one kind would need the other kind between each pair: there are three axes, so at most two)
    for (int i = 0; i < nk; ++i) { lv.kept[2 - nk + i][0] = kept[i][0]; lv.kept[2 - nk + i][1] = kept[i][1]; }
    for (int i = 0; i < nr; ++i) { lv.red[2 - nr + i][0] = red[i][0]; lv.red[2 - nr + i][1] = red[i][1]; }
    return lv;
}

// the levels as a kernel's argument struct carries them (RdArgs, LnArgs embed this); the default is the fold of no axis
struct SiLevelArgs {
    int K1 = 1, ks0 = 0, ks1 = 0;          // kept pixel kp starts at input pixel (kp / K1) * ks0 + (kp % K1) * ks1
    int R = 1, R1 = 1, rs0 = 0, rs1 = 0;   // position r is (r / R1) * rs0 + (r % R1) * rs1 pixels further
};

static inline SiLevelArgs si_level_args(const SiLevels& lv) {
    SiLevelArgs a;
    a.K1 = lv.kept[1][0];
    a.ks0 = lv.kept[0][1];
    a.ks1 = lv.kept[1][1];
    a.R = (int)lv.positions;
    a.R1 = lv.red[1][0];
    a.rs0 = lv.red[0][1];
    a.rs1 = lv.red[1][1];
    return a;
}

// pixels of the output under a mask: the product of the kept spatial extents
static inline uint64_t si_masked_pixels(int n, int h, int w, int axes) {
    return (uint64_t)((axes & SI_AXIS_N) ? 1 : n) * (uint64_t)((axes & SI_AXIS_H) ? 1 : h) * (uint64_t)((axes & SI_AXIS_W) ? 1 : w);
}

// log2 of the lanes per row of a group form: the power of two at or above cv / per, at most 64
static inline int si_group_lg(int cv, int per) {
    int lg = 0;
    while ((1 << lg) < 64 && (1 << lg) * per < cv) ++lg;
    return lg;
}

// The front half of a descriptor check: positive extents and strides that hold their channels (SI_PLAN_BADARG), then row, pixel and
// element counts that fit 31-bit offsets on both sides (SI_PLAN_UNSUPPORTED); 0 otherwise.  `opix`, `oc`: the output's pixels and channels.
// What is a file's own (op, p and axis ranges, eps, the mask rules) stays in its check_desc, placed so that each code is found as before.
static inline int si_check_reduce_views(int n, int h, int w, int c, int in_ld, int out_ld, uint64_t opix, int oc) {
    if (n <= 0 || h <= 0 || w <= 0 || c <= 0) return SI_PLAN_BADARG;
    if (in_ld < c || out_ld < oc) return SI_PLAN_BADARG;
    const uint64_t rows = (uint64_t)n * (uint64_t)h;   // < 2^62
    if (rows > SI_INDEX_LIMIT || rows * (uint64_t)w > SI_INDEX_LIMIT) return SI_PLAN_UNSUPPORTED;
    const uint64_t pix = rows * (uint64_t)w;
    // offsets, and with them the grids: at most one workgroup per pixel, at most one lane per element (c <= ld)
    if (pix * (uint64_t)in_ld > SI_INDEX_LIMIT || opix * (uint64_t)out_ld > SI_INDEX_LIMIT) return SI_PLAN_UNSUPPORTED;
    return 0;
}

// The four instantiations of a kernel template <T, VW> as a profile names them, from its stem, and the entry a launch picks.
#define SI_KERNEL_NAMES(stem) {stem "<float, 4>", stem "<float, 1>", stem "<_Float16, 8>", stem "<_Float16, 1>"}
static inline int si_kernel_name_index(bool half, bool vec) { return (half ? 2 : 0) + (vec ? 0 : 1); }

#endif  // SI_REDUCE_PLAN_H_
