// cdist_plan.h -- the host arithmetic of the pairwise-distance kernels (include/si_cdist.h): the refusals, which kernel and which
// instantiation serve a descriptor, the view extents with their 31-bit checks and the grid.  Pure: nothing of the device runtime, so it is
// exercised without a device (tests/cpp/test_cdist_plan.cpp).
#ifndef SI_CDIST_PLAN_H_
#define SI_CDIST_PLAN_H_

#include <cstdint>

#include "si_cdist.h"

namespace si_cdist_plan {

constexpr uint64_t kIndexLimit = 0x7fffffffull;   // kernels index with 32-bit element offsets
constexpr uint64_t kGridLimitZ = 65535;           // a grid's z extent: the kernels loop over further batch items
constexpr int kTile = 64;                         // rows and columns of a workgroup's tile of out, in both kernels

enum Form { kNone = 0, kMm = 1, kDirect = 2 };

inline int Batch(const SiCdistDesc& d) { return d.b1 > d.b2 ? d.b1 : d.b2; }

// one past the last element offset of a view of `items` batch items of `rows` rows of `width` elements
inline uint64_t ViewExtent(int items, int rows, int width, int sb, int ld) {
    return (uint64_t)(items - 1) * (uint64_t)sb + (uint64_t)(rows - 1) * (uint64_t)ld + (uint64_t)width;
}
// the same with the batch stride an operand is really read with: 0 for a single item
inline uint64_t OperandExtent(int items, int rows, int width, int sb, int ld) { return ViewExtent(items, rows, width, items > 1 ? sb : 0, ld); }

// 0, SI_E_BADARG or SI_E_UNSUPPORTED for the descriptor alone (the pointers: Overlaps below); SI_E_BADARG is looked for first
inline int Check(const SiCdistDesc& d) {
    if (d.b1 <= 0 || d.b2 <= 0 || d.p <= 0 || d.r <= 0 || d.m <= 0) return SI_E_BADARG;
    if (d.b1 != d.b2 && d.b1 != 1 && d.b2 != 1) return SI_E_BADARG;
    if (d.x1_ld < d.m || d.x2_ld < d.m || d.out_ld < d.r) return SI_E_BADARG;
    // batch items at least one item apart (64-bit: an item may itself be beyond the index limit)
    if (d.b1 > 1 && (int64_t)d.x1_sb < (int64_t)(d.p - 1) * d.x1_ld + d.m) return SI_E_BADARG;
    if (d.b2 > 1 && (int64_t)d.x2_sb < (int64_t)(d.r - 1) * d.x2_ld + d.m) return SI_E_BADARG;
    if (Batch(d) > 1 && (int64_t)d.out_sb < (int64_t)(d.p - 1) * d.out_ld + d.r) return SI_E_BADARG;
    if (d.norm != SI_CDIST_NORM_1 && d.norm != SI_CDIST_NORM_2 && d.norm != SI_CDIST_NORM_INF) return SI_E_UNSUPPORTED;
    if (d.mode != SI_CDIST_MODE_MM_IF_NECESSARY && d.mode != SI_CDIST_MODE_MM && d.mode != SI_CDIST_MODE_NO_MM) return SI_E_UNSUPPORTED;
    if (OperandExtent(d.b1, d.p, d.m, d.x1_sb, d.x1_ld) > kIndexLimit || OperandExtent(d.b2, d.r, d.m, d.x2_sb, d.x2_ld) > kIndexLimit ||
        OperandExtent(Batch(d), d.p, d.r, d.out_sb, d.out_ld) > kIndexLimit)
        return SI_E_UNSUPPORTED;
    return 0;
}

// torch's rule, from the descriptor alone
inline Form FormOf(const SiCdistDesc& d) {
    if (Check(d) != 0) return kNone;
    if (d.norm != SI_CDIST_NORM_2 || d.mode == SI_CDIST_MODE_NO_MM) return kDirect;
    if (d.mode == SI_CDIST_MODE_MM) return kMm;
    return (d.p > SI_CDIST_MM_THRESHOLD || d.r > SI_CDIST_MM_THRESHOLD) ? kMm : kDirect;
}

// the mm kernel's 16-byte vector instantiation: `width` elements per vector (4 floats, 8 halves)
inline bool Vector(const SiCdistDesc& d, int width, uintptr_t x1, uintptr_t x2) {
    if (d.m % width || d.x1_ld % width || d.x2_ld % width || (x1 & 15) || (x2 & 15)) return false;
    return (d.b1 == 1 || d.x1_sb % width == 0) && (d.b2 == 1 || d.x2_sb % width == 0);
}

// does out share a byte with x1 or x2?  (esize: bytes of an element)
inline bool Overlaps(const SiCdistDesc& d, uintptr_t x1, uintptr_t x2, uintptr_t out, uint64_t esize) {
    const uint64_t o = OperandExtent(Batch(d), d.p, d.r, d.out_sb, d.out_ld) * esize;
    const uint64_t a = OperandExtent(d.b1, d.p, d.m, d.x1_sb, d.x1_ld) * esize, b = OperandExtent(d.b2, d.r, d.m, d.x2_sb, d.x2_ld) * esize;
    return (out < x1 + a && x1 < out + o) || (out < x2 + b && x2 < out + o);
}

struct Grid {
    unsigned x = 0, z = 0;
    int p_tiles = 0, r_tiles = 0;
};

// x: the tiles under the numbering of si_g64_tile (the p tiles rounded up to 8), z: min(B, 65535).  A descriptor that passed Check has
// p * r < 2^31 outputs, so x <= (p / 64 + 8) * (r / 64 + 1) <= p r / 4096 + p / 64 + r / 8 + 8 fits 31 bits with room to spare
inline Grid MakeGrid(const SiCdistDesc& d) {
    Grid g;
    g.p_tiles = (d.p + kTile - 1) / kTile;
    g.r_tiles = (d.r + kTile - 1) / kTile;
    g.x = (unsigned)((uint64_t)((g.p_tiles + 7) / 8 * 8) * (uint64_t)g.r_tiles);
    g.z = (unsigned)((uint64_t)Batch(d) < kGridLimitZ ? (uint64_t)Batch(d) : kGridLimitZ);
    return g;
}

}  // namespace si_cdist_plan

#endif  // SI_CDIST_PLAN_H_
