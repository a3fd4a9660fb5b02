// nearest_plan.h -- the host arithmetic of the fused nearest-row search (include/si_nearest.h): the refusals, the view extents with their
// 31-bit checks, the split over r, the workspace and the grids.  Pure: nothing of the device runtime, so it is exercised without a device
// (tests/cpp/test_nearest_plan.cpp).  The pointer rules (alignment, overlap) are si_views.h's and are asked in nearest.hip.
#ifndef SI_NEAREST_PLAN_H_
#define SI_NEAREST_PLAN_H_

#include <cstddef>
#include <cstdint>

#include "si_nearest.h"

namespace si_nearest_plan {

constexpr uint64_t kIndexLimit = 0x7fffffffull;   // kernels index with 32-bit element offsets
constexpr uint64_t kGridLimitZ = 65535;           // a grid's z extent: the kernels loop over further batch items
constexpr int kTile = 64;                         // rows of a workgroup's panel and columns of a tile
constexpr int kColumnLimit = (int)((1ull << 31) / kTile);   // r below this: r_tiles * 64 fits 31 bits
constexpr int kCus = 256;                         // the compute units the auto split fills: the MI355X's, a constant (no device query), so
                                                  // every other gfx950 part gets the MI355X's choice
constexpr size_t kPairBytes = 8;                  // a (key, column) pair of the workspace

inline int Batch(const SiNearestDesc& d) { return d.b1 > d.b2 ? d.b1 : d.b2; }

// one past the last element offset of `items` batch items (read with stride 0 when there is one) of `rows` rows of `width` elements
inline uint64_t OperandExtent(int items, int rows, int width, int sb, int ld) {
    return (uint64_t)(items - 1) * (uint64_t)(items > 1 ? sb : 0) + (uint64_t)(rows - 1) * (uint64_t)ld + (uint64_t)width;
}

// 0, SI_E_BADARG or SI_E_UNSUPPORTED for the descriptor alone; SI_E_BADARG is looked for first.  half: the fp16 entry
inline int Check(const SiNearestDesc& d, bool half) {
    if (d.b1 <= 0 || d.b2 <= 0 || d.p <= 0 || d.r <= 0 || d.m <= 0) return SI_E_BADARG;
    if (d.b1 != d.b2 && d.b1 != 1 && d.b2 != 1) return SI_E_BADARG;
    if ((d.k != 1 && d.k != 2) || d.r < d.k) return SI_E_BADARG;
    if (d.splits < 0 || d.splits > SI_NEAREST_MAX_SPLITS) return SI_E_BADARG;
    if (d.x1_ld < d.m || d.x2_ld < d.m || d.rows_ld < d.m) return SI_E_BADARG;
    if (d.b1 > 1 && (int64_t)d.x1_sb < (int64_t)(d.p - 1) * d.x1_ld + d.m) return SI_E_BADARG;
    if (d.b2 > 1 && (int64_t)d.x2_sb < (int64_t)(d.r - 1) * d.x2_ld + d.m) return SI_E_BADARG;
    if (Batch(d) > 1 && (int64_t)d.rows_sb < (int64_t)(d.p - 1) * d.rows_ld + d.m) return SI_E_BADARG;
    if (d.r >= kColumnLimit) return SI_E_UNSUPPORTED;
    if (OperandExtent(d.b1, d.p, d.m, d.x1_sb, d.x1_ld) > kIndexLimit || OperandExtent(d.b2, d.r, d.m, d.x2_sb, d.x2_ld) > kIndexLimit ||
        OperandExtent(Batch(d), d.p, d.m, d.rows_sb, d.rows_ld) > kIndexLimit)
        return SI_E_UNSUPPORTED;
    if ((uint64_t)Batch(d) * (uint64_t)d.p * (uint64_t)d.k > kIndexLimit) return SI_E_UNSUPPORTED;   // idx / dist
    if (half && (d.m % 8 || d.x1_ld % 8 || d.x2_ld % 8 || d.rows_ld % 8 || (d.b1 > 1 && d.x1_sb % 8) || (d.b2 > 1 && d.x2_sb % 8) ||
                 (Batch(d) > 1 && d.rows_sb % 8)))
        return SI_E_UNSUPPORTED;
    return 0;
}

inline int Tiles(int extent) { return (int)(((int64_t)extent + kTile - 1) / kTile); }

// the workgroups that share a row panel: the descriptor's, or the choice from p, r, B and the CU count
inline int Splits(const SiNearestDesc& d, int cus = kCus) {
    if (d.splits > 0) return d.splits;
    const int64_t panels = (int64_t)Tiles(d.p) * Batch(d);
    if (panels >= cus) return 1;
    int64_t s = cus / panels;
    if (s > Tiles(d.r)) s = Tiles(d.r);
    if (s > SI_NEAREST_MAX_SPLITS) s = SI_NEAREST_MAX_SPLITS;
    return (int)s;
}

// column tiles per split: split s takes tiles [s * T, (s + 1) * T) of Tiles(r)
inline int TilesPerSplit(const SiNearestDesc& d, int splits) { return (Tiles(d.r) + splits - 1) / splits; }

// B * p * splits * k pairs; B * p * k < 2^31 (Check), so the product fits 64 bits with room to spare
inline size_t WorkspaceBytes(const SiNearestDesc& d, int splits) {
    if (splits <= 1) return 0;
    return (size_t)((uint64_t)Batch(d) * (uint64_t)d.p * (uint64_t)d.k * (uint64_t)splits * kPairBytes);
}

// the vector instantiation of the search: `width` elements per 16-byte vector
inline bool Vector(const SiNearestDesc& d, int width, bool x1_aligned, bool x2_aligned) {
    if (d.m % width || d.x1_ld % width || d.x2_ld % width || !x1_aligned || !x2_aligned) return false;
    return (d.b1 == 1 || d.x1_sb % width == 0) && (d.b2 == 1 || d.x2_sb % width == 0);
}
// ... and of the copy of the winning rows (x2 -> rows)
inline bool RowsVector(const SiNearestDesc& d, int width, bool x2_aligned, bool rows_aligned) {
    if (d.m % width || d.x2_ld % width || d.rows_ld % width || !x2_aligned || !rows_aligned) return false;
    return (d.b2 == 1 || d.x2_sb % width == 0) && (Batch(d) == 1 || d.rows_sb % width == 0);
}

struct Grid {
    unsigned x = 0, combine_x = 0, z = 0;
    int p_tiles = 0, r_tiles = 0, splits = 0, tiles_per_split = 0;
};

// x: panel-major, the splits of a panel side by side; p * m < 2^31 gives p_tiles < 2^25 and x < 2^29
inline Grid MakeGrid(const SiNearestDesc& d, int cus = kCus) {
    Grid g;
    g.p_tiles = Tiles(d.p);
    g.r_tiles = Tiles(d.r);
    g.splits = Splits(d, cus);
    g.tiles_per_split = TilesPerSplit(d, g.splits);
    g.x = (unsigned)g.p_tiles * (unsigned)g.splits;
    g.combine_x = g.splits > 1 ? (unsigned)g.p_tiles : 0u;
    g.z = (unsigned)((uint64_t)Batch(d) < kGridLimitZ ? (uint64_t)Batch(d) : kGridLimitZ);
    return g;
}

}  // namespace si_nearest_plan

#endif  // SI_NEAREST_PLAN_H_
