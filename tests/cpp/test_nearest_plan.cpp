// The host arithmetic of the fused nearest-row search: nearest_plan.h (simpleinfer_amd/csrc/hip: refusals, extents next to 2^31, the split
// over r, the workspace, the grids).  Stand-alone (plain C++ headers only); built with -fsanitize=address,undefined by tests/test_nearest_cpu.py.
#include <cstdio>
#include <initializer_list>

#include "nearest_plan.h"

namespace plan = si_nearest_plan;

static int failures = 0;
#define EXPECT(cond) \
    do { if (!(cond)) { std::printf("%s:%d: EXPECT(%s) failed\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

// dense operands [b1, p, m] and [b2, r, m]
static SiNearestDesc Desc(int b1, int b2, int p, int r, int m, int k = 1, int splits = 0) {
    SiNearestDesc d = {};
    d.b1 = b1; d.b2 = b2; d.p = p; d.r = r; d.m = m;
    d.x1_ld = d.x2_ld = d.rows_ld = m;
    d.x1_sb = d.rows_sb = (int)((long long)p * m); d.x2_sb = (int)((long long)r * m);
    d.k = k; d.splits = splits;
    return d;
}

int main() {
    // ---- refusals
    EXPECT(plan::Check(Desc(3, 3, 5, 4, 8), false) == 0 && plan::Check(Desc(1, 3, 5, 4, 8, 2, 16), true) == 0);
    EXPECT(plan::Check(Desc(3, 2, 5, 4, 8), false) == SI_E_BADARG && plan::Check(Desc(1, 1, 5, 0, 8), false) == SI_E_BADARG);
    EXPECT(plan::Check(Desc(1, 1, 5, 1, 8, 1), false) == 0 && plan::Check(Desc(1, 1, 5, 1, 8, 2), false) == SI_E_BADARG);       // k = 2 needs two rows
    for (int k : {0, 3, -1}) EXPECT(plan::Check(Desc(1, 1, 5, 4, 8, k), false) == SI_E_BADARG);
    EXPECT(plan::Check(Desc(1, 1, 5, 4, 8, 1, 17), false) == SI_E_BADARG && plan::Check(Desc(1, 1, 5, 4, 8, 1, -1), false) == SI_E_BADARG);
    SiNearestDesc d = Desc(1, 1, 5, 4, 8);
    d.rows_ld = 7;
    EXPECT(plan::Check(d, false) == SI_E_BADARG);
    d = Desc(2, 2, 5, 4, 8);
    d.rows_sb = 39;
    EXPECT(plan::Check(d, false) == SI_E_BADARG);
    // fp16: rows of a multiple of 8 halves, strides too; a bad stride is looked for before it
    EXPECT(plan::Check(Desc(1, 1, 5, 4, 12), false) == 0 && plan::Check(Desc(1, 1, 5, 4, 12), true) == SI_E_UNSUPPORTED);
    d = Desc(1, 1, 5, 4, 8);
    d.x2_ld = 12;
    EXPECT(plan::Check(d, false) == 0 && plan::Check(d, true) == SI_E_UNSUPPORTED);
    d.x2_ld = 7;
    EXPECT(plan::Check(d, true) == SI_E_BADARG);
    // ---- next to 2^31: r * 64 must fit, and every view's last element offset
    EXPECT(plan::kColumnLimit == 1 << 25);
    EXPECT(plan::Check(Desc(1, 1, 5, (1 << 25) - 1, 8), false) == 0 && plan::Tiles((1 << 25) - 1) == 1 << 19);
    EXPECT(plan::Check(Desc(1, 1, 5, 1 << 25, 8), false) == SI_E_UNSUPPORTED && plan::Check(Desc(1, 1, 5, 0x7fffffff, 1), false) == SI_E_UNSUPPORTED);
    EXPECT(plan::Tiles(0x7fffffff) == 1 << 25);                                                            // (no overflow in the round-up)
    EXPECT(plan::Check(Desc(1, 1, 1 << 27, 4, 8), false) == 0 && plan::Check(Desc(1, 1, (1 << 28) + 1, 4, 8), false) == SI_E_UNSUPPORTED);
    EXPECT(plan::Check(Desc(2, 1, 1 << 27, 4, 8), false) == SI_E_UNSUPPORTED);                            // the second item of x1 ends at 2^31
    EXPECT(plan::OperandExtent(2, 1 << 27, 8, 1 << 30, 8) == 1ull << 31 && plan::OperandExtent(1, 1 << 27, 8, 1 << 30, 8) == 1ull << 30);
    EXPECT(plan::Check(Desc(1, 1, 0x7fffffff, 4, 1, 1), false) == 0 && plan::Check(Desc(1, 1, 0x7fffffff, 4, 1, 2), false) == SI_E_UNSUPPORTED);   // idx: p * k
    // ---- the split: fill `cus` compute units, at most 16, at most the column tiles; a forced value stands
    EXPECT(plan::Splits(Desc(1, 1, 8192, 8192, 64)) == 2 && plan::Splits(Desc(2, 1, 8192, 8192, 64)) == 1 &&plan::Splits(Desc(1, 1, 64 * 256, 64, 8)) == 1 && plan::Splits(Desc(1, 1, 64 * 255, 6400, 8)) == 1);
    EXPECT(plan::Splits(Desc(1, 1, 256, 16384, 64)) == 16 && plan::Splits(Desc(1, 1, 64 * 100, 16384, 64)) == 2 && plan::Splits(Desc(1, 1, 64 * 129, 16384, 64)) == 1);
    EXPECT(plan::Splits(Desc(3, 1, 70, 200, 24)) == 4 && plan::Splits(Desc(1, 3, 5, 65, 24)) == 2 && plan::Splits(Desc(1, 1, 5, 64, 24)) == 1);
    EXPECT(plan::Splits(Desc(1, 1, 256, 16384, 64), 8) == 2 && plan::Splits(Desc(1, 1, 256, 16384, 64), 4) == 1);
    EXPECT(plan::Splits(Desc(1, 1, 5, 65, 24, 1, 16)) == 16 && plan::Splits(Desc(1, 1, 8192, 8192, 64, 1, 3)) == 3);
    // every column tile belongs to exactly one split, also where some splits get none
    for (int r : {1, 64, 65, 200, 1000, (1 << 25) - 1})
        for (int s = 1; s <= SI_NEAREST_MAX_SPLITS; ++s) {
            const SiNearestDesc e = Desc(1, 1, 5, r, 8, 1, s);
            const long long t = plan::TilesPerSplit(e, s);
            EXPECT(t * s >= plan::Tiles(r) && (t - 1) * s < plan::Tiles(r));
        }
    // ---- the workspace and the grids
    EXPECT(plan::WorkspaceBytes(Desc(1, 1, 256, 16384, 64), 1) == 0 && plan::WorkspaceBytes(Desc(3, 1, 70, 200, 24, 2), 4) == 3u * 70 * 2 * 4 * 8);
    EXPECT(plan::WorkspaceBytes(Desc(1, 1, 0x7fffffff, 4, 1, 1), 16) == (size_t)0x7fffffffull * 16 * 8);
    plan::Grid g = plan::MakeGrid(Desc(70000, 1, 65, 200, 8, 2, 3));
    EXPECT(g.p_tiles == 2 && g.r_tiles == 4 && g.splits == 3 && g.tiles_per_split == 2 && g.x == 6 && g.combine_x == 2 && g.z == 65535);
    g = plan::MakeGrid(Desc(1, 1, 0x7fffffff, 4, 1, 1, 16));
    EXPECT(g.p_tiles == 1 << 25 && g.x == 1u << 29 && g.z == 1);
    g = plan::MakeGrid(Desc(2, 1, 8192, 8192, 64));
    EXPECT(g.splits == 1 && g.x == 128 && g.combine_x == 0 && g.tiles_per_split == 128 && g.z == 2);

    std::printf(failures ? "%d failures\n" : "nearest plan ok\n", failures);
    return failures ? 1 : 0;
}
