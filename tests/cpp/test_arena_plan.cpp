// The activation arena packer (simpleinfer_amd/csrc/host/arena_plan.h) on its own: fixed cases with offsets worked by hand and seeded random cases
// held to the packer's invariants.  Stand-alone; built with -fsanitize=address,undefined by tests/test_arena_plan_cpu.py.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "arena_plan.h"

using SimpleInfer::ArenaBuffer;
using SimpleInfer::ArenaLayout;
using SimpleInfer::PackArena;

static int failures = 0;
#define EXPECT(cond)                                                            \
    do {                                                                        \
        if (!(cond)) {                                                          \
            std::printf("%s:%d: EXPECT(%s) failed\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                         \
        }                                                                       \
    } while (0)

static size_t Rounded(size_t b) { return (b + 255) / 256 * 256; }

static bool SameOffsets(const ArenaLayout& l, std::vector<size_t> want) { return l.offsets == want; }

static void FixedCases() {
    {
        ArenaLayout l = PackArena({}, 7);
        EXPECT(l.total == 0 && l.offsets.empty());
    }
    {   // pairwise disjoint lifetimes: everything at 0, the total is the largest rounded size
        ArenaLayout l = PackArena({{300, 0, 1}, {5000, 2, 2}, {1, 3, 9}, {4097, 10, 11}}, 12);
        EXPECT(SameOffsets(l, {0, 0, 0, 0}));
        EXPECT(l.total == 5120);
    }
    {   // all lifetimes intersect (step 4 is in every one): the total is the sum of the rounded sizes
        std::vector<ArenaBuffer> b = {{300, 0, 4}, {5000, 4, 9}, {1, 2, 6}, {4097, 4, 4}};
        ArenaLayout l = PackArena(b, 10);
        EXPECT(l.total == 512 + 5120 + 256 + 4352);
        EXPECT(SameOffsets(l, {5120 + 4352, 0, 5120 + 4352 + 512, 5120}));   // by size: 1 (5120), 3 (4352), 0 (512), 2 (256)
    }
    {   // the gap case.  Index: bytes -> rounded, life
        //   0: 1000 -> 1024 [0,1]    1: 257 -> 512 [2,5]    2: 700 -> 768 [1,3]    3: 1 -> 256 [4,6]    4: 256 -> 256 [3,4]
        // Placing order (size descending, ties by index): 0, 2, 1, 3, 4.
        //   0: nothing placed                                         -> 0      [0, 1024)
        //   2: alive with 0 (step 1): busy [0,1024)                   -> 1024   [1024, 1792)
        //   1: not alive with 0 (1 < 2); alive with 2 (steps 2..3): busy [1024,1792); 0 + 512 <= 1024: the hole below 2 -> 0   [0, 512)
        //   3: alive with 1 only (steps 4..5; 2 ends at 3): busy [0,512)               -> 512    [512, 768)
        //   4: alive with 2 (3), 1 (3..4), 3 (4): busy [0,512) [512,768) [1024,1792): 768 + 256 <= 1024: the hole between 3 and 2 -> 768
        // total 1792
        ArenaLayout l = PackArena({{1000, 0, 1}, {257, 2, 5}, {700, 1, 3}, {1, 4, 6}, {256, 3, 4}}, 7);
        EXPECT(SameOffsets(l, {0, 0, 1024, 512, 768}));
        EXPECT(l.total == 1792);
    }
    {   // equal (rounded) sizes are placed in index order
        ArenaLayout l = PackArena({{512, 0, 3}, {300, 1, 2}, {257, 0, 5}}, 6);
        EXPECT(SameOffsets(l, {0, 512, 1024}));
        EXPECT(l.total == 1536);
    }
    {   // lifetimes are inclusive on both ends: a.last == b.first overlaps, a.last + 1 == b.first does not
        ArenaLayout touch = PackArena({{256, 0, 3}, {256, 3, 5}}, 6);
        EXPECT(SameOffsets(touch, {0, 256}) && touch.total == 512);
        ArenaLayout apart = PackArena({{256, 0, 3}, {256, 4, 5}}, 6);
        EXPECT(SameOffsets(apart, {0, 0}) && apart.total == 256);
    }
    {   // a buffer no step touches lives for [0, plan size]: it shares with nothing, not even with a buffer of the last step
        ArenaLayout l = PackArena({{256, -1, -1}, {512, 0, 0}, {512, 9, 9}}, 9);
        EXPECT(SameOffsets(l, {512, 0, 0}) && l.total == 768);
    }
}

static uint32_t Next(uint32_t& s) {
    s = s * 1664525u + 1013904223u;
    return s >> 8;
}

static void RandomCases() {
    const int plan_steps = 16;
    for (uint32_t seed = 1; seed <= 400; ++seed) {
        uint32_t s = seed;
        std::vector<ArenaBuffer> b(Next(s) % 13);
        for (ArenaBuffer& x : b) {
            x.bytes = 1 + Next(s) % (seed % 3 ? 5000 : 600);   // (small ranges give equal rounded sizes)
            if (Next(s) % 8 == 0) { x.first = x.last = -1; continue; }
            x.first = (int)(Next(s) % plan_steps);
            x.last = x.first + (int)(Next(s) % (plan_steps - x.first));
        }
        const ArenaLayout l = PackArena(b, plan_steps);
        const ArenaLayout again = PackArena(b, plan_steps);
        EXPECT(l.offsets == again.offsets && l.total == again.total);
        EXPECT(l.offsets.size() == b.size());
        size_t sum = 0, largest = 0;
        for (size_t i = 0; i < b.size(); ++i) {
            const size_t ri = Rounded(b[i].bytes);
            sum += ri;
            if (ri > largest) largest = ri;
            EXPECT(l.offsets[i] % 256 == 0);
            EXPECT(l.offsets[i] + ri <= l.total);
            const int fi = b[i].first < 0 ? 0 : b[i].first, li = b[i].first < 0 ? plan_steps : b[i].last;
            for (size_t j = i + 1; j < b.size(); ++j) {
                const int fj = b[j].first < 0 ? 0 : b[j].first, lj = b[j].first < 0 ? plan_steps : b[j].last;
                if (fi > lj || fj > li) continue;   // never alive together: may share
                const size_t rj = Rounded(b[j].bytes);
                EXPECT(l.offsets[i] + ri <= l.offsets[j] || l.offsets[j] + rj <= l.offsets[i]);
            }
        }
        EXPECT(l.total <= sum && l.total >= largest);
    }
}

int main() {
    FixedCases();
    RandomCases();
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("arena plan ok\n");
    return 0;
}
