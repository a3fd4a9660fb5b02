// The host arithmetic of the recurrent step kernel (simpleinfer_amd/csrc/hip/rnn_plan.h): gate count, padded k, grid, the W_hh image and its
// index, view extents next to 2^31, the row-sharing rule.  Stand-alone; built with -fsanitize=address,undefined by tests/test_rnn_cpu.py, so
// an overflow in a size computation or an image index out of its buffer ends the program.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "rnn_plan.h"

namespace plan = si_rnn_plan;

static int failures = 0;
#define EXPECT(cond)                                                              \
    do {                                                                          \
        if (!(cond)) {                                                            \
            std::printf("%s:%d: EXPECT(%s) failed\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                           \
        }                                                                         \
    } while (0)

int main() {
    EXPECT(plan::Gates(0) == 4 && plan::Gates(1) == 3 && plan::Gates(2) == 0 && plan::Gates(-1) == 0);
    EXPECT(plan::KStep(false) == 4 && plan::KStep(true) == 32);

    // the padded k and the unit tiles at H = 1, 15, 16, 17 and around the fp16 step
    const int hs[] = {1, 15, 16, 17, 31, 32, 33, 64, 136, 256, 2048};
    const int kp32[] = {4, 16, 16, 20, 32, 32, 36, 64, 136, 256, 2048};
    const int kp16[] = {32, 32, 32, 32, 32, 32, 64, 64, 160, 256, 2048};
    const int tiles[] = {1, 1, 1, 2, 2, 2, 3, 4, 9, 16, 128};
    for (int i = 0; i < 11; ++i) {
        EXPECT(plan::PaddedK(hs[i], false) == kp32[i]);
        EXPECT(plan::PaddedK(hs[i], true) == kp16[i]);
        EXPECT(plan::UnitTiles(hs[i]) == tiles[i]);
    }

    // the grid: (direction, 16 batch rows, 64 units)
    plan::Grid g;
    EXPECT(plan::MakeGrid(1, 1, 1, g) && g.blocks == 1 && g.row_tiles == 1 && g.unit_blocks == 1);
    EXPECT(plan::MakeGrid(16, 64, 2, g) && g.blocks == 2);
    EXPECT(plan::MakeGrid(17, 65, 2, g) && g.row_tiles == 2 && g.unit_blocks == 2 && g.blocks == 8);
    EXPECT(plan::MakeGrid(32, 256, 2, g) && g.blocks == 16);
    EXPECT(!plan::MakeGrid(0, 8, 1, g) && !plan::MakeGrid(8, 0, 1, g) && !plan::MakeGrid(8, 8, 0, g) && !plan::MakeGrid(8, 8, 3, g) && !plan::MakeGrid(-1, 8, 1, g));
    EXPECT(plan::MakeGrid(0x7fffffff, 64, 2, g) && g.row_tiles == (1u << 27) && g.blocks == (1ull << 28));
    EXPECT(!plan::MakeGrid(0x7fffffff, 0x7fffffff, 2, g));

    // the W_hh image: every (direction, tile, k step, gate, lane) has a slot of its own inside the image, and the slots fill it
    for (int cell = 0; cell < 2; ++cell)
        for (int half = 0; half < 2; ++half)
            for (int hidden : {1, 15, 16, 17, 33, 136})
                for (int dirs = 1; dirs <= 2; ++dirs) {
                    const uint64_t elems = plan::WhhImageElems(cell, hidden, dirs, half != 0);
                    const int per = half ? 8 : 1, ks = plan::PaddedK(hidden, half != 0) / plan::KStep(half != 0);
                    EXPECT(elems == (uint64_t)dirs * plan::UnitTiles(hidden) * plan::Gates(cell) * 16 * plan::PaddedK(hidden, half != 0));
                    EXPECT(elems % per == 0);
                    std::vector<unsigned char> seen(elems / per, 0);
                    for (int d = 0; d < dirs; ++d)
                        for (int tile = 0; tile < plan::UnitTiles(hidden); ++tile)
                            for (int s = 0; s < ks; ++s)
                                for (int q = 0; q < plan::Gates(cell); ++q)
                                    for (int lane = 0; lane < 64; ++lane) {
                                        const uint64_t at = plan::WhhImageIndex(cell, hidden, half != 0, d, tile, s, q, lane);
                                        EXPECT(at < seen.size());
                                        if (at < seen.size()) {
                                            EXPECT(seen[at] == 0);
                                            seen[at] = 1;
                                        }
                                    }
                    uint64_t filled = 0;
                    for (unsigned char v : seen) filled += v;
                    EXPECT(filled == seen.size());
                }
    EXPECT(plan::WhhImageElems(2, 8, 1, false) == 0 && plan::WhhImageElems(0, 0, 1, false) == 0 && plan::WhhImageElems(0, 8, 3, false) == 0);
    // H = 2048, bidirectional LSTM: 2 * 128 * 4 * 16 * 2048 = 2^25 elements, far inside 31 bits
    EXPECT(plan::WhhImageElems(0, 2048, 2, false) == (1ull << 25) && plan::WhhImageElems(0, 2048, 2, true) == (1ull << 25));

    // the dense gate workspace T N D G H next to 2^31
    EXPECT(plan::DenseGateElems(0, 26, 32, 256, 2) == 26ull * 32 * 2 * 4 * 256);
    EXPECT(plan::DenseGateElems(0, 1 << 10, 1 << 10, 1 << 7, 2) == 1ull << 30);          // 2^20 rows x 2^10 columns
    EXPECT(plan::DenseGateElems(0, 1 << 10, 1 << 10, 1 << 8, 2) == 0);                   // 2^31: one too many
    EXPECT(plan::DenseGateElems(0, 2047, 1 << 10, 1 << 7, 2) == 2047ull << 20);          // 2^31 - 2^20
    EXPECT(plan::DenseGateElems(1, 0x7fffffff, 0x7fffffff, 2048, 2) == 0);               // the products stay inside 64 bits
    EXPECT(plan::DenseGateElems(1, 1, 1, 1, 1) == 3 && plan::DenseGateElems(2, 1, 1, 1, 1) == 0 && plan::DenseGateElems(0, 0, 1, 1, 1) == 0);
    EXPECT(plan::StateElems(32, 256, 2) == 16384 && plan::StateElems(0, 8, 1) == 0);
    EXPECT(plan::StateElems(0x7fffffff, 2048, 2) == 2ull * 0x7fffffffull * 2048ull);

    // view extents: one past the last offset; 0 beyond 31 bits or for a negative stride
    EXPECT(plan::ViewExtent(1, 1, 8, 8, 8) == 8);
    EXPECT(plan::ViewExtent(10, 4, 4 * 24, 24, 12) == 9 * 96 + 3 * 24 + 12);
    EXPECT(plan::ViewExtent(10, 4, 24, 10 * 24, 12) == 9 * 24 + 3 * 240 + 12);
    EXPECT(plan::ViewExtent(2, 1, 0x7fffffffll - 7, 8, 8) == 0x80000000ull);              // last offset 2^31 - 1: the largest that fits
    EXPECT(plan::ViewExtent(2, 1, 0x7fffffffll - 6, 8, 8) == 0);                          // last offset 2^31
    EXPECT(plan::ViewExtent(0x7fffffff, 0x7fffffff, 0x7fffffff, 0x7fffffff, 0x7fffffff) == 0);
    EXPECT(plan::ViewExtent(2, 2, -8, 8, 8) == 0 && plan::ViewExtent(2, 2, 8, -8, 8) == 0 && plan::ViewExtent(2, 2, 1ll << 40, 8, 8) == 0);
    EXPECT(plan::ViewExtent(0, 2, 8, 8, 8) == 0 && plan::ViewExtent(2, 2, 8, 8, 0) == 0);

    // rows of a written view must not share an element
    EXPECT(plan::RowsDisjoint(10, 4, 4 * 12, 12, 12) && plan::RowsDisjoint(10, 4, 12, 10 * 12, 12));
    EXPECT(plan::RowsDisjoint(10, 4, 4 * 16, 16, 12) && plan::RowsDisjoint(1, 4, 0, 12, 12) && plan::RowsDisjoint(10, 1, 12, 0, 12));
    EXPECT(!plan::RowsDisjoint(10, 4, 12, 12, 12));       // (s = 1, b = 0) on (s = 0, b = 1)
    EXPECT(!plan::RowsDisjoint(10, 4, 8, 120, 12) && !plan::RowsDisjoint(10, 4, 48, 8, 12));
    EXPECT(!plan::RowsDisjoint(10, 4, 3 * 12, 12, 12));   // the time stride one batch row short

    // LDS of the h tile: H = 2048 in fp32 is the largest, 139264 bytes, inside 160 KB
    EXPECT(plan::LdsBytes(256, false) == 256 * 17 * 4 && plan::LdsBytes(256, true) == 256 * 16 * 2 && plan::LdsBytes(1, true) == 32 * 32);
    EXPECT(plan::LdsBytes(plan::kMaxHidden, false) == 139264 && plan::LdsBytes(plan::kMaxHidden, false) <= 160 * 1024);

    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("rnn plan ok\n");
    return 0;
}
