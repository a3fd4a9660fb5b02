// rnn_plan.h -- the host arithmetic of the recurrent step kernel (include/si_rnn.h): gate count, padded k, grid, buffer sizes and the 31-bit
// checks.  Pure: nothing of HIP, so it is exercised without a device (tests/cpp/test_rnn_plan.cpp).
#ifndef SI_RNN_PLAN_H_
#define SI_RNN_PLAN_H_

#include <cstdint>

namespace si_rnn_plan {

constexpr uint64_t kIndexLimit = 0x7fffffffull;   // kernels index with 32-bit element offsets
constexpr int kTileRows = 16;                     // batch rows of a workgroup (the N of the MFMA)
constexpr int kWaveUnits = 16;                    // hidden units of a wave (the M of the MFMA)
constexpr int kBlockUnits = 64;                   // hidden units of a workgroup of four waves
constexpr int kMaxHidden = 2048;                  // fp32 LDS image of h: 17 * 4 * padded k bytes <= 160 KB

// gates of a cell: 0 LSTM (i, f, g, o), 1 GRU (r, z, n); 0 for anything else
inline int Gates(int cell) { return cell == 0 ? 4 : cell == 1 ? 3 : 0; }

// the k of one MFMA: v_mfma_f32_16x16x4_f32 / v_mfma_f32_16x16x32_f16
inline int KStep(bool half) { return half ? 32 : 4; }

// hidden rounded up to the instruction's k (hidden > 0)
inline int PaddedK(int hidden, bool half) {
    const int k = KStep(half);
    return (int)(((int64_t)hidden + k - 1) / k * k);
}

inline int UnitTiles(int hidden) { return (int)(((int64_t)hidden + kWaveUnits - 1) / kWaveUnits); }

struct Grid {
    unsigned dirs = 0, row_tiles = 0, unit_blocks = 0;
    uint64_t blocks = 0;
};

// the grid of one step: (direction, tile of 16 batch rows, block of 64 hidden units); false: sizes out of range or beyond 31 bits
inline bool MakeGrid(int batch, int hidden, int dirs, Grid& g) {
    if (batch <= 0 || hidden <= 0 || dirs < 1 || dirs > 2) return false;
    g.dirs = (unsigned)dirs;
    g.row_tiles = (unsigned)(((int64_t)batch + kTileRows - 1) / kTileRows);
    g.unit_blocks = (unsigned)(((int64_t)hidden + kBlockUnits - 1) / kBlockUnits);
    g.blocks = (uint64_t)g.dirs * g.row_tiles * g.unit_blocks;
    return g.blocks <= kIndexLimit;
}

// elements of the W_hh image: [dirs][unit tile][k step][gate][64 lanes][1 float | 8 halves] = dirs * tiles * G * 16 * padded k
inline uint64_t WhhImageElems(int cell, int hidden, int dirs, bool half) {
    if (Gates(cell) == 0 || hidden <= 0 || dirs < 1 || dirs > 2) return 0;
    return (uint64_t)dirs * (uint64_t)UnitTiles(hidden) * (uint64_t)Gates(cell) * (uint64_t)kWaveUnits * (uint64_t)PaddedK(hidden, half);
}

// where (direction, unit tile, k step, gate, lane) starts in the image, in operand elements (floats, or groups of 8 halves)
inline uint64_t WhhImageIndex(int cell, int hidden, bool half, int dir, int tile, int kstep, int gate, int lane) {
    const uint64_t ks = (uint64_t)(PaddedK(hidden, half) / KStep(half));
    return ((((uint64_t)dir * UnitTiles(hidden) + tile) * ks + kstep) * Gates(cell) + gate) * 64 + lane;
}

// elements of the fp32 c buffer / of h_n / of c_n: [dirs, batch, hidden]
inline uint64_t StateElems(int batch, int hidden, int dirs) {
    if (batch <= 0 || hidden <= 0 || dirs < 1) return 0;
    return (uint64_t)dirs * (uint64_t)batch * (uint64_t)hidden;
}

// one past the last element offset of a view of t x batch rows of `width` elements, or 0 when a stride is negative or the offset does not
// fit 31 bits (every factor is below 2^31, so neither product nor their sum leaves 64 bits)
inline uint64_t ViewExtent(int t, int batch, long long st, long long sb, long long width) {
    if (t <= 0 || batch <= 0 || width <= 0 || st < 0 || sb < 0) return 0;
    if ((uint64_t)st > kIndexLimit || (uint64_t)sb > kIndexLimit || (uint64_t)width > kIndexLimit) return 0;
    const uint64_t last = (uint64_t)(t - 1) * (uint64_t)st + (uint64_t)(batch - 1) * (uint64_t)sb + (uint64_t)width - 1;
    return last > kIndexLimit ? 0 : last + 1;
}

// elements of the dense gate workspace [t * batch, dirs * G * hidden]; 0: beyond 31 bits
inline uint64_t DenseGateElems(int cell, int t, int batch, int hidden, int dirs) {
    if (Gates(cell) == 0 || t <= 0 || batch <= 0 || hidden <= 0 || dirs < 1 || dirs > 2) return 0;
    const uint64_t width = (uint64_t)dirs * Gates(cell) * (uint64_t)hidden;   // < 2^34
    const uint64_t rows = (uint64_t)t * (uint64_t)batch;                      // < 2^62
    if (width > kIndexLimit || rows > kIndexLimit) return 0;
    const uint64_t n = rows * width;
    return n > kIndexLimit ? 0 : n;
}

// rows (s, b) of a written view must not share an element: the stride of each index at least the width, and one index stepping over the
// whole of the other one
inline bool RowsDisjoint(int t, int batch, long long st, long long sb, long long width) {
    if (t > 1 && st < width) return false;
    if (batch > 1 && sb < width) return false;
    if (t > 1 && batch > 1 && st < (long long)(batch - 1) * sb + width && sb < (long long)(t - 1) * st + width) return false;
    return true;
}

// LDS bytes of the h_{t-1} tile: fp32 [padded k][17] floats (row pitch 17: the staging stores of neighbouring k take neighbouring banks),
// fp16 [padded k / 8][16 rows][8 halves]
inline uint64_t LdsBytes(int hidden, bool half) {
    const uint64_t kp = (uint64_t)PaddedK(hidden, half);
    return half ? kp * kTileRows * 2 : kp * (kTileRows + 1) * 4;
}

}  // namespace si_rnn_plan

#endif  // SI_RNN_PLAN_H_
