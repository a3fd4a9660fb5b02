// binary_plan.h -- the host arithmetic of the constant-operand kernel (include/si_binary.h): the op-code tables, descriptor validation,
// the choice of form and vector arm, the grid.  Pure: nothing of HIP, so it is exercised without a device (tests/cpp/test_binary_plan.cpp).
#ifndef SI_BINARY_PLAN_H_
#define SI_BINARY_PLAN_H_

#include <cstdint>

#include "si_binary.h"
#include "si_views.h"

// ---- the BinaryOp codes of pnnx's expression lowering (0 add, 1 sub, 2 mul, 3 div, 6 pow, 10 atan2; 7, 8, 9, 11 their operand-reversed
// forms).  One table for every kernel file that serves them.
constexpr bool si_binary_op_known(int op) { return (op >= 0 && op <= 3) || (op >= 6 && op <= 11); }
// the code that computes op(y, x) as f(x, y): add and mul commute exactly
constexpr int si_binary_op_reversed(int op) {
    switch (op) {
        case 1: return 7; case 7: return 1;
        case 3: return 8; case 8: return 3;
        case 6: return 9; case 9: return 6;
        case 10: return 11; case 11: return 10;
        default: return op;
    }
}

namespace si_binary_plan {

constexpr uint64_t kIndexLimit = 0x7fffffffull;   // kernels index with 32-bit element offsets
constexpr int kThreads = 256;
constexpr unsigned kGridCap = 256u * 8u;          // ~8 workgroups per CU; the rest by grid stride

enum Form { kChan = 0, kPixel = 1, kFull = 2 };

struct Plan {
    int form = kFull;
    int vw = 1;                  // elements of x / out per lane: 16 bytes' worth, or 1
    int cvec[2] = {0, 0};        // full form: this stage's constant is read as vectors of vw elements
    int cv = 0;                  // lanes per run: d[3] / vw
    unsigned pixels = 0;         // d[0] * d[1] * d[2]
    unsigned items = 0;          // pixels * cv
    unsigned blocks = 0;         // workgroups of kThreads lanes
    unsigned lanes = 0;          // chan form: the lanes that work, a multiple of cv (a lane keeps its place in the run on every pass)
    unsigned pixel_step = 0;     // chan form: lanes / cv, the pixels between two passes of a lane
};

inline const int* Strides(const SiBinaryDesc* d, int stage) { return stage == 0 ? d->c0_stride : d->c1_stride; }

// everything that can be decided without a device: SI_E_BADARG / SI_E_UNSUPPORTED / 0.  elem: bytes of an element (4 or 2).
inline int MakePlan(const SiBinaryDesc* d, const void* x, const void* c0, const void* c1, const void* out, int elem, Plan& p) {
    if (!d || !x || !c0 || !out) return SI_E_BADARG;
    if (d->stages < 1 || d->stages > 2) return SI_E_BADARG;
    if (d->stages == 2 && !c1) return SI_E_BADARG;
    if (d->grid_cap < 0) return SI_E_BADARG;
    for (int i = 0; i < 4; ++i)
        if (d->d[i] <= 0) return SI_E_BADARG;
    if (d->x_ld < d->d[3] || d->out_ld < d->d[3]) return SI_E_BADARG;
    for (int s = 0; s < d->stages; ++s)
        for (int i = 0; i < 4; ++i)
            if (Strides(d, s)[i] < 0) return SI_E_BADARG;
    // x and out: pixels * ld elements; every factor is below 2^31, so each product is checked before the next can overflow 64 bits
    uint64_t pixels = (uint64_t)d->d[0] * (uint64_t)d->d[1];
    if (pixels > kIndexLimit) return SI_E_BADARG;
    pixels *= (uint64_t)d->d[2];
    if (pixels > kIndexLimit) return SI_E_BADARG;
    if (pixels * (uint64_t)d->x_ld > kIndexLimit || pixels * (uint64_t)d->out_ld > kIndexLimit) return SI_E_BADARG;
    // a constant: the offset of its last element
    for (int s = 0; s < d->stages; ++s) {
        uint64_t last = 0;
        for (int i = 0; i < 4; ++i) {
            last += (uint64_t)(d->d[i] - 1) * (uint64_t)Strides(d, s)[i];   // < 2^62 each; checked before the next is added
            if (last >= kIndexLimit) return SI_E_BADARG;
        }
    }
    for (int s = 0; s < d->stages; ++s)
        if (!si_binary_op_known(d->op[s])) return SI_E_UNSUPPORTED;

    const int full = 16 / elem;
    const bool vec = d->d[3] % full == 0 && d->x_ld % full == 0 && d->out_ld % full == 0 && si_aligned_to(x, 16) && si_aligned_to(out, 16);
    p.vw = vec ? full : 1;
    p.cv = d->d[3] / p.vw;
    p.pixels = (unsigned)pixels;
    p.items = (unsigned)(pixels * (uint64_t)p.cv);
    const unsigned cap = d->grid_cap > 0 && (unsigned)d->grid_cap < kGridCap ? (unsigned)d->grid_cap : kGridCap;
    unsigned blocks = (p.items + kThreads - 1) / kThreads;
    p.blocks = blocks > cap ? cap : blocks;

    bool chan = true, pixel = true;
    for (int s = 0; s < d->stages; ++s) {
        const int* cs = Strides(d, s);
        chan = chan && cs[0] == 0 && cs[1] == 0 && cs[2] == 0;
        pixel = pixel && cs[3] == 0;
        const void* c = s == 0 ? c0 : c1;
        p.cvec[s] = p.vw > 1 && cs[3] == 1 && cs[0] % p.vw == 0 && cs[1] % p.vw == 0 && cs[2] % p.vw == 0 && si_aligned_to(c, 16);
    }
    // a lane of the chan form keeps its place in the run: the run has to fit the grid once (it does unless grid_cap is tiny)
    const unsigned threads = p.blocks * (unsigned)kThreads;
    if (chan && (unsigned)p.cv <= threads) {
        p.form = kChan;
        p.pixel_step = threads / (unsigned)p.cv;
        if (p.pixel_step > p.pixels) p.pixel_step = p.pixels;
        p.lanes = p.pixel_step * (unsigned)p.cv;
    } else {
        p.form = pixel ? kPixel : kFull;
    }
    return 0;
}

}  // namespace si_binary_plan

#endif  // SI_BINARY_PLAN_H_
