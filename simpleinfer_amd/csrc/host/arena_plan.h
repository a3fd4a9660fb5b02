// arena_plan.h -- packing of the activation arena: buffers with a size and a lifetime in plan steps get offsets into ONE allocation so that two
// buffers overlap in memory only when no step needs both.  Pure: standard headers only, so it is tested without a device (tests/cpp/test_arena_plan.cpp).
#ifndef SIMPLE_INFER_SRC_ARENA_PLAN_H_
#define SIMPLE_INFER_SRC_ARENA_PLAN_H_

#include <algorithm>
#include <cstddef>
#include <utility>
#include <vector>

namespace SimpleInfer {

struct ArenaBuffer {
    size_t bytes;      // as the operand needs them: the packer rounds up to 256
    int first, last;   // the first step that writes the buffer and the last that reads it, both inclusive; first < 0: no step touches it
};

struct ArenaLayout {
    std::vector<size_t> offsets;   // per buffer, a multiple of 256
    size_t total = 0;
};

// Greedy by size (descending, ties by index): each buffer goes to the lowest offset that is free during its whole life.  A buffer that no step
// of the plan touches (an operand only a fused-away operator produced) lives for the whole forward, [0, plan_steps].
inline ArenaLayout PackArena(std::vector<ArenaBuffer> bufs, int plan_steps) {
    for (ArenaBuffer& b : bufs) {
        b.bytes = (b.bytes + 255) & ~size_t(255);
        if (b.first < 0) { b.first = 0; b.last = plan_steps; }
    }
    ArenaLayout out;
    out.offsets.assign(bufs.size(), 0);
    std::vector<size_t> order(bufs.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = i;
    std::sort(order.begin(), order.end(), [&](size_t x, size_t y) { return bufs[x].bytes != bufs[y].bytes ? bufs[x].bytes > bufs[y].bytes : x < y; });
    std::vector<size_t> placed;
    for (size_t bi : order) {
        const ArenaBuffer& b = bufs[bi];
        std::vector<std::pair<size_t, size_t>> busy;   // [offset, end) of placed buffers alive at the same time
        for (size_t pj : placed) {
            const ArenaBuffer& o = bufs[pj];
            if (o.first <= b.last && b.first <= o.last) busy.push_back(std::make_pair(out.offsets[pj], out.offsets[pj] + o.bytes));
        }
        std::sort(busy.begin(), busy.end());
        size_t off = 0;
        for (auto& iv : busy) {
            if (off + b.bytes <= iv.first) break;
            if (iv.second > off) off = iv.second;
        }
        out.offsets[bi] = off;
        if (off + b.bytes > out.total) out.total = off + b.bytes;
        placed.push_back(bi);
    }
    return out;
}

}  // namespace SimpleInfer

#endif
