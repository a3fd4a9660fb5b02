// si_reduce_dev.h -- device commons of the reduction files (softmax.hip, reduce.hip, lpnorm.hip, groupnorm.hip): the combine operations, the
// lane butterfly, the whole-workgroup combine, the register-resident row tile and the two-level position walk.  The ORDER in which values
// meet is what these operators promise (batch invariance, the same bits twice, the restatements under tests/): it is defined here, once.
// Included from si_hip_internal.h; a kernel file defines none of these for itself ("Device commons").
#ifndef SI_REDUCE_DEV_H_
#define SI_REDUCE_DEV_H_

#include <type_traits>

#include "si_reduce_plan.h"

// ---- combine operations.  Two maxima with different rules for a NaN; neither is a slip of the other (as si_act / si_act_exact).
//   SiMaxNum  fmaxf: a NaN operand is skipped.  softmax: the maximum only shifts the exponentials, and a NaN reaches the row through
//             exp(NaN - m) in the sum; a NaN maximum would poison rows that torch leaves finite nowhere else.
//   SiMaxNan  a NaN on either side comes out.  amax / amin and the p = inf norm, whose result IS the maximum: torch returns NaN.
struct SiSum {
    __device__ static __forceinline__ float apply(float a, float b) { return a + b; }
};
struct SiMaxNum {
    __device__ static __forceinline__ float apply(float a, float b) { return fmaxf(a, b); }
};
struct SiMaxNan {
    __device__ static __forceinline__ float apply(float a, float b) { return (a != a || a > b) ? a : b; }
};
template <bool MAX> using SiSumOrMaxNan = typename std::conditional<MAX, SiMaxNan, SiSum>::type;

// butterfly over the xor offsets below `lanes` (a power of two <= 64): lane j's value becomes v[j] (+) v[j ^ off] at every step, so lanes
// outside the team never enter, and for a commutative (+) every lane of the team ends with the same bits
template <typename Op>
__device__ __forceinline__ float si_team(float v, int lanes) {
    for (int off = lanes >> 1; off > 0; off >>= 1) v = Op::apply(v, __shfl_xor(v, off, 64));
    return v;
}

// the whole workgroup of WAVES waves: per wave as above, then the wave values from LDS in index order, read by every thread.  `part`: WAVES
// floats; the caller synchronises before it is written again.
template <typename Op, int WAVES = 4>
__device__ __forceinline__ float si_block(float v, float* part) {
    v = si_team<Op>(v, 64);
    if (((int)threadIdx.x & 63) == 0) part[(int)threadIdx.x >> 6] = v;
    __syncthreads();
    float r = part[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) r = Op::apply(r, part[w]);
    return r;
}

// ---- the register-resident row.  A ROW of cv items (channel vectors of VW elements) is spread over L lanes: the whole workgroup of
// THREADS (BLOCK), or a group of 1 << lg lanes with THREADS >> lg rows per workgroup.  Lane j keeps items j, j + L, ...: at most ITEMS
// of them, 16 floats.  The row loop, `live` (row < rows) and the exchanges between the passes are the caller's; a dead row's lanes load and
// store nothing but take part in every exchange.
constexpr int SI_ROW_LANE_ELEMS = 16;   // floats of a row that a lane keeps

// The registers of a lane, declared by the caller (Regs).  A bare array of single elements becomes ONE 16-wide value in the compiler's hands, a
// struct stays single registers: each is what the rows written out in softmax.hip and lpnorm.hip compiled to.  The other way round costs the
// vector forms up to 16 VGPRs and softmax's scalar group form a wave per SIMD (profiles/reduction_commons_be2e378.txt, 1a: hipcc of ROCm 7.2;
// tabulate again when the compiler changes).
template <int ITEMS, int VW>
struct SiRowRegs {
    float v[ITEMS][VW];
};

template <typename T, int VW, int THREADS, bool BLOCK>
struct SiRowTile {
    static constexpr int ITEMS = SI_ROW_LANE_ELEMS / VW;
    typedef typename std::conditional<VW == 1, float[ITEMS][VW], SiRowRegs<ITEMS, VW>>::type Regs;
    int L, j;              // lanes per row; this lane's index in its row
    int rows_per_block;    // rows of a workgroup
    int sub;               // this lane's row among them

    __device__ static __forceinline__ float (&items(SiRowRegs<ITEMS, VW>& regs))[ITEMS][VW] { return regs.v; }
    __device__ static __forceinline__ float (&items(float (&regs)[ITEMS][VW]))[ITEMS][VW] { return regs; }

    __device__ __forceinline__ explicit SiRowTile(int lg) {
        const int tid = (int)threadIdx.x;
        L = BLOCK ? THREADS : (1 << lg);
        j = BLOCK ? tid : (tid & (L - 1));
        rows_per_block = BLOCK ? 1 : (THREADS >> lg);
        sub = BLOCK ? 0 : (tid >> lg);
    }

    // the lane's items into its registers, the items beyond the row (and all of a dead row) zero-filled; returns the fold acc = visit(acc, x) over the
    // loaded elements in channel order
    template <typename F>
    __device__ __forceinline__ float load_row(Regs& regs, const T* in, bool live, int cv, float acc, F visit) const {
        float (&v)[ITEMS][VW] = items(regs);
#pragma unroll
        for (int i = 0; i < ITEMS; ++i) {
            const int item = i * L + j;
            if (live && item < cv) {
                si_load_vec<T, VW>(in + item * VW, v[i]);
#pragma unroll
                for (int e = 0; e < VW; ++e) acc = visit(acc, v[i][e]);
            } else {
#pragma unroll
                for (int e = 0; e < VW; ++e) v[i][e] = 0.0f;
            }
        }
        return acc;
    }

    // a second pass over the elements this lane holds, in channel order: acc = update(acc, x), which may rewrite x
    template <typename F>
    __device__ __forceinline__ float update_row(Regs& regs, bool live, int cv, float acc, F update) const {
        float (&v)[ITEMS][VW] = items(regs);
#pragma unroll
        for (int i = 0; i < ITEMS; ++i) {
            if (live && i * L + j < cv) {
#pragma unroll
                for (int e = 0; e < VW; ++e) acc = update(acc, v[i][e]);
            }
        }
        return acc;
    }

    // a live row's items out as result(x)
    template <typename F>
    __device__ __forceinline__ void store_row(Regs& regs, T* out, int cv, F result) const {
        float (&v)[ITEMS][VW] = items(regs);
#pragma unroll
        for (int i = 0; i < ITEMS; ++i) {
            const int item = i * L + j;
            if (item < cv) {
#pragma unroll
                for (int e = 0; e < VW; ++e) v[i][e] = result(v[i][e]);
                si_store_vec<T, VW>(out + item * VW, v[i]);
            }
        }
    }
};

// ---- the positions of an item, outer level first (increasing (n, h, w)).  `off` is `first` plus the distance of the current position from
// position 0, in units of `scale` per pixel (1: pixels; a pixel stride: elements); next() moves one position on.  Unsigned: the step past
// the last position may wrap, and is unused.  The loop is the caller's (for (r = start; r < end; ++r, walk.next()) ...), with its own unroll
// request: as a function taking the body, the walk cost the half-vector forms of reduce.hip a register copy per position (same file, 1b).
struct SiLevelWalk {
    unsigned off;
    __device__ __forceinline__ SiLevelWalk(const SiLevelArgs& lv, unsigned scale, unsigned first, int start) : R1(lv.R1) {
        const int r0 = start / lv.R1;
        r1 = start - r0 * lv.R1;
        off = first + (unsigned)(r0 * lv.rs0 + r1 * lv.rs1) * scale;
        step = (unsigned)lv.rs1 * scale;
        wrap = (unsigned)(lv.rs0 - lv.R1 * lv.rs1) * scale;
    }
    __device__ __forceinline__ void next() {
        off += step;
        if (++r1 == R1) {
            r1 = 0;
            off += wrap;
        }
    }

private:
    int r1, R1;
    unsigned step, wrap;
};

#endif  // SI_REDUCE_DEV_H_
