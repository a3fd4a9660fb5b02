// si_hip_internal.h -- shared helpers for the HIP translation units (not part of the C-ABI).
#ifndef SI_HIP_INTERNAL_H_
#define SI_HIP_INTERNAL_H_

#include <hip/hip_runtime.h>

#include <map>
#include <mutex>
#include <utility>

#include "si_hip.h"
#include "si_magic.h"
#include "si_views.h"

// ---- device commons: what every kernel file shares.  A kernel file defines no activation formula, no division helper (si_magic.h), no
// vector typedef, no buffer flag, no channel-vector load/store, and no alignment, extent or overlap helper (si_views.h) of its own
// ("Device commons").

// Vector types, under the names the kernels use
typedef _Float16 half_t;
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
template <typename T, int N> using si_vec = T __attribute__((ext_vector_type(N)));   // for a width that is a template parameter

// Environment switches (ablations, sweeps) exist in the EXPERIMENT build of the library only (-DSI_EXPERIMENT: tools/hip_variant.sh,
// simpleinfer_amd/build.py build_hip(defines=...)); in the product build the expression is its default and nothing reads the environment
// (round 6).  Choices a caller may legitimately make per call travel in SiConv2dDesc::plan (include/si_hip.h).
#ifdef SI_EXPERIMENT
#include <cstdlib>
#define SI_ENV_INT(name, dflt) ([] { const char* e_ = getenv(name); return e_ ? atoi(e_) : (dflt); }())
#else
#define SI_ENV_INT(name, dflt) (dflt)
#endif

#define SI_HIP_TRY(expr)                      \
    do {                                      \
        hipError_t _e = (expr);               \
        if (_e != hipSuccess) return (int)_e; \
    } while (0)

// memory-bound kernels: cap the grid at ~8 workgroups per CU and grid-stride the rest
// (2048 x 256 = 524288 items per pass: tests/test_gpu_elementwise_edges.py test_grid_stride_* make every capped launch go round three times)
static inline unsigned si_grid_for(size_t work_items, unsigned block = 256) {
    size_t blocks = (work_items + block - 1) / block;
    const size_t cap = 256u * 8u;
    if (blocks > cap) blocks = cap;
    if (blocks == 0) blocks = 1;
    return (unsigned)blocks;
}

// Workgroups of `kern` that are resident per CU at this block size and dynamic-LDS size: the grid of a persistent kernel
// (a workgroup that has to wait for a slot starts its share of the work when the others are finishing theirs).  Cached
// per (kernel, LDS size); engines may launch from several host threads, hence the lock.
template <typename Kern>
static inline int si_resident_blocks(Kern kern, int threads, size_t lds) {
    static std::mutex mu;
    static std::map<std::pair<const void*, size_t>, int> cache;
    const std::pair<const void*, size_t> key(reinterpret_cast<const void*>(kern), lds);
    std::lock_guard<std::mutex> lock(mu);
    auto it = cache.find(key);
    if (it != cache.end()) return it->second;
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kern, threads, lds) != hipSuccess || nb < 1) nb = 1;
    cache[key] = nb;
    return nb;
}

// Dynamic LDS above the 64 KB default needs the per-function opt-in once (not again during a stream capture).
template <typename Kern>
static inline hipError_t si_allow_dynamic_lds(Kern kern, size_t lds) {
    if (lds <= 64 * 1024) return hipSuccess;
    static std::mutex mu;
    static std::map<const void*, size_t> allowed;
    std::lock_guard<std::mutex> lock(mu);
    size_t& have = allowed[reinterpret_cast<const void*>(kern)];
    if (have >= lds) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e == hipSuccess) have = lds;
    return e;
}

// (the host-side preamble of the descriptor operators -- alignment, vector width, extents, overlap: si_views.h)

// fp32 -> storage type. For _Float16 the empty asm keeps the value opaque so the compiler cannot fold the multiply / add
// that produced it into v_fma_mix{lo,hi}_f16 for some unrolled elements and not others: the fused form rounds once, the
// separate form twice, and an image's result would then depend on which accumulator slot (= batch position) it used.
template <typename T>
__device__ __forceinline__ T si_store_cast(float v) {
    if constexpr (sizeof(T) == 2) asm("" : "+v"(v));
    return (T)v;
}

// One lane's piece of a pixel's channels as fp32: VW = 1 is a single element, otherwise a full 16-byte vector (f32x4 or f16x8) at a
// 16-byte aligned address.  The store rounds through si_store_cast; EXACT marks values that are already exactly representable in T and
// stores them with a plain cast, without the barrier (binary_const.hip: it rounds once per stage, before the store).
template <typename T, int VW>
__device__ __forceinline__ void si_load_vec(const T* p, float (&v)[VW]) {
    static_assert(VW == 1 || VW == (int)(16 / sizeof(T)), "a single element or a full 16-byte vector");
    if constexpr (VW == 1) {
        v[0] = (float)*p;
    } else if constexpr (sizeof(T) == 4) {
        const f32x4 r = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = r[i];
    } else {
        const f16x8 r = *reinterpret_cast<const f16x8*>(p);
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = (float)r[i];
    }
}

template <typename T, int VW, bool EXACT = false>
__device__ __forceinline__ void si_store_vec(T* p, const float (&v)[VW]) {
    static_assert(VW == 1 || VW == (int)(16 / sizeof(T)), "a single element or a full 16-byte vector");
    if constexpr (VW == 1) {
        if constexpr (EXACT) *p = (T)v[0];
        else *p = si_store_cast<T>(v[0]);
    } else if constexpr (sizeof(T) == 4) {
        f32x4 r;
#pragma unroll
        for (int i = 0; i < 4; ++i) r[i] = v[i];
        *reinterpret_cast<f32x4*>(p) = r;
    } else {
        f16x8 r;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if constexpr (EXACT) r[i] = (_Float16)v[i];
            else r[i] = si_store_cast<_Float16>(v[i]);
        }
        *reinterpret_cast<f16x8*>(p) = r;
    }
}

// Lanes 2k and 2k+1 of a 32x32 MFMA C/D tile hold neighbouring channels of the same pixels.  The pair trades one value
// each (DPP quad_perm [1,0,3,2]) so that every lane stores ONE dword -- two channels of one pixel -- instead of two 2-byte
// values: half the store instructions for fp16 activations.  v0 / v1: this lane's channel at two pixels; afterwards the
// even lane owns the first pixel and the odd lane the second.  Returns {channel 2k, channel 2k+1} as packed halves.
__device__ __forceinline__ unsigned si_pair_halves(float v0, float v1, bool odd) {
    const float send = odd ? v0 : v1;
    const float recv = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, send), 0xB1, 0xF, 0xF, true));
    f16x2 p;
    p[0] = si_store_cast<_Float16>(odd ? recv : v0);
    p[1] = si_store_cast<_Float16>(odd ? v1 : recv);
    return __builtin_bit_cast(unsigned, p);
}

// ---- activations.  Two families with different rules for special values and rounding; neither is a slip of the other.
//   * Fused epilogues (si_act): the value is a convolution's or a normalisation's accumulator on its way to the store.  ReLU and the two
//     clamps are plain fmaxf / fminf (v_max_f32 / v_min_f32 return the OTHER operand for a NaN), so ReLU and the hard sigmoid turn a NaN into 0;
//     it passes through the others (hard swish multiplies that 0 by the NaN again).  Leaky ReLU is the fp32 product v * p; under fp16 storage the store rounds it a second
//     time.
//   * Stand-alone operators (si_act_exact<T>, T the storage type): a NaN passes through every activation, as in torch, and under fp16
//     storage the leaky product is rounded to odd so that the store's rounding is the only one (mul_round_odd).
// Both use the fast sigmoid.  v_rcp_f32 / v_exp_f32 are accurate to 1 ulp: SiLU and sigmoid are within ~2e-7 relative of the exact
// value, three orders inside the parity bar, at 5 instructions instead of the 15 of an IEEE division.
// The formulas take the floating-point contraction of the file that includes them: a kernel file whose `#pragma clang fp contract(off)`
// stands above this header's include computes the hard sigmoid's v * (1/6) + 0.5 as a multiply and an add, every other file as one fma.
__device__ __forceinline__ float si_sigmoid_fast(float v) { return __builtin_amdgcn_rcpf(1.0f + __expf(-v)); }
__device__ __forceinline__ float si_silu_fast(float v) { return v * si_sigmoid_fast(v); }

// compile-time form: the activation of a template instance
template <int ACT>
__device__ __forceinline__ float si_act(float v, float p) {
    if (ACT == SI_ACT_RELU) return fmaxf(v, 0.0f);
    if (ACT == SI_ACT_SILU) return si_silu_fast(v);
    if (ACT == SI_ACT_SIGMOID) return si_sigmoid_fast(v);
    if (ACT == SI_ACT_HARDSIGMOID) return fminf(fmaxf(v * (1.0f / 6.0f) + 0.5f, 0.0f), 1.0f);
    if (ACT == SI_ACT_HARDSWISH) return v * fminf(fmaxf(v * (1.0f / 6.0f) + 0.5f, 0.0f), 1.0f);
    if (ACT == SI_ACT_LEAKYRELU) return v > 0.0f ? v : v * p;
    return v;
}
// run-time form: the same formulas behind a switch that a kernel resolves once per workgroup, not per element
__device__ __forceinline__ float si_act(int act, float v, float p) {
    switch (act) {
        case SI_ACT_RELU: return si_act<SI_ACT_RELU>(v, p);
        case SI_ACT_SILU: return si_act<SI_ACT_SILU>(v, p);
        case SI_ACT_SIGMOID: return si_act<SI_ACT_SIGMOID>(v, p);
        case SI_ACT_HARDSIGMOID: return si_act<SI_ACT_HARDSIGMOID>(v, p);
        case SI_ACT_HARDSWISH: return si_act<SI_ACT_HARDSWISH>(v, p);
        case SI_ACT_LEAKYRELU: return si_act<SI_ACT_LEAKYRELU>(v, p);
        default: return v;
    }
}

// The stand-alone activation operator passes a NaN on, as torch does: fmaxf / fminf alone (v_max_f32 / v_min_f32) return the OTHER operand for
// a NaN, which turned relu(NaN) and hardsigmoid(NaN) into 0.  Every other input keeps the bits fmaxf / fminf gave it.
__device__ __forceinline__ float act_relu(float v) { return v != v ? v : fmaxf(v, 0.0f); }
__device__ __forceinline__ float act_clamp01(float t) { return t != t ? t : fminf(fmaxf(t, 0.0f), 1.0f); }
// v * p rounded to odd.  The slope is an fp32 value, so the product of a widened half and the slope has up to 35 significant bits: rounded to
// fp32's 24 and then to fp16's 11 it can differ from the product rounded once (it lands on an fp16 tie that the exact product only came
// near: 103 of the 65536 inputs at slope 0.1).  Rounding the fp32 product to odd keeps a sticky last bit, and the store's round-to-nearest-even
// then gives the exact product rounded once.  fmaf returns the rounding error of `hi` exactly.
__device__ __forceinline__ float mul_round_odd(float v, float p) {
    const float hi = v * p;
    const float lo = fmaf(v, p, -hi);
    unsigned u = __builtin_bit_cast(unsigned, hi);
    if (lo != 0.0f && !(u & 1u) && fabsf(hi) < __builtin_inff()) u += ((lo < 0.0f) == (hi < 0.0f)) ? 1u : ~0u;
    return __builtin_bit_cast(float, u);
}
// T: the storage type the result is rounded to (as for si_store_cast)
template <typename T>
__device__ __forceinline__ float si_act_exact(int act, float v, float p) {
    switch (act) {
        case SI_ACT_RELU: return act_relu(v);
        case SI_ACT_SILU: return si_silu_fast(v);
        case SI_ACT_SIGMOID: return si_sigmoid_fast(v);
        case SI_ACT_HARDSIGMOID: return act_clamp01(v * (1.0f / 6.0f) + 0.5f);
        case SI_ACT_HARDSWISH: return v * act_clamp01(v * (1.0f / 6.0f) + 0.5f);
        case SI_ACT_LEAKYRELU:
            if constexpr (sizeof(T) == 2) return v > 0.0f ? v : mul_round_odd(v, p);
            else return v > 0.0f ? v : v * p;
        default: return v;
    }
}

// ---- buffer views: raw buffer loads and stores check the byte offset against `bytes` in hardware; a load beyond it returns zeros and a
// store beyond it is dropped, so an out-of-image tap or a row past M needs no branch, only one of the two offsets below.
// The flag word is dword 3 of the gfx9 buffer descriptor: DATA_FORMAT = BUF_DATA_FORMAT_32 (value 4 in bits 15..18) and every other
// field zero -- no index stride, no swizzle, no add-tid; the raw instructions carry their own width and ignore the destination selects.
template <typename T>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t si_buffer(const T* p, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(p), 0, bytes, 0x00020000);
}
constexpr unsigned SI_OOB = 0xFFFFFF00u;       // >= any legal num_records
constexpr unsigned SI_OOB_HALF = 0x80000000u;  // for a view below 2 GB (weights): + kt*128 cannot wrap

// The two fp32 MFMA tiles the kernels use.  Both round like ONE sequential fma chain over k (tools/mfma_chain_test.hip, measured:
// v_mfma_f32_32x32x2_f32, v_mfma_f32_16x16x4_f32 and a scalar fmaf loop agree bit for bit), so a kernel on 16x16 tiles that feeds
// k in the same order as one on 32x32 tiles produces the same bits per output element -- the tile policy may follow the batch
// size without breaking the engine's batch-invariance contract.
//   32x32x2: A/B operand of lane l = row (l & 31), k = l >> 5;   C/D: col = l & 31, row = (e&3) + 8*(e>>2) + 4*(l>>5), 16 registers
//   16x16x4: A/B operand of lane l = row (l & 15), k = l >> 4;   C/D: col = l & 15, row = e + 4*(l>>4),             4 registers
// The fp16 instructions with a 32x32 fp32 result (v_mfma_f32_32x32x16_f16) have the same C/D map.
// SI_MMA32_ROW: the 32x32 row map as an expression, for a site where the compiler treats the inlined call unlike the written-out sum
// (conv_stem_s2c32_f16.hip, phase A's patch rows: two LDS stores split base and offset another way).  Same value; use Mma<32>::row.
#define SI_MMA32_ROW(e) ((e & 3) + 8 * (e >> 2))
template <int MT> struct Mma;
template <> struct Mma<32> {
    typedef f32x16 acc_t;
    static constexpr int NE = 16;
    __device__ static __forceinline__ constexpr int row(int e) { return SI_MMA32_ROW(e); }
};
template <> struct Mma<16> {
    typedef f32x4 acc_t;
    static constexpr int NE = 4;
    __device__ static __forceinline__ constexpr int row(int e) { return e; }
};

// UnaryOp codes of expand_expression.cpp:146-165 (ncnn's numbering): 0 abs 1 neg 2 floor 3 ceil 4 square 5 sqrt 6 rsqrt 7 exp
// 8 log 9 sin 10 cos 11 tan 12 asin 13 acos 14 atan 15 reciprocal 16 tanh 17 log10.  Library-accurate functions, IEEE sqrt and
// division: this is a standalone arithmetic operator, not a fused epilogue.
__device__ __forceinline__ float si_unary_apply(int op, float x) {
    switch (op) {
        case 0: return fabsf(x);
        case 1: return -x;
        case 2: return floorf(x);
        case 3: return ceilf(x);
        case 4: return x * x;
        case 5: return sqrtf(x);
        case 6: return 1.0f / sqrtf(x);
        case 7: return expf(x);
        case 8: return logf(x);
        case 9: return sinf(x);
        case 10: return cosf(x);
        case 11: return tanf(x);
        case 12: return asinf(x);
        case 13: return acosf(x);
        case 14: return atanf(x);
        case 15: return 1.0f / x;
        case 16: return tanhf(x);
        case 17: return log10f(x);
        default: return x;
    }
}

// YOLOv5 Detect decode of one workgroup's conv tile, straight-line form for a tile that lies inside ONE image and below M
// (reference src/layer/yolo_detect.cpp:223-266: sigmoid, xy = (2s + grid) * stride, wh = (2s)^2 * anchor, rows
// [img][row_off + pix*na + anchor][ne]).  Per lane (= output channel) the element kind, the grid / anchor pointer and
// the output pointer are fixed before the 16-element loop; per element: sigmoid and one store, for the waves that hold box
// columns also one masked 4-byte load and a bit-select.  Args: the conv kernels' argument structs (ocg, bias, yna, yne, ohow, ygrid,
// yanchor, ystride, yrows_total, yrow_off).  C/D map of the 32x32 MFMA tile as everywhere: col = lane&31 (channel),
// row = (e&3) + 8*(e>>2) + 4*(lane>>5) (pixel).
// MT: the MFMA tile the accumulators come from -- 32 (16 registers, rows (e&3) + 8*(e>>2)) or 16 (v_mfma_f32_16x16x4_f32: 4
// registers, rows e; col = lane&15, + 4*(lane>>4) already in mrow0)
template <int TM, int TN, typename Args, int MT = 32, typename AccT = f32x16>
__device__ __forceinline__ void si_yolo_tile_one_image(const Args& a, float* out, AccT (&acc)[TM][TN], int mrow0, int ocol0, int img) {
#pragma clang fp contract(off)
    const int per_pix = a.yna * a.yne;
#pragma unroll
    for (int u = 0; u < TN; ++u) {
        const int o = ocol0 + u * MT;
        const bool live = o < a.ocg;
        const int oo = live ? o : 0;
        const float bv = a.bias ? a.bias[oo] : 0.0f;
        const int anc = oo / a.yne;
        const int e_ = oo - anc * a.yne;
        const bool is_xy = e_ < 2, is_box = e_ < 4;
        const float* const auxp = (is_xy ? a.ygrid + e_ : a.yanchor + (is_box ? e_ - 2 : 0)) + anc * 2;
        // a wave whose columns hold no box entry (x, y, w, h of an anchor: 12 of 255 columns, in three of eight 32-column blocks)
        // never sees the box arithmetic (wave-uniform branch)
        const bool any_box = __builtin_amdgcn_ballot_w64(is_box && live) != 0ull;
        const unsigned mxy = is_xy ? ~0u : 0u, mwh = (is_box && !is_xy) ? ~0u : 0u, msg = is_box ? 0u : ~0u;
#pragma unroll
        for (int t = 0; t < TM; ++t) {
            const int pix0 = mrow0 + t * MT - img * a.ohow;
            float* const op = out + ((size_t)img * a.yrows_total + a.yrow_off) * a.yne + (size_t)pix0 * per_pix + oo;
            constexpr int NE = MT == 32 ? 16 : 4;
            // the sigmoid for every element, nothing else (round 5: the select chain below used to sit in this loop, and hipcc turned
            // it into two exec-masked branches per element plus one around every store: ~25 instructions per element)
            float v[NE];
#pragma unroll
            for (int e = 0; e < NE; ++e) v[e] = si_sigmoid_fast(acc[t][u][e] + bv);
            if (any_box) {
                const float* const ap = auxp + (size_t)pix0 * a.yna * 2;
                // the box lanes' grid / anchor values, ALL requested before the first one is used: with the load inside the element
                // loop hipcc waits for each one in turn (16 L2 round trips per 32x32 block on the waves that own a box column)
                float auxv[NE];
#pragma unroll
                for (int e = 0; e < NE; ++e) auxv[e] = 0.0f;
                if (is_box) {
#pragma unroll
                    for (int e = 0; e < NE; ++e) auxv[e] = ap[Mma<MT>::row(e) * a.yna * 2];
                }
#pragma unroll
                for (int e = 0; e < NE; ++e) {
                    const float t2 = v[e] * 2.0f;
                    const float xy = (t2 + auxv[e]) * a.ystride;
                    const float wh = t2 * t2 * auxv[e];
                    // (the same three values as `is_xy ? xy : (is_box ? wh : sg)`, selected by bit masks: no branches)
                    v[e] = __builtin_bit_cast(float, (__builtin_bit_cast(unsigned, xy) & mxy) | (__builtin_bit_cast(unsigned, wh) & mwh) |
                                                         (__builtin_bit_cast(unsigned, v[e]) & msg));
                }
            }
            if (live) {
#pragma unroll
                for (int e = 0; e < NE; ++e) op[Mma<MT>::row(e) * per_pix] = v[e];
            }
        }
    }
}

// ---- reductions: combine operations, lane butterfly, workgroup combine, row tile, position walk (device), and the host plan they go with
#include "si_reduce_dev.h"
static_assert(SI_PLAN_BADARG == SI_E_BADARG && SI_PLAN_UNSUPPORTED == SI_E_UNSUPPORTED, "si_reduce_plan.h returns the C-ABI's codes");

// ---- diagnostic build only (-DSI_DIAG_STAMPS; tools/conv_diag.py): per-workgroup s_memtime / s_memrealtime stamps at the phase
// boundaries of a kernel, written to a __device__ array of their own that nothing else reads.  In the product build no stamp
// executes and every macro expands to nothing.  Slots: [0] realtime at start, [1..5] cycle stamps, [6] realtime at end, [7] hw id.
#ifdef SI_DIAG_STAMPS
#define SI_STAMP_ARRAY(name) __device__ unsigned long long name[65536 * 8]
#define SI_STAMP_DECL unsigned long long st_[8] = {0, 0, 0, 0, 0, 0, 0, 0}
#define SI_STAMP(i) st_[i] = __builtin_amdgcn_s_memtime()
#define SI_STAMP_RT(i) st_[i] = __builtin_amdgcn_s_memrealtime()
#define SI_STAMP_FLUSH(name)                                                                                    \
    if (threadIdx.x == 0 && blockIdx.y == 0 && blockIdx.x < 65536) {                                            \
        unsigned hw_, xcc_;                                                                                     \
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw_));                                       \
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc_));                                     \
        st_[7] = ((unsigned long long)xcc_ << 32) | hw_;                                                        \
        for (int i_ = 0; i_ < 8; ++i_) name[(size_t)blockIdx.x * 8 + i_] = st_[i_];                             \
    }
#define SI_STAMP_ACCESSORS(name, read_fn, clear_fn)                                                                              \
    extern "C" int read_fn(unsigned long long* host, size_t count) {                                                             \
        return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(name), count * sizeof(unsigned long long), 0, hipMemcpyDeviceToHost);   \
    }                                                                                                                            \
    extern "C" int clear_fn(void) {                                                                                              \
        void* p_ = nullptr;                                                                                                      \
        hipError_t e_ = hipGetSymbolAddress(&p_, HIP_SYMBOL(name));                                                              \
        if (e_ != hipSuccess) return (int)e_;                                                                                    \
        return (int)hipMemset(p_, 0, sizeof(unsigned long long) * 65536 * 8);                                                    \
    }
#else
#define SI_STAMP_ARRAY(name) static_assert(true, "")
#define SI_STAMP_DECL
#define SI_STAMP(i)
#define SI_STAMP_RT(i)
#define SI_STAMP_FLUSH(name)
#endif

#endif  // SI_HIP_INTERNAL_H_
