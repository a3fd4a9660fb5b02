// si_mma_dev.h -- device commons of the matrix-core operator files: the 16x16 MFMA steps (conv1d.hip, xcorr.hip, conv_border.hip, rnn.hip), the
// 64 x 64 x 32 one-stage fp32 GEMM core (conv_transpose.hip, deform_conv.hip) and the "pixel on x, four filters per lane" tile (xcorr.hip,
// conv_border.hip).  The ORDER in which products enter an accumulator is what these operators promise (the same bits twice, batch
// invariance); it is defined here, once.  The epilogues here hold adds, si_act and the store cast only -- no multiply of theirs feeds an add of
// theirs -- so a file's `#pragma clang fp contract(off)` may stand above or below its includes without changing a rounding of them.
// Included from si_hip_internal.h; a kernel file defines none of these for itself ("Device commons").  The benchmarked convolution
// and attention files keep their builtin calls: their loops were tuned instruction by instruction.
#ifndef SI_MMA_DEV_H_
#define SI_MMA_DEV_H_

// ---- 1. the 16x16 steps (operand and C/D maps: Mma<16> in si_hip_internal.h).  fp32: v_mfma_f32_16x16x4_f32, one k per lane group; fp16:
// v_mfma_f32_16x16x32_f16, eight k per lane group.
__device__ __forceinline__ f32x4 si_mma16(float a, float b, f32x4 acc) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0); }
__device__ __forceinline__ f32x4 si_mma16(f16x8 a, f16x8 b, f32x4 acc) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, acc, 0, 0, 0); }

// one channel block of 16-byte fragments into an accumulator: fp32 is four 16x16x4 steps, step j taking element j of every lane's fragment
// (channels 4 g + j, g = lane >> 4, of the block of 16); fp16 is ONE 16x16x32 step
__device__ __forceinline__ f32x4 si_mma16_block(f32x4 a, f32x4 b, f32x4 acc) {
#pragma unroll
    for (int j = 0; j < 4; ++j) acc = si_mma16(a[j], b[j], acc);
    return acc;
}
__device__ __forceinline__ f32x4 si_mma16_block(f16x8 a, f16x8 b, f32x4 acc) { return si_mma16(a, b, acc); }

// ---- 2. the 64 x 64 x 32 fp32 GEMM core (v_mfma_f32_32x32x2_f32: exact fp32, k-ordered fma chain).  Per workgroup of 256 threads: four waves
// as 2 x 2, one 32x32 accumulator per wave, one LDS stage ([row][32 + 4]: 18 KB, so many workgroups share a CU) with the next K-tile's global
// loads in flight during the MFMAs -- the form conv_igemm.hip measured fastest for the fp32 MFMA.  A and B are both [row][k]: A's rows are the
// tile's 64 GEMM rows, B's its 64 columns.  The caller produces the operands (its loader) and owns M, K and the meaning of a row.
constexpr int SI_G64_BM = 64, SI_G64_BN = 64, SI_G64_BK = 32, SI_G64_LDL = SI_G64_BK + 4;
constexpr int SI_G64_LDS_FLOATS = (SI_G64_BM + SI_G64_BN) * SI_G64_LDL;   // the LDS image the caller declares, 16-byte aligned

// tile mapping as conv_igemm.hip: the n_tiles workgroups that share one A panel get the same blockIdx % 8 (same XCD / L2).  `none`: the
// workgroup is one of the grid's round-up and has no tile.
struct SiG64Tile {
    int m_tile, n_tile;
    bool none;
};
__device__ __forceinline__ SiG64Tile si_g64_tile(int m_tiles, int n_tiles) {
    const int per_chunk = 8 * n_tiles;
    const int chunk = (int)blockIdx.x / per_chunk;
    const int r = (int)blockIdx.x - chunk * per_chunk;
    const int m_tile = chunk * 8 + (r & 7);
    return SiG64Tile{m_tile, r >> 3, m_tile >= m_tiles};
}

// A thread's places in the tile.  Staging: the 4-wide K vector kv of the 32-wide K-tile, at tile rows r0 and r0 + 32 of A and of B.
struct SiG64Stage {
    int kv, r0;
};
__device__ __forceinline__ SiG64Stage si_g64_stage(int tid) { return SiG64Stage{tid & 7, tid >> 3}; }
// MFMA: the wave's 32x32 tile (wm, wn) of the 2 x 2 and the lane's place in it; C/D map: the lane's GEMM column col(n0), its rows row0() +
// Mma<32>::row(e).
struct SiG64Lane {
    int wm, wn, l31, lh;
    __device__ __forceinline__ int col(int n0) const { return n0 + wn * 32 + l31; }   // n0: the tile's first column
    __device__ __forceinline__ int row0() const { return wm * 32 + 4 * lh; }
};
__device__ __forceinline__ SiG64Lane si_g64_lane(int tid) {
    const int wave = tid >> 6, lane = tid & 63;
    return SiG64Lane{wave >> 1, wave & 1, lane & 31, lane >> 5};
}

// The K loop stays written out in the two kernels, around their loaders: stage pa / pb at (r0 + 32 q, kv), barrier, load K-tile kt + 1, si_g64_mma,
// barrier.  As one function of this header it compiled to another schedule, and conv_transpose.hip's one-tap kernel measured 1.5 - 2 % slower on
// two shapes (LAB_NOTEBOOK.md).  si_g64_mma: the staged K-tile into the wave's accumulator.  One ds_read_b128 per lane of
// A[row][16 p + 8 h + 4 (lane >> 5) .. + 3]; MFMA j of that group takes element j from A and B alike (a K permutation inside the tile, the same products).
__device__ __forceinline__ void si_g64_mma(const float (&lds)[SI_G64_LDS_FLOATS], const SiG64Lane& ln, f32x16& acc) {
    const float* As = lds + (ln.wm * 32 + ln.l31) * SI_G64_LDL + ln.lh * 4;
    const float* Bs = lds + (SI_G64_BM + ln.wn * 32 + ln.l31) * SI_G64_LDL + ln.lh * 4;
#pragma unroll
    for (int p = 0; p < SI_G64_BK / 16; ++p) {
        f32x4 fa[2], fb[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            fa[h] = *reinterpret_cast<const f32x4*>(As + p * 16 + h * 8);
            fb[h] = *reinterpret_cast<const f32x4*>(Bs + p * 16 + h * 8);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int h = 0; h < 2; ++h) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[h][j], fb[h][j], acc, 0, 0, 0);
    }
}

// The epilogue: bias, activation, one 4-byte store per element.  Args: the caller's argument struct (bias, out, out_ld, act, act_param).
// rows[]: the output pixel of each of the workgroup's 64 rows (-1 past M); o: this lane's output channel (`live`: it exists); col_pix: a pixel
// offset that belongs to the lane's column (conv_transpose.hip's one-tap pixel shuffle; else 0).
template <int ACT, typename Args>
__device__ __forceinline__ void si_g64_store(const Args& a, const f32x16& acc, const int* rows, int row0, bool live, int o, int col_pix) {
    if (!live) return;
    const float bv = a.bias ? a.bias[o] : 0.0f;
    float* const ob = a.out + o;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int pix = rows[row0 + Mma<32>::row(e)];
        if (pix >= 0) ob[(size_t)(pix + col_pix) * a.out_ld] = si_act<ACT>(acc[e] + bv, a.act_param);
    }
}
// (a template instance per activation: the switch is resolved once per workgroup and the element loop is straight-line code)
template <typename Args>
__device__ __forceinline__ void si_g64_epilogue(const Args& a, const f32x16& acc, const int* rows, int row0, bool live, int o, int col_pix) {
    switch (a.act) {
        case SI_ACT_RELU: si_g64_store<SI_ACT_RELU>(a, acc, rows, row0, live, o, col_pix); break;
        case SI_ACT_SILU: si_g64_store<SI_ACT_SILU>(a, acc, rows, row0, live, o, col_pix); break;
        case SI_ACT_SIGMOID: si_g64_store<SI_ACT_SIGMOID>(a, acc, rows, row0, live, o, col_pix); break;
        case SI_ACT_HARDSIGMOID: si_g64_store<SI_ACT_HARDSIGMOID>(a, acc, rows, row0, live, o, col_pix); break;
        case SI_ACT_HARDSWISH: si_g64_store<SI_ACT_HARDSWISH>(a, acc, rows, row0, live, o, col_pix); break;
        case SI_ACT_LEAKYRELU: si_g64_store<SI_ACT_LEAKYRELU>(a, acc, rows, row0, live, o, col_pix); break;
        default: si_g64_store<SI_ACT_NONE>(a, acc, rows, row0, live, o, col_pix); break;
    }
}

// Host.  The weight image's channel pitch: a 4-wide K vector never straddles two taps.
inline int si_g64_pitch(int channels) { return (channels + 3) & ~3; }
inline long long si_g64_tiles(long long extent) { return (extent + SI_G64_BM - 1) / SI_G64_BM; }   // (BM == BN)
// grid.x for m_tiles x n_tiles tiles under si_g64_tile's mapping (the M tiles rounded up to the 8 XCDs), or 0 when it does not fit 31 bits
inline long long si_g64_grid_x(long long m_tiles, long long n_tiles) {
    const long long blocks = (m_tiles + 7) / 8 * 8 * n_tiles;
    return blocks >= (1LL << 31) ? 0 : blocks;
}

// ---- 3. the "pixel on x, four filters per lane" tile.  With lane = 16 g + x (g = 0..3, x = 0..15) a wave owns 16 pixels and TILES tiles of 16
// filters, one accumulator each: the A fragment of tile t is filter 16 t + x, the B fragment the lane's pixel, and the C/D map puts the PIXEL
// on x and filter 16 t + 4 g + r in register r -- a lane stores four consecutive channels of one NHWC pixel at once.

// this lane's filter of every tile, the first being `o`: its element offset into the filters (0, never dereferenced as live, beyond the oc
// filters), and the cleared accumulators.  A filter's stride is rows * pitch, multiplied in that order (o * rows is wave-uniform work plus one
// lane multiply by a scalar; rows = 1 for a stride that is one number)
template <int TILES>
__device__ __forceinline__ void si_pix16_filters(int o, int oc, int rows, int pitch, int (&wo)[TILES], bool (&wl)[TILES], f32x4 (&acc)[TILES]) {
#pragma unroll
    for (int t = 0; t < TILES; ++t) {
        wl[t] = o + 16 * t < oc;
        wo[t] = wl[t] ? (o + 16 * t) * rows * pitch : 0;
        acc[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    }
}

// A 16-byte fragment at p + off.  The load itself is unconditional -- a fragment that is not live reads element 0 of its view, which always
// exists, and is then replaced by zeros -- so that the loads of several fragments can be in flight before the first MFMA needs one.
__device__ __forceinline__ f32x4 si_frag16(const float* p, int off, bool live) {
    f32x4 v = *reinterpret_cast<const f32x4*>(p + (live ? off : 0));
    if (!live) v = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    return v;
}
__device__ __forceinline__ f16x8 si_frag16(const _Float16* p, int off, bool live) {
    f16x8 v = *reinterpret_cast<const f16x8*>(p + (live ? off : 0));
    if (!live) v = f16x8{0, 0, 0, 0, 0, 0, 0, 0};
    return v;
}

// The epilogue of a live pixel: register r of accumulator t is filter ob0 + 16 t + r (ob0: the first filter of the lane's group of four in tile 0).
// yp: the pixel's channel 0; bias: fp32 or null; y_vec: yp + a multiple of 4 takes a 4-element store.  RES: act1, then the residual (rp: the
// pixel's channel 0 of it, or null), then act2; without it act1 alone, and no code for the rest.
template <typename T, int TILES, bool RES>
__device__ __forceinline__ void si_pix16_store(T* yp, const T* rp, const float* bias, const f32x4 (&acc)[TILES], int ob0, int oc, bool y_vec, int act1,
                                               int act2, float act_param) {
#pragma unroll
    for (int t = 0; t < TILES; ++t) {
        const int ob = ob0 + 16 * t;
        if (ob >= oc) continue;
        T out[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const bool lo = ob + r < oc;
            const float bv = (bias && lo) ? bias[ob + r] : 0.0f;
            float val = si_act(act1, acc[t][r] + bv, act_param);
            if constexpr (RES) {
                if (rp) val = val + (lo ? (float)rp[ob + r] : 0.0f);
                val = si_act(act2, val, act_param);
            }
            out[r] = si_store_cast<T>(val);
        }
        if (y_vec && ob + 3 < oc) {
            typedef T V4 __attribute__((ext_vector_type(4)));
            *reinterpret_cast<V4*>(yp + ob) = V4{out[0], out[1], out[2], out[3]};
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (ob + r < oc) yp[ob + r] = out[r];
        }
    }
}

#endif  // SI_MMA_DEV_H_
