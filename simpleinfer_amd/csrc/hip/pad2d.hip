// pad2d.hip -- the explicit 2-D pads (include/si_pad.h): nn.ReflectionPad2d / ReplicationPad2d / ZeroPad2d / ConstantPad2d /
// CircularPad2d and F.pad on NHWC fp32 and fp16 tensors with pixel strides on both sides.  Pure data movement: values travel as
// integer words, the constant as the bits the host made of it; nothing here does arithmetic on a value.
//
// Work unit: PAD_ROWS consecutive output rows of one image x 256 consecutive items of the row, an item being one channel
// vector of one output pixel (16 bytes, or one element in the scalar form).  Consecutive lanes take consecutive channel
// vectors of a pixel, then consecutive pixels: a wave reads and writes whole runs of the row.  blockIdx = (items of the row,
// row group, image).  A lane maps its column once (one 32-bit division, item -> pixel, and the mode's index rule) and keeps it for
// all its rows; a row's source is the same in every lane (scalar).  The loads of the PAD_ROWS rows are issued before the first
// store.  Element offsets are 32-bit: the host refuses tensors whose offsets do not fit 31 bits.
//
// Register table per instantiation: DESIGN.md section 9d.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "si_hip_internal.h"
#include "si_pad.h"

namespace {

constexpr int PAD_THREADS = 256;
constexpr int PAD_ROWS = 4;

// the integer word a <T, VW> item travels as
template <typename T, int VW> struct PadWord { typedef u32x4 type; };
template <> struct PadWord<float, 1> { typedef uint32_t type; };
template <> struct PadWord<_Float16, 1> { typedef uint16_t type; };

struct PadArgs {
    const void* in;
    void* out;
    int ih, iw, oh, ow;
    int cv;          // items per pixel
    int in_ld, out_ld;
    int pad_l, pad_t, mode;
    int row_items;   // ow * cv
    unsigned fill;   // the constant as 32 bits (fp16: the half twice)
};

// source index of i = o - pad on an axis of `size`; -1: the constant.  The host has checked the mode's limits, under which one
// reflection / one wrap lands inside; the final clamp costs two instructions per lane and axis and keeps every read inside whatever happens.
__device__ __forceinline__ int pad_src(int i, int size, int mode) {
    if (mode == SI_PAD_CONSTANT) return (unsigned)i < (unsigned)size ? i : -1;
    if (mode == SI_PAD_REFLECT) {
        i = i < 0 ? -i : i;
        i = i > size - 1 ? 2 * (size - 1) - i : i;
    } else if (mode == SI_PAD_CIRCULAR) {
        i = i < 0 ? i + size : i;
        i = i >= size ? i - size : i;
    }
    return min(max(i, 0), size - 1);
}

template <typename W>
__device__ __forceinline__ W pad_fill(unsigned bits) {
    if constexpr (sizeof(W) == 16) {
        return W{bits, bits, bits, bits};
    } else {
        return (W)bits;
    }
}

template <typename T, int VW>
__global__ __launch_bounds__(PAD_THREADS) void pad2d_kernel(PadArgs a) {
    typedef typename PadWord<T, VW>::type W;
    const int item = (int)blockIdx.x * PAD_THREADS + (int)threadIdx.x;
    if (item >= a.row_items) return;
    const int ox = item / a.cv;
    const int v = item - ox * a.cv;
    const int sx = pad_src(ox - a.pad_l, a.iw, a.mode);
    const int img = (int)blockIdx.z;
    const T* const in = static_cast<const T*>(a.in) + v * VW;
    T* const out = static_cast<T*>(a.out) + ox * a.out_ld + v * VW;
    const W fill = pad_fill<W>(a.fill);
    for (int oy0 = (int)blockIdx.y * PAD_ROWS; oy0 < a.oh; oy0 += (int)gridDim.y * PAD_ROWS) {
        W val[PAD_ROWS];
#pragma unroll
        for (int r = 0; r < PAD_ROWS; ++r) {
            const int oy = oy0 + r;
            const int sy = oy < a.oh ? pad_src(oy - a.pad_t, a.ih, a.mode) : -1;
            val[r] = fill;
            if (sy >= 0 && sx >= 0) val[r] = *reinterpret_cast<const W*>(in + ((img * a.ih + sy) * a.iw + sx) * a.in_ld);
        }
#pragma unroll
        for (int r = 0; r < PAD_ROWS; ++r) {
            const int oy = oy0 + r;
            if (oy < a.oh) *reinterpret_cast<W*>(out + (img * a.oh + oy) * a.ow * a.out_ld) = val[r];
        }
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------
// everything that can be decided without a device: SI_E_BADARG / SI_E_UNSUPPORTED / 0
int check_desc(const SiPad2dDesc* d) {
    if (!d) return SI_E_BADARG;
    if (d->n <= 0 || d->ih <= 0 || d->iw <= 0 || d->c <= 0 || d->oh <= 0 || d->ow <= 0) return SI_E_BADARG;
    if (d->in_ld < d->c || d->out_ld < d->c) return SI_E_BADARG;
    if (d->mode < SI_PAD_CONSTANT || d->mode > SI_PAD_CIRCULAR) return SI_E_BADARG;
    const int64_t pl = d->pad_l, pr = d->pad_r, pt = d->pad_t, pb = d->pad_b;
    if ((int64_t)d->ih + pt + pb != (int64_t)d->oh || (int64_t)d->iw + pl + pr != (int64_t)d->ow) return SI_E_BADARG;
    // a crop leaves at least one row and one column
    if ((int64_t)d->iw + (pl < 0 ? pl : 0) + (pr < 0 ? pr : 0) < 1 || (int64_t)d->ih + (pt < 0 ? pt : 0) + (pb < 0 ? pb : 0) < 1) return SI_E_UNSUPPORTED;
    const int64_t mw = pl > pr ? pl : pr, mh = pt > pb ? pt : pb;
    if (d->mode == SI_PAD_REFLECT && (mw >= d->iw || mh >= d->ih)) return SI_E_UNSUPPORTED;
    if (d->mode == SI_PAD_CIRCULAR && (pl < 0 || pr < 0 || pt < 0 || pb < 0 || mw > d->iw || mh > d->ih)) return SI_E_UNSUPPORTED;
    if (d->n > 65535) return SI_E_UNSUPPORTED;
    const uint64_t in_rows = (uint64_t)d->n * d->ih, out_rows = (uint64_t)d->n * d->oh;   // < 2^47
    if (in_rows > SI_INDEX_LIMIT || out_rows > SI_INDEX_LIMIT) return SI_E_UNSUPPORTED;
    const uint64_t in_pix = in_rows * d->iw, out_pix = out_rows * d->ow;                    // < 2^62
    if (in_pix > SI_INDEX_LIMIT || out_pix > SI_INDEX_LIMIT) return SI_E_UNSUPPORTED;
    if (in_pix * (uint64_t)d->in_ld > SI_INDEX_LIMIT || out_pix * (uint64_t)d->out_ld > SI_INDEX_LIMIT) return SI_E_UNSUPPORTED;
    return 0;
}

template <typename T>
int vector_width(const SiPad2dDesc* d, const void* in, const void* out) { return si_vector_width<T>(d->c, d->in_ld, d->out_ld, in, out); }

template <typename T, int VW>
int launch(const SiPad2dDesc* d, const T* in, T* out, unsigned fill, hipStream_t stream) {
    PadArgs a;
    a.in = in;
    a.out = out;
    a.ih = d->ih; a.iw = d->iw; a.oh = d->oh; a.ow = d->ow;
    a.cv = d->c / VW;
    a.in_ld = d->in_ld;
    a.out_ld = d->out_ld;
    a.pad_l = d->pad_l;
    a.pad_t = d->pad_t;
    a.mode = d->mode;
    a.row_items = d->ow * a.cv;
    a.fill = fill;
    unsigned groups = ((unsigned)d->oh + PAD_ROWS - 1) / PAD_ROWS;
    if (groups > 65535u) groups = 65535u;
    const dim3 grid(((unsigned)a.row_items + PAD_THREADS - 1) / PAD_THREADS, groups, (unsigned)d->n);
    hipLaunchKernelGGL((pad2d_kernel<T, VW>), grid, dim3(PAD_THREADS), 0, stream, a);
    return (int)hipGetLastError();
}

template <typename T>
int run(const SiPad2dDesc* d, const T* in, T* out, si_stream_t stream) {
    const int rc = check_desc(d);
    if (rc != 0) return rc;
    if (!in || !out) return SI_E_BADARG;
    unsigned fill;
    if constexpr (sizeof(T) == 4) {
        fill = __builtin_bit_cast(unsigned, d->value);
    } else {
        const unsigned h = __builtin_bit_cast(unsigned short, (_Float16)d->value);   // round to nearest even, once
        fill = h | (h << 16);
    }
    hipStream_t s = (hipStream_t)stream;
    constexpr int full = (int)(16 / sizeof(T));
    return vector_width<T>(d, in, out) == full ? launch<T, full>(d, in, out, fill, s) : launch<T, 1>(d, in, out, fill, s);
}

}  // namespace

extern "C" {

int si_hip_pad2d_f32(const SiPad2dDesc* d, const float* in, float* out, si_stream_t stream) { return run<float>(d, in, out, stream); }

int si_hip_pad2d_f16(const SiPad2dDesc* d, const void* in, void* out, si_stream_t stream) {
    return run<_Float16>(d, static_cast<const _Float16*>(in), static_cast<_Float16*>(out), stream);
}

const char* si_hip_pad2d_kernel_name(const SiPad2dDesc* d, const void* in, const void* out, int half) {
    if (check_desc(d) != 0) return "none";
    if (half) return vector_width<_Float16>(d, in, out) > 1 ? "pad2d_kernel<_Float16, 8>" : "pad2d_kernel<_Float16, 1>";
    return vector_width<float>(d, in, out) > 1 ? "pad2d_kernel<float, 4>" : "pad2d_kernel<float, 1>";
}

}  // extern "C"
