// ops.hip -- the HBM-bound half of the operator set: activations, add/mul with broadcast,
// batch-norm, max / adaptive-average pooling, nearest upsample, concat slice copies,
// NHWC->NCHW flatten, linear and the YOLOv5 Detect decode, and the fp32 <-> fp16 conversions at the graph boundary.
// Each kernel that does arithmetic exists once, as a template over the storage type (float, or half_t with fp32 arithmetic and one
// rounding on the store: BASELINE.json configs[3]).  Pure data movement (upsample, concat slice copies, flatten of a 1x1 map) has
// no fp16 form: the host passes those tensors to the fp32 kernels as half as many 4-byte words.
//
// All of these move bytes, not flops: channels are the fastest NHWC axis, so each lane owns a
// 16-byte channel vector (consecutive lanes -> consecutive addresses), grids are capped at ~8
// workgroups per CU and grid-stride over the rest.  Tensors carry a pixel stride (`ld`) so they
// can sit inside a wider concat buffer.  Reference routines replaced: see include/si_hip.h.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <type_traits>

#include "binary_plan.h"
#include "si_hip.h"
#include "si_hip_internal.h"

namespace {

// ---- the pointwise skeleton ----------------------------------------------------------------------------------------------------
// item -> (pixel, first channel of the lane's piece): a piece is VW channels, VW = 1 or a full 16-byte vector (16 / sizeof(T)), c a
// multiple of VW.  Every grid-stride kernel over [pixels, c] below is this loop around its per-piece function f(pixel, channel).
// GRID_LANES: this lane's first item and the grid's step.  It stands in the kernel's own body: read inside a helper, blockDim loses the
// uniform-work-group form the compiler gives it in a kernel and costs a vector load per launch.
struct Lanes {
    size_t first, step;
};
#define GRID_LANES Lanes{(size_t)blockIdx.x * blockDim.x + threadIdx.x, (size_t)gridDim.x * blockDim.x}
template <int VW, typename F>
__device__ __forceinline__ void for_each_piece(Lanes lanes, size_t pixels, int c, F f) {
    const int cv = c / VW;
    const size_t total = pixels * (size_t)cv;
    for (size_t i = lanes.first; i < total; i += lanes.step) {
        const size_t p = i / cv;
        f(p, (int)(i - p * cv) * VW);
    }
}

// choose VW, size the grid, launch: what every entry does once its own argument checks have passed.  `launch(vw, grid)` gets VW as an
// integral_constant, so it can name the kernel instance.
template <typename T, typename Launch>
int launch_pieces(bool vec, size_t pixels, int c, Launch launch) {
    constexpr int full = (int)(16 / sizeof(T));
    if (vec) launch(std::integral_constant<int, full>{}, si_grid_for(pixels * (size_t)(c / full)));
    else launch(std::integral_constant<int, 1>{}, si_grid_for(pixels * (size_t)c));
    return (int)hipGetLastError();
}

// one input, one output: out[p][ch..] = op(in[p][ch..]), arithmetic in fp32, stored through si_store_cast
template <typename T, int VW, typename Op>
__global__ void pointwise_kernel(Op op, const T* __restrict__ in, size_t pixels, int c, int in_ld, T* __restrict__ out, int out_ld) {
    for_each_piece<VW>(GRID_LANES, pixels, c, [&](size_t p, int ch) {
        float v[VW];
        si_load_vec<T, VW>(in + p * in_ld + ch, v);
        op.template apply<T, VW>(v);
        si_store_vec<T, VW>(out + p * out_ld + ch, v);
    });
}
template <typename T, typename Op>
int launch_pointwise(Op op, const T* in, size_t pixels, int c, int in_ld, T* out, int out_ld, hipStream_t s) {
    return launch_pieces<T>(si_vector_width<T>(c, in_ld, out_ld, in, out) > 1, pixels, c, [&](auto vw, unsigned grid) {
        hipLaunchKernelGGL((pointwise_kernel<T, decltype(vw)::value, Op>), dim3(grid), dim3(256), 0, s, op, in, pixels, c, in_ld, out, out_ld);
    });
}

// ---- activation ------------------------------------------------------------------------
struct ActivationOp {
    int act;
    float ap;
    template <typename T, int VW>
    __device__ __forceinline__ void apply(float (&v)[VW]) const {
#pragma unroll
        for (int k = 0; k < VW; ++k) v[k] = si_act_exact<T>(act, v[k], ap);
    }
};

// ---- binary ops with tiling broadcast ------------------------------------------------------
struct Shape4 {
    int d[4];
};

// operator codes of the BinaryOp layers pnnx's expression lowering emits (reference src/pnnx/expand_expression.cpp:198-244):
// 0 add, 1 sub, 2 mul, 3 div, 6 pow, 10 atan2 and their operand-reversed forms 7 (y - x), 8 (y / x), 9 (pow(y, x)), 11.
// Division is IEEE (correctly rounded): no reciprocal approximation in a standalone arithmetic operator.
__device__ __forceinline__ float binary_apply(int op, float x, float y) {
    switch (op) {
        case 0: return x + y;
        case 1: return x - y;
        case 2: return x * y;
        case 3: return x / y;
        case 6: return powf(x, y);
        case 7: return y - x;
        case 8: return y / x;
        case 9: return powf(y, x);
        case 10: return atan2f(x, y);
        case 11: return atan2f(y, x);
        default: return x;
    }
}
// r = x (op) y on one piece; r may be x
template <typename T, int VW>
__device__ __forceinline__ void binary_apply_piece(int op, const float (&x)[VW], const float (&y)[VW], float (&r)[VW]) {
#define BINARY_EACH(expr) _Pragma("unroll") for (int k = 0; k < VW; ++k) r[k] = (expr)
    if constexpr (sizeof(T) == 2) {
        // fp16 storage: the entries serve add (0) and mul (2) only and refuse every other code
        BINARY_EACH((op == 0) ? x[k] + y[k] : x[k] * y[k]);
    } else {
        // fp32: every code of binary_plan.h; add, mul and the two subtractions are chosen once per piece, not per element
        if (op == 0) BINARY_EACH(x[k] + y[k]);
        else if (op == 2) BINARY_EACH(x[k] * y[k]);
        else if (op == 1) BINARY_EACH(x[k] - y[k]);
        else if (op == 7) BINARY_EACH(y[k] - x[k]);
        else BINARY_EACH(binary_apply(op, x[k], y[k]));
    }
#undef BINARY_EACH
}
// (the code tables: binary_plan.h, shared with binary_const.hip)
inline bool binary_op_known(int op) { return si_binary_op_known(op); }
inline int binary_op_reversed(int op) { return si_binary_op_reversed(op); }

template <typename T, int VW>
__global__ void binary_same_kernel(int op, const T* __restrict__ a, int a_ld, const T* __restrict__ b, int b_ld, T* __restrict__ out, int out_ld,
                                   size_t pixels, int c) {
    for_each_piece<VW>(GRID_LANES, pixels, c, [&](size_t p, int ch) {
        float x[VW], y[VW];
        si_load_vec<T, VW>(a + p * a_ld + ch, x);
        si_load_vec<T, VW>(b + p * b_ld + ch, y);
        binary_apply_piece<T, VW>(op, x, y, x);
        si_store_vec<T, VW>(out + p * out_ld + ch, x);
    });
}
template <typename T>
int launch_binary_same(int op, const T* a, int a_ld, const T* b, int b_ld, T* out, int out_ld, size_t pixels, int c, hipStream_t s) {
    constexpr int full = (int)(16 / sizeof(T));
    const bool vec = c % full == 0 && a_ld % full == 0 && b_ld % full == 0 && out_ld % full == 0 && si_aligned_to(a, 16) && si_aligned_to(b, 16) &&
                     si_aligned_to(out, 16);
    return launch_pieces<T>(vec, pixels, c, [&](auto vw, unsigned grid) {
        hipLaunchKernelGGL((binary_same_kernel<T, decltype(vw)::value>), dim3(grid), dim3(256), 0, s, op, a, a_ld, b, b_ld, out, out_ld, pixels, c);
    });
}

// squeeze-excite form of the broadcast: full [N,H,W,C] op per-image channel vector [N or 1,1,1,C] (MobileNet's x * se(x); BinaryOp with
// broadcast factors H, W on the second operand, reference src/layer/binary_op.cpp:52-94): 16-byte vectors only, no per-element index
// arithmetic (the general kernel below ran 16 us on these 12 MB tensors).  vec_img_stride: elements between two images' vectors, 0 for one
// vector for all.
template <typename T>
__global__ void binary_chan_kernel(int op, const T* __restrict__ full, int full_ld, const T* __restrict__ vec, int vec_img_stride,
                                   T* __restrict__ out, int out_ld, size_t pixels, size_t hw, int c) {
    constexpr int VW = (int)(16 / sizeof(T));
    for_each_piece<VW>(GRID_LANES, pixels, c, [&](size_t p, int ch) {
        const size_t img = p / hw;
        float x[VW], y[VW];
        si_load_vec<T, VW>(full + p * full_ld + ch, x);
        si_load_vec<T, VW>(vec + img * vec_img_stride + ch, y);
        binary_apply_piece<T, VW>(op, x, y, x);
        si_store_vec<T, VW>(out + p * out_ld + ch, x);
    });
}
template <typename T>
int launch_binary_chan(int op, const T* full, int full_ld, const T* vec, int vec_img_stride, T* out, int out_ld, size_t pixels, size_t hw, int c,
                       hipStream_t s) {
    hipLaunchKernelGGL(binary_chan_kernel<T>, dim3(si_grid_for(pixels * (size_t)(c / (int)(16 / sizeof(T))))), dim3(256), 0, s, op, full, full_ld, vec,
                       vec_img_stride, out, out_ld, pixels, hw, c);
    return (int)hipGetLastError();
}

__global__ void binary_bcast_kernel(int op, const float* __restrict__ a, Shape4 as, int a_ld,
                                    const float* __restrict__ b, Shape4 bs, int b_ld, float* __restrict__ out,
                                    Shape4 os, int out_ld) {
    const size_t total = (size_t)os.d[0] * os.d[1] * os.d[2] * os.d[3];
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        size_t t = i;
        const int i3 = (int)(t % os.d[3]); t /= os.d[3];
        const int i2 = (int)(t % os.d[2]); t /= os.d[2];
        const int i1 = (int)(t % os.d[1]); t /= os.d[1];
        const int i0 = (int)t;
        const size_t ap = ((size_t)(i0 % as.d[0]) * as.d[1] + (i1 % as.d[1])) * as.d[2] + (i2 % as.d[2]);
        const size_t bp = ((size_t)(i0 % bs.d[0]) * bs.d[1] + (i1 % bs.d[1])) * bs.d[2] + (i2 % bs.d[2]);
        const size_t op_ = ((size_t)i0 * os.d[1] + i1) * os.d[2] + i2;
        const float x = a[ap * a_ld + (i3 % as.d[3])];
        const float y = b[bp * b_ld + (i3 % bs.d[3])];
        out[op_ * out_ld + i3] = binary_apply(op, x, y);
    }
}

// tensor (op) scalar: the `with_scalar` BinaryOp form (params "1" = 1, "2" = value; expand_expression.cpp:206-236)
struct BinaryScalarOp {
    int op;
    float scalar;
    template <typename T, int VW>
    __device__ __forceinline__ void apply(float (&v)[VW]) const {
        float y[VW];
#pragma unroll
        for (int k = 0; k < VW; ++k) y[k] = scalar;
        binary_apply_piece<T, VW>(op, v, y, v);
    }
};

// UnaryOp (si_unary_apply: si_hip_internal.h): the fp32 function on the widened value, one rounding on the way out
struct UnaryOp {
    int op;
    template <typename T, int VW>
    __device__ __forceinline__ void apply(float (&v)[VW]) const {
#pragma unroll
        for (int k = 0; k < VW; ++k) v[k] = si_unary_apply(op, v[k]);
    }
};

// strided slice copies (and nothing else: the words pass through unchanged)
struct CopyOp {
    template <typename T, int VW>
    __device__ __forceinline__ void apply(float (&)[VW]) const {}
};

// ---- batch norm -------------------------------------------------------------------------
__global__ void batchnorm_kernel(const float* __restrict__ in, size_t pixels, int c, int in_ld,
                                 const float* __restrict__ mean, const float* __restrict__ var,
                                 const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                 float* __restrict__ out, int out_ld) {
    for_each_piece<1>(GRID_LANES, pixels, c, [&](size_t p, int ch) {
        const float inv = 1.0f / sqrtf(var[ch] + eps);
        out[p * out_ld + ch] = (in[p * in_ld + ch] - mean[ch]) * inv * gamma[ch] + beta[ch];
    });
}

// ---- max pool ---------------------------------------------------------------------------
// The floor an empty or all-smaller window gives, and the comparison: behaviour, not accidents (NaN and signed zero differ between the two).
template <typename T> struct PoolMax;
template <> struct PoolMax<float> {   // fp32: fmaxf from -FLT_MAX
    static constexpr float lowest = -FLT_MAX;
    __device__ static __forceinline__ float max(float m, float v) { return fmaxf(m, v); }
};
template <> struct PoolMax<half_t> {  // fp16: `>` from -65504 (the widened halves compare as the halves do; a window max is exact in any precision)
    static constexpr float lowest = -65504.0f;
    __device__ static __forceinline__ float max(float m, float v) { return v > m ? v : m; }
};

// output pixel p of an [n, oh, ow] map -> (image, row, column)
__device__ __forceinline__ void out_pixel(size_t p, int oh, int ow, int& b, int& y, int& x) {
    x = (int)(p % ow); p /= ow;
    y = (int)(p % oh); p /= oh;
    b = (int)p;
}

template <typename T, int VW>
__global__ void maxpool_kernel(const SiPool2dDesc d, const T* __restrict__ in, T* __restrict__ out) {
    for_each_piece<VW>(GRID_LANES, (size_t)d.n * d.oh * d.ow, d.c, [&](size_t op, int ch) {
        int b, y, x;
        out_pixel(op, d.oh, d.ow, b, y, x);
        float m[VW];
#pragma unroll
        for (int k = 0; k < VW; ++k) m[k] = PoolMax<T>::lowest;
        for (int ky = 0; ky < d.kh; ++ky) {
            const int yy = y * d.sh - d.pt + ky * d.dh;
            if ((unsigned)yy >= (unsigned)d.ih) continue;
            for (int kx = 0; kx < d.kw; ++kx) {
                const int xx = x * d.sw - d.pl + kx * d.dw;
                if ((unsigned)xx >= (unsigned)d.iw) continue;
                float v[VW];
                si_load_vec<T, VW>(in + ((size_t)(b * d.ih + yy) * d.iw + xx) * d.in_ld + ch, v);
#pragma unroll
                for (int k = 0; k < VW; ++k) m[k] = PoolMax<T>::max(m[k], v[k]);
            }
        }
        si_store_vec<T, VW, /*exact=*/true>(out + op * d.out_ld + ch, m);   // (an input value or the floor)
    });
}
template <typename T>
int launch_maxpool(const SiPool2dDesc* d, const T* in, T* out, hipStream_t s) {
    return launch_pieces<T>(si_vector_width<T>(d->c, d->in_ld, d->out_ld, in, out) > 1, (size_t)d->n * d->oh * d->ow, d->c, [&](auto vw, unsigned grid) {
        hipLaunchKernelGGL((maxpool_kernel<T, decltype(vw)::value>), dim3(grid), dim3(256), 0, s, *d, in, out);
    });
}

// ---- adaptive average pool (uniform windows) -----------------------------------------------
// single elements only; the mean is rounded with a plain cast (the sum's division is the last fp32 operation: nothing to keep apart)
template <typename T>
__global__ void avgpool_kernel(const T* __restrict__ in, int n, int ih, int iw, int c, int in_ld, T* __restrict__ out, int oh, int ow, int out_ld,
                               int kh, int kw) {
    const float denom = (float)(kh * kw);
    for_each_piece<1>(GRID_LANES, (size_t)n * oh * ow, c, [&](size_t op, int ch) {
        int b, y, x;
        out_pixel(op, oh, ow, b, y, x);
        float s = 0.0f;
        for (int ky = 0; ky < kh; ++ky)
            for (int kx = 0; kx < kw; ++kx)
                s += (float)in[((size_t)(b * ih + y * kh + ky) * iw + x * kw + kx) * in_ld + ch];
        out[op * out_ld + ch] = (T)(s / denom);
    });
}

// Global average (output 1x1, the squeeze-excite / classifier-head case): the window is the whole map, so one thread
// per output would walk thousands of strided elements alone.  Instead a workgroup owns one image and `cw` consecutive
// channels (cw = power of two <= 64): lane -> channel (coalesced rows), the 256/cw thread groups stride over the pixels,
// partial sums meet in LDS and are added in a fixed order (results do not depend on the launch shape).
template <typename T>
__global__ __launch_bounds__(256) void global_avgpool_kernel(const T* __restrict__ in, int pixels, int c, int in_ld,
                                                             T* __restrict__ out, int out_ld, int cw) {
    __shared__ float part[256];
    const int b = blockIdx.y;
    const int ch = blockIdx.x * cw + (threadIdx.x % cw);
    const int pg = threadIdx.x / cw, groups = 256 / cw;
    float s = 0.0f;
    if (ch < c) {
        const T* p = in + (size_t)b * pixels * in_ld + ch;
        for (int i = pg; i < pixels; i += groups) s += (float)p[(size_t)i * in_ld];
    }
    part[threadIdx.x] = s;
    __syncthreads();
    if (pg == 0 && ch < c) {
        float t = 0.0f;
        for (int g = 0; g < groups; ++g) t += part[g * cw + (threadIdx.x % cw)];
        out[(size_t)b * out_ld + ch] = (T)(t / (float)pixels);
    }
}

// both average pools behind the entries' own checks
template <typename T>
int launch_avgpool(const T* in, int n, int ih, int iw, int c, int in_ld, T* out, int oh, int ow, int out_ld, bool global, hipStream_t s) {
    if (global) {
        // 8 channels x 32 pixel groups per workgroup: short per-thread sums (pixels / 32 terms) and c/8 x n workgroups.  The
        // map is small, so this is a latency problem, not a bandwidth one: 64 x 4 ran 13.8 us on MobileNet's squeeze-excite
        // blocks; same-box, MobileNetV3-Small: 69.2 k (64) / 72.8 k (16) / 73.6 k (8) img/s
        int cw = 8;
        while (cw > 1 && cw / 2 >= c) cw /= 2;
        hipLaunchKernelGGL(global_avgpool_kernel<T>, dim3((c + cw - 1) / cw, n), dim3(256), 0, s, in, ih * iw, c, in_ld, out, out_ld, cw);
    } else {
        hipLaunchKernelGGL(avgpool_kernel<T>, dim3(si_grid_for((size_t)n * oh * ow * c)), dim3(256), 0, s, in, n, ih, iw, c, in_ld, out, oh, ow, out_ld,
                           ih / oh, iw / ow);
    }
    return (int)hipGetLastError();
}

// ---- nearest upsample ----------------------------------------------------------------------
template <int VW>
__global__ void upsample_kernel(const float* __restrict__ in, int n, int ih, int iw, int c, int in_ld,
                                float inv_h, float inv_w, float* __restrict__ out, int oh, int ow, int out_ld) {
    for_each_piece<VW>(GRID_LANES, (size_t)n * oh * ow, c, [&](size_t op, int ch) {
        int b, y, x;
        out_pixel(op, oh, ow, b, y, x);
        // reference src/layer/upsample.cpp:85-92: int(float(dst) * inv), clamped to [0, in-1]
        int ys = (int)((float)y * inv_h);
        ys = max(0, min(ih - 1, ys));
        int xs = (int)((float)x * inv_w);
        xs = max(0, min(iw - 1, xs));
        float v[VW];
        si_load_vec<float, VW>(in + ((size_t)(b * ih + ys) * iw + xs) * in_ld + ch, v);
        si_store_vec<float, VW>(out + op * out_ld + ch, v);
    });
}
int launch_upsample(const float* in, int n, int ih, int iw, int c, int in_ld, float inv_h, float inv_w, float* out, int oh, int ow, int out_ld,
                    hipStream_t s) {
    return launch_pieces<float>(si_vector_width<float>(c, in_ld, out_ld, in, out) > 1, (size_t)n * oh * ow, c, [&](auto vw, unsigned grid) {
        hipLaunchKernelGGL(upsample_kernel<decltype(vw)::value>, dim3(grid), dim3(256), 0, s, in, n, ih, iw, c, in_ld, inv_h, inv_w, out, oh, ow, out_ld);
    });
}

// ---- fp32 <-> fp16 at the graph boundary: single elements, a plain cast -------------------------
template <typename TI, typename TO>
__global__ void convert_kernel(const TI* __restrict__ in, size_t pixels, int c, int in_ld, TO* __restrict__ out, int out_ld) {
    for_each_piece<1>(GRID_LANES, pixels, c, [&](size_t p, int ch) { out[p * out_ld + ch] = (TO)in[p * in_ld + ch]; });
}

__global__ void cat_axis_kernel(const float* __restrict__ in, Shape4 s, float* __restrict__ out, Shape4 o, int axis,
                                int offset) {
    const size_t total = (size_t)s.d[0] * s.d[1] * s.d[2] * s.d[3];
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        size_t t = i;
        int idx[4];
        idx[3] = (int)(t % s.d[3]); t /= s.d[3];
        idx[2] = (int)(t % s.d[2]); t /= s.d[2];
        idx[1] = (int)(t % s.d[1]); t /= s.d[1];
        idx[0] = (int)t;
        idx[axis] += offset;
        out[(((size_t)idx[0] * o.d[1] + idx[1]) * o.d[2] + idx[2]) * o.d[3] + idx[3]] = in[i];
    }
}

// out is NCHW dense: consecutive threads walk w (coalesced writes); reads are strided by ld but
// the flatten inputs in these nets are tiny (ResNet18: 64x1x1x512).
__global__ void nhwc_to_nchw_kernel(const float* __restrict__ in, int n, int h, int w, int c, int in_ld,
                                    float* __restrict__ out) {
    const size_t total = (size_t)n * c * h * w;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        size_t t = i;
        const int x = (int)(t % w); t /= w;
        const int y = (int)(t % h); t /= h;
        const int ch = (int)(t % c); t /= c;
        const int b = (int)t;
        out[i] = in[((size_t)(b * h + y) * w + x) * in_ld + ch];
    }
}

// ---- linear: one wave per output element, lanes stride K (coalesced), shuffle reduce --------
__global__ void linear_kernel(const float* __restrict__ x, int n, int in_f, const float* __restrict__ w,
                              const float* __restrict__ bias, int out_f, float* __restrict__ y) {
    const int lane = threadIdx.x & 63;
    const size_t wave = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const size_t n_waves = ((size_t)gridDim.x * blockDim.x) >> 6;
    const size_t total = (size_t)n * out_f;
    for (size_t e = wave; e < total; e += n_waves) {
        const int row = (int)(e / out_f), o = (int)(e - (size_t)row * out_f);
        const float* xr = x + (size_t)row * in_f;
        const float* wr = w + (size_t)o * in_f;
        float acc = 0.0f;
        for (int k = lane; k < in_f; k += 64) acc = fmaf(xr[k], wr[k], acc);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
        if (lane == 0) y[e] = bias ? acc + bias[o] : acc;
    }
}

// ---- YOLOv5 Detect decode --------------------------------------------------------------------
__global__ void yolo_decode_kernel(const float* __restrict__ conv, int n, size_t rows, int ne,
                                   const float* __restrict__ grid, const float* __restrict__ anchor, float stride,
                                   float* __restrict__ out, int rows_total, int row_off) {
    const size_t total = (size_t)n * rows * ne;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int e = (int)(i % ne);
        const size_t t = i / ne;
        const size_t r = t % rows;
        const size_t b = t / rows;
        const float s = si_sigmoid_fast(conv[i]);
        float v = s;
        if (e < 2) {
            v = (s * 2.0f + grid[r * 2 + e]) * stride;
        } else if (e < 4) {
            const float t2 = s * 2.0f;
            v = t2 * t2 * anchor[r * 2 + (e - 2)];
        }
        out[(b * rows_total + row_off + r) * ne + e] = v;
    }
}

}  // namespace

extern "C" {

int si_hip_activation_f32(int act, float act_param, const float* in, size_t pixels, int c, int in_ld, float* out,
                          int out_ld, si_stream_t stream) {
    if (!in || !out || c <= 0 || in_ld < c || out_ld < c) return SI_E_BADARG;
    if (act < SI_ACT_NONE || act > SI_ACT_LEAKYRELU) return SI_E_UNSUPPORTED;
    if (pixels == 0) return 0;
    // a dense tensor is one long row: lets odd channel counts (e.g. 3) still take the 16-byte path (this entry only)
    if (in_ld == c && out_ld == c) {
        const size_t total = pixels * (size_t)c;
        if (total % 4 == 0 && total < 0x7fffffff && si_aligned_to(in, 16) && si_aligned_to(out, 16))
            return launch_pointwise<float>(ActivationOp{act, act_param}, in, (size_t)1, (int)total, (int)total, out, (int)total, (hipStream_t)stream);
    }
    return launch_pointwise<float>(ActivationOp{act, act_param}, in, pixels, c, in_ld, out, out_ld, (hipStream_t)stream);
}

int si_hip_activation_f16(int act, float act_param, const void* in, size_t pixels, int c, int in_ld, void* out, int out_ld,
                          si_stream_t stream) {
    if (!in || !out || c <= 0 || in_ld < c || out_ld < c) return SI_E_BADARG;
    if (act < SI_ACT_NONE || act > SI_ACT_LEAKYRELU) return SI_E_UNSUPPORTED;
    if (pixels == 0) return 0;
    return launch_pointwise<half_t>(ActivationOp{act, act_param}, static_cast<const half_t*>(in), pixels, c, in_ld, static_cast<half_t*>(out), out_ld,
                                    (hipStream_t)stream);
}

int si_hip_binary_f32(int op, const float* a, const int a_shape[4], int a_ld, const float* b, const int b_shape[4],
                      int b_ld, float* out, const int out_shape[4], int out_ld, si_stream_t stream) {
    if (!a || !b || !out || !a_shape || !b_shape || !out_shape) return SI_E_BADARG;
    if (!binary_op_known(op)) return SI_E_UNSUPPORTED;  // the reference layer itself only has add / mul (binary_op.cpp:27-30)
    bool same = true;
    Shape4 as, bs, os;
    for (int i = 0; i < 4; ++i) {
        as.d[i] = a_shape[i]; bs.d[i] = b_shape[i]; os.d[i] = out_shape[i];
        if (as.d[i] <= 0 || bs.d[i] <= 0 || os.d[i] <= 0) return SI_E_BADARG;
        if (os.d[i] % as.d[i] != 0 || os.d[i] % bs.d[i] != 0) return SI_E_BADARG;
        same = same && as.d[i] == os.d[i] && bs.d[i] == os.d[i];
    }
    hipStream_t s = (hipStream_t)stream;
    const size_t pixels = (size_t)os.d[0] * os.d[1] * os.d[2];
    const int c = os.d[3];
    if (same) return launch_binary_same<float>(op, a, a_ld, b, b_ld, out, out_ld, pixels, c, s);
    // one operand is the whole tensor, the other a per-image (or global) channel vector; when the vector is `a` the
    // operator is applied operand-reversed (add and mul commute exactly)
    auto full_shape = [&](const Shape4& t) { return t.d[0] == os.d[0] && t.d[1] == os.d[1] && t.d[2] == os.d[2] && t.d[3] == os.d[3]; };
    auto chan_shape = [&](const Shape4& t) { return (t.d[0] == os.d[0] || t.d[0] == 1) && t.d[1] == 1 && t.d[2] == 1 && t.d[3] == os.d[3]; };
    const bool ab = full_shape(as) && chan_shape(bs), ba = full_shape(bs) && chan_shape(as);
    if ((ab || ba) && c % 4 == 0 && a_ld % 4 == 0 && b_ld % 4 == 0 && out_ld % 4 == 0 && si_aligned_to(a, 16) && si_aligned_to(b, 16) &&
        si_aligned_to(out, 16)) {
        const int vec_ld = ab ? b_ld : a_ld;
        const Shape4& vs = ab ? bs : as;
        return launch_binary_chan<float>(ab ? op : binary_op_reversed(op), ab ? a : b, ab ? a_ld : b_ld, ab ? b : a, vs.d[0] == 1 ? 0 : vec_ld, out, out_ld,
                                         pixels, (size_t)(os.d[1] * os.d[2]), c, s);
    }
    hipLaunchKernelGGL(binary_bcast_kernel, dim3(si_grid_for(pixels * c)), dim3(256), 0, s, op, a, as, a_ld, b, bs, b_ld, out, os, out_ld);
    return (int)hipGetLastError();
}

int si_hip_binary_same_f16(int op, const void* a, int a_ld, const void* b, int b_ld, void* out, int out_ld, size_t pixels,
                           int c, si_stream_t stream) {
    if (!a || !b || !out || c <= 0 || a_ld < c || b_ld < c || out_ld < c) return SI_E_BADARG;
    if (op != 0 && op != 2) return SI_E_UNSUPPORTED;
    if (pixels == 0) return 0;
    return launch_binary_same<half_t>(op, static_cast<const half_t*>(a), a_ld, static_cast<const half_t*>(b), b_ld, static_cast<half_t*>(out), out_ld,
                                      pixels, c, (hipStream_t)stream);
}

// out[b][p][c] = a[b][p][c] (op) s[b][c]: the squeeze-excite scale with fp16 storage; computed in fp32, rounded once
int si_hip_binary_bcast_f16(int op, const void* a, int a_ld, const void* s, int s_ld, void* out, int out_ld, int n,
                            size_t pixels_per_image, int c, si_stream_t stream) {
    if (!a || !s || !out || c <= 0 || n < 0 || a_ld < c || s_ld < c || out_ld < c) return SI_E_BADARG;
    if (op != 0 && op != 2) return SI_E_UNSUPPORTED;
    if (n == 0 || pixels_per_image == 0) return 0;
    if (c % 8 != 0 || a_ld % 8 != 0 || s_ld % 8 != 0 || out_ld % 8 != 0 || !si_aligned_to(a, 16) || !si_aligned_to(s, 16) || !si_aligned_to(out, 16)) return SI_E_UNSUPPORTED;
    return launch_binary_chan<half_t>(op, static_cast<const half_t*>(a), a_ld, static_cast<const half_t*>(s), s_ld, static_cast<half_t*>(out), out_ld,
                                      (size_t)n * pixels_per_image, pixels_per_image, c, (hipStream_t)stream);
}

int si_hip_binary_scalar_f32(int op, const float* in, size_t pixels, int c, int in_ld, float scalar, float* out, int out_ld,
                             si_stream_t stream) {
    if (!in || !out || c <= 0) return SI_E_BADARG;
    if (!binary_op_known(op)) return SI_E_UNSUPPORTED;
    if (pixels == 0) return 0;
    return launch_pointwise<float>(BinaryScalarOp{op, scalar}, in, pixels, c, in_ld, out, out_ld, (hipStream_t)stream);
}

int si_hip_unary_f32(int op, const float* in, size_t pixels, int c, int in_ld, float* out, int out_ld, si_stream_t stream) {
    if (!in || !out || c <= 0) return SI_E_BADARG;   // (no check of ld here; the fp16 entry has one)
    if (op < 0 || op > 17) return SI_E_UNSUPPORTED;
    if (pixels == 0) return 0;
    return launch_pointwise<float>(UnaryOp{op}, in, pixels, c, in_ld, out, out_ld, (hipStream_t)stream);
}

int si_hip_unary_f16(int op, const void* in, size_t pixels, int c, int in_ld, void* out, int out_ld, si_stream_t stream) {
    if (!in || !out || c <= 0 || in_ld < c || out_ld < c) return SI_E_BADARG;
    if (op < 0 || op > 17) return SI_E_UNSUPPORTED;
    if (pixels == 0) return 0;
    return launch_pointwise<half_t>(UnaryOp{op}, static_cast<const half_t*>(in), pixels, c, in_ld, static_cast<half_t*>(out), out_ld, (hipStream_t)stream);
}

int si_hip_batchnorm2d_f32(const float* in, size_t pixels, int c, int in_ld, const float* mean, const float* var,
                           const float* gamma, const float* beta, float eps, float* out, int out_ld,
                           si_stream_t stream) {
    if (!in || !out || !mean || !var || !gamma || !beta || c <= 0) return SI_E_BADARG;
    if (pixels == 0) return 0;
    hipLaunchKernelGGL(batchnorm_kernel, dim3(si_grid_for(pixels * c)), dim3(256), 0, (hipStream_t)stream, in, pixels,
                       c, in_ld, mean, var, gamma, beta, eps, out, out_ld);
    return (int)hipGetLastError();
}

int si_hip_maxpool2d_f32(const SiPool2dDesc* d, const float* in, float* out, si_stream_t stream) {
    if (!d || !in || !out || d->c <= 0 || d->oh <= 0 || d->ow <= 0) return SI_E_BADARG;   // (the output size; the fp16 entry checks the window instead)
    return launch_maxpool<float>(d, in, out, (hipStream_t)stream);
}

int si_hip_maxpool2d_f16(const SiPool2dDesc* d, const void* in, void* out, si_stream_t stream) {
    if (!d || !in || !out || d->c <= 0 || d->in_ld < d->c || d->out_ld < d->c) return SI_E_BADARG;
    if (d->kh <= 0 || d->kw <= 0 || d->sh <= 0 || d->sw <= 0 || d->dh <= 0 || d->dw <= 0) return SI_E_BADARG;
    if ((size_t)d->n * d->oh * d->ow == 0) return 0;
    return launch_maxpool<half_t>(d, static_cast<const half_t*>(in), static_cast<half_t*>(out), (hipStream_t)stream);
}

int si_hip_adaptive_avgpool2d_f32(const float* in, int n, int ih, int iw, int c, int in_ld, float* out, int oh, int ow,
                                  int out_ld, si_stream_t stream) {
    if (!in || !out || oh <= 0 || ow <= 0) return SI_E_BADARG;
    if (ih % oh != 0 || iw % ow != 0) return SI_E_UNSUPPORTED;  // reference adaptive_avg_pool_2d.cpp:78-84
    return launch_avgpool<float>(in, n, ih, iw, c, in_ld, out, oh, ow, out_ld, oh == 1 && ow == 1 && n > 0 && c > 0, (hipStream_t)stream);
}

int si_hip_adaptive_avgpool2d_f16(const void* in, int n, int ih, int iw, int c, int in_ld, void* out, int oh, int ow,
                                  int out_ld, si_stream_t stream) {
    if (!in || !out || n <= 0 || c <= 0 || oh <= 0 || ow <= 0) return SI_E_BADARG;
    if (ih % oh != 0 || iw % ow != 0) return SI_E_UNSUPPORTED;  // uniform windows only, as the fp32 kernel
    return launch_avgpool<half_t>(static_cast<const half_t*>(in), n, ih, iw, c, in_ld, static_cast<half_t*>(out), oh, ow, out_ld, oh == 1 && ow == 1,
                                  (hipStream_t)stream);
}

int si_hip_upsample_nearest_f32(const float* in, int n, int ih, int iw, int c, int in_ld, float scale_h, float scale_w,
                                float* out, int oh, int ow, int out_ld, si_stream_t stream) {
    if (!in || !out || scale_h <= 0.f || scale_w <= 0.f) return SI_E_BADARG;
    return launch_upsample(in, n, ih, iw, c, in_ld, 1.0f / scale_h, 1.0f / scale_w, out, oh, ow, out_ld, (hipStream_t)stream);
}

int si_hip_upsample_nearest_steps_f32(const float* in, int n, int ih, int iw, int c, int in_ld, float step_h, float step_w,
                                      float* out, int oh, int ow, int out_ld, si_stream_t stream) {
    if (!in || !out || n <= 0 || ih <= 0 || iw <= 0 || c <= 0 || oh <= 0 || ow <= 0 || in_ld < c || out_ld < c) return SI_E_BADARG;
    if (!(step_h >= 0.f) || !(step_w >= 0.f) || step_h > FLT_MAX || step_w > FLT_MAX) return SI_E_BADARG;
    // as the bilinear entries: element offsets must fit 31 bits (the kernel indexes pixels in int).  A step beyond the source
    // extent only ever clamps, so it is cut there; then dst * step < out * in, which must stay inside int before the clamp
    if ((unsigned long long)n * ih * iw * (unsigned long long)in_ld > 0x7fffffffull ||
        (unsigned long long)n * oh * ow * (unsigned long long)out_ld > 0x7fffffffull ||
        (unsigned long long)oh * ih > 0x7fffffffull || (unsigned long long)ow * iw > 0x7fffffffull)
        return SI_E_UNSUPPORTED;
    return launch_upsample(in, n, ih, iw, c, in_ld, fminf(step_h, (float)ih), fminf(step_w, (float)iw), out, oh, ow, out_ld, (hipStream_t)stream);
}

int si_hip_copy_channels_f32(const float* in, size_t pixels, int c, int in_ld, float* out, int out_ld,
                             si_stream_t stream) {
    if (!in || !out || c <= 0) return SI_E_BADARG;
    if (pixels == 0) return 0;
    return launch_pointwise<float>(CopyOp{}, in, pixels, c, in_ld, out, out_ld, (hipStream_t)stream);
}

int si_hip_convert_f32_f16(const float* in, size_t pixels, int c, int in_ld, void* out, int out_ld, si_stream_t stream) {
    if (!in || !out || c <= 0 || in_ld < c || out_ld < c) return SI_E_BADARG;
    if (pixels == 0) return 0;
    hipLaunchKernelGGL((convert_kernel<float, half_t>), dim3(si_grid_for(pixels * (size_t)c)), dim3(256), 0, (hipStream_t)stream, in, pixels, c, in_ld,
                       static_cast<half_t*>(out), out_ld);
    return (int)hipGetLastError();
}

int si_hip_convert_f16_f32(const void* in, size_t pixels, int c, int in_ld, float* out, int out_ld, si_stream_t stream) {
    if (!in || !out || c <= 0 || in_ld < c || out_ld < c) return SI_E_BADARG;
    if (pixels == 0) return 0;
    hipLaunchKernelGGL((convert_kernel<half_t, float>), dim3(si_grid_for(pixels * (size_t)c)), dim3(256), 0, (hipStream_t)stream,
                       static_cast<const half_t*>(in), pixels, c, in_ld, out, out_ld);
    return (int)hipGetLastError();
}

int si_hip_cat_axis_f32(const float* in, const int in_shape[4], float* out, const int out_shape[4], int axis,
                        int offset, si_stream_t stream) {
    if (!in || !out || axis < 0 || axis > 3) return SI_E_BADARG;
    Shape4 s, o;
    size_t total = 1;
    for (int i = 0; i < 4; ++i) {
        s.d[i] = in_shape[i]; o.d[i] = out_shape[i];
        total *= (size_t)s.d[i];
    }
    if (total == 0) return 0;
    hipLaunchKernelGGL(cat_axis_kernel, dim3(si_grid_for(total)), dim3(256), 0, (hipStream_t)stream, in, s, out, o, axis,
                       offset);
    return (int)hipGetLastError();
}

int si_hip_nhwc_to_nchw_f32(const float* in, int n, int h, int w, int c, int in_ld, float* out, si_stream_t stream) {
    if (!in || !out) return SI_E_BADARG;
    hipLaunchKernelGGL(nhwc_to_nchw_kernel, dim3(si_grid_for((size_t)n * h * w * c)), dim3(256), 0, (hipStream_t)stream,
                       in, n, h, w, c, in_ld, out);
    return (int)hipGetLastError();
}

int si_hip_linear_f32(const float* x, int n, int in_features, const float* w, const float* bias, int out_features,
                      float* y, si_stream_t stream) {
    if (!x || !w || !y || n <= 0 || in_features <= 0 || out_features <= 0) return SI_E_BADARG;
    const size_t waves = (size_t)n * out_features;
    hipLaunchKernelGGL(linear_kernel, dim3(si_grid_for(waves * 64)), dim3(256), 0, (hipStream_t)stream, x, n,
                       in_features, w, bias, out_features, y);
    return (int)hipGetLastError();
}

int si_hip_yolo_decode_f32(const float* conv, int n, int h, int w, int na, int ne, const float* grid_hwa2,
                           const float* anchor_hwa2, float stride, float* out, int rows_total, int row_off,
                           si_stream_t stream) {
    if (!conv || !grid_hwa2 || !anchor_hwa2 || !out || ne < 4) return SI_E_BADARG;
    const size_t rows = (size_t)h * w * na;
    hipLaunchKernelGGL(yolo_decode_kernel, dim3(si_grid_for((size_t)n * rows * ne)), dim3(256), 0, (hipStream_t)stream,
                       conv, n, rows, ne, grid_hwa2, anchor_hwa2, stride, out, rows_total, row_off);
    return (int)hipGetLastError();
}

}  // extern "C"
