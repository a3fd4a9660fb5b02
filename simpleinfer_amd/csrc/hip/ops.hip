// ops.hip -- the HBM-bound half of the operator set: activations, add/mul with broadcast,
// batch-norm, max / adaptive-average pooling, nearest upsample, concat slice copies,
// NHWC->NCHW flatten, linear and the YOLOv5 Detect decode.
//
// All of these move bytes, not flops: channels are the fastest NHWC axis, so each lane owns a
// 16-byte channel vector (consecutive lanes -> consecutive addresses), grids are capped at ~8
// workgroups per CU and grid-stride over the rest.  Tensors carry a pixel stride (`ld`) so they
// can sit inside a wider concat buffer.  Reference routines replaced: see include/si_hip.h.
#include <hip/hip_runtime.h>

#include <cfloat>

#include "binary_plan.h"
#include "si_hip.h"
#include "si_hip_internal.h"

namespace {

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ---- activation ------------------------------------------------------------------------
template <bool VEC>
__global__ void activation_kernel(int act, float ap, const float* __restrict__ in, size_t pixels, int c, int in_ld,
                                  float* __restrict__ out, int out_ld) {
    const int cv = VEC ? c / 4 : c;
    const size_t total = pixels * (size_t)cv;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t p = i / cv;
        const int ch = (int)(i - p * cv);
        if (VEC) {
            f32x4 v = *reinterpret_cast<const f32x4*>(in + p * in_ld + ch * 4);
            v.x = si_act_exact<float>(act, v.x, ap);
            v.y = si_act_exact<float>(act, v.y, ap);
            v.z = si_act_exact<float>(act, v.z, ap);
            v.w = si_act_exact<float>(act, v.w, ap);
            *reinterpret_cast<f32x4*>(out + p * out_ld + ch * 4) = v;
        } else {
            out[p * out_ld + ch] = si_act_exact<float>(act, in[p * in_ld + ch], ap);
        }
    }
}

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
__device__ __forceinline__ f32x4 binary_apply4(int op, f32x4 x, f32x4 y) {
    if (op == 0) return x + y;
    if (op == 2) return x * y;
    if (op == 1) return x - y;
    if (op == 7) return y - x;
    f32x4 r;
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = binary_apply(op, x[i], y[i]);
    return r;
}
// (the code tables: binary_plan.h, shared with binary_const.hip)
inline bool binary_op_known(int op) { return si_binary_op_known(op); }
inline int binary_op_reversed(int op) { return si_binary_op_reversed(op); }

template <bool VEC>
__global__ void binary_same_kernel(int op, const float* __restrict__ a, int a_ld, const float* __restrict__ b,
                                   int b_ld, float* __restrict__ out, int out_ld, size_t pixels, int c) {
    const int cv = VEC ? c / 4 : c;
    const size_t total = pixels * (size_t)cv;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t p = i / cv;
        const int ch = (int)(i - p * cv);
        if (VEC) {
            const f32x4 x = *reinterpret_cast<const f32x4*>(a + p * a_ld + ch * 4);
            const f32x4 y = *reinterpret_cast<const f32x4*>(b + p * b_ld + ch * 4);
            *reinterpret_cast<f32x4*>(out + p * out_ld + ch * 4) = binary_apply4(op, x, y);
        } else {
            const float x = a[p * a_ld + ch], y = b[p * b_ld + ch];
            out[p * out_ld + ch] = binary_apply(op, x, y);
        }
    }
}

// squeeze-excite form of the broadcast: full [N,H,W,C] op per-image channel vector [N or 1,1,1,C] (MobileNet's x * se(x)):
// 16-byte vectors, no per-element index arithmetic (the general kernel below ran 16 us on these 12 MB tensors)
__global__ void binary_chan_kernel(int op, const float* __restrict__ full, int full_ld, const float* __restrict__ vec,
                                   int vec_img_stride, float* __restrict__ out, int out_ld, size_t pixels, int hw, int c) {
    const int cv = c / 4;
    const size_t total = pixels * cv;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t p = i / cv;
        const int ch = (int)(i - p * cv);
        const size_t img = p / hw;
        const f32x4 x = *reinterpret_cast<const f32x4*>(full + p * full_ld + ch * 4);
        const f32x4 y = *reinterpret_cast<const f32x4*>(vec + img * vec_img_stride + ch * 4);
        *reinterpret_cast<f32x4*>(out + p * out_ld + ch * 4) = binary_apply4(op, x, y);
    }
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
template <bool VEC>
__global__ void binary_scalar_kernel(int op, const float* __restrict__ in, int in_ld, float scalar, float* __restrict__ out, int out_ld,
                                     size_t pixels, int c) {
    const int cv = VEC ? c / 4 : c;
    const size_t total = pixels * (size_t)cv;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t p = i / cv;
        const int ch = (int)(i - p * cv);
        if (VEC) {
            const f32x4 x = *reinterpret_cast<const f32x4*>(in + p * in_ld + ch * 4);
            const f32x4 y = {scalar, scalar, scalar, scalar};
            *reinterpret_cast<f32x4*>(out + p * out_ld + ch * 4) = binary_apply4(op, x, y);
        } else {
            out[p * out_ld + ch] = binary_apply(op, in[p * in_ld + ch], scalar);
        }
    }
}

// (si_unary_apply: si_hip_internal.h -- shared with the fp16-storage form in ops_f16.hip)
template <bool VEC>
__global__ void unary_kernel(int op, const float* __restrict__ in, int in_ld, float* __restrict__ out, int out_ld, size_t pixels, int c) {
    const int cv = VEC ? c / 4 : c;
    const size_t total = pixels * (size_t)cv;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t p = i / cv;
        const int ch = (int)(i - p * cv);
        if (VEC) {
            const f32x4 x = *reinterpret_cast<const f32x4*>(in + p * in_ld + ch * 4);
            f32x4 r;
#pragma unroll
            for (int k = 0; k < 4; ++k) r[k] = si_unary_apply(op, x[k]);
            *reinterpret_cast<f32x4*>(out + p * out_ld + ch * 4) = r;
        } else {
            out[p * out_ld + ch] = si_unary_apply(op, in[p * in_ld + ch]);
        }
    }
}

// ---- batch norm -------------------------------------------------------------------------
__global__ void batchnorm_kernel(const float* __restrict__ in, size_t pixels, int c, int in_ld,
                                 const float* __restrict__ mean, const float* __restrict__ var,
                                 const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                 float* __restrict__ out, int out_ld) {
    const size_t total = pixels * (size_t)c;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t p = i / c;
        const int ch = (int)(i - p * c);
        const float inv = 1.0f / sqrtf(var[ch] + eps);
        out[p * out_ld + ch] = (in[p * in_ld + ch] - mean[ch]) * inv * gamma[ch] + beta[ch];
    }
}

// ---- max pool ---------------------------------------------------------------------------
template <bool VEC>
__global__ void maxpool_kernel(const SiPool2dDesc d, const float* __restrict__ in, float* __restrict__ out) {
    const int cv = VEC ? d.c / 4 : d.c;
    const size_t total = (size_t)d.n * d.oh * d.ow * cv;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        size_t t = i;
        const int ch = (int)(t % cv); t /= cv;
        const int x = (int)(t % d.ow); t /= d.ow;
        const int y = (int)(t % d.oh); t /= d.oh;
        const int b = (int)t;
        f32x4 m = {-FLT_MAX, -FLT_MAX, -FLT_MAX, -FLT_MAX};
        for (int ky = 0; ky < d.kh; ++ky) {
            const int yy = y * d.sh - d.pt + ky * d.dh;
            if ((unsigned)yy >= (unsigned)d.ih) continue;
            for (int kx = 0; kx < d.kw; ++kx) {
                const int xx = x * d.sw - d.pl + kx * d.dw;
                if ((unsigned)xx >= (unsigned)d.iw) continue;
                const float* p = in + ((size_t)(b * d.ih + yy) * d.iw + xx) * d.in_ld;
                if (VEC) {
                    const f32x4 v = *reinterpret_cast<const f32x4*>(p + ch * 4);
                    m.x = fmaxf(m.x, v.x); m.y = fmaxf(m.y, v.y); m.z = fmaxf(m.z, v.z); m.w = fmaxf(m.w, v.w);
                } else {
                    m.x = fmaxf(m.x, p[ch]);
                }
            }
        }
        float* o = out + ((size_t)(b * d.oh + y) * d.ow + x) * d.out_ld;
        if (VEC)
            *reinterpret_cast<f32x4*>(o + ch * 4) = m;
        else
            o[ch] = m.x;
    }
}

// ---- adaptive average pool (uniform windows) -----------------------------------------------
__global__ void avgpool_kernel(const float* __restrict__ in, int n, int ih, int iw, int c, int in_ld,
                               float* __restrict__ out, int oh, int ow, int out_ld, int kh, int kw) {
    const size_t total = (size_t)n * oh * ow * c;
    const float denom = (float)(kh * kw);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        size_t t = i;
        const int ch = (int)(t % c); t /= c;
        const int x = (int)(t % ow); t /= ow;
        const int y = (int)(t % oh); t /= oh;
        const int b = (int)t;
        float s = 0.0f;
        for (int ky = 0; ky < kh; ++ky)
            for (int kx = 0; kx < kw; ++kx)
                s += in[((size_t)(b * ih + y * kh + ky) * iw + x * kw + kx) * in_ld + ch];
        out[((size_t)(b * oh + y) * ow + x) * out_ld + ch] = s / denom;
    }
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

// ---- nearest upsample ----------------------------------------------------------------------
template <bool VEC>
__global__ void upsample_kernel(const float* __restrict__ in, int n, int ih, int iw, int c, int in_ld,
                                float inv_h, float inv_w, float* __restrict__ out, int oh, int ow, int out_ld) {
    const int cv = VEC ? c / 4 : c;
    const size_t total = (size_t)n * oh * ow * cv;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        size_t t = i;
        const int ch = (int)(t % cv); t /= cv;
        const int x = (int)(t % ow); t /= ow;
        const int y = (int)(t % oh); t /= oh;
        const int b = (int)t;
        // reference src/layer/upsample.cpp:85-92: int(float(dst) * inv), clamped to [0, in-1]
        int ys = (int)((float)y * inv_h);
        ys = max(0, min(ih - 1, ys));
        int xs = (int)((float)x * inv_w);
        xs = max(0, min(iw - 1, xs));
        const float* p = in + ((size_t)(b * ih + ys) * iw + xs) * in_ld;
        float* o = out + ((size_t)(b * oh + y) * ow + x) * out_ld;
        if (VEC)
            *reinterpret_cast<f32x4*>(o + ch * 4) = *reinterpret_cast<const f32x4*>(p + ch * 4);
        else
            o[ch] = p[ch];
    }
}

// ---- strided slice copies --------------------------------------------------------------------
template <bool VEC>
__global__ void copy_channels_kernel(const float* __restrict__ in, size_t pixels, int c, int in_ld,
                                     float* __restrict__ out, int out_ld) {
    const int cv = VEC ? c / 4 : c;
    const size_t total = pixels * (size_t)cv;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t p = i / cv;
        const int ch = (int)(i - p * cv);
        if (VEC)
            *reinterpret_cast<f32x4*>(out + p * out_ld + ch * 4) = *reinterpret_cast<const f32x4*>(in + p * in_ld + ch * 4);
        else
            out[p * out_ld + ch] = in[p * in_ld + ch];
    }
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
    hipStream_t s = (hipStream_t)stream;
    // a dense tensor is one long row: lets odd channel counts (e.g. 3) still take the 16-byte path
    if (in_ld == c && out_ld == c) {
        const size_t total = pixels * (size_t)c;
        if (total % 4 == 0 && total < 0x7fffffff && aligned16(in) && aligned16(out)) {
            hipLaunchKernelGGL(activation_kernel<true>, dim3(si_grid_for(total / 4)), dim3(256), 0, s, act, act_param,
                               in, (size_t)1, (int)total, (int)total, out, (int)total);
            return (int)hipGetLastError();
        }
    }
    const bool vec = (c % 4 == 0) && (in_ld % 4 == 0) && (out_ld % 4 == 0) && aligned16(in) && aligned16(out);
    if (vec)
        hipLaunchKernelGGL(activation_kernel<true>, dim3(si_grid_for(pixels * (c / 4))), dim3(256), 0, s, act,
                           act_param, in, pixels, c, in_ld, out, out_ld);
    else
        hipLaunchKernelGGL(activation_kernel<false>, dim3(si_grid_for(pixels * c)), dim3(256), 0, s, act, act_param,
                           in, pixels, c, in_ld, out, out_ld);
    return (int)hipGetLastError();
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
    if (same) {
        const bool vec = (c % 4 == 0) && (a_ld % 4 == 0) && (b_ld % 4 == 0) && (out_ld % 4 == 0) && aligned16(a) &&
                         aligned16(b) && aligned16(out);
        if (vec)
            hipLaunchKernelGGL(binary_same_kernel<true>, dim3(si_grid_for(pixels * (c / 4))), dim3(256), 0, s, op, a,
                               a_ld, b, b_ld, out, out_ld, pixels, c);
        else
            hipLaunchKernelGGL(binary_same_kernel<false>, dim3(si_grid_for(pixels * c)), dim3(256), 0, s, op, a, a_ld,
                               b, b_ld, out, out_ld, pixels, c);
    } else {
        // one operand is the whole tensor, the other a per-image (or global) channel vector; when the vector is `a` the
        // operator is applied operand-reversed (add and mul commute exactly)
        auto full_shape = [&](const Shape4& t) { return t.d[0] == os.d[0] && t.d[1] == os.d[1] && t.d[2] == os.d[2] && t.d[3] == os.d[3]; };
        auto chan_shape = [&](const Shape4& t) { return (t.d[0] == os.d[0] || t.d[0] == 1) && t.d[1] == 1 && t.d[2] == 1 && t.d[3] == os.d[3]; };
        const bool ab = full_shape(as) && chan_shape(bs), ba = full_shape(bs) && chan_shape(as);
        if ((ab || ba) && c % 4 == 0 && a_ld % 4 == 0 && b_ld % 4 == 0 && out_ld % 4 == 0 && aligned16(a) && aligned16(b) &&
            aligned16(out)) {
            const float* full = ab ? a : b;
            const float* vec = ab ? b : a;
            const int full_ld = ab ? a_ld : b_ld, vec_ld = ab ? b_ld : a_ld;
            const Shape4& vs = ab ? bs : as;
            hipLaunchKernelGGL(binary_chan_kernel, dim3(si_grid_for(pixels * (c / 4))), dim3(256), 0, s, ab ? op : binary_op_reversed(op),
                               full, full_ld, vec, vs.d[0] == 1 ? 0 : vec_ld, out, out_ld, pixels, os.d[1] * os.d[2], c);
        } else {
            hipLaunchKernelGGL(binary_bcast_kernel, dim3(si_grid_for(pixels * c)), dim3(256), 0, s, op, a, as, a_ld, b, bs,
                               b_ld, out, os, out_ld);
        }
    }
    return (int)hipGetLastError();
}

int si_hip_binary_scalar_f32(int op, const float* in, size_t pixels, int c, int in_ld, float scalar, float* out, int out_ld,
                             si_stream_t stream) {
    if (!in || !out || c <= 0) return SI_E_BADARG;
    if (!binary_op_known(op)) return SI_E_UNSUPPORTED;
    if (pixels == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const bool vec = (c % 4 == 0) && (in_ld % 4 == 0) && (out_ld % 4 == 0) && aligned16(in) && aligned16(out);
    if (vec)
        hipLaunchKernelGGL(binary_scalar_kernel<true>, dim3(si_grid_for(pixels * (c / 4))), dim3(256), 0, s, op, in, in_ld, scalar, out,
                           out_ld, pixels, c);
    else
        hipLaunchKernelGGL(binary_scalar_kernel<false>, dim3(si_grid_for(pixels * c)), dim3(256), 0, s, op, in, in_ld, scalar, out, out_ld,
                           pixels, c);
    return (int)hipGetLastError();
}

int si_hip_unary_f32(int op, const float* in, size_t pixels, int c, int in_ld, float* out, int out_ld, si_stream_t stream) {
    if (!in || !out || c <= 0) return SI_E_BADARG;
    if (op < 0 || op > 17) return SI_E_UNSUPPORTED;
    if (pixels == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const bool vec = (c % 4 == 0) && (in_ld % 4 == 0) && (out_ld % 4 == 0) && aligned16(in) && aligned16(out);
    if (vec)
        hipLaunchKernelGGL(unary_kernel<true>, dim3(si_grid_for(pixels * (c / 4))), dim3(256), 0, s, op, in, in_ld, out, out_ld, pixels, c);
    else
        hipLaunchKernelGGL(unary_kernel<false>, dim3(si_grid_for(pixels * c)), dim3(256), 0, s, op, in, in_ld, out, out_ld, pixels, c);
    return (int)hipGetLastError();
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
    if (!d || !in || !out || d->c <= 0 || d->oh <= 0 || d->ow <= 0) return SI_E_BADARG;
    const bool vec = (d->c % 4 == 0) && (d->in_ld % 4 == 0) && (d->out_ld % 4 == 0) && aligned16(in) && aligned16(out);
    const size_t px = (size_t)d->n * d->oh * d->ow;
    if (vec)
        hipLaunchKernelGGL(maxpool_kernel<true>, dim3(si_grid_for(px * (d->c / 4))), dim3(256), 0, (hipStream_t)stream,
                           *d, in, out);
    else
        hipLaunchKernelGGL(maxpool_kernel<false>, dim3(si_grid_for(px * d->c)), dim3(256), 0, (hipStream_t)stream, *d,
                           in, out);
    return (int)hipGetLastError();
}

int si_hip_adaptive_avgpool2d_f32(const float* in, int n, int ih, int iw, int c, int in_ld, float* out, int oh, int ow,
                                  int out_ld, si_stream_t stream) {
    if (!in || !out || oh <= 0 || ow <= 0) return SI_E_BADARG;
    if (ih % oh != 0 || iw % ow != 0) return SI_E_UNSUPPORTED;  // reference adaptive_avg_pool_2d.cpp:78-84
    if (oh == 1 && ow == 1 && n > 0 && c > 0) {
        // 8 channels x 32 pixel groups per workgroup: short per-thread sums (pixels / 32 terms) and c/8 x n workgroups.  The
        // map is small, so this is a latency problem, not a bandwidth one: 64 x 4 ran 13.8 us on MobileNet's squeeze-excite
        // blocks; same-box, MobileNetV3-Small: 69.2 k (64) / 72.8 k (16) / 73.6 k (8) img/s
        int cw = 8;
        while (cw > 1 && cw / 2 >= c) cw /= 2;
        hipLaunchKernelGGL(global_avgpool_kernel<float>, dim3((c + cw - 1) / cw, n), dim3(256), 0, (hipStream_t)stream, in,
                           ih * iw, c, in_ld, out, out_ld, cw);
        return (int)hipGetLastError();
    }
    hipLaunchKernelGGL(avgpool_kernel, dim3(si_grid_for((size_t)n * oh * ow * c)), dim3(256), 0, (hipStream_t)stream,
                       in, n, ih, iw, c, in_ld, out, oh, ow, out_ld, ih / oh, iw / ow);
    return (int)hipGetLastError();
}

int si_hip_upsample_nearest_f32(const float* in, int n, int ih, int iw, int c, int in_ld, float scale_h, float scale_w,
                                float* out, int oh, int ow, int out_ld, si_stream_t stream) {
    if (!in || !out || scale_h <= 0.f || scale_w <= 0.f) return SI_E_BADARG;
    const float inv_h = 1.0f / scale_h, inv_w = 1.0f / scale_w;
    const bool vec = (c % 4 == 0) && (in_ld % 4 == 0) && (out_ld % 4 == 0) && aligned16(in) && aligned16(out);
    const size_t px = (size_t)n * oh * ow;
    if (vec)
        hipLaunchKernelGGL(upsample_kernel<true>, dim3(si_grid_for(px * (c / 4))), dim3(256), 0, (hipStream_t)stream, in,
                           n, ih, iw, c, in_ld, inv_h, inv_w, out, oh, ow, out_ld);
    else
        hipLaunchKernelGGL(upsample_kernel<false>, dim3(si_grid_for(px * c)), dim3(256), 0, (hipStream_t)stream, in, n,
                           ih, iw, c, in_ld, inv_h, inv_w, out, oh, ow, out_ld);
    return (int)hipGetLastError();
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
    step_h = fminf(step_h, (float)ih);
    step_w = fminf(step_w, (float)iw);
    const bool vec = (c % 4 == 0) && (in_ld % 4 == 0) && (out_ld % 4 == 0) && aligned16(in) && aligned16(out);
    const size_t px = (size_t)n * oh * ow;
    if (vec)
        hipLaunchKernelGGL(upsample_kernel<true>, dim3(si_grid_for(px * (c / 4))), dim3(256), 0, (hipStream_t)stream, in,
                           n, ih, iw, c, in_ld, step_h, step_w, out, oh, ow, out_ld);
    else
        hipLaunchKernelGGL(upsample_kernel<false>, dim3(si_grid_for(px * c)), dim3(256), 0, (hipStream_t)stream, in, n,
                           ih, iw, c, in_ld, step_h, step_w, out, oh, ow, out_ld);
    return (int)hipGetLastError();
}

int si_hip_copy_channels_f32(const float* in, size_t pixels, int c, int in_ld, float* out, int out_ld,
                             si_stream_t stream) {
    if (!in || !out || c <= 0) return SI_E_BADARG;
    if (pixels == 0) return 0;
    const bool vec = (c % 4 == 0) && (in_ld % 4 == 0) && (out_ld % 4 == 0) && aligned16(in) && aligned16(out);
    if (vec)
        hipLaunchKernelGGL(copy_channels_kernel<true>, dim3(si_grid_for(pixels * (c / 4))), dim3(256), 0,
                           (hipStream_t)stream, in, pixels, c, in_ld, out, out_ld);
    else
        hipLaunchKernelGGL(copy_channels_kernel<false>, dim3(si_grid_for(pixels * c)), dim3(256), 0,
                           (hipStream_t)stream, in, pixels, c, in_ld, out, out_ld);
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
