// detect_masks.hip -- instance masks from the payload the detection post-processing carries (include/si_detect.h): ultralytics' process_mask
// without the upsample.  mask[b][d][r][c] = crop(box of d, r, c) && dot(coefficients of d, prototypes of (r, c)) > 0, the dot accumulated in index
// order with every product and every sum rounded on its own, so that numpy restates it bit for bit (tests/detect_reference.py masks_ref).
// Shapes, forms and refusals: detect_plan.h.
//
// A workgroup owns a tile of consecutive pixels of one image, one pixel per lane, and loops over that image's detections: the prototypes of the
// tile are read once (into registers when nm == 32, into LDS otherwise) and the coefficients and the box of a detection are the same for every
// lane.  The kernel is bound by its count * mh * mw bytes of stores once the crop has skipped the dots outside the boxes, which is why the
// matrix cores (whose accumulation order would give up the bit rule) have nothing to add.
#include "si_hip.h"
#include "si_detect.h"
#include "si_hip_internal.h"
#include "detect_plan.h"

#pragma clang fp contract(off)

namespace {

namespace plan = si_detect_plan;

struct MaskArgs {
    const float* protos;
    const float* extras;
    const float* net_boxes;
    const int* counts;
    unsigned char* masks;
    int mh, mw, nm, proto_ld, max_det, extra, coef_off;
    float ratio_w, ratio_h;
    int word_stores;
};

constexpr int MASK_T_REG = 256;   // pixels of a tile, register form
constexpr int MASK_T_LDS = 128;   // ... LDS form: 128 rows of at most 65 floats

// NM == 32: the lane's 32 prototypes live in registers.  NM == 0: a.nm prototypes per pixel in LDS, row stride nm | 1 (odd: the lanes of a wave,
// one row each, meet distinct banks).
template <int NM>
__global__ __launch_bounds__(NM ? MASK_T_REG : MASK_T_LDS) void detect_masks_kernel(const MaskArgs a) {
    constexpr int T = NM ? MASK_T_REG : MASK_T_LDS;
    extern __shared__ float tile[];
    const int b = blockIdx.y;
    const int pixels = a.mh * a.mw;
    const int p0 = blockIdx.x * T;
    const int pix = p0 + (int)threadIdx.x;
    const bool inside = pix < pixels;
    const int count = min(a.counts[b], a.max_det);
    if (count <= 0) return;   // (uniform over the workgroup)
    const float* img = a.protos + (size_t)b * (size_t)pixels * (size_t)a.proto_ld;

    float p[NM ? NM : 1];
    const int stride = a.nm | 1;
    if (NM) {
        if (inside) {
            const float4* src = reinterpret_cast<const float4*>(img + (size_t)pix * a.proto_ld);
#pragma unroll
            for (int q = 0; q < NM / 4; ++q) {
                const float4 v = src[q];
                p[4 * q] = v.x; p[4 * q + 1] = v.y; p[4 * q + 2] = v.z; p[4 * q + 3] = v.w;
            }
        } else {
#pragma unroll
            for (int k = 0; k < NM; ++k) p[k] = 0.0f;
        }
    } else {
        const int npix = min(T, pixels - p0);
        const int total = npix * a.nm;
        for (int i = threadIdx.x; i < total; i += T) {
            const int q = i / a.nm, k = i - q * a.nm;
            tile[q * stride + k] = img[(size_t)(p0 + q) * a.proto_ld + k];
        }
        __syncthreads();
    }

    const int r = inside ? pix / a.mw : 0;
    const float fr = (float)r, fc = (float)(inside ? pix - r * a.mw : 0);
    const int lane = threadIdx.x & 63;
    const size_t plane = (size_t)pixels;
    for (int d = 0; d < count; ++d) {
        const size_t det = (size_t)b * a.max_det + d;
        const float* box = a.net_boxes + det * 4;
        const float* coef = a.extras + det * (size_t)a.extra + a.coef_off;
        const float bx = box[0], by = box[1], bw = box[2], bh = box[3];
        const float x1 = bx * a.ratio_w, x2 = (bx + bw) * a.ratio_w;
        const float y1 = by * a.ratio_h, y2 = (by + bh) * a.ratio_h;
        const bool crop = inside && fc >= x1 && fc < x2 && fr >= y1 && fr < y2;
        unsigned bit = 0;
        if (__any(crop)) {   // wave-uniform: the dot is formed only by waves with a pixel inside the box
            float acc = 0.0f;
            if (NM) {
#pragma unroll
                for (int k = 0; k < NM; ++k) acc = __fadd_rn(acc, __fmul_rn(coef[k], p[k]));
            } else {
                const float* row = tile + threadIdx.x * stride;
                for (int k = 0; k < a.nm; ++k) acc = __fadd_rn(acc, __fmul_rn(coef[k], row[k]));
            }
            bit = (crop && acc > 0.0f) ? 1u : 0u;
        }
        unsigned char* out = a.masks + det * plane;
        if (a.word_stores) {
            // four neighbouring lanes' bytes in one store (pixels and planes are multiples of four, so a group is wholly inside or outside)
            unsigned w = bit;
            w |= (unsigned)__shfl(bit, lane + 1) << 8;
            w |= (unsigned)__shfl(bit, lane + 2) << 16;
            w |= (unsigned)__shfl(bit, lane + 3) << 24;
            if (inside && (lane & 3) == 0) *reinterpret_cast<unsigned*>(out + pix) = w;
        } else if (inside) {
            out[pix] = (unsigned char)bit;
        }
    }
}

plan::MaskShape mask_shape(const SiDetectMaskDesc* d) {
    plan::MaskShape v;
    v.n = d->n; v.mh = d->mh; v.mw = d->mw; v.nm = d->nm; v.proto_ld = d->proto_ld; v.max_det = d->max_det; v.extra = d->extra; v.coef_off = d->coef_off;
    return v;
}

}  // namespace

extern "C" {

const char* si_hip_detect_masks_kernel_name(const SiDetectMaskDesc* d, const void* protos) {
    if (!d || !protos || !si_aligned_to(protos, 4)) return "none";
    switch (plan::MaskFormOf(mask_shape(d), si_aligned_to(protos, 16))) {
        case plan::kMaskRegisters: return "detect_masks_kernel<32>";
        case plan::kMaskGeneric: return "detect_masks_kernel<0>";
        default: return "none";
    }
}

int si_hip_detect_masks_f32(const SiDetectMaskDesc* d, const float* protos, const float* extras, const float* net_boxes, const int* counts,
                            unsigned char* masks, si_stream_t stream) {
    if (!d || !protos || !extras || !net_boxes || !counts || !masks) return SI_E_BADARG;
    if (!si_aligned_to(protos, 4) || !si_aligned_to(extras, 4) || !si_aligned_to(net_boxes, 4) || !si_aligned_to(counts, 4)) return SI_E_BADARG;
    const plan::MaskShape v = mask_shape(d);
    const int rc = plan::MaskStatusOf(v);
    if (rc != plan::kOk) return rc == plan::kBadArg ? SI_E_BADARG : SI_E_UNSUPPORTED;
    if (d->max_det == 0) return 0;
    const plan::MaskForm form = plan::MaskFormOf(v, si_aligned_to(protos, 16));
    MaskArgs a{protos, extras, net_boxes, counts, masks, d->mh, d->mw, d->nm, d->proto_ld, d->max_det, d->extra, d->coef_off,
               d->ratio_w, d->ratio_h, plan::MaskWordStores(v, si_aligned_to(masks, 4)) ? 1 : 0};
    const int pixels = d->mh * d->mw;
    hipStream_t s = (hipStream_t)stream;
    if (form == plan::kMaskRegisters) {
        hipLaunchKernelGGL(detect_masks_kernel<32>, dim3((pixels + MASK_T_REG - 1) / MASK_T_REG, d->n), dim3(MASK_T_REG), 0, s, a);
    } else {
        const size_t lds = (size_t)MASK_T_LDS * (size_t)(d->nm | 1) * sizeof(float);
        hipLaunchKernelGGL(detect_masks_kernel<0>, dim3((pixels + MASK_T_LDS - 1) / MASK_T_LDS, d->n), dim3(MASK_T_LDS), lds, s, a);
    }
    return (int)hipGetLastError();
}

}  // extern "C"
