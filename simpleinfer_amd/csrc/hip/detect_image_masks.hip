// detect_image_masks.hip -- instance masks at image size (include/si_imgmask.h): coefficients x prototypes, the bilinear upsample to the network
// or the source frame, crop and threshold in one kernel.  The low-resolution logits are never stored: they live in LDS, memory sees one read of
// the prototypes and one store of the final bytes.  Shapes, the tile, the LDS budget, the arm rule and the refusals: imgmask_plan.h.
//
// A workgroup owns one 128 x 8 tile of the output of one image, a lane 4 consecutive bytes of a row (32 lanes store a whole 128-byte line), and
// loops over that image's live detections.  The output has (OW / mw)^2 times the pixels of the prototypes, so a lane that evaluated its four
// taps itself would do 4 nm multiply-adds per byte, 64 times the necessary work at x4; the shared arm forms a logit once per prototype pixel:
//   once       the tile's prototype footprint [pixels][nm] goes into LDS, rows padded to the odd stride nm | 1
//   per box    1. wave-uniform: does the box (under crop-first, the footprint) meet the tile?  If not the tile is stored as zeros, no arithmetic.
//              2. lane f forms the dot of footprint pixel f (f += 256 for larger footprints) in index order and writes it to a logit tile.
//                 Its reads are LDS words f * stride + k: stride is odd, and multiplying by an odd number permutes the residues of 32 and of
//                 64, so the lanes of a pass meet distinct banks for every k.  The coefficients are the same for every lane (scalar loads).
//              3. ONE barrier, then every lane blends four taps per output pixel from the logit tile (neighbouring lanes read neighbouring or
//                 equal words: broadcasts, no conflicts to speak of), crops, thresholds and stores.
//   The logit tile is double-buffered: the tile written for box d + 1 is not the one lanes may still be blending box d from, and the barrier
//   of box d + 1 separates the blend of box d from the writes of box d + 2.  Boxes that miss the tile take no barrier and no buffer.
// The direct arm is the same rule with every lane forming the dots of its own taps from global memory; it serves footprints the LDS budget does
// not hold or that share nothing (down-scaling), and a tile of the shared kernel whose own geometry breaks the rule.  Same bits.
// The matrix cores are deliberately not used: their accumulation order would give up the bit rule (include/si_imgmask.h).
#include "si_hip.h"
#include "si_imgmask.h"
#include "si_hip_internal.h"
#include "imgmask_plan.h"

// every product and every sum below is an operation of its own
#pragma clang fp contract(off)

namespace {

namespace plan = si_imgmask_plan;

struct ImgMaskArgs {
    const float* protos;
    const float* extras;
    const float* boxes;
    const int* counts;
    const int* geom;
    unsigned char* masks;
    int mh, mw, nm, proto_ld, max_det, extra, coef_off, oh, ow, box_ld, crop;
    int tiles_x, capacity, word_stores, vector_loads;
};

struct Tap {
    int i0, i1;
    float l0, l1;
};

// taps and weights of destination index d of an axis with `in` source pixels: upsample_bilinear.hip's rule for align_corners = false
__device__ __forceinline__ Tap tap_of(int d, int in, float step) {
    const float src = fmaxf(0.0f, __fmaf_rn(step, __fadd_rn((float)d, 0.5f), -0.5f));
    Tap t;
    t.i0 = min((int)src, in - 1);
    t.i1 = t.i0 + (t.i0 < in - 1 ? 1 : 0);
    t.l1 = __fsub_rn(src, (float)t.i0);
    t.l0 = __fsub_rn(1.0f, t.l1);
    return t;
}

// the blend of upsample_bilinear.hip with each of its three fused operations written as a product and a sum
__device__ __forceinline__ float blend(float v00, float v01, float v10, float v11, float l0w, float l1w, float l0h, float l1h) {
    const float top = __fadd_rn(__fmul_rn(l0w, v00), __fmul_rn(l1w, v01));
    const float bot = __fadd_rn(__fmul_rn(l0w, v10), __fmul_rn(l1w, v11));
    return __fadd_rn(__fmul_rn(l0h, top), __fmul_rn(l1h, bot));
}

struct Box {
    float x1, x2, y1, y2;
};

// the crop test of detect_masks; a NaN edge passes nowhere
__device__ __forceinline__ bool pass(const Box& q, int r, int c) {
    const float fr = (float)r, fc = (float)c;
    return fc >= q.x1 && fc < q.x2 && fr >= q.y1 && fr < q.y2;
}

// (((0 + c0 p0) + c1 p1) + ...): p in LDS or in global memory, coef the same address for every lane
__device__ __forceinline__ float dot_of(const float* __restrict__ coef, const float* __restrict__ p, int nm) {
    float acc = 0.0f;
    for (int k = 0; k < nm; ++k) acc = __fadd_rn(acc, __fmul_rn(coef[k], p[k]));
    return acc;
}

// a lane's four bytes of one plane: packed when every row starts on a 4-byte boundary (a group is then wholly inside or outside the row)
__device__ __forceinline__ void store_four(unsigned char* plane, unsigned off, int x, int ow, bool row_in, bool words, unsigned bits) {
    if (!row_in) return;
    if (words) {
        if (x < ow) *reinterpret_cast<unsigned*>(plane + off) = bits;
    } else {
#pragma unroll
        for (int j = 0; j < plan::kLaneBytes; ++j)
            if (x + j < ow) plane[off + j] = (unsigned char)((bits >> (8 * j)) & 0xffu);
    }
}

// grid: (tiles of a plane, images); block 256.  SHARED: the launch carries plan::LdsBytes of dynamic LDS.
template <bool SHARED>
__global__ __launch_bounds__(plan::kThreads) void detect_image_masks_kernel(const ImgMaskArgs a) {
    extern __shared__ float lds[];
    const int b = blockIdx.y;
    const int count = min(a.counts[b], a.max_det);
    if (count <= 0) return;   // (uniform over the workgroup)
    const int tile_y = (int)(blockIdx.x / (unsigned)a.tiles_x), tile_x = (int)(blockIdx.x - (unsigned)tile_y * (unsigned)a.tiles_x);
    const int tx0 = tile_x * plan::kTileW, ty0 = tile_y * plan::kTileH;
    const int x = tx0 + plan::kLaneBytes * (int)(threadIdx.x & 31u), y = ty0 + (int)(threadIdx.x >> 5);
    const bool row_in = y < a.oh;
    const bool words = a.word_stores != 0;
    const unsigned plane = (unsigned)a.oh * (unsigned)a.ow;             // < 2^31 (imgmask_plan.h)
    const unsigned off = (unsigned)y * (unsigned)a.ow + (unsigned)x;    // used only where row_in and x < ow: inside the plane
    unsigned char* const out0 = a.masks + (size_t)b * (size_t)a.max_det * (size_t)plane;

    const int* const g = a.geom + (size_t)b * 6;
    const int wx0 = g[0], wy0 = g[1], ww = g[2], wh = g[3], out_w = g[4], out_h = g[5];
    // the record cannot be checked on the host: a window that leaves the plane or an output that leaves OH x OW writes zeros and reads nothing
    const bool geom_ok = wx0 >= 0 && wy0 >= 0 && ww > 0 && wh > 0 && (long long)wx0 + ww <= a.mw && (long long)wy0 + wh <= a.mh && out_w > 0 &&
                         out_h > 0 && out_w <= a.ow && out_h <= a.oh;
    if (!geom_ok || tx0 >= out_w || ty0 >= out_h) {   // (uniform) nothing of this tile is inside the image's output
        for (int d = 0; d < count; ++d) store_four(out0 + (size_t)d * plane, off, x, a.ow, row_in, words, 0u);
        return;
    }

    // the lane's taps, the same for every detection; a pixel outside out_h x out_w borrows the last live one's taps and stores 0
    const float step_w = __fdiv_rn((float)ww, (float)out_w), step_h = __fdiv_rn((float)wh, (float)out_h);
    const int lx1 = min(tx0 + plan::kTileW, out_w), ly1 = min(ty0 + plan::kTileH, out_h);   // one past the tile's live pixels
    Tap tw[plan::kLaneBytes];
    bool alive[plan::kLaneBytes];
    const bool row_alive = y < out_h;
#pragma unroll
    for (int j = 0; j < plan::kLaneBytes; ++j) {
        alive[j] = row_alive && x + j < out_w;
        tw[j] = tap_of(min(x + j, out_w - 1), ww, step_w);
    }
    const Tap th = tap_of(min(y, out_h - 1), wh, step_h);
    // the footprint: taps are monotonic in the destination index, so the first live pixel's i0 and the last one's i1 bound every lane's taps
    const int fx0 = tap_of(tx0, ww, step_w).i0, fx1 = tap_of(lx1 - 1, ww, step_w).i1;
    const int fy0 = tap_of(ty0, wh, step_h).i0, fy1 = tap_of(ly1 - 1, wh, step_h).i1;
    const int fw = fx1 - fx0 + 1, fh = fy1 - fy0 + 1;
    const int foot = fw * fh;                                        // <= mh * mw < 2^31
    const bool first = a.crop == plan::kCropFirst;
    const float* const img = a.protos + (size_t)b * (size_t)a.mh * (size_t)a.mw * (size_t)a.proto_ld;
    const unsigned origin = ((unsigned)(wy0 + fy0) * (unsigned)a.mw + (unsigned)(wx0 + fx0));   // prototype pixel of footprint pixel 0
    const bool shares = SHARED && plan::TileShares(foot, (lx1 - tx0) * (ly1 - ty0), a.capacity);   // (uniform)

    const int stride = plan::RowStride(a.nm);
    float* const staged = lds;                                        // [capacity][stride]
    float* const logits = lds + (size_t)a.capacity * stride;          // [2][capacity]
    if (SHARED && shares) {
        if (a.vector_loads) {
            const int nq = a.nm / 4, total = foot * nq;               // foot <= capacity <= 48 KB / 12: no overflow
            for (int i = threadIdx.x; i < total; i += plan::kThreads) {
                const int f = i / nq, q = i - f * nq, fr = f / fw, fc = f - fr * fw;
                const float4 v = *reinterpret_cast<const float4*>(img + (origin + (unsigned)fr * a.mw + fc) * (unsigned)a.proto_ld + 4 * q);
                float* dst = staged + f * stride + 4 * q;
                dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w;
            }
        } else {
            const int total = foot * a.nm;
            for (int i = threadIdx.x; i < total; i += plan::kThreads) {
                const int f = i / a.nm, k = i - f * a.nm, fr = f / fw, fc = f - fr * fw;
                staged[f * stride + k] = img[(origin + (unsigned)fr * a.mw + fc) * (unsigned)a.proto_ld + k];
            }
        }
        __syncthreads();
    }
    // the lane's taps as offsets into a logit tile
    const int r0 = (th.i0 - fy0) * fw, r1 = (th.i1 - fy0) * fw;
    int buf = 0;

    for (int d = 0; d < count; ++d) {
        const size_t det = (size_t)b * a.max_det + d;
        const float* const row = a.boxes + det * (size_t)a.box_ld;
        const float* const coef = a.extras + det * (size_t)a.extra + a.coef_off;
        const float bx = row[0], by = row[1], bw = row[2], bh = row[3];
        const Box q{bx, __fadd_rn(bx, bw), by, __fadd_rn(by, bh)};
        unsigned char* const out = out0 + (size_t)d * plane;
        // (uniform) no pixel of the tile -- under crop-first no pixel of the footprint -- can pass: zeros, no arithmetic
        const bool meets = first ? ((float)fx1 >= q.x1 && (float)fx0 < q.x2 && (float)fy1 >= q.y1 && (float)fy0 < q.y2)
                                 : ((float)(lx1 - 1) >= q.x1 && (float)tx0 < q.x2 && (float)(ly1 - 1) >= q.y1 && (float)ty0 < q.y2);
        if (!meets) {
            store_four(out, off, x, a.ow, row_in, words, 0u);
            continue;
        }
        unsigned bits = 0;
        if (SHARED && shares) {
            float* const tile = logits + (size_t)buf * a.capacity;
            buf ^= 1;
            for (int f = threadIdx.x; f < foot; f += plan::kThreads) {
                const int fr = f / fw, fc = f - fr * fw;
                tile[f] = (!first || pass(q, fy0 + fr, fx0 + fc)) ? dot_of(coef, staged + f * stride, a.nm) : 0.0f;
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < plan::kLaneBytes; ++j) {
                if (!alive[j] || !(first || pass(q, y, x + j))) continue;
                const int c0 = tw[j].i0 - fx0, c1 = tw[j].i1 - fx0;
                const float v = blend(tile[r0 + c0], tile[r0 + c1], tile[r1 + c0], tile[r1 + c1], tw[j].l0, tw[j].l1, th.l0, th.l1);
                bits |= (v > 0.0f ? 1u : 0u) << (8 * j);
            }
        } else {
#pragma unroll
            for (int j = 0; j < plan::kLaneBytes; ++j) {
                if (!alive[j] || !(first || pass(q, y, x + j))) continue;
                float v[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int iy = (t & 2) ? th.i1 : th.i0, ix = (t & 1) ? tw[j].i1 : tw[j].i0;
                    const unsigned pix = (unsigned)(wy0 + iy) * (unsigned)a.mw + (unsigned)(wx0 + ix);
                    v[t] = (!first || pass(q, iy, ix)) ? dot_of(coef, img + pix * (unsigned)a.proto_ld, a.nm) : 0.0f;
                }
                const float r = blend(v[0], v[1], v[2], v[3], tw[j].l0, tw[j].l1, th.l0, th.l1);
                bits |= (r > 0.0f ? 1u : 0u) << (8 * j);
            }
        }
        store_four(out, off, x, a.ow, row_in, words, bits);
    }
}

plan::Shape shape_of(const SiImageMaskDesc* d) {
    plan::Shape v;
    v.n = d->n; v.mh = d->mh; v.mw = d->mw; v.nm = d->nm; v.proto_ld = d->proto_ld; v.max_det = d->max_det; v.extra = d->extra;
    v.coef_off = d->coef_off; v.oh = d->oh; v.ow = d->ow; v.box_ld = d->box_ld; v.crop = d->crop; v.flags = d->flags;
    return v;
}

}  // namespace

extern "C" {

const char* si_hip_detect_image_masks_kernel_name(const SiImageMaskDesc* d, const void* protos, const void* masks) {
    if (!d || !protos || !masks || !si_aligned_to(protos, 4)) return "none";
    switch (plan::ArmOf(shape_of(d))) {
        case plan::kShared: return "detect_image_masks_kernel<shared>";
        case plan::kDirect: return "detect_image_masks_kernel<direct>";
        default: return "none";
    }
}

int si_hip_detect_image_masks_f32(const SiImageMaskDesc* d, const float* protos, const float* extras, const float* boxes, const int* counts,
                                  const int* geom, unsigned char* masks, si_stream_t stream) {
    if (!d || !protos || !extras || !boxes || !counts || !geom || !masks) return SI_E_BADARG;
    if (!si_aligned_to(protos, 4) || !si_aligned_to(extras, 4) || !si_aligned_to(boxes, 4) || !si_aligned_to(counts, 4) || !si_aligned_to(geom, 4))
        return SI_E_BADARG;
    const plan::Shape v = shape_of(d);
    const int rc = plan::StatusOf(v);
    if (rc != plan::base::kOk) return rc == plan::base::kBadArg ? SI_E_BADARG : SI_E_UNSUPPORTED;
    if (d->max_det == 0) return 0;
    const plan::Arm arm = plan::ArmOf(v);
    ImgMaskArgs a{protos, extras, boxes, counts, geom, masks, d->mh, d->mw, d->nm, d->proto_ld, d->max_det, d->extra, d->coef_off, d->oh, d->ow,
                  d->box_ld, d->crop, (int)plan::TilesX(v), plan::Capacity(v), plan::WordStores(v, si_aligned_to(masks, 4)) ? 1 : 0,
                  plan::VectorLoads(v, si_aligned_to(protos, 16)) ? 1 : 0};
    const dim3 grid((unsigned)(plan::TilesX(v) * plan::TilesY(v)), (unsigned)d->n);   // tiles <= OH * OW < 2^31
    hipStream_t s = (hipStream_t)stream;
    if (arm == plan::kShared) {
        hipLaunchKernelGGL(detect_image_masks_kernel<true>, grid, dim3(plan::kThreads), plan::LdsBytes(v), s, a);
    } else {
        hipLaunchKernelGGL(detect_image_masks_kernel<false>, grid, dim3(plan::kThreads), 0, s, a);
    }
    return (int)hipGetLastError();
}

}  // extern "C"
