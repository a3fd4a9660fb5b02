"""Restatement of torchvision.ops.RoIAlign / roi_align for the tests (test infrastructure, no product code): the rule of include/si_roi.h.

roi_align_ref decides in FLOAT32 with the header's operations in the header's order -- the scaled coordinates, the bin sizes, the sample counts
(ceilf), every sample coordinate, the inside test, the floor / clamp of the taps and the two weights of an axis -- and accumulates in FLOAT64.
The rule is discontinuous at y = -1 and y = h and in ceilf: a float64 restatement of the coordinates would disagree by whole samples.

The sum over the samples of a bin is separable: sum_iy sum_ix (hy, ly) x (hx, lx) applied to the four taps is Wy[i] X Wx[j]^T with Wy[i][row] the
sum of the y-weights that the inside samples of bin i put on `row`.  So a roi 4096 px wide costs 4096 one-dimensional samples here, not 4096^2.
(The kernel rounds the products hy * hx to fp32 and sums in fp32; this form keeps them in float64.  Where weights and values are dyadic both are
exact, which is what the bit-for-bit tests use.)

eval_graph: torch CPU float64 arithmetic for the operator set of build_toy_box_head / build_toy_mask_head around roi_align_ref's pooled features,
with the rnd= hook of tests/ct_reference.py.  matrix_*: the GPU case matrix and its shared references.
"""
import itertools
import os

import numpy as np

import util
from ct_reference import _ints, _parse, round_f16  # noqa: F401  (round_f16 re-exported)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "si_roi.h")
INTERVAL_HEADER = os.path.join(ROOT, "simpleinfer_amd", "csrc", "hip", "roi_interval.h")
ENTRIES = ["si_hip_roi_align_f32", "si_hip_roi_align_f16", "si_hip_roi_align_kernel_name"]
TYPES = ("torchvision.ops.RoIAlign", "torchvision.ops.roi_align")
GRID_LIMIT = 1 << 22       # SI_ROI_GRID_LIMIT
F = np.float32


def _pair(v):
    return (int(v), int(v)) if np.isscalar(v) else (int(v[0]), int(v[1]))


def roi_setup(roi, n, ph, pw, scale, sampling_ratio, aligned):
    """si_roi_setup of roi_interval.h in float32: None for an invalid roi, else (img, sw, sh, bw, bh, gw, gh, count)"""
    roi = np.asarray(roi, F)
    idx = roi[0]
    if not (idx >= 0 and idx < n and idx == np.floor(idx)):
        return None
    o, scale = F(0.5 if aligned else 0.0), F(scale)
    with np.errstate(over="ignore", invalid="ignore"):
        sw, sh, ew, eh = (roi[1] * scale - o, roi[2] * scale - o, roi[3] * scale - o, roi[4] * scale - o)
        if not all(np.isfinite(v) for v in (sw, sh, ew, eh)):
            return None
        rw, rh = ew - sw, eh - sh
        if not aligned:
            rw, rh = np.maximum(rw, F(1)), np.maximum(rh, F(1))
        if not (np.isfinite(rw) and np.isfinite(rh)):
            return None
        bh, bw = rh / F(ph), rw / F(pw)
        gh = F(sampling_ratio) if sampling_ratio > 0 else np.ceil(rh / F(ph))
        gw = F(sampling_ratio) if sampling_ratio > 0 else np.ceil(rw / F(pw))
    if not (gh <= GRID_LIMIT and gw <= GRID_LIMIT):
        return None
    gh, gw = np.maximum(gh, F(0)), np.maximum(gw, F(0))
    count = np.maximum(gh * gw, F(1))
    assert all(v.dtype == F for v in (sw, sh, bw, bh, gh, gw, count))
    return int(idx), sw, sh, bw, bh, int(gw), int(gh), count


def axis_weights(start, bin_size, g, pooled, size):
    """W [pooled, size] float64: W[i][p] is the weight that the inside samples of bin i put on pixel p of the axis; every decision in float32"""
    W = np.zeros((pooled, size), np.float64)
    if g == 0:
        return W
    i = np.arange(pooled, dtype=F)[:, None]
    s = np.arange(g, dtype=F)[None, :]
    with np.errstate(over="ignore", invalid="ignore"):
        base = start + i * bin_size                       # float32 throughout: (start + i * bin) + (((s + 0.5) * bin) / g)
        t = ((s + F(0.5)) * bin_size) / F(g)
        y = base + t
    assert y.dtype == F
    inside = ~((y < F(-1)) | (y > F(size)))
    y = np.maximum(y, F(0))
    lo = np.where(inside, y, F(0)).astype(np.int64)          # (int)y
    top = lo >= size - 1
    lo = np.where(top, size - 1, lo)
    hi = np.where(top, size - 1, lo + 1)
    y = np.where(top, lo.astype(F), y)
    l = (y - lo.astype(F)).astype(F)
    h = (F(1) - l).astype(F)
    rows = np.broadcast_to(np.arange(pooled)[:, None], lo.shape)
    np.add.at(W, (rows[inside], lo[inside]), h[inside].astype(np.float64))
    np.add.at(W, (rows[inside], hi[inside]), l[inside].astype(np.float64))
    return W


def roi_align_ref(x, rois, output_size, spatial_scale=1.0, sampling_ratio=-1, aligned=False):
    """x [n, h, w, c] (any float type; its values are taken as they are), rois [k, 5] -> float64 [k, ph, pw, c]; NaN rows for invalid rois"""
    x64 = np.asarray(x, np.float64)
    n, h, w, c = x64.shape
    rois = np.asarray(rois, F)
    ph, pw = _pair(output_size)
    out = np.empty((rois.shape[0], ph, pw, c), np.float64)
    for r in range(rois.shape[0]):
        box = roi_setup(rois[r], n, ph, pw, spatial_scale, sampling_ratio, aligned)
        if box is None:
            out[r] = np.nan
            continue
        img, sw, sh, bw, bh, gw, gh, count = box
        Wy, Wx = axis_weights(sh, bh, gh, ph, h), axis_weights(sw, bw, gw, pw, w)
        out[r] = np.einsum("iy,yxc,jx->ijc", Wy, x64[img], Wx, optimize=True) / np.float64(count)
    return out


def expected_kernel(c, half, in_ld=None, out_ld=None, misaligned=False):
    """the instantiation for 16-byte aligned buffers: fp32 4 | 1, fp16 8 | 4 | 2 | 1 from c and both pixel strides"""
    lds = [c, in_ld or c, out_ld or c]
    widths = (8, 4, 2) if half else (4,)
    vw = 1 if misaligned else next((v for v in widths if all(d % v == 0 for d in lds)), 1)
    return "roi_align_kernel<%s, %d>" % ("_Float16" if half else "float", vw)


# ---- the GPU case matrix ------------------------------------------------------------------------------------------------------
MATRIX_N, MATRIX_H, MATRIX_W, MATRIX_CMAX = 2, 9, 11, 16
MATRIX_C = (1, 3, 4, 5, 8, 12, 16)
MATRIX_OUT = ((1, 1), (2, 3), (7, 7))
MATRIX_RATIO = (-1, 0, 1, 2, 3)
MATRIX_ALIGNED = (False, True)
MATRIX_SCALE = (1.0, 0.25, 0.0625)
MATRIX_K = (1, 5, 70)


def matrix_x():
    """[2, 9, 11, 16] float32 whose values are fp16 numbers: one reference serves both storage types, channels [:c] every c of the matrix"""
    return util.rng_uniform(101, (MATRIX_N, MATRIX_H, MATRIX_W, MATRIX_CMAX), -1.0, 1.0).astype(np.float16).astype(np.float32)


def matrix_rois(scale):
    """70 boxes in image pixels for a map of 9 x 11 at `scale` (map coordinates over scale: exact, the scales are powers of two).  By hand:
    inside, crossing each border, wholly outside, zero-size, x2 < x1, both images, one 4096 map pixels wide; the rest from a fixed seed.
    K = 1 and K = 5 are prefixes."""
    hand = [
        (0, 2.25, 1.5, 7.75, 6.0),        # inside
        (1, -3.0, 2.0, 4.5, 5.5),         # crossing the left border, image 1
        (0, 6.5, 1.0, 14.0, 4.0),         # the right one
        (1, 3.0, -4.0, 8.0, 3.25),        # the top one
        (0, 1.0, 5.0, 6.0, 12.5),         # the bottom one
        (1, 20.0, 15.0, 26.0, 21.0),      # wholly outside
        (0, -9.0, -8.0, -3.0, -2.5),      # wholly outside, negative
        (1, 4.0, 3.0, 4.0, 3.0),          # zero-size
        (0, 7.0, 6.0, 2.0, 1.0),          # x2 < x1, y2 < y1
        (1, 5.5, 2.0, 3.5, 7.0),          # x2 < x1 only
        (0, -100.0, 2.0, 3996.0, 6.0),    # 4096 map pixels wide
        (1, 0.0, 0.0, 11.0, 9.0),         # the whole map
        (0, 0.0, 0.0, 0.0, 0.0),          # a zero-padded slot
        (1, -1.0, -1.0, 12.0, 10.0),      # one pixel beyond every border
    ]
    rest = 70 - len(hand)
    u = util.rng_uniform(102, (rest, 4), 0.0, 1.0).astype(np.float64)
    rnd = np.empty((rest, 5), np.float64)
    rnd[:, 0] = np.arange(rest) % MATRIX_N
    rnd[:, 1] = u[:, 0] * 14.0 - 2.0
    rnd[:, 2] = u[:, 1] * 12.0 - 2.0
    rnd[:, 3] = rnd[:, 1] + u[:, 2] * 9.0
    rnd[:, 4] = rnd[:, 2] + u[:, 3] * 8.0
    rois = np.concatenate([np.asarray(hand, np.float64), rnd])
    rois[:, 1:] /= scale
    return rois.astype(F)


def matrix_params():
    """(output_size, sampling_ratio, aligned, scale): 90 combinations; with c and K the matrix has 90 x 7 x 3 cases per storage type"""
    return list(itertools.product(MATRIX_OUT, MATRIX_RATIO, MATRIX_ALIGNED, MATRIX_SCALE))


_MATRIX_REF = {}


def matrix_ref(out, ratio, aligned, scale):
    """float64 [70, ph, pw, 16], computed once per combination, read-only: the cases of every c and K are slices of it (rows are independent)"""
    key = (out, ratio, aligned, scale)
    if key not in _MATRIX_REF:
        ref = roi_align_ref(matrix_x(), matrix_rois(scale), out, scale, ratio, aligned)
        ref.setflags(write=False)
        _MATRIX_REF[key] = ref
    return _MATRIX_REF[key]


# ---- graphs -------------------------------------------------------------------------------------------------------------------
def eval_graph(builder, xs, rnd=None):
    """float64 evaluation of a PnnxBuilder graph of RoIAlign / roi_align, Conv2d, ConvTranspose2d, ReLU, Sigmoid, flatten, Linear and Output:
    torch CPU arithmetic around roi_align_ref.  xs: one array per graph input in order (NHWC for rank 4).  Returns the list of the graph outputs
    as the engine stores them (NHWC for rank 4).  rnd: applied to the inputs, the weights and every operator's output (None: exact)."""
    import torch
    import torch.nn.functional as tf

    q = rnd or (lambda a: np.asarray(a, np.float64))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64)))
    nchw = lambda a: t(a).permute(0, 3, 1, 2)
    nhwc = lambda y: y.permute(0, 2, 3, 1).contiguous().numpy()
    vals, results, feed = {}, [], list(xs)
    lines = [_parse(ln) for ln in builder.lines]
    graph_outs = {ins[0] for typ, _, ins, _, _ in lines if typ == "pnnx.Output"}      # (a graph output keeps fp32: not rounded)
    for typ, name, ins, outs, prm in lines:
        a = lambda k: q(builder.attrs["%s.%s" % (name, k)])
        if typ == "pnnx.Input":
            src = feed.pop(0)
            vals[outs[0]] = np.asarray(src, F) if len(builder.shapes[outs[0]]) == 2 and builder.shapes[outs[0]][1] == 5 else q(src)   # (boxes stay fp32)
            continue
        if typ == "pnnx.Output":
            results.append(vals[ins[0]])
            continue
        x = vals[ins[0]]
        if typ in TYPES:
            y = roi_align_ref(x, vals[ins[1]], _ints(prm["output_size"]), float(prm["spatial_scale"]), int(prm["sampling_ratio"]), prm["aligned"] == "True")
        elif typ == "nn.Conv2d":
            y = nhwc(tf.conv2d(nchw(x), t(a("weight")), t(a("bias")) if prm["bias"] == "True" else None, _ints(prm["stride"]), _ints(prm["padding"])))
        elif typ == "nn.ConvTranspose2d":
            y = nhwc(tf.conv_transpose2d(nchw(x), t(a("weight")), t(a("bias")) if prm["bias"] == "True" else None, _ints(prm["stride"]),
                                         _ints(prm["padding"]), _ints(prm["output_padding"])))
        elif typ == "nn.ReLU":
            y = np.maximum(x, 0.0)
        elif typ == "nn.Sigmoid":
            y = 1.0 / (1.0 + np.exp(-x))
        elif typ == "torch.flatten":
            y = x.transpose(0, 3, 1, 2).reshape(x.shape[0], -1) if x.ndim == 4 else x.reshape(x.shape[0], -1)      # (NCHW order, as torch)
        elif typ == "nn.Linear":
            y = tf.linear(t(x), t(a("weight")), t(a("bias")) if prm["bias"] == "True" else None).numpy()
        else:
            raise NotImplementedError(typ)
        vals[outs[0]] = np.asarray(y, np.float64) if outs[0] in graph_outs else q(y)
    return results
