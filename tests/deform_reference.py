"""Restatements for the deformable-convolution tests (test infrastructure, no product code).

deform_conv2d_ref: torchvision.ops.deform_conv2d in numpy on NHWC arrays, the rule of include/si_deform.h.  The sampling coordinate is
evaluated in fp32 exactly as the rule writes it (one fp32 addition of the fp32 base coordinate and the offset), so that floor() and the range
test decide as the kernel does; everything after that is float64.  A NaN coordinate gives NaN, a coordinate outside (-1, size) -- +-Inf
included -- gives 0, a corner outside the image contributes exactly 0 and is never read, a corner inside is multiplied by its weight even
when the weight is 0.

deform_conv2d_grid_sample: an independent float64 restatement on torch -- F.grid_sample(align_corners=True, padding_mode="zeros") per tap and
offset group on the coordinates of sample_coords, the mask multiply, an einsum.  tests/test_deform_cpu.py pins the numpy rule to it.

CASES / operands: the case table and the operand recipe of the GPU tests.  eval_graph: a float64 evaluator of a PnnxBuilder graph for the
operator set of build_toy_dcn_head, with the rnd= hook of tests/ct_reference.py for the fp16-storage emulation.
"""
import os

import numpy as np

import util
from ct_reference import ACTS, _ints, _parse, conv2d_ref, round_f16  # noqa: F401  (round_f16 re-exported)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "si_deform.h")
ENTRIES = ["si_hip_deform_conv2d_weight_elems", "si_hip_deform_conv2d_pack_weight_host", "si_hip_deform_conv2d_f32", "si_hip_deform_conv2d_kernel_name"]
TYPE = "torchvision.ops.DeformConv2d"


def _pair(v):
    return (int(v), int(v)) if np.isscalar(v) else (int(v[0]), int(v[1]))


def out_hw(ih, iw, k, s, p, d):
    return ((ih + 2 * p[0] - d[0] * (k[0] - 1) - 1) // s[0] + 1, (iw + 2 * p[1] - d[1] * (k[1] - 1) - 1) // s[1] + 1)


def sample_coords(offset_nhwc, in_hw, k, s, p, d):
    """(y, x) as fp32 arrays [n, oh, ow, og, kh * kw]: float32(ho * sh - ph + i * dh) + dy in ONE fp32 addition, likewise x"""
    off = np.asarray(offset_nhwc, np.float32)
    n, oh, ow, oc = off.shape
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = k, s, p, d
    taps = kh * kw
    assert oc % (2 * taps) == 0, (oc, taps)
    og = oc // (2 * taps)
    off = off.reshape(n, oh, ow, og, taps, 2)
    ti, tj = np.divmod(np.arange(taps), kw)
    by = (np.arange(oh)[:, None] * sh - ph + ti[None, :] * dh).astype(np.float32)       # [oh, taps]
    bx = (np.arange(ow)[:, None] * sw - pw + tj[None, :] * dw).astype(np.float32)       # [ow, taps]
    with np.errstate(invalid="ignore", over="ignore"):
        y = by[None, :, None, None, :] + off[..., 0]
        x = bx[None, None, :, None, :] + off[..., 1]
    assert y.dtype == np.float32 and x.dtype == np.float32
    return y, x


def sample_columns(x_nhwc, offset_nhwc, mask_nhwc, k, s, p, d):
    """col [n, oh, ow, taps, ic] float64: mask * sample for every tap and input channel"""
    X = np.asarray(x_nhwc, np.float64)
    n, ih, iw, ic = X.shape
    y32, x32 = sample_coords(offset_nhwc, (ih, iw), k, s, p, d)
    _, oh, ow, og, taps = y32.shape
    assert ic % og == 0, (ic, og)
    cpo = ic // og
    with np.errstate(invalid="ignore", over="ignore"):
        nan = np.isnan(y32) | np.isnan(x32)
        inside = (y32 > -1) & (y32 < ih) & (x32 > -1) & (x32 < iw)                       # the range test comes first, in fp32
        y = np.where(inside, y32, 0).astype(np.float64)
        x = np.where(inside, x32, 0).astype(np.float64)
        hl, wl = np.floor(y).astype(np.int64), np.floor(x).astype(np.int64)            # ... the conversion to an integer after it
        lh, lw = y - hl, x - wl
        hh, hw = 1.0 - lh, 1.0 - lw
        img = np.arange(n)[:, None, None, None, None]
        col = np.zeros((n, oh, ow, taps, ic), np.float64)
        for g in range(og):
            ch = slice(g * cpo, (g + 1) * cpo)
            acc = None
            for wgt, yy, xx in ((hh * hw, hl, wl), (hh * lw, hl, wl + 1), (lh * hw, hl + 1, wl), (lh * lw, hl + 1, wl + 1)):
                ok = inside[:, :, :, g] & (yy[:, :, :, g] >= 0) & (yy[:, :, :, g] <= ih - 1) & (xx[:, :, :, g] >= 0) & (xx[:, :, :, g] <= iw - 1)
                v = X[img[:, :, :, 0], np.clip(yy[:, :, :, g], 0, ih - 1), np.clip(xx[:, :, :, g], 0, iw - 1)][..., ch]    # [n, oh, ow, taps, cpo]
                term = np.where(ok[..., None], wgt[:, :, :, g, :, None] * v, 0.0)      # inside: multiplied even by a zero weight; outside: exactly 0
                acc = term if acc is None else acc + term
            acc = np.where(nan[:, :, :, g, :, None], np.nan, np.where(inside[:, :, :, g, :, None], acc, 0.0))
            if mask_nhwc is not None:
                m = np.asarray(mask_nhwc, np.float64).reshape(n, oh, ow, og, taps)[:, :, :, g]
                acc = m[..., None] * acc
            col[..., ch] = acc
    return col


def deform_conv2d_ref(x_nhwc, offset_nhwc, w_oihw, bias=None, mask_nhwc=None, stride=(1, 1), padding=(0, 0), dilation=(1, 1), groups=1,
                      act="none", act_param=0.0):
    """float64 NHWC result of torchvision.ops.deform_conv2d (the offset-group count is read off the offset's channels)"""
    s, p, d = _pair(stride), _pair(padding), _pair(dilation)
    w = np.asarray(w_oihw, np.float64)
    oc, cg, kh, kw = w.shape
    n, ih, iw, ic = np.asarray(x_nhwc).shape
    assert ic == cg * groups and oc % groups == 0, (ic, cg, groups, oc)
    assert tuple(np.asarray(offset_nhwc).shape[1:3]) == out_hw(ih, iw, (kh, kw), s, p, d)
    col = sample_columns(x_nhwc, offset_nhwc, mask_nhwc, (kh, kw), s, p, d)
    cog = oc // groups
    out = np.zeros(col.shape[:3] + (oc,), np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for g in range(groups):
            wg = w[g * cog:(g + 1) * cog].reshape(cog, cg, kh * kw)
            out[..., g * cog:(g + 1) * cog] = np.einsum("nhwtc,oct->nhwo", col[..., g * cg:(g + 1) * cg], wg)
        if bias is not None:
            out = out + np.asarray(bias, np.float64)
        return ACTS[act](out, act_param)


def deform_conv2d_grid_sample(x_nhwc, offset_nhwc, w_oihw, bias=None, mask_nhwc=None, stride=(1, 1), padding=(0, 0), dilation=(1, 1), groups=1,
                              coords64=False):
    """the independent restatement: F.grid_sample per (tap, offset group) in float64 on the fp32 coordinates of sample_coords (coords64: the
    coordinates summed in float64 instead), then the mask and an einsum.  Needs ih, iw > 1 (align_corners normalises by size - 1)."""
    import torch
    s, p, d = _pair(stride), _pair(padding), _pair(dilation)
    X = torch.from_numpy(np.ascontiguousarray(np.asarray(x_nhwc, np.float64).transpose(0, 3, 1, 2)))
    w = np.asarray(w_oihw, np.float64)
    oc, cg, kh, kw = w.shape
    n, ic, ih, iw = X.shape
    assert ih > 1 and iw > 1
    if coords64:
        off = np.asarray(offset_nhwc, np.float64)
        oh, ow = off.shape[1:3]
        taps = kh * kw
        og = off.shape[3] // (2 * taps)
        off = off.reshape(n, oh, ow, og, taps, 2)
        ti, tj = np.divmod(np.arange(taps), kw)
        y = (np.arange(oh)[:, None] * s[0] - p[0] + ti[None, :] * d[0])[None, :, None, None, :] + off[..., 0]
        x = (np.arange(ow)[:, None] * s[1] - p[1] + tj[None, :] * d[1])[None, None, :, None, :] + off[..., 1]
    else:
        y, x = (c.astype(np.float64) for c in sample_coords(offset_nhwc, (ih, iw), (kh, kw), s, p, d))
    _, oh, ow, og, taps = y.shape
    cpo = ic // og
    col = np.zeros((n, oh, ow, taps, ic), np.float64)
    for g in range(og):
        for t in range(taps):
            grid = np.stack([2.0 * x[:, :, :, g, t] / (iw - 1) - 1.0, 2.0 * y[:, :, :, g, t] / (ih - 1) - 1.0], -1)
            v = torch.nn.functional.grid_sample(X[:, g * cpo:(g + 1) * cpo], torch.from_numpy(grid), mode="bilinear", padding_mode="zeros",
                                                align_corners=True).numpy()            # [n, cpo, oh, ow]
            v = v.transpose(0, 2, 3, 1)
            if mask_nhwc is not None:
                v = v * np.asarray(mask_nhwc, np.float64)[..., g * taps + t, None]
            col[:, :, :, t, g * cpo:(g + 1) * cpo] = v
    cog = oc // groups
    out = np.zeros((n, oh, ow, oc), np.float64)
    for g in range(groups):
        out[..., g * cog:(g + 1) * cog] = np.einsum("nhwtc,oct->nhwo", col[..., g * cg:(g + 1) * cg], w[g * cog:(g + 1) * cog].reshape(cog, cg, taps))
    return out if bias is None else out + np.asarray(bias, np.float64)


# ---- the case table: (k, s, p, d, (N, H, W), (Cin, Cout), groups, og, mask, bias) -- the smallest shapes at which the kernel can go wrong ----
CASES = [
    ((3, 3), (1, 1), (1, 1), (1, 1), (2, 8, 8), (16, 16), 1, 1, True, True),       # 1  the DCNv2 base, M = 128
    ((3, 3), (1, 1), (1, 1), (1, 1), (2, 8, 8), (16, 16), 1, 1, False, False),     # 2  DCNv1
    ((1, 1), (1, 1), (0, 0), (1, 1), (1, 5, 13), (17, 65), 1, 1, False, False),    # 3  M = 65 and N = 65: one past a tile both ways, scalar arm
    ((3, 3), (2, 2), (1, 1), (1, 1), (1, 9, 7), (36, 5), 1, 2, True, False),       # 4  a K-tile straddles the offset groups at channel 18
    ((3, 2), (1, 2), (2, 1), (2, 1), (2, 9, 7), (8, 8), 2, 4, False, False),       # 5  rectangular
    ((3, 3), (1, 1), (1, 1), (1, 1), (1, 1, 1), (4, 4), 1, 1, False, False),       # 6  almost every corner outside
    ((3, 3), (1, 1), (1, 1), (1, 1), (1, 3, 21), (3, 1), 1, 1, False, False),      # 7  M = 63
    ((5, 5), (1, 1), (2, 2), (1, 1), (1, 6, 6), (4, 8), 1, 1, False, False),       # 8  25 taps, several taps per K-tile
    ((3, 3), (1, 1), (1, 1), (1, 1), (1, 4, 4), (1, 1), 1, 1, False, False),       # 9  single channel
    ((3, 3), (1, 1), (1, 1), (1, 1), (3, 4, 11), (40, 72), 2, 2, True, False),     # 10 M = 132: two tile edges and batch boundaries inside tiles
]


def case_id(c):
    k, s, p, d, (n, h, w), (ci, co), g, og, mask, bias = c
    return "k%dx%d_s%dx%d_p%dx%d_d%dx%d_n%d_%dx%d_%d-%d_g%d_og%d%s%s" % (*k, *s, *p, *d, n, h, w, ci, co, g, og, "_mask" if mask else "", "_bias" if bias else "")


def offsets(seed, shape):
    """U(-2.5, 2.5), every 7th (flat index) rounded to an integer, every 11th multiplied by 4"""
    off = util.rng_uniform(seed, shape, -2.5, 2.5).reshape(-1)
    off[::7] = np.round(off[::7])
    off[::11] *= np.float32(4)
    return off.reshape(shape)


def operands(c, seed=0):
    """(x, offset, mask or None, weight [Cout][Cin/groups][kh][kw], bias or None): x and weights U(-1, 1), the weights scaled by sqrt(3 / K)"""
    k, s, p, d, (n, h, w), (ci, co), g, og, mask, bias = c
    oh, ow = out_hw(h, w, k, s, p, d)
    taps = k[0] * k[1]
    x = util.rng_uniform(seed, (n, h, w, ci), -1.0, 1.0)
    a = np.float32(np.sqrt(3.0 / (ci // g * taps)))
    wt = util.rng_uniform(seed + 1, (co, ci // g, k[0], k[1]), -1.0, 1.0) * a
    off = offsets(seed + 2, (n, oh, ow, 2 * og * taps))
    m = util.rng_uniform(seed + 3, (n, oh, ow, og * taps), 0.0, 1.0) if mask else None
    b = util.rng_uniform(seed + 4, (co,), -0.1, 0.1) if bias else None
    return x, off, m, wt, b


def run_ref(c, ops, act="none", act_param=0.0):
    x, off, m, wt, b = ops
    return deform_conv2d_ref(x, off, wt, b, m, c[1], c[2], c[3], c[6], act, act_param)


# ---- graphs -----------------------------------------------------------------------------------------------------------------
def eval_graph(builder, x_nhwc, rnd=None):
    """float64 evaluation of a PnnxBuilder graph on NHWC tensors: the operators of tests/ct_reference.py's evaluator that the DCN toys use
    (Conv2d, ReLU) plus nn.SiLU, nn.Sigmoid, torch.split on the channels and torchvision.ops.DeformConv2d.  rnd: applied to the input, every
    weight / bias and every layer's output except the graph output (None: exact)."""
    q = rnd or (lambda a: np.asarray(a, np.float64))
    vals, result = {}, None
    lines = [_parse(ln) for ln in builder.lines]
    graph_outs = {ins[0] for typ, _, ins, _, _ in lines if typ == "pnnx.Output"}
    for typ, name, ins, outs, prm in lines:
        a = lambda k: builder.attrs["%s.%s" % (name, k)]
        if typ == "pnnx.Input":
            vals[outs[0]] = q(x_nhwc)
            continue
        if typ == "pnnx.Output":
            result = vals[ins[0]]
            continue
        x = vals[ins[0]]
        if typ == "torch.split":
            assert int(prm["dim"]) == 1
            at = 0
            for o, n in zip(outs, _ints(prm["split_size_or_sections"])):
                vals[o] = x[..., at:at + n]        # (a view of a stored tensor: nothing is rounded again)
                at += n
            continue
        if typ == "nn.Conv2d":
            assert _ints(prm["dilation"]) == (1, 1) and int(prm["groups"]) == 1
            y = conv2d_ref(x, q(a("weight")), q(a("bias")) if prm["bias"] == "True" else None, _ints(prm["stride"]), _ints(prm["padding"]))
        elif typ == TYPE:
            # (the coordinates are fp32 in the rule: the offsets are what the engine stores, fp32 values either way)
            y = deform_conv2d_ref(x, vals[ins[1]], q(a("weight")), q(a("bias")) if prm["bias"] == "True" else None, vals[ins[2]] if len(ins) == 3 else None,
                                  _ints(prm["stride"]), _ints(prm["padding"]), _ints(prm["dilation"]), int(prm["groups"]))
        elif typ == "nn.SiLU":
            y = ACTS["silu"](x, 0.0)
        elif typ == "nn.ReLU":
            y = ACTS["relu"](x, 0.0)
        elif typ == "nn.Sigmoid":
            y = ACTS["sigmoid"](x, 0.0)
        else:
            raise NotImplementedError(typ)
        assert tuple(y.shape) == tuple(np.array(builder.shapes[outs[0]])[[0, 2, 3, 1]]), (typ, name, y.shape, builder.shapes[outs[0]])
        vals[outs[0]] = y if outs[0] in graph_outs else q(y)
    return result
