"""Restatements for the F.conv2d (tensor filter) tests (test infrastructure, no product code).

conv2d_ref: numpy float64 of torch's rule, zero padding:
    y[n, o, oy, ox] = b[o] + sum over c in the group, ky, kx of w[o, c, ky, kx] * x[n, c, oy sh - pt + ky dh, ox sw - pl + kx dw]
padding is an int or a pair (both sides), 'valid', or 'same' (stride 1: d (K - 1) per axis, the odd one on the far side).  With rnd= (round_f16)
the operands are rounded to half, every sum stays float64, and the caller rounds the result ONCE: the fp16 restatement of the kernels' storage
rule.  per_sample_ref: filter n [C, kh, kw] meets image n, the depthwise cross-correlation of the Siamese trackers.

eval_graph: a float64 evaluator of a PnnxBuilder graph for the operator set of the five toys, with the rnd= hook of tests/conv1d_reference.py:
applied to the inputs, every weight and constant, and every stored tensor (each layer's output except the graph outputs).

Arrays are torch's layouts here ([N, C, H, W], [O, C / g, kh, kw]); nhwc() / nchw() go to and from what hipops.xcorr and the engine take.
"""
import os
import re

import numpy as np

from conv1d_reference import activation  # noqa: F401  (re-exported)
from ct_reference import _ints, _parse, round_f16  # noqa: F401  (round_f16 re-exported)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "si_xcorr.h")
ENTRIES = ["si_hip_xcorr_f32", "si_hip_xcorr_f16", "si_hip_xcorr_kernel_name"]

# (N, C, H, W, O, KH, KW, stride, padding, dilation, groups): the smallest shapes at which each mechanism can fail.  Together: O in
# {1, 3, 16, 17, 33}; C in {1, 3, 4, 5, 8, 32, 40}; kernels 1x1, 3x3, 1x5, 6x6 and one larger than the unpadded image; 1, 63, 64 and 65 output
# pixels; N in {1, 3}; strides 1, 2 and (2, 1); dilations 1 and 2; pads 0, 1 and an asymmetric 'same'
DENSE_CASES = [
    (1, 1, 8, 8, 3, 1, 1, 1, 0, 1, 1),            # C = 1, 1x1: 64 pixels, exactly one tile
    (3, 3, 9, 11, 3, 3, 3, 1, 0, 1, 1),           # 7 x 9 = 63 pixels, nothing divides
    (1, 4, 5, 13, 16, 3, 3, 1, 1, 1, 1),          # pad 1: 5 x 13 = 65 pixels, one past a tile; one full filter tile
    (1, 5, 6, 6, 17, 6, 6, 1, 0, 1, 1),           # the kernel is the image: ONE output pixel; one filter past a tile
    (3, 8, 12, 10, 33, 1, 5, (2, 1), 0, 1, 1),    # 1x5, stride (2, 1), three filter tiles with one live filter in the last
    (1, 32, 9, 9, 3, 3, 3, 2, 1, 1, 1),           # stride 2, pad 1
    (1, 40, 8, 8, 16, 3, 3, 1, "same", 2, 1),     # dilation 2, a symmetric 'same'; C = 40: a ragged fp16 channel group
    (1, 8, 8, 8, 5, 4, 2, 1, "same", 1, 1),       # 'same' with odd totals: pads (1, 2) and (0, 1)
    (1, 4, 3, 3, 3, 5, 5, 1, 2, 1, 1),            # the kernel is larger than the unpadded image
    (1, 16, 22, 22, 1, 6, 6, 1, 0, 1, 1),         # SiamFC's form: O = 1, several workgroups
    (3, 8, 7, 9, 70, 3, 3, 1, 1, 1, 1),           # two filter blocks of 64
]
# groups == C == O (C = 1 with one filter among them: both forms compute the same thing there, the depthwise kernel is chosen)
DEPTHWISE_CASES = [
    (1, 1, 9, 9, 1, 3, 3, 1, 0, 1, 1),
    (2, 3, 10, 9, 3, 3, 3, 2, 1, 1, 3),
    (1, 4, 8, 8, 4, 1, 5, (2, 1), 0, 1, 4),
    (2, 7, 9, 9, 7, 4, 2, 1, "same", 1, 7),
    (2, 64, 31, 31, 64, 7, 7, 1, 0, 1, 64),       # SiamRPN++ at its true spatial size
    (1, 8, 3, 3, 8, 5, 5, 1, 2, 1, 8),            # the kernel is larger than the unpadded image
    (2, 12, 9, 9, 12, 3, 3, 1, 1, 2, 12),         # dilation 2; C = 12: a whole and a ragged run of 8 halves
]
CASES = DENSE_CASES + DEPTHWISE_CASES
# fp16: the dense subset with C % 8 == 0 and the depthwise form (which has no such rule)
F16_CASES = [c for c in DENSE_CASES if c[1] % 8 == 0] + [(1, 8, 9, 11, 17, 3, 3, 1, 0, 1, 1), (3, 16, 5, 13, 33, 3, 3, 1, 1, 1, 1)] + DEPTHWISE_CASES


def case_id(c):
    return "N%d_C%d_%dx%d_O%d_k%dx%d_s%s_p%s_d%s_g%d" % tuple(str(v).replace(" ", "").replace("(", "").replace(")", "").replace(",", "x")
                                                              if not isinstance(v, int) else v for v in c)


def is_depthwise(c):
    return c[10] == c[1] == c[4]     # (one channel and one filter: the depthwise kernel serves it)


def kname(case, dtype, depthwise=None):
    dw = is_depthwise(case) if depthwise is None else depthwise
    return "xcorr_%s_kernel<%s>" % ("depthwise" if dw else "dense", "_Float16" if np.dtype(dtype) == np.float16 else "float")


def header_fields():
    """(name, C type) of SiXcorrDesc's fields, in the header's order"""
    m = re.search(r"typedef struct SiXcorrDesc \{(.*?)\} SiXcorrDesc;", open(HEADER).read(), flags=re.S)
    body = re.sub(r"/\*.*?\*/", " ", m.group(1), flags=re.S)
    return [(n.strip(), typ) for typ, names in re.findall(r"\b(int|long long|float)\s+([^;]+);", body) for n in names.split(",")]


def pair(v):
    return (int(v), int(v)) if isinstance(v, (int, np.integer)) else (int(v[0]), int(v[1]))


def pads(kh, kw, padding, dilation=1, stride=1):
    """((top, bottom), (left, right))"""
    (dh, dw), (sh, sw) = pair(dilation), pair(stride)
    if padding == "valid":
        return (0, 0), (0, 0)
    if padding == "same":
        assert sh == 1 and sw == 1
        th, tw = dh * (kh - 1), dw * (kw - 1)
        return (th // 2, th - th // 2), (tw // 2, tw - tw // 2)
    ph, pw = pair(padding)
    return (ph, ph), (pw, pw)


def out_hw(h, w, kh, kw, stride, padding, dilation):
    (pt, pb), (pl, pr) = pads(kh, kw, padding, dilation, stride)
    (sh, sw), (dh, dw) = pair(stride), pair(dilation)
    eh, ew = h + pt + pb - dh * (kh - 1) - 1, w + pl + pr - dw * (kw - 1) - 1
    return (eh // sh + 1 if eh >= 0 else 0), (ew // sw + 1 if ew >= 0 else 0)


def nhwc(a):
    return np.ascontiguousarray(np.asarray(a).transpose(0, 2, 3, 1))


def nchw(a):
    return np.ascontiguousarray(np.asarray(a).transpose(0, 3, 1, 2))


def operands(case, seed=0, dtype=np.float32, bias=True):
    """(x, w, b) of a case in torch's layouts: x U(-1, 1) and w U(-a, a), a = sqrt(3 / fan_in), in `dtype` (both are tensors of the graph);
    b fp32 U(-0.5, 0.5) or None"""
    n, c, h, wd, oc, kh, kw, s, p, d, g = case
    r = np.random.Generator(np.random.Philox(seed + 1000 * c + 10 * kh + kw))
    x = r.uniform(-1, 1, (n, c, h, wd)).astype(np.float32).astype(dtype)
    a = np.sqrt(3.0 / ((c // g) * kh * kw))
    w = r.uniform(-a, a, (oc, c // g, kh, kw)).astype(np.float32).astype(dtype)
    b = r.uniform(-0.5, 0.5, oc).astype(np.float32) if bias else None
    return x, w, b


def templates(case, seed=0, dtype=np.float32):
    """the per-sample filters z [N, C, kh, kw] of a depthwise case"""
    n, c, h, wd, oc, kh, kw, s, p, d, g = case
    r = np.random.Generator(np.random.Philox(seed + 77 + 1000 * c + 10 * kh + kw))
    a = np.sqrt(3.0 / (kh * kw))
    return r.uniform(-a, a, (n, c, kh, kw)).astype(np.float32).astype(dtype)


def conv2d_ref(x, w, b=None, stride=1, padding=0, dilation=1, groups=1, act="none", act_param=0.0, rnd=None):
    """float64 [N, O, Ho, Wo]; rnd: applied to x and w (the bias is fp32 in the kernels and stays as given)"""
    q = rnd or (lambda a: np.asarray(a, np.float64))
    x, w = q(x), q(w)
    n, c, h, wd = x.shape
    oc, cg, kh, kw = w.shape
    assert cg * groups == c and oc % groups == 0
    (pt, pb), (pl, pr) = pads(kh, kw, padding, dilation, stride)
    (sh, sw), (dh, dw) = pair(stride), pair(dilation)
    ho, wo = out_hw(h, wd, kh, kw, stride, padding, dilation)
    assert ho > 0 and wo > 0
    xp = np.zeros((n, c, pt + h + pb + sh * ho + dh * kh, pl + wd + pr + sw * wo + dw * kw), np.float64)   # (room behind: a window never leaves)
    xp[:, :, pt:pt + h, pl:pl + wd] = x
    ocg = oc // groups
    y = np.zeros((n, oc, ho, wo), np.float64)
    for g in range(groups):
        xs, ws = xp[:, g * cg:(g + 1) * cg], w[g * ocg:(g + 1) * ocg]
        for ky in range(kh):
            for kx in range(kw):
                win = xs[:, :, ky * dh: ky * dh + (ho - 1) * sh + 1: sh, kx * dw: kx * dw + (wo - 1) * sw + 1: sw]     # [N, cg, Ho, Wo]
                y[:, g * ocg:(g + 1) * ocg] += np.einsum("oc,nchw->nohw", ws[:, :, ky, kx], win)
    if b is not None:
        y += np.asarray(b, np.float64)[None, :, None, None]
    return activation(act, y, act_param)


def per_sample_ref(x, z, b=None, stride=1, padding=0, dilation=1, act="none", act_param=0.0, rnd=None):
    """y[n] = conv2d(x[n], z[n] as [C, 1, kh, kw], groups = C): float64 [N, C, Ho, Wo]"""
    return np.concatenate([conv2d_ref(x[i:i + 1], np.asarray(z[i])[:, None], b, stride, padding, dilation, x.shape[1], act, act_param, rnd)
                           for i in range(x.shape[0])], axis=0)


def conv2d_torch(x, w, b=None, stride=1, padding=0, dilation=1, groups=1):
    import torch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64)))
    p = padding if isinstance(padding, str) else pair(padding)
    return torch.nn.functional.conv2d(t(x), t(w), None if b is None else t(b), pair(stride), p, pair(dilation), groups).numpy()


# ---- graphs -----------------------------------------------------------------------------------------------------------------
def _padding_of(text):
    return text if text in ("same", "valid") else tuple(_ints(text))


def eval_graph(builder, inputs, rnd=None):
    """float64 evaluation of a PnnxBuilder graph in file order: the list of graph outputs in torch's layout.  `inputs`: the graph inputs in
    file order (torch's layout)"""
    q = rnd or (lambda a: np.asarray(a, np.float64))
    vals, results = {}, []
    lines = [_parse(ln) for ln in builder.lines]
    graph_outs = {ins[0] for typ, _, ins, _, _ in lines if typ == "pnnx.Output"}
    feed = list(inputs)
    for typ, name, ins, outs, prm in lines:
        a = lambda k: builder.attrs["%s.%s" % (name, k)]
        if typ == "pnnx.Input":
            vals[outs[0]] = q(feed.pop(0))
            continue
        if typ == "pnnx.Attribute":
            vals[outs[0]] = q(a("data"))
            continue
        if typ == "pnnx.Output":
            results.append(np.ascontiguousarray(vals[ins[0]]))
            continue
        v = vals[ins[0]]
        if typ == "nn.Conv2d":
            y = conv2d_ref(v, q(a("weight")), a("bias") if prm["bias"] == "True" else None, tuple(_ints(prm["stride"])), tuple(_ints(prm["padding"])),
                           tuple(_ints(prm["dilation"])), int(prm["groups"]))
        elif typ == "F.conv2d":
            bias = np.asarray(builder.attrs[_producer(lines, ins[2]) + ".data"], np.float64) if len(ins) == 3 else None
            y = conv2d_ref(v, vals[ins[1]], bias, tuple(_ints(prm["stride"])), _padding_of(prm["padding"]), tuple(_ints(prm["dilation"])),
                           int(prm["groups"]))
        elif typ == "nn.ReLU":
            y = np.maximum(v, 0.0)
        elif typ == "nn.Sigmoid":
            y = 1.0 / (1.0 + np.exp(-v))
        elif typ == "nn.AdaptiveAvgPool2d":
            assert tuple(_ints(prm["output_size"])) == (1, 1)
            y = v.mean(axis=(2, 3), keepdims=True)
        elif typ in ("Tensor.view", "Tensor.reshape"):
            y = v.reshape(builder.shapes[outs[0]])
        else:
            raise NotImplementedError(typ)
        assert tuple(y.shape) == tuple(builder.shapes[outs[0]]), (typ, name, tuple(y.shape), builder.shapes[outs[0]])
        vals[outs[0]] = y if outs[0] in graph_outs else q(y)
    return results


def _producer(lines, operand):
    for typ, name, ins, outs, prm in lines:
        if operand in outs:
            return name
    raise KeyError(operand)
