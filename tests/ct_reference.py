"""fp64 numpy restatements for the nn.ConvTranspose2d tests (test infrastructure, no product code).

conv_transpose2d_ref is torch's semantics in the SCATTER form -- for each tap (ky, kx),
  out[:, iy*sh - ph + ky*dh, ix*sw - pw + kx*dw, :] += x @ W[:, :, ky, kx]
-- a different algorithm from the kernel's gather / sub-pixel-phase form.  tests/test_conv_transpose_cpu.py pins it to
torch.nn.functional.conv_transpose2d; the GPU tests compare against it and need no torch.

eval_graph evaluates a PnnxBuilder graph (the toy U-Net's operator set) from the builder's own lines and attrs, in fp64, with an
optional rounding applied to the weights, biases, the input and every layer's output (the fp16-storage emulation).
"""
import numpy as np

import util

ACTS = {
    "none": lambda v, p: v,
    "relu": lambda v, p: np.maximum(v, 0.0),
    "silu": lambda v, p: v / (1.0 + np.exp(-v)),
    "sigmoid": lambda v, p: 1.0 / (1.0 + np.exp(-v)),
    "hardsigmoid": lambda v, p: np.clip(v / 6.0 + 0.5, 0.0, 1.0),
    "hardswish": lambda v, p: v * np.clip(v / 6.0 + 0.5, 0.0, 1.0),
    "leakyrelu": lambda v, p: np.where(v > 0, v, v * p),
}


def _pair(v):
    return (int(v), int(v)) if np.isscalar(v) else (int(v[0]), int(v[1]))


def out_hw(ih, iw, k, s, p, op, d):
    return ((ih - 1) * s[0] - 2 * p[0] + d[0] * (k[0] - 1) + op[0] + 1,
            (iw - 1) * s[1] - 2 * p[1] + d[1] * (k[1] - 1) + op[1] + 1)


def conv_transpose2d_ref(x_nhwc, w_iohw, bias=None, stride=(1, 1), padding=(0, 0), output_padding=(0, 0), dilation=(1, 1),
                         act="none", act_param=0.0):
    """fp64 NHWC result of torch.nn.ConvTranspose2d (groups 1), scatter form"""
    s, p, op, d = _pair(stride), _pair(padding), _pair(output_padding), _pair(dilation)
    x = np.asarray(x_nhwc, np.float64)
    w = np.asarray(w_iohw, np.float64)
    n, ih, iw, ic = x.shape
    wic, oc, kh, kw = w.shape
    assert wic == ic
    oh, ow = out_hw(ih, iw, (kh, kw), s, p, op, d)
    # canvas rows -ph .. oh + ph - 1 hold every scattered position ((ih - 1) * sh + (kh - 1) * dh <= oh + 2 ph - 1)
    canvas = np.zeros((n, oh + 2 * p[0], ow + 2 * p[1], oc), np.float64)
    for ky in range(kh):
        for kx in range(kw):
            contrib = x @ w[:, :, ky, kx]   # [n, ih, iw, oc]
            y0, x0 = ky * d[0], kx * d[1]
            canvas[:, y0:y0 + (ih - 1) * s[0] + 1:s[0], x0:x0 + (iw - 1) * s[1] + 1:s[1], :] += contrib
    out = canvas[:, p[0]:p[0] + oh, p[1]:p[1] + ow, :]
    if bias is not None:
        out = out + np.asarray(bias, np.float64)
    return ACTS[act](out, act_param)


def conv2d_ref(x_nhwc, w_oihw, bias, stride, padding):
    """fp64 NHWC conv2d (groups 1, dilation 1), tap by tap"""
    x = np.asarray(x_nhwc, np.float64)
    w = np.asarray(w_oihw, np.float64)
    n, ih, iw, ic = x.shape
    oc, _, kh, kw = w.shape
    (sh, sw), (ph, pw) = _pair(stride), _pair(padding)
    oh, ow = (ih + 2 * ph - kh) // sh + 1, (iw + 2 * pw - kw) // sw + 1
    xp = np.zeros((n, ih + 2 * ph, iw + 2 * pw, ic), np.float64)
    xp[:, ph:ph + ih, pw:pw + iw, :] = x
    out = np.zeros((n, oh, ow, oc), np.float64)
    for ky in range(kh):
        for kx in range(kw):
            out += xp[:, ky:ky + (oh - 1) * sh + 1:sh, kx:kx + (ow - 1) * sw + 1:sw, :] @ w[:, :, ky, kx].T
    if bias is not None:
        out = out + np.asarray(bias, np.float64)
    return out


def _parse(line):
    toks = line.split()
    typ, name, nin, nout = toks[0], toks[1], int(toks[2]), int(toks[3])
    ins, outs = toks[4:4 + nin], toks[4 + nin:4 + nin + nout]
    params = {}
    for t in toks[4 + nin + nout:]:
        if t[0] in "@#":
            continue
        k, v = t.split("=", 1)
        params[k] = v
    return typ, name, ins, outs, params


def _ints(v):
    return tuple(int(t) for t in v.strip("()").split(",") if t)


def eval_graph(builder, x_nhwc, rnd=None):
    """fp64 evaluation of a PnnxBuilder graph (NHWC tensors; operators: Conv2d, ConvTranspose2d, BatchNorm2d, ReLU, MaxPool2d, cat,
    Output).  rnd: applied to the input, every conv weight / bias and every layer's output except the graph output (None: exact)."""
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
        if typ == "nn.Conv2d":
            b = q(a("bias")) if prm["bias"] == "True" else None
            y = conv2d_ref(x, q(a("weight")), b, _ints(prm["stride"]), _ints(prm["padding"]))
        elif typ == "nn.ConvTranspose2d":
            b = q(a("bias")) if prm["bias"] == "True" else None
            y = conv_transpose2d_ref(x, q(a("weight")), b, _ints(prm["stride"]), _ints(prm["padding"]), _ints(prm["output_padding"]),
                                     _ints(prm["dilation"]))
        elif typ == "nn.BatchNorm2d":
            mean, var = np.float64(a("running_mean")), np.float64(a("running_var"))
            y = (x - mean) / np.sqrt(var + float(prm["eps"])) * np.float64(a("weight")) + np.float64(a("bias"))
        elif typ == "nn.ReLU":
            y = np.maximum(x, 0.0)
        elif typ == "nn.MaxPool2d":
            k, s = _ints(prm["kernel_size"]), _ints(prm["stride"])
            assert k == s == (2, 2) and _ints(prm["padding"]) == (0, 0)
            n, h, w, c = x.shape
            y = x[:, :h // 2 * 2, :w // 2 * 2, :].reshape(n, h // 2, 2, w // 2, 2, c).max(axis=(2, 4))
        elif typ == "torch.cat":
            assert int(prm["dim"]) == 1
            y = np.concatenate([vals[i] for i in ins], axis=3)
        else:
            raise NotImplementedError(typ)
        vals[outs[0]] = y if outs[0] in graph_outs else q(y)
    return result


def round_f16(a):
    return np.asarray(a, np.float64).astype(np.float16).astype(np.float64)


# (kernel, stride, padding, output_padding, dilation), (batch, h, w), (cin, cout): the op-level shape list of the GPU tests
SHAPES = [
    ((2, 2), (2, 2), (0, 0), (0, 0), (1, 1), (2, 16, 16), (64, 32)),
    ((2, 2), (2, 2), (0, 0), (0, 0), (1, 1), (1, 8, 8), (1024, 512)),
    ((3, 3), (2, 2), (1, 1), (1, 1), (1, 1), (2, 10, 14), (32, 48)),
    ((3, 3), (2, 2), (1, 1), (0, 0), (1, 1), (3, 9, 7), (16, 16)),
    ((4, 4), (2, 2), (1, 1), (0, 0), (1, 1), (2, 12, 12), (64, 64)),
    ((3, 3), (1, 1), (1, 1), (0, 0), (1, 1), (2, 11, 13), (32, 32)),
    ((1, 1), (2, 2), (0, 0), (0, 0), (1, 1), (2, 6, 6), (8, 8)),
    ((3, 3), (2, 2), (0, 0), (0, 0), (2, 2), (1, 7, 9), (16, 24)),
    ((3, 2), (2, 1), (1, 0), (1, 0), (1, 1), (2, 8, 10), (12, 20)),
]


def shape_id(s):
    k, st, p, op, d, (n, h, w), (ci, co) = s
    return "k%dx%d_s%dx%d_p%dx%d_op%dx%d_d%dx%d_n%d_%dx%d_%d-%d" % (*k, *st, *p, *op, *d, n, h, w, ci, co)


def operands(s, seed=0):
    k, st, p, op, d, (n, h, w), (ci, co) = s
    x = util.rng_uniform(seed, (n, h, w, ci), -1.0, 1.0)
    a = np.sqrt(3.0 / (ci * k[0] * k[1]))
    wt = util.rng_uniform(seed + 1, (ci, co, k[0], k[1]), -a, a)
    b = util.rng_uniform(seed + 2, (co,), -0.1, 0.1)
    return x, wt, b
