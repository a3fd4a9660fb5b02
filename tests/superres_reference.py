"""numpy restatements for the super-resolution tests (test infrastructure, no product code, no torch).

pixel_shuffle_ref: the index rule of include/si_superres.h as an explicit gather on an NHWC array of any dtype -- with q = i r + j,
shuffle: out[n, h r + i, w r + j, c] = in[n, h, w, c r r + q]; unshuffle: out[n, h, w, c r r + q] = in[n, h r + i, w r + j, c].
The gather moves array elements, so a NaN payload or a -0.0 comes out with the bits it went in with.  tests/test_superres_cpu.py
pins it to torch.nn.functional.pixel_shuffle / pixel_unshuffle bit for bit; the GPU tests compare against it and need no torch.

prelu_ref: y = x > 0 ? x : slope[ch] * x with the product in fp32 (one IEEE multiply: numpy's float32 product is the kernel's); an
fp16 input is widened, multiplied in fp32 and rounded once.

eval_graph: fp64 evaluation of a PnnxBuilder graph with the operators the three toy super-resolution models use, with the same
rnd= hook for the fp16-storage emulation that gn_reference.eval_graph and pad_reference.eval_graph have.
"""
import numpy as np

from ct_reference import _ints, _parse, round_f16  # noqa: F401  (round_f16 re-exported)
from up_reference import RESIZE_TYPES, conv2d_ref, resize_args, upsample_nearest_ref

SHUFFLE_TYPES = ("nn.PixelShuffle", "F.pixel_shuffle")
UNSHUFFLE_TYPES = ("nn.PixelUnshuffle", "F.pixel_unshuffle")
FIVE = SHUFFLE_TYPES + UNSHUFFLE_TYPES + ("nn.PReLU",)


def out_shape(shape_nhwc, r, inverse=False):
    n, h, w, c = shape_nhwc
    if inverse:
        assert h % r == 0 and w % r == 0, (shape_nhwc, r)
        return (n, h // r, w // r, c * r * r)
    assert c % (r * r) == 0, (shape_nhwc, r)
    return (n, h * r, w * r, c // (r * r))


def pixel_shuffle_ref(x_nhwc, r, inverse=False):
    """the rule on an NHWC array, element by element through an index map; the result has x's dtype and bits"""
    x = np.asarray(x_nhwc)
    n, oh, ow, oc = out_shape(x.shape, r, inverse)
    y = np.empty((n, oh, ow, oc), x.dtype)
    rr = r * r
    if not inverse:
        c = np.arange(oc)
        for i in range(r):
            for j in range(r):
                y[:, i::r, j::r, :] = x[:, :, :, c * rr + i * r + j]
    else:
        c = np.arange(x.shape[3])
        for i in range(r):
            for j in range(r):
                y[:, :, :, c * rr + i * r + j] = x[:, i::r, j::r, :]
    return y


def prelu_ref(x, slope):
    """x: fp32 or fp16, channels last; slope: 1 or C fp32 values.  fp32 arithmetic, the result in x's dtype (fp16: rounded once)"""
    x = np.asarray(x)
    s = np.asarray(slope, np.float32).reshape(-1)
    assert s.size in (1, x.shape[-1]), (s.size, x.shape)
    xf = x.astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        y = np.where(xf > 0, xf, s * xf)
    return y.astype(x.dtype)


def factor(typ, prm):
    return int(prm["upscale_factor" if typ in SHUFFLE_TYPES else "downscale_factor"])


def eval_graph(builder, x_nhwc, rnd=None):
    """fp64 evaluation of a PnnxBuilder graph (NHWC tensors).  rnd: applied to the input, every conv weight / bias and every layer's
    output except the graph output (None: exact) -- the fp16-storage emulation; BatchNorm's parameters and PReLU's slopes stay fp32,
    as in the engine."""
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
        if typ in SHUFFLE_TYPES or typ in UNSHUFFLE_TYPES:
            y = pixel_shuffle_ref(x, factor(typ, prm), typ in UNSHUFFLE_TYPES)
        elif typ == "nn.PReLU":
            w = np.asarray(a("weight"), np.float64)
            assert w.size == int(prm["num_parameters"]) and w.size in (1, x.shape[-1])
            y = np.where(x > 0, x, w * x)
        elif typ == "nn.LeakyReLU":
            y = np.where(x > 0, x, np.float64(np.float32(float(prm["negative_slope"]))) * x)
        elif typ == "nn.Tanh":
            y = np.tanh(x)
        elif typ == "nn.ReLU":
            y = np.maximum(x, 0.0)
        elif typ == "nn.Conv2d":
            b = q(a("bias")) if prm["bias"] == "True" else None
            y = conv2d_ref(x, q(a("weight")), b, _ints(prm["stride"]), _ints(prm["padding"]), _ints(prm["dilation"]))
        elif typ == "nn.BatchNorm2d":
            mean, var = np.asarray(a("running_mean"), np.float64), np.asarray(a("running_var"), np.float64)
            y = (x - mean) / np.sqrt(var + float(prm["eps"])) * np.asarray(a("weight"), np.float64) + np.asarray(a("bias"), np.float64)
        elif typ == "torch.cat":
            assert int(prm["dim"]) == 1
            y = np.concatenate([vals[i] for i in ins], axis=3)
        elif typ == "pnnx.Expression":
            assert prm["expr"] == "add(@0,@1)"
            y = vals[ins[0]] + vals[ins[1]]
        elif typ in RESIZE_TYPES:
            mode, kw, ac, rec = resize_args(prm)
            assert mode == "nearest", mode
            y = upsample_nearest_ref(x, **kw)
        else:
            raise NotImplementedError(typ)
        vals[outs[0]] = y if outs[0] in graph_outs else q(y)
    return result
