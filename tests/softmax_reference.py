"""Restatements for the softmax tests (test infrastructure, no product code).

softmax_ref: numpy float64 softmax / log_softmax along an NHWC axis with torch's special values: m = max over the axis (NaNs
skipped), s = sum exp(x - m); exp(x - m) / s or (x - m) - log(s).  A -inf element of a row with a finite maximum is exactly 0 (-inf for
the logarithm); a row whose maximum is +inf and a row of only -inf are NaN throughout (inf - inf); a NaN makes its own row NaN.

softmax_f64_torch: torch.softmax / torch.log_softmax in float64 on the values the device sees (halves widened): the independent
yardstick.  tests/test_softmax_cpu.py pins the numpy rule to it, NaN positions as a mask.

CONTIG_C / STRIDED_SHAPES / special_rows: the case tables of the GPU tests.

eval_graph: a torch-float64 evaluator of a PnnxBuilder graph for the five softmax type strings and the operators of build_toy_classifier,
build_toy_segnet and build_toy_unet, with the rnd= hook of pool_reference.eval_graph for the fp16-storage emulation.
"""
import os

import numpy as np

from ct_reference import _ints, _parse, round_f16  # noqa: F401  (round_f16 re-exported)
from reduction_reference import header_enum_of, kname_of

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "si_softmax.h")
SOFTMAX_TYPES = ("nn.Softmax", "nn.LogSoftmax", "nn.Softmax2d", "F.softmax", "F.log_softmax")
FORMS = ("group", "block", "block_online", "strided", "strided_online")


header_enum = header_enum_of(HEADER)
kname = kname_of("softmax")


def expected_form(shape, axis):
    """the form the header promises for an NHWC shape and axis"""
    if axis == 3:
        c = shape[3]
        return "group" if c <= header_enum("SI_SOFTMAX_GROUP_MAX_C") else "block" if c <= header_enum("SI_SOFTMAX_BLOCK_MAX_C") else "block_online"
    return "strided" if shape[axis] <= header_enum("SI_SOFTMAX_STRIDED_REG_A") else "strided_online"


def softmax_ref(x_nhwc, axis, log=False):
    x = np.asarray(x_nhwc, np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        m = np.fmax.reduce(x, axis=axis, keepdims=True)   # (fmax skips NaNs; an all-NaN row stays NaN)
        d = x - m
        e = np.exp(d)
        s = e.sum(axis=axis, keepdims=True)
        return d - np.log(s) if log else e / s


def softmax_f64_torch(x_nhwc, axis, log=False):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(np.asarray(x_nhwc, np.float64)))
    return (torch.log_softmax(t, axis) if log else torch.softmax(t, axis)).numpy()


def nhwc_axis(dim, rank):
    """torch's dim on an NCHW (or [N, F]) tensor -> the NHWC axis of the descriptor"""
    dim = dim + rank if dim < 0 else dim
    assert 0 <= dim < rank and rank in (2, 4), (dim, rank)
    return (0, 3)[dim] if rank == 2 else (0, 3, 1, 2)[dim]


def special_rows(c, dtype=np.float32):
    """[8, c] rows: 0 plain; 1 some -inf among finite values; 2 plain; 3 only -inf; 4 plain; 5 a +inf; 6 a NaN; 7 plain.  Rows 0, 2, 4
    and 7 are the neighbours that must stay untouched."""
    r = np.random.Generator(np.random.Philox(77))
    x = (r.random((8, c), dtype=np.float32) * 4 - 2).astype(np.float32)
    x[1, ::2] = -np.inf
    if c == 1:
        x[1, 0] = 0.5            # (a one-element row of -inf is row 3)
    x[3, :] = -np.inf
    x[5, c // 2] = np.inf
    x[6, c - 1] = np.nan
    return x.astype(dtype)


# contiguous axis: the channel counts of the GPU test (thresholds from the header), and the strided shapes
def contig_c():
    g, b = header_enum("SI_SOFTMAX_GROUP_MAX_C"), header_enum("SI_SOFTMAX_BLOCK_MAX_C")
    return [1, 2, 3, 5, 8, 21, 63, 64, 65, 1000, g, g + 1, b, b + 4, b + 5]


CONTIG_ROWS = (1, 3, 130)
STRIDED_SHAPES_F32 = [(2, 5, 7, 8), (2, 5, 7, 6), (3, 1, 33, 12), (2, 40, 3, 4), (3, 1, 33, 6)]   # (the last: the scalar online form)
STRIDED_SHAPES_F16 = [(2, 5, 7, 8), (2, 5, 7, 12), (2, 5, 7, 6), (3, 1, 33, 8), (3, 1, 33, 12), (2, 40, 3, 6)]


def eval_graph(builder, x_nhwc, rnd=None):
    """torch-float64 evaluation of a PnnxBuilder graph; NHWC in, NHWC (rank 4) or [n, features] out.  rnd: applied to the input, every
    weight / bias / statistic and every layer's output except the graph output (None: exact)."""
    import torch
    F = torch.nn.functional
    q = rnd or (lambda a: np.asarray(a, np.float64))
    qt = lambda t: torch.from_numpy(np.ascontiguousarray(q(t.numpy())))
    vals, result = {}, None
    lines = [_parse(ln) for ln in builder.lines]
    graph_outs = {ins[0] for typ, _, ins, _, _ in lines if typ == "pnnx.Output"}
    for typ, name, ins, outs, prm in lines:
        a = lambda k: torch.from_numpy(np.ascontiguousarray(q(builder.attrs["%s.%s" % (name, k)])))
        if typ == "pnnx.Input":
            t = torch.from_numpy(np.ascontiguousarray(q(x_nhwc)))
            vals[outs[0]] = t.permute(0, 3, 1, 2).contiguous() if t.ndim == 4 else t
            continue
        if typ == "pnnx.Output":
            result = vals[ins[0]]
            continue
        x = vals[ins[0]]
        if typ in SOFTMAX_TYPES:
            dim = -3 if typ == "nn.Softmax2d" else int(prm["dim"])
            y = torch.log_softmax(x, dim) if typ in ("nn.LogSoftmax", "F.log_softmax") else torch.softmax(x, dim)
        elif typ == "nn.Conv2d":
            y = F.conv2d(x, a("weight"), a("bias") if prm["bias"] == "True" else None, _ints(prm["stride"]), _ints(prm["padding"]),
                         _ints(prm["dilation"]), int(prm["groups"]))
        elif typ == "nn.ConvTranspose2d":
            y = F.conv_transpose2d(x, a("weight"), a("bias") if prm["bias"] == "True" else None, _ints(prm["stride"]), _ints(prm["padding"]),
                                   _ints(prm["output_padding"]), int(prm["groups"]), _ints(prm["dilation"]))
        elif typ == "nn.BatchNorm2d":
            y = F.batch_norm(x, a("running_mean"), a("running_var"), a("weight"), a("bias"), False, 0.0, float(prm["eps"]))
        elif typ == "nn.ReLU":
            y = F.relu(x)
        elif typ == "nn.Sigmoid":
            y = torch.sigmoid(x)
        elif typ == "nn.Hardswish":
            y = F.hardswish(x)
        elif typ == "nn.Hardsigmoid":
            y = F.hardsigmoid(x)
        elif typ == "nn.MaxPool2d":
            y = F.max_pool2d(x, _ints(prm["kernel_size"]), _ints(prm["stride"]), _ints(prm["padding"]))
        elif typ == "nn.AdaptiveAvgPool2d":
            y = F.adaptive_avg_pool2d(x, _ints(prm["output_size"]))
        elif typ == "torch.cat":
            y = torch.cat([vals[i] for i in ins], int(prm["dim"]))
        elif typ == "pnnx.Expression":
            assert prm["expr"] in ("add(@0,@1)", "mul(@0,@1)"), prm["expr"]
            y = vals[ins[0]] + vals[ins[1]] if prm["expr"].startswith("add") else vals[ins[0]] * vals[ins[1]]
        elif typ == "torch.flatten":
            y = torch.flatten(x, 1)
        elif typ == "nn.Linear":
            y = F.linear(x, a("weight"), a("bias") if prm["bias"] == "True" else None)
        elif typ in ("F.interpolate", "nn.Upsample"):
            assert prm["mode"] == "bilinear"
            ac = prm.get("align_corners", "None") == "True"
            if prm.get("size", "None") != "None":
                y = F.interpolate(x, size=_ints(prm["size"]), mode="bilinear", align_corners=ac)
            else:
                y = F.interpolate(x, scale_factor=tuple(float(v) for v in prm["scale_factor"].strip("()").split(",")), mode="bilinear", align_corners=ac)
        else:
            raise NotImplementedError(typ)
        vals[outs[0]] = y if outs[0] in graph_outs else qt(y)
    r = result.numpy()
    return np.ascontiguousarray(r.transpose(0, 2, 3, 1)) if r.ndim == 4 else r
