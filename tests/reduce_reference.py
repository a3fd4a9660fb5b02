"""Restatements for the reduction tests (test infrastructure, no product code).

reduce_ref: numpy float64 sum / mean / amax / amin over the NHWC axes of a bit mask (1 n, 2 h, 4 w, 8 c), keepdims; np.max / np.min
propagate a NaN, as torch.amax / torch.amin do.

reduce_f64_torch: torch.sum / torch.mean / torch.amax / torch.amin in float64 on the values the device sees (halves widened): the
independent yardstick.  tests/test_reduce_cpu.py pins the numpy rule to it, NaN positions as a mask.

nhwc_mask / expected_form / vectorised / kname: the rules of include/si_reduce.h restated, the switch values read from the header's enums.

The case tables of the GPU tests, and eval_graph: a torch-float64 evaluator of a PnnxBuilder graph for the four reduction type strings, the
operators of build_toy_timm_head / build_toy_cbam / build_toy_coordatt / build_toy_layernorm2d and the expression operators they use,
with the rnd= hook of softmax_reference.eval_graph for the fp16-storage emulation (applied after every operator an expression lowers to).
"""
import os
import re

import numpy as np

from ct_reference import _ints, _parse, round_f16  # noqa: F401  (round_f16 re-exported)
from reduction_reference import AXIS_C, AXIS_H, AXIS_N, AXIS_W, header_enum_of, kname_of, mask_axes, nhwc_mask, positions  # noqa: F401  (re-exported)

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "si_reduce.h")
REDUCE_TYPES = ("torch.mean", "torch.sum", "torch.amax", "torch.amin")
OPS = ("sum", "mean", "amax", "amin")
FORMS = ("row_group", "row_block", "col_lane", "col_coop")
MASKS = (8, 1, 2, 3, 4, 5, 6, 7)   # every supported mask: the channel axis alone, and every non-empty subset of {n, h, w}


header_enum = header_enum_of(HEADER)
kname = kname_of("reduce")


def out_shape(shape, axes):
    return tuple(1 if (axes >> a) & 1 else s for a, s in enumerate(shape))


def expected_form(shape, axes):
    """the form the header promises for an NHWC shape and mask"""
    if axes == AXIS_C:
        return "row_group" if shape[3] <= header_enum("SI_REDUCE_GROUP_MAX_C") else "row_block"
    assert axes & AXIS_C == 0
    outputs = (1 if axes & AXIS_H else shape[1]) * (1 if axes & AXIS_W else shape[2]) * shape[3]   # per image: a kept n is never counted
    coop = positions(shape, axes) >= header_enum("SI_REDUCE_COOP_MIN_POSITIONS") and outputs <= header_enum("SI_REDUCE_COOP_MAX_OUTPUTS")
    return "col_coop" if coop else "col_lane"


def vectorised(shape, axes, dtype, **views):
    """16-byte vectors: c, the input stride and offset -- and, for the col forms (which store vectors), the output's"""
    v = 16 // np.dtype(dtype).itemsize
    oc = 1 if axes & AXIS_C else shape[3]
    ks = [shape[3], views.get("in_ld") or shape[3], views.get("in_c_off", 0)]
    if not axes & AXIS_C:
        ks += [views.get("out_ld") or oc, views.get("out_c_off", 0)]
    return all(int(k) % v == 0 for k in ks)


def reduce_ref(x_nhwc, op, axes):
    x = np.asarray(x_nhwc, np.float64)
    fn = dict(sum=np.sum, mean=np.mean, amax=np.max, amin=np.min)[op]
    with np.errstate(invalid="ignore", over="ignore"):
        return fn(x, axis=mask_axes(axes), keepdims=True)


def reduce_f64_torch(x_nhwc, op, axes):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(np.asarray(x_nhwc, np.float64)))
    return getattr(torch, op)(t, dim=mask_axes(axes), keepdim=True).numpy()


# ---- the case tables ---------------------------------------------------------------------------------------------------------------------------
MASK_SHAPES = [(2, 5, 7, 8), (2, 5, 7, 6)]
ROW_PIXELS = (1, 3, 130)


def row_c():
    g = header_enum("SI_REDUCE_GROUP_MAX_C")
    return [1, 2, 3, 5, 8, 21, 63, 64, 65, 1000, g, g + 1, g + 8, 4099]


def coop_cases():
    """(shape, mask) around the col_lane / col_coop switch, kept channels 8 and 6: positions just below, at and just above
    SI_REDUCE_COOP_MIN_POSITIONS (one position per part, the other parts empty); 65 positions (parts of 2, the last one short, 31 empty)
    and 400 (parts of 7, the last one of 1, six empty); two reduced levels (n and w around a kept h) and two kept levels (n and w around
    a reduced h), where a part starts in the middle of a run; and the outputs rule at and above SI_REDUCE_COOP_MAX_OUTPUTS."""
    p, o = header_enum("SI_REDUCE_COOP_MIN_POSITIONS"), header_enum("SI_REDUCE_COOP_MAX_OUTPUTS")
    assert p == 32 and o % 64 == 0, "the shapes below are written for 32 positions"
    cases = []
    for c in (8, 6):
        cases += [((2, 31, 1, c), 6), ((2, 8, 4, c), 6), ((2, 3, 11, c), 6), ((2, 5, 13, c), 6), ((2, 20, 20, c), 6), ((2, 3, 33, c), 4),
                  ((3, 4, 30, c), 5), ((2, 70, 3, c), 2), ((70, 2, 3, c), 1), ((4, 4, 5, c), 7)]
    cases += [((1, o // 64, p, 64), 4), ((1, o // 64 + 1, p, 64), 4)]   # p positions; kept h x 64 channels of outputs
    return cases


def eval_expr(expr, args, q):
    """pnnx's prefix expression on torch tensors; q rounds every operator's result, as every lowered BinaryOp / UnaryOp stores its own"""
    import torch
    toks = re.findall(r"[^(),]+", expr)
    pos = [0]

    def term():
        t = toks[pos[0]]
        pos[0] += 1
        if t.startswith("@"):
            return args[int(t[1:])]
        if t in ("add", "sub", "mul", "div"):
            a, b = term(), term()
            return q(dict(add=torch.add, sub=torch.sub, mul=torch.mul, div=torch.div)[t](a, b))
        if t in ("square", "sqrt"):
            a = term()
            return q(a * a if t == "square" else torch.sqrt(a))
        return torch.tensor(float(np.float32(float(t))), dtype=torch.float64)   # a literal, as the loader's float

    r = term()
    assert pos[0] == len(toks), expr
    return r


def eval_graph(builder, x_nhwc, rnd=None):
    """torch-float64 evaluation of a PnnxBuilder graph; NHWC in, NHWC (rank 4) or [n, features] out.  rnd: applied to the input, every
    weight / bias and every operator's output except the graph output (None: exact)."""
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
        if typ in REDUCE_TYPES:
            dim = _ints(prm["dim"]) if prm["dim"].startswith("(") else int(prm["dim"])
            y = getattr(torch, typ.split(".")[1])(x, dim=dim, keepdim=prm.get("keepdim", "False") == "True")
        elif typ == "nn.Conv2d":
            y = F.conv2d(x, a("weight"), a("bias") if prm["bias"] == "True" else None, _ints(prm["stride"]), _ints(prm["padding"]),
                         _ints(prm["dilation"]), int(prm["groups"]))
        elif typ == "nn.ReLU":
            y = F.relu(x)
        elif typ == "nn.Sigmoid":
            y = torch.sigmoid(x)
        elif typ == "torch.cat":
            y = torch.cat([vals[i] for i in ins], int(prm["dim"]))
        elif typ == "pnnx.Expression":
            y = eval_expr(prm["expr"], [vals[i] for i in ins], (lambda t: t) if outs[0] in graph_outs and rnd is None else qt)
        elif typ == "nn.Linear":
            y = F.linear(x, a("weight"), a("bias") if prm["bias"] == "True" else None)
        else:
            raise NotImplementedError(typ)
        vals[outs[0]] = y if outs[0] in graph_outs else qt(y)
    r = result.numpy()
    return np.ascontiguousarray(r.transpose(0, 2, 3, 1)) if r.ndim == 4 else r
