"""numpy restatements for the chunk / split / slice tests (test infrastructure, no product code, no torch).

chunk_ref / split_ref / slice_ref: torch.chunk, torch.split and Tensor.slice on an NHWC array (or [N, F]) of any dtype, `dim` being the
NCHW dimension the file names (negative: from the end).  They index the array, so a NaN payload or a -0.0 comes out with the bits it went in
with.  tests/test_slice_cpu.py pins them to torch.chunk / torch.split / Python slicing on CPU torch; the GPU tests compare against them
and need no torch.

eval_graph: fp64 evaluation of a PnnxBuilder graph with the operators the four toy models and the planner graphs use, with the same rnd=
hook for the fp16-storage emulation that superres_reference.eval_graph has.
"""
import numpy as np

from ct_reference import _ints, _parse, round_f16  # noqa: F401  (round_f16 re-exported)
from up_reference import conv2d_ref

THREE = ("torch.chunk", "torch.split", "Tensor.slice")
OPEN_END = 2147483647   # what pnnx writes for an open end


def nhwc_axis(dim, rank):
    """the array axis of the file's NCHW dimension: rank 4 0 -> 0, 1 -> 3, 2 -> 1, 3 -> 2; rank 2 stays"""
    dim = dim + rank if dim < 0 else dim
    assert 0 <= dim < rank, (dim, rank)
    return (0, 3, 1, 2)[dim] if rank == 4 else dim


def chunk_lengths(size, chunks):
    """torch.chunk: pieces of ceil(size / chunks); the last may be smaller and there may be fewer than `chunks`"""
    assert chunks >= 1
    each = -(-size // chunks)
    return [min(each, size - at) for at in range(0, size, each)]


def split_lengths(size, split_size_or_sections):
    if isinstance(split_size_or_sections, (int, np.integer)):
        each = int(split_size_or_sections)
        assert each >= 1
        return [min(each, size - at) for at in range(0, size, each)]
    lens = [int(v) for v in split_size_or_sections]
    assert sum(lens) == size, (lens, size)
    return lens


def _cut(x, axis, lens):
    x = np.asarray(x)
    out, at = [], 0
    for n in lens:
        idx = [slice(None)] * x.ndim
        idx[axis] = slice(at, at + n)
        out.append(np.ascontiguousarray(x[tuple(idx)]))
        at += n
    return out


def chunk_ref(x, chunks, dim=1):
    x = np.asarray(x)
    axis = nhwc_axis(dim, x.ndim)
    return _cut(x, axis, chunk_lengths(x.shape[axis], chunks))


def split_ref(x, split_size_or_sections, dim=1):
    x = np.asarray(x)
    axis = nhwc_axis(dim, x.ndim)
    return _cut(x, axis, split_lengths(x.shape[axis], split_size_or_sections))


def slice_index(shape, dims, starts, ends, steps):
    """the tuple of Python slices (array order) of Tensor.slice over the NCHW dimensions `dims`; an end of None / OPEN_END is the size"""
    idx = [slice(None)] * len(shape)
    for d, s0, e, st in zip(dims, starts, ends, steps):
        assert st >= 1, st
        idx[nhwc_axis(d, len(shape))] = slice(0 if s0 is None else int(s0), None if e is None else int(e), int(st))
    return tuple(idx)


def slice_ref(x, dims, starts, ends, steps):
    x = np.asarray(x)
    one = isinstance(dims, (int, np.integer))
    dims, starts, ends, steps = ((v,) if one else tuple(v) for v in (dims, starts, ends, steps))
    return np.ascontiguousarray(x[slice_index(x.shape, dims, starts, ends, steps)])


def _opt(v):
    return None if v == "None" else int(v)


def apply_line(typ, prm, x):
    """the outputs (a list) of one torch.chunk / torch.split / Tensor.slice line of a .param file on the array x"""
    if typ == "torch.chunk":
        return chunk_ref(x, int(prm["chunks"]), int(prm["dim"]))
    if typ == "torch.split":
        v = prm["split_size_or_sections"]
        return split_ref(x, _ints(v) if v.startswith("(") else int(v), int(prm["dim"]))
    assert typ == "Tensor.slice", typ
    if "dims" in prm:
        k = len(_ints(prm["dims"]))
        many = lambda key, dflt: [_opt(t) for t in prm[key].strip("()").split(",")] if key in prm else [dflt] * k
        return [slice_ref(x, _ints(prm["dims"]), many("starts", 0), many("ends", None), many("steps", 1))]
    return [slice_ref(x, int(prm["dim"]), _opt(prm.get("start", "0")) or 0, _opt(prm.get("end", "None")), _opt(prm.get("step", "1")) or 1)]


def grouped_conv2d_ref(x, w, bias, stride, padding, dilation, groups):
    if groups == 1:
        return conv2d_ref(x, w, bias, stride, padding, dilation)
    ic, oc = x.shape[3] // groups, w.shape[0] // groups
    ys = [conv2d_ref(x[..., g * ic:(g + 1) * ic], w[g * oc:(g + 1) * oc], None if bias is None else bias[g * oc:(g + 1) * oc], stride, padding,
                     dilation) for g in range(groups)]
    return np.concatenate(ys, axis=3)


def maxpool2d_ref(x, k, s, p):
    """nn.MaxPool2d on an NHWC array (dilation 1, floor mode): the padding never wins"""
    n, h, w, c = x.shape
    xp = np.full((n, h + 2 * p[0], w + 2 * p[1], c), -np.inf, np.float64)
    xp[:, p[0]:p[0] + h, p[1]:p[1] + w] = x
    oh, ow = (h + 2 * p[0] - k[0]) // s[0] + 1, (w + 2 * p[1] - k[1]) // s[1] + 1
    y = np.full((n, oh, ow, c), -np.inf, np.float64)
    for dy in range(k[0]):
        for dx in range(k[1]):
            y = np.maximum(y, xp[:, dy:dy + (oh - 1) * s[0] + 1:s[0], dx:dx + (ow - 1) * s[1] + 1:s[1]])
    return y


def eval_graph(builder, x_nhwc, rnd=None):
    """fp64 evaluation of a PnnxBuilder graph (NHWC tensors; [N, F] behind a flatten).  rnd: applied to the input, every conv / linear weight
    and bias and every layer's output except the graph outputs (None: exact) -- the fp16-storage emulation.  Returns the graph output, or the
    list of them when the graph has several."""
    q = rnd or (lambda a: np.asarray(a, np.float64))
    vals, results = {}, []
    lines = [_parse(ln) for ln in builder.lines]
    graph_outs = {ins[0] for typ, _, ins, _, _ in lines if typ == "pnnx.Output"}
    for typ, name, ins, outs, prm in lines:
        a = lambda k: builder.attrs["%s.%s" % (name, k)]
        if typ == "pnnx.Input":
            vals[outs[0]] = q(x_nhwc)
            continue
        if typ == "pnnx.Output":
            results.append(vals[ins[0]])
            continue
        x = vals[ins[0]]
        if typ in THREE:
            ys = apply_line(typ, prm, x)             # (a piece of a rounded tensor is already rounded)
            assert len(ys) == len(outs), (typ, len(ys), len(outs))
            for o, y in zip(outs, ys):
                vals[o] = y
            continue
        if typ == "nn.Conv2d":
            b = q(a("bias")) if prm["bias"] == "True" else None
            y = grouped_conv2d_ref(x, q(a("weight")), b, _ints(prm["stride"]), _ints(prm["padding"]), _ints(prm["dilation"]), int(prm["groups"]))
        elif typ == "nn.SiLU":
            y = x / (1.0 + np.exp(-x))
        elif typ == "nn.ReLU":
            y = np.maximum(x, 0.0)
        elif typ == "torch.cat":
            y = np.concatenate([vals[i] for i in ins], axis=nhwc_axis(int(prm["dim"]), x.ndim))
        elif typ == "pnnx.Expression":
            assert prm["expr"] in ("add(@0,@1)", "mul(@0,@1)"), prm["expr"]
            y = vals[ins[0]] + vals[ins[1]] if prm["expr"].startswith("add") else vals[ins[0]] * vals[ins[1]]   # (numpy broadcasts [N,1,1,C])
        elif typ == "nn.Hardsigmoid":
            y = np.clip(x + 3.0, 0.0, 6.0) / 6.0
        elif typ == "nn.MaxPool2d":
            y = maxpool2d_ref(x, _ints(prm["kernel_size"]), _ints(prm["stride"]), _ints(prm["padding"]))
        elif typ == "nn.Upsample":
            assert prm["mode"] == "nearest" and prm["size"] == "None", prm
            sh, sw = (float(v) for v in prm["scale_factor"].strip("()").split(","))
            assert sh == int(sh) and sw == int(sw), prm    # (whole factors: torch's nearest index rule is then a repeat)
            y = np.repeat(np.repeat(x, int(sh), axis=1), int(sw), axis=2)
        elif typ == "nn.AdaptiveAvgPool2d":
            assert _ints(prm["output_size"]) == (1, 1)
            y = x.mean(axis=(1, 2), keepdims=True)
        elif typ == "torch.flatten":
            y = np.transpose(x, (0, 3, 1, 2)).reshape(x.shape[0], -1)
        elif typ == "nn.Linear":
            y = x @ q(a("weight")).T + (q(a("bias")) if prm["bias"] == "True" else 0.0)
        else:
            raise NotImplementedError(typ)
        vals[outs[0]] = y if outs[0] in graph_outs else q(y)
    return results[0] if len(results) == 1 else results
