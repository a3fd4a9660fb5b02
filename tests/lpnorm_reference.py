"""Restatements for the Lp-norm tests (test infrastructure, no product code).

lpnorm_ref: numpy float64 torch.norm(p) over the NHWC axes of a bit mask (1 n, 2 h, 4 w, 8 c), keepdims, or F.normalize(p, eps) along the
one axis of the mask, on the values the device sees (halves widened).  tests/test_lpnorm_cpu.py pins it to torch float64.

lpnorm_f32: the float32 arithmetic of include/si_lpnorm.h restated in numpy, addition by addition in the header's documented order for
the form the launch takes -- lane j of a group adds items j, j + L, ...; a __shfl_xor butterfly is v[j] + v[j ^ off] for off = L / 2 .. 1;
a workgroup adds its four wave values in index order; a col_lane lane adds its positions in increasing (n, h, w) order.  The device's
result must have these bits.

expected_form / vectorised / kname / group_lanes: the form rules of the header restated, the switch values read from the header's enums.

chain_length and the bars: with A the longest chain of additions that order gives a set and u = 2^-24,
    p = 1    |sum - exact| <= A u |exact|            (non-negative terms: no cancellation; each addition rounds once)      bar (A + 1) u
    p = 2    the squares round once each, the sum as above, the square root halves the relative error and rounds once:
             (A + 1) / 2 + 1 <= A + 3 in units of u                                                                          bar (A + 3) u
    p = inf  a selection: exact
    normalize adds ONE rounding (the division) to the norm's bound; the fp16 entry adds 2^-11 relative for the one store rounding plus 2^-25
    absolute for subnormal halves.
The bars are derived for inputs with |x| in [2^-10, 2^10] (no overflow, no subnormal square) and are not fitted to a measurement.

eval_graph: a torch-float64 evaluator of build_toy_superpoint / build_toy_embedding_head with the rnd= hook of softmax_reference.eval_graph
for the fp16-storage emulation.
"""
import os

import numpy as np

from ct_reference import _ints, _parse, round_f16  # noqa: F401  (round_f16 re-exported)
from reduction_reference import AXIS_C, AXIS_H, AXIS_N, AXIS_W, header_enum_of, kname_of, mask_axes, nhwc_mask, positions  # noqa: F401  (re-exported)

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "si_lpnorm.h")
LPNORM_TYPES = ("F.normalize", "torch.norm")
MASKS = (8, 1, 2, 3, 4, 5, 6, 7)   # every supported mask: the channel axis alone, and every non-empty subset of {n, h, w}
PS = (1, 2, float("inf"))
U = 2.0 ** -24


header_enum = header_enum_of(HEADER)
kname = kname_of("lpnorm")


def out_shape(shape, axes, normalize=False):
    return tuple(shape) if normalize else tuple(1 if (axes >> a) & 1 else s for a, s in enumerate(shape))


# ---- float64 ---------------------------------------------------------------------------------------------------------------------------------
def norm_f64(x, p, axes):
    x = np.abs(np.asarray(x, np.float64))
    ax = mask_axes(axes)
    with np.errstate(invalid="ignore", over="ignore"):
        if p == 1:
            return x.sum(axis=ax, keepdims=True)
        if p == 2:
            return np.sqrt((x * x).sum(axis=ax, keepdims=True))
        return x.max(axis=ax, keepdims=True)   # (np.max keeps a NaN)


def lpnorm_ref(x, p, axes, normalize=False, eps=0.0):
    x = np.asarray(x, np.float64)
    n = norm_f64(x, p, axes)
    if not normalize:
        return n
    with np.errstate(invalid="ignore", divide="ignore"):
        return x / np.where(n < eps, np.float64(eps), n)


def lpnorm_f64_torch(x, p, axes, normalize=False, eps=0.0):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float64)))
    if normalize:
        return torch.nn.functional.normalize(t, p=float(p), dim=mask_axes(axes)[0], eps=eps).numpy()
    return torch.norm(t, p=float(p), dim=mask_axes(axes), keepdim=True).numpy()


# ---- the form rules ---------------------------------------------------------------------------------------------------------------------------
def expected_form(shape, axes, normalize=False):
    """the form the header promises for an NHWC shape and mask"""
    if axes == AXIS_C:
        c = shape[3]
        return "row_group" if c <= header_enum("SI_LPNORM_GROUP_MAX_C") else "row_block" if c <= header_enum("SI_LPNORM_BLOCK_MAX_C") else "row_block_2pass"
    assert axes & AXIS_C == 0
    return "col_lane_reg" if normalize and positions(shape, axes) <= header_enum("SI_LPNORM_COL_REG_POSITIONS") else "col_lane"


def vectorised(shape, axes, dtype, normalize=False, **views):
    """16-byte vectors: c, the input stride and offset -- and, unless the launch stores one element per pixel (a row form writing the norm),
    the output's"""
    v = 16 // np.dtype(dtype).itemsize
    oc = shape[3] if normalize or not axes & AXIS_C else 1
    ks = [shape[3], views.get("in_ld") or shape[3], views.get("in_c_off", 0)]
    if normalize or not axes & AXIS_C:
        ks += [views.get("out_ld") or oc, views.get("out_c_off", 0)]
    return all(int(k) % v == 0 for k in ks)


def expected_kernel(shape, axes, dtype, normalize=False, **views):
    return kname(expected_form(shape, axes, normalize), dtype, vectorised(shape, axes, dtype, normalize, **views))


def group_lanes(cv, vw):
    """lanes per row of row_group: the smallest power of two L with L * per >= cv, per = min(16 / vw, 4), at most 64"""
    per = min(16 // vw, 4)
    L = 1
    while L < 64 and L * per < cv:
        L *= 2
    return L


def chain_length(shape, axes, dtype, vec, normalize=False):
    """A: the additions on the longest path from an element to its set's sum, in the documented order of the form"""
    form = expected_form(shape, axes, normalize)
    if form.startswith("col"):
        return positions(shape, axes)
    vw = (16 // np.dtype(dtype).itemsize) if vec else 1
    cv = shape[3] // vw
    if form == "row_group":
        L = group_lanes(cv, vw)
        return -(-cv // L) * vw + int(np.log2(L))
    return -(-cv // 256) * vw + 6 + 3


def bar(shape, axes, p, dtype, vec, normalize=False):
    """(relative, absolute) bound of the device's result against float64, derived in the module docstring"""
    a = chain_length(shape, axes, dtype, vec, normalize)
    rel = 0.0 if p == float("inf") else (a + 1) * U if p == 1 else (a + 3) * U
    if normalize:
        rel += U
    if np.dtype(dtype) == np.float16:
        return rel + 2.0 ** -11, 2.0 ** -25
    return rel, 0.0


# ---- float32, addition by addition ---------------------------------------------------------------------------------------------------------------
def _prep(x, p):
    return x * x if p == 2 else np.abs(x)


def _combine(a, b, p):
    if p == float("inf"):
        with np.errstate(invalid="ignore"):
            return np.where((a != a) | (a > b), a, b)
    return a + b


def _butterfly(v, p):
    """v[..., lanes]: every lane's value after the xor exchanges lanes / 2 .. 1"""
    lanes = v.shape[-1]
    idx = np.arange(lanes)
    off = lanes >> 1
    while off > 0:
        v = _combine(v, v[..., idx ^ off], p)
        off >>= 1
    return v


def _finish(acc, p):
    with np.errstate(invalid="ignore"):
        return np.sqrt(acc) if p == 2 else acc


def _divide(x, norm, eps):
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.where(norm < np.float32(eps), np.float32(eps), norm).astype(np.float32)
        return (x / d).astype(np.float32)


def lpnorm_f32(x_nhwc, p, axes, normalize=False, eps=0.0, vec=None, **views):
    """the device's bits for an NHWC array of float32 or float16: float32 arithmetic in the order of the form, rounded once to the
    array's type.  vec: the instantiation (None: from the shape and the view keywords, as vectorised())"""
    x_nhwc = np.asarray(x_nhwc)
    dtype = x_nhwc.dtype
    assert dtype in (np.float32, np.float16)
    shape = x_nhwc.shape
    x = x_nhwc.astype(np.float32)
    if vec is None:
        vec = vectorised(shape, axes, dtype, normalize, **views)
    form = expected_form(shape, axes, normalize)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        if form.startswith("row"):
            c = shape[3]
            vw = (16 // dtype.itemsize) if vec else 1
            cv = c // vw
            L = group_lanes(cv, vw) if form == "row_group" else 256
            rows = x.reshape(-1, c)
            acc = np.zeros((rows.shape[0], L), np.float32)
            for i in range(-(-cv // L)):
                n = min(L, cv - i * L)
                for e in range(vw):
                    acc[:, :n] = _combine(acc[:, :n], _prep(rows[:, (i * L + np.arange(n)) * vw + e], p), p)
            if form == "row_group":
                norm = _butterfly(acc, p)[:, 0]
            else:
                w = _butterfly(acc.reshape(-1, 4, 64), p)[:, :, 0]
                norm = w[:, 0]
                for k in range(1, 4):
                    norm = _combine(norm, w[:, k], p)
            norm = _finish(norm.astype(np.float32), p).reshape(shape[:3] + (1,))
        else:
            red = mask_axes(axes)
            acc = np.zeros(out_shape(shape, axes), np.float32)
            for pos in np.ndindex(*[shape[a] for a in red]):   # (C order: increasing (n, h, w))
                sl = [slice(None)] * 4
                for a, k in zip(red, pos):
                    sl[a] = slice(k, k + 1)
                acc = _combine(acc, _prep(x[tuple(sl)], p), p)
            norm = _finish(acc.astype(np.float32), p)
        out = _divide(x, norm, eps) if normalize else norm
        return out.astype(dtype)


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------------
def ranged(shape, seed, dtype=np.float32):
    """values with |x| in [2^-10, 2^10], both signs, log-uniform: the range the bars are derived for"""
    r = np.random.RandomState(seed)
    v = np.exp2(r.uniform(-10.0, 10.0, size=shape)) * r.choice([-1.0, 1.0], size=shape)
    return v.astype(dtype)


def check_bar(got, want64, rel, absolute=0.0):
    """max over the elements of |got - want| - (rel |want| + abs) <= 0; returns the worst relative error for the print"""
    got = np.asarray(got, np.float64)
    if got.size == 0:
        return 0.0
    err = np.abs(got - want64)
    worst = float(np.max(err / np.maximum(np.abs(want64), 1e-300)))
    assert np.all(err <= rel * np.abs(want64) + absolute), (worst, rel, absolute)
    return worst


# ---- graphs ----------------------------------------------------------------------------------------------------------------------------------
def eval_graph(builder, x_nhwc, rnd=None, unstored=()):
    """torch-float64 evaluation of a PnnxBuilder graph; NHWC in; a list with one array per graph output, file order (NCHW / [N, H, W] /
    [N, F]).  rnd: applied to the input, every weight / bias and every operator's output except the graph outputs (None: exact) and the
    outputs of the operator types in `unstored`: the plan with fuse_norm writes no norm tensor, so its emulation passes ("torch.norm",)."""
    import torch
    F = torch.nn.functional
    q = rnd or (lambda a: np.asarray(a, np.float64))
    qt = lambda t: torch.from_numpy(np.ascontiguousarray(q(t.numpy())))
    vals, results = {}, []
    lines = [_parse(ln) for ln in builder.lines]
    graph_outs = {ins[0] for typ, _, ins, _, _ in lines if typ == "pnnx.Output"}
    for typ, name, ins, outs, prm in lines:
        a = lambda k: torch.from_numpy(np.ascontiguousarray(q(builder.attrs["%s.%s" % (name, k)])))
        if typ == "pnnx.Input":
            t = torch.from_numpy(np.ascontiguousarray(q(x_nhwc)))
            vals[outs[0]] = t.permute(0, 3, 1, 2).contiguous() if t.ndim == 4 else t
            continue
        if typ == "pnnx.Output":
            results.append(np.ascontiguousarray(vals[ins[0]].numpy()))
            continue
        x = vals[ins[0]]
        if typ == "torch.norm":
            dim = _ints(prm["dim"]) if prm["dim"].startswith("(") else int(prm["dim"])
            y = torch.norm(x, p=float(prm["p"]) if prm["p"] != "fro" else 2.0, dim=dim, keepdim=prm.get("keepdim", "False") == "True")
        elif typ == "F.normalize":
            y = F.normalize(x, p=float(prm["p"]), dim=int(prm["dim"]), eps=float(prm["eps"]))
        elif typ == "torch.mean":
            y = torch.mean(x, dim=_ints(prm["dim"]), keepdim=prm.get("keepdim", "False") == "True")
        elif typ == "nn.Conv2d":
            y = F.conv2d(x, a("weight"), a("bias") if prm["bias"] == "True" else None, _ints(prm["stride"]), _ints(prm["padding"]),
                         _ints(prm["dilation"]), int(prm["groups"]))
        elif typ == "nn.ReLU":
            y = F.relu(x)
        elif typ == "nn.MaxPool2d":
            y = F.max_pool2d(x, _ints(prm["kernel_size"]), _ints(prm["stride"]), _ints(prm["padding"]))
        elif typ == "nn.Softmax":
            y = torch.softmax(x, int(prm["dim"]))
        elif typ == "Tensor.slice":
            y = torch.narrow(x, int(prm["dim"]), int(prm["start"]), min(int(prm["end"]), x.shape[int(prm["dim"])]) - int(prm["start"]))
        elif typ == "Tensor.permute":
            y = x.permute(*_ints(prm["dims"]))
        elif typ == "Tensor.reshape":
            y = x.reshape(*_ints(prm["shape"]))
        elif typ == "torch.unsqueeze":
            y = torch.unsqueeze(x, int(prm["dim"]))
        elif typ == "pnnx.Expression":
            assert prm["expr"] in ("div(@0,@1)", "mul(@0,@1)"), prm["expr"]
            y = (torch.div if prm["expr"].startswith("div") else torch.mul)(vals[ins[0]], vals[ins[1]])
        elif typ == "nn.Linear":
            y = F.linear(x, a("weight"), a("bias") if prm["bias"] == "True" else None)
        else:
            raise NotImplementedError(typ)
        assert tuple(y.shape) == tuple(builder.shapes[outs[0]]), (typ, name, tuple(y.shape), builder.shapes[outs[0]])
        vals[outs[0]] = y if outs[0] in graph_outs or typ in ("Tensor.permute", "Tensor.reshape", "torch.unsqueeze", "Tensor.slice") + tuple(unstored) else qt(y)
    return results
