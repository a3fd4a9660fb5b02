"""Restatements for the nn.Conv1d tests (test infrastructure, no product code).

conv1d_ref: numpy float64 of torch's rule, zero padding:
    y[n, oc, lo] = b[oc] + sum over c in the group, k < K of w[oc, c, k] * x[n, c, lo * s - pl + k * d]
padding is an int (both sides), 'valid', or 'same' (stride 1: d (K - 1) in all, the odd one on the right).  With rnd= (round_f16) the operands are
rounded to half, every sum stays float64, and the caller rounds the result ONCE: the fp16 restatement of the kernels' storage rule.

eval_graph: a float64 evaluator of a PnnxBuilder graph for the operator set of build_toy_quartznet / build_toy_conv_gru, with the rnd= hook of
tests/rnn_reference.py: applied to the input, every weight and every stored tensor (each layer's output except the graph outputs).
"""
import os
import re

import numpy as np

import rnn_reference as rr
from ct_reference import _ints, _parse, round_f16  # noqa: F401  (round_f16 re-exported)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "si_conv1d.h")
ENTRIES = ["si_hip_conv1d_f32", "si_hip_conv1d_f16", "si_hip_conv1d_weight_bytes", "si_hip_conv1d_pack_weights_f32", "si_hip_conv1d_pack_weights_f16",
           "si_hip_conv1d_kernel_name"]

# (N, C, L, OC, K, s, pad, d, g): the smallest shapes at which each mechanism can fail
DENSE_CASES = [
    (2, 4, 16, 16, 1, 1, 0, 1, 1),         # exactly one tile
    (1, 3, 17, 5, 3, 1, 1, 1, 1),          # nothing divides, one position past a tile
    (2, 8, 33, 24, 5, 2, 2, 1, 1),         # stride 2, 1.5 channel tiles
    (1, 16, 40, 32, 3, 1, "same", 4, 1),
    (1, 8, 20, 8, 4, 1, "same", 1, 1),     # right pad > left pad
    (2, 6, 9, 7, 9, 1, 4, 1, 1),           # K = L
    (1, 5, 8, 3, 11, 1, 5, 1, 1),          # K > L
    (1, 64, 130, 64, 3, 1, 1, 1, 1),       # several reduction chunks
    (3, 1, 50, 8, 7, 1, 3, 1, 1),          # C = 1
    (1, 32, 1, 16, 1, 1, 0, 1, 1),         # L = 1
    (2, 12, 21, 18, 3, 3, 0, 2, 3),        # groups 3
    (1, 4, 20, 8, 5, 1, 2, 1, 4),          # multiplier 2: the grouped dense form
]
DEPTHWISE_CASES = [
    (2, 8, 40, 8, 33, 1, 16, 1, 8),
    (1, 5, 19, 5, 3, 2, 1, 1, 5),
    (1, 16, 64, 16, 87, 1, 43, 1, 16),
]
CASES = DENSE_CASES + DEPTHWISE_CASES
# fp16: the dense subset with (C / g) % 8 == 0, one case whose rows are not 16-byte aligned, and the depthwise form (which has no such rule)
F16_CASES = [c for c in DENSE_CASES if (c[1] // c[8]) % 8 == 0] + [(1, 8, 17, 5, 3, 1, 1, 1, 1)] + DEPTHWISE_CASES
# 'same' with an even and an odd d (K - 1), beside the list above, for the CPU pin against torch
SAME_CASES = [(2, 3, 11, 4, 4, 1, "same", 1, 1), (2, 3, 11, 4, 3, 1, "same", 3, 1), (1, 4, 9, 4, 2, 1, "same", 3, 2), (1, 2, 7, 2, 5, 1, "valid", 1, 1)]


def case_id(c):
    return "N%d_C%d_L%d_OC%d_K%d_s%d_p%s_d%d_g%d" % c


def is_depthwise(c):
    return c[8] == c[1] == c[3]


def kname(case, dtype):
    return "conv1d_%s_kernel<%s>" % ("depthwise" if is_depthwise(case) else "dense", "_Float16" if np.dtype(dtype) == np.float16 else "float")


def header_fields():
    """(name, C type) of SiConv1dDesc's fields, in the header's order"""
    m = re.search(r"typedef struct SiConv1dDesc \{(.*?)\} SiConv1dDesc;", open(HEADER).read(), flags=re.S)
    body = re.sub(r"/\*.*?\*/", " ", m.group(1), flags=re.S)
    return [(n.strip(), typ) for typ, names in re.findall(r"\b(int|long long|float)\s+([^;]+);", body) for n in names.split(",")]


def pads(k, padding, d=1, s=1):
    if padding == "valid":
        return 0, 0
    if padding == "same":
        assert s == 1
        total = d * (k - 1)
        return total // 2, total - total // 2
    return int(padding), int(padding)


def out_len(l, k, s, padding, d):
    pl, pr = pads(k, padding, d, s)
    e = l + pl + pr - d * (k - 1) - 1
    return e // s + 1 if e >= 0 else 0


def operands(case, seed=0, dtype=np.float32, bias=True):
    """(x, w, b) of a case: x U(-1, 1) in `dtype`, w fp32 U(-a, a) with a = sqrt(3 / fan_in), b fp32 U(-0.5, 0.5) or None"""
    n, c, l, oc, k, s, p, d, g = case
    r = np.random.Generator(np.random.Philox(seed + 1000 * c + k))
    x = r.uniform(-1, 1, (n, c, l)).astype(np.float32).astype(dtype)
    a = np.sqrt(3.0 / ((c // g) * k))
    w = r.uniform(-a, a, (oc, c // g, k)).astype(np.float32)
    b = r.uniform(-0.5, 0.5, oc).astype(np.float32) if bias else None
    return x, w, b


def activation(act, v, param=0.0):
    v = np.asarray(v, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        if act == "none":
            return v
        if act == "relu":
            return np.where(np.isnan(v), v, np.maximum(v, 0.0))
        if act == "silu":
            return v / (1.0 + np.exp(-v))
        if act == "sigmoid":
            return 1.0 / (1.0 + np.exp(-v))
        if act == "hardsigmoid":
            return np.clip(v / 6.0 + 0.5, 0.0, 1.0)
        if act == "hardswish":
            return v * np.clip(v / 6.0 + 0.5, 0.0, 1.0)
        if act == "leakyrelu":
            return np.where(v > 0, v, v * param)
    raise NotImplementedError(act)


def conv1d_ref(x, w, b=None, stride=1, padding=0, dilation=1, groups=1, act="none", act_param=0.0, rnd=None):
    """float64 [N, OC, Lo]; rnd: applied to x and w (the bias is fp32 in the kernels and stays as given)"""
    q = rnd or (lambda a: np.asarray(a, np.float64))
    x, w = q(x), q(w)
    n, c, l = x.shape
    oc, cg, k = w.shape
    assert cg * groups == c and oc % groups == 0
    pl, pr = pads(k, padding, dilation, stride)
    lo = out_len(l, k, stride, padding, dilation)
    assert lo > 0
    xp = np.zeros((n, c, pl + l + max(pr, 0) + stride * lo + dilation * k), np.float64)   # (room behind: a window never leaves the array)
    xp[:, :, pl:pl + l] = x
    ocg = oc // groups
    y = np.zeros((n, oc, lo), np.float64)
    for g in range(groups):
        xs, ws = xp[:, g * cg:(g + 1) * cg], w[g * ocg:(g + 1) * ocg]
        for kk in range(k):
            win = xs[:, :, kk * dilation: kk * dilation + (lo - 1) * stride + 1: stride]          # [N, cg, Lo]
            y[:, g * ocg:(g + 1) * ocg] += np.einsum("oc,ncl->nol", ws[:, :, kk], win)
    if b is not None:
        y += np.asarray(b, np.float64)[None, :, None]
    return activation(act, y, act_param)


def conv1d_torch(x, w, b=None, stride=1, padding=0, dilation=1, groups=1):
    import torch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64)))
    p = padding if isinstance(padding, str) else int(padding)
    return torch.nn.functional.conv1d(t(x), t(w), None if b is None else t(b), stride, p, dilation, groups).numpy()


# ---- the weight images, stated in numpy ---------------------------------------------------------------------------------------
def dense_image(w, groups, half):
    """[group][oc tile][channel step][tap][g][x](8 halves): lane 16 g + x holds filter 16 tile + x of the group at channel 4 q + g (fp32) or
    channels 32 q + 8 g + 0..7 (fp16); filters and channels beyond the group's are zeros"""
    oc, cg, k = w.shape
    ocg = oc // groups
    tiles, per = (ocg + 15) // 16, 32 if half else 4
    steps = (cg + per - 1) // per
    full = np.zeros((groups, tiles * 16, steps * per, k), np.float16 if half else np.float32)
    full[:, :ocg, :cg] = w.reshape(groups, ocg, cg, k)
    if half:
        return full.reshape(groups, tiles, 16, steps, 4, 8, k).transpose(0, 1, 3, 6, 4, 2, 5)     # [grp][tile][q][k][g][x][j]
    return full.reshape(groups, tiles, 16, steps, 4, k).transpose(0, 1, 3, 5, 4, 2)               # [grp][tile][q][k][g][x]


# ---- graphs -----------------------------------------------------------------------------------------------------------------
def eval_graph(builder, x, rnd=None):
    """float64 evaluation of a PnnxBuilder graph in file order: the list of graph outputs, every tensor in file order (rank 3 as stored)"""
    q = rnd or (lambda a: np.asarray(a, np.float64))
    vals, results = {}, []
    lines = [_parse(ln) for ln in builder.lines]
    graph_outs = {ins[0] for typ, _, ins, _, _ in lines if typ == "pnnx.Output"}
    for typ, name, ins, outs, prm in lines:
        a = lambda k: builder.attrs["%s.%s" % (name, k)]
        if typ == "pnnx.Input":
            vals[outs[0]] = q(x)
            continue
        if typ == "pnnx.Output":
            results.append(np.ascontiguousarray(vals[ins[0]]))
            continue
        v = vals[ins[0]]
        if typ == "nn.Conv1d":
            p = prm["padding"] if prm["padding"] in ("same", "valid") else _ints(prm["padding"])[0]
            y = conv1d_ref(v, q(a("weight")), a("bias") if prm["bias"] == "True" else None, _ints(prm["stride"])[0], p, _ints(prm["dilation"])[0],
                           int(prm["groups"]))
        elif typ == "nn.ReLU":
            y = np.maximum(v, 0.0)
        elif typ == "nn.Hardtanh":
            y = np.clip(v, float(prm["min_val"]), float(prm["max_val"]))
        elif typ == "pnnx.Expression":
            assert prm["expr"] == "add(@0,@1)", prm["expr"]
            y = v + vals[ins[1]]
        elif typ == "Tensor.permute":
            y = np.ascontiguousarray(v.transpose(*_ints(prm["dims"])))
        elif typ == "nn.Linear":
            y = v @ q(a("weight")).T + (np.asarray(a("bias"), np.float64) if prm["bias"] == "True" else 0.0)
        elif typ == "nn.GRU":
            dirs = 2 if prm["bidirectional"] == "True" else 1
            w = rr.builder_weights(builder, name, "gru", int(prm["num_layers"]), dirs, prm["bias"] == "True")
            y = rr.rnn_ref("gru", v, w, prm["batch_first"] == "True", rnd=rnd)[0]
        else:
            raise NotImplementedError(typ)
        assert tuple(y.shape) == tuple(builder.shapes[outs[0]]), (typ, name, tuple(y.shape), builder.shapes[outs[0]])
        vals[outs[0]] = y if outs[0] in graph_outs else q(y)
    return results
