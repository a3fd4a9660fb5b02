"""float64 restatements for the nn.GroupNorm / nn.InstanceNorm2d tests (test infrastructure, no product code).

group_norm_ref: torch's eval-mode semantics on an NHWC array -- per image and group the mean and the biased variance over the
h * w * cg elements, y = act((x - mean) / sqrt(var + eps) * gamma + beta).  tests/test_groupnorm_cpu.py pins it to
torch.nn.functional.group_norm / instance_norm; the GPU tests compare against it and need no torch.

eval_graph: up_reference.eval_graph's operator set (its conv, transposed-conv, resize references; the 2x2 pool and the channel
concat restated as there) plus nn.GroupNorm, nn.InstanceNorm2d and nn.SiLU, with the same rnd= hook for the fp16-storage
emulation (gamma and beta stay fp32 in the engine, so they are not rounded here either).
"""
import numpy as np

from ct_reference import _ints, _parse, conv_transpose2d_ref, round_f16  # noqa: F401  (round_f16 re-exported)
from up_reference import RESIZE_TYPES, conv2d_ref, resize_args, upsample_bilinear_ref, upsample_nearest_ref


def act_ref(y, act="none", act_param=0.0):
    y = np.asarray(y, np.float64)
    if act == "none":
        return y
    if act == "relu":
        return np.maximum(y, 0.0)
    if act == "silu":
        return y / (1.0 + np.exp(-y))
    if act == "sigmoid":
        return 1.0 / (1.0 + np.exp(-y))
    if act == "hardsigmoid":
        return np.clip(y / 6.0 + 0.5, 0.0, 1.0)
    if act == "hardswish":
        return y * np.clip(y / 6.0 + 0.5, 0.0, 1.0)
    if act == "leakyrelu":
        return np.where(y > 0.0, y, y * float(act_param))
    raise ValueError(act)


def group_norm_ref(x_nhwc, G, gamma=None, beta=None, eps=1e-5, act="none", act_param=0.0):
    """float64 nn.GroupNorm(G, C) in eval mode on an NHWC array (G = C: nn.InstanceNorm2d); gamma / beta None: 1 / 0"""
    x = np.asarray(x_nhwc, np.float64)
    n, h, w, c = x.shape
    assert G > 0 and c % G == 0, (c, G)
    v = x.reshape(n, h * w, G, c // G)
    mean = v.mean(axis=(1, 3), keepdims=True)
    var = ((v - mean) ** 2).mean(axis=(1, 3), keepdims=True)
    y = ((v - mean) / np.sqrt(var + float(eps))).reshape(n, h, w, c)
    if gamma is not None:
        y = y * np.asarray(gamma, np.float64)
    if beta is not None:
        y = y + np.asarray(beta, np.float64)
    return act_ref(y, act, act_param)


# (n, h, w, C, G): the op-level shape list of the GPU tests, and of the CPU pin to torch
SHAPES = [
    (2, 12, 10, 24, 3),     # vector path, pixel count not a tile multiple
    (2, 12, 10, 12, 4),     # cg = 3: vectors straddle groups
    (1, 9, 7, 6, 2),        # scalar path, odd cg
    (3, 5, 6, 7, 7),        # C % 4 != 0, instance form
    (2, 16, 16, 64, 64),    # instance form, vector path
    (1, 8, 8, 1024, 32),    # wide C, small slab
    (2, 48, 40, 32, 4),     # the general two-launch form
    (1, 1, 1, 8, 1),        # single pixel, one group of 8 channels
    (1, 1, 1, 8, 8),        # one element per group: act(beta) exactly
]
# beyond the issue's list: the two-launch form on the scalar path (cg = 3), and with more than one slice whose last is shorter
EXTRA_SHAPES = [(1, 40, 30, 6, 2), (2, 37, 29, 16, 2)]
OFFSET_SHAPES = [(2, 12, 10, 24, 3), (1, 64, 64, 8, 2), (1, 9, 7, 6, 2)]
HALF_SHAPES = SHAPES[:5] + [(2, 10, 6, 21, 3)]
TWO_LAUNCH = (2, 48, 40, 32, 4)


def shape_id(s):
    return "n%d_%dx%d_c%d_g%d" % tuple(s)


def operands(s, seed=0, offset=0.0):
    """(x, gamma, beta) for a shape; x = offset + U[-1, 1)"""
    n, h, w, c, g = s
    r = np.random.Generator(np.random.Philox(seed))
    x = (np.float32(offset) + (2.0 * r.random((n, h, w, c), dtype=np.float32) - 1.0)).astype(np.float32)
    gamma = (0.5 + r.random(c, dtype=np.float32)).astype(np.float32)
    beta = (r.random(c, dtype=np.float32) - 0.5).astype(np.float32)
    return x, gamma, beta


def eval_graph(builder, x_nhwc, rnd=None):
    """fp64 evaluation of a PnnxBuilder graph (NHWC tensors).  rnd: applied to the input, every conv weight / bias and every layer's
    output except the graph output (None: exact) -- the fp16-storage emulation, as up_reference.eval_graph."""
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
            y = conv2d_ref(x, q(a("weight")), b, _ints(prm["stride"]), _ints(prm["padding"]), _ints(prm["dilation"]))
        elif typ == "nn.ConvTranspose2d":
            b = q(a("bias")) if prm["bias"] == "True" else None
            y = conv_transpose2d_ref(x, q(a("weight")), b, _ints(prm["stride"]), _ints(prm["padding"]), _ints(prm["output_padding"]),
                                     _ints(prm["dilation"]))
        elif typ == "nn.BatchNorm2d":
            mean, var = np.float64(a("running_mean")), np.float64(a("running_var"))
            y = (x - mean) / np.sqrt(var + float(prm["eps"])) * np.float64(a("weight")) + np.float64(a("bias"))
        elif typ in ("nn.GroupNorm", "nn.InstanceNorm2d"):
            assert prm.get("track_running_stats", "False") == "False"
            affine = prm["affine"] == "True"
            groups = int(prm["num_groups"]) if typ == "nn.GroupNorm" else x.shape[-1]
            assert int(prm["num_channels"] if typ == "nn.GroupNorm" else prm["num_features"]) == x.shape[-1]
            y = group_norm_ref(x, groups, a("weight") if affine else None, a("bias") if affine else None, float(prm["eps"]))
        elif typ == "nn.ReLU":
            y = np.maximum(x, 0.0)
        elif typ == "nn.SiLU":
            y = act_ref(x, "silu")
        elif typ == "nn.MaxPool2d":
            k, s = _ints(prm["kernel_size"]), _ints(prm["stride"])
            assert k == s == (2, 2) and _ints(prm["padding"]) == (0, 0)
            n, h, w, c = x.shape
            y = x[:, :h // 2 * 2, :w // 2 * 2, :].reshape(n, h // 2, 2, w // 2, 2, c).max(axis=(2, 4))
        elif typ == "torch.cat":
            assert int(prm["dim"]) == 1
            y = np.concatenate([vals[i] for i in ins], axis=3)
        elif typ == "pnnx.Expression":
            assert prm["expr"] == "add(@0,@1)"
            y = vals[ins[0]] + vals[ins[1]]
        elif typ in RESIZE_TYPES:
            mode, kw, ac, rec = resize_args(prm)
            y = upsample_bilinear_ref(x, align_corners=ac, recompute=rec, **kw) if mode == "bilinear" else upsample_nearest_ref(x, **kw)
        else:
            raise NotImplementedError(typ)
        vals[outs[0]] = y if outs[0] in graph_outs else q(y)
    return result
