"""Reference for include/si_act.h (clamp / softplus / mish) in float64, the float32 emulations of the kernel's formulas and of the naive ones
(the control of tests/test_param_act_cpu.py), a torch-float64 evaluator of PnnxBuilder graphs that hold the new type strings, and the case
tables the CPU and the GPU file share."""
import os

import numpy as np

import elementwise_reference as er
from ct_reference import _ints, _parse, round_f16  # noqa: F401  (round_f16: the rnd= hook of the evaluators)
from reduce_reference import eval_expr

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "si_act.h")
OPS = ("clamp", "softplus", "mish")
OP_CODE = {"clamp": 0, "softplus": 1, "mish": 2}
PARAM_TYPES = ("nn.ReLU6", "F.relu6", "nn.Hardtanh", "F.hardtanh", "torch.clamp", "nn.Softplus", "F.softplus", "nn.Mish", "F.mish")
FUNCTIONAL_TWINS = {"F.relu": "nn.ReLU", "F.silu": "nn.SiLU", "F.sigmoid": "nn.Sigmoid", "F.hardsigmoid": "nn.Hardsigmoid",
                    "F.hardswish": "nn.Hardswish", "F.leaky_relu": "nn.LeakyReLU", "F.tanh": "nn.Tanh"}
MISH_CUT = 30.0
INF = float("inf")

# clamp bounds of the GPU file: ReLU6, Hardtanh, one open side each, lo > hi (hi everywhere), and the two zeros
CLAMP_BOUNDS = [(0.0, 6.0), (-1.0, 1.0), (-INF, 0.5), (0.1, INF), (2.0, -2.0), (-0.0, 0.0)]
# softplus (beta, threshold): torch's defaults, and betas whose product with x is exact in fp32 (a power of two), so that the bar measures the
# function and not the rounding of beta * x (include/si_act.h)
SOFTPLUS_PARAMS = [(1.0, 20.0), (0.5, 20.0), (2.0, 5.0)]
# what a half can hold exactly: the fp16 clamp is then equal bits
CLAMP_BOUNDS_F16 = [(0.0, 6.0), (-1.0, 1.0), (-INF, 0.5), (0.125, INF), (2.0, -2.0), (-0.0, 0.0)]


def kname(op, dtype, vec):
    """the string si_hip_param_act_kernel_name returns"""
    if np.dtype(dtype) == np.float16:
        return "param_act_kernel<%s, _Float16, %d>" % (op, 8 if vec else 1)
    return "param_act_kernel<%s, float, %d>" % (op, 4 if vec else 1)


def vectorised(shape, dtype, in_ld=None, out_ld=None, in_c_off=0, out_c_off=0, **_):
    """does a launch on 16-byte aligned buffers take 16-byte vectors?  (the rule of the header: the dense arm, or c, strides and offsets)"""
    v = 16 // np.dtype(dtype).itemsize
    c = shape[-1]
    in_ld, out_ld = in_ld or c, out_ld or c
    if in_c_off % v or out_c_off % v:
        return False
    if in_ld == c and out_ld == c and int(np.prod(shape)) % v == 0:
        return True
    return c % v == 0 and in_ld % v == 0 and out_ld % v == 0


def param_act_ref(op, x, p0=0.0, p1=0.0):
    """the three definitions of include/si_act.h in float64.  p0 / p1 enter as the fp32 values the descriptor holds."""
    x = np.asarray(x, np.float64)
    p0, p1 = float(np.float32(p0)), float(np.float32(p1))
    with np.errstate(all="ignore"):
        if op == "clamp":
            y = np.where(x < p0, p0, x)
            return np.where(y > p1, p1, y)
        if op == "softplus":
            z = p0 * x
            soft = (np.maximum(z, 0.0) + np.log1p(np.exp(-np.abs(z)))) / p0
            return np.where(z > p1, x, soft)
        assert op == "mish", op
        sp = np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))
        return x * np.tanh(sp)


def param_act_torch(op, x, p0=0.0, p1=0.0):
    """torch float64 on the same inputs (clamp: None for an infinite bound)"""
    import torch
    F = torch.nn.functional
    t = torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float64)))
    p0, p1 = float(np.float32(p0)), float(np.float32(p1))
    if op == "clamp":
        y = torch.clamp(t, None if p0 == -INF else p0, None if p1 == INF else p1)
    elif op == "softplus":
        y = F.softplus(t, p0, p1)
    else:
        y = F.mish(t)
    return y.numpy()


# ---- float32 emulations: every operation rounds to fp32, as the kernel's do (numpy's exp / log1p stand for the device's) -----------------------
def softplus_f32(x, beta=1.0, threshold=20.0, naive=False):
    f = np.float32
    x = np.asarray(x, f)
    with np.errstate(all="ignore"):
        z = f(beta) * x
        if naive:
            soft = np.log(f(1) + np.exp(z)) / f(beta)
        else:
            e = np.exp(-np.abs(z))
            u = f(1) + e
            log1p = np.log(u) - ((u - f(1)) - e) / u        # the kernel's log1p on [0, 1]: log of the rounded sum, corrected by its rounding error
            soft = (np.where(z > 0, z, f(0)) + log1p) / f(beta)
        return np.where(z > f(threshold), x, soft).astype(f)


def mish_f32(x, naive=False):
    f = np.float32
    x = np.asarray(x, f)
    with np.errstate(all="ignore"):
        if naive:
            return (x * np.tanh(np.where(x > f(20), x, np.log(f(1) + np.exp(x))))).astype(f)
        e = np.exp(np.minimum(x, f(MISH_CUT)))
        n = e * (e + f(2))
        return np.where(x > f(MISH_CUT), x, x * (n / (n + f(2)))).astype(f)


def clamp_f32(x, lo, hi):
    f = np.float32
    x = np.asarray(x, f)
    y = np.where(x < f(lo), f(lo), x)
    return np.where(y > f(hi), f(hi), y).astype(f)


# ---- graphs ------------------------------------------------------------------------------------------------------------------------------
def _num(prm, key, default):
    v = prm.get(key, "None")
    return default if v == "None" else float(np.float32(float(v)))


def act_of_line(typ, prm):
    """(op, p0, p1) of one of PARAM_TYPES as the layer reads the line"""
    if typ in ("nn.ReLU6", "F.relu6"):
        return "clamp", 0.0, 6.0
    if typ in ("nn.Hardtanh", "F.hardtanh"):
        return "clamp", _num(prm, "min_val", -1.0), _num(prm, "max_val", 1.0)
    if typ == "torch.clamp":
        return "clamp", _num(prm, "min", -INF), _num(prm, "max", INF)
    if typ in ("nn.Softplus", "F.softplus"):
        return "softplus", _num(prm, "beta", 1.0), _num(prm, "threshold", 20.0)
    assert typ in ("nn.Mish", "F.mish"), typ
    return "mish", 0.0, 0.0


def eval_graph(builder, x_nhwc, rnd=None):
    """torch-float64 evaluation of a PnnxBuilder graph, the scheme of reduce_reference.eval_graph / softmax_reference.eval_graph with the
    types of this feature added; NHWC in, NHWC (rank 4) or [n, features] out.  rnd: applied to the input, every weight / bias / statistic
    and every operator's output except the graph output (None: exact)."""
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
        typ = FUNCTIONAL_TWINS.get(typ, typ)
        if typ in PARAM_TYPES:
            op, p0, p1 = act_of_line(typ, prm)
            y = torch.from_numpy(param_act_ref(op, x.numpy(), p0, p1))
        elif typ == "nn.Conv2d":
            y = F.conv2d(x, a("weight"), a("bias") if prm["bias"] == "True" else None, _ints(prm["stride"]), _ints(prm["padding"]),
                         _ints(prm["dilation"]), int(prm["groups"]))
        elif typ == "nn.BatchNorm2d":
            y = F.batch_norm(x, a("running_mean"), a("running_var"), a("weight"), a("bias"), False, 0.0, float(prm["eps"]))
        elif typ == "nn.ReLU":
            y = F.relu(x)
        elif typ == "nn.SiLU":
            y = F.silu(x)
        elif typ == "nn.Sigmoid":
            y = torch.sigmoid(x)
        elif typ == "nn.Tanh":
            y = torch.tanh(x)
        elif typ == "nn.Hardswish":
            y = F.hardswish(x)
        elif typ == "nn.Hardsigmoid":
            y = F.hardsigmoid(x)
        elif typ == "nn.LeakyReLU":
            y = F.leaky_relu(x, float(np.float32(float(prm["negative_slope"]))))
        elif typ == "nn.AdaptiveAvgPool2d":
            y = F.adaptive_avg_pool2d(x, _ints(prm["output_size"]))
        elif typ == "torch.cat":
            y = torch.cat([vals[i] for i in ins], int(prm["dim"]))
        elif typ == "torch.chunk":
            for o, piece in zip(outs, torch.chunk(x, int(prm["chunks"]), int(prm["dim"]))):
                vals[o] = piece.contiguous()      # (views of the input: nothing is stored again)
            continue
        elif typ == "pnnx.Expression":
            y = eval_expr(prm["expr"], [vals[i] for i in ins], (lambda t: t) if outs[0] in graph_outs and rnd is None else qt)
        elif typ == "torch.flatten":
            y = torch.flatten(x, 1)
        elif typ == "nn.Linear":
            y = F.linear(x, a("weight"), a("bias") if prm["bias"] == "True" else None)
        else:
            raise NotImplementedError(typ)
        vals[outs[0]] = y if outs[0] in graph_outs else qt(y)
    r = result.numpy()
    return np.ascontiguousarray(r.transpose(0, 2, 3, 1)) if r.ndim == 4 else r


def one_op_graph(typ, shape_file=(2, 8, 5, 7), **params):
    """input -> one of PARAM_TYPES -> output.  params: the builder method's (min_val / max_val, min / max, beta / threshold)"""
    from simpleinfer_amd import modelgen as mg
    b = mg.PnnxBuilder(seed=5)
    method = {"relu6": b.relu6, "hardtanh": b.hardtanh, "clamp": b.clamp, "softplus": b.softplus, "mish": b.mish}[typ.split(".")[1].lower()]
    b.output(method(b.input(shape_file), functional=typ.startswith("F."), **params))
    return b


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
def fp32_inputs():
    """special values, the band where a sigmoid's exponential overflows, and a log-spaced sweep of both signs"""
    return np.concatenate([er.special_f32(), er.sigmoid_band(), er.wide_sweep("any")]).astype(np.float32)
