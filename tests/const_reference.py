"""Numpy restatement of the constant-operand kernel (include/si_binary.h, simpleinfer_amd/csrc/hip/binary_const.hip): fp32 arithmetic, one
stage or two, under fp16 storage one round-to-nearest-even to half after EACH stage.  Pure numpy: tests/test_const_cpu.py pins it without a
GPU, tests/test_gpu_const.py holds the HIP kernel to it bit for bit (add / sub / mul / div and their reversed forms are IEEE operations,
which numpy's fp32 arithmetic performs with the same single rounding; pow / atan2 are library functions and are compared with the parent
kernel si_hip_binary_f32 instead)."""
import itertools
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "si_binary.h")
ENTRIES = ["si_hip_binary_const_f32", "si_hip_binary_const_f16", "si_hip_binary_const_kernel_name"]

OPS = (0, 1, 2, 3, 6, 7, 8, 9, 10, 11)            # the ten BinaryOp codes
EXACT_OPS = (0, 1, 2, 3, 7, 8)                    # IEEE arithmetic: bit for bit against numpy
REVERSED = {0: 0, 2: 2, 1: 7, 7: 1, 3: 8, 8: 3, 6: 9, 9: 6, 10: 11, 11: 10}
MASKS = list(itertools.product((0, 1), repeat=4))  # per dimension: 1 the constant has x's extent, 0 it is broadcast


def stage_f32(op, v, c):
    """one stage in fp32: v and c are float32 arrays (c broadcasts); the result is float32 (numpy rounds each operation once)"""
    v, c = np.asarray(v, np.float32), np.asarray(c, np.float32)
    with np.errstate(all="ignore"):
        if op == 0: return v + c
        if op == 1: return v - c
        if op == 2: return v * c
        if op == 3: return v / c
        if op == 7: return c - v
        if op == 8: return c / v
        if op == 6: return np.power(v, c)
        if op == 9: return np.power(c, v)
        if op == 10: return np.arctan2(v, c)
        if op == 11: return np.arctan2(c, v)
    raise ValueError(op)


def kernel_ref(x, ops, consts):
    """out = ops[1](ops[0](x, consts[0]), consts[1]) as the kernel computes it: operands widened to fp32, every stage an fp32 operation, and
    -- when x is float16 -- the stage's result rounded to half (round-to-nearest-even, numpy's astype) before the next stage or the store"""
    x = np.asarray(x)
    half = x.dtype == np.float16
    v = x.astype(np.float32)
    for op, c in zip(ops, consts):
        c = np.asarray(c)
        assert c.dtype == x.dtype, (c.dtype, x.dtype)
        v = stage_f32(op, v, c.astype(np.float32))
        if half:
            with np.errstate(over="ignore"):
                v = v.astype(np.float16).astype(np.float32)
    return v.astype(x.dtype)


def const_shape(x_shape, mask):
    return tuple(d if m else 1 for d, m in zip(x_shape, mask))


def expected_form(x_shape, const_shapes):
    """the form si_hip_binary_const_kernel_name reports (binary_plan.h), for a grid that is not capped below one run: chan when every
    constant varies along d3 only, pixel when every constant is constant along d3, full otherwise.  A dimension of extent 1 has stride 0
    whatever the constant's shape says."""
    varies = [[c[i] != 1 for i in range(4)] for c in const_shapes]
    if all(not (v[0] or v[1] or v[2]) for v in varies):
        return "chan"
    if all(not v[3] for v in varies):
        return "pixel"
    return "full"


def special_values(dtype):
    """±0, ±Inf, NaN, subnormals, the ends of the finite range; 65504 (the largest half) with 15 and 16: 65504 + 15 rounds back to 65504,
    65504 + 16 = 65520 is the tie that round-to-nearest-even sends to Inf in half"""
    info = np.finfo(dtype)
    v = [0.0, 1.0, 0.5, 3.0, float(info.max), float(info.tiny), float(info.tiny) / 4, float(info.smallest_subnormal), 65504.0, 15.0, 16.0, 1e-3, 255.0]
    v = np.array(v, dtype)
    return np.concatenate([v, -v, np.array([np.inf, -np.inf, np.nan], dtype)]).astype(dtype)


# ---- graphs -----------------------------------------------------------------------------------------------------------------
_EXPR_BINARY = {"add": lambda a, b: a + b, "sub": lambda a, b: a - b, "mul": lambda a, b: a * b, "div": lambda a, b: a / b}
_EXPR_UNARY = {"exp": np.exp, "neg": lambda a: -a, "sqrt": np.sqrt}


def eval_expr(expr, args):
    """a pnnx.Expression string over its inputs: name(arg, ..) with add / sub / mul / div / exp / neg / sqrt, @k the k-th input, numeric
    literals.  Plain numpy broadcasting, which is torch's: shapes are right-aligned in file order."""
    pos = [0]

    def node():
        i = pos[0]
        j = i
        while j < len(expr) and expr[j] not in "(),":
            j += 1
        tok = expr[i:j]
        pos[0] = j
        if j < len(expr) and expr[j] == "(":
            pos[0] += 1
            operands = [node()]
            while expr[pos[0]] == ",":
                pos[0] += 1
                operands.append(node())
            assert expr[pos[0]] == ")", expr
            pos[0] += 1
            return _EXPR_BINARY[tok](*operands) if tok in _EXPR_BINARY else _EXPR_UNARY[tok](*operands)
        return args[int(tok[1:])] if tok.startswith("@") else np.float64(tok)

    y = node()
    assert pos[0] == len(expr), expr
    return y


def conv2d_groups_ref(x_nhwc, w_oihw, bias, stride, padding, groups):
    from ct_reference import conv2d_ref
    if groups == 1:
        return conv2d_ref(x_nhwc, w_oihw, bias, stride, padding)
    ic, oc = x_nhwc.shape[3] // groups, w_oihw.shape[0] // groups
    parts = [conv2d_ref(x_nhwc[..., g * ic:(g + 1) * ic], w_oihw[g * oc:(g + 1) * oc], None if bias is None else bias[g * oc:(g + 1) * oc], stride, padding)
             for g in range(groups)]
    return np.concatenate(parts, axis=3)


def eval_graph(builder, inputs, rnd=None):
    """float64 evaluation of a PnnxBuilder graph with the operators of the constant toys (simpleinfer_amd/modelgen.py): pnnx.Attribute,
    pnnx.Expression (eval_expr), Conv2d with groups, ReLU, SiLU, Tanh, torch.flatten, Tensor.permute, Linear, nn.MultiheadAttention
    (tests/attention_reference.py) and F.grid_sample (tests/grid_reference.py, coordinates in float64).  inputs: one array per graph input,
    rank 4 ones NHWC (as the engine takes them).  Values are held in FILE order; every graph output comes back as the engine stores it
    (rank 4: NHWC), in the file's order of outputs -- one array, or a list when there are several.  rnd: applied to the inputs, every
    weight, bias and constant and every operator's output -- except a graph output that a Conv2d or a Linear writes: under fp16 storage those
    two write the file's fp32 from their own epilogue, while any other producer of a graph output writes a half staging operand that a
    convert step widens (EngineImpl::InsertOutputCasts), so its result IS stored as a half (None: exact)."""
    from attention_reference import mha_ref
    from ct_reference import _ints, _parse
    from grid_reference import grid_sample_ref
    q = rnd or (lambda a: np.asarray(a, np.float64))
    to_file = lambda a: a.transpose(0, 3, 1, 2) if a.ndim == 4 else a
    to_nhwc = lambda a: a.transpose(0, 2, 3, 1) if a.ndim == 4 else a
    inputs = list(inputs) if isinstance(inputs, (list, tuple)) else [inputs]
    vals, results = {}, []
    lines = [_parse(ln) for ln in builder.lines]
    graph_outs = {ins[0] for typ, _, ins, _, _ in lines if typ == "pnnx.Output"}
    for typ, name, ins, outs, prm in lines:
        a = lambda k: builder.attrs["%s.%s" % (name, k)]
        if typ == "pnnx.Input":
            vals[outs[0]] = to_file(q(inputs.pop(0)))
            continue
        if typ == "pnnx.Attribute":
            vals[outs[0]] = q(a("data"))
            continue
        if typ == "pnnx.Output":
            results.append(np.ascontiguousarray(to_nhwc(vals[ins[0]])))
            continue
        x = vals[ins[0]]
        if typ == "nn.Conv2d":
            assert _ints(prm["dilation"]) == (1, 1)
            y = to_file(conv2d_groups_ref(to_nhwc(x), q(a("weight")), q(a("bias")) if prm["bias"] == "True" else None, _ints(prm["stride"]),
                                          _ints(prm["padding"]), int(prm["groups"])))
        elif typ == "nn.ReLU":
            y = np.maximum(x, 0.0)
        elif typ == "nn.SiLU":
            y = x / (1.0 + np.exp(-x))
        elif typ == "nn.Tanh":
            y = np.tanh(x)
        elif typ == "torch.flatten":
            y = x.reshape(x.shape[:int(prm["start_dim"])] + (-1,))
        elif typ == "Tensor.permute":
            y = x.transpose(_ints(prm["dims"]))
        elif typ == "nn.Linear":
            y = x @ q(a("weight")).T + (q(a("bias")) if prm["bias"] == "True" else 0.0)
        elif typ == "pnnx.Expression":
            y = eval_expr(prm["expr"], [vals[i] for i in ins])
        elif typ == "nn.MultiheadAttention":
            bias = prm["bias"] == "True"
            y = mha_ref([vals[i] for i in ins], q(a("in_proj_weight")), q(a("in_proj_bias")) if bias else None, q(a("out_proj.weight")),
                        q(a("out_proj.bias")) if bias else None, int(prm["num_heads"]), prm["batch_first"] == "True", rnd=rnd)
        elif typ == "F.grid_sample":
            y = to_file(grid_sample_ref(to_nhwc(x), vals[ins[1]], prm["mode"], prm["padding_mode"], prm["align_corners"] == "True", coords64=True))
        else:
            raise NotImplementedError(typ)
        assert tuple(y.shape) == tuple(builder.shapes[outs[0]]), (typ, name, y.shape, builder.shapes[outs[0]])
        vals[outs[0]] = y if outs[0] in graph_outs and typ in ("nn.Conv2d", "nn.Linear") else q(y)
    return results[0] if len(results) == 1 else results
