"""What the F.layer_norm / F.gelu tests share: the float64 rules (pinned to torch float64 by tests/test_layernorm_cpu.py) and the float64
evaluation of the toy graphs."""
import math
import os

import numpy as np

import attention_reference as atr
from ct_reference import _ints, _parse, round_f16  # noqa: F401  (round_f16 re-exported)
from reduction_reference import header_enum_of, kname_of

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "si_layernorm.h")
header_enum = header_enum_of(HEADER)
kname = kname_of("layernorm")


def layernorm_ref(x, gamma=None, beta=None, eps=1e-5):
    x = np.asarray(x, np.float64)
    d = x - x.mean(axis=-1, keepdims=True)
    y = d / np.sqrt((d * d).mean(axis=-1, keepdims=True) + np.float64(np.float32(eps)))
    if gamma is not None:
        y = y * np.asarray(gamma, np.float64)
    return y if beta is None else y + np.asarray(beta, np.float64)


def gelu_ref(x, approximate="none"):
    x = np.asarray(x, np.float64)
    with np.errstate(all="ignore"):
        if approximate == "tanh":
            # 0.5 x (1 + tanh(u)) = x / (1 + exp(-2u)): the same function, without float64's own cancellation in 1 + tanh(u) below u = -10
            return x / (1.0 + np.exp(-2.0 * math.sqrt(2.0 / math.pi) * (x + 0.044715 * x * x * x)))
        return 0.5 * x * np.vectorize(math.erfc, otypes=[np.float64])(-x / math.sqrt(2.0))


def expected_kernel(c, dtype, vec):
    g, b = header_enum("SI_LAYERNORM_GROUP_MAX_C"), header_enum("SI_LAYERNORM_BLOCK_MAX_C")
    return kname("row_group" if c <= g else "row_block" if c <= b else "row_block_3pass", dtype, vec)


def eval_graph(builder, x_nhwc, rnd=None):
    """float64 evaluation of a PnnxBuilder graph of the toy's operators, file order inside (NHWC in; tokens out).  rnd: applied to the input,
    the weights and every operator's output except the graph output -- wherever the engine stores a half (None: exact).  The constants of
    F.layer_norm stay fp32 under fp16 storage and are not rounded."""
    import torch
    F = torch.nn.functional
    q = lambda v: np.asarray(rnd(v) if rnd else v, np.float64)
    lines = [_parse(ln) for ln in builder.lines]
    consts = {outs[0]: builder.attrs[name + ".data"] for typ, name, _, outs, _ in lines if typ == "pnnx.Attribute"}
    vals = {}
    for typ, name, ins, outs, prm in lines:
        a = lambda k: torch.from_numpy(q(builder.attrs["%s.%s" % (name, k)]))
        bias = lambda k: a(k) if prm["bias"] == "True" else None
        x = torch.from_numpy(np.ascontiguousarray(vals[ins[0]])) if ins and ins[0] in vals else None
        if typ == "pnnx.Attribute":
            continue
        if typ == "pnnx.Output":
            return np.ascontiguousarray(vals[ins[0]])
        if typ == "pnnx.Input":
            y = np.ascontiguousarray(q(x_nhwc).transpose(0, 3, 1, 2))
        elif typ == "F.layer_norm":
            rest = [consts[i] for i in ins[1:]]
            gamma = rest.pop(0) if prm.get("weight") != "None" and rest else None
            y = layernorm_ref(vals[ins[0]], gamma, rest.pop(0) if rest else None, float(prm["eps"]))
        elif typ == "F.gelu":
            y = gelu_ref(vals[ins[0]], prm.get("approximate", "none"))
        elif typ == "nn.Conv2d":
            y = F.conv2d(x, a("weight"), bias("bias"), _ints(prm["stride"]), _ints(prm["padding"]), _ints(prm["dilation"]), int(prm["groups"])).numpy()
        elif typ == "Tensor.permute":
            y = x.permute(*_ints(prm["dims"])).contiguous().numpy()
        elif typ == "Tensor.view":
            y = x.reshape(*_ints(prm["shape"])).numpy()
        elif typ == "pnnx.Expression" and prm["expr"] == "add(@0,@1)":
            y = vals[ins[0]] + vals[ins[1]]
        elif typ == "nn.Linear":
            y = F.linear(x, a("weight"), bias("bias")).numpy()
        elif typ == "nn.MultiheadAttention":
            y = atr.mha_ref([vals[i] for i in ins], a("in_proj_weight").numpy(), bias("in_proj_bias").numpy(), a("out_proj.weight").numpy(),
                            bias("out_proj.bias").numpy(), int(prm["num_heads"]), prm["batch_first"] == "True", rnd=rnd)
        else:
            raise NotImplementedError(typ)
        assert tuple(y.shape) == tuple(builder.shapes[outs[0]]), (typ, name, y.shape)
        vals[outs[0]] = y if any(t == "pnnx.Output" and i[0] == outs[0] for t, _, i, _, _ in lines) else q(y)
