"""Restatements for the attention tests (test infrastructure, no product code).

attention_ref: numpy float64 scaled dot-product attention on token arrays [L, N, E] / [N, L, E] split into heads, with torch's special
values: m = the row maximum of the scaled scores (NaNs skipped), p = exp(s - m), out = (p @ v) / sum p.  A NaN score makes its row NaN;
0 * NaN in p @ v is NaN, so a NaN in V poisons its column.

mha_ref / mha_torch: nn.MultiheadAttention from its four parameter arrays, in numpy on top of attention_ref and as the torch module in
float64 with the same weights.  sdpa_torch: F.scaled_dot_product_attention in a chosen dtype on the same token arrays.
tests/test_attention_cpu.py pins the numpy rule to both.

kernel_cases / D_F32 / D_F16 / LENGTHS: the case tables of the GPU tests.

eval_graph: a float64 evaluator of a PnnxBuilder graph for the operator set of build_toy_c3tr and build_toy_mhsa_head, with an rnd= hook
for the fp16-storage emulation: applied to the input, every weight and every stored tensor -- each layer's output except the graph output
and, inside nn.MultiheadAttention, the Q | K | V workspace, P and the attention output.
"""
import os
import re

import numpy as np

from ct_reference import _ints, _parse, round_f16  # noqa: F401  (round_f16 re-exported)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "si_attention.h")
ENTRIES = ["si_hip_attention_f32", "si_hip_attention_f16", "si_hip_attention_kernel_name"]
ABSENT_TYPES = ("F.scaled_dot_product_attention", "nn.LayerNorm", "nn.TransformerEncoderLayer", "nn.GELU", "torch.matmul", "torch.bmm")


def header_enum(name):
    return int(re.search(r"\b%s = (\d+)" % name, open(HEADER).read()).group(1))


def kname(d, dtype):
    """the instantiation the header promises for head dim d"""
    half = np.dtype(dtype) == np.float16
    dp = 32 if half else 16
    while dp < d:
        dp *= 2
    return "attention_kernel<%s, %d>" % ("_Float16" if half else "float", dp)


def heads_of(t, heads, batch_first):
    """[L, N, E] / [N, L, E] -> [N, heads, L, d] float64"""
    t = np.asarray(t, np.float64)
    if not batch_first:
        t = t.transpose(1, 0, 2)
    n, l, e = t.shape
    return t.reshape(n, l, heads, e // heads).transpose(0, 2, 1, 3)


def tokens_of(t, batch_first):
    """[N, heads, L, d] -> [L, N, E] / [N, L, E]"""
    n, h, l, d = t.shape
    t = t.transpose(0, 2, 1, 3).reshape(n, l, h * d)
    return np.ascontiguousarray(t if batch_first else t.transpose(1, 0, 2))


def attention_parts(q, k, v, heads, scale=None, batch_first=False, rnd_p=None):
    """(out, sum_j p_j |v_j|) as token arrays; rnd_p: applied to the normalised-by-maximum p before both sums (the fp16 kernel's P)"""
    qh, kh, vh = (heads_of(t, heads, batch_first) for t in (q, k, v))
    d = qh.shape[-1]
    scale = 1.0 / np.sqrt(d) if scale is None else float(scale)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        s = scale * (qh @ kh.transpose(0, 1, 3, 2))
        m = np.fmax.reduce(s, axis=-1, keepdims=True)
        p = np.exp(s - m)
        if rnd_p is not None:
            p = rnd_p(p)
        l = p.sum(axis=-1, keepdims=True)
        out = (p @ vh) / l
        mag = ((p / l) @ np.abs(vh))
    return tokens_of(out, batch_first), tokens_of(mag, batch_first)


def attention_ref(q, k, v, heads, scale=None, batch_first=False):
    return attention_parts(q, k, v, heads, scale, batch_first)[0]


def sdpa_torch(q, k, v, heads, scale=None, batch_first=False, dtype=np.float64):
    """torch.nn.functional.scaled_dot_product_attention on the CPU, computed in `dtype`, returned as float64 tokens"""
    import torch
    tq, tk, tv = (torch.from_numpy(np.ascontiguousarray(heads_of(t, heads, batch_first).astype(dtype))) for t in (q, k, v))
    out = torch.nn.functional.scaled_dot_product_attention(tq, tk, tv, scale=scale)
    return tokens_of(out.numpy().astype(np.float64), batch_first)


def mha_ref(inputs, w_in, b_in, w_out, b_out, heads, batch_first=False, rnd=None):
    """nn.MultiheadAttention's attention output from 1, 2 or 3 token arrays; rnd: the fp16-storage emulation (the Q | K | V workspace, P and
    the attention output are rounded; the caller rounds the operands, the weights and the result)"""
    r = rnd or (lambda a: a)
    xs = [np.asarray(t, np.float64) for t in inputs]
    xq, xk = xs[0], xs[1] if len(xs) > 1 else xs[0]
    xv = xs[2] if len(xs) > 2 else xk
    w_in, w_out = np.asarray(w_in, np.float64), np.asarray(w_out, np.float64)
    e = w_out.shape[0]
    b_in = np.zeros(3 * e) if b_in is None else np.asarray(b_in, np.float64)
    b_out = np.zeros(e) if b_out is None else np.asarray(b_out, np.float64)
    q, k, v = (r(x @ w_in[j * e:(j + 1) * e].T + b_in[j * e:(j + 1) * e]) for j, x in enumerate((xq, xk, xv)))
    att = r(attention_parts(q, k, v, heads, None, batch_first, rnd_p=rnd)[0])
    return att @ w_out.T + b_out


def mha_torch(inputs, w_in, b_in, w_out, b_out, heads, batch_first=False):
    """torch.nn.MultiheadAttention in float64 with these weights (need_weights=False)"""
    import torch
    e = np.asarray(w_out).shape[0]
    m = torch.nn.MultiheadAttention(e, heads, bias=b_in is not None, batch_first=batch_first, dtype=torch.float64).eval()
    with torch.no_grad():
        m.in_proj_weight.copy_(torch.from_numpy(np.asarray(w_in, np.float64)))
        m.out_proj.weight.copy_(torch.from_numpy(np.asarray(w_out, np.float64)))
        if b_in is not None:
            m.in_proj_bias.copy_(torch.from_numpy(np.asarray(b_in, np.float64)))
            m.out_proj.bias.copy_(torch.from_numpy(np.asarray(b_out, np.float64)))
        ts = [torch.from_numpy(np.ascontiguousarray(np.asarray(t, np.float64))) for t in inputs]
        q, k = ts[0], ts[1] if len(ts) > 1 else ts[0]
        v = ts[2] if len(ts) > 2 else k
        return m(q, k, v, need_weights=False)[0].numpy()


# ---- case tables ------------------------------------------------------------------------------------------------------------
D_F32 = (1, 3, 4, 8, 16, 20, 32, 64, 128)
D_F16 = (8, 16, 32, 64, 128)
LENGTHS = (1, 15, 16, 17, 63, 64, 65, 129, 200)


def kernel_cases(ds, seed=11):
    """(d, lq, lk, heads, batch): a seeded subset of the full table that covers every value of every axis and every (lq mod 64, lk mod 64)
    boundary class -- below / at / above a tile on either side (1, 15 .. 17, 63 .. 65, 129, 200 give the classes 1, 15, 16, 17, 63, 0, 1, 1, 8)"""
    rng = np.random.Generator(np.random.Philox(seed))
    cases = []
    # every (lq, lk) pair once: 81 pairs, the other axes cycled through a shuffled order
    pairs = [(a, b) for a in LENGTHS for b in LENGTHS]
    order = rng.permutation(len(pairs))
    for i, j in enumerate(order):
        lq, lk = pairs[int(j)]
        cases.append((ds[i % len(ds)], lq, lk, (1, 3)[(i // len(ds)) % 2], (1, 2)[(i // (2 * len(ds))) % 2]))
    assert {c[0] for c in cases} == set(ds) and {c[3] for c in cases} == {1, 3} and {c[4] for c in cases} == {1, 2}
    return cases


def tokens(seed, length, batch, e, lo=-1.0, hi=1.0, batch_first=False, dtype=np.float32):
    r = np.random.Generator(np.random.Philox(seed))
    shape = (batch, length, e) if batch_first else (length, batch, e)
    return (lo + (hi - lo) * r.random(shape, dtype=np.float32)).astype(dtype)


# ---- graphs -----------------------------------------------------------------------------------------------------------------
def eval_graph(builder, x_nhwc, rnd=None, want=None):
    """float64 evaluation of a PnnxBuilder graph (file order inside; NHWC in, NHWC / [n, features] / tokens out).  rnd: see the module text."""
    import torch
    F = torch.nn.functional
    q = rnd or (lambda a: np.asarray(a, np.float64))
    qt = lambda t: torch.from_numpy(np.ascontiguousarray(q(t.numpy())))
    vals, result = {}, None
    lines = [_parse(ln) for ln in builder.lines]
    graph_outs = {ins[0] for typ, _, ins, _, _ in lines if typ == "pnnx.Output"}
    for typ, name, ins, outs, prm in lines:
        has = lambda k: "%s.%s" % (name, k) in builder.attrs
        a = lambda k: torch.from_numpy(np.ascontiguousarray(q(builder.attrs["%s.%s" % (name, k)])))
        if typ == "pnnx.Input":
            t = torch.from_numpy(np.ascontiguousarray(q(x_nhwc)))
            vals[outs[0]] = t.permute(0, 3, 1, 2).contiguous() if t.ndim == 4 else t
            continue
        if typ == "pnnx.Output":
            result = vals[ins[0]]
            continue
        x = vals[ins[0]]
        if typ == "nn.Conv2d":
            y = F.conv2d(x, a("weight"), a("bias") if prm["bias"] == "True" else None, _ints(prm["stride"]), _ints(prm["padding"]),
                         _ints(prm["dilation"]), int(prm["groups"]))
        elif typ == "nn.SiLU":
            y = F.silu(x)
        elif typ == "nn.ReLU":
            y = F.relu(x)
        elif typ == "torch.flatten":
            y = torch.flatten(x, int(prm["start_dim"]))
        elif typ == "Tensor.permute":
            y = x.permute(*_ints(prm["dims"])).contiguous()
        elif typ in ("Tensor.view", "Tensor.reshape"):
            y = x.reshape(*_ints(prm["shape"]))
        elif typ == "pnnx.Expression":
            assert prm["expr"] == "add(@0,@1)", prm["expr"]
            y = vals[ins[0]] + vals[ins[1]]
        elif typ == "nn.Linear":
            y = F.linear(x, a("weight"), a("bias") if prm["bias"] == "True" else None)
        elif typ == "torch.mean":
            y = x.mean(dim=_ints(prm["dim"]), keepdim=prm.get("keepdim", "False") == "True")
        elif typ == "nn.MultiheadAttention":
            bias = prm["bias"] == "True"
            y = torch.from_numpy(mha_ref([vals[i].numpy() for i in ins], a("in_proj_weight").numpy(), a("in_proj_bias").numpy() if bias else None,
                                         a("out_proj.weight").numpy(), a("out_proj.bias").numpy() if bias else None, int(prm["num_heads"]),
                                         prm["batch_first"] == "True", rnd=rnd))
            assert has("in_proj_weight")
        else:
            raise NotImplementedError(typ)
        assert tuple(y.shape) == tuple(builder.shapes[outs[0]]), (typ, name, tuple(y.shape), builder.shapes[outs[0]])
        vals[outs[0]] = y if outs[0] in graph_outs else qt(y)
    if want is not None:
        return {r: np.ascontiguousarray(vals[r].numpy()) for r in want}
    r = result.numpy()
    return np.ascontiguousarray(r.transpose(0, 2, 3, 1)) if r.ndim == 4 else np.ascontiguousarray(r)
