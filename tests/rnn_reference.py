"""Restatements for the nn.LSTM / nn.GRU tests (test infrastructure, no product code).

rnn_ref: numpy float64 of torch's inference semantics -- layers, directions, batch_first, zero initial state:
    LSTM  i, f, o = sigmoid, g = tanh of W_i* x + b_i* + W_h* h + b_h*;  c = f c + i g;  h = o tanh(c)              gates i, f, g, o
    GRU   r, z = sigmoid of the same sum;  n = tanh(W_in x + b_in + r (W_hn h + b_hn));  h = (1 - z) n + z h         gates r, z, n
Without rnd every sum is float64 (the biases too).  With rnd= (round_f16) it rounds exactly where the fp16 kernel path does: W_ih and W_hh,
the stored gate workspace (x W_ih^T + the ONE fp32 bias sum of include/si_rnn.h, one rounding) and h at the store into y (the next step and the next layer read the rounded value); the caller rounds
x.  Gates, c and the cell arithmetic stay unrounded, as they are fp32 in the kernel.

rnn_torch: torch.nn.LSTM / torch.nn.GRU on the CPU with the same weights, in a chosen dtype.  tests/test_rnn_cpu.py pins rnn_ref to it.

eval_graph: a float64 evaluator of a PnnxBuilder graph for the operator set of build_toy_crnn, with the rnd= hook of
tests/attention_reference.py: applied to the input, every weight and every stored tensor (each layer's output except the graph outputs).
"""
import os
import re

import numpy as np

from ct_reference import _ints, _parse, round_f16  # noqa: F401  (round_f16 re-exported)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "si_rnn.h")
ENTRIES = ["si_hip_rnn_layer_f32", "si_hip_rnn_layer_f16", "si_hip_rnn_workspace_bytes", "si_hip_rnn_pack_whh_f32", "si_hip_rnn_pack_whh_f16",
           "si_hip_rnn_kernel_name"]
GATES = {"lstm": 4, "gru": 3}


def header_enum(name):
    return int(re.search(r"\b%s = (\d+)" % name, open(HEADER).read()).group(1))


def kname(cell, dtype):
    return "rnn_step_kernel<%s, %d>" % ("_Float16" if np.dtype(dtype) == np.float16 else "float", GATES[cell])


def make_weights(cell, input_size, hidden, layers=1, dirs=1, bias=True, seed=0, scale=None):
    """weights[layer][direction] = (w_ih, w_hh, b_ih, b_hh) fp32, U(-a, a) with torch's a = 1 / sqrt(hidden) (or `scale`); biases None without"""
    r = np.random.Generator(np.random.Philox(seed))
    a = 1.0 / np.sqrt(hidden) if scale is None else float(scale)
    g = GATES[cell] * hidden
    u = lambda *shape: r.uniform(-a, a, shape).astype(np.float32)
    return [[(u(g, input_size if l == 0 else dirs * hidden), u(g, hidden), u(g) if bias else None, u(g) if bias else None) for _ in range(dirs)]
            for l in range(layers)]


def sequence(seed, t, batch, features, lo=-1.0, hi=1.0, batch_first=False, dtype=np.float32):
    r = np.random.Generator(np.random.Philox(seed))
    x = (lo + (hi - lo) * r.random((t, batch, features), dtype=np.float32)).astype(dtype)
    return np.ascontiguousarray(x.transpose(1, 0, 2)) if batch_first else x


def projection_bias(cell, b_ih, b_hh):
    """(the bias of the input projection, b_hn): ONE fp32 sum -- LSTM b_ih + b_hh; GRU b_ih + b_hh for r and z, b_ih alone for n"""
    b_ih, b_hh = np.asarray(b_ih, np.float32), np.asarray(b_hh, np.float32)
    if cell == "lstm":
        return b_ih + b_hh, None
    h = b_ih.size // 3
    return np.concatenate([b_ih[:2 * h] + b_hh[:2 * h], b_ih[2 * h:]]), b_hh[2 * h:].copy()


def sigmoid(v):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-v))


def direction_ref(cell, x, w, reverse=False, rnd=None):
    """one direction of one layer on seq-first x [T, N, I] float64: (y [T, N, H], c_n or None)"""
    w_ih, w_hh, b_ih, b_hh = w
    r = rnd or (lambda a: np.asarray(a, np.float64))
    hid = w_hh.shape[1]
    if b_ih is None:
        bias, b_hn = np.zeros(w_ih.shape[0]), np.zeros(hid)
    elif rnd is not None:   # the kernel path: the one fp32 sum
        bias, b_hn = projection_bias(cell, b_ih, b_hh)
        b_hn = np.zeros(hid) if b_hn is None else b_hn
    else:                   # the exact rule: every sum in float64
        b_ih, b_hh = np.asarray(b_ih, np.float64), np.asarray(b_hh, np.float64)
        bias, b_hn = b_ih + b_hh, np.zeros(hid)
        if cell == "gru":
            bias, b_hn = np.concatenate([bias[:2 * hid], b_ih[2 * hid:]]), b_hh[2 * hid:]
    w_ih64, w_hh64 = r(w_ih).astype(np.float64), r(w_hh).astype(np.float64)
    gates = r(x @ w_ih64.T + bias.astype(np.float64))
    t_len, n = x.shape[:2]
    y = np.zeros((t_len, n, hid))
    h, c = np.zeros((n, hid)), np.zeros((n, hid))
    for s in range(t_len):
        t = t_len - 1 - s if reverse else s
        p = h @ w_hh64.T
        gx = gates[t]
        if cell == "lstm":
            pre = gx + p
            i, f, g, o = (pre[:, k * hid:(k + 1) * hid] for k in range(4))
            c = sigmoid(f) * c + sigmoid(i) * np.tanh(g)
            h = sigmoid(o) * np.tanh(c)
        else:
            rg = sigmoid(gx[:, :hid] + p[:, :hid])
            zg = sigmoid(gx[:, hid:2 * hid] + p[:, hid:2 * hid])
            ng = np.tanh(gx[:, 2 * hid:] + rg * (p[:, 2 * hid:] + b_hn.astype(np.float64)))
            h = (1.0 - zg) * ng + zg * h
        h = r(h)
        y[t] = h
    return y, (c if cell == "lstm" else None)


def rnn_ref(cell, x, weights, batch_first=False, rnd=None):
    """(y, h_n, c_n) float64 (c_n None for a GRU); the states are [layers * dirs, N, H]"""
    cur = np.asarray(x, np.float64)
    if batch_first:
        cur = cur.transpose(1, 0, 2)
    h_n, c_n = [], []
    for per_dir in weights:
        ys = []
        for d, w in enumerate(per_dir):
            y, c = direction_ref(cell, cur, w, reverse=d == 1, rnd=rnd)
            ys.append(y)
            h_n.append(y[0] if d == 1 else y[-1])
            c_n.append(c)
        cur = np.concatenate(ys, axis=2)
    y = np.ascontiguousarray(cur.transpose(1, 0, 2)) if batch_first else cur
    return y, np.stack(h_n), (np.stack(c_n) if cell == "lstm" else None)


def rnn_torch(cell, x, weights, batch_first=False, dtype=np.float64):
    """torch.nn.LSTM / torch.nn.GRU on the CPU in `dtype` with these weights: (y, h_n, c_n) as float64"""
    import torch
    tdt = torch.float64 if np.dtype(dtype) == np.float64 else torch.float32
    layers, dirs = len(weights), len(weights[0])
    hid, in_f = weights[0][0][1].shape[1], weights[0][0][0].shape[1]
    bias = weights[0][0][2] is not None
    mod = (torch.nn.LSTM if cell == "lstm" else torch.nn.GRU)(in_f, hid, num_layers=layers, bias=bias, batch_first=batch_first,
                                                               bidirectional=dirs == 2, dtype=tdt).eval()
    with torch.no_grad():
        for l, per_dir in enumerate(weights):
            for d, w in enumerate(per_dir):
                sfx = "_l%d%s" % (l, "_reverse" if d else "")
                for key, arr in zip(("weight_ih", "weight_hh", "bias_ih", "bias_hh"), w):
                    if arr is not None:
                        getattr(mod, key + sfx).copy_(torch.from_numpy(np.asarray(arr, dtype)))
        y, state = mod(torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype))))
    f64 = lambda t: t.numpy().astype(np.float64)
    return (f64(y), f64(state[0]), f64(state[1])) if cell == "lstm" else (f64(y), f64(state), None)


def builder_weights(builder, name, cell, layers, dirs, bias):
    """the weights[layer][direction] tuples of the operator `name` of a PnnxBuilder"""
    a = lambda key: builder.attrs.get("%s.%s" % (name, key))
    return [[tuple(a(k + "_l%d%s" % (l, "_reverse" if d else "")) if (bias or k.startswith("weight")) else None
                   for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")) for d in range(dirs)] for l in range(layers)]


# ---- graphs -----------------------------------------------------------------------------------------------------------------
def eval_graph(builder, x_nhwc, rnd=None):
    """float64 evaluation of a PnnxBuilder graph (file order inside): the list of graph outputs in file order, rank 4 as NHWC"""
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
            r = vals[ins[0]].numpy()
            results.append(np.ascontiguousarray(r.transpose(0, 2, 3, 1)) if r.ndim == 4 else np.ascontiguousarray(r))
            continue
        x = vals[ins[0]]
        if typ == "nn.Conv2d":
            ys = [F.conv2d(x, a("weight"), a("bias") if prm["bias"] == "True" else None, _ints(prm["stride"]), _ints(prm["padding"]),
                           _ints(prm["dilation"]), int(prm["groups"]))]
        elif typ == "nn.ReLU":
            ys = [F.relu(x)]
        elif typ == "nn.MaxPool2d":
            ys = [F.max_pool2d(x, _ints(prm["kernel_size"]), _ints(prm["stride"]), _ints(prm["padding"]))]
        elif typ == "torch.flatten":
            ys = [torch.flatten(x, int(prm["start_dim"]))]
        elif typ == "Tensor.permute":
            ys = [x.permute(*_ints(prm["dims"])).contiguous()]
        elif typ == "nn.Linear":
            ys = [F.linear(x, a("weight"), a("bias") if prm["bias"] == "True" else None)]
        elif typ in ("nn.LSTM", "nn.GRU"):
            cell = "lstm" if typ == "nn.LSTM" else "gru"
            dirs = 2 if prm["bidirectional"] == "True" else 1
            w = builder_weights(builder, name, cell, int(prm["num_layers"]), dirs, prm["bias"] == "True")
            y, h_n, c_n = rnn_ref(cell, x.numpy(), w, prm["batch_first"] == "True", rnd=rnd)
            ys = [torch.from_numpy(np.ascontiguousarray(v)) for v in (y, h_n, c_n)[:len(outs)]]
        else:
            raise NotImplementedError(typ)
        for o, y in zip(outs, ys):
            assert tuple(y.shape) == tuple(builder.shapes[o]), (typ, name, tuple(y.shape), builder.shapes[o])
            vals[o] = y if o in graph_outs else qt(y)
    return results
