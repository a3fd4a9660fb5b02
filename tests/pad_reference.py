"""numpy restatements for the explicit-pad tests (test infrastructure, no product code).

pad2d_ref: the index rule of include/si_pad.h as an explicit gather on an NHWC array of any dtype -- per axis, output index o reads
source i = o - pad_before; constant: x[i] inside, `value` outside; replicate: clamp; reflect: -i below 0, 2 (size - 1) - i above
size - 1; circular: i mod size.  No np.pad: negative pads (crops) go through the same map.  The gather moves array elements, so a
NaN payload or a -0.0 comes out with the bits it went in with.  tests/test_pad_cpu.py pins it to torch.nn.functional.pad bit for
bit on the accepted set; the GPU tests compare against it and need no torch.

accepts: the acceptance predicate of include/si_pad.h.

eval_graph: gn_reference.eval_graph's operator set plus the six pad type strings and nn.Tanh, with the same rnd= hook for the
fp16-storage emulation.
"""
import numpy as np

import gn_reference as gr
from ct_reference import _ints, _parse, conv_transpose2d_ref, round_f16  # noqa: F401  (round_f16 re-exported)
from up_reference import conv2d_ref

MODES = ("constant", "reflect", "replicate", "circular")
PAD_MODULES = {"nn.ReflectionPad2d": "reflect", "nn.ReplicationPad2d": "replicate", "nn.CircularPad2d": "circular", "nn.ZeroPad2d": "constant",
               "nn.ConstantPad2d": "constant"}
PAD_TYPES = tuple(PAD_MODULES) + ("F.pad",)


def accepts(ih, iw, pads, mode):
    """include/si_pad.h's accepted set for an ih x iw input and pads (left, right, top, bottom)"""
    pl, pr, pt, pb = pads
    if ih + pt + pb < 1 or iw + pl + pr < 1:
        return False
    if iw + min(pl, 0) + min(pr, 0) < 1 or ih + min(pt, 0) + min(pb, 0) < 1:
        return False
    if mode == "reflect":
        return max(pl, pr) < iw and max(pt, pb) < ih
    if mode == "circular":
        return min(pads) >= 0 and max(pl, pr) <= iw and max(pt, pb) <= ih
    return mode in ("constant", "replicate")


def _axis_map(size, before, after, mode):
    """(source index per output index, mask of the outputs that read the constant)"""
    i = np.arange(size + before + after, dtype=np.int64) - before
    outside = (i < 0) | (i > size - 1)
    if mode == "constant":
        return np.where(outside, 0, i), outside
    if mode == "replicate":
        src = np.clip(i, 0, size - 1)
    elif mode == "reflect":
        src = np.where(i < 0, -i, np.where(i > size - 1, 2 * (size - 1) - i, i))
    elif mode == "circular":
        src = np.mod(i, size)
    else:
        raise ValueError(mode)
    assert ((src >= 0) & (src <= size - 1)).all(), (size, before, after, mode)
    return src, np.zeros_like(outside)


def pad2d_ref(x_nhwc, pads, mode="constant", value=0.0):
    """the rule on an NHWC array; the result has x's dtype, `value` converted to it once (numpy rounds to nearest even)"""
    x = np.asarray(x_nhwc)
    n, ih, iw, c = x.shape
    pl, pr, pt, pb = (int(p) for p in pads)
    assert accepts(ih, iw, (pl, pr, pt, pb), mode), (x.shape, pads, mode)
    sy, oy = _axis_map(ih, pt, pb, mode)
    sx, ox = _axis_map(iw, pl, pr, mode)
    y = x[:, sy][:, :, sx].copy()
    fill = np.float32(value).astype(x.dtype) if x.dtype.kind == "f" else x.dtype.type(value)
    y[:, oy] = fill
    y[:, :, ox] = fill
    return y


def pad_args(typ, prm):
    """((l, r, t, b), mode, value) of a parsed pad line"""
    if typ == "F.pad":
        p = _ints(prm["pad"])
        assert len(p) in (2, 4), p
        p = p + (0, 0) * (len(p) == 2)
        return p, prm["mode"], 0.0 if prm.get("value", "None") == "None" else float(prm["value"])
    p = prm["padding"]
    p = _ints(p) if p.startswith("(") else (int(p),) * 4
    return p, PAD_MODULES[typ], float(prm["value"]) if typ == "nn.ConstantPad2d" else 0.0


def eval_graph(builder, x_nhwc, rnd=None):
    """fp64 evaluation of a PnnxBuilder graph (NHWC tensors): the pads and nn.Tanh here, every other operator by
    gn_reference.eval_graph's rules (restated for the ones the generator uses).  rnd: as there."""
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
        if typ in PAD_TYPES:
            y = pad2d_ref(x, *pad_args(typ, prm))
        elif typ == "nn.Tanh":
            y = np.tanh(x)
        elif typ == "nn.Conv2d":
            b = q(a("bias")) if prm["bias"] == "True" else None
            y = conv2d_ref(x, q(a("weight")), b, _ints(prm["stride"]), _ints(prm["padding"]), _ints(prm["dilation"]))
        elif typ == "nn.ConvTranspose2d":
            b = q(a("bias")) if prm["bias"] == "True" else None
            y = conv_transpose2d_ref(x, q(a("weight")), b, _ints(prm["stride"]), _ints(prm["padding"]), _ints(prm["output_padding"]),
                                     _ints(prm["dilation"]))
        elif typ == "nn.InstanceNorm2d":
            assert prm["track_running_stats"] == "False" and prm["affine"] == "False" and int(prm["num_features"]) == x.shape[-1]
            y = gr.group_norm_ref(x, x.shape[-1], None, None, float(prm["eps"]))
        elif typ == "nn.ReLU":
            y = np.maximum(x, 0.0)
        elif typ == "torch.cat":
            assert int(prm["dim"]) == 1
            y = np.concatenate([vals[i] for i in ins], axis=3)
        elif typ == "pnnx.Expression":
            assert prm["expr"] == "add(@0,@1)"
            y = vals[ins[0]] + vals[ins[1]]
        else:
            raise NotImplementedError(typ)
        vals[outs[0]] = y if outs[0] in graph_outs else q(y)
    return result
