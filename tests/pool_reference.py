"""Restatements for the average-pool tests (test infrastructure, no product code).

out_size / windows / adaptive_windows: the window rule of include/si_pool.h for one axis, in integers.

avgpool2d_ref: the rule on an NHWC array with SEQUENTIAL adds (row by row, left to right, from +0) in `acc` and one division by the
divisor converted to `acc`.  acc=np.float64: the result is float64 (the exact statement, pinned to torch's float64 to 0 ulp by
tests/test_avgpool_cpu.py).  acc=np.float32: the emulation of the windowed kernel's arithmetic -- a float32 array gives float32, a
float16 array is widened, summed and divided in float32 and rounded once (numpy: to nearest even) -- pinned there to the bits of
torch's float32 / half CPU kernels.  The GPU tests hold the windowed form to the emulation bit for bit and need no torch for that.

avgpool2d_f64_torch: torch.nn.functional.avg_pool2d / adaptive_avg_pool2d in float64 on the NCHW view: the independent yardstick.

TABLE_A / TABLE_B / ADAPTIVE_A / ADAPTIVE_B: the case tables.

eval_graph: a torch-float64 evaluator of a PnnxBuilder graph for the operators of build_toy_densenet / build_toy_pspnet and the
one-op graphs, with the rnd= hook of pad_reference.eval_graph for the fp16-storage emulation.
"""
import itertools

import numpy as np

from ct_reference import _ints, _parse, round_f16  # noqa: F401  (round_f16 re-exported)

SHAPE_A = (2, 11, 14)   # n, h, w of table A and ADAPTIVE_A
SHAPE_B = (2, 23, 29)   # ... of table B and ADAPTIVE_B

# (kernel, stride, padding) as (h, w) pairs
KSP_A = [((2, 2), (2, 2), (0, 0)), ((3, 3), (2, 2), (1, 1)), ((3, 3), (1, 1), (1, 1)), ((2, 3), (2, 1), (1, 0)), ((5, 3), (3, 2), (2, 1)),
         ((3, 2), (3, 2), (0, 1)), ((7, 7), (4, 5), (3, 3)), ((2, 2), (3, 3), (1, 1)), ((11, 14), (1, 1), (0, 0))]
KSP_B = [((20, 23), (3, 6), (0, 0)), ((17, 19), (8, 9), (8, 9)), ((23, 29), (1, 1), (0, 0)), ((9, 8), (7, 7), (4, 4))]
# (k, s, p, ceil_mode, count_include_pad, divisor_override)
TABLE_A = [ksp + (ce, cip, div) for ksp in KSP_A for ce, cip, div in itertools.product((False, True), (True, False), (None, 3))]
TABLE_B = [ksp + (ce, cip, None) for ksp in KSP_B for ce, cip in itertools.product((False, True), (True, False))]
ADAPTIVE_A = [(5, 3), (3, 4), (7, 7), (1, 1), (11, 14), (4, 9), (6, 5)]
ADAPTIVE_B = [(2, 3), (1, 2), (25, 31), (23, 1), (5, 30)]
assert len(TABLE_A) == 72 and len(TABLE_B) == 16


def case_id(case):
    k, s, p, ce, cip, div = case
    return "k%dx%d_s%dx%d_p%dx%d%s%s%s" % (k + s + p + ("_ceil" if ce else "", "" if cip else "_nopad", "_div%d" % div if div else ""))


def out_size(i, k, s, p, ceil_mode=False):
    """o = floor_or_ceil((i + 2p - k) / s) + 1; with ceil_mode, decremented when (o - 1) s >= i + p"""
    span = i + 2 * p - k
    assert span >= 0 and k >= 1 and s >= 1 and 0 <= p <= k // 2, (i, k, s, p)
    o = (-(-span // s) if ceil_mode else span // s) + 1
    if ceil_mode and (o - 1) * s >= i + p:
        o -= 1
    return o


def windows(i, k, s, p, ceil_mode=False):
    """[(lo, hi, padded extent)] per output index: [a, b) = [j s - p, min(a + k, i + p)), clipped to [max(a, 0), min(b, i))"""
    res = []
    for j in range(out_size(i, k, s, p, ceil_mode)):
        a = j * s - p
        b = min(a + k, i + p)
        lo, hi = max(a, 0), min(b, i)
        assert lo < hi, (i, k, s, p, ceil_mode, j)
        res.append((lo, hi, b - a))
    return res


def adaptive_windows(i, o):
    """[floor(j i / o), ceil((j + 1) i / o)); the padded extent is the clipped one"""
    res = []
    for j in range(o):
        lo, hi = (j * i) // o, -((-(j + 1) * i) // o)
        assert 0 <= lo < hi <= i
        res.append((lo, hi, hi - lo))
    return res


def max_taps(ih, iw, k=None, s=None, p=None, ceil_mode=False, adaptive=None):
    """the tap count of the largest clipped window: what the form switch looks at"""
    wy = adaptive_windows(ih, adaptive[0]) if adaptive else windows(ih, k[0], s[0], p[0], ceil_mode)
    wx = adaptive_windows(iw, adaptive[1]) if adaptive else windows(iw, k[1], s[1], p[1], ceil_mode)
    return max(hi - lo for lo, hi, _ in wy) * max(hi - lo for lo, hi, _ in wx)


def avgpool2d_ref(x_nhwc, k=None, s=None, p=(0, 0), ceil_mode=False, count_include_pad=True, divisor_override=None, adaptive=None,
                  acc=np.float64):
    x = np.asarray(x_nhwc)
    n, ih, iw, c = x.shape
    if adaptive is not None:
        wy, wx = adaptive_windows(ih, adaptive[0]), adaptive_windows(iw, adaptive[1])
        count_include_pad, divisor_override = False, None
    else:
        s = k if s is None else s
        wy, wx = windows(ih, k[0], s[0], p[0], ceil_mode), windows(iw, k[1], s[1], p[1], ceil_mode)
    xa = x.astype(acc)
    out = np.empty((n, len(wy), len(wx), c), acc)
    for oy, (y0, y1, py) in enumerate(wy):
        for ox, (x0, x1, px) in enumerate(wx):
            t = np.zeros((n, c), acc)
            for yy in range(y0, y1):
                for xx in range(x0, x1):
                    t = t + xa[:, yy, xx, :]
            div = divisor_override if divisor_override else (py * px if count_include_pad else (y1 - y0) * (x1 - x0))
            out[:, oy, ox, :] = t / acc(div)
    if acc == np.float64:
        return out
    assert out.dtype == np.float32
    return out.astype(x.dtype)   # float32: as it is; float16: one rounding, to nearest even


def avgpool2d_torch(x_nhwc, k=None, s=None, p=(0, 0), ceil_mode=False, count_include_pad=True, divisor_override=None, adaptive=None):
    """torch's CPU kernel in the array's own dtype, NHWC in and out"""
    import torch
    F = torch.nn.functional
    # the NHWC array as torch's channels_last NCHW tensor: the layout of this project, and the CPU kernels whose arithmetic is the rule
    # (torch's kernel for contiguous NCHW divides an adaptive window's sum twice, by its height and then by its width)
    t = torch.from_numpy(np.ascontiguousarray(x_nhwc)).permute(0, 3, 1, 2).contiguous(memory_format=torch.channels_last)
    if adaptive is not None:
        y = F.adaptive_avg_pool2d(t, tuple(adaptive))
    else:
        y = F.avg_pool2d(t, tuple(k), tuple(k if s is None else s), tuple(p), ceil_mode, count_include_pad, divisor_override)
    return y.permute(0, 2, 3, 1).contiguous().numpy()


def avgpool2d_f64_torch(x_nhwc, *a, **kw):
    return avgpool2d_torch(np.asarray(x_nhwc, np.float64), *a, **kw)


def pool_args(typ, prm):
    """keyword arguments of avgpool2d_ref / avgpool2d_torch of a parsed pool line"""
    if typ in ("nn.AdaptiveAvgPool2d", "F.adaptive_avg_pool2d"):
        return dict(adaptive=_ints(prm["output_size"]))
    assert typ in ("nn.AvgPool2d", "F.avg_pool2d"), typ
    div = prm["divisor_override"]
    return dict(k=_ints(prm["kernel_size"]), s=_ints(prm["stride"]), p=_ints(prm["padding"]), ceil_mode=prm["ceil_mode"] == "True",
                count_include_pad=prm["count_include_pad"] == "True", divisor_override=None if div == "None" else int(div))


POOL_TYPES = ("nn.AvgPool2d", "F.avg_pool2d", "nn.AdaptiveAvgPool2d", "F.adaptive_avg_pool2d")


def eval_graph(builder, x_nhwc, rnd=None):
    """torch-float64 evaluation of a PnnxBuilder graph; NHWC in, NHWC (rank 4) or [n, features] out.  rnd: applied to the input, every
    weight / bias / statistic and every layer's output except the graph output (None: exact)."""
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
            vals[outs[0]] = torch.from_numpy(np.ascontiguousarray(q(x_nhwc))).permute(0, 3, 1, 2).contiguous()
            continue
        if typ == "pnnx.Output":
            result = vals[ins[0]]
            continue
        x = vals[ins[0]]
        if typ in POOL_TYPES:
            kw = pool_args(typ, prm)
            if "adaptive" in kw:
                y = F.adaptive_avg_pool2d(x, kw["adaptive"])
            else:
                y = F.avg_pool2d(x, kw["k"], kw["s"], kw["p"], kw["ceil_mode"], kw["count_include_pad"], kw["divisor_override"])
        elif typ == "nn.Conv2d":
            y = F.conv2d(x, a("weight"), a("bias") if prm["bias"] == "True" else None, _ints(prm["stride"]), _ints(prm["padding"]),
                         _ints(prm["dilation"]), int(prm["groups"]))
        elif typ == "nn.BatchNorm2d":
            y = F.batch_norm(x, a("running_mean"), a("running_var"), a("weight"), a("bias"), False, 0.0, float(prm["eps"]))
        elif typ == "nn.ReLU":
            y = F.relu(x)
        elif typ == "torch.cat":
            assert int(prm["dim"]) == 1
            y = torch.cat([vals[i] for i in ins], 1)
        elif typ == "pnnx.Expression":
            assert prm["expr"] == "add(@0,@1)"
            y = vals[ins[0]] + vals[ins[1]]
        elif typ == "torch.flatten":
            y = torch.flatten(x, 1)
        elif typ == "nn.Linear":
            y = F.linear(x, a("weight"), a("bias") if prm["bias"] == "True" else None)
        elif typ in ("F.interpolate", "nn.Upsample"):
            assert prm["mode"] == "bilinear" and prm["size"] != "None"
            y = F.interpolate(x, size=_ints(prm["size"]), mode="bilinear", align_corners=prm["align_corners"] == "True")
        else:
            raise NotImplementedError(typ)
        vals[outs[0]] = y if outs[0] in graph_outs else qt(y)
    r = result.numpy()
    return np.ascontiguousarray(r.transpose(0, 2, 3, 1)) if r.ndim == 4 else r
