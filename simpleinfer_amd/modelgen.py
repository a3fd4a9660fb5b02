"""pnnx model synthesizer (tooling, host-only, numpy).

The reference ships no model files (its ``3rdparty/tmp`` submodule is absent),
and batch size is baked into a ``.pnnx.param`` (reference
``src/pnnx/ir.cpp:597-651``: every operand shape comes from ``#name=(...)f32``),
so benchmarks and parity tests need to *write* models.  This module emits the
two files the reference's loader reads:

* ``*.pnnx.param`` -- text: magic ``7767517``, ``<ops> <operands>``, one line
  per operator (``src/pnnx/ir.cpp:709-815``; value syntax ``:479-550``).
* ``*.pnnx.bin``  -- ZIP, stored-only, entries ``<opname>.<attr>`` holding raw
  little-endian tensors (``src/pnnx/storezip.cpp:117-229``).

Graphs follow SURVEY.md Appendix A (YOLOv5s v6) / A2 (torchvision ResNet18, BN
folded).  Weights come from a portable counter-based generator (splitmix64
keyed by ``fnv1a("<op>.<attr>")``), so the same seeds give the same bytes on
any machine; nothing is trained, nothing is downloaded.
"""
from __future__ import annotations

import math
import zipfile
from typing import Dict, List, Sequence, Tuple

import numpy as np

_U64 = np.uint64


def fnv1a64(s: str) -> int:
    h = 1469598103934665603
    for ch in s.encode():
        h ^= ch
        h = (h * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def splitmix_uniform(seed: int, count: int) -> np.ndarray:
    """``count`` floats in [0,1): splitmix64 of (seed + (i+1)*golden), top 24 bits."""
    with np.errstate(over="ignore"):
        idx = np.arange(1, count + 1, dtype=_U64)
        z = _U64(seed & 0xFFFFFFFFFFFFFFFF) + idx * _U64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> _U64(30))) * _U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> _U64(27))) * _U64(0x94D049BB133111EB)
        z = z ^ (z >> _U64(31))
    return ((z >> _U64(40)).astype(np.float64) / float(1 << 24)).astype(np.float32)


def seeded_uniform(key: str, shape: Sequence[int], lo: float, hi: float, seed: int = 0) -> np.ndarray:
    n = int(np.prod(shape)) if len(shape) else 1
    u = splitmix_uniform(fnv1a64(key) ^ (seed * 0x2545F4914F6CDD1D), n)
    return (lo + (hi - lo) * u).astype(np.float32).reshape(shape)


def synth_input(shape_nhwc: Sequence[int], seed: int = 1) -> np.ndarray:
    """NHWC fp32 U[0,1) -- mimics the /255 normalisation of test_yolo.cpp:252."""
    return seeded_uniform("input", shape_nhwc, 0.0, 1.0, seed)


def _fmt_shape(shape: Sequence[int]) -> str:
    return "(" + ",".join(str(int(s)) for s in shape) + ")f32"


def _fmt_val(v) -> str:
    if isinstance(v, bool):
        return "True" if v else "False"
    if isinstance(v, int):
        return str(v)
    if isinstance(v, float):
        return "%e" % v
    if isinstance(v, str):
        return v
    if isinstance(v, (tuple, list)):
        def one(x):
            if isinstance(x, float):
                return repr(float(x)) if "." in repr(float(x)) or "e" in repr(float(x)) else "%.1f" % x
            return str(x)
        return "(" + ",".join(one(x) for x in v) + ")"
    raise TypeError(type(v))


class PnnxBuilder:
    """Accumulates operators/operands in NCHW (the file's convention) and writes the pair."""

    def __init__(self, seed: int = 0):
        self.seed = seed
        self.lines: List[str] = []
        self.attrs: Dict[str, np.ndarray] = {}
        self.shapes: Dict[str, Tuple[int, ...]] = {}
        self._n_operand = 0
        self._counts: Dict[str, int] = {}
        self.n_ops = 0

    # -- plumbing -----------------------------------------------------------
    def _new_operand(self, shape: Sequence[int]) -> str:
        name = str(self._n_operand)
        self._n_operand += 1
        self.shapes[name] = tuple(int(s) for s in shape)
        return name

    def _opname(self, prefix: str) -> str:
        i = self._counts.get(prefix, 0)
        self._counts[prefix] = i + 1
        return "%s_%d" % (prefix, i)

    def _emit(self, typ: str, name: str, ins: Sequence[str], outs: Sequence[str],
              params: Dict[str, object] = None, attrs: Dict[str, np.ndarray] = None):
        toks = [typ, name, str(len(ins)), str(len(outs)), *ins, *outs]
        for k, v in (params or {}).items():
            toks.append("%s=%s" % (k, _fmt_val(v)))
        for k, arr in (attrs or {}).items():
            arr = np.ascontiguousarray(arr, dtype=np.float32)
            toks.append("@%s=%s" % (k, _fmt_shape(arr.shape)))
            self.attrs["%s.%s" % (name, k)] = arr
        for r in list(ins) + list(outs):
            toks.append("#%s=%s" % (r, _fmt_shape(self.shapes[r])))
        self.lines.append(" ".join(toks))
        self.n_ops += 1

    # -- operators ----------------------------------------------------------
    def input(self, shape_nchw: Sequence[int]) -> str:
        out = self._new_operand(shape_nchw)
        self._emit("pnnx.Input", self._opname("pnnx_input"), [], [out])
        return out

    def output(self, x: str):
        self._emit("pnnx.Output", self._opname("pnnx_output"), [x], [])

    def attribute(self, array, name: str = None) -> str:
        """A graph constant as pnnx writes every tensor that is neither a module weight nor an input: `pnnx.Attribute name 0 1 out
        @data=(shape)f32`, the values (file order) in the .bin under name.data"""
        arr = np.ascontiguousarray(array, dtype=np.float32)
        assert arr.ndim >= 1
        out = self._new_operand(arr.shape)
        self._emit("pnnx.Attribute", name or self._opname("pnnx_attr"), [], [out], attrs={"data": arr})
        return out

    def conv(self, x: str, cout: int, k, s=1, p=None, d=1, groups: int = 1, bias: bool = True,
             name: str = None) -> str:
        n, cin, h, w = self.shapes[x]
        kh, kw = (k, k) if isinstance(k, int) else k
        sh, sw = (s, s) if isinstance(s, int) else s
        dh, dw = (d, d) if isinstance(d, int) else d
        if p is None:
            p = (kh // 2, kw // 2)
        ph, pw = (p, p) if isinstance(p, int) else p
        oh = (h + 2 * ph - ((kh - 1) * dh + 1)) // sh + 1
        ow = (w + 2 * pw - ((kw - 1) * dw + 1)) // sw + 1
        name = name or self._opname("conv")
        fan_in = (cin // groups) * kh * kw
        a = math.sqrt(3.0 / fan_in)
        attrs = {"weight": seeded_uniform(name + ".weight", (cout, cin // groups, kh, kw), -a, a, self.seed)}
        if bias:
            attrs["bias"] = seeded_uniform(name + ".bias", (cout,), -0.1, 0.1, self.seed)
        out = self._new_operand((n, cout, oh, ow))
        self._emit("nn.Conv2d", name, [x], [out],
                   dict(bias=bool(bias), dilation=(dh, dw), groups=groups, in_channels=cin,
                        kernel_size=(kh, kw), out_channels=cout, padding=(ph, pw),
                        padding_mode="zeros", stride=(sh, sw)), attrs)
        return out

    def conv1d(self, x: str, cout: int, k: int, s: int = 1, p=None, d: int = 1, groups: int = 1, bias: bool = True, padding_mode: str = "zeros",
               name: str = None) -> str:
        """pnnx's nn.Conv1d line on a rank-3 operand [N, C, L] (an unbatched [C, L] is written too: the engine refuses it): one-element tuples
        for kernel_size / stride / dilation; padding an int tuple, or the text `same` / `valid`; weight (Cout, Cin / groups, K).  p=None: K // 2"""
        *lead, cin, l = self.shapes[x]
        if p is None:
            p = (d * (k - 1)) // 2
        total = d * (k - 1) if p == "same" else 0 if p == "valid" else 2 * int(p)
        lo = (l + total - d * (k - 1) - 1) // s + 1
        name = name or self._opname("conv1d")
        a = math.sqrt(3.0 / ((cin // groups) * k))
        attrs = {"weight": seeded_uniform(name + ".weight", (cout, cin // groups, k), -a, a, self.seed)}
        if bias:
            attrs["bias"] = seeded_uniform(name + ".bias", (cout,), -0.1, 0.1, self.seed)
        out = self._new_operand(tuple(lead) + (cout, lo))
        self._emit("nn.Conv1d", name, [x], [out],
                   dict(bias=bool(bias), dilation=(d,), groups=groups, in_channels=cin, kernel_size=(k,), out_channels=cout,
                        padding=p if isinstance(p, str) else (int(p),), padding_mode=padding_mode, stride=(s,)), attrs)
        return out

    def conv2d_functional(self, x: str, w: str, bias: str = None, stride=1, padding=0, dilation=1, groups: int = 1) -> str:
        """F.conv2d as pnnx writes the function, the filter an OPERAND: `F.conv2d name 2 1 x w out bias=None stride=(..) padding=(..) dilation=(..)
        groups=G`, or three inputs x w b and no bias= key; padding an int pair or the bare text `same` / `valid`.  x [N, C, H, W],
        w [O, C / groups, kh, kw] (an activation or an attribute()), bias [O]"""
        n, c, h, wd = self.shapes[x]
        oc, cg, kh, kw = self.shapes[w]
        assert cg * groups == c and oc % groups == 0, (self.shapes[x], self.shapes[w], groups)
        sh, sw = (stride, stride) if isinstance(stride, int) else stride
        dh, dw = (dilation, dilation) if isinstance(dilation, int) else dilation
        if padding == "same":
            th, tw = dh * (kh - 1), dw * (kw - 1)
        elif padding == "valid":
            th = tw = 0
        else:
            ph, pw = (padding, padding) if isinstance(padding, int) else padding
            th, tw = 2 * ph, 2 * pw
        oh = (h + th - dh * (kh - 1) - 1) // sh + 1
        ow = (wd + tw - dw * (kw - 1) - 1) // sw + 1
        out = self._new_operand((n, oc, oh, ow))
        params = {} if bias is not None else {"bias": "None"}
        params.update(stride=(sh, sw), padding=padding if isinstance(padding, str) else (ph, pw), dilation=(dh, dw), groups=int(groups))
        self._emit("F.conv2d", self._opname("F_conv2d"), [x, w] + ([bias] if bias is not None else []), [out], params)
        return out

    def conv_transpose(self, x: str, cout: int, k, s=1, p=0, output_padding=0, d=1, bias: bool = True,
                       name: str = None) -> str:
        """pnnx's nn.ConvTranspose2d line; weight [Cin][Cout][kh][kw] (torch's layout), groups 1"""
        n, cin, h, w = self.shapes[x]
        pair = lambda v: (v, v) if isinstance(v, int) else tuple(v)
        (kh, kw), (sh, sw), (ph, pw), (oph, opw), (dh, dw) = pair(k), pair(s), pair(p), pair(output_padding), pair(d)
        oh = (h - 1) * sh - 2 * ph + dh * (kh - 1) + oph + 1
        ow = (w - 1) * sw - 2 * pw + dw * (kw - 1) + opw + 1
        name = name or self._opname("convtranspose")
        a = math.sqrt(3.0 / (cin * kh * kw))
        attrs = {"weight": seeded_uniform(name + ".weight", (cin, cout, kh, kw), -a, a, self.seed)}
        if bias:
            attrs["bias"] = seeded_uniform(name + ".bias", (cout,), -0.1, 0.1, self.seed)
        out = self._new_operand((n, cout, oh, ow))
        self._emit("nn.ConvTranspose2d", name, [x], [out],
                   dict(bias=bool(bias), dilation=(dh, dw), groups=1, in_channels=cin, kernel_size=(kh, kw),
                        out_channels=cout, output_padding=(oph, opw), padding=(ph, pw), padding_mode="zeros",
                        stride=(sh, sw)), attrs)
        return out

    def deform_conv(self, x: str, offset: str, mask: str = None, cout: int = None, k=3, s=1, p=None, d=1, groups: int = 1, bias: bool = True,
                    name: str = None) -> str:
        """torchvision.ops.DeformConv2d as pnnx writes the module: inputs (x, offset) or (x, offset, mask), Conv2d's keys without
        padding_mode, weight [Cout][Cin/groups][kh][kw].  offset is [N, 2 og kh kw, Ho, Wo], mask [N, og kh kw, Ho, Wo]."""
        n, cin, h, w = self.shapes[x]
        pair = lambda v: (v, v) if isinstance(v, int) else tuple(v)
        (kh, kw), (sh, sw), (dh, dw) = pair(k), pair(s), pair(d)
        ph, pw = (kh // 2, kw // 2) if p is None else pair(p)
        oh = (h + 2 * ph - ((kh - 1) * dh + 1)) // sh + 1
        ow = (w + 2 * pw - ((kw - 1) * dw + 1)) // sw + 1
        name = name or self._opname("deformconv")
        a = math.sqrt(3.0 / ((cin // groups) * kh * kw))
        attrs = {"weight": seeded_uniform(name + ".weight", (cout, cin // groups, kh, kw), -a, a, self.seed)}
        if bias:
            attrs["bias"] = seeded_uniform(name + ".bias", (cout,), -0.1, 0.1, self.seed)
        out = self._new_operand((n, cout, oh, ow))
        self._emit("torchvision.ops.DeformConv2d", name, [x, offset] + ([mask] if mask is not None else []), [out],
                   dict(bias=bool(bias), dilation=(dh, dw), groups=groups, in_channels=cin, kernel_size=(kh, kw), out_channels=cout,
                        padding=(ph, pw), stride=(sh, sw)), attrs)
        return out

    def grid_sample(self, x: str, grid: str, mode: str = "bilinear", padding_mode: str = "zeros", align_corners=False) -> str:
        """F.grid_sample as pnnx writes the function: inputs (x [N, C, H, W], grid [N, Ho, Wo, 2]), keys align_corners= (a bool, or None for
        torch's default), mode= and padding_mode= (bare strings)"""
        n, c = self.shapes[x][:2]
        gs = self.shapes[grid]
        out = self._new_operand((n, c) + tuple(gs[1:-1]))
        self._emit("F.grid_sample", self._opname("F_grid_sample"), [x, grid], [out],
                   dict(align_corners="None" if align_corners is None else bool(align_corners), mode=str(mode), padding_mode=str(padding_mode)))
        return out

    def affine_grid(self, theta: str, size: Sequence[int], align_corners=False) -> str:
        """F.affine_grid: theta [N, 2, 3] -> [N, H, W, 2] for size=(N, C, H, W); keys align_corners= and size="""
        size = tuple(int(s) for s in size)
        out = self._new_operand((size[0],) + size[2:] + (len(size) - 2,))
        self._emit("F.affine_grid", self._opname("F_affine_grid"), [theta], [out],
                   dict(align_corners="None" if align_corners is None else bool(align_corners), size=size))
        return out

    def roi_align(self, x: str, rois: str, output_size, spatial_scale: float = 1.0, sampling_ratio: int = -1, aligned: bool = False,
                  functional: bool = False) -> str:
        """torchvision.ops.RoIAlign as pnnx writes the module (functional: torchvision.ops.roi_align, the same keys): inputs (x [N, C, H, W],
        rois [K, 5] with rows (image index, x1, y1, x2, y2)), keys aligned=, output_size= (a pair), sampling_ratio=, spatial_scale="""
        c = self.shapes[x][1]
        ph, pw = (output_size, output_size) if isinstance(output_size, int) else tuple(output_size)
        out = self._new_operand((self.shapes[rois][0], c, ph, pw))
        typ, prefix = ("torchvision.ops.roi_align", "torchvision_ops_roi_align") if functional else ("torchvision.ops.RoIAlign", "roialign")
        self._emit(typ, self._opname(prefix), [x, rois], [out],
                   dict(aligned=bool(aligned), output_size=(ph, pw), sampling_ratio=int(sampling_ratio), spatial_scale=float(spatial_scale)))
        return out

    def _unary(self, typ: str, prefix: str, x: str, params=None) -> str:
        out = self._new_operand(self.shapes[x])
        self._emit(typ, self._opname(prefix), [x], [out], params or {})
        return out

    def _act(self, module: str, prefix: str, fname: str, x: str, functional: bool, params=None) -> str:
        """an activation as its module line, or (functional=True) as pnnx's F.<fname> line with the same keys"""
        if functional:
            return self._unary("F." + fname, "F_" + fname, x, params)
        return self._unary(module, prefix, x, params)

    def silu(self, x, functional=False): return self._act("nn.SiLU", "silu", "silu", x, functional)
    def relu(self, x, functional=False): return self._act("nn.ReLU", "relu", "relu", x, functional)
    def sigmoid(self, x, functional=False): return self._act("nn.Sigmoid", "sigmoid", "sigmoid", x, functional)
    def hardsigmoid(self, x, functional=False): return self._act("nn.Hardsigmoid", "hsigmoid", "hardsigmoid", x, functional)
    def hardswish(self, x, functional=False): return self._act("nn.Hardswish", "hswish", "hardswish", x, functional)
    def tanh(self, x, functional=False): return self._act("nn.Tanh", "tanh", "tanh", x, functional)

    def leaky_relu(self, x, negative_slope: float = 0.01, functional=False):
        return self._act("nn.LeakyReLU", "leakyrelu", "leaky_relu", x, functional, dict(negative_slope=float(negative_slope)))

    def relu6(self, x, functional=False): return self._act("nn.ReLU6", "relu6", "relu6", x, functional)
    def mish(self, x, functional=False): return self._act("nn.Mish", "mish", "mish", x, functional)

    def hardtanh(self, x, min_val: float = -1.0, max_val: float = 1.0, functional=False):
        """pnnx's nn.Hardtanh / F.hardtanh line with torch's keys min_val / max_val"""
        return self._act("nn.Hardtanh", "hardtanh", "hardtanh", x, functional, dict(max_val=float(max_val), min_val=float(min_val)))

    def softplus(self, x, beta: float = 1.0, threshold: float = 20.0, functional=False):
        """pnnx's nn.Softplus / F.softplus line with torch's keys beta / threshold"""
        return self._act("nn.Softplus", "softplus", "softplus", x, functional, dict(beta=float(beta), threshold=float(threshold)))

    def clamp(self, x, min=None, max=None, functional=True):
        """pnnx's torch.clamp line: max= and min=, a bound that is None written None.  (A tensor function: there is no module spelling,
        and `functional` is accepted for symmetry only.)"""
        one = lambda v: "None" if v is None else float(v)
        return self._unary("torch.clamp", "torch_clamp", x, dict(max=one(max), min=one(min)))

    def pixel_shuffle(self, x: str, r: int, functional: bool = False) -> str:
        """pnnx's nn.PixelShuffle line with torch's key `upscale_factor` (functional=True: F.pixel_shuffle, the same key):
        [n, c r r, h, w] -> [n, c, h r, w r]"""
        n, c, h, w = self.shapes[x]
        r = int(r)
        assert r >= 1 and c % (r * r) == 0, (c, r)
        out = self._new_operand((n, c // (r * r), h * r, w * r))
        typ, prefix = ("F.pixel_shuffle", "F_pixel_shuffle") if functional else ("nn.PixelShuffle", "pixelshuffle")
        self._emit(typ, self._opname(prefix), [x], [out], dict(upscale_factor=r))
        return out

    def pixel_unshuffle(self, x: str, r: int, functional: bool = False) -> str:
        """pnnx's nn.PixelUnshuffle line with torch's key `downscale_factor` (functional=True: F.pixel_unshuffle):
        [n, c, h r, w r] -> [n, c r r, h, w]"""
        n, c, h, w = self.shapes[x]
        r = int(r)
        assert r >= 1 and h % r == 0 and w % r == 0, (h, w, r)
        out = self._new_operand((n, c * r * r, h // r, w // r))
        typ, prefix = ("F.pixel_unshuffle", "F_pixel_unshuffle") if functional else ("nn.PixelUnshuffle", "pixelunshuffle")
        self._emit(typ, self._opname(prefix), [x], [out], dict(downscale_factor=r))
        return out

    def prelu(self, x: str, num_parameters: int = 1) -> str:
        """pnnx's nn.PReLU line: num_parameters (1, or the channel count) and weight of shape (num_parameters), seeded slopes in
        [0.05, 0.4) (torch's initial value is 0.25)"""
        c = self.shapes[x][1]
        assert num_parameters in (1, c), (num_parameters, c)
        name = self._opname("prelu")
        out = self._new_operand(self.shapes[x])
        self._emit("nn.PReLU", name, [x], [out], dict(num_parameters=int(num_parameters)),
                   dict(weight=seeded_uniform(name + ".weight", (int(num_parameters),), 0.05, 0.4, self.seed)))
        return out

    def softmax(self, x: str, dim: int, functional: bool = False, log: bool = False) -> str:
        """pnnx's nn.Softmax line with torch's key `dim` (functional=True: F.softmax; log=True: nn.LogSoftmax / F.log_softmax)"""
        if log:
            typ, prefix = ("F.log_softmax", "F_log_softmax") if functional else ("nn.LogSoftmax", "logsoftmax")
        else:
            typ, prefix = ("F.softmax", "F_softmax") if functional else ("nn.Softmax", "softmax")
        return self._unary(typ, prefix, x, dict(dim=int(dim)))

    def log_softmax(self, x: str, dim: int, functional: bool = False) -> str:
        return self.softmax(x, dim, functional, log=True)

    def softmax2d(self, x: str) -> str:
        """nn.Softmax2d: no parameter (softmax over the channels of a rank-4 tensor)"""
        return self._unary("nn.Softmax2d", "softmax2d", x)

    def _reduce(self, op: str, x: str, dim, keepdim: bool) -> str:
        """pnnx's torch.mean / torch.sum / torch.amax / torch.amin line: dim= an int or a tuple as given ((2,3), (1,) is written (1)),
        keepdim=; torch.mean and torch.sum also carry dtype=None.  The output shape is torch's rule."""
        shp = self.shapes[x]
        dims = sorted({d % len(shp) for d in ((dim,) if isinstance(dim, int) else dim)})
        out_shape = [1 if i in dims else s for i, s in enumerate(shp)] if keepdim else [s for i, s in enumerate(shp) if i not in dims]
        out = self._new_operand(out_shape)
        params = dict(dim=int(dim) if isinstance(dim, int) else tuple(int(d) for d in dim))
        if op in ("mean", "sum"):
            params["dtype"] = "None"
        params["keepdim"] = bool(keepdim)
        self._emit("torch." + op, self._opname("torch_" + op), [x], [out], params)
        return out

    def mean(self, x: str, dim, keepdim: bool = False) -> str: return self._reduce("mean", x, dim, keepdim)
    def sum(self, x: str, dim, keepdim: bool = False) -> str: return self._reduce("sum", x, dim, keepdim)
    def amax(self, x: str, dim, keepdim: bool = False) -> str: return self._reduce("amax", x, dim, keepdim)
    def amin(self, x: str, dim, keepdim: bool = False) -> str: return self._reduce("amin", x, dim, keepdim)

    def normalize(self, x: str, dim: int = 1, p=2.0, eps: float = 1e-12) -> str:
        """pnnx's F.normalize line: dim= an int, eps= and p= floats (float("inf") is written inf, as pnnx writes it)"""
        return self._unary("F.normalize", "F_normalize", x, dict(dim=int(dim), eps=float(eps), p=p if isinstance(p, str) else float(p)))

    def norm(self, x: str, dim, p=2, keepdim: bool = False) -> str:
        """pnnx's torch.norm line: dim= an int or a tuple as given, keepdim=, p= as given (an int, a float, or a text such as fro).  dim=None
        writes dim=None (the reduction to a scalar).  The output shape is torch's rule."""
        shp = self.shapes[x]
        dims = list(range(len(shp))) if dim is None else sorted({d % len(shp) for d in ((dim,) if isinstance(dim, int) else dim)})
        out_shape = [1 if i in dims else s for i, s in enumerate(shp)] if keepdim else [s for i, s in enumerate(shp) if i not in dims]
        out = self._new_operand(out_shape)
        params = dict(dim="None" if dim is None else int(dim) if isinstance(dim, int) else tuple(int(d) for d in dim), keepdim=bool(keepdim), p=p)
        self._emit("torch.norm", self._opname("torch_norm"), [x], [out], params)
        return out

    def div(self, a: str, b: str) -> str:
        sa, sb = self.shapes[a], self.shapes[b]
        return self.expression("div(@0,@1)", [a, b], tuple(max(x, y) for x, y in zip(sa, sb)))

    def _head(self, x: str, head) -> str:
        """the optional last layer of the toy builders: None, "softmax" or "log_softmax" over dim 1"""
        assert head in (None, "softmax", "log_softmax"), head
        return x if head is None else self.softmax(x, 1, log=head == "log_softmax")

    PAD_MODULES = {"reflect": "nn.ReflectionPad2d", "replicate": "nn.ReplicationPad2d", "circular": "nn.CircularPad2d"}

    def pad(self, x: str, pads, mode: str = "constant", value=0.0, functional: bool = False, module: str = None) -> str:
        """An explicit pad of H and W.  pads: one int (all four sides), (left, right) or (left, right, top, bottom), torch's order;
        negative: crop.  functional=False: the module line with torch's constructor keys -- nn.ReflectionPad2d / nn.ReplicationPad2d /
        nn.CircularPad2d by mode; mode "constant": nn.ZeroPad2d when value == 0, else nn.ConstantPad2d with its value (module=:
        that type string instead) -- padding written as given (an int stays an int).  functional=True: the F.pad line with pad=,
        mode= and value= (None when value is None or the mode is not constant, as torch's default)."""
        n, c, h, w = self.shapes[x]
        p4 = (pads,) * 4 if isinstance(pads, int) else tuple(int(p) for p in pads) + (0, 0) * (len(pads) == 2)
        assert len(p4) == 4, pads
        pl, pr, pt, pb = p4
        out = self._new_operand((n, c, h + pt + pb, w + pl + pr))
        if functional:
            assert not isinstance(pads, int), "F.pad takes a tuple"
            v = "None" if (value is None or mode != "constant") else value
            self._emit("F.pad", self._opname("F_pad"), [x], [out], dict(mode=mode, pad=tuple(int(p) for p in pads), value=v))
            return out
        typ = module or self.PAD_MODULES.get(mode) or ("nn.ZeroPad2d" if not value else "nn.ConstantPad2d")
        assert mode in self.PAD_MODULES or mode == "constant", mode
        assert len(p4) == 4 and (isinstance(pads, int) or len(pads) == 4), "the 2-D modules take one int or four"
        params = dict(padding=pads if isinstance(pads, int) else p4)
        if typ == "nn.ConstantPad2d":
            params["value"] = value
        self._emit(typ, self._opname("pad"), [x], [out], params)
        return out

    def maxpool(self, x: str, k, s, p) -> str:
        """k, s, p: an int (both axes) or an (h, w) pair, as conv takes them"""
        n, c, h, w = self.shapes[x]
        pair = lambda v: (v, v) if isinstance(v, int) else (int(v[0]), int(v[1]))
        (kh, kw), (sh, sw), (ph, pw) = pair(k), pair(s), pair(p)
        oh = (h + 2 * ph - kh) // sh + 1
        ow = (w + 2 * pw - kw) // sw + 1
        out = self._new_operand((n, c, oh, ow))
        self._emit("nn.MaxPool2d", self._opname("maxpool"), [x], [out],
                   dict(ceil_mode=False, dilation=(1, 1), kernel_size=(kh, kw), padding=(ph, pw),
                        return_indices=False, stride=(sh, sw)))
        return out

    def adaptive_avgpool(self, x: str, out_hw=(1, 1), functional: bool = False) -> str:
        """functional=True: the F.adaptive_avg_pool2d line (the same key)"""
        n, c, h, w = self.shapes[x]
        out = self._new_operand((n, c, out_hw[0], out_hw[1]))
        typ, prefix = ("F.adaptive_avg_pool2d", "F_adaptive_avg_pool2d") if functional else ("nn.AdaptiveAvgPool2d", "avgpool")
        self._emit(typ, self._opname(prefix), [x], [out], dict(output_size=(int(out_hw[0]), int(out_hw[1]))))
        return out

    @staticmethod
    def avgpool_out_size(i: int, k: int, s: int, p: int, ceil_mode: bool = False) -> int:
        """torch's rule for one axis: floor or ceil of (i + 2p - k) / s, + 1; with ceil_mode the last window must start inside the input
        or its left pad"""
        span = i + 2 * p - k
        assert span >= 0 and s >= 1, (i, k, s, p)
        o = (-(-span // s) if ceil_mode else span // s) + 1
        if ceil_mode and (o - 1) * s >= i + p:
            o -= 1
        return o

    def avgpool(self, x: str, k, s=None, p=0, ceil_mode: bool = False, count_include_pad: bool = True, divisor_override=None,
                functional: bool = False) -> str:
        """pnnx's nn.AvgPool2d line (functional=True: F.avg_pool2d, the same keys).  k, s, p: an int (both axes) or an (h, w) pair;
        s=None: the kernel size, torch's default.  The output shape is torch's rule."""
        n, c, h, w = self.shapes[x]
        pair = lambda v: (v, v) if isinstance(v, int) else (int(v[0]), int(v[1]))
        (kh, kw), (ph, pw) = pair(k), pair(p)
        sh, sw = (kh, kw) if s is None else pair(s)
        out = self._new_operand((n, c, self.avgpool_out_size(h, kh, sh, ph, ceil_mode), self.avgpool_out_size(w, kw, sw, pw, ceil_mode)))
        typ, prefix = ("F.avg_pool2d", "F_avg_pool2d") if functional else ("nn.AvgPool2d", "avgpool2d")
        self._emit(typ, self._opname(prefix), [x], [out],
                   dict(ceil_mode=bool(ceil_mode), count_include_pad=bool(count_include_pad),
                        divisor_override="None" if divisor_override is None else int(divisor_override), kernel_size=(kh, kw),
                        padding=(ph, pw), stride=(sh, sw)))
        return out

    def _resized(self, x: str, scale, size):
        """output operand of a resize: size=(h, w), or torch's floor(in * scale_factor)"""
        n, c, h, w = self.shapes[x]
        if size is not None:
            return self._new_operand((n, c, int(size[0]), int(size[1])))
        sh, sw = (scale, scale) if isinstance(scale, (int, float)) else scale
        return self._new_operand((n, c, int(math.floor(h * float(sh))), int(math.floor(w * float(sw)))))

    def upsample(self, x: str, scale: float = 2.0, mode: str = "nearest", align_corners=None, size=None) -> str:
        """pnnx's nn.Upsample line.  size=(h, w) replaces the scale factor (scale_factor=None in the file); align_corners is
        written for the modes that have it (pnnx omits it for nearest)."""
        if mode == "nearest" and align_corners is None and size is None:
            n, c, h, w = self.shapes[x]
            out = self._new_operand((n, c, int(h * scale), int(w * scale)))
            self._emit("nn.Upsample", self._opname("upsample"), [x], [out],
                       dict(mode="nearest", scale_factor=(float(scale), float(scale)), size="None"))
            return out
        out = self._resized(x, scale, size)
        params = {}
        if mode != "nearest" or align_corners is not None:
            params["align_corners"] = "None" if align_corners is None else bool(align_corners)
        params["mode"] = mode
        if size is not None:
            params.update(scale_factor="None", size=(int(size[0]), int(size[1])))
        else:
            sh, sw = (scale, scale) if isinstance(scale, (int, float)) else scale
            params.update(scale_factor=(float(sh), float(sw)), size="None")
        self._emit("nn.Upsample", self._opname("upsample"), [x], [out], params)
        return out

    def interpolate(self, x: str, scale=None, mode: str = "nearest", align_corners=None, size=None, recompute_scale_factor=None,
                    functional: str = "F.interpolate") -> str:
        """pnnx's F.interpolate line (functional="F.upsample": the older spelling, which has no recompute_scale_factor)"""
        assert (scale is None) != (size is None), "give scale or size"
        if recompute_scale_factor and scale is not None:
            n, c, h, w = self.shapes[x]
            sh, sw = (scale, scale) if isinstance(scale, (int, float)) else scale
            out = self._new_operand((n, c, int(math.floor(h * float(sh))), int(math.floor(w * float(sw)))))
        else:
            out = self._resized(x, scale, size)
        params = dict(align_corners="None" if align_corners is None else bool(align_corners), mode=mode)
        if functional == "F.interpolate":
            params["recompute_scale_factor"] = "None" if recompute_scale_factor is None else bool(recompute_scale_factor)
        if size is not None:
            params.update(scale_factor="None", size=(int(size[0]), int(size[1])))
        else:
            sh, sw = (scale, scale) if isinstance(scale, (int, float)) else scale
            params.update(scale_factor=(float(sh), float(sw)), size="None")
        self._emit(functional, self._opname(functional.replace(".", "_")), [x], [out], params)
        return out

    def cat(self, xs: Sequence[str], dim: int = 1) -> str:
        shp = list(self.shapes[xs[0]])
        shp[dim] = sum(self.shapes[x][dim] for x in xs)
        out = self._new_operand(shp)
        self._emit("torch.cat", self._opname("cat"), list(xs), [out], dict(dim=dim))
        return out

    def _pieces(self, typ: str, prefix: str, x: str, dim: int, lens: Sequence[int], params) -> List[str]:
        shp = list(self.shapes[x])
        outs = []
        for n in lens:
            shp[dim] = int(n)
            outs.append(self._new_operand(shp))
        self._emit(typ, self._opname(prefix), [x], outs, params)
        return outs

    def chunk(self, x: str, chunks: int, dim: int = 1) -> List[str]:
        """pnnx's torch.chunk line (chunks=, dim=), one output operand per chunk: pieces of ceil(size / chunks), the last one may be smaller"""
        size = self.shapes[x][dim]
        each = -(-size // int(chunks))
        lens = [min(each, size - at) for at in range(0, size, each)]
        return self._pieces("torch.chunk", "torch_chunk", x, dim % len(self.shapes[x]), lens, dict(chunks=int(chunks), dim=int(dim)))

    def split(self, x: str, split_size_or_sections, dim: int = 1) -> List[str]:
        """pnnx's torch.split line (split_size_or_sections= an int or a list, dim=), one output operand per piece"""
        size = self.shapes[x][dim]
        if isinstance(split_size_or_sections, int):
            each = int(split_size_or_sections)
            lens, arg = [min(each, size - at) for at in range(0, size, each)], each
        else:
            lens = arg = tuple(int(v) for v in split_size_or_sections)
            assert sum(lens) == size, (lens, size)
        return self._pieces("torch.split", "torch_split", x, dim % len(self.shapes[x]), lens, dict(dim=int(dim), split_size_or_sections=arg))

    def slice(self, x: str, dim, start=0, end=None, step=1) -> str:
        """pnnx's Tensor.slice line.  An int `dim` writes the one-axis spelling dim= start= end= step=; a tuple writes dims= starts= ends=
        steps= with several axes in one operator (start / end / step are then tuples too).  end=None is written as 2147483647, as pnnx
        writes an open end; the string "None" is written as it is."""
        shp = list(self.shapes[x])
        many = not isinstance(dim, int)
        dims = tuple(dim) if many else (dim,)
        starts, ends, steps = (tuple(v) if many else (v,) for v in (start, end, step))
        ends = tuple(2147483647 if e is None else e for e in ends)
        for d, s0, e, st in zip(dims, starts, ends, steps):
            shp[d] = len(range(*slice(s0, None if e == "None" else e, st).indices(shp[d])))
            assert shp[d] > 0 and st >= 1, (d, s0, e, st)
        out = self._new_operand(shp)
        params = dict(dims=dims, ends=ends, starts=starts, steps=steps) if many else dict(dim=dims[0], end=ends[0], start=starts[0], step=steps[0])
        self._emit("Tensor.slice", self._opname("Tensor_slice"), [x], [out], params)
        return out

    # the layout operators (layer/layout.h): pnnx's lines for the tensor methods it passes through
    def _layout(self, typ: str, x: str, shape: Sequence[int], params) -> str:
        out = self._new_operand(shape)
        self._emit(typ, self._opname(typ.replace(".", "_")), [x], [out], params)
        return out

    def permute(self, x: str, dims: Sequence[int], functional: bool = False) -> str:
        """Tensor.permute (torch.permute with functional=True): dims="""
        shp = self.shapes[x]
        dims = tuple(int(d) for d in dims)
        assert sorted(d % len(shp) for d in dims) == list(range(len(shp))), (dims, shp)
        return self._layout("torch.permute" if functional else "Tensor.permute", x, [shp[d] for d in dims], dict(dims=dims))

    def _reshaped(self, typ: str, x: str, shape: Sequence[int]) -> str:
        shape = tuple(int(s) for s in shape)
        count = int(np.prod(self.shapes[x], dtype=np.int64))
        known = int(np.prod([s for s in shape if s != -1], dtype=np.int64))
        assert shape.count(-1) <= 1 and known > 0 and count % known == 0 and (-1 in shape or known == count), (self.shapes[x], shape)
        return self._layout(typ, x, [count // known if s == -1 else s for s in shape], dict(shape=shape))

    def reshape(self, x: str, shape: Sequence[int]) -> str:
        """Tensor.reshape: shape=, one entry may be -1 (it is written as it is; the output operand carries the resolved shape)"""
        return self._reshaped("Tensor.reshape", x, shape)

    def view(self, x: str, shape: Sequence[int]) -> str:
        """Tensor.view: shape=, as reshape"""
        return self._reshaped("Tensor.view", x, shape)

    def transpose(self, x: str, dim0: int, dim1: int) -> str:
        """torch.transpose: dim0= dim1="""
        shp = list(self.shapes[x])
        shp[dim0], shp[dim1] = shp[dim1], shp[dim0]
        return self._layout("torch.transpose", x, shp, dict(dim0=int(dim0), dim1=int(dim1)))

    def squeeze(self, x: str, dim: int) -> str:
        """torch.squeeze: dim= (a dimension that is not 1 stays, torch's rule)"""
        shp = list(self.shapes[x])
        if shp[dim] == 1:
            del shp[dim % len(shp)]
        return self._layout("torch.squeeze", x, shp, dict(dim=int(dim)))

    def unsqueeze(self, x: str, dim: int) -> str:
        """torch.unsqueeze: dim="""
        shp = list(self.shapes[x])
        shp.insert(dim if dim >= 0 else dim + len(shp) + 1, 1)
        return self._layout("torch.unsqueeze", x, shp, dict(dim=int(dim)))

    def contiguous(self, x: str) -> str:
        """Tensor.contiguous: no parameters"""
        return self._layout("Tensor.contiguous", x, self.shapes[x], {})

    def expression(self, expr: str, xs: Sequence[str], out_shape=None) -> str:
        out = self._new_operand(out_shape or self.shapes[xs[0]])
        self._emit("pnnx.Expression", self._opname("pnnx_expr"), list(xs), [out], dict(expr=expr))
        return out

    def add(self, a: str, b: str) -> str:
        return self.expression("add(@0,@1)", [a, b])

    def mul(self, a: str, b: str) -> str:
        sa, sb = self.shapes[a], self.shapes[b]
        return self.expression("mul(@0,@1)", [a, b], tuple(max(x, y) for x, y in zip(sa, sb)))

    def batchnorm(self, x: str, eps: float = 1e-5) -> str:
        n, c, h, w = self.shapes[x]
        name = self._opname("bn")
        attrs = dict(
            running_mean=seeded_uniform(name + ".running_mean", (c,), -0.5, 0.5, self.seed),
            running_var=seeded_uniform(name + ".running_var", (c,), 0.5, 1.5, self.seed),
            weight=seeded_uniform(name + ".weight", (c,), 0.5, 1.5, self.seed),
            bias=seeded_uniform(name + ".bias", (c,), -0.5, 0.5, self.seed))
        out = self._new_operand((n, c, h, w))
        self._emit("nn.BatchNorm2d", name, [x], [out], dict(affine=True, eps=float(eps), num_features=c), attrs)
        return out

    def _norm_affine(self, name: str, c: int) -> Dict[str, np.ndarray]:
        return dict(weight=seeded_uniform(name + ".weight", (c,), 0.5, 1.5, self.seed),
                    bias=seeded_uniform(name + ".bias", (c,), -0.5, 0.5, self.seed))

    def group_norm(self, x: str, groups: int, eps: float = 1e-5, affine: bool = True) -> str:
        """pnnx's nn.GroupNorm line: num_groups, num_channels, eps, affine and, when affine, weight / bias of shape (C)"""
        n, c, h, w = self.shapes[x]
        assert groups > 0 and c % groups == 0, (c, groups)
        name = self._opname("gn")
        out = self._new_operand((n, c, h, w))
        self._emit("nn.GroupNorm", name, [x], [out], dict(affine=bool(affine), eps=float(eps), num_channels=c, num_groups=int(groups)),
                   self._norm_affine(name, c) if affine else {})
        return out

    def instance_norm(self, x: str, eps: float = 1e-5, affine: bool = False, track_running_stats: bool = False) -> str:
        """pnnx's nn.InstanceNorm2d line: num_features, eps, affine, track_running_stats and, when affine, weight / bias"""
        n, c, h, w = self.shapes[x]
        name = self._opname("in")
        out = self._new_operand((n, c, h, w))
        self._emit("nn.InstanceNorm2d", name, [x], [out],
                   dict(affine=bool(affine), eps=float(eps), num_features=c, track_running_stats=bool(track_running_stats)),
                   self._norm_affine(name, c) if affine else {})
        return out

    def flatten(self, x: str, start_dim: int = 1) -> str:
        shp = self.shapes[x]
        out = self._new_operand(tuple(shp[:start_dim]) + (int(np.prod(shp[start_dim:])),))
        self._emit("torch.flatten", self._opname("flatten"), [x], [out], dict(end_dim=-1, start_dim=int(start_dim)))
        return out

    def linear(self, x: str, out_f: int, bias: bool = True) -> str:
        """nn.Linear over the last dimension of an operand of any rank >= 2 ([N, F]; token tensors [L, N, E] / [N, L, E])"""
        *lead, in_f = self.shapes[x]
        name = self._opname("linear")
        a = math.sqrt(3.0 / in_f)
        attrs = {"weight": seeded_uniform(name + ".weight", (out_f, in_f), -a, a, self.seed),
                 # the reference requires the attribute even for bias=False
                 "bias": seeded_uniform(name + ".bias", (out_f,), -0.1, 0.1, self.seed)}
        out = self._new_operand(tuple(lead) + (out_f,))
        self._emit("nn.Linear", name, [x], [out], dict(bias=bool(bias), in_features=in_f, out_features=out_f), attrs)
        return out

    def multihead_attention(self, q: str, k: str = None, v: str = None, num_heads: int = 1, bias: bool = True, batch_first: bool = False,
                            add_bias_kv: bool = False, add_zero_attn: bool = False, kdim: int = None, vdim: int = None,
                            need_weights: bool = False) -> str:
        """pnnx's nn.MultiheadAttention line: 1 input (self-attention), 2 (query; key = value) or 3 (query, key, value), rank-3 operands
        [L, N, E], or [N, L, E] with batch_first; params embed_dim, num_heads, bias, batch_first, add_bias_kv, add_zero_attn, kdim, vdim;
        attributes in_proj_weight (3E, E), out_proj.weight (E, E) and, with bias, in_proj_bias (3E) / out_proj.bias (E).  need_weights adds
        the second output operand [N, Lq, Lk] (the engine refuses it)."""
        ins = [q] + ([k] if k is not None else []) + ([v] if v is not None else [])
        assert v is None or k is not None
        e = self.shapes[q][-1]
        name = self._opname("attention")
        a = math.sqrt(3.0 / e)
        attrs = {"in_proj_weight": seeded_uniform(name + ".in_proj_weight", (3 * e, e), -a, a, self.seed),
                 "out_proj.weight": seeded_uniform(name + ".out_proj.weight", (e, e), -a, a, self.seed)}
        if bias:
            attrs["in_proj_bias"] = seeded_uniform(name + ".in_proj_bias", (3 * e,), -0.1, 0.1, self.seed)
            attrs["out_proj.bias"] = seeded_uniform(name + ".out_proj.bias", (e,), -0.1, 0.1, self.seed)
        outs = [self._new_operand(self.shapes[q])]
        if need_weights:
            kshape = self.shapes[ins[1] if len(ins) > 1 else q]
            bi, li = (0, 1) if batch_first else (1, 0)
            outs.append(self._new_operand((self.shapes[q][bi], self.shapes[q][li], kshape[li])))
        self._emit("nn.MultiheadAttention", name, ins, outs,
                   dict(add_bias_kv=bool(add_bias_kv), add_zero_attn=bool(add_zero_attn), batch_first=bool(batch_first), bias=bool(bias),
                        embed_dim=e, kdim=e if kdim is None else int(kdim), num_heads=int(num_heads), vdim=e if vdim is None else int(vdim)), attrs)
        return outs[0]

    def _recurrent(self, cell: str, x: str, hidden: int, num_layers: int, bias: bool, batch_first: bool, bidirectional: bool, states: bool,
                   proj_size: int, initial: Sequence[str]):
        n_gates, typ = (4, "nn.LSTM") if cell == "lstm" else (3, "nn.GRU")
        shp = self.shapes[x]
        assert len(shp) == 3, shp
        in_f, dirs = shp[2], 2 if bidirectional else 1
        name = self._opname(cell)
        a = 1.0 / math.sqrt(hidden)   # torch's reset_parameters
        attrs = {}
        for l in range(num_layers):
            for sfx in ["_l%d" % l] + (["_l%d_reverse" % l] if bidirectional else []):
                shapes = [("weight_ih", (n_gates * hidden, in_f if l == 0 else dirs * hidden)), ("weight_hh", (n_gates * hidden, hidden))]
                if bias:
                    shapes += [("bias_ih", (n_gates * hidden,)), ("bias_hh", (n_gates * hidden,))]
                for key, shape in shapes:
                    attrs[key + sfx] = seeded_uniform("%s.%s%s" % (name, key, sfx), shape, -a, a, self.seed)
        outs = [self._new_operand(tuple(shp[:2]) + (dirs * hidden,))]
        if states:
            batch = shp[0] if batch_first else shp[1]
            outs += [self._new_operand((num_layers * dirs, batch, hidden)) for _ in range(2 if cell == "lstm" else 1)]
        params = dict(batch_first=bool(batch_first), bias=bool(bias), bidirectional=bool(bidirectional), dropout=0.0, hidden_size=int(hidden),
                      input_size=int(in_f), num_layers=int(num_layers))
        if cell == "lstm":
            params["proj_size"] = int(proj_size)
        self._emit(typ, name, [x] + list(initial), outs, params, attrs)
        return tuple(outs) if states else outs[0]

    def lstm(self, x: str, hidden: int, num_layers: int = 1, bias: bool = True, batch_first: bool = False, bidirectional: bool = False,
             states: bool = False, proj_size: int = 0, initial: Sequence[str] = ()):
        """pnnx's nn.LSTM line on a rank-3 operand [T, N, I], or [N, T, I] with batch_first: params input_size, hidden_size, num_layers, bias,
        batch_first, bidirectional, proj_size, dropout; attributes weight_ih_l{k} (4H, I_k), weight_hh_l{k} (4H, H) and, with bias,
        bias_ih_l{k} / bias_hh_l{k} (4H), with their _reverse twins.  Returns y [.., D H]; states=True: (y, h_n, c_n), the states
        [layers * D, N, H].  proj_size != 0 and initial (h0, c0 as further inputs) write lines the engine refuses."""
        return self._recurrent("lstm", x, hidden, num_layers, bias, batch_first, bidirectional, states, proj_size, initial)

    def gru(self, x: str, hidden: int, num_layers: int = 1, bias: bool = True, batch_first: bool = False, bidirectional: bool = False,
            states: bool = False, initial: Sequence[str] = ()):
        """pnnx's nn.GRU line, as lstm() above with three gates (r, z, n) and no proj_size; states=True: (y, h_n)"""
        return self._recurrent("gru", x, hidden, num_layers, bias, batch_first, bidirectional, states, 0, initial)

    def detect(self, xs: Sequence[str], strides=(8.0, 16.0, 32.0), anchors=None, nc: int = 80) -> str:
        """models.yolo.Detect -- attribute names per reference src/layer/yolo_detect.cpp:19-145."""
        anchors = anchors or [[(10, 13), (16, 30), (33, 23)], [(30, 61), (62, 45), (59, 119)],
                              [(116, 90), (156, 198), (373, 326)]]
        ne, na = nc + 5, 3
        name = self._opname("detect")
        attrs = {"pnnx_5": np.asarray(strides, dtype=np.float32)}
        anchor_idx, grid_idx = (4, 2, 0), (6, 3, 1)
        rows = 0
        n = self.shapes[xs[0]][0]
        for i, x in enumerate(xs):
            _, c, h, w = self.shapes[x]
            a = math.sqrt(3.0 / c)
            attrs["m.%d.weight" % i] = seeded_uniform("%s.m.%d.weight" % (name, i), (na * ne, c, 1, 1), -a, a, self.seed)
            attrs["m.%d.bias" % i] = seeded_uniform("%s.m.%d.bias" % (name, i), (na * ne,), -0.1, 0.1, self.seed)
            gy, gx = np.meshgrid(np.arange(h, dtype=np.float32), np.arange(w, dtype=np.float32), indexing="ij")
            grid = np.stack([gx - 0.5, gy - 0.5], axis=-1)  # [h,w,2], (x,y)
            attrs["pnnx_%d" % grid_idx[i]] = np.broadcast_to(grid[None, None], (1, na, h, w, 2)).copy()
            ag = np.asarray(anchors[i], dtype=np.float32).reshape(1, na, 1, 1, 2)
            attrs["pnnx_%d" % anchor_idx[i]] = np.broadcast_to(ag, (1, na, h, w, 2)).copy()
            rows += na * h * w
        out = self._new_operand((n, rows, ne))
        self._emit("models.yolo.Detect", name, list(xs), [out], {}, attrs)
        return out

    # -- writing ------------------------------------------------------------
    def save(self, param_path: str, bin_path: str):
        with open(param_path, "w") as f:
            f.write("7767517\n%d %d\n" % (self.n_ops, self._n_operand))
            for ln in self.lines:
                f.write(ln + "\n")
        with zipfile.ZipFile(bin_path, "w", compression=zipfile.ZIP_STORED) as z:
            for k, arr in self.attrs.items():
                zi = zipfile.ZipInfo(k, date_time=(1980, 1, 1, 0, 0, 0))
                zi.compress_type = zipfile.ZIP_STORED
                z.writestr(zi, arr.astype("<f4").tobytes())


# ---------------------------------------------------------------------------
# YOLOv5 building blocks
# ---------------------------------------------------------------------------
def _Conv(b: PnnxBuilder, x, c2, k=1, s=1):
    return b.silu(b.conv(x, c2, k, s, k // 2))


def _C3(b: PnnxBuilder, x, c2, n=1, shortcut=True):
    c_ = c2 // 2
    y1 = _Conv(b, x, c_, 1)
    for _ in range(n):
        t = _Conv(b, _Conv(b, y1, c_, 1), c_, 3)
        y1 = b.add(y1, t) if shortcut else t
    y2 = _Conv(b, x, c_, 1)
    return _Conv(b, b.cat([y1, y2], 1), c2, 1)


def _SPPF(b: PnnxBuilder, x, c2, k=5):
    c1 = b.shapes[x][1]
    x = _Conv(b, x, c1 // 2, 1)
    y1 = b.maxpool(x, k, 1, k // 2)
    y2 = b.maxpool(y1, k, 1, k // 2)
    y3 = b.maxpool(y2, k, 1, k // 2)
    return _Conv(b, b.cat([x, y1, y2, y3], 1), c2, 1)


def build_yolov5s(batch: int, size: int = 640, seed: int = 0, width: float = 0.5,
                  depth: float = 1.0 / 3.0, nc: int = 80) -> PnnxBuilder:
    def ch(c):
        return int(math.ceil(c * width / 8) * 8)

    def dn(n):
        return max(round(n * depth), 1)

    b = PnnxBuilder(seed)
    x = b.input((batch, 3, size, size))
    x = b.silu(b.conv(x, ch(64), 6, 2, 2))         # 0: Conv(3,32,k6,s2,p2)
    x = _Conv(b, x, ch(128), 3, 2)                 # 1
    x = _C3(b, x, ch(128), dn(3))                  # 2
    x = _Conv(b, x, ch(256), 3, 2)                 # 3
    p3 = _C3(b, x, ch(256), dn(6))                 # 4
    x = _Conv(b, p3, ch(512), 3, 2)                # 5
    p4 = _C3(b, x, ch(512), dn(9))                 # 6
    x = _Conv(b, p4, ch(1024), 3, 2)               # 7
    x = _C3(b, x, ch(1024), dn(3))                 # 8
    x = _SPPF(b, x, ch(1024), 5)                   # 9
    h10 = _Conv(b, x, ch(512), 1, 1)               # 10
    x = b.upsample(h10, 2.0)                       # 11
    x = b.cat([x, p4], 1)                          # 12
    x = _C3(b, x, ch(512), dn(3), False)           # 13
    h14 = _Conv(b, x, ch(256), 1, 1)               # 14
    x = b.upsample(h14, 2.0)                       # 15
    x = b.cat([x, p3], 1)                          # 16
    d3 = _C3(b, x, ch(256), dn(3), False)          # 17 -> P3
    x = _Conv(b, d3, ch(256), 3, 2)                # 18
    x = b.cat([x, h14], 1)                         # 19
    d4 = _C3(b, x, ch(512), dn(3), False)          # 20 -> P4
    x = _Conv(b, d4, ch(512), 3, 2)                # 21
    x = b.cat([x, h10], 1)                         # 22
    d5 = _C3(b, x, ch(1024), dn(3), False)         # 23 -> P5
    out = b.detect([d3, d4, d5], nc=nc)            # 24
    b.output(out)
    return b


def build_resnet18(batch: int, size: int = 224, num_classes: int = 1000, seed: int = 0,
                   base: int = 64) -> PnnxBuilder:
    """torchvision ResNet18 with BN folded into the convs."""
    b = PnnxBuilder(seed)
    x = b.input((batch, 3, size, size))
    x = b.relu(b.conv(x, base, 7, 2, 3))
    x = b.maxpool(x, 3, 2, 1)
    cin = base
    for stage, c in enumerate((base, base * 2, base * 4, base * 8)):
        for blk in range(2):
            s = 2 if (stage > 0 and blk == 0) else 1
            idt = x
            y = b.relu(b.conv(x, c, 3, s, 1))
            y = b.conv(y, c, 3, 1, 1)
            if s != 1 or cin != c:
                idt = b.conv(x, c, 1, s, 0)
            x = b.relu(b.add(y, idt))
            cin = c
    x = b.adaptive_avgpool(x, (1, 1))
    x = b.flatten(x)
    x = b.linear(x, num_classes)
    b.output(x)
    return b


def build_toy_yolo(batch: int = 2, size: int = 64, seed: int = 0) -> PnnxBuilder:
    """A narrow YOLOv5 (width 0.125 -> channels 8..128) for fast graph-level parity tests."""
    return build_yolov5s(batch, size, seed, width=0.125, depth=1.0 / 3.0, nc=3)


def build_toy_classifier(batch: int = 2, size: int = 32, seed: int = 0, head=None) -> PnnxBuilder:
    """Small net touching the MobileNet-side ops: BN, hardswish, hardsigmoid, SE-style broadcast mul,
    grouped conv, sigmoid, avgpool, flatten, linear.  head="softmax" / "log_softmax": nn.Softmax(dim=1) / nn.LogSoftmax(dim=1) on the logits."""
    b = PnnxBuilder(seed)
    x = b.input((batch, 3, size, size))
    x = b.hardswish(b.batchnorm(b.conv(x, 16, 3, 2, 1, bias=False)))
    y = b.relu(b.conv(x, 16, 3, 1, 1, groups=16))          # depthwise
    se = b.adaptive_avgpool(y, (1, 1))
    se = b.relu(b.conv(se, 8, 1))
    se = b.hardsigmoid(b.conv(se, 16, 1))
    y = b.mul(y, se)                                        # broadcast over H, W
    y = b.conv(y, 16, 1)
    x = b.add(x, y)
    x = b.sigmoid(b.conv(x, 24, 3, 2, 1, groups=2))
    x = b.adaptive_avgpool(x, (1, 1))
    x = b.flatten(x)
    x = b.linear(x, 10)
    b.output(b._head(x, head))
    return b


def build_toy_timm_head(batch: int = 2, size: int = 32, seed: int = 0) -> PnnxBuilder:
    """The head of a timm export: a conv stack, x.mean((2, 3)) -- torch.mean, keepdim=False, the [N, C] result -- and nn.Linear."""
    b = PnnxBuilder(seed)
    x = b.input((batch, 3, size, size))
    x = b.relu(b.conv(x, 16, 3, 2, 1))
    x = b.relu(b.conv(x, 32, 3, 2, 1))
    x = b.mean(x, (2, 3))
    b.output(b.linear(x, 10))
    return b


def build_toy_cbam(batch: int = 2, size: int = 16, seed: int = 0) -> PnnxBuilder:
    """CBAM on one feature map.  Channel attention: mean and amax over (2, 3) with keepdim, the same two 1x1 convs (shared weights) on
    both, add, sigmoid, broadcast mul.  Spatial attention: mean and amax over dim 1 with keepdim, cat, a 7x7 conv, sigmoid, broadcast
    mul over the channels.  A 1x1 conv closes the file."""
    b = PnnxBuilder(seed)
    x = b.input((batch, 3, size, size))
    f = b.relu(b.conv(x, 16, 3, 1, 1))
    avg, mx = b.mean(f, (2, 3), True), b.amax(f, (2, 3), True)

    def mlp(v, tag):
        return b.conv(b.relu(b.conv(v, 4, 1, name="mlp0_" + tag)), 16, 1, name="mlp1_" + tag)

    a, m = mlp(avg, "avg"), mlp(mx, "max")
    for layer in ("mlp0_", "mlp1_"):   # one MLP: the second pair of lines carries the first pair's weights
        for k in ("weight", "bias"):
            b.attrs[layer + "max." + k] = b.attrs[layer + "avg." + k].copy()
    f = b.mul(f, b.sigmoid(b.add(a, m)))
    s = b.cat([b.mean(f, 1, True), b.amax(f, 1, True)], 1)
    f = b.mul(f, b.sigmoid(b.conv(s, 1, 7, 1, 3)))
    b.output(b.conv(f, 8, 1))
    return b


def build_toy_coordatt(batch: int = 2, height: int = 12, width: int = 20, seed: int = 0) -> PnnxBuilder:
    """Coordinate attention: mean(3, keepdim) -> [N, C, H, 1] and mean(2, keepdim) -> [N, C, 1, W], each through a 1x1 conv and a
    sigmoid, then two broadcast muls; a 1x1 conv closes the file."""
    b = PnnxBuilder(seed)
    x = b.input((batch, 3, height, width))
    f = b.relu(b.conv(x, 16, 3, 1, 1))
    ah = b.sigmoid(b.conv(b.mean(f, 3, True), 16, 1))
    aw = b.sigmoid(b.conv(b.mean(f, 2, True), 16, 1))
    b.output(b.conv(b.mul(b.mul(f, ah), aw), 8, 1))
    return b


def build_toy_layernorm2d(batch: int = 2, size: int = 16, seed: int = 0, eps: str = "1e-06") -> PnnxBuilder:
    """ConvNeXt's channels-first LayerNorm as its export writes it: u = x.mean(1, keepdim), d = x - u, s = (d * d).mean(1, keepdim),
    d / sqrt(s + eps) with the arithmetic in pnnx.Expression operators; a 1x1 conv follows."""
    b = PnnxBuilder(seed)
    x = b.input((batch, 3, size, size))
    f = b.conv(x, 16, 3, 1, 1)
    d = b.expression("sub(@0,@1)", [f, b.mean(f, 1, True)])
    s = b.mean(b.expression("square(@0)", [d]), (1,), True)
    y = b.expression("div(@0,sqrt(add(@1,%s)))" % eps, [d, s])
    b.output(b.conv(y, 8, 1))
    return b


def build_toy_superpoint(batch: int = 2, size: int = 32, functional: bool = False, seed: int = 0) -> PnnxBuilder:
    """SuperPoint in small: a shared stack of three 3x3 convs, each behind a 2x2 max pool (cell size 8), then two heads and two graph outputs.
    Detector: conv -> conv to 65 channels -> softmax(dim=1) -> slice off the dustbin channel -> permute(0,2,3,1) -> reshape(N, Hc, Wc, 8, 8) ->
    permute(0,1,3,2,4) -> reshape(N, 8 Hc, 8 Wc), the depth-to-space of its export.  Descriptor: conv -> conv to 32 channels, then the norm
    as the export writes it out -- dn = torch.norm(desc, p=2, dim=1); desc.div(torch.unsqueeze(dn, 1)) -- or, functional=True,
    F.normalize(desc, p=2, dim=1)."""
    assert size % 8 == 0, size
    b = PnnxBuilder(seed)
    x = b.input((batch, 1, size, size))
    x = b.maxpool(b.relu(b.conv(x, 8, 3, 1, 1)), 2, 2, 0)
    x = b.maxpool(b.relu(b.conv(x, 16, 3, 1, 1)), 2, 2, 0)
    x = b.maxpool(b.relu(b.conv(x, 32, 3, 1, 1)), 2, 2, 0)
    hc = size // 8
    s = b.conv(b.relu(b.conv(x, 32, 3, 1, 1)), 65, 1)
    s = b.slice(b.softmax(s, 1), 1, 0, 64)
    s = b.reshape(b.permute(s, (0, 2, 3, 1)), (batch, hc, hc, 8, 8))
    b.output(b.reshape(b.permute(s, (0, 1, 3, 2, 4)), (batch, hc * 8, hc * 8)))
    d = b.conv(b.relu(b.conv(x, 32, 3, 1, 1)), 32, 1)
    if functional:
        b.output(b.normalize(d, 1, 2.0))
    else:
        b.output(b.div(d, b.unsqueeze(b.norm(d, 1, 2, False), 1)))
    return b


def build_toy_embedding_head(batch: int = 2, size: int = 32, dim: int = 24, seed: int = 0) -> PnnxBuilder:
    """A face / re-ID / retrieval embedding head: a conv stack, x.mean((2, 3)), nn.Linear to `dim` features and F.normalize(dim=1) on the
    rank-2 result: unit rows."""
    b = PnnxBuilder(seed)
    x = b.input((batch, 3, size, size))
    x = b.relu(b.conv(x, 16, 3, 2, 1))
    x = b.relu(b.conv(x, 32, 3, 2, 1))
    b.output(b.normalize(b.linear(b.mean(x, (2, 3)), dim), 1))
    return b


def build_toy_mobilenetv2(batch: int = 2, size: int = 32, seed: int = 0, ncls: int = 10, functional: bool = False) -> PnnxBuilder:
    """MobileNetV2 in small: a 3x3 s2 stem with ReLU6, three inverted-residual blocks -- 1x1 expand, ReLU6, 3x3 depthwise, ReLU6, 1x1 project
    (linear), and the residual add where the stride is 1 and the widths match -- then the global pool, flatten and nn.Linear.
    functional=True: F.relu6 lines."""
    b = PnnxBuilder(seed)
    x = b.input((batch, 3, size, size))
    x = b.relu6(b.conv(x, 8, 3, 2, 1), functional)
    for cout, stride, expand in ((8, 1, 2), (16, 2, 4), (16, 1, 4)):
        cin = b.shapes[x][1]
        y = b.relu6(b.conv(x, cin * expand, 1), functional)
        y = b.relu6(b.conv(y, cin * expand, 3, stride, 1, groups=cin * expand), functional)
        y = b.conv(y, cout, 1)
        x = b.add(x, y) if stride == 1 and cin == cout else y
    x = b.flatten(b.adaptive_avgpool(x, (1, 1)))
    b.output(b.linear(x, ncls))
    return b


def build_toy_csp_mish(batch: int = 2, size: int = 16, seed: int = 0, functional: bool = False) -> PnnxBuilder:
    """A CSPDarknet-Mish block (YOLOv4): a 3x3 s2 conv, two 1x1 branches, a 1x1 / 3x3 residual unit on one of them, torch.cat, a 1x1
    conv -- nn.Mish after every convolution."""
    b = PnnxBuilder(seed)
    m = lambda v: b.mish(v, functional)
    x = b.input((batch, 3, size, size))
    x = m(b.conv(x, 16, 3, 2, 1))
    left, right = m(b.conv(x, 8, 1)), m(b.conv(x, 8, 1))
    r = m(b.conv(m(b.conv(right, 8, 1)), 8, 3, 1, 1))
    right = m(b.conv(b.add(right, r), 8, 1))
    b.output(m(b.conv(b.cat([right, left], 1), 16, 1)))
    return b


def build_toy_clamp_head(batch: int = 2, size: int = 16, seed: int = 0) -> PnnxBuilder:
    """A positive-output head: conv, nn.Softplus, then x.clamp(min=0.1) -- torch.clamp with max=None."""
    b = PnnxBuilder(seed)
    x = b.input((batch, 3, size, size))
    x = b.softplus(b.conv(x, 8, 3, 1, 1))
    b.output(b.clamp(x, min=0.1))
    return b


def build_toy_unet(batch: int = 2, size: int = 64, base: int = 16, depth: int = 3, ncls: int = 4, seed: int = 0,
                   up: str = "convtranspose", norm: str = "bn", act: str = "relu", norm_groups: int = 4, head=None) -> PnnxBuilder:
    """A small U-Net: per encoder level two [conv3x3 -> BatchNorm2d -> ReLU] then MaxPool2d(2, 2); the same block as bottleneck;
    per decoder level an up-conv, torch.cat([skip, up]) and two blocks; a 1x1 conv head.  The up-convs alternate k2 s2 p0 (one
    tap per output pixel) and k3 s2 p1 output_padding 1 (four sub-pixel phases of 4 / 2 / 2 / 1 taps).  up="bilinear": each up-conv
    is nn.Upsample(scale_factor=2, mode="bilinear", align_corners=True) + conv3x3 instead (the other widely used decoder).
    norm="gn": nn.GroupNorm(norm_groups, c) in place of every BatchNorm2d (the diffusion / modern segmentation U-Net block);
    norm="in": nn.InstanceNorm2d(c), no affine (the pix2pix / CycleGAN generator block).  act="silu": nn.SiLU for every ReLU.
    head="softmax" / "log_softmax": nn.Softmax(dim=1) / nn.LogSoftmax(dim=1) over the classes of the 1x1 conv head."""
    assert up in ("convtranspose", "bilinear"), up
    assert norm in ("bn", "gn", "in") and act in ("relu", "silu"), (norm, act)
    b = PnnxBuilder(seed)
    x = b.input((batch, 3, size, size))

    def block(x, c):
        for _ in range(2):
            x = b.conv(x, c, 3, 1, 1)
            x = b.batchnorm(x) if norm == "bn" else b.group_norm(x, norm_groups) if norm == "gn" else b.instance_norm(x)
            x = b.relu(x) if act == "relu" else b.silu(x)
        return x

    skips, c = [], base
    for _ in range(depth):
        x = block(x, c)
        skips.append(x)
        x = b.maxpool(x, 2, 2, 0)
        c *= 2
    x = block(x, c)
    for i, skip in enumerate(reversed(skips)):
        c //= 2
        if up == "bilinear":
            u = b.conv(b.upsample(x, 2.0, mode="bilinear", align_corners=True), c, 3, 1, 1)
        else:
            u = b.conv_transpose(x, c, 2, 2, 0) if i % 2 == 0 else b.conv_transpose(x, c, 3, 2, 1, output_padding=1)
        x = block(b.cat([skip, u]), c)
    x = b.conv(x, ncls, 1, 1, 0)
    b.output(b._head(x, head))
    return b


def build_toy_cyclegan(batch: int = 2, size: int = 32, base: int = 8, blocks: int = 2, pad: str = "reflect", seed: int = 0) -> PnnxBuilder:
    """The CycleGAN / Johnson style-transfer ResNet generator at toy width: ReflectionPad2d(3) -> conv7x7 (p = 0) -> InstanceNorm2d
    (no affine) -> ReLU; two stride-2 conv3x3 -> IN -> ReLU; `blocks` residual blocks [pad 1 -> conv3x3 (p = 0) -> IN -> ReLU ->
    pad 1 -> conv3x3 (p = 0) -> IN] + x; two ConvTranspose2d(3, s2, p1, op1) -> IN -> ReLU; ReflectionPad2d(3) -> conv7x7 -> Tanh.
    pad: the mode of every explicit pad ("reflect", "replicate", "circular", "constant").  At size 32 the residual blocks run at
    8 x 8: every reflect pad is below its input size."""
    b = PnnxBuilder(seed)
    x = b.input((batch, 3, size, size))

    def cnr(x, c, k, s, p):
        return b.relu(b.instance_norm(b.conv(x, c, k, s, p)))

    x = cnr(b.pad(x, 3, pad), base, 7, 1, 0)
    x = cnr(x, 2 * base, 3, 2, 1)
    x = cnr(x, 4 * base, 3, 2, 1)
    for _ in range(blocks):
        y = cnr(b.pad(x, 1, pad), 4 * base, 3, 1, 0)
        y = b.instance_norm(b.conv(b.pad(y, 1, pad), 4 * base, 3, 1, 0))
        x = b.add(x, y)
    for c in (2 * base, base):
        x = b.relu(b.instance_norm(b.conv_transpose(x, c, 3, 2, 1, output_padding=1)))
    x = b.tanh(b.conv(b.pad(x, 3, pad), 3, 7, 1, 0))
    b.output(x)
    return b


def build_toy_espcn(batch: int = 2, size: int = 16, r: int = 2, channels: int = 3, width: int = 16, seed: int = 0) -> PnnxBuilder:
    """ESPCN (sub-pixel CNN) at toy width: conv5x5 -> Tanh -> conv3x3 -> Tanh -> conv3x3 to channels * r * r -> PixelShuffle(r)"""
    b = PnnxBuilder(seed)
    x = b.input((batch, channels, size, size))
    x = b.tanh(b.conv(x, width, 5, 1, 2))
    x = b.tanh(b.conv(x, width // 2, 3, 1, 1))
    x = b.pixel_shuffle(b.conv(x, channels * r * r, 3, 1, 1), r)
    b.output(x)
    return b


def build_toy_srresnet(batch: int = 2, size: int = 12, width: int = 16, blocks: int = 2, seed: int = 0) -> PnnxBuilder:
    """SRResNet (the SRGAN generator) at toy width, x4: conv9x9 -> PReLU; `blocks` residual blocks [conv3x3 -> BN -> PReLU -> conv3x3 ->
    BN] + x; conv3x3 -> BN, + the long skip from the first PReLU; two upsampling stages conv3x3 to 4 * width -> PixelShuffle(2) ->
    PReLU; conv9x9 to RGB -> Tanh.  The PReLUs alternate between one shared slope (torch's default, what SRGAN uses) and one per
    channel."""
    b = PnnxBuilder(seed)
    x = b.input((batch, 3, size, size))
    x = first = b.prelu(b.conv(x, width, 9, 1, 4))
    for k in range(blocks):
        y = b.prelu(b.batchnorm(b.conv(x, width, 3, 1, 1)), width if k % 2 else 1)
        y = b.batchnorm(b.conv(y, width, 3, 1, 1))
        x = b.add(x, y)
    x = b.add(first, b.batchnorm(b.conv(x, width, 3, 1, 1)))
    for k in range(2):
        x = b.prelu(b.pixel_shuffle(b.conv(x, 4 * width, 3, 1, 1), 2), 1 if k % 2 else width)
    x = b.tanh(b.conv(x, 3, 9, 1, 4))
    b.output(x)
    return b


def build_toy_esrgan_head(batch: int = 2, size: int = 16, width: int = 16, seed: int = 0) -> PnnxBuilder:
    """The x2 head and tail of Real-ESRGAN's generator at toy width: PixelUnshuffle(2) (3 -> 12 channels at half the size) -> conv3x3 ->
    LeakyReLU(0.2) -> nearest Upsample x2 -> conv3x3 to RGB"""
    b = PnnxBuilder(seed)
    x = b.input((batch, 3, size, size))
    x = b.leaky_relu(b.conv(b.pixel_unshuffle(x, 2), width, 3, 1, 1), 0.2)
    x = b.conv(b.upsample(x, 2.0), 3, 3, 1, 1)
    b.output(x)
    return b


def build_toy_c2f(batch: int = 2, size: int = 16, c1: int = 16, c2: int = 32, n: int = 2, shortcut: bool = True, seed: int = 0) -> PnnxBuilder:
    """YOLOv8's C2f block: cv1 (1x1 to 2 c) -> chunk(2, 1) -> n bottlenecks (3x3 -> 3x3, + shortcut), each fed by the tensor before it ->
    cat of both halves and every bottleneck output -> cv2 (1x1); c = c2 / 2, every conv with SiLU"""
    b = PnnxBuilder(seed)
    x = b.input((batch, c1, size, size))
    c = c2 // 2
    y = b.chunk(_Conv(b, x, 2 * c, 1), 2, 1)
    for _ in range(n):
        t = _Conv(b, _Conv(b, y[-1], c, 3), c, 3)
        y.append(b.add(y[-1], t) if shortcut else t)
    b.output(_Conv(b, b.cat(y, 1), c2, 1))
    return b


def build_toy_focus(batch: int = 2, size: int = 16, c2: int = 16, seed: int = 0) -> PnnxBuilder:
    """The Focus stem of YOLOv5 v1 - v5: cat of x[..., ::2, ::2], x[..., 1::2, ::2], x[..., ::2, 1::2], x[..., 1::2, 1::2] (3 -> 12 channels at
    half the size) -> conv3x3 with SiLU"""
    b = PnnxBuilder(seed)
    x = b.input((batch, 3, size, size))
    parts = [b.slice(x, (2, 3), (i, j), (None, None), (2, 2)) for i, j in ((0, 0), (1, 0), (0, 1), (1, 1))]
    b.output(_Conv(b, b.cat(parts, 1), c2, 3))
    return b


def build_toy_res2net_block(batch: int = 2, size: int = 12, width: int = 8, scale: int = 4, seed: int = 0) -> PnnxBuilder:
    """A Res2Net bottleneck at toy width: conv3x3 stem -> conv1x1 to width * scale -> torch.split(width, 1) -> the hierarchical 3x3 convs
    (piece i plus the output before it; the last piece passes through) -> cat -> conv1x1, + the block's input, ReLU"""
    b = PnnxBuilder(seed)
    x = b.input((batch, 3, size, size))
    x = b.relu(b.conv(x, width * scale, 3, 1, 1))
    xs = b.split(b.relu(b.conv(x, width * scale, 1)), width, 1)
    outs, sp = [], None
    for i in range(scale - 1):
        sp = b.relu(b.conv(xs[i] if i == 0 else b.add(sp, xs[i]), width, 3, 1, 1))
        outs.append(sp)
    outs.append(xs[-1])
    y = b.conv(b.cat(outs, 1), width * scale, 1)
    b.output(b.relu(b.add(y, x)))
    return b


def build_toy_ghost(batch: int = 2, size: int = 16, oup: int = 27, seed: int = 0) -> PnnxBuilder:
    """GhostNet's Ghost module: primary conv1x1 to ceil(oup / 2) channels -> cheap depthwise conv3x3 over them -> cat -> out[:, :oup]"""
    b = PnnxBuilder(seed)
    x = b.input((batch, 16, size, size))
    init = -(-oup // 2)
    x1 = b.relu(b.conv(x, init, 1))
    x2 = b.relu(b.conv(x1, init, 3, 1, 1, groups=init))
    b.output(b.slice(b.cat([x1, x2], 1), 1, 0, oup, 1))
    return b


def _toy_pyramid(b: PnnxBuilder, batch: int, size: int, c: int = 16, levels: int = 2) -> List[str]:
    """a stem and `levels` stride-2 feature maps (size / 4, size / 8, ..) of c, 2c, .. channels"""
    x = b.relu(b.conv(b.input((batch, 3, size, size)), c, 3, 2, 1))
    feats = []
    for lv in range(levels):
        x = b.relu(b.conv(x, c << lv, 3, 2, 1))
        feats.append(x)
    return feats


def build_toy_ssd_head(batch: int = 2, size: int = 32, num_classes: int = 3, anchors: int = 2, seed: int = 0) -> PnnxBuilder:
    """An SSD / RetinaFace style head on two levels: loc and conf convs, each conv -> permute(0,2,3,1) -> view(N,-1,4 | K) -- the bytes the conv
    wrote, in order --, cat(dim=1) over the levels, sigmoid on the scores, cat(dim=2): [N, anchors, 4 + K]."""
    b = PnnxBuilder(seed)
    locs, confs = [], []
    for f in _toy_pyramid(b, batch, size):
        locs.append(b.view(b.permute(b.conv(f, anchors * 4, 3, 1, 1), (0, 2, 3, 1)), (batch, -1, 4)))
        confs.append(b.view(b.permute(b.conv(f, anchors * num_classes, 3, 1, 1), (0, 2, 3, 1)), (batch, -1, num_classes)))
    b.output(b.cat([b.cat(locs, 1), b.sigmoid(b.cat(confs, 1))], 2))
    return b


def build_toy_anchorfree_head(batch: int = 2, size: int = 64, no: int = 32, seed: int = 0) -> PnnxBuilder:
    """A YOLOX / YOLOv8 style head: per level a conv to `no` channels -> view(N, no, -1); cat(dim=2) over the levels -> permute(0,2,1):
    [N, cells, no]."""
    b = PnnxBuilder(seed)
    rows = [b.view(b.conv(f, no, 1), (batch, no, -1)) for f in _toy_pyramid(b, batch, size)]
    b.output(b.permute(b.cat(rows, 2), (0, 2, 1)))
    return b


def build_toy_yolov8_seg(batch: int = 2, size: int = 64, nc: int = 5, nm: int = 32, channels_first: bool = True, seed: int = 0) -> PnnxBuilder:
    """A YOLOv8-seg style export: per level a conv to no = 4 + nc + nm channels (box as cx cy w h, class scores, mask coefficients) -> view(N, no, -1);
    cat(dim=2) over the levels: [N, no, cells], channel-major as ultralytics exports it -- or [N, cells, no] behind the closing permute(0,2,1)
    when channels_first is False; and the prototype branch, two convs on the finest level: [N, nm, size / 4, size / 4], a second graph output."""
    b = PnnxBuilder(seed)
    feats = _toy_pyramid(b, batch, size)
    no = 4 + nc + nm
    rows = []
    for lv, f in enumerate(feats):
        name = "seg_head_%d" % lv
        rows.append(b.view(b.conv(f, no, 1, name=name), (batch, no, -1)))
        # boxes of a plausible size around the image centre instead of a few pixels around the origin: they overlap, and they cover mask pixels
        b.attrs[name + ".weight"][:4] *= size / 2.0
        b.attrs[name + ".bias"][:4] = (size / 2.0, size / 2.0, size / 3.0, size / 3.0)
    y = b.cat(rows, 2)
    b.output(y if channels_first else b.permute(y, (0, 2, 1)))
    b.output(b.conv(b.relu(b.conv(feats[0], nm, 3, 1, 1)), nm, 1))
    return b


def build_toy_yolov5_raw_head(batch: int = 2, size: int = 32, na: int = 3, no: int = 7, seed: int = 0) -> PnnxBuilder:
    """A raw YOLOv5 export's head: per level conv to na * no channels -> view(N, na, no, H, W) -> permute(0,1,3,4,2) -> view(N, -1, no) (the
    rank-5 route), sigmoid, cat(dim=1) over the levels: [N, na * cells, no]."""
    b = PnnxBuilder(seed)
    rows = []
    for f in _toy_pyramid(b, batch, size):
        y = b.conv(f, na * no, 1)
        _, _, h, w = b.shapes[y]
        y = b.view(b.permute(b.view(y, (batch, na, no, h, w)), (0, 1, 3, 4, 2)), (batch, -1, no))
        rows.append(b.sigmoid(y))
    b.output(b.cat(rows, 1))
    return b


def build_toy_view_classifier(batch: int = 2, size: int = 32, pool: int = 1, ncls: int = 10, flatten: bool = False, seed: int = 0) -> PnnxBuilder:
    """conv stack -> adaptive average pool to (pool, pool) -> x.view(N, -1) -> nn.Linear.  pool=1: the view moves no byte; pool=2: a transpose
    of [4, C] per image.  flatten=True writes torch.flatten in place of the view (the same model, for the A/B)."""
    b = PnnxBuilder(seed)
    x = _toy_pyramid(b, batch, size)[-1]
    x = b.adaptive_avgpool(x, (pool, pool))
    x = b.flatten(x) if flatten else b.view(x, (batch, -1))
    b.output(b.linear(x, ncls))
    return b


def build_toy_c3tr(batch: int = 2, size: int = 32, c: int = 32, heads: int = 4, layers: int = 2, seed: int = 0) -> PnnxBuilder:
    """YOLOv5's C3TR / TransformerBlock as its export writes it: conv -> torch.flatten(start_dim=2) -> Tensor.permute(2, 0, 1) ->
    p + linear(p); per layer three bias-free Linears -> nn.MultiheadAttention with 3 inputs -> + x -> fc2(fc1(x)) + x (no LayerNorm, no
    activation); then permute(1, 2, 0) -> reshape(b, c, w, h) -> conv.  Tokens are seq-first [L, N, E]."""
    b = PnnxBuilder(seed)
    x = b.silu(b.conv(b.input((batch, 3, size, size)), c, 3, 2, 1))
    x = b.silu(b.conv(x, c, 3, 2, 1))
    _, _, h, w = b.shapes[x]
    p = b.permute(b.flatten(x, 2), (2, 0, 1))
    x = b.add(p, b.linear(p, c))
    for _ in range(layers):
        q, k, v = (b.linear(x, c, bias=False) for _ in range(3))
        x = b.add(b.multihead_attention(q, k, v, num_heads=heads), x)
        x = b.add(b.linear(b.linear(x, c, bias=False), c, bias=False), x)
    x = b.reshape(b.permute(x, (1, 2, 0)), (batch, c, w, h))
    b.output(b.silu(b.conv(x, c, 1)))
    return b


def build_toy_mhsa_head(batch: int = 2, size: int = 16, c: int = 24, heads: int = 3, seed: int = 0) -> PnnxBuilder:
    """A self-attention pooling head on batch-first tokens: convs -> permute(0, 2, 3, 1) -> view(N, -1, C) (a view, not a launch) ->
    nn.MultiheadAttention(batch_first=True) with one input -> the mean over the tokens -> nn.Linear.  The mean is written on the feature map
    the tokens came from, permute(0, 2, 1) -> view(N, C, H, W) (again a view) -> mean((2, 3)): reductions over a rank-3 operand are not served."""
    b = PnnxBuilder(seed)
    x = b.relu(b.conv(b.input((batch, 3, size, size)), 16, 3, 2, 1))
    x = b.relu(b.conv(x, c, 3, 1, 1))
    _, _, h, w = b.shapes[x]
    t = b.view(b.permute(x, (0, 2, 3, 1)), (batch, -1, c))
    t = b.multihead_attention(t, num_heads=heads, batch_first=True)
    m = b.mean(b.view(b.permute(t, (0, 2, 1)), (batch, c, h, w)), (2, 3))
    b.output(b.linear(m, 10))
    return b


def build_toy_crnn(batch: int = 2, height: int = 16, width: int = 40, hidden: int = 32, layers: int = 2, cell: str = "lstm",
                   bidirectional: bool = True, batch_first: bool = False, states: bool = False, channels: int = 32, ncls: int = 11,
                   seed: int = 0) -> PnnxBuilder:
    """A CRNN text recogniser at toy width: three conv + ReLU + max pool stages that take the height to 1 and the width to width / 4 ->
    torch.flatten(start_dim=2) [N, C, T] -> Tensor.permute(2, 0, 1) [T, N, C] (batch_first: (0, 2, 1), [N, T, C]) -> nn.LSTM / nn.GRU ->
    nn.Linear to the classes, per time step.  No softmax: the argmax over the classes is the host's.  states=True: the operator's state outputs
    are operands too, and h_n feeds a second nn.Linear whose result is a second graph output."""
    assert height % 4 == 0 and width % 4 == 0 and cell in ("lstm", "gru")
    b = PnnxBuilder(seed)
    x = b.maxpool(b.relu(b.conv(b.input((batch, 3, height, width)), 16, 3, 1, 1)), 2, 2, 0)
    x = b.maxpool(b.relu(b.conv(x, channels, 3, 1, 1)), 2, 2, 0)
    x = b.maxpool(b.relu(b.conv(x, channels, 3, 1, 1)), (height // 4, 1), (height // 4, 1), 0)
    t = b.permute(b.flatten(x, 2), (0, 2, 1) if batch_first else (2, 0, 1))
    rec = b.lstm if cell == "lstm" else b.gru
    y = rec(t, hidden, num_layers=layers, batch_first=batch_first, bidirectional=bidirectional, states=states)
    if states:
        b.output(b.linear(y[0], ncls))
        b.output(b.linear(y[1], ncls))
    else:
        b.output(b.linear(y, ncls))
    return b


def build_toy_quartznet(batch: int = 2, frames: int = 64, feats: int = 16, width: int = 32, ncls: int = 12, seed: int = 0) -> PnnxBuilder:
    """QuartzNet at toy width on a rank-3 graph input [N, feats, T]: a strided dense stem (K = 11, stride 2) + ReLU; two blocks of depthwise
    K = 33 -> pointwise -> ReLU with a pointwise residual branch, `+`, ReLU; a dilated K = 3 conv (dilation 2, `same`) + ReLU; a pointwise conv
    to the classes, per frame [N, ncls, T / 2].  BatchNorm1d is absent as pnnx folds it into the convs at export"""
    b = PnnxBuilder(seed)
    x = b.relu(b.conv1d(b.input((batch, feats, frames)), width, 11, 2, 5))
    for _ in range(2):
        y = b.relu(b.conv1d(b.conv1d(x, width, 33, 1, 16, groups=width), width, 1, 1, 0))
        x = b.relu(b.add(y, b.conv1d(x, width, 1, 1, 0)))
    x = b.relu(b.conv1d(x, width, 3, 1, "same", d=2))
    b.output(b.conv1d(x, ncls, 1, 1, 0))
    return b


def build_toy_conv_gru(batch: int = 2, frames: int = 50, feats: int = 8, width: int = 16, hidden: int = 16, ncls: int = 9,
                       seed: int = 0) -> PnnxBuilder:
    """A DeepSpeech2-style front end at toy width: two strided nn.Conv1d + nn.Hardtanh(0, 20) on [N, feats, T] -> Tensor.permute(2, 0, 1)
    [T', N, C] -> nn.GRU -> nn.Linear to the classes, per time step"""
    b = PnnxBuilder(seed)
    x = b.hardtanh(b.conv1d(b.input((batch, feats, frames)), width, 11, 2, 5), 0.0, 20.0)
    x = b.hardtanh(b.conv1d(x, width, 5, 2, 2), 0.0, 20.0)
    b.output(b.linear(b.gru(b.permute(x, (2, 0, 1)), hidden), ncls))
    return b


def build_toy_siamfc(batch: int = 1, seed: int = 0) -> PnnxBuilder:
    """SiamFC at toy width: two graph inputs, the template z [1, 3, 17, 17] and the search image x [N, 3, 33, 33], each through a stack of two
    valid 3x3 convs (3 -> 8 + ReLU, 8 -> 16; the two stacks have weights of their own: pnnx writes a shared module once per call all the same);
    the response map is F.conv2d(search features [N, 16, 29, 29], template features [1, 16, 13, 13]) -> [N, 1, 17, 17]: the dense form, O = 1"""
    b = PnnxBuilder(seed)
    z, x = b.input((1, 3, 17, 17)), b.input((batch, 3, 33, 33))
    fz = b.conv(b.relu(b.conv(z, 8, 3, 1, 0)), 16, 3, 1, 0)
    fx = b.conv(b.relu(b.conv(x, 8, 3, 1, 0)), 16, 3, 1, 0)
    b.output(b.conv2d_functional(fx, fz))
    return b


def build_toy_siamrpn(k: int = 5, batch: int = 1, seed: int = 0) -> PnnxBuilder:
    """SiamRPN's up-channel classification branch at toy width: the template z [1, 3, 12, 12] -> conv 3 -> 8 + ReLU -> conv 8 -> 2k * 8, 7x7
    valid -> [1, 2k * 8, 4, 4] -> Tensor.view to 2k filters [2k, 8, 4, 4]; the search image x [N, 3, 20, 20] -> two convs -> [N, 8, 16, 16];
    F.conv2d(x features, filters) -> [N, 2k, 13, 13] -> ReLU (the launch's epilogue)"""
    b = PnnxBuilder(seed)
    z, x = b.input((1, 3, 12, 12)), b.input((batch, 3, 20, 20))
    fz = b.conv(b.relu(b.conv(z, 8, 3, 1, 0)), 2 * k * 8, 7, 1, 0)
    fx = b.conv(b.relu(b.conv(x, 8, 3, 1, 0)), 8, 3, 1, 0)
    b.output(b.relu(b.conv2d_functional(fx, b.view(fz, (2 * k, 8, 4, 4)))))
    return b


def build_toy_siamrpnpp(batch: int = 1, c: int = 8, seed: int = 0) -> PnnxBuilder:
    """SiamRPN++'s depthwise cross-correlation at toy width: z [N, 3, 11, 11] and x [N, 3, 19, 19] through two valid 3x3 convs each ->
    [N, c, 7, 7] and [N, c, 15, 15]; the sandwich x.view(1, N c, 15, 15), z.view(N c, 1, 7, 7), F.conv2d(groups = N c), .view(N, c, 9, 9);
    a 1x1 head c -> 4 behind it"""
    b = PnnxBuilder(seed)
    z, x = b.input((batch, 3, 11, 11)), b.input((batch, 3, 19, 19))
    fz = b.conv(b.relu(b.conv(z, c, 3, 1, 0)), c, 3, 1, 0)
    fx = b.conv(b.relu(b.conv(x, c, 3, 1, 0)), c, 3, 1, 0)
    y = b.conv2d_functional(b.view(fx, (1, batch * c, 15, 15)), b.view(fz, (batch * c, 1, 7, 7)), groups=batch * c)
    b.output(b.conv(b.view(y, (batch, c, 9, 9)), 4, 1, 1, 0))
    return b


def build_toy_dynamic_head(batch: int = 1, constant: bool = False, seed: int = 0) -> PnnxBuilder:
    """SOLOv2 / CondInst at toy width: the mask feature x [N, 3, 16, 16] -> conv 3 -> 8 + ReLU; the kernel branch pools it to [1, 8, 1, 1] and a
    1x1 conv predicts 4 * 8 values, viewed as four 1x1 kernels [4, 8, 1, 1] (batch 1: a kernel set belongs to one image);
    F.conv2d(feature, kernels) -> [N, 4, 16, 16] -> Sigmoid.  constant=True: the kernels are a constant of the file behind the same view --
    filters DERIVED from a constant, which the batch modes may cut"""
    b = PnnxBuilder(seed)
    assert constant or batch == 1
    f = b.relu(b.conv(b.input((batch, 3, 16, 16)), 8, 3, 1, 1))
    if constant:
        k = b.attribute(seeded_uniform("dynamic_head.kernels", (1, 32, 1, 1), -0.5, 0.5, seed))
    else:
        k = b.conv(b.adaptive_avgpool(f, (1, 1)), 32, 1, 1, 0)
    b.output(b.sigmoid(b.conv2d_functional(f, b.view(k, (4, 8, 1, 1)))))
    return b


def build_toy_blurpool(batch: int = 2, c: int = 8, seed: int = 0) -> PnnxBuilder:
    """Anti-aliased downsampling (timm's BlurPool2d): conv 3 -> c + ReLU, then F.conv2d(x, buffer, stride=2, padding=1, groups=c) with the
    binomial 3x3 filter [c, 1, 3, 3] / 16 kept as a constant of the file, then a 1x1 head.  The engine lowers the function to nn.Conv2d"""
    b = PnnxBuilder(seed)
    x = b.relu(b.conv(b.input((batch, 3, 16, 16)), c, 3, 1, 1))
    a = np.array([1.0, 2.0, 1.0], np.float32)
    blur = np.broadcast_to((a[:, None] * a[None, :] / 16.0)[None, None], (c, 1, 3, 3))
    b.output(b.conv(b.conv2d_functional(x, b.attribute(blur), stride=2, padding=1, groups=c), 4, 1, 1, 0))
    return b


def build_toy_dcn_head(batch: int = 2, size: int = 32, mask: bool = True, seed: int = 0) -> PnnxBuilder:
    """The usual DCNv2 block at toy width: stem conv 3 -> 16 stride 2 + SiLU; an offset conv 3x3 16 -> 27 whose output torch.split([18, 9]) cuts
    into the offsets (a channel view) and the mask logits -> nn.Sigmoid; torchvision.ops.DeformConv2d 16 -> 24 3x3 pad 1 on (x, offset, mask)
    + ReLU; a 1x1 conv to 8 channels.  mask=False: DCNv1 -- an 18-channel offset conv and two inputs."""
    b = PnnxBuilder(seed)
    x = b.silu(b.conv(b.input((batch, 3, size, size)), 16, 3, 2, 1))
    if mask:
        off, m = b.split(b.conv(x, 27, 3, 1, 1), [18, 9], 1)
        y = b.deform_conv(x, off, b.sigmoid(m), cout=24, k=3, s=1, p=1)
    else:
        y = b.deform_conv(x, b.conv(x, 18, 3, 1, 1), cout=24, k=3, s=1, p=1)
    b.output(b.conv(b.relu(y), 8, 1))
    return b


def build_toy_stn(batch: int = 2, size: int = 32, seed: int = 0) -> PnnxBuilder:
    """A spatial transformer at toy width: the localisation net conv 3 -> 8 stride 2 + ReLU -> maxpool 2 -> conv 8 -> 16 -> AdaptiveAvgPool2d(1) ->
    flatten -> Linear(6) whose bias is the identity transform (1, 0, 0, 0, 1, 0) and whose weight is small, so theta stays near the identity ->
    view(N, 2, 3) -> F.affine_grid(size of the image) -> F.grid_sample(image, grid; bilinear, zeros, align_corners=False) -> conv 3 -> 8."""
    b = PnnxBuilder(seed)
    img = b.input((batch, 3, size, size))
    x = b.relu(b.conv(img, 8, 3, 2, 1))
    x = b.conv(b.maxpool(x, 2, 2, 0), 16, 3, 1, 1)
    x = b.flatten(b.adaptive_avgpool(x, (1, 1)))
    theta = b.linear(x, 6)
    name = "linear_%d" % (b._counts["linear"] - 1)
    b.attrs[name + ".weight"] *= np.float32(0.25)
    b.attrs[name + ".bias"][:] = np.asarray([1, 0, 0, 0, 1, 0], np.float32)
    grid = b.affine_grid(b.view(theta, (batch, 2, 3)), (batch, 3, size, size), align_corners=False)
    b.output(b.conv(b.grid_sample(img, grid, "bilinear", "zeros", False), 8, 3, 1, 1))
    return b


def build_toy_flow_warp(batch: int = 2, height: int = 24, width: int = 20, c: int = 8, seed: int = 0) -> PnnxBuilder:
    """Warping features by a predicted flow (EDVR / BasicVSR++ / RIFE style).  Two graph inputs: the image [N, 3, H, W] and a channels-first
    base grid [N, 2, H, W] (channel 0 x, channel 1 y, normalised for align_corners=True: flow_base_grid; build_toy_flow_warp_const holds it
    as a graph constant instead).  A feature conv 3 -> c; a 3x3 flow conv c -> 2 + nn.Tanh; base + flow -> permute(0, 2, 3, 1) ->
    F.grid_sample(features, grid; bilinear, border, align_corners=True) -> 1x1 conv c -> c."""
    b = PnnxBuilder(seed)
    img = b.input((batch, 3, height, width))
    base = b.input((batch, 2, height, width))
    feat = b.conv(img, c, 3, 1, 1)
    flow = b.tanh(b.conv(feat, 2, 3, 1, 1))
    grid = b.permute(b.add(base, flow), (0, 2, 3, 1))
    b.output(b.conv(b.grid_sample(feat, grid, "bilinear", "border", True), c, 1))
    return b


def build_toy_flow_warp_const(batch: int = 2, height: int = 24, width: int = 20, c: int = 8, seed: int = 0) -> PnnxBuilder:
    """build_toy_flow_warp as an export writes it: the base grid is a graph constant [1, 2, H, W] (flow_base_grid in file order), broadcast
    over the batch by the add, and the image is the only graph input.  Same weights, same operators otherwise."""
    b = PnnxBuilder(seed)
    img = b.input((batch, 3, height, width))
    base = b.attribute(flow_base_grid(1, height, width).transpose(0, 3, 1, 2))
    feat = b.conv(img, c, 3, 1, 1)
    flow = b.tanh(b.conv(feat, 2, 3, 1, 1))
    grid = b.permute(b.expression("add(@0,@1)", [base, flow], b.shapes[flow]), (0, 2, 3, 1))
    b.output(b.conv(b.grid_sample(feat, grid, "bilinear", "border", True), c, 1))
    return b


def build_toy_frozenbn_block(batch: int = 2, size: int = 16, c: int = 16, seed: int = 0) -> PnnxBuilder:
    """A torchvision detection backbone's residual block: FrozenBatchNorm2d is no module to pnnx but `x * scale + shift`, one
    pnnx.Expression over two [1, C, 1, 1] constants.  stem conv 3 -> c stride 2 + ReLU; conv 3x3 -> frozen bn -> ReLU -> conv 3x3 ->
    frozen bn -> + skip -> ReLU."""
    b = PnnxBuilder(seed)
    x = b.relu(b.conv(b.input((batch, 3, size, size)), c, 3, 2, 1))

    def frozen_bn(y, tag):
        scale = b.attribute(seeded_uniform(tag + ".scale", (1, c, 1, 1), 0.5, 1.5, seed))
        shift = b.attribute(seeded_uniform(tag + ".shift", (1, c, 1, 1), -0.5, 0.5, seed))
        return b.expression("add(mul(@0,@1),@2)", [y, scale, shift])

    y = b.relu(frozen_bn(b.conv(x, c, 3, 1, 1, bias=False), "fbn0"))
    y = frozen_bn(b.conv(y, c, 3, 1, 1, bias=False), "fbn1")
    b.output(b.relu(b.add(y, x)))
    return b


def build_toy_layer_scale(batch: int = 2, size: int = 16, c: int = 24, seed: int = 0) -> PnnxBuilder:
    """A ConvNeXt-style block at toy width: stem conv 3 -> c stride 2; depthwise 3x3 -> 1x1 + ReLU -> 1x1 -> gamma * y with the layer scale
    gamma a constant [C, 1, 1] on the LEFT (rank 3 against rank 4: torch right-aligns it to [1, C, 1, 1]) -> + x."""
    b = PnnxBuilder(seed)
    x = b.conv(b.input((batch, 3, size, size)), c, 3, 2, 1)
    y = b.conv(b.relu(b.conv(b.conv(x, c, 3, 1, 1, groups=c), 2 * c, 1)), c, 1)
    gamma = b.attribute(seeded_uniform("layer_scale.gamma", (c, 1, 1), 0.05, 0.5, seed))
    b.output(b.add(b.expression("mul(@0,@1)", [gamma, y], b.shapes[y]), x))
    return b


def build_toy_pos_embed(batch: int = 2, size: int = 16, c: int = 32, heads: int = 4, batch_first: bool = False, seed: int = 0) -> PnnxBuilder:
    """Learned position embeddings on tokens around nn.MultiheadAttention.  Seq-first (C3TR's order): convs -> flatten(2) -> permute(2, 0, 1),
    tokens [L, N, E] + a constant [L, 1, E].  batch_first: permute(0, 2, 1), tokens [N, L, E] + a constant [1, L, E].  Then self-attention
    + x and a Linear."""
    b = PnnxBuilder(seed)
    x = b.silu(b.conv(b.input((batch, 3, size, size)), c, 3, 2, 1))
    x = b.silu(b.conv(x, c, 3, 2, 1))
    _, _, h, w = b.shapes[x]
    t = b.permute(b.flatten(x, 2), (0, 2, 1) if batch_first else (2, 0, 1))
    pos = b.attribute(seeded_uniform("pos_embed", (1, h * w, c) if batch_first else (h * w, 1, c), -0.5, 0.5, seed))
    t = b.expression("add(@0,@1)", [t, pos])
    t = b.add(b.multihead_attention(t, num_heads=heads, batch_first=batch_first), t)
    b.output(b.linear(t, c))
    return b


def build_toy_fcos_scale(batch: int = 2, size: int = 32, seed: int = 0) -> PnnxBuilder:
    """FCOS's box regression: per pyramid level conv -> exp(x * s) with s a learned scalar, a constant of shape [1] per level; the two
    levels are two graph outputs."""
    b = PnnxBuilder(seed)
    for i, f in enumerate(_toy_pyramid(b, batch, size)):
        s = b.attribute(np.asarray([0.75 + 0.5 * i], np.float32))
        y = b.conv(f, 4, 3, 1, 1)
        b.output(b.expression("exp(mul(@0,@1))", [y, s]))
    return b


def flow_base_grid(batch: int, height: int, width: int) -> np.ndarray:
    """the base grid input of build_toy_flow_warp as an NHWC array [N, H, W, 2] (the storage of the channels-first [N, 2, H, W] operand):
    torch.linspace(-1, 1, size) per axis, x in channel 0 and y in channel 1 -- the identity warp under align_corners=True"""
    xs = np.linspace(-1.0, 1.0, width, dtype=np.float64) if width > 1 else np.zeros(1)
    ys = np.linspace(-1.0, 1.0, height, dtype=np.float64) if height > 1 else np.zeros(1)
    g = np.empty((batch, height, width, 2), np.float32)
    g[..., 0] = xs[None, None, :]
    g[..., 1] = ys[None, :, None]
    return g


def build_toy_box_head(batch: int = 2, boxes: int = 6, c: int = 8, height: int = 20, width: int = 24, classes: int = 5, seed: int = 0,
                       spatial_scale: float = 0.25, sampling_ratio: int = 2, aligned: bool = False) -> PnnxBuilder:
    """The box head of Faster R-CNN at toy width.  Two graph inputs: the features [N, c, H, W] and the boxes [K, 5], rows (image index, x1,
    y1, x2, y2) in image pixels.  RoIAlign 7x7 -> 3x3 conv c -> 2c + ReLU -> flatten -> Linear(32) + ReLU -> two Linear heads: the class
    scores [K, classes] and the box deltas [K, 4 classes]."""
    b = PnnxBuilder(seed)
    feat = b.input((batch, c, height, width))
    rois = b.input((boxes, 5))
    x = b.roi_align(feat, rois, 7, spatial_scale, sampling_ratio, aligned)
    x = b.relu(b.conv(x, 2 * c, 3, 1, 1))
    x = b.relu(b.linear(b.flatten(x), 32))
    scores, deltas = b.linear(x, classes), b.linear(x, 4 * classes)
    b.output(scores)
    b.output(deltas)
    return b


def build_toy_mask_head(batch: int = 2, boxes: int = 5, c: int = 8, height: int = 20, width: int = 24, classes: int = 3, seed: int = 0,
                        spatial_scale: float = 0.25, sampling_ratio: int = 2, aligned: bool = True) -> PnnxBuilder:
    """The mask head of Mask R-CNN at toy width.  Graph inputs as build_toy_box_head's.  The functional torchvision.ops.roi_align 14x14 -> two
    3x3 convs c -> c + ReLU -> ConvTranspose2d 2x2 stride 2 + ReLU -> 1x1 conv to `classes` -> Sigmoid: masks [K, classes, 28, 28]."""
    b = PnnxBuilder(seed)
    feat = b.input((batch, c, height, width))
    rois = b.input((boxes, 5))
    x = b.roi_align(feat, rois, 14, spatial_scale, sampling_ratio, aligned, functional=True)
    x = b.relu(b.conv(x, c, 3, 1, 1))
    x = b.relu(b.conv(x, c, 3, 1, 1))
    x = b.relu(b.conv_transpose(x, c, 2, 2))
    b.output(b.sigmoid(b.conv(x, classes, 1)))
    return b


def toy_rois(boxes: int, batch: int, height: int, width: int, spatial_scale: float = 0.25, seed: int = 0) -> np.ndarray:
    """boxes [K, 5] for the two toys: image indices round the batch, corners in image pixels (the map's extent over spatial_scale), a few of
    them crossing the border"""
    u = seeded_uniform("toy_rois", (boxes, 4), 0.0, 1.0, seed)
    ih, iw = height / spatial_scale, width / spatial_scale
    r = np.empty((boxes, 5), np.float32)
    r[:, 0] = np.arange(boxes) % batch
    r[:, 1] = (u[:, 0] * 0.8 - 0.1) * iw
    r[:, 2] = (u[:, 1] * 0.8 - 0.1) * ih
    r[:, 3] = r[:, 1] + (0.1 + 0.5 * u[:, 2]) * iw
    r[:, 4] = r[:, 2] + (0.1 + 0.5 * u[:, 3]) * ih
    return r


def build_toy_channel_shuffle(batch: int = 2, size: int = 16, c: int = 24, groups: int = 3, seed: int = 0) -> PnnxBuilder:
    """ShuffleNet's channel shuffle written out: two convs -> view(N, g, C / g, H, W) -> transpose(1, 2) -> view(N, C, H, W) -> 1x1 conv"""
    b = PnnxBuilder(seed)
    x = b.relu(b.conv(b.input((batch, 3, size, size)), 16, 3, 1, 1))
    x = b.relu(b.conv(x, c, 3, 1, 1))
    y = b.view(b.transpose(b.view(x, (batch, groups, c // groups, size, size)), 1, 2), (batch, c, size, size))
    b.output(b.conv(y, c, 1))
    return b


def build_toy_densenet(batch: int = 2, size: int = 33, growth: int = 8, ncls: int = 10, seed: int = 0) -> PnnxBuilder:
    """The average-pool idioms of the classification families at toy width: a conv3x3 stem (p = 0, 16 channels); two dense blocks (BN -> ReLU ->
    conv3x3 to `growth` channels, concatenated onto their input: DenseNet); a transition BN -> ReLU -> conv1x1 -> AvgPool2d(2, 2); an
    Inception-style block of three branches into one concat, the pool branch AvgPool2d(3, 1, 1, count_include_pad=False) -> conv1x1; a
    ResNet-D downsampling block on the odd map -- main branch conv3x3 s2 p1, shortcut AvgPool2d(2, 2, ceil_mode=True,
    count_include_pad=False) -> conv1x1, added; and the head AdaptiveAvgPool2d((1, 1)) -> flatten -> Linear.  The stem has no padding:
    at size 33 the map is 31 -> 15 (transition, the last row and column dropped) -> 8 (ResNet-D: ceil_mode keeps the odd map's last
    row and column, as a one-tap-wide window divided by its own extent)."""
    b = PnnxBuilder(seed)
    x = b.input((batch, 3, size, size))
    x = b.relu(b.conv(x, 2 * growth, 3, 1, 0))
    for _ in range(2):                                                   # dense blocks
        y = b.conv(b.relu(b.batchnorm(x)), growth, 3, 1, 1)
        x = b.cat([x, y])
    x = b.avgpool(b.conv(b.relu(b.batchnorm(x)), 2 * growth, 1, 1, 0), 2, 2)     # transition
    br1 = b.relu(b.conv(x, growth, 1, 1, 0))                             # Inception block
    br3 = b.relu(b.conv(b.relu(b.conv(x, growth, 1, 1, 0)), 2 * growth, 3, 1, 1))
    brp = b.conv(b.avgpool(x, 3, 1, 1, count_include_pad=False), growth, 1, 1, 0)
    x = b.relu(b.cat([br1, br3, brp]))
    main = b.conv(b.relu(b.conv(x, 4 * growth, 3, 2, 1)), 4 * growth, 3, 1, 1)   # ResNet-D block
    short = b.conv(b.avgpool(x, 2, 2, 0, ceil_mode=True, count_include_pad=False), 4 * growth, 1, 1, 0)
    x = b.relu(b.add(main, short))
    x = b.linear(b.flatten(b.adaptive_avgpool(x, (1, 1))), ncls)
    b.output(x)
    return b


def build_toy_pspnet(batch: int = 2, size: int = 52, ncls: int = 5, width: int = 16, bins=(1, 2, 3, 6), seed: int = 0) -> PnnxBuilder:
    """PSPNet's pyramid pooling module at toy width: two stride-2 conv3x3 -> ReLU to a size / 4 map (13 x 13 at size 52); per bin
    AdaptiveAvgPool2d((bin, bin)) -> conv1x1 -> ReLU -> F.interpolate(size=map, bilinear, align_corners=False); the four results
    concatenated with the map -> conv3x3 -> ReLU -> conv1x1 to ncls classes -> F.interpolate(size=input, bilinear).  Bins 2, 3 and 6 do not
    divide 13: the general adaptive windows."""
    b = PnnxBuilder(seed)
    x = b.input((batch, 3, size, size))
    x = b.relu(b.conv(x, width, 3, 2, 1))
    x = b.relu(b.conv(x, 2 * width, 3, 2, 1))
    h, w = b.shapes[x][2:]
    pyramid = [x]
    for bin_ in bins:
        y = b.relu(b.conv(b.adaptive_avgpool(x, (bin_, bin_)), width // 2, 1, 1, 0))
        pyramid.append(b.interpolate(y, mode="bilinear", align_corners=False, size=(h, w)))
    x = b.relu(b.conv(b.cat(pyramid), 2 * width, 3, 1, 1))
    x = b.conv(x, ncls, 1, 1, 0)
    x = b.interpolate(x, mode="bilinear", align_corners=False, size=(size, size))
    b.output(x)
    return b


def build_toy_segnet(batch: int = 2, size: int = 64, ncls: int = 21, seed: int = 0, head=None) -> PnnxBuilder:
    """A small FCN-style segmentation net: a stride-8 conv / BatchNorm2d / ReLU backbone with an FPN-style lateral in the middle
    (F.interpolate x2, align_corners=False, + add), ending in a dilated 3x3 (d = 2); a 1x1 classifier to ncls classes; then
    F.interpolate(size=(size, size), mode="bilinear", align_corners=False), the last line of torchvision's FCN / DeepLabV3 heads.
    head="softmax" / "log_softmax": nn.Softmax(dim=1) / nn.LogSoftmax(dim=1) over the classes of the resized map."""
    b = PnnxBuilder(seed)
    x = b.input((batch, 3, size, size))

    def cbr(x, c, k=3, s=1, p=1, d=1):
        return b.relu(b.batchnorm(b.conv(x, c, k, s, p, d)))

    c2 = cbr(cbr(x, 16, 3, 2), 32, 3, 2)       # stride 4
    c3 = cbr(c2, 64, 3, 2)                     # stride 8
    c4 = cbr(c3, 64, 3, 2)                     # stride 16
    top = b.interpolate(b.conv(c4, 64, 1, 1, 0), scale=2.0, mode="bilinear", align_corners=False)
    x = b.add(b.conv(c3, 64, 1, 1, 0), top)    # stride 8
    x = cbr(x, 64, 3, 1, 2, 2)                 # dilated
    x = b.conv(x, ncls, 1, 1, 0)
    x = b.interpolate(x, mode="bilinear", align_corners=False, size=(size, size))
    b.output(b._head(x, head))
    return b


def build_mobilenetv3_small(batch: int, size: int = 224, num_classes: int = 1000, seed: int = 0) -> PnnxBuilder:
    """torchvision MobileNetV3-Small topology with BatchNorm folded into the convolutions (nn.Conv2d bias=True), the
    model family of the reference's test_classify (test/test_classify/test_classify.cpp:12-15): 3x3 / 5x5 depthwise
    convs, squeeze-excite (global average pool -> 1x1 -> ReLU -> 1x1 -> Hardsigmoid -> broadcast mul), Hardswish,
    residual adds."""
    b = PnnxBuilder(seed)

    def act(x, kind):
        return b.hardswish(x) if kind == "HS" else b.relu(x)

    def make_div(v, d=8):
        return max(d, int(v + d / 2) // d * d)

    x = b.input((batch, 3, size, size))
    x = b.hardswish(b.conv(x, 16, 3, 2, 1))
    cin = 16
    # kernel, expanded channels, output channels, squeeze-excite, activation, stride
    cfg = [(3, 16, 16, True, "RE", 2), (3, 72, 24, False, "RE", 2), (3, 88, 24, False, "RE", 1), (5, 96, 40, True, "HS", 2),
           (5, 240, 40, True, "HS", 1), (5, 240, 40, True, "HS", 1), (5, 120, 48, True, "HS", 1), (5, 144, 48, True, "HS", 1),
           (5, 288, 96, True, "HS", 2), (5, 576, 96, True, "HS", 1), (5, 576, 96, True, "HS", 1)]
    for k, exp, cout, se, nl, s in cfg:
        y = x
        if exp != cin:
            y = act(b.conv(y, exp, 1), nl)
        y = act(b.conv(y, exp, k, s, k // 2, groups=exp), nl)          # depthwise
        if se:
            q = b.adaptive_avgpool(y, (1, 1))
            q = b.relu(b.conv(q, make_div(exp // 4), 1))
            q = b.hardsigmoid(b.conv(q, exp, 1))
            y = b.mul(y, q)                                            # broadcast over H, W
        y = b.conv(y, cout, 1)
        x = b.add(x, y) if (s == 1 and cin == cout) else y
        cin = cout
    x = b.hardswish(b.conv(x, 576, 1))
    x = b.adaptive_avgpool(x, (1, 1))
    x = b.flatten(x)
    x = b.hardswish(b.linear(x, 1024))
    x = b.linear(x, num_classes)
    b.output(x)
    return b


def conv_flops(builder: PnnxBuilder) -> int:
    """Direct-convolution FLOPs (2*MAC) of every nn.Conv2d + Detect 1x1 conv in the graph
    (sum N*OH*OW*KH*KW*(Cin/g)*Cout)."""
    total = 0
    for ln in builder.lines:
        t = ln.split()
        if t[0] == "nn.Conv2d":
            kv = dict(x.split("=", 1) for x in t[4 + int(t[2]) + int(t[3]):])
            out = t[4 + int(t[2])]
            n, co, oh, ow = builder.shapes[out]
            kh, kw = (int(v) for v in kv["kernel_size"].strip("()").split(","))
            total += 2 * n * oh * ow * kh * kw * (int(kv["in_channels"]) // int(kv["groups"])) * co
        elif t[0] == "models.yolo.Detect":
            nin = int(t[2])
            out = t[4 + nin]
            ne = builder.shapes[out][2]
            for x in t[4:4 + nin]:
                n, c, h, w = builder.shapes[x]
                total += 2 * n * h * w * c * 3 * ne
    return total
