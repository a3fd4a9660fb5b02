"""numpy restatements for the bilinear / by-size upsample tests (test infrastructure, no product code).

The rule (include/si_hip.h, "bilinear upsample"), per axis with `n_in` source and `n_out` destination samples, float32 throughout:
  align_corners:  s = n_out > 1 ? (n_in - 1) / (n_out - 1) : 0             src = s * d
  otherwise:      s = float32(1 / scale) when a scale factor is given,      src = max(0, fma(s, d + 0.5, -0.5))
                  else n_in / n_out
  i0 = min(int(src), n_in - 1), i1 = i0 + (i0 < n_in - 1), l1 = src - i0, l0 = 1 - l1
The fused multiply-add is restated as exact float64 arithmetic rounded once (a 24-bit step times a 13-bit d + 0.5 and the
subtraction of 0.5 are exact in float64).  upsample_bilinear_ref blends in float64 with those float32 weights;
tests/test_upsample_cpu.py pins it to torch.nn.functional.interpolate, the GPU tests compare against it and need no torch.

eval_graph: ct_reference.eval_graph's operator set plus dilated Conv2d, nn.Upsample / F.interpolate / F.upsample and the add
expression (the toy segmentation net and the bilinear toy U-Net).
"""
import numpy as np

from ct_reference import _ints, _parse, conv_transpose2d_ref, round_f16  # noqa: F401  (round_f16 re-exported)

F32 = np.float32
EPS = 2.0 ** -24          # half an fp32 ulp of 1: one rounding of a value of magnitude <= 1
BLEND_ULPS = 8.0          # five roundings of the fp32 blend, rounded up to a power of two


def out_size(n_in, scale):
    """torch's output size of a scale factor: floor(double(in) * scale)"""
    return int(np.floor(float(n_in) * float(scale)))


def axis_step(mode, n_in, n_out, align_corners=False, scale=None):
    if align_corners:
        assert mode == "bilinear"
        return F32(n_in - 1) / F32(n_out - 1) if n_out > 1 else F32(0.0)
    if scale is not None:
        return F32(1.0 / float(scale))
    return F32(n_in) / F32(n_out)


def axis_taps(n_in, n_out, step, align_corners):
    """(i0, i1, l0, l1) of every destination index; l0 / l1 are float32 values"""
    d = np.arange(n_out)
    if align_corners:
        src = (F32(step) * d.astype(F32)).astype(F32)
    else:
        src = np.maximum((np.float64(step) * (d + 0.5) - 0.5).astype(F32), F32(0.0))
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = (src - i0.astype(F32)).astype(F32)
    l0 = (F32(1.0) - l1).astype(F32)
    return i0, i1, l0, l1


def resolve(in_hw, out_hw=None, scale=None, recompute=False):
    """((oh, ow), (scale_h, scale_w) or (None, None)) of a call with torch's size= / scale_factor= / recompute_scale_factor="""
    assert (out_hw is None) != (scale is None)
    if scale is None:
        return (int(out_hw[0]), int(out_hw[1])), (None, None)
    sh, sw = (scale, scale) if np.isscalar(scale) else scale
    hw = (out_size(in_hw[0], sh), out_size(in_hw[1], sw))
    return hw, ((None, None) if recompute else (sh, sw))


def upsample_bilinear_ref(x_nhwc, out_hw=None, scale=None, align_corners=False, recompute=False, blend=np.float64):
    """NHWC result of F.interpolate(mode="bilinear"): float32 coordinates and weights, `blend` arithmetic (float64: the reference)"""
    x = np.asarray(x_nhwc)
    n, ih, iw, c = x.shape
    (oh, ow), (sh, sw) = resolve((ih, iw), out_hw, scale, recompute)
    y0, y1, lh0, lh1 = axis_taps(ih, oh, axis_step("bilinear", ih, oh, align_corners, sh), align_corners)
    x0, x1, lw0, lw1 = axis_taps(iw, ow, axis_step("bilinear", iw, ow, align_corners, sw), align_corners)
    v = x.astype(blend)
    lw0, lw1 = lw0.astype(blend)[None, None, :, None], lw1.astype(blend)[None, None, :, None]
    lh0, lh1 = lh0.astype(blend)[None, :, None, None], lh1.astype(blend)[None, :, None, None]
    top = lw0 * v[:, y0][:, :, x0] + lw1 * v[:, y0][:, :, x1]
    bot = lw0 * v[:, y1][:, :, x0] + lw1 * v[:, y1][:, :, x1]
    return lh0 * top + lh1 * bot


def upsample_nearest_ref(x_nhwc, out_hw=None, scale=None):
    """torch's nearest: index min(int(float32(d) * s), in - 1) with s = in / out (size=) or float32(1 / scale)"""
    x = np.asarray(x_nhwc)
    n, ih, iw, c = x.shape
    (oh, ow), (sh, sw) = resolve((ih, iw), out_hw, scale)
    ys = np.minimum((np.arange(oh).astype(F32) * axis_step("nearest", ih, oh, False, sh)).astype(F32).astype(np.int64), ih - 1)
    xs = np.minimum((np.arange(ow).astype(F32) * axis_step("nearest", iw, ow, False, sw)).astype(F32).astype(np.int64), iw - 1)
    return x[:, ys][:, :, xs]


def blend_bound(x):
    """the fp32 blend's error bound: 8 * 2^-24 * max|x|"""
    return BLEND_ULPS * EPS * float(np.abs(np.asarray(x, np.float64)).max())


def label_ref(logits, out_hw, align_corners=False):
    """(labels, near_tie): float64 argmax per pixel (lowest index first) and the pixels whose two largest reference values are closer
    than twice the blend bound -- there an fp32 blend may legitimately pick the other class"""
    ref = upsample_bilinear_ref(logits, out_hw=out_hw, align_corners=align_corners)
    labels = ref.argmax(axis=-1).astype(np.uint8)
    if ref.shape[-1] < 2:
        return labels, np.zeros(labels.shape, bool)
    top2 = np.partition(ref, ref.shape[-1] - 2, axis=-1)[..., -2:]
    near = (top2[..., 1] - top2[..., 0]) < 2.0 * blend_bound(logits)
    return labels, near


# the label-map cases of the GPU test: (seed, logits shape, output size, align_corners)
LABEL_CASES = [(0, (2, 64, 64, 21), (512, 512), False), (1, (2, 65, 65, 21), (513, 513), True),
               (2, (1, 60, 80, 19), (480, 640), False), (3, (2, 32, 32, 2), (256, 256), False)]
LABEL_TIE_CAP = 2e-4


def label_logits(seed, shape, half=False):
    x = np.random.default_rng(seed).standard_normal(shape).astype(np.float32)
    return x.astype(np.float16) if half else x


# ---- op-level case lists ---------------------------------------------------------------------------------------------------
BASE_SHAPES = [(2, 16, 16, 8), (1, 7, 300, 3), (1, 13, 9, 21), (2, 5, 11, 4), (1, 32, 24, 16), (3, 10, 10, 5)]
FORMS = ["x2", "x1.5", "x3.7", "size"]


def form_args(shape, form):
    """kwargs (out_hw= or scale=) of one of the four scale forms for an input shape"""
    if form == "size":
        return dict(out_hw=(2 * shape[1] + 1, 3 * shape[2] - 2))
    return dict(scale=float(form[1:]))


BASE_CASES = [(s, ac, f) for s in BASE_SHAPES for ac in (False, True) for f in FORMS]   # 48

# (shape, kwargs): downscaling (bilinear without antialias, as torch), ih = 1, identity, a wide decoder level, c = 1
EXTRA_CASES = [((1, 12, 9, 6), dict(out_hw=(7, 4))), ((2, 1, 9, 4), dict(out_hw=(1, 20))), ((2, 1, 9, 4), dict(out_hw=(5, 20))),
               ((1, 11, 6, 8), dict(out_hw=(11, 6))), ((2, 16, 16, 1024), dict(scale=2.0)), ((2, 9, 14, 1), dict(scale=2.0))]
DECODER_SHAPES = [(2, 16, 16, 1024), (2, 32, 32, 512), (2, 64, 64, 256), (2, 128, 128, 128)]


def case_id(shape, ac, kw):
    tag = "x%g" % kw["scale"] if "scale" in kw else "to%dx%d" % tuple(kw["out_hw"])
    return "%s_%s_%s" % ("x".join(str(v) for v in shape), tag, "ac" if ac else "noac")


def case_input(shape, seed=0, half=False):
    x = np.random.default_rng(seed).uniform(-1.0, 1.0, shape).astype(np.float32)
    return x.astype(np.float16) if half else x


# ---- graph evaluation ---------------------------------------------------------------------------------------------------------
def conv2d_ref(x_nhwc, w_oihw, bias, stride, padding, dilation=(1, 1)):
    """fp64 NHWC conv2d (groups 1), tap by tap"""
    x = np.asarray(x_nhwc, np.float64)
    w = np.asarray(w_oihw, np.float64)
    n, ih, iw, ic = x.shape
    oc, _, kh, kw = w.shape
    (sh, sw), (ph, pw), (dh, dw) = stride, padding, dilation
    oh, ow = (ih + 2 * ph - (kh - 1) * dh - 1) // sh + 1, (iw + 2 * pw - (kw - 1) * dw - 1) // sw + 1
    xp = np.zeros((n, ih + 2 * ph, iw + 2 * pw, ic), np.float64)
    xp[:, ph:ph + ih, pw:pw + iw, :] = x
    out = np.zeros((n, oh, ow, oc), np.float64)
    for ky in range(kh):
        for kx in range(kw):
            out += xp[:, ky * dh:ky * dh + (oh - 1) * sh + 1:sh, kx * dw:kx * dw + (ow - 1) * sw + 1:sw, :] @ w[:, :, ky, kx].T
    if bias is not None:
        out = out + np.asarray(bias, np.float64)
    return out


RESIZE_TYPES = ("nn.Upsample", "F.interpolate", "F.upsample")


def resize_args(prm):
    """(mode, kwargs for upsample_*_ref, align_corners) of an nn.Upsample / F.interpolate / F.upsample line's parameters"""
    none = lambda k: prm.get(k, "None") == "None"
    kw = {}
    if not none("size"):
        kw["out_hw"] = _ints(prm["size"])
    else:
        kw["scale"] = tuple(float(t) for t in prm["scale_factor"].strip("()").split(","))
    return prm["mode"], kw, prm.get("align_corners", "None") == "True", prm.get("recompute_scale_factor", "None") == "True"


def eval_graph(builder, x_nhwc, rnd=None):
    """fp64 evaluation of a PnnxBuilder graph (NHWC tensors).  rnd: applied to the input, every conv weight / bias and every layer's
    output except the graph output (None: exact) -- the fp16-storage emulation, as ct_reference.eval_graph."""
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
        elif typ == "nn.ReLU":
            y = np.maximum(x, 0.0)
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
