"""The rectangular conv / pool matrix (test infrastructure, no product code): kernels, strides, pads and dilations whose two axes DIFFER, for
every convolution family and the max pool, with torch's float64 CPU operators as the reference.

Why torch: it is the plain high-precision statement of the operation and independent of the oracle, whose own rectangular handling
tests/test_rect_cpu.py holds to it as well.  Every case has a TWIN -- image, kernel, stride, pad and dilation axes swapped -- so that an h / w
mix-up cannot cancel inside one case.  tests/test_rect_cpu.py checks the table and the oracle on the CPU; tests/test_gpu_rect.py runs the HIP kernels.
"""
import collections

import numpy as np

import util

# family: which kernel family the case is written for; kern: a substring of the kernel instantiation si_hip_conv2d_kernel_name must report
Case = collections.namedtuple("Case", "family shape oc k s p d g kern note")

FAMILIES = ("igemm_fast", "igemm_padk", "igemm_generic", "depthwise", "grouped", "stem")
FAST, GENERIC, SMALLC = "conv_igemm_f32_fast_kernel<", "conv_igemm_f32_kernel<", "conv_smallc_rows_kernel<"
DW_VEC, DW_SCALAR = "conv_depthwise_kernel<true", "conv_depthwise_kernel<false"


def dw_cols(kw, sw):
    return "conv_depthwise_cols_kernel<4, %d, %d>" % (kw, sw)


# (family, shape NHWC, oc, k, s, p, d, groups, kernel, the TWIN's kernel when it differs, note)
_BASE = [
    # implicit GEMM, fast path (ic / groups % 32 == 0)
    ("igemm_fast", (2, 13, 17, 32), 48, (1, 3), (1, 1), (0, 1), (1, 1), 1, FAST, None, "1x3"),
    ("igemm_fast", (2, 13, 17, 32), 48, (3, 1), (1, 1), (1, 0), (1, 1), 1, FAST, None, "3x1"),
    ("igemm_fast", (1, 19, 23, 64), 64, (1, 7), (1, 1), (0, 3), (1, 1), 1, FAST, None, "1x7"),
    ("igemm_fast", (1, 19, 23, 64), 64, (7, 1), (1, 1), (3, 0), (1, 1), 1, FAST, None, "7x1"),
    ("igemm_fast", (2, 20, 14, 32), 40, (3, 3), (2, 1), (1, 1), (1, 1), 1, FAST, None, "3x3 stride (2,1): Winograd near-miss"),
    ("igemm_fast", (2, 14, 20, 32), 40, (3, 3), (1, 2), (1, 1), (1, 1), 1, FAST, None, "3x3 stride (1,2): Winograd near-miss"),
    ("igemm_fast", (1, 15, 15, 32), 32, (3, 3), (1, 1), (2, 1), (2, 1), 1, FAST, None, "straight-line 3x3 mask, dh != dw"),
    ("igemm_fast", (1, 15, 15, 32), 32, (3, 3), (1, 1), (1, 3), (1, 3), 1, FAST, None, "straight-line 3x3 mask, dh != dw"),
    ("igemm_fast", (1, 9, 12, 32), 32, (8, 8), (1, 1), (4, 4), (1, 1), 1, FAST, None, "64 taps: the mask's last bit (the one deliberate square)"),
    ("igemm_fast", (1, 6, 40, 32), 32, (1, 9), (1, 1), (0, 4), (1, 2), 1, FAST, None, "1x9 dilated along w"),
    ("igemm_fast", (1, 8, 20, 32), 32, (5, 13), (1, 1), (2, 6), (1, 1), 1, GENERIC, None, "65 taps: leaves the fast kernel"),
    ("igemm_fast", (2, 10, 14, 32), 32, (3, 3), (1, 1), (1, 0), (1, 1), 1, FAST, None, "3x3 pad (1,0): Winograd near-miss"),
    # zero-padded-K 1x1 off the pointwise path
    ("igemm_padk", (2, 12, 16, 24), 36, (1, 1), (2, 1), (0, 0), (1, 1), 1, FAST, None, "stride (2,1)"),
    ("igemm_padk", (2, 12, 16, 40), 24, (1, 1), (2, 2), (0, 0), (1, 1), 1, FAST, None, "stride (2,2), rectangular image"),
    ("igemm_padk", (2, 12, 16, 24), 24, (1, 1), (1, 1), (1, 0), (1, 1), 1, FAST, None, "pad (1,0)"),
    ("igemm_padk", (1, 9, 11, 72), 40, (1, 1), (1, 2), (0, 1), (1, 1), 1, FAST, None, "72 channels: three K blocks, the last one ragged"),
    # generic kernel (ragged channels)
    ("igemm_generic", (2, 11, 9, 5), 7, (2, 3), (1, 2), (0, 2), (1, 1), 1, GENERIC, None, "ragged everything"),
    # depthwise
    ("depthwise", (2, 12, 12, 16), 16, (3, 5), (2, 1), (1, 2), (1, 1), 16, dw_cols(5, 1), dw_cols(3, 2), "column kernel, kh != KW"),
    ("depthwise", (2, 12, 12, 16), 16, (5, 3), (1, 2), (2, 1), (1, 1), 16, dw_cols(3, 2), dw_cols(5, 1), "column kernel, kh != KW"),
    ("depthwise", (2, 12, 12, 16), 16, (1, 3), (1, 1), (0, 1), (1, 1), 16, dw_cols(3, 1), DW_VEC, "column kernel, kh = 1"),
    ("depthwise", (2, 12, 12, 12), 12, (3, 3), (1, 1), (2, 1), (2, 1), 12, DW_VEC, None, "generic vector kernel, dh != dw"),
    ("depthwise", (2, 11, 13, 6), 6, (3, 5), (2, 1), (1, 2), (1, 1), 6, DW_SCALAR, None, "c % 4 != 0: scalar kernel"),
    ("depthwise", (2, 12, 14, 8), 8, (3, 7), (1, 2), (1, 3), (1, 1), 8, DW_VEC, dw_cols(3, 1), "kw = 7: generic kernel; the twin is a 7-row column kernel"),
    # grouped, merged into dense 32-channel super-groups
    ("grouped", (2, 12, 12, 32), 64, (3, 1), (1, 1), (1, 0), (1, 1), 4, FAST, None, "8 per group: merged"),
    ("grouped", (2, 12, 12, 32), 32, (1, 3), (1, 2), (0, 1), (1, 1), 8, FAST, None, "4 per group: merged"),
    # RGB / small-channel stems
    ("stem", (2, 24, 30, 3), 32, (6, 7), (2, 2), (2, 3), (1, 1), 1, SMALLC, None, "6x7: KH = 6 templates with kw = 7"),
    ("stem", (2, 24, 30, 3), 32, (7, 6), (2, 2), (3, 2), (1, 1), 1, SMALLC, None, "7x6: KH = 7 templates with kw = 6"),
    ("stem", (2, 24, 30, 3), 16, (5, 3), (2, 1), (2, 1), (1, 1), 1, SMALLC, GENERIC, "kw * ic = 9; the twin's 15 is no stem row"),
    ("stem", (2, 24, 30, 3), 16, (1, 3), (1, 2), (0, 1), (1, 1), 1, SMALLC, GENERIC, "one kernel row"),
    ("stem", (2, 24, 30, 2), 16, (2, 5), (2, 2), (0, 2), (1, 1), 1, SMALLC, GENERIC, "two channels, kw * ic = 10"),
    ("stem", (2, 24, 30, 3), 16, (7, 3), (2, 2), (3, 1), (1, 1), 1, GENERIC, SMALLC, "kw * ic = 9 but sh + kh = 9 staged rows: no stem instantiation, the implicit GEMM"),
    ("stem", (2, 24, 30, 3), 16, (7, 3), (1, 1), (3, 1), (1, 1), 1, GENERIC, SMALLC, "7x3 at stride 1: sh + kh = 8, the implicit GEMM"),
    ("stem", (2, 24, 30, 3), 16, (6, 3), (2, 1), (2, 1), (1, 1), 1, GENERIC, SMALLC, "6x3 at sh = 2: sh + kh = 8, the implicit GEMM"),
    ("stem", (2, 24, 30, 3), 16, (6, 3), (1, 2), (2, 1), (1, 1), 1, SMALLC, None, "6x3 at sh = 1: sh + kh = 7, the tallest the 9-element stem row serves"),
    ("stem", (2, 24, 30, 3), 32, (6, 6), (2, 1), (2, 2), (1, 1), 1, SMALLC, None, "square, sh != sw: not the rolling-window stem"),
    ("stem", (2, 24, 30, 3), 32, (3, 3), (1, 2), (1, 1), (1, 1), 1, SMALLC, None, "square, sh != sw: not the rolling-window stem"),
]


def swap(pair):
    return (pair[1], pair[0])


def twin(c):
    """the case with the image, kernel, stride, pad and dilation axes swapped (channels, groups and family stay)"""
    n, h, w, ch = c.shape
    return c._replace(shape=(n, w, h, ch), k=swap(c.k), s=swap(c.s), p=swap(c.p), d=swap(c.d))


def key(c):
    return (c.shape, c.oc, c.k, c.s, c.p, c.d, c.g)


def _table():
    cases, seen = [], {}
    for fam, shape, oc, k, s, p, d, g, kern, twin_kern, note in _BASE:
        c = Case(fam, shape, oc, k, s, p, d, g, kern, note)
        if key(c) not in seen:
            seen[key(c)] = len(cases)
            cases.append(c)
        t = twin(c)._replace(kern=twin_kern or kern, note="twin of: " + note)
        if key(t) not in seen:
            seen[key(t)] = len(cases)
            cases.append(t)
    return cases


RECT_CASES = _table()


def case_id(c):
    n, h, w, ch = c.shape
    return "%s-n%d_%dx%dx%d-oc%d-k%dx%d-s%dx%d-p%dx%d-d%dx%d-g%d" % ((c.family, n, h, w, ch, c.oc) + c.k + c.s + c.p + c.d + (c.g,))


def cases_of(*families):
    return [c for c in RECT_CASES if c.family in families]


def ids_of(cases):
    return [case_id(c) for c in cases]


def seed_of(c):
    """arithmetic in the case's own numbers (no hash(): the same seed in every process)"""
    v = 0
    for f in c.shape + (c.oc,) + c.k + c.s + c.p + c.d + (c.g,):
        v = (v * 131 + int(f)) % 1000003
    return 10 * v


def operands(c, w_scale=0.5):
    """x in [-1, 1), weights in [-w_scale, w_scale), bias in [-0.5, 0.5), all float32"""
    s = seed_of(c)
    x = util.rng_uniform(s, c.shape, -1, 1)
    w = util.rng_uniform(s + 1, (c.oc, c.shape[3] // c.g) + c.k, -w_scale, w_scale)
    b = util.rng_uniform(s + 2, (c.oc,), -0.5, 0.5)
    return x, w, b


def merged_groups_dense(w_oihw, groups):
    """(dense weights, groups / G) of a grouped conv with 4, 8 or 16 input channels per group, as the merged-group path runs it: G = 32 / (ic /
    groups) neighbouring groups as ONE group of 32 input channels whose weight image is block-diagonal (zeros where an output channel does not
    see an input channel of its super-group).  fma(x, 0, acc) = acc, so the oracle's fma chain on THIS problem is the device's chain."""
    w = np.asarray(w_oihw, np.float32)
    oc, icg = w.shape[0], w.shape[1]
    G, ocg = 32 // icg, oc // groups
    assert icg in (4, 8, 16) and groups % G == 0
    dense = np.zeros((oc, 32) + w.shape[2:], np.float32)
    for o in range(oc):
        gi = (o // ocg) % G
        dense[o, gi * icg:(gi + 1) * icg] = w[o]
    return dense, groups // G


def out_hw(ih, iw, k, s, p, d):
    return ((ih + 2 * p[0] - ((k[0] - 1) * d[0] + 1)) // s[0] + 1, (iw + 2 * p[1] - ((k[1] - 1) * d[1] + 1)) // s[1] + 1)


def conv2d_f64(x_nhwc, w_oihw, b=None, stride=(1, 1), padding=(0, 0), dilation=(1, 1), groups=1):
    """torch.nn.functional.conv2d on the CPU in float64; NHWC in, NHWC float64 out"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(np.asarray(x_nhwc, np.float64).transpose(0, 3, 1, 2)))
    w = torch.from_numpy(np.ascontiguousarray(np.asarray(w_oihw, np.float64)))
    bias = None if b is None else torch.from_numpy(np.ascontiguousarray(np.asarray(b, np.float64)))
    y = torch.nn.functional.conv2d(t, w, bias, stride=tuple(stride), padding=tuple(padding), dilation=tuple(dilation), groups=int(groups))
    return np.ascontiguousarray(y.numpy().transpose(0, 2, 3, 1))


def maxpool2d_f64(x_nhwc, k, s, p, d=(1, 1)):
    """torch.nn.functional.max_pool2d on the CPU in float64; NHWC in and out.  The padding is written out as -inf columns and rows first:
    torch refuses an implicit pad above half the kernel, its own implicit pad is -inf, and a max is exact in any precision."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(np.asarray(x_nhwc, np.float64).transpose(0, 3, 1, 2)))
    t = torch.nn.functional.pad(t, (p[1], p[1], p[0], p[0]), value=float("-inf"))
    y = torch.nn.functional.max_pool2d(t, tuple(k), stride=tuple(s), padding=0, dilation=tuple(d))
    return np.ascontiguousarray(y.numpy().transpose(0, 2, 3, 1))


ACTS64 = {"none": lambda v: v, "relu": lambda v: np.maximum(v, 0.0), "silu": lambda v: v / (1.0 + np.exp(-v))}


def epilogue_f64(y, act1="none", residual=None, act2="none"):
    """act2(act1(y) + residual) in float64: the fused epilogue's definition"""
    v = ACTS64[act1](np.asarray(y, np.float64))
    if residual is not None:
        v = v + np.asarray(residual, np.float64)
    return ACTS64[act2](v)


# f32_split: ic 64 and ic 96 (both K-tile widths), the two 5-tap strips, 3x3 at the two one-axis strides, and a kernel of 4x8 = 32 taps (the limit).
# (shape NHWC, oc, k, s, p)
SPLIT3_CASES = [
    ((2, 11, 14, 64), 48, (1, 5), (1, 1), (0, 2)),
    ((2, 11, 14, 96), 48, (5, 1), (1, 1), (2, 0)),
    ((2, 13, 10, 64), 64, (3, 3), (2, 1), (1, 1)),
    ((2, 13, 10, 96), 40, (3, 3), (1, 2), (1, 1)),
    ((1, 9, 12, 64), 32, (4, 8), (1, 1), (2, 4)),
    ((1, 9, 12, 96), 32, (8, 4), (1, 1), (4, 2)),
]
SPLIT3_CASES += [((n, w, h, c), oc, swap(k), swap(s), swap(p)) for (n, h, w, c), oc, k, s, p in SPLIT3_CASES[:4]]


def split3_id(c):
    (n, h, w, ch), oc, k, s, p = c
    return "n%d_%dx%dx%d-oc%d-k%dx%d-s%dx%d-p%dx%d" % ((n, h, w, ch, oc) + k + s + p)


# max pool: (k, s, p, d)
POOL_PARAMS = [
    ((3, 2), (2, 1), (1, 0), (1, 1)),
    ((2, 3), (1, 2), (0, 1), (1, 1)),
    ((1, 5), (1, 1), (0, 2), (1, 1)),
    ((5, 1), (1, 1), (2, 0), (1, 1)),
    ((3, 3), (1, 1), (2, 1), (2, 1)),
    ((3, 3), (1, 1), (1, 2), (1, 2)),
]
POOL_SHAPE = (2, 11, 14)   # n, h, w; c = 8 (vector path) and c = 6 (scalar path)


def pool_id(q):
    k, s, p, d = q
    return "k%dx%d-s%dx%d-p%dx%d-d%dx%d" % (k + s + p + d)


def pool_input(c, seed=0):
    """all-negative: a padded tap that took part in the max (as 0, or as anything finite above -3) would win it"""
    return util.rng_uniform(9100 + 10 * c + seed, POOL_SHAPE + (c,), -3, -1)


# ---- the engine-level graph: every layer rectangular ------------------------------------------------------------------------------------------
def build_rect_graph(mg, batch=2, h=48, w=60, seed=3):
    """7x6 stride-2 RGB stem, 1x7 then 7x1 over 64 channels, 3x3 pad (1,0), 3x3 stride (1,2), depthwise 3x5 stride (2,1), 1x1 stride (2,1) over
    24 channels, max pool (3,2) / (2,1), a 1x1 head.  No layer is Winograd-eligible."""
    b = mg.PnnxBuilder(seed=seed)
    x = b.input((batch, 3, h, w))
    x = b.relu(b.conv(x, 64, (7, 6), (2, 2), (3, 2)))
    x = b.relu(b.conv(x, 64, (1, 7), 1, (0, 3)))
    x = b.relu(b.conv(x, 64, (7, 1), 1, (3, 0)))
    x = b.relu(b.conv(x, 32, (3, 3), 1, (1, 0)))
    x = b.relu(b.conv(x, 24, (3, 3), (1, 2), (1, 1)))
    x = b.relu(b.conv(x, 24, (3, 5), (2, 1), (1, 2), groups=24))
    x = b.relu(b.conv(x, 40, (1, 1), (2, 1), (0, 0)))
    x = b.maxpool(x, (3, 2), (2, 1), (1, 0))
    x = b.conv(x, 10, 1, 1, 0)
    b.output(x)
    return b


def _parse(line):
    toks = line.split()
    typ, name, nin, nout = toks[0], toks[1], int(toks[2]), int(toks[3])
    ins, outs = toks[4:4 + nin], toks[4 + nin:4 + nin + nout]
    params = dict(t.split("=", 1) for t in toks[4 + nin + nout:] if t[0] not in "@#")
    return typ, name, ins, outs, params


def _ints(v):
    return tuple(int(t) for t in v.strip("()").split(",") if t)


def eval_rect_graph(builder, x_nhwc):
    """the builder's own lines composed from conv2d_f64 / maxpool2d_f64 with float64 activations"""
    vals, result = {}, None
    for typ, name, ins, outs, prm in (_parse(ln) for ln in builder.lines):
        if typ == "pnnx.Input":
            vals[outs[0]] = np.asarray(x_nhwc, np.float64)
        elif typ == "pnnx.Output":
            result = vals[ins[0]]
        elif typ == "nn.Conv2d":
            b = builder.attrs[name + ".bias"] if prm["bias"] == "True" else None
            vals[outs[0]] = conv2d_f64(vals[ins[0]], builder.attrs[name + ".weight"], b, _ints(prm["stride"]), _ints(prm["padding"]),
                                       _ints(prm["dilation"]), int(prm["groups"]))
        elif typ == "nn.ReLU":
            vals[outs[0]] = np.maximum(vals[ins[0]], 0.0)
        elif typ == "nn.MaxPool2d":
            vals[outs[0]] = maxpool2d_f64(vals[ins[0]], _ints(prm["kernel_size"]), _ints(prm["stride"]), _ints(prm["padding"]), _ints(prm["dilation"]))
        else:
            raise NotImplementedError(typ)
    return result
