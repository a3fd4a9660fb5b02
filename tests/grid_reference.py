"""Restatements for the F.grid_sample / F.affine_grid tests (test infrastructure, no product code).

grid_sample_ref: the rule of include/si_grid.h in numpy on an NHWC x and a logical grid [n, ho, wo, 2].  The pixel coordinates are computed in
fp32 with the kernel's operations in the kernel's order (unnormalise, reflect, clip), so that floor(), nearbyint() and the range tests decide
as the kernel does; everything after that is float64.  coords64=True computes the coordinates in float64 with the same formulas: that form is
what tests/test_grid_cpu.py pins to torch.nn.functional.grid_sample in float64.

affine_grid_ref: F.affine_grid for theta [n, 2, 3]; fp32 with the kernel's base coordinates and fused multiply-adds (emulated through float64:
the product of two fp32 values is exact there), or float64 throughout with coords64=True.

stored_grid / in_place_grid / dense_grid: the three memory images of a logical grid and their element strides.  CASES: the GPU case table.
eval_graph: a float64 evaluator for the operator set of build_toy_stn and build_toy_flow_warp, with the rnd= hook of tests/ct_reference.py.
"""
import os

import numpy as np

import util
from ct_reference import _ints, _parse, conv2d_ref, round_f16  # noqa: F401  (round_f16 re-exported)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "si_grid.h")
ENTRIES = ["si_hip_grid_sample_f32", "si_hip_grid_sample_f16", "si_hip_grid_sample_kernel_name", "si_hip_affine_grid_f32", "si_hip_affine_grid_f16",
           "si_hip_affine_grid_kernel_name"]
SAMPLE, AFFINE = "F.grid_sample", "F.affine_grid"
MODES, PADDINGS = ("bilinear", "nearest"), ("zeros", "border", "reflection")


# ---- coordinates ------------------------------------------------------------------------------------------------------------
def source_coord(g, size, padding_mode, align_corners, dt=np.float32):
    """grid values -> pixel coordinates on an axis of `size`, padding applied, every operation in `dt`"""
    g = np.asarray(g).astype(dt)
    fs, one, half, zero = dt(size), dt(1), dt(0.5), dt(0)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        p = ((g + one) * half) * (fs - one) if align_corners else ((g + one) * fs - one) * half
        if padding_mode == "zeros":
            return p
        if padding_mode == "reflection":
            lo, span = (zero, fs - one) if align_corners else (dt(-0.5), fs)
            if span == 0:
                p = np.zeros_like(p)
            else:
                a = np.abs(p - lo)
                e = np.fmod(a, span)
                f = np.floor(a / span)
                even = (f - dt(2) * np.floor(f * half)) == 0
                p = np.where(even, e + lo, span - e + lo)
        else:
            assert padding_mode == "border", padding_mode
        p = np.fmin(np.fmax(p, zero), fs - one)       # (fmax / fmin drop a NaN operand: NaN becomes 0)
    assert p.dtype == dt
    return p


def pixel_coords(grid, h, w, padding_mode="zeros", align_corners=False, coords64=False):
    """(py, px) of a logical grid [..., 2] (x first), as float64 arrays holding fp32 values (or float64 ones with coords64)"""
    dt = np.float64 if coords64 else np.float32
    g = np.asarray(grid)
    px = source_coord(g[..., 0], w, padding_mode, align_corners, dt)
    py = source_coord(g[..., 1], h, padding_mode, align_corners, dt)
    return py.astype(np.float64), px.astype(np.float64)


def sample_at(x_nhwc, py, px, mode="bilinear"):
    """float64 [n, ho, wo, c]: x sampled at the pixel coordinates py, px [n, ho, wo] by the rule (NaN coordinate: NaN; a tap inside the image
    is multiplied also by a weight of 0, a tap outside adds exactly 0 and is not read; integers formed from a clamped float)"""
    X = np.asarray(x_nhwc, np.float64)
    n, h, w, c = X.shape
    img = np.arange(n)[:, None, None]
    nan = np.isnan(py) | np.isnan(px)
    py0, px0 = np.where(nan, 0.0, py), np.where(nan, 0.0, px)
    with np.errstate(invalid="ignore", over="ignore"):
        if mode == "nearest":
            yn = np.clip(np.rint(py0), -2, h).astype(np.int64)
            xn = np.clip(np.rint(px0), -2, w).astype(np.int64)
            ok = (yn >= 0) & (yn < h) & (xn >= 0) & (xn < w)
            out = np.where(ok[..., None], X[img, np.clip(yn, 0, h - 1), np.clip(xn, 0, w - 1)], 0.0)
        else:
            assert mode == "bilinear", mode
            y0f, x0f = np.floor(py0), np.floor(px0)
            wy1, wx1 = py0 - y0f, px0 - x0f
            wy0, wx0 = (y0f + 1.0) - py0, (x0f + 1.0) - px0
            y0, x0 = np.clip(y0f, -2, h).astype(np.int64), np.clip(x0f, -2, w).astype(np.int64)
            out = np.zeros(py.shape + (c,), np.float64)
            for wgt, yy, xx in ((wx0 * wy0, y0, x0), (wx1 * wy0, y0, x0 + 1), (wx0 * wy1, y0 + 1, x0), (wx1 * wy1, y0 + 1, x0 + 1)):
                ok = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
                v = X[img, np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)]
                out = out + np.where(ok[..., None], wgt[..., None] * v, 0.0)
        return np.where(nan[..., None], np.nan, out)


def grid_sample_ref(x_nhwc, grid, mode="bilinear", padding_mode="zeros", align_corners=False, coords64=False):
    """float64 NHWC result of F.grid_sample for an NHWC x and a logical grid [n, ho, wo, 2]"""
    n, h, w, _ = np.asarray(x_nhwc).shape
    py, px = pixel_coords(grid, h, w, padding_mode, align_corners, coords64)
    return sample_at(x_nhwc, py, px, mode)


def affine_base(size, align_corners, dt=np.float32):
    j = np.arange(size)
    if align_corners:
        return (dt(2) * j.astype(dt) / dt(size - 1) - dt(1)).astype(dt) if size > 1 else np.zeros(1, dt)
    return ((2 * j + 1 - size).astype(dt) / dt(size)).astype(dt)


def affine_grid_ref(theta, out_hw, align_corners=False, coords64=False):
    """the logical grid [n, H, W, 2] of F.affine_grid(theta [n, 2, 3], (n, C, H, W)): fp32 values (coords64: float64 arithmetic throughout)"""
    h, w = out_hw
    dt = np.float64 if coords64 else np.float32
    t = np.asarray(theta).astype(dt).astype(np.float64)                # [n, 2, 3]
    xb = affine_base(w, align_corners, dt).astype(np.float64)[None, None, :, None]
    yb = affine_base(h, align_corners, dt).astype(np.float64)[None, :, None, None]
    t0, t1, t2 = (t[:, None, None, :, k] for k in range(3))           # [n, 1, 1, 2]
    if coords64:
        return t0 * xb + t1 * yb + t2
    inner = (t1 * yb + t2).astype(np.float32).astype(np.float64)        # fmaf(t1, yb, t2): the product is exact in float64
    return (t0 * xb + inner).astype(np.float32)                         # fmaf(t0, xb, inner)


# ---- the memory images of a logical grid [n, ho, wo, 2] ---------------------------------------------------------------------
def dense_grid(grid):
    """torch's bytes"""
    n, ho, wo, _ = grid.shape
    return np.ascontiguousarray(grid), (ho * wo * 2, wo * 2, 2, 1)


def stored_grid(grid, ld=None):
    """the rank-4 tensor [n, ho, wo, 2] as this project stores it: [n][wo][2][ho], rows ld apart (what lies between the rows is NaN)"""
    n, ho, wo, _ = grid.shape
    ld = ld or ho
    img = np.full((n, wo, 2, ld), np.nan, grid.dtype)
    img[..., :ho] = grid.transpose(0, 2, 3, 1)
    return img, (2 * wo * ld, 1, 2 * ld, ld)


def in_place_grid(grid, ld=None, c_off=0):
    """the channels-first tensor [n, 2, ho, wo] in front of permute(0, 2, 3, 1), stored NHWC with pixel stride ld, the two coordinates at
    channel c_off; returns (array, strides, element offset)"""
    n, ho, wo, _ = grid.shape
    ld = ld or 2
    img = np.full((n, ho, wo, ld), np.nan, grid.dtype)
    img[..., c_off:c_off + 2] = grid
    return img, (ho * wo * ld, wo * ld, ld, 1), c_off


# ---- the case table -----------------------------------------------------------------------------------------------------------
def make_grid(seed, n, ho, wo, lo=-1.3, hi=1.3):
    """U(lo, hi); every 7th value (flat index) snapped to a multiple of 1/4, every 11th pushed out to +-2.5"""
    g = util.rng_uniform(seed, (n, ho, wo, 2), lo, hi).reshape(-1)
    g[::7] = np.round(g[::7] * 4) / 4
    g[::11] = np.sign(g[::11]) * np.float32(2.5)
    return g.reshape(n, ho, wo, 2)


def _table():
    """one row per (storage type, mode, padding, align_corners); c, n, h x w and ho x wo cycle through their values, so every value of every
    factor occurs at least three times and no two rows have the same shape"""
    cs, ns = (1, 2, 3, 4, 5, 8, 12, 20), (1, 3)
    hws, outs = ((1, 1), (1, 6), (7, 2), (9, 11)), ((2, 2), (5, 1), (13, 17))
    rows, i = [], 0
    for half in (False, True):
        for mode in MODES:
            for pad in PADDINGS:
                for ac in (False, True):
                    rows.append(dict(half=half, mode=mode, pad=pad, ac=ac, c=cs[(i * 3 + i // 8) % 8], n=ns[(i + i // 2) % 2], hw=hws[(i + i // 4) % 4],
                                     out=outs[(i + i // 3) % 3], seed=1000 + i))
                    i += 1
    return rows


CASES = _table()


def case_id(r):
    return "%s_%s_%s_%s_c%d_n%d_%dx%d_to_%dx%d" % ("f16" if r["half"] else "f32", r["mode"], r["pad"], "ac" if r["ac"] else "noac", r["c"], r["n"],
                                                   r["hw"][0], r["hw"][1], r["out"][0], r["out"][1])


def case_operands(r):
    """(x NHWC, logical grid) in the row's storage type"""
    dt = np.float16 if r["half"] else np.float32
    x = util.rng_uniform(r["seed"], (r["n"],) + r["hw"] + (r["c"],), -1.0, 1.0).astype(dt)
    return x, make_grid(r["seed"] + 1, r["n"], *r["out"]).astype(dt)


def expected_kernel(c, half, source="pair"):
    widths = (8, 4, 2) if half else (4,)
    vw = next((v for v in widths if c % v == 0), 1)
    return "grid_sample_kernel<%s, %d, %s>" % ("_Float16" if half else "float", vw, source)


# ---- graphs -----------------------------------------------------------------------------------------------------------------
def eval_graph(builder, inputs, rnd=None):
    """float64 evaluation of a PnnxBuilder graph with the operators of the two toys: Conv2d, ReLU, Tanh, MaxPool2d(2), AdaptiveAvgPool2d(1),
    torch.flatten, Linear, Tensor.view, Tensor.permute, the add expression, F.affine_grid and F.grid_sample (coordinates in float64).
    inputs: one array per graph input, rank 4 ones NHWC (as the engine takes them).  Values are held in FILE order (NCHW); the graph
    output comes back as the engine stores it (rank 4: NHWC).  rnd: applied to the inputs, every weight / bias and every operator's output
    except the graph output (None: exact)."""
    q = rnd or (lambda a: np.asarray(a, np.float64))
    to_file = lambda a: a.transpose(0, 3, 1, 2) if a.ndim == 4 else a
    to_nhwc = lambda a: a.transpose(0, 2, 3, 1) if a.ndim == 4 else a
    inputs = list(inputs) if isinstance(inputs, (list, tuple)) else [inputs]
    vals, result = {}, None
    lines = [_parse(ln) for ln in builder.lines]
    graph_outs = {ins[0] for typ, _, ins, _, _ in lines if typ == "pnnx.Output"}
    for typ, name, ins, outs, prm in lines:
        a = lambda k: builder.attrs["%s.%s" % (name, k)]
        if typ == "pnnx.Input":
            vals[outs[0]] = to_file(q(inputs.pop(0)))
            continue
        if typ == "pnnx.Output":
            result = to_nhwc(vals[ins[0]])
            continue
        x = vals[ins[0]]
        if typ == "nn.Conv2d":
            assert _ints(prm["dilation"]) == (1, 1) and int(prm["groups"]) == 1
            y = to_file(conv2d_ref(to_nhwc(x), q(a("weight")), q(a("bias")) if prm["bias"] == "True" else None, _ints(prm["stride"]), _ints(prm["padding"])))
        elif typ == "nn.ReLU":
            y = np.maximum(x, 0.0)
        elif typ == "nn.Tanh":
            y = np.tanh(x)
        elif typ == "nn.MaxPool2d":
            assert _ints(prm["kernel_size"]) == _ints(prm["stride"]) == (2, 2) and _ints(prm["padding"]) == (0, 0)
            n, c, h, w = x.shape
            y = x[:, :, :h // 2 * 2, :w // 2 * 2].reshape(n, c, h // 2, 2, w // 2, 2).max(axis=(3, 5))
        elif typ == "nn.AdaptiveAvgPool2d":
            assert _ints(prm["output_size"]) == (1, 1)
            y = x.mean(axis=(2, 3), keepdims=True)
        elif typ == "torch.flatten":
            y = x.reshape(x.shape[:int(prm["start_dim"])] + (-1,))
        elif typ == "nn.Linear":
            y = x @ q(a("weight")).T + (q(a("bias")) if prm["bias"] == "True" else 0.0)
        elif typ == "Tensor.view":
            y = x.reshape(_ints(prm["shape"]))
        elif typ == "Tensor.permute":
            y = x.transpose(_ints(prm["dims"]))
        elif typ == "pnnx.Expression":
            assert prm["expr"] == "add(@0,@1)", prm
            y = x + vals[ins[1]]
        elif typ == AFFINE:
            size = _ints(prm["size"])
            y = affine_grid_ref(x, size[2:], prm["align_corners"] == "True", coords64=True)
        elif typ == SAMPLE:
            y = to_file(grid_sample_ref(to_nhwc(x), vals[ins[1]], prm["mode"], prm["padding_mode"], prm["align_corners"] == "True", coords64=True))
        else:
            raise NotImplementedError(typ)
        assert tuple(y.shape) == tuple(builder.shapes[outs[0]]), (typ, name, y.shape, builder.shapes[outs[0]])
        vals[outs[0]] = y if outs[0] in graph_outs else q(y)
    return result
