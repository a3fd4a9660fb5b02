"""numpy restatements of the image-size instance masks (include/si_imgmask.h) and the inputs of their tests (test infrastructure, no product code).

masks_f32   the rule in float32, operation by operation: detect_reference.mask_dots, up_reference.axis_taps inside the window, the blend as three
            products-and-sums, crop and threshold.  The kernel reproduces its bytes.
rule_f64    the same with dots and blend in float64 (the float32 taps and weights are part of the rule; exact=True takes the coordinates in
            float64 too, which is what torch's float64 interpolate computes and what tests/test_image_masks_cpu.py pins it to).

The bound of the float64 comparison.  With u = 2^-24, the fp32 dot in index order rounds nm products and nm - 1 sums that matter (0 + x is
exact), so term i of the sum carries at most nm roundings: |fl(dot) - dot| <= ((1 + u)^nm - 1) * sum |c_i p_i|.  On its way to the output a tap
value then passes one product and one sum of the horizontal blend and one product and one sum of the vertical one: four more factors (1 + u).
The weights are the same non-negative fp32 numbers on both sides and a masked tap is +0 on both sides, so
    |v32 - v64| <= ((1 + u)^(nm + 4) - 1) * B <= (nm + 5) * u * B,   B = sum |c_i p_i| blended with the same weights
((1 + u)^(nm + 4) - 1 < (nm + 4) u + ((nm + 4) u)^2 and (68 u)^2 < u).  A pixel whose |v64| exceeds that bound has the same sign in fp32.
"""
import functools
from typing import NamedTuple

import numpy as np

import detect_reference as dr
from up_reference import axis_step, axis_taps

F = np.float32
U = 2.0 ** -24
MAX_DET = 16                       # the fourteen fixed boxes of detect_reference.mask_boxes and two random ones
PLANES = ((5, 7), (20, 24))
NMS = (1, 32, 33, 64)
CROPS = ("after", "first")
COUNTS = ((0, 3), (MAX_DET, MAX_DET + 5))      # 0, below, at and above max_det: two images per call
EXCLUDED_CAP = 0.01


def geometries(mh, mw):
    """name -> ((win_x0, win_y0, win_w, win_h, out_w, out_h), (OH, OW), arm or None where the arm depends on nm)"""
    big = mw >= 16
    return {
        "identity": ((0, 0, mw, mh, mw, mh), (mh, mw), None),
        "x4": ((0, 0, mw, mh, 4 * mw, 4 * mh), (4 * mh, 4 * mw), "shared"),
        # a non-integer up-scale of a window off the origin
        "offset": ((3, 2, 13, 9, 50, 37) if big else (2, 1, 4, 3, 15, 11), (37, 50) if big else (11, 15), "shared"),
        # one pixel wider and one taller than the 128 x 8 tile: partial tiles, and a packed group of four with one live pixel
        "tile+1": ((0, 0, mw, mh, 129, 9), (9, 132), None),
        "down": ((0, 0, mw, mh, (mw + 1) // 3, (mh + 1) // 3), ((mh + 1) // 3, (mw + 1) // 3), "direct"),
        # the image's output is smaller than the planes: a zero border, rows off a 4-byte boundary for the larger plane
        "border": ((0, 0, mw, mh, 3 * mw - 2, 2 * mh + 1), (2 * mh + 4, 3 * mw + 3), None),
    }


def geom_ok(g, mh, mw, oh, ow):
    x0, y0, ww, wh, out_w, out_h = (int(v) for v in g)
    return x0 >= 0 and y0 >= 0 and ww > 0 and wh > 0 and x0 + ww <= mw and y0 + wh <= mh and 0 < out_w <= ow and 0 < out_h <= oh


def taps(n_in, n_out, exact=False):
    if not exact:
        return axis_taps(n_in, n_out, axis_step("bilinear", n_in, n_out), False)
    src = np.maximum((n_in / n_out) * (np.arange(n_out) + 0.5) - 0.5, 0.0)
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    return i0, i0 + (i0 < n_in - 1), 1.0 - (src - i0), src - i0


def blend(v, ty, tx, dt):
    """top = l0w v00 + l1w v01, bot = l0w v10 + l1w v11, l0h top + l1h bot: every product and sum an operation of type dt"""
    (y0, y1, lh0, lh1), (x0, x1, lw0, lw1) = ty, tx
    v, lw0, lw1, lh0, lh1 = v.astype(dt), lw0.astype(dt), lw1.astype(dt), lh0.astype(dt)[:, None], lh1.astype(dt)[:, None]
    top = lw0 * v[y0][:, x0] + lw1 * v[y0][:, x1]
    bot = lw0 * v[y1][:, x0] + lw1 * v[y1][:, x1]
    return lh0 * top + lh1 * bot


def _planes(protos, extras, boxes, counts, geom, out_hw, crop, coef_off, nm, per_plane):
    """the frame of both rules: per image [k][OH][OW] planes; per_plane(window prototypes, coefficients, box, taps, (out_h, out_w)) fills one"""
    n, mh, mw, pnm = protos.shape
    nm = pnm if nm is None else nm
    oh, ow = out_hw
    out = []
    for b in range(n):
        k = min(int(counts[b]), extras.shape[1])
        planes = [np.zeros((k, oh, ow), t) for t in per_plane.types]
        if geom_ok(geom[b], mh, mw, oh, ow):
            x0, y0, ww, wh, out_w, out_h = (int(v) for v in geom[b])
            win = protos[b, y0:y0 + wh, x0:x0 + ww, :nm]
            for d in range(k):
                for p, v in zip(planes, per_plane(win, extras[b, d, coef_off:coef_off + nm], boxes[b, d, :4], crop, (out_h, out_w))):
                    p[d, :out_h, :out_w] = v
        out.append(planes[0] if len(planes) == 1 else planes)
    return out


def _f32_plane(win, coef, box, crop, out_hw):
    wh, ww = win.shape[:2]
    with np.errstate(all="ignore"):
        logit = dr.mask_dots(np.ascontiguousarray(win, F), np.asarray(coef, F))
        if crop == "first":
            logit = np.where(dr.mask_crop(box, wh, ww, F(1), F(1)), logit, F(0))
        v = blend(logit, taps(wh, out_hw[0]), taps(ww, out_hw[1]), F)
        assert v.dtype == F
        bit = v > 0
        if crop == "after":
            bit &= dr.mask_crop(box, out_hw[0], out_hw[1], F(1), F(1))
    return (bit.astype(np.uint8),)


_f32_plane.types = (np.uint8,)


def masks_f32(protos, extras, boxes, counts, geom, out_hw, crop, coef_off=0, nm=None):
    """per image [min(count, max_det)][OH][OW] uint8: the bytes of the kernel"""
    return _planes(np.asarray(protos, F), extras, boxes, counts, geom, out_hw, crop, coef_off, nm, _f32_plane)


def rule_f64(protos, extras, boxes, counts, geom, out_hw, crop, coef_off=0, nm=None, exact=False):
    """per image [bytes, v64, bound]: the float64 logit of every output pixel, the bound of the module docstring, and the rule's byte"""
    def plane(win, coef, box, crop, out_hw):
        wh, ww = win.shape[:2]
        with np.errstate(all="ignore"):
            c, p = np.asarray(coef, np.float64), np.asarray(win, np.float64)
            logit, mag = p @ c, np.abs(p) @ np.abs(c)
            if crop == "first":
                inside = dr.mask_crop(box, wh, ww, F(1), F(1))
                logit, mag = np.where(inside, logit, 0.0), np.where(inside, mag, 0.0)
            ty, tx = taps(wh, out_hw[0], exact), taps(ww, out_hw[1], exact)
            v = blend(logit, ty, tx, np.float64)
            bit = v > 0
            if crop == "after":
                bit &= dr.mask_crop(box, out_hw[0], out_hw[1], F(1), F(1))
        return bit.astype(np.uint8), v, (len(c) + 5) * U * blend(mag, ty, tx, np.float64)

    plane.types = (np.uint8, np.float64, np.float64)
    return _planes(np.asarray(protos, F), extras, boxes, counts, geom, out_hw, crop, coef_off, nm, plane)


def decided(ref):
    """(per image the pixels of rule_f64's result that the bound decides, the share of the others); a pixel with a bound of 0 has only zero
    products behind it and is exactly 0 in fp32 too"""
    masks = [(np.abs(v) > bound) | (bound == 0) for _, v, bound in ref]
    total = sum(m.size for m in masks)
    return masks, (sum(int((~m).sum()) for m in masks) / total if total else 0.0)


class Case(NamedTuple):
    protos: np.ndarray      # [2][mh][mw][nm]
    extras: np.ndarray      # [2][MAX_DET][nm + coef_off]
    boxes: np.ndarray       # [2][MAX_DET][4], in the frame the crop asks for
    counts: np.ndarray
    geom: np.ndarray        # [2][6]
    out_hw: tuple
    crop: str
    coef_off: int
    arm: object


@functools.lru_cache(maxsize=None)
def case(plane, nm, crop, gname, counts, seed=0):
    """the boxes are detect_reference.mask_boxes around the frame the crop tests in: the output (after) or the window (first)"""
    mh, mw = plane
    g, out_hw, arm = geometries(mh, mw)[gname]
    r = np.random.Generator(np.random.Philox(9100 + seed))
    coef_off = nm % 3
    protos = r.uniform(-1, 1, (2, mh, mw, nm)).astype(F)
    extras = r.uniform(-1, 1, (2, MAX_DET, nm + coef_off)).astype(F)
    fh, fw = (g[5], g[4]) if crop == "after" else (g[3], g[2])
    boxes = np.stack([dr.mask_boxes(fh, fw, 1.0, 1.0, r, MAX_DET) for _ in range(2)])
    c = Case(protos, extras, boxes, np.asarray(counts, np.int32), np.asarray([g, g], np.int32), out_hw, crop, coef_off, arm)
    for a in (c.protos, c.extras, c.boxes, c.counts, c.geom):
        a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def expected(plane, nm, crop, gname, counts, seed=0):
    c = case(plane, nm, crop, gname, counts, seed)
    return masks_f32(c.protos, c.extras, c.boxes, c.counts, c.geom, c.out_hw, c.crop, c.coef_off, nm)


@functools.lru_cache(maxsize=None)
def expected_f64(plane, nm, crop, gname, counts, seed=0):
    c = case(plane, nm, crop, gname, counts, seed)
    return rule_f64(c.protos, c.extras, c.boxes, c.counts, c.geom, c.out_hw, c.crop, c.coef_off, nm)
