"""Restatement and case table for the border-mapped convolution tests (test infrastructure, no product code).  Torch's layouts.
conv2d_border_ref: float64 F.pad(x, (pl, pl, pt, pt), mode) then conv2d without padding -- the specification of include/si_border.h; rnd=
(round_f16) rounds x, w and the stored result to half, sums stay float64, the bias fp32: the kernels' fp16 storage rule.
CASES: (N, C, H, W, O, k, stride, pad, dilation, mode) built from the header's tile enums: the smallest shapes at which a mechanism can fail."""
import os
import re

import numpy as np

from ct_reference import round_f16  # noqa: F401  (re-exported)
from xcorr_reference import nchw, nhwc, pair  # noqa: F401  (re-exported)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "si_border.h")
ENUMS = {k: int(v) for k, v in re.findall(r"\b(SI_BORDER_[A-Z0-9_]+) = (-?\d+)", open(HEADER).read())}
TH, TW, OCB, KC = ENUMS["SI_BORDER_TH"], ENUMS["SI_BORDER_TW"], ENUMS["SI_BORDER_OC"], ENUMS["SI_BORDER_KC"]
NP_MODE = {"replicate": "edge", "reflect": "reflect", "circular": "wrap"}   # numpy.pad's names

CASES = [
    # the pad limits
    (1, 3, 1, 1, 17, 3, 1, 2, 1, "replicate"),                # a 1x1 image, pad > n: every tap of every output is the one pixel
    (1, 5, 1, 7, 1, 3, 1, 2, 1, "replicate"),                 # a 1xW image, pad > H
    (1, 8, 4, 4, 33, 7, 1, 3, 1, "reflect"),                  # reflect at pad = n - 1; smaller than a tile: one patch touches both borders
    (1, 8, 3, 5, 65, (7, 11), 1, (3, 5), 1, "circular"),      # circular at pad = n on both axes
    # tile boundaries: output extents one below, at and one above TH x TW, and the channel block
    (1, 3, TH - 1, TW - 1, 1, 3, 1, 1, 1, "reflect"),
    (1, 8, TH, TW, OCB, 3, 1, 1, 1, "circular"),
    (3, KC + 8, TH + 1, TW + 1, OCB + 1, 3, 1, 1, 1, "replicate"),   # two channel chunks with a ragged second one, two tiles each way, N = 3
    (1, 5, 9, 9, OCB - 1, 3, 1, 1, 1, "reflect"),
    # geometries
    (1, 8, 9, TW + 4, 17, 7, 1, 3, 1, "reflect"),             # 7x7 p3
    (3, 8, 6, 9, 33, (1, 5), 1, (0, 2), 1, "replicate"),      # 1x5 with pads (0, 2)
    (1, 5, 9, 11, 17, 4, 2, 1, 1, "reflect"),                 # 4x4 s2 p1: the far pad is only partly used
    (1, KC + 8, 8, 8, 33, 3, 1, 2, 2, "circular"),            # 3x3 d2 p2
    (3, 1, 9, 10, 1, 3, (2, 1), 1, 1, "circular"),            # stride (2, 1), C = O = 1
    (1, 8, 9, 2 * TW + 3, 17, 3, (1, 2), 1, 1, "reflect"),    # stride 2 along W over three tiles: the phase-major column order
    (1, 8, 7, 9, 17, 5, 2, 4, 2, "reflect"),                  # 5x5 s2 d2 p4: the fp32 patch fits LDS with two live rows of the tile only
]
F16_CASES = [c for c in CASES if c[1] % 8 == 0]


def case_id(c):
    return "N%s_C%s_%sx%s_O%s_k%s_s%s_p%s_d%s_%s" % tuple(str(v).replace(" ", "").replace("(", "").replace(")", "").replace(",", "x") for v in c)


def operands(case, seed=0, dtype=np.float32, bias=True):
    """(x, w, b) in torch's layouts: x U(-1, 1) and w U(-a, a), a = sqrt(3 / fan_in), in `dtype`; b fp32 U(-0.5, 0.5) or None"""
    n, c, h, wd, oc, k = case[:6]
    kh, kw = pair(k)
    r = np.random.Generator(np.random.Philox(seed + 1000 * c + 10 * kh + kw))
    a = np.sqrt(3.0 / (c * kh * kw))
    x = r.uniform(-1, 1, (n, c, h, wd)).astype(np.float32).astype(dtype)
    w = r.uniform(-a, a, (oc, c, kh, kw)).astype(np.float32).astype(dtype)
    return x, w, (r.uniform(-0.5, 0.5, oc).astype(np.float32) if bias else None)


def conv2d_border_ref(x, w, b=None, stride=1, pad=1, dilation=1, mode="reflect", groups=1, rnd=None):
    """float64 [N, O, Ho, Wo]"""
    import torch
    q = rnd or (lambda a: np.asarray(a, np.float64))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64)))
    ph, pw = pair(pad)
    xp = torch.nn.functional.pad(t(q(x)), (pw, pw, ph, ph), mode=mode) if (ph or pw) else t(q(x))
    y = torch.nn.functional.conv2d(xp, t(q(w)), None if b is None else t(b), pair(stride), 0, pair(dilation), groups).numpy()
    return q(y) if rnd else y
