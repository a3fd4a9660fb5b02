"""torch.cdist (include/si_cdist.h): the float64 rule, the derived error bars of the two kernel forms, the numpy restatement of the mm
kernel's order of additions for the squared row norms, and a float64 evaluation of the two toy graphs."""
import numpy as np
import torch

from ct_reference import _ints, _parse

U = 2.0 ** -24      # the unit roundoff of float32


def round_f16(a):
    return np.asarray(a, np.float64).astype(np.float16).astype(np.float64)


def cdist_ref(x1, x2, p=2.0):
    """the plain definition in float64 on [.., P, M] and [.., R, M] (batch dimensions broadcast): (sum |a - b|^p)^(1/p), or the max"""
    a, b = np.asarray(x1, np.float64), np.asarray(x2, np.float64)
    d = np.abs(a[..., :, None, :] - b[..., None, :, :])
    if np.isinf(p):
        return d.max(axis=-1)
    return (d ** p).sum(axis=-1) ** (1.0 / p)


def _norms(x1, x2):
    a, b = np.asarray(x1, np.float64), np.asarray(x2, np.float64)
    return np.sqrt((a * a).sum(-1))[..., :, None] + np.sqrt((b * b).sum(-1))[..., None, :]


def check(got, x1, x2, p=2.0, mm=False):
    """(worst error / bar, ok) of a result against float64 on the operands as stored.  The bars are derived, not measured:
      mm      |got^2 - ref^2| <= 2 D + 4 u ref^2,  D = (M + 3) u (|a| + |b|)^2: three fp32 sums of M terms in any order, the subtraction, the root
      direct  |got - ref| <= (M + 2) u ref: one fp32 sum of M rounded terms, the root
    Under fp16 storage the result was rounded once more: the stored half stands for every value within half an fp16 ulp of it, and the
    one nearest the reference is held to the bar."""
    m = np.asarray(x1).shape[-1]
    ref = cdist_ref(x1, x2, p)
    g = np.asarray(got, np.float64)
    assert g.shape == ref.shape, (g.shape, ref.shape)
    if np.asarray(got).dtype == np.float16:
        h = 0.5 * np.spacing(np.abs(np.asarray(got))).astype(np.float64)
        g = np.clip(ref, g - h, g + h)
    if mm:
        err, bar = np.abs(g * g - ref * ref), 2.0 * (m + 3) * U * _norms(x1, x2) ** 2 + 4.0 * U * ref * ref
    else:
        err, bar = np.abs(g - ref), (m + 2) * U * ref
    ratio = float((err / np.maximum(bar, 1e-300)).max()) if err.max() > 0 else 0.0
    return ratio, bool(np.all(err <= bar))


def mm_sqnorm(x):
    """the squared norms of the rows of x [.., M] as cdist_mm_kernel adds them (fp32 or fp16 storage, float32 arithmetic): an item is 4 floats
    / 8 halves, a K-tile 8 items; partial q[v] takes the squares of item v of every K-tile, elements in k order, K-tile after K-tile; then
    ((((((q0 + q1) + q2) + q3) + q4) + q5) + q6) + q7"""
    x = np.asarray(x)
    vw = 8 if x.dtype == np.float16 else 4
    m = x.shape[-1]
    tiles = -(-m // (8 * vw))
    sq = np.zeros(x.shape[:-1] + (tiles * 8 * vw,), np.float32)
    sq[..., :m] = x.astype(np.float32) * x.astype(np.float32)
    sq = sq.reshape(x.shape[:-1] + (tiles, 8, vw))
    q = np.zeros(x.shape[:-1] + (8,), np.float32)
    for t in range(tiles):
        for j in range(vw):
            q = q + sq[..., t, :, j]
    n = q[..., 0]
    for v in range(1, 8):
        n = n + q[..., v]
    return n


def kname(kind, dtype, arg):
    """cdist_mm_kernel<T, VEC> (arg: the vector instantiation) or cdist_direct_kernel<T, NORM> (arg: p)"""
    t = "_Float16" if np.dtype(dtype) == np.float16 else "float"
    if kind == "mm":
        return "cdist_mm_kernel<%s, %s>" % (t, "true" if arg else "false")
    return "cdist_direct_kernel<%s, %d>" % (t, {1.0: 1, 2.0: 2, float("inf"): 3}[float(arg)])


def eval_toy(builder, inputs_nhwc, rnd=None):
    """float64 evaluation of build_toy_descriptor_matcher / build_toy_vq_encoder (NHWC graph inputs, in order).  rnd: applied to the inputs,
    the conv weights, the constants and every layer's output except the graph output -- the fp16-storage emulation; None: exact."""
    q = (lambda t: torch.from_numpy(rnd(t.numpy()))) if rnd else (lambda t: t)
    t64 = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    vals, feeds, result = {}, list(inputs_nhwc), None
    for typ, name, ins, outs, prm in [_parse(ln) for ln in builder.lines]:
        x = vals[ins[0]] if ins else None
        if typ == "pnnx.Input":
            y = q(t64(feeds.pop(0)).permute(0, 3, 1, 2))
        elif typ == "pnnx.Attribute":
            y = q(t64(builder.attrs[name + ".data"]))
        elif typ == "nn.Conv2d":
            w, b = q(t64(builder.attrs[name + ".weight"])), q(t64(builder.attrs[name + ".bias"]))
            y = q(torch.nn.functional.conv2d(x, w, b, _ints(prm["stride"]), _ints(prm["padding"])))
        elif typ == "nn.ReLU":
            y = torch.relu(x)
        elif typ == "F.normalize":
            y = q(torch.nn.functional.normalize(x, float(prm["p"]), int(prm["dim"]), float(prm["eps"])))
        elif typ == "Tensor.permute":
            y = x.permute(*_ints(prm["dims"])).contiguous()
        elif typ == "Tensor.view":
            y = x.reshape(*_ints(prm["shape"]))
        elif typ == "torch.cdist":
            y = t64(cdist_ref(x.numpy(), vals[ins[1]].numpy(), float(prm["p"])))
        elif typ == "pnnx.Output":
            result = x.numpy()
            continue
        else:
            raise AssertionError(typ)
        vals[outs[0]] = y
    return result
