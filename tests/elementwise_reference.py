"""Float64 statements of the elementwise operators (ops.hip, fp32 and fp16 storage), the input sets that reach their edges and the comparators that
hold a kernel to them.  Pure numpy: tests/test_elementwise_reference_cpu.py pins this file against torch and the C oracle without a GPU,
tests/test_gpu_elementwise_edges.py holds the HIP kernels to it.

Every function takes any float array and computes in the array's own type when that is float32 or float64 (float16 is widened to float32
first): called with float64 it is the reference, called with float32 it is "a correct fp32 implementation", which the CPU tests use to show
that the bars below can be met.  Non-finite inputs are data: nothing here raises on them."""
import numpy as np

GRID_CAP = 2048 * 256     # work items of one pass of a capped launch: si_grid_for (simpleinfer_amd/csrc/hip/si_hip_internal.h)

FLT_MAX = float(np.finfo(np.float32).max)
FLT_MIN = float(np.finfo(np.float32).tiny)
FLT_DENORM = float(np.float32(1e-45))
F32_EPS = float(np.finfo(np.float32).eps)   # 2^-23
H_MAX = 65504.0

UNARY_NAMES = ["abs", "neg", "floor", "ceil", "square", "sqrt", "rsqrt", "exp", "log", "sin", "cos", "tan", "asin", "acos", "atan",
               "reciprocal", "tanh", "log10"]
UNARY_EXACT = (0, 1, 2, 3, 4, 5, 6, 15)          # IEEE arithmetic: bit-exact in fp32
BINARY_NAMES = {0: "add", 1: "sub", 2: "mul", 3: "div", 6: "pow", 7: "rsub", 8: "rdiv", 9: "rpow", 10: "atan2", 11: "ratan2"}
BINARY_EXACT = (0, 1, 2, 3, 7, 8)
ACTIVATIONS = ("relu", "silu", "sigmoid", "hardsigmoid", "hardswish", "leakyrelu")
# fp16 storage: the functions whose result is the correctly rounded fp32 operation(s) on fp16 operands rounded once more to 11 bits -- with a
# 24-bit intermediate that second rounding never changes the result (test_elementwise_reference_cpu.py counts it), so the bar is equality
H_EXACT_UNARY = (0, 1, 2, 3, 4, 5, 6, 15, 16)
H_EXACT_ACT = ("relu", "leakyrelu", "hardsigmoid")
H_MISMATCH_SHARE = 0.01                          # of the other functions at most this share of the 65536 inputs may differ (by 1 ulp) at all


def _work(x):
    x = np.asarray(x)
    return x.astype(np.float32) if x.dtype == np.float16 else x


def unary_ref(op, x):
    """UnaryOp code `op` (si_unary_apply's numbering).  rsqrt is the operator as the project defines it -- an IEEE square root and an IEEE
    division (`1.0f / sqrtf(x)`) -- so in float64 the square root is rounded to fp32 before the division: two fp32 roundings, not one."""
    x = _work(x)
    one = x.dtype.type(1)
    with np.errstate(all="ignore"):
        if op == 0: return np.abs(x)
        if op == 1: return -x
        if op == 2: return np.floor(x)
        if op == 3: return np.ceil(x)
        if op == 4: return x * x
        if op == 5: return np.sqrt(x)
        if op == 6: return one / np.sqrt(x).astype(np.float32).astype(x.dtype)
        if op == 7: return np.exp(x)
        if op == 8: return np.log(x)
        if op == 9: return np.sin(x)
        if op == 10: return np.cos(x)
        if op == 11: return np.tan(x)
        if op == 12: return np.arcsin(x)
        if op == 13: return np.arccos(x)
        if op == 14: return np.arctan(x)
        if op == 15: return one / x
        if op == 16: return np.tanh(x)
        if op == 17: return np.log10(x)
    raise ValueError(op)


def binary_ref(op, x, y):
    """BinaryOp code `op` of binary_apply (ops.hip): 7 / 8 / 9 / 11 are the operand-reversed forms"""
    x, y = _work(x), _work(y)
    if np.ndim(y) == 0:
        y = x.dtype.type(y)
    with np.errstate(all="ignore"):
        if op == 0: return x + y
        if op == 1: return x - y
        if op == 2: return x * y
        if op == 3: return x / y
        if op == 6: return np.power(x, y)
        if op == 7: return y - x
        if op == 8: return y / x
        if op == 9: return np.power(y, x)
        if op == 10: return np.arctan2(x, y)
        if op == 11: return np.arctan2(y, x)
    raise ValueError(op)


BINARY_REVERSED = {0: 0, 2: 2, 1: 7, 7: 1, 3: 8, 8: 3, 6: 9, 9: 6, 10: 11, 11: 10}


def activation_ref(kind, x, param=0.0):
    """torch's definitions; NaN goes through every one of them, silu(-inf) and hardswish(-inf) are -inf * 0 = NaN"""
    x = _work(x)
    t = x.dtype.type
    with np.errstate(all="ignore"):
        if kind == "relu": return np.maximum(x, t(0))
        if kind == "sigmoid": return t(1) / (t(1) + np.exp(-x))
        if kind == "silu": return x * (t(1) / (t(1) + np.exp(-x)))
        if kind == "hardsigmoid": return np.clip(x / t(6) + t(0.5), t(0), t(1))
        if kind == "hardswish": return x * np.clip(x / t(6) + t(0.5), t(0), t(1))
        if kind == "leakyrelu": return np.where(x > 0, x, x * t(param))
    raise ValueError(kind)


def mul_round_odd_f32(x, p):
    """the fp32 product x * p rounded to odd (a sticky last bit), for fp32 x and an fp32 scalar p whose product is exact in float64: what an
    fp32 implementation has to hand to an fp16 store for the stored value to be the exact product rounded ONCE (the slope of a leaky relu is
    an fp32 value, so the product of a widened half and the slope has up to 35 significant bits and fp32 -> fp16 would round a second time)"""
    x = np.asarray(x, np.float32)
    exact = x.astype(np.float64) * np.float64(np.float32(p))
    with np.errstate(all="ignore"):
        hi = exact.astype(np.float32)
    lo = exact - hi.astype(np.float64)
    u = hi.view(np.uint32).copy()
    fix = np.isfinite(hi) & (lo != 0) & ((u & 1) == 0)
    up = (lo < 0) == (hi < 0)
    u[fix & up] += np.uint32(1)
    u[fix & ~up] -= np.uint32(1)
    return u.view(np.float32)


def batchnorm_ref(x, mean, var, gamma, beta, eps):
    f = np.float64
    return (np.asarray(x, f) - np.asarray(mean, f)) / np.sqrt(np.asarray(var, f) + f(eps)) * np.asarray(gamma, f) + np.asarray(beta, f)


def avgpool_ref(x, out_hw):
    """uniform windows (ih % oh == 0, iw % ow == 0): the float64 mean of each"""
    x = np.asarray(x, np.float64)
    n, ih, iw, c = x.shape
    oh, ow = out_hw
    assert ih % oh == 0 and iw % ow == 0
    return x.reshape(n, oh, ih // oh, ow, iw // ow, c).mean(axis=(2, 4))


def maxpool_ref(x, k, s, p, d=(1, 1), lowest=-FLT_MAX, dtype=np.float64):
    """the window maximum over the taps inside the map, starting from `lowest` -- the reference starts its running maximum at
    numeric_limits::lowest() (the oracle restates it), so a window that holds only -inf returns the lowest FINITE value of the storage type.
    dtype: a maximum is exact in any type, so a large tensor may stay in its own"""
    x = np.asarray(x, dtype)
    n, ih, iw, c = x.shape
    oh = (ih + 2 * p[0] - ((k[0] - 1) * d[0] + 1)) // s[0] + 1
    ow = (iw + 2 * p[1] - ((k[1] - 1) * d[1] + 1)) // s[1] + 1
    ph, pw = (oh - 1) * s[0] + (k[0] - 1) * d[0] + 1, (ow - 1) * s[1] + (k[1] - 1) * d[1] + 1
    xp = np.full((n, max(ph, ih + p[0]), max(pw, iw + p[1]), c), lowest, dtype)
    xp[:, p[0]:p[0] + ih, p[1]:p[1] + iw] = x
    out = np.full((n, oh, ow, c), lowest, dtype)
    for ky in range(k[0]):
        for kx in range(k[1]):
            y0, x0 = ky * d[0], kx * d[1]
            np.maximum(out, xp[:, y0:y0 + (oh - 1) * s[0] + 1:s[0], x0:x0 + (ow - 1) * s[1] + 1:s[1]], out=out)
    return out


def linear_ref(x, w, b=None):
    y = np.asarray(x, np.float64) @ np.asarray(w, np.float64).T
    return y if b is None else y + np.asarray(b, np.float64)


# ---- input sets ------------------------------------------------------------------------------------------------------------------------------
def all_halves():
    """the 65536 fp16 bit patterns, in bit order"""
    return np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16)


def convert_probe():
    """fp32 values that pin fp32 -> fp16 rounding: every finite half, every tie between two neighbouring halves with the fp32 value on either
    side of it, the overflow threshold, the underflow tie and fp32 denormals"""
    f = np.float32
    h = all_halves()
    finite = h[np.isfinite(h)].astype(f)
    pos = np.sort(finite[(finite > 0) | ((finite == 0) & ~np.signbit(finite))])          # +0 .. 65504, ascending
    mid = ((pos[:-1].astype(np.float64) + pos[1:].astype(np.float64)) / 2).astype(f)     # 12 significant bits: exact in fp32
    assert (mid.astype(np.float64) * 2 == pos[:-1].astype(np.float64) + pos[1:]).all()
    ties = np.concatenate([mid, np.nextafter(mid, f(0)), np.nextafter(mid, f(np.inf))])
    tiny = f(2.0 ** -25)
    edge = np.array([np.nextafter(f(65520), f(0)), 65520.0, np.nextafter(f(65520), f(np.inf)), FLT_MAX, np.inf,
                     tiny, np.nextafter(tiny, f(1)), np.nextafter(tiny, f(0)), FLT_DENORM, 1e-40, 1e-39, np.nextafter(f(FLT_MIN), f(0)), FLT_MIN], f)
    return np.concatenate([finite, ties, -ties, edge, -edge, np.array([np.nan], f)])


_EDGES = [1.0, 88.72, 88.73, 87.3, 103.9, 104.0, 0.5, 2.0, 3.0, 6.0, 3.1415927, 1.5707964, 0.7853982, 1e5, 1e10, 1e22, 65504.0, 2.0 ** -24]


def special_f32():
    """±0, ±inf, NaN, the ends of the finite and of the normal range, ±1 and every function's domain edges (asin / acos: ±1 and the fp32 values
    next to them; exp: overflow at 88.72, denormal results below -87.3, zero below -103.9; log: 0; trigonometric range reduction: multiples
    of pi/4 and large arguments), each in both signs"""
    f = np.float32
    v = [0.0, np.inf, FLT_MAX, FLT_MIN, FLT_DENORM, float(np.nextafter(f(FLT_MIN), f(0))), float(np.nextafter(f(1), f(0))),
         float(np.nextafter(f(1), f(2)))] + _EDGES
    v = np.array(v, f)
    return np.concatenate([v, -v, np.array([np.nan], f)])


def _log_spaced(lo_exp, hi, n):
    """n fp32 magnitudes from 2^lo_exp up to hi, evenly spaced in log2"""
    e = np.linspace(lo_exp, np.log2(hi), n)
    return np.minimum(np.exp2(e), hi).astype(np.float32)


def wide_sweep(op, n=1 << 18):
    """about n fp32 values log-spaced in magnitude over the whole finite domain of `op` (a unary name, an activation name, or "any"), both
    signs where the domain has both"""
    if op in ("sqrt", "rsqrt", "log", "log10"):
        return _log_spaced(-149, FLT_MAX, n)
    if op in ("asin", "acos"):
        m = _log_spaced(-149, 1.0, n // 2)
        return np.concatenate([m, -m])
    if op == "exp":      # finite non-zero results: -103.98 < x < 88.73
        return np.concatenate([_log_spaced(-149, 88.73, n // 2), -_log_spaced(-149, 104.0, n // 2)])
    m = _log_spaced(-149, FLT_MAX, n // 2)
    return np.concatenate([m, -m])


def sigmoid_band():
    """-104 <= x <= -87 in steps of 1/64: exp(-x) overflows fp32 inside it and 1 / (1 + exp(-x)) is an fp32 denormal"""
    return (-104.0 + np.arange((104 - 87) * 64 + 1) / 64.0).astype(np.float32)


# ---- comparators ---------------------------------------------------------------------------------------------------------------------------
def round_to(ref, dtype):
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return np.asarray(ref, np.float64).astype(dtype)


def class_errors(got, ref, dtype=None, skip=None):
    """boolean map of the elements whose class is wrong: NaN exactly where the reference has NaN, an infinity of the same sign exactly where
    the reference ROUNDED TO THE STORAGE TYPE has one.  skip: elements not judged (the overflow band)"""
    got = np.asarray(got)
    r = round_to(ref, dtype or got.dtype)
    g = got.astype(np.float64)
    bad = (np.isnan(g) != np.isnan(r)) | (np.isposinf(g) != np.isposinf(r)) | (np.isneginf(g) != np.isneginf(r))
    if skip is not None:
        bad &= ~skip
    return bad


def assert_class(got, ref, what="", dtype=None, skip=None):
    bad = class_errors(got, ref, dtype, skip)
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise AssertionError("%s: %d elements of the wrong class (NaN / +inf / -inf); first at %d: got %r, reference %r" % (
            what, int(bad.sum()), i, np.asarray(got).reshape(-1)[i], np.asarray(ref).reshape(-1)[i]))


def overflow_band(ref, ulps=4):
    """where |ref| lies within `ulps` fp32 ulps of FLT_MAX, on either side: an fp32 function may land on a finite value or on the infinity"""
    a = np.abs(np.asarray(ref, np.float64))
    return (a >= FLT_MAX * (1 - ulps * F32_EPS)) & (a <= FLT_MAX * (1 + ulps * F32_EPS))


def ulp32(got, ref):
    """error of the finite elements in units of 2^-23 * |ref|, after the absolute allowance of test_oracle.assert_ulp (1e-37); 0 elsewhere"""
    g, r = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    fin = np.isfinite(g) & np.isfinite(round_to(r, np.float32))
    with np.errstate(all="ignore"):
        e = np.maximum(np.abs(g - r) - 1e-37, 0) / (F32_EPS * np.abs(r))
    e[~fin] = 0
    return np.nan_to_num(e, nan=0.0, posinf=np.inf)


def assert_ulp32(got, ref, ulps, what="", band=False):
    """class everywhere, then test_oracle.assert_ulp's rule (|got - ref| <= ulps * 2^-23 * |ref| + 1e-37) on the finite elements.  band: inside
    overflow_band(ref) a finite value of that band or the infinity of the right sign is accepted.  Returns (worst ulp, elements in the band)"""
    got = np.asarray(got, np.float32)
    ref = np.asarray(ref, np.float64)
    skip = overflow_band(ref, ulps) if band else np.zeros(ref.shape, bool)
    if skip.any():
        g = got[skip].astype(np.float64)
        ok = (np.sign(g) == np.sign(ref[skip])) & (np.abs(g) >= FLT_MAX * (1 - ulps * F32_EPS))
        assert ok.all(), "%s: %d results in the overflow band are neither a value within %g ulp of FLT_MAX nor the infinity" % (what, int((~ok).sum()), ulps)
    assert_class(got, ref, what, np.float32, skip)
    e = ulp32(got, ref)
    e[skip] = 0
    worst = float(e.max()) if e.size else 0.0
    if worst > ulps:
        i = int(np.argmax(e))
        raise AssertionError("%s: %d elements beyond %g ulp, worst %.3g ulp at %d: got %r, reference %r" % (
            what, int((e > ulps).sum()), ulps, worst, i, got.reshape(-1)[i], ref.reshape(-1)[i]))
    return worst, int(skip.sum())


def assert_bits32(got, ref, what=""):
    """fp32 equality of bits with the float64 reference rounded once to fp32, signs of zero included; NaN by class"""
    got = np.asarray(got, np.float32)
    r = round_to(ref, np.float32)
    nan = np.isnan(r)
    bad = (np.isnan(got) != nan) | (~nan & (got.view(np.uint32) != r.view(np.uint32)))
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise AssertionError("%s: %d of %d elements differ in their bits; first at %d: got %r, reference %r" % (
            what, int(bad.sum()), bad.size, i, got.reshape(-1)[i], r.reshape(-1)[i]))


def half_order(h):
    """the ordered-integer map of fp16 bit patterns: monotonic in the value, neighbours 1 apart, +0 and -0 both 0"""
    b = np.ascontiguousarray(np.asarray(h, np.float16)).view(np.uint16).astype(np.int32)
    mag = b & 0x7FFF
    return np.where(b & 0x8000, -mag, mag)


def half_ulp(got, ref):
    """(distance in fp16 ulps of got from the float64 reference rounded once to fp16, 0 where both are NaN) after the class check"""
    got = np.asarray(got, np.float16)
    r = round_to(ref, np.float16)
    d = np.abs(half_order(got) - half_order(r))
    d[np.isnan(r) & np.isnan(got)] = 0
    return d


def assert_half(got, ref, max_ulp, what="", max_share=None):
    """class everywhere; every element within max_ulp fp16 ulps of the reference rounded once to fp16; at most max_share of the elements
    differ at all.  Returns (elements that differ, worst ulp)"""
    assert_class(np.asarray(got, np.float16), ref, what, np.float16)
    d = half_ulp(got, ref)
    n, worst = int((d > 0).sum()), int(d.max()) if d.size else 0
    if worst > max_ulp:
        i = int(np.argmax(d))
        raise AssertionError("%s: %d elements differ, worst %d fp16 ulp (allowed %d) at %d: got %r, reference %r" % (
            what, n, worst, max_ulp, i, np.asarray(got).reshape(-1)[i], np.asarray(ref).reshape(-1)[i]))
    if max_share is not None:
        assert n <= max_share * d.size, "%s: %d of %d elements differ by one ulp: more than %g%%" % (what, n, d.size, 100 * max_share)
    return n, worst


def same_bits_or_nan(a, b):
    """True where two arrays of one float type hold the same bits, or both a NaN"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, a.dtype, b.shape, b.dtype)
    u = {2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return (a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))


def assert_arms_agree(a, b, what=""):
    ok = same_bits_or_nan(a, b)
    if not ok.all():
        i = int(np.flatnonzero(~ok)[0])
        raise AssertionError("%s: %d of %d elements differ between two arms of one entry; first at %d: %r vs %r" % (
            what, int((~ok).sum()), ok.size, i, np.asarray(a).reshape(-1)[i], np.asarray(b).reshape(-1)[i]))


# ---- layouts: one flat value list as the tensor a dispatch arm takes ------------------------------------------------------------------------
def as_rows(flat, c, odd_pixels=False):
    """flat values as [1, 1, pixels, c]; the tail repeats the first values.  odd_pixels: an odd pixel count, so that with odd c the element
    count is odd (no 16-byte arm can take the dense tensor as one long row).  Returns (tensor, number of leading elements that are `flat`)"""
    flat = np.asarray(flat).reshape(-1)
    px = -(-flat.size // c)
    if odd_pixels and px % 2 == 0:
        px += 1
    t = np.resize(flat, px * c).reshape(1, 1, px, c)
    return t, flat.size
