"""The yardstick of tests/test_gpu_f16_rounding.py (pinned on the CPU by tests/test_f16_rounding_cpu.py): what the STORED half of an fp16
convolution has to be.  The contract: the epilogue runs in fp32, the store rounds ONCE to nearest-even, subnormal halves are kept,
and a value overflows to inf from 65520 on.

Two kinds of expected value:
  * the kernel's own fp32 store rounded here (assert_f16_store): accumulation order drops out, only the store is on test;
  * operands built so that every product and every partial sum is exact in fp32 in ANY order (the builders below): the expected half is
    rne16 of plain float64 arithmetic and owes nothing to the kernel.
"""
import itertools

import numpy as np

from util import rng_uniform

F64 = np.float64
F32 = np.float32
SCALE_KS = (0, -6, -14, 5)     # 2^k of the selector cases: identity, an inexact shift, gradual underflow at the store, the overflow threshold
# (k -> subnormal results, inexact results, zeros, infs) of x * 2^k over all finite halves: what the GPU cases rely on, asserted on the CPU
SCALE_CLASSES = {0: (2046, 0, 2, 0), -6: (14268, 12288, 66, 0), -14: (22524, 28672, 8194, 0), 5: (62, 10240, 2, 10240)}


def rne16(a):
    """float64 / float32 -> fp16, ONE rounding to nearest-even (overflow to inf from 65520, gradual underflow)"""
    with np.errstate(over="ignore"):
        return np.asarray(a).astype(np.float16)


def rne16_model_bits(v):
    """The bit pattern of rne16(v) from an integer model of binary16 -- independent of numpy's conversion.  v: finite values whose significand
    fits fp32 (every scaling below is then exact in float64)."""
    v = np.asarray(v, F64)
    sign = np.where(np.signbit(v), 0x8000, 0).astype(np.int64)
    a = np.abs(v)
    _, e = np.frexp(a)                                  # a = m * 2^e, m in [0.5, 1): the leading bit has weight 2^(e - 1)
    E = np.where(a == 0, -14, np.maximum(e - 1, -14))   # exponent of the half's binade; subnormals share the lowest one
    scaled = np.ldexp(a, 10 - E)                        # in units of that binade's ulp: [1024, 2048) for normals, [0, 1024) below
    n = np.floor(scaled)
    frac = scaled - n
    n = n.astype(np.int64)
    n += ((frac > 0.5) | ((frac == 0.5) & (n % 2 == 1))).astype(np.int64)
    normal = n >= 1024                                  # (a carry out of a subnormal lands on 0x0400, out of a binade on the next exponent)
    bits = np.where(normal, ((E + 15) << 10) + (n - 1024), n)
    bits = np.where((E > 15) | (bits >= 0x7C00), 0x7C00, bits)
    return (bits | sign).astype(np.uint16)


def all_finite_halves():
    """the 63488 finite fp16 bit patterns (2046 of them subnormal), in bit order"""
    b = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    return b[(b & 0x7C00) != 0x7C00].view(np.float16)


def halves_tensor(shape):
    """every finite half at least once, laid out as `shape` (wrapping around when the shape holds more)"""
    hv = all_finite_halves()
    assert int(np.prod(shape)) >= hv.size, shape
    return np.resize(hv, shape)


def is_subnormal16(a):
    b = np.asarray(a, np.float16).view(np.uint16)
    return ((b & 0x7C00) == 0) & ((b & 0x03FF) != 0)


def class_shares(v):
    """(share of subnormal halves, share of inf) among rne16(v)"""
    r = rne16(v)
    return float(is_subnormal16(r).mean()), float(np.isinf(r).mean())


def assert_f16_store(got16, v32, what=""):
    """got16 holds the bits of rne16(v32) everywhere; +0 and -0 are one class, nothing else is excused"""
    got16 = np.asarray(got16)
    assert got16.dtype == np.float16, (what, got16.dtype)
    want = rne16(v32)
    assert got16.shape == want.shape, (what, got16.shape, want.shape)
    g, w = got16.view(np.uint16).reshape(-1), want.view(np.uint16).reshape(-1)
    bad = (g != w) & (((g | w) & 0x7FFF) != 0)
    if bad.any():
        i = int(np.argmax(bad))
        raise AssertionError("%s: %d of %d stored halves are not the nearest-even rounding; first at flat index %d: got 0x%04x (%r), want 0x%04x (%r) from %r"
                             % (what, int(bad.sum()), bad.size, i, int(g[i]), float(got16.reshape(-1)[i]), int(w[i]), float(want.reshape(-1)[i]),
                                float(np.asarray(v32).reshape(-1)[i])))


def f16_bound(ref, a):
    """Element-wise bar of ONE fp16 conv against the float64 conv on the same rounded operands.  a: the bar the fp32 store of the same call
    carries (2e-5 * max|ref| plain, 1e-4 * max|ref| with a fused activation).  Then: the half-ulp of one nearest-even store of a value that far
    from ref, four fp32 roundings of the epilogue, and half the subnormal step."""
    r = np.abs(np.asarray(ref, F64))
    return a + 2.0 ** -11 * (r + a) + 2.0 ** -22 * r + 2.0 ** -25


def assert_f16_elementwise(got16, ref, a_rel, what=""):
    ref = np.asarray(ref, F64)
    a = a_rel * float(np.abs(ref).max())
    d = np.abs(np.asarray(got16).astype(F64) - ref)
    over = d > f16_bound(ref, a)
    assert not over.any(), "%s: %d of %d elements beyond the element-wise fp16 bound; worst |d| - bound = %.3e" % (
        what, int(over.sum()), over.size, float((d - f16_bound(ref, a)).max()))


def act32(kind, v, p=0.0):
    """the IEEE-exact fused activations, in float32 as the epilogue evaluates them"""
    v = np.asarray(v, F32)
    if kind == "none":
        return v
    if kind == "relu":
        return np.maximum(v, F32(0))
    if kind == "leakyrelu":
        return np.where(v > 0, v, v * F32(p)).astype(F32)
    raise ValueError(kind)


def epilogue_ref32(acc, bias=None, act1="none", residual=None, act2="none", p=0.0):
    """The documented epilogue order in float32: (acc + bias), act1, + residual, act2 -- the caller rounds the result once (rne16).
    acc: exact accumulators (float64 values representable in fp32)."""
    v = np.asarray(acc, F64).astype(F32)
    assert np.array_equal(v.astype(F64), np.asarray(acc, F64)), "the accumulator is not exact in fp32"
    if bias is not None:
        v = v + np.asarray(bias, F32)
    v = act32(act1, v, p)
    if residual is not None:
        v = v + np.asarray(residual, np.float16).astype(F32)
    return act32(act2, v, p)


def partial_sums_exact(terms):
    """terms [..., T] (float64 products of one output's non-zero taps): every sum over every non-empty subset survives float64 -> float32 ->
    float64, so an fp32 accumulator is exact whatever order the kernel adds them in (the other taps contribute exact zeros)"""
    terms = np.asarray(terms, F64)
    T = terms.shape[-1]
    for r in range(1, T + 1):
        for idx in itertools.combinations(range(T), r):
            s = terms[..., list(idx)].sum(-1)        # (float64 holds these sums exactly: <= 3 terms of <= 24 bits within 2^40 of each other)
            if not np.array_equal(s.astype(F32).astype(F64), s):
                return False
    return True


# ---- exact-by-construction operands ------------------------------------------------------------------------------------------------------------
def selector_weights(oc, icg, kh, kw, k, src, taps=None, dtype=F32):
    """w[o, src[o], tap[o]] = 2^k and zero elsewhere; tap[o] = o % (kh * kw) unless given.  Returns (w OIHW, tap rows, tap columns)."""
    taps = np.arange(oc) % (kh * kw) if taps is None else np.asarray(taps)
    ty, tx = taps // kw, taps % kw
    w = np.zeros((oc, icg, kh, kw), dtype)
    w[np.arange(oc), np.asarray(src), ty, tx] = 2.0 ** k
    return w, ty, tx


def selector_expected(x, src, ty, tx, k, stride=1, pad=0, kh=1, kw=1):
    """float64 value of the selector conv: output channel o is x's channel src[o] at tap (ty[o], tx[o]) times 2^k, zero outside the image"""
    x = np.asarray(x).astype(F64)
    n, h, w, _ = x.shape
    oh, ow = (h + 2 * pad - kh) // stride + 1, (w + 2 * pad - kw) // stride + 1
    xp = np.pad(x, ((0, 0), (pad, pad), (pad, pad), (0, 0)))
    out = np.empty((n, oh, ow, len(src)), F64)
    for o, c in enumerate(src):
        out[..., o] = xp[:, ty[o]:ty[o] + (oh - 1) * stride + 1:stride, tx[o]:tx[o] + (ow - 1) * stride + 1:stride, c]
    return out * 2.0 ** k


def permutation(n, seed):
    return np.random.Generator(np.random.Philox(seed)).permutation(n)


TIE_EXPONENTS = range(-4, 15)
TIE_TRIPLES = 8     # triples (x_a, x_b, x_c) in channels 3t .. 3t + 2 of a 32-channel pixel; channels 24 .. 31 carry values no weight selects


def tie_case():
    """y = x_a + 2^-11 x_b + s 2^-13 x_c with x_b = sign(x_a) 2^floor(log2 |x_a|), x_c = 2^-10 x_b, s = -1 / 0 / +1 by output channel:
    x_a + 2^-11 x_b is exactly the midpoint between x_a and the next half away from zero, and s moves it by one fp32 ulp.  x_a runs over every
    normal half of exponent -4 .. 14.  Returns x [2, 19, 128, 32] (fp16), w [24, 32, 1, 1], the float64 sums [.., 24], the terms [.., 24, 3]
    and s per output channel."""
    hv = all_finite_halves()
    b = hv.view(np.uint16)
    e = ((b >> 10) & 31).astype(np.int64) - 15
    xa = hv[(((b >> 10) & 31) != 0) & (e >= TIE_EXPONENTS[0]) & (e <= TIE_EXPONENTS[-1])].astype(F64)
    assert xa.size == 2 * 1024 * len(TIE_EXPONENTS)
    xb = np.sign(xa) * 2.0 ** np.floor(np.log2(np.abs(xa)))
    xc = xb * 2.0 ** -10
    pix = xa.size // TIE_TRIPLES
    x = np.empty((pix, 32), F64)
    for t in range(TIE_TRIPLES):
        sl = slice(t * pix, (t + 1) * pix)
        x[:, 3 * t], x[:, 3 * t + 1], x[:, 3 * t + 2] = xa[sl], xb[sl], xc[sl]
    x[:, 24:] = rng_uniform(77, (pix, 8), -4, 4).astype(np.float16)
    x16 = x.astype(np.float16)
    assert np.array_equal(x16.astype(F64), x)
    oc = 3 * TIE_TRIPLES
    s = np.arange(oc) % 3 - 1
    w = np.zeros((oc, 32, 1, 1), F32)
    terms = np.empty((pix, oc, 3), F64)
    for o in range(oc):
        t = o // 3
        w[o, 3 * t, 0, 0], w[o, 3 * t + 1, 0, 0], w[o, 3 * t + 2, 0, 0] = 1.0, 2.0 ** -11, s[o] * 2.0 ** -13
        terms[:, o, 0], terms[:, o, 1], terms[:, o, 2] = x[:, 3 * t], x[:, 3 * t + 1] * 2.0 ** -11, x[:, 3 * t + 2] * (s[o] * 2.0 ** -13)
    shape = (2, len(TIE_EXPONENTS), pix // (2 * len(TIE_EXPONENTS)))
    return x16.reshape(shape + (32,)), w, terms.sum(-1).reshape(shape + (oc,)), terms.reshape(shape + (oc, 3)), s


def stem_tie_image(shape=(2, 126, 252, 3)):
    """fp32 image of the stem cases: the midpoint between every two neighbouring positive finite halves, the fp32 value on either side of it,
    and their negatives (everything below 65520, so the image's halves are finite): the in-kernel fp32 -> fp16 conversion sees every tie"""
    hv = all_finite_halves()
    pos = np.sort(hv[~np.signbit(hv)].astype(F64))
    mid = ((pos[:-1] + pos[1:]) / 2).astype(F32)
    assert np.array_equal(mid.astype(F64), (pos[:-1] + pos[1:]) / 2)
    v = np.concatenate([mid, np.nextafter(mid, F32(0)), np.nextafter(mid, F32(np.inf))])
    v = np.concatenate([v, -v])
    assert np.abs(v).max() < 65520 and int(np.prod(shape)) >= v.size
    return np.resize(v, shape).astype(F32)


# ---- wide-range data: outputs that are subnormal halves, overflow, and everything between ------------------------------------------------------
def wide_range_case(seed, xshape, oc, k, groups=1, bias=False, lo_exp=-18, w_amp=0.3):
    """x = h(16 U(-1,1)), w[o] = h(U(-w_amp,w_amp) 2^(lo_exp + o % 32)), bias scaled the same way per channel (fp32).  Returns x (fp16), w (fp32
    values that are halves), bias or None."""
    x = rng_uniform(seed, xshape, -16, 16).astype(np.float16)
    sc = (2.0 ** (lo_exp + np.arange(oc) % 32)).astype(F32)
    w = (rng_uniform(seed + 1, (oc, xshape[-1] // groups, k, k), -w_amp, w_amp) * sc[:, None, None, None]).astype(np.float16).astype(F32)
    b = (rng_uniform(seed + 2, (oc,), -0.5, 0.5) * sc) if bias else None
    return x, w, b


def scaled_weights(seed, oc, icg, k, lo_exp, amp):
    """one stage of the fused-launch cases: w[o] = h(U(-amp,amp) 2^(lo_exp + o % 32)) and an fp32 bias scaled the same way per channel"""
    sc = (2.0 ** (lo_exp + np.arange(oc) % 32)).astype(F32)
    w = (rng_uniform(seed, (oc, icg, k, k), -amp, amp) * sc[:, None, None, None]).astype(np.float16).astype(F32)
    return w, rng_uniform(seed + 1, (oc,), -0.5, 0.5) * sc


# exponent of the smallest channel scale of a fused launch's stages: -25 where the stage's output is an intermediate (2^-25 .. 2^6: it stays
# finite -- the GPU test asserts that -- and a quarter of it is subnormal), -22 for the stage that stores the result (subnormal halves to inf)
FUSED_MID_EXP, FUSED_OUT_EXP = -25, -22
