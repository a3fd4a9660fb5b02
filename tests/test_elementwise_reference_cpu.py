"""CPU: pins tests/elementwise_reference.py -- the float64 statements, the input sets and the comparators that
tests/test_gpu_elementwise_edges.py holds the elementwise HIP kernels to -- before any kernel is compared with it:

1. the float64 functions agree with torch in float64 (values and NaN / inf classes, special values included) and with the C oracle at the
   oracle's own bars on the oracle's own inputs;
2. the input sets contain what they promise, and numpy's fp32 -> fp16 conversion (the expected value of the conversion kernels) is torch's;
3. the fp16 bars are reachable: the same functions evaluated in float32 numpy and rounded to fp16 meet them;
4. the comparators reject what they are there to reject (a truncating store, a flushed denormal, a wrong class, a wrong sign of zero).
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import elementwise_reference as er
from test_oracle import assert_ulp, unary_input
from util import assert_exact, assert_parity, rng_uniform

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "ops_golden.npz"))

T = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64))


def close64(got, ref, what, rel=1e-13):
    """two float64 evaluations of one function: the same classes, and values within a few ulps of double"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert not er.class_errors(got, ref, np.float64).any(), "%s: NaN / inf classes differ at %s" % (what, np.flatnonzero(er.class_errors(got, ref, np.float64))[:5])
    fin = np.isfinite(ref)
    assert (np.abs(got[fin] - ref[fin]) <= rel * np.abs(ref[fin]) + 1e-300).all(), what


def probe64(name):
    """special values plus a thinned wide sweep, widened"""
    return np.concatenate([er.special_f32(), er.wide_sweep(name)[::37]]).astype(np.float64)


TORCH_UNARY = {0: torch.abs, 1: torch.neg, 2: torch.floor, 3: torch.ceil, 4: torch.square, 5: torch.sqrt,
               6: lambda x: 1.0 / torch.sqrt(x).float().double(), 7: torch.exp, 8: torch.log, 9: torch.sin, 10: torch.cos, 11: torch.tan,
               12: torch.asin, 13: torch.acos, 14: torch.atan, 15: torch.reciprocal, 16: torch.tanh, 17: torch.log10}


@pytest.mark.parametrize("op", range(18))
def test_unary_reference_is_torch_float64(op):
    x = probe64(er.UNARY_NAMES[op])
    close64(er.unary_ref(op, x), TORCH_UNARY[op](T(x)).numpy(), er.UNARY_NAMES[op])


def test_rsqrt_reference_is_two_fp32_operations():
    """the operator is `1.0f / sqrtf(x)` (si_unary_apply): the reference rounds the square root to fp32, so it equals the fp32 evaluation bit
    for bit, and lies within one fp32 ulp of the one-rounding 1 / sqrt(x)"""
    x = er.wide_sweep("rsqrt")
    two = er.round_to(er.unary_ref(6, x.astype(np.float64)), np.float32)
    er.assert_bits32(np.float32(1) / np.sqrt(x), er.unary_ref(6, x.astype(np.float64)), "rsqrt fp32")
    one = 1.0 / np.sqrt(x.astype(np.float64))
    assert er.ulp32(two, one).max() <= 1.0


def test_binary_reference_is_torch_float64():
    s = er.special_f32().astype(np.float64)
    x, y = [g.reshape(-1) for g in np.meshgrid(s, s, indexing="ij")]
    tf = {0: torch.add, 1: torch.sub, 2: torch.mul, 3: torch.div, 6: torch.pow, 10: torch.atan2}
    for op, fn in tf.items():
        close64(er.binary_ref(op, x, y), fn(T(x), T(y)).numpy(), er.BINARY_NAMES[op])
        close64(er.binary_ref(er.BINARY_REVERSED[op], x, y), fn(T(y), T(x)).numpy(), er.BINARY_NAMES[op] + " reversed")
        close64(er.binary_ref(op, x, 2.5), fn(T(x), torch.tensor(2.5, dtype=torch.float64)).numpy(), er.BINARY_NAMES[op] + " scalar")


@pytest.mark.parametrize("kind", er.ACTIVATIONS)
def test_activation_reference_is_torch_float64(kind):
    x = np.concatenate([probe64("any"), er.sigmoid_band().astype(np.float64)])
    fn = {"relu": torch.relu, "silu": F.silu, "sigmoid": torch.sigmoid, "hardsigmoid": F.hardsigmoid, "hardswish": F.hardswish,
          "leakyrelu": lambda t: F.leaky_relu(t, 0.1)}[kind]
    # (torch states silu as x / (1 + exp(-x)): within a few ulps of x * sigmoid(x) except where sigmoid itself is denormal)
    close64(er.activation_ref(kind, x, 0.1), fn(T(x)).numpy(), kind, rel=1e-13 if kind != "silu" else 1e-12)
    assert np.isnan(er.activation_ref(kind, np.array([np.nan]))).all(), "NaN goes through " + kind
    if kind in ("silu", "hardswish"):
        assert np.isnan(er.activation_ref(kind, np.array([-np.inf]))).all() and np.isnan(fn(T([-np.inf])).numpy()).all()


def test_layer_references_are_torch_float64():
    nchw = lambda a: T(a).permute(0, 3, 1, 2)
    nhwc = lambda t: t.permute(0, 2, 3, 1).numpy()
    x = rng_uniform(1, (2, 12, 10, 5), -3, 1)
    for k, s, p, d in (((3, 3), (1, 1), (1, 1), (1, 1)), ((5, 5), (1, 1), (2, 2), (1, 1)), ((3, 2), (2, 3), (1, 0), (1, 2)), ((2, 2), (2, 2), (0, 0), (1, 1))):
        assert_exact(er.maxpool_ref(x, k, s, p, d), nhwc(F.max_pool2d(nchw(x), k, s, p, d)), "maxpool %s" % (k,))
    for out_hw in ((1, 1), (6, 5), (3, 2)):
        close64(er.avgpool_ref(x, out_hw), nhwc(F.adaptive_avg_pool2d(nchw(x), out_hw)), "avgpool %s" % (out_hw,))
    m, v, g, b = rng_uniform(2, (5,), -1, 1), rng_uniform(3, (5,), 0, 2), rng_uniform(4, (5,), -2, 2), rng_uniform(5, (5,), -1, 1)
    v[0], g[1], g[2] = 0.0, 0.0, -1.5
    close64(er.batchnorm_ref(x, m, v, g, b, 1e-5), nhwc(F.batch_norm(nchw(x), T(m), T(v), T(g), T(b), False, 0.0, 1e-5)), "batchnorm", rel=1e-12)
    xl, w, bl = rng_uniform(6, (3, 65), -1, 1), rng_uniform(7, (7, 65), -1, 1), rng_uniform(8, (7,), -1, 1)
    close64(er.linear_ref(xl, w, bl), F.linear(T(xl), T(w), T(bl)).numpy(), "linear", rel=1e-12)
    close64(er.linear_ref(xl, w), F.linear(T(xl), T(w)).numpy(), "linear, no bias", rel=1e-12)


# ---- the C oracle at its own bars on its own inputs (tests/test_oracle.py) ------------------------------------------------------------------
@pytest.mark.parametrize("op", range(18))
def test_unary_reference_vs_oracle(orc, op):
    x = unary_input(op)
    ref = er.unary_ref(op, x.astype(np.float64))
    if op in er.UNARY_EXACT:
        er.assert_bits32(orc.unary_op(op, x), ref, "unary %d" % op)
    else:
        assert_ulp(orc.unary_op(op, x), ref, 2, "unary %d" % op)


def test_binary_reference_vs_oracle(orc):
    a, b = rng_uniform(1, (2, 3, 4, 8), 0.5, 3.0), rng_uniform(2, (2, 3, 4, 8), 0.5, 3.0)
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    for op in er.BINARY_EXACT:
        er.assert_bits32(orc.binary_op(op, a, b), er.binary_ref(op, a64, b64), "binary %d" % op)
        er.assert_bits32(orc.binary_scalar(op, a, 1.75), er.binary_ref(op, a64, 1.75), "binary scalar %d" % op)
    assert_ulp(orc.binary_op(6, a, b), er.binary_ref(6, a64, b64), 2, "pow")
    assert_ulp(orc.binary_scalar(9, a, 2.5), er.binary_ref(9, a64, 2.5), 2, "2.5 ** x")
    assert_ulp(orc.binary_op(10, a, b - 1.5), er.binary_ref(10, a64, (b - np.float32(1.5)).astype(np.float64)), 2, "atan2")
    assert_ulp(orc.binary_op(11, a, b - 1.5), er.binary_ref(11, a64, (b - np.float32(1.5)).astype(np.float64)), 2, "atan2 reversed")


def test_layer_references_vs_oracle(orc):
    x = GOLD["act/x"]
    for kind in ("silu", "relu", "sigmoid", "hardsigmoid", "hardswish"):
        assert_parity(orc.activation(kind, x), er.activation_ref(kind, x.astype(np.float64)), 1e-6, kind)
    assert_parity(orc.batchnorm2d(GOLD["bn/x"], GOLD["bn/mean"], GOLD["bn/var"], GOLD["bn/gamma"], GOLD["bn/beta"], 1e-5),
                  er.batchnorm_ref(GOLD["bn/x"], GOLD["bn/mean"], GOLD["bn/var"], GOLD["bn/gamma"], GOLD["bn/beta"], 1e-5), 1e-6)
    assert_parity(orc.linear(GOLD["linear/x"], GOLD["linear/w"], GOLD["linear/b"]), er.linear_ref(GOLD["linear/x"], GOLD["linear/w"], GOLD["linear/b"]), 1e-6)
    assert_parity(orc.adaptive_avgpool2d(GOLD["gap/x"], (1, 1)), er.avgpool_ref(GOLD["gap/x"], (1, 1)), 1e-6)
    assert_exact(orc.maxpool2d(GOLD["maxpool_k5s1p2/x"], (5, 5), (1, 1), (2, 2)), er.maxpool_ref(GOLD["maxpool_k5s1p2/x"], (5, 5), (1, 1), (2, 2)))
    assert_exact(orc.maxpool2d(GOLD["maxpool_k3s2p1/x"], (3, 3), (2, 2), (1, 1)), er.maxpool_ref(GOLD["maxpool_k3s2p1/x"], (3, 3), (2, 2), (1, 1)))


def test_maxpool_floor_is_the_oracles(orc):
    """a window of -inf only returns the lowest finite fp32 (the reference's numeric_limits::lowest() start), one that holds +inf returns it"""
    x = rng_uniform(9, (1, 6, 6, 3), -5, -1)
    x[0, :3, :3, 0] = -np.inf
    x[0, 4, 4, 1] = np.inf
    got = orc.maxpool2d(x, (3, 3), (1, 1), (1, 1))
    ref = er.maxpool_ref(x, (3, 3), (1, 1), (1, 1))
    assert_exact(got, ref.astype(np.float32))
    assert got[0, 0, 0, 0] == -er.FLT_MAX and got[0, 1, 1, 0] == -er.FLT_MAX and np.isposinf(got[0, 3:, 3:, 1]).all()


# ---- the input sets --------------------------------------------------------------------------------------------------------------------------
def test_input_sets_hold_what_they_promise():
    h = er.all_halves()
    assert h.size == 65536 and np.unique(h.view(np.uint16)).size == 65536
    p = er.convert_probe()
    assert p.dtype == np.float32 and np.isnan(p).sum() == 1
    fin = h[np.isfinite(h)].astype(np.float32)
    assert np.isin(fin.view(np.uint32), p.view(np.uint32)).all(), "every finite half, both zeros included"
    up = np.sort(np.unique(fin))
    mid = (up[:-1].astype(np.float64) + up[1:]) / 2
    mid = mid[mid != 0]
    for v in (mid, np.nextafter(mid.astype(np.float32), np.float32(np.inf)), np.nextafter(mid.astype(np.float32), np.float32(-np.inf))):
        assert np.isin(v.astype(np.float32), p).all(), "every tie between neighbouring halves and the fp32 value on either side"
    for v in (65519.996, 65520.0, er.FLT_MAX, np.inf, -np.inf, 2.0 ** -25, -2.0 ** -25, float(np.nextafter(np.float32(2.0 ** -25), np.float32(1))), 1e-45, 1e-40):
        assert np.float32(v) in p, v
    with np.errstate(over="ignore"):
        q = p.astype(np.float16)
    assert np.isposinf(q[p == np.float32(65520.0)]).all() and (q[p == np.float32(65519.996)] == 65504).all()
    assert (q[p == np.float32(2.0 ** -25)] == 0).all() and (q[p == np.nextafter(np.float32(2.0 ** -25), np.float32(1))].view(np.uint16) == 1).all()
    s = er.special_f32()
    for v in (0.0, np.inf, er.FLT_MAX, er.FLT_MIN, 1e-45, 1.0, 88.72, 87.3, 103.9):
        assert np.float32(v) in s and np.float32(-v) in s, v
    assert np.signbit(s[s == 0]).sum() == 1 and np.isnan(s).sum() == 1
    for name in ("any", "sqrt", "asin", "exp"):
        w = er.wide_sweep(name)
        assert w.dtype == np.float32 and abs(w.size - (1 << 18)) <= 2 and np.isfinite(w).all()
    assert (er.wide_sweep("sqrt") > 0).all() and np.abs(er.wide_sweep("asin")).max() == 1.0
    assert er.wide_sweep("any").min() == -er.FLT_MAX and np.abs(er.wide_sweep("any")).min() == np.float32(1e-45)
    b = er.sigmoid_band()
    assert b[0] == -104 and b[-1] == -87 and np.allclose(np.diff(b), 1 / 64, atol=0)


def test_numpy_conversion_is_torchs():
    p = er.convert_probe()
    with np.errstate(over="ignore"):
        q = p.astype(np.float16)
    t = torch.from_numpy(p).to(torch.float16).numpy()
    assert er.same_bits_or_nan(q, t).all() and (np.isnan(q) == np.isnan(p)).all()
    back = torch.from_numpy(er.all_halves()).to(torch.float32).numpy()
    assert er.same_bits_or_nan(er.all_halves().astype(np.float32), back).all()


# ---- the fp16 bars are reachable by a correct fp32 implementation ------------------------------------------------------------------------------
def _h_bar(exact):
    return (0, None) if exact else (1, er.H_MISMATCH_SHARE)


@pytest.mark.parametrize("op", range(18))
def test_fp32_unary_meets_the_fp16_bar(op):
    h = er.all_halves()
    with np.errstate(all="ignore"):
        got = er.unary_ref(op, h.astype(np.float32)).astype(np.float16)
    bar = _h_bar(op in er.H_EXACT_UNARY)
    n, worst = er.assert_half(got, er.unary_ref(op, h.astype(np.float64)), bar[0], er.UNARY_NAMES[op], bar[1])
    assert n <= 8, (er.UNARY_NAMES[op], n)


@pytest.mark.parametrize("kind", er.ACTIVATIONS)
def test_fp32_activation_meets_the_fp16_bar(kind):
    h = er.all_halves()
    with np.errstate(all="ignore"):
        got = er.activation_ref(kind, h.astype(np.float32), 0.1).astype(np.float16)
    ref = er.activation_ref(kind, h.astype(np.float64), np.float64(np.float32(0.1)))
    if kind == "leakyrelu":
        # x * 0.1f is no fp32 operation on fp16 operands: the slope has 24 bits, the product 35, and the plain fp32 product rounded again to
        # fp16 differs from the product rounded once on 103 inputs (by 1 ulp).  The bar is equality all the same, and it is reachable in fp32
        # arithmetic: the product rounded to odd (what the kernel computes, mul_round_odd in si_hip_internal.h), then the one rounding of the store
        assert er.assert_half(got, ref, 1, kind, er.H_MISMATCH_SHARE) == (103, 1)
        x = h.astype(np.float32)
        with np.errstate(all="ignore"):
            got = np.where(x > 0, x, er.mul_round_odd_f32(x, 0.1)).astype(np.float16)
    bar = _h_bar(kind in er.H_EXACT_ACT)
    n, worst = er.assert_half(got, ref, bar[0], kind, bar[1])
    assert n <= 8, (kind, n)


def test_fp32_add_mul_are_exact_in_fp16():
    r = np.random.Generator(np.random.Philox(11))
    h = er.all_halves()
    a = np.concatenate([h, h, r.integers(0, 65536, 1 << 21).astype(np.uint16).view(np.float16)])
    b = np.concatenate([h[::-1], h[r.permutation(65536)], r.integers(0, 65536, 1 << 21).astype(np.uint16).view(np.float16)])
    for op in (0, 2):
        with np.errstate(all="ignore"):
            got = er.binary_ref(op, a.astype(np.float32), b.astype(np.float32)).astype(np.float16)
        er.assert_half(got, er.binary_ref(op, a.astype(np.float64), b.astype(np.float64)), 0, er.BINARY_NAMES[op])


# ---- the comparators reject what they are there to reject ----------------------------------------------------------------------------------
def test_comparators_reject_wrong_kernels():
    p = er.convert_probe()
    p = p[np.isfinite(p) & (np.abs(p) < 65504)]
    trunc = (p.view(np.uint32) & np.uint32(0xFFFFE000)).view(np.float32).astype(np.float16)   # round toward zero: drop the 13 low bits
    with pytest.raises(AssertionError):
        er.assert_half(trunc, p.astype(np.float64), 0, "truncating store")
    with pytest.raises(AssertionError, match="more than"):
        er.assert_half(trunc, p.astype(np.float64), 1, "truncating store", er.H_MISMATCH_SHARE)
    den = np.array([3e-6, -3e-6, 6e-8], np.float64)                                            # fp16 denormals: a flush to zero is 50, 50 and 1 ulp
    with pytest.raises(AssertionError):
        er.assert_half(np.zeros(3, np.float16), den, 1, "flushed denormals")
    assert er.assert_half(np.array([-0.0, 0.0], np.float16), np.array([0.0, -0.0]), 0) == (0, 0), "+0 and -0 are 0 apart"
    o = er.half_order(np.sort(er.all_halves()[np.isfinite(er.all_halves())].astype(np.float32)).astype(np.float16))
    assert (np.diff(o) >= 0).all() and np.diff(o).max() == 1
    for got, ref in (([0.0], [np.nan]), ([np.nan], [1.0]), ([np.inf], [-np.inf]), ([3.0e38], [np.inf]), ([np.inf], [3.0e38])):
        with pytest.raises(AssertionError, match="class"):
            er.assert_ulp32(np.array(got, np.float32), np.array(ref), 4)
    with pytest.raises(AssertionError):
        er.assert_bits32(np.array([0.0], np.float32), np.array([-0.0]))
    with pytest.raises(AssertionError, match="ulp"):
        er.assert_ulp32(np.array([1.0 + 5 * er.F32_EPS], np.float32), np.array([1.0]), 4)
    assert er.assert_ulp32(np.array([1.0 + 3 * er.F32_EPS, 1e-40], np.float32), np.array([1.0, 0.0]), 4)[0] == 3.0
    # the overflow band: a value within 4 ulp of FLT_MAX or the infinity, for a reference on either side of FLT_MAX -- and nothing else
    edge = np.array([er.FLT_MAX * (1 + 2 * er.F32_EPS), er.FLT_MAX * (1 - 2 * er.F32_EPS), -er.FLT_MAX])
    assert er.assert_ulp32(np.array([er.FLT_MAX, np.inf, -np.inf], np.float32), edge, 4, band=True)[1] == 3
    with pytest.raises(AssertionError, match="band"):
        er.assert_ulp32(np.array([1e38, np.inf, -np.inf], np.float32), edge, 4, band=True)
    with pytest.raises(AssertionError):
        er.assert_arms_agree(np.array([1.0, np.nan], np.float32), np.array([1.0, 2.0], np.float32))
    er.assert_arms_agree(np.array([1.0, np.nan], np.float32), np.array([1.0, np.nan], np.float32))


def test_layouts():
    t, n = er.as_rows(np.arange(65536), 7)
    assert t.shape == (1, 1, 9363, 7) and n == 65536 and (t.reshape(-1)[n:] == np.arange(5)).all()
    t, n = er.as_rows(np.arange(20), 7, odd_pixels=True)
    assert t.shape == (1, 1, 3, 7) and t.size % 2 == 1
    assert er.GRID_CAP == 524288
