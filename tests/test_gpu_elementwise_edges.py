"""GPU: the elementwise kernels of ops.hip (fp32 and fp16 storage) against the float64 reference of tests/elementwise_reference.py (pinned on the CPU by
tests/test_elementwise_reference_cpu.py), where the round-1 tests of test_gpu_ops.py / test_gpu_f16.py never looked:

  B1  every fp16 kernel on all 65536 bit patterns, in a shape the 16-byte arm takes and in one it cannot take;
  B2  the fp32 unary / binary / scalar / activation kernels on non-finite and extreme values and on a sweep of each function's whole domain;
  B3  every capped launch with more than two passes of its grid-stride loop and a ragged last pass;
  B4  the dispatch arms of one entry (16-byte vectors / scalar / dense long row / channel-vector / general broadcast) against each other;
  B5  pools, batch norm and linear against float64 at their edges.

The bars (elementwise_reference.py states them): IEEE arithmetic is bit-exact in fp32, signs of zero included; library functions are within
4 fp32 ulp with NaN / inf classes matching; fp16 results equal the float64 reference rounded ONCE to fp16 for the functions made of correctly
rounded fp32 operations, and are within 1 fp16 ulp on at most 1% of the inputs for the others.  Every figure a test measures is printed as an
`edges:` line (`pytest -s` shows them): profiles/elementwise_edges_*.txt holds the lines of one run.
"""
import numpy as np
import pytest

import elementwise_reference as er
from containment import checked_dest
from util import assert_parity, rng_uniform

pytestmark = pytest.mark.gpu

SENTINEL = 0x7B            # 1.3e36 as fp32, 61280 as fp16: what a destination holds before the kernel runs, and what its gaps must still hold after
GRID_CAP = er.GRID_CAP     # 524288 = 2048 workgroups x 256 threads: the cap of si_grid_for (simpleinfer_amd/csrc/hip/si_hip_internal.h)
ACT_ABS = 2e-6             # test_gpu_ops.test_activations' absolute bar on the fp32 activations
F64 = np.float64

def record(line):
    print("edges: " + line)


@pytest.fixture(scope="module")
def hops(gpu):
    from simpleinfer_amd import hipops
    return hipops


def fill(hops):
    return hops.ByteFill(SENTINEL)


def both_arms(call, flats, cs=(8, 7), odd_pixels=False):
    """call(*tensors) on the flat value lists laid out with each channel count of `cs`; the results cut back to the lists' length.  All arms
    must agree bit for bit (NaN with NaN)"""
    outs = []
    for c in cs:
        ts = [er.as_rows(f, c, odd_pixels)[0] for f in flats]
        outs.append(np.asarray(call(*ts)).reshape(-1)[:np.asarray(flats[0]).size])
    for o in outs[1:]:
        er.assert_arms_agree(outs[0], o, "arms c = %s" % (cs,))
    return outs[0]


# =============================================================================================================================================
# B1: exhaustive fp16
# =============================================================================================================================================
HALVES = er.all_halves()
SLOPE = 0.1


def h_bar(exact):
    return (0, None) if exact else (1, er.H_MISMATCH_SHARE)


@pytest.mark.parametrize("kind", er.ACTIVATIONS)
def test_fp16_activation_all_patterns(hops, kind):
    got = both_arms(lambda t: hops.activation_f16(kind, t, SLOPE), [HALVES])
    ref = er.activation_ref(kind, HALVES.astype(F64), F64(np.float32(SLOPE)))
    bar = h_bar(kind in er.H_EXACT_ACT)
    d = er.half_ulp(got, ref)
    record("fp16 activation %-11s mismatches %5d of 65536, worst %d ulp (bar: %s)" % (kind, int((d > 0).sum()), int(d.max()), "equal" if not bar[0] else "1 ulp, 1%"))
    er.assert_half(got, ref, bar[0], kind, bar[1])


@pytest.mark.parametrize("op", range(18))
def test_fp16_unary_all_patterns(hops, op):
    got = both_arms(lambda t: hops.unary_op_f16(op, t), [HALVES])
    ref = er.unary_ref(op, HALVES.astype(F64))
    bar = h_bar(op in er.H_EXACT_UNARY)
    d = er.half_ulp(got, ref)
    record("fp16 unary %-10s mismatches %5d of 65536, worst %d ulp (bar: %s)" % (er.UNARY_NAMES[op], int((d > 0).sum()), int(d.max()), "equal" if not bar[0] else "1 ulp, 1%"))
    er.assert_half(got, ref, bar[0], er.UNARY_NAMES[op], bar[1])


def test_fp16_conversions_on_the_probe(hops):
    """fp32 -> fp16 is round-to-nearest-even on every tie between two halves, overflows to inf from 65520 on, keeps fp16 denormals (2^-25 is
    the tie that goes to 0, the next fp32 value goes to the smallest denormal) and keeps a NaN a NaN; fp16 -> fp32 is exact on every pattern"""
    p = er.convert_probe()
    with np.errstate(over="ignore"):
        want = p.astype(np.float16)
    for c in (8, 7):
        t, n = er.as_rows(p, c)
        half, back = hops.convert_roundtrip_f16(t)
        half, back = half.reshape(-1)[:n], back.reshape(-1)[:n]
        ok = er.same_bits_or_nan(half, want)
        assert ok.all(), "fp32 -> fp16 (c = %d): %d of %d differ, first %r -> %r, expected %r" % (c, int((~ok).sum()), n, p[~ok][0], half[~ok][0], want[~ok][0])
        assert (np.isnan(half) == np.isnan(p)).all()
        assert er.same_bits_or_nan(back, want.astype(np.float32)).all(), "fp16 -> fp32 (c = %d)" % c
    for c in (8, 7):                                                   # every pattern as the SOURCE of fp16 -> fp32, through an exact fp32 -> fp16
        t, n = er.as_rows(HALVES.astype(np.float32), c)
        half, back = hops.convert_roundtrip_f16(t)
        assert er.same_bits_or_nan(half.reshape(-1)[:n][~np.isnan(HALVES)], HALVES[~np.isnan(HALVES)]).all()
        assert er.same_bits_or_nan(back.reshape(-1)[:n], HALVES.astype(np.float32)).all()
    record("fp16 conversions        mismatches     0 of %d probe values and 65536 patterns (bar: equal)" % p.size)


@pytest.mark.parametrize("op,code", [("add", 0), ("mul", 2)])
def test_fp16_binary_all_patterns(hops, op, code):
    perm = np.random.Generator(np.random.Philox(7)).permutation(65536)
    for name, other in (("reversed", HALVES[::-1]), ("permuted", HALVES[perm])):
        got = both_arms(lambda a, b: hops.binary_same_f16(op, a, b), [HALVES, other])
        n, worst = er.assert_half(got, er.binary_ref(code, HALVES.astype(F64), other.astype(F64)), 0, "%s %s" % (op, name))
        record("fp16 binary %-3s %-9s mismatches %5d of 65536, worst %d ulp (bar: equal)" % (op, name, n, worst))
    r = np.random.Generator(np.random.Philox(8))
    a, s = HALVES[r.permutation(65536)].reshape(8, 1, 1024, 8), HALVES[r.integers(0, 65536, (8, 8))]
    s[0, :4] = np.array([np.inf, -np.inf, 0.0, -0.0], np.float16)
    got = hops.binary_bcast_f16(op, a, s)
    n, worst = er.assert_half(got, er.binary_ref(code, a.astype(F64), s.astype(F64)[:, None, None, :]), 0, op + " broadcast")
    record("fp16 binary %-3s broadcast mismatches %5d of 65536, worst %d ulp (bar: equal)" % (op, n, worst))


# =============================================================================================================================================
# B2: fp32 special values and wide domains
# =============================================================================================================================================
SPECIAL = er.special_f32()

# A device library function that misses 4 ulp on a stretch of its sweep: (lo, hi) of |x| taken out of that function's sweep, with the measured
# error in LAB_NOTEBOOK.md.  Empty: none does.
SWEEP_EXCLUDED = {}


def sweep(name):
    w = er.wide_sweep(name)
    if name in SWEEP_EXCLUDED:
        lo, hi = SWEEP_EXCLUDED[name]
        keep = ~((np.abs(w) >= lo) & (np.abs(w) <= hi))
        assert keep.mean() >= 0.95, "an exclusion may remove at most 5% of a sweep"
        w = w[keep]
    return w


@pytest.mark.parametrize("op", range(18))
def test_fp32_unary_special_and_sweep(hops, op):
    name = er.UNARY_NAMES[op]
    x = np.concatenate([SPECIAL, sweep(name)])
    got = both_arms(lambda t: hops.unary_op(op, t), [x])
    ref = er.unary_ref(op, x.astype(F64))
    if op in er.UNARY_EXACT:
        er.assert_bits32(got, ref, name)
        record("fp32 unary %-10s bit-exact on %d values" % (name, x.size))
    else:
        e = er.ulp32(got, ref)
        e[er.overflow_band(ref)] = 0
        record("fp32 unary %-10s worst %.2f ulp on %d values, %d in the overflow band" % (name, float(e.max()), x.size, int(er.overflow_band(ref).sum())))
        er.assert_ulp32(got, ref, 4, name, band=True)


@pytest.mark.parametrize("op", sorted(er.BINARY_NAMES))
def test_fp32_binary_special_grid(hops, op):
    a, b = [g.reshape(-1) for g in np.meshgrid(SPECIAL, SPECIAL, indexing="ij")]
    got = both_arms(lambda x, y: hops.binary_op(op, x, y), [a, b])
    ref = er.binary_ref(op, a.astype(F64), b.astype(F64))
    if op in er.BINARY_EXACT:
        er.assert_bits32(got, ref, er.BINARY_NAMES[op])
    else:
        worst, band = er.assert_ulp32(got, ref, 4, er.BINARY_NAMES[op], band=True)
        record("fp32 binary %-7s worst %.2f ulp on the %d x %d special grid, %d in the overflow band" % (er.BINARY_NAMES[op], worst, SPECIAL.size, SPECIAL.size, band))


@pytest.mark.parametrize("op", sorted(er.BINARY_NAMES))
def test_fp32_binary_scalar_special_and_sweep(hops, op):
    x = np.concatenate([SPECIAL, sweep("any")])
    for scalar in (2.5, 0.0, -0.0, np.inf, -np.inf, np.nan, -3.0):
        xs = x if scalar == 2.5 else SPECIAL
        got = both_arms(lambda t: hops.binary_scalar(op, t, scalar), [xs])
        ref = er.binary_ref(op, xs.astype(F64), F64(scalar))
        what = "%s with scalar %r" % (er.BINARY_NAMES[op], scalar)
        if op in er.BINARY_EXACT:
            er.assert_bits32(got, ref, what)
        else:
            e = er.ulp32(got, ref)
            e[er.overflow_band(ref)] = 0
            if scalar == 2.5:
                record("fp32 scalar %-7s worst %.2f ulp on %d values (scalar 2.5), %d in the overflow band" % (er.BINARY_NAMES[op], float(e.max()), xs.size, int(er.overflow_band(ref).sum())))
            er.assert_ulp32(got, ref, 4, what, band=True)


def assert_activation32(got, ref, what):
    """class for NaN and the infinities; |got - ref| <= 2e-6 + 4 * 2^-23 * |ref| on the rest"""
    er.assert_class(got, ref, what, np.float32)
    g, r = np.asarray(got, F64), np.asarray(ref, F64)
    fin = np.isfinite(g)
    excess = np.abs(g[fin] - r[fin]) - (ACT_ABS + 4 * er.F32_EPS * np.abs(r[fin]))
    assert (excess <= 0).all(), "%s: %d elements beyond 2e-6 + 4 ulp; worst excess %.3g" % (what, int((excess > 0).sum()), float(excess.max()))
    return float(np.abs(g[fin] - r[fin]).max()) if fin.any() else 0.0


@pytest.mark.parametrize("kind", er.ACTIVATIONS)
def test_fp32_activation_special_band_and_sweep(hops, kind):
    """through the dense long-row arm (c = 8 dense), the per-pixel 16-byte arm (c = 8 inside rows of 16) and the scalar arm (c = 7, an odd
    element count).  The band -104 .. -87: __expf(-x) overflows there and v_rcp_f32 meets (or returns) denormals; silu(-inf) is NaN as in torch"""
    x = np.concatenate([SPECIAL, er.sigmoid_band(), sweep("any")])
    ref = er.activation_ref(kind, x.astype(F64), F64(np.float32(SLOPE)))
    outs = []
    for c, views in ((8, {}), (8, dict(in_ld=16, in_c_off=8, out_ld=16, out_c_off=4)), (7, {})):
        t, n = er.as_rows(x, c, odd_pixels=True)
        outs.append(hops.activation(kind, t, SLOPE, **views).reshape(-1)[:n])
        er.assert_arms_agree(outs[0], outs[-1], "%s arm %d" % (kind, len(outs)))
    worst = assert_activation32(outs[0], ref, kind)
    band = np.abs(outs[0][SPECIAL.size:SPECIAL.size + er.sigmoid_band().size].astype(F64) - ref[SPECIAL.size:SPECIAL.size + er.sigmoid_band().size]).max()
    record("fp32 activation %-11s worst |diff| %.3g on %d values (in the band -104 .. -87: %.3g)" % (kind, worst, x.size, band))


# =============================================================================================================================================
# B3: more than two passes of the grid-stride loop, ragged last pass
# =============================================================================================================================================
V4 = (1, 1031, 1019, 4)      # 1050589 pixels: one 16-byte fp32 vector each (fp16: c = 8)
S3 = (1, 593, 593, 3)        # 351649 pixels x 3 = 1054947 scalar items (fp16: c = 7)


def items_ok(n):
    return n >= 2 * GRID_CAP + 1 and n % 256 != 0


def test_grid_stride_shapes_make_three_passes():
    assert items_ok(V4[1] * V4[2]) and items_ok(S3[1] * S3[2] * 3) and items_ok(S3[1] * S3[2] * 7) and items_ok(V4[1] * V4[2] * 4 // 4)
    assert (V4[1] * V4[2] * 4) % 4 == 0          # the dense long-row arm of activation needs total % 4 == 0


def gapped(hops, call, c, out_ld, out_c_off):
    """call(**views) with a sentinel-filled destination of rows of out_ld elements; the gap must still hold the sentinel (an overrun shows there),
    and an element the kernel skipped holds it inside the slice (it then fails the comparison with the expected values)"""
    full = call(out_ld=out_ld, out_c_off=out_c_off, out_fill=fill(hops), full=True)
    return checked_dest(full, out_c_off, c, SENTINEL, "destination rows")


def shape_c(shape, c):
    return shape[:3] + (c,)


# (name, vector-arm shape / views, scalar-arm shape / views): every arm gets a destination with a gap
ARMS32 = [("vector", V4, dict(out_ld=8, out_c_off=4)), ("scalar", S3, dict(out_ld=4, out_c_off=1))]
ARMS16 = [("vector", shape_c(V4, 8), dict(out_ld=16, out_c_off=8)), ("scalar", shape_c(S3, 7), dict(out_ld=8, out_c_off=1))]


@pytest.mark.parametrize("arm", ["dense", "vector", "scalar"])
def test_grid_stride_activation_f32(hops, arm):
    shape, views = {"dense": (V4, dict(out_ld=4, out_c_off=0)), "vector": ARMS32[0][1:], "scalar": ARMS32[1][1:]}[arm]
    x = rng_uniform(300, shape, -8, 8)
    got = gapped(hops, lambda **v: hops.activation("silu", x, **v), shape[3], **views)
    assert_activation32(got, er.activation_ref("silu", x.astype(F64)), "silu " + arm)


@pytest.mark.parametrize("arm,shape,views", ARMS16)
def test_grid_stride_activation_f16(hops, arm, shape, views):
    x = rng_uniform(301, shape, -8, 8).astype(np.float16)
    got = gapped(hops, lambda **v: hops.activation_f16("silu", x, **v), shape[3], **views)
    er.assert_half(got, er.activation_ref("silu", x.astype(F64)), 1, "silu " + arm, er.H_MISMATCH_SHARE)


@pytest.mark.parametrize("arm,shape,views", ARMS32)
def test_grid_stride_unary_f32(hops, arm, shape, views):
    x = rng_uniform(302, shape, -8, 8)
    px = shape[1] * shape[2]
    got = gapped(hops, lambda **v: hops.unary_op(4, x, **v).reshape(1, 1, px, -1), shape[3], **views)
    er.assert_bits32(got.reshape(shape), er.unary_ref(4, x.astype(F64)), "square " + arm)


@pytest.mark.parametrize("arm,shape,views", ARMS16)
def test_grid_stride_unary_f16(hops, arm, shape, views):
    x = rng_uniform(303, shape, -8, 8).astype(np.float16)
    px = shape[1] * shape[2]
    got = gapped(hops, lambda **v: hops.unary_op_f16(4, x, **v).reshape(1, 1, px, -1), shape[3], **views)
    er.assert_half(got.reshape(shape), er.unary_ref(4, x.astype(F64)), 0, "square " + arm)


@pytest.mark.parametrize("arm,shape,views", ARMS32)
def test_grid_stride_binary_same_and_scalar_f32(hops, arm, shape, views):
    a, b = rng_uniform(304, shape, -8, 8), rng_uniform(305, shape, -8, 8)
    got = gapped(hops, lambda **v: hops.binary_op(1, a, b, **v), shape[3], **views)
    er.assert_bits32(got, er.binary_ref(1, a.astype(F64), b.astype(F64)), "sub " + arm)
    got = gapped(hops, lambda **v: hops.binary_scalar(2, a, 1.75, **v), shape[3], **views)
    er.assert_bits32(got, er.binary_ref(2, a.astype(F64), 1.75), "mul scalar " + arm)


@pytest.mark.parametrize("arm,shape,views", ARMS16)
def test_grid_stride_binary_same_f16(hops, arm, shape, views):
    a, b = rng_uniform(306, shape, -8, 8).astype(np.float16), rng_uniform(307, shape, -8, 8).astype(np.float16)
    got = gapped(hops, lambda **v: hops.binary_same_f16("add", a, b, **v), shape[3], **views)
    er.assert_half(got, er.binary_ref(0, a.astype(F64), b.astype(F64)), 0, "add " + arm)


def test_grid_stride_binary_broadcast_f32(hops):
    """the per-image channel-vector kernel (aligned, c % 4 == 0) and the general broadcast kernel (c = 3)"""
    for (arm, shape, views) in ARMS32:
        a, b = rng_uniform(308, shape, -8, 8), rng_uniform(309, (1, 1, 1, shape[3]), 1, 2)
        got = gapped(hops, lambda **v: hops.binary_op(3, a, b, **v), shape[3], **views)
        er.assert_bits32(got, er.binary_ref(3, a.astype(F64), b.astype(F64)), "div broadcast " + arm)


def test_grid_stride_binary_broadcast_f16(hops):
    shape = (2, 1031, 511, 8)                     # 2 x 526841 pixels: the image index changes inside the second pass
    assert items_ok(shape[0] * shape[1] * shape[2])
    a, s = rng_uniform(310, shape, -8, 8).astype(np.float16), rng_uniform(311, (2, 8), -2, 2).astype(np.float16)
    got = gapped(hops, lambda **v: hops.binary_bcast_f16("mul", a, s, **v), 8, out_ld=16, out_c_off=8)
    er.assert_half(got, er.binary_ref(2, a.astype(F64), s.astype(F64)[:, None, None, :]), 0, "mul broadcast f16")


def test_grid_stride_batchnorm(hops):
    x = rng_uniform(312, S3, -8, 8)
    m, v, g, b = (rng_uniform(313 + i, (3,), lo, hi) for i, (lo, hi) in enumerate(((-1, 1), (0.5, 2), (-2, 2), (-1, 1))))
    got = gapped(hops, lambda **kw: hops.batchnorm2d(x, m, v, g, b, 1e-5, **kw), 3, out_ld=4, out_c_off=1)
    assert_parity(got, er.batchnorm_ref(x, m, v, g, b, 1e-5), 1e-5, "batchnorm")


@pytest.mark.parametrize("arm,shape,views", ARMS32)
def test_grid_stride_maxpool_f32(hops, arm, shape, views):
    x = rng_uniform(320, shape, -8, 8)
    got = gapped(hops, lambda **v: hops.maxpool2d(x, (3, 3), (1, 1), (1, 1), **v), shape[3], **views)
    assert np.array_equal(got, er.maxpool_ref(x, (3, 3), (1, 1), (1, 1), dtype=np.float32)), "maxpool " + arm


@pytest.mark.parametrize("arm,shape,views", ARMS16)
def test_grid_stride_maxpool_f16(hops, arm, shape, views):
    x = rng_uniform(321, shape, -8, 8).astype(np.float16)
    got = gapped(hops, lambda **v: hops.maxpool2d_f16(x, (3, 3), (1, 1), (1, 1), **v), shape[3], **views)
    assert np.array_equal(got, er.maxpool_ref(x, (3, 3), (1, 1), (1, 1), lowest=-er.H_MAX, dtype=np.float16)), "maxpool f16 " + arm


def test_grid_stride_avgpool(hops):
    x = rng_uniform(322, (1, 1186, 1186, 3), 0, 8)
    ref = er.avgpool_ref(x, (593, 593))
    got = gapped(hops, lambda **v: hops.adaptive_avgpool2d(x, (593, 593), **v), 3, out_ld=4, out_c_off=1)
    assert np.abs(got - ref).max() <= 1e-6 * np.abs(ref).max()
    xh = x.astype(np.float16)
    got = gapped(hops, lambda **v: hops.adaptive_avgpool2d_f16(xh, (593, 593), **v), 3, out_ld=4, out_c_off=1)
    er.assert_half(got, er.avgpool_ref(xh, (593, 593)), 1, "avgpool f16")


def test_grid_stride_upsample(hops):
    for (arm, shape, views) in ARMS32:
        oh, ow, c = shape[1:]
        x = rng_uniform(323, (1, (oh + 1) // 2, (ow + 1) // 2, c), -8, 8)
        got = gapped(hops, lambda **v: hops.upsample_nearest(x, 2.0, 2.0, out_hw=(oh, ow), **v), c, **views)
        assert np.array_equal(got, x[:, np.arange(oh) // 2][:, :, np.arange(ow) // 2]), "upsample " + arm


def test_grid_stride_copies(hops):
    for (arm, shape, views) in ARMS32:
        x = rng_uniform(324, shape, -8, 8)
        got = gapped(hops, lambda **v: hops.copy_channels(x, **v), shape[3], **views)
        assert np.array_equal(got, x), "copy_channels " + arm
    a, b = rng_uniform(325, S3, -8, 8), rng_uniform(326, S3, -8, 8)
    for axis in (1, 2):                           # cat_axis_kernel, one launch per operand, each of 1054947 items
        assert np.array_equal(hops.cat([a, b], axis, out_fill=fill(hops)), np.concatenate([a, b], axis)), "cat axis %d" % axis
    assert np.array_equal(hops.flatten_nhwc(a, out_fill=fill(hops)), a.transpose(0, 3, 1, 2).reshape(1, -1)), "flatten"


def test_grid_stride_conversions(hops):
    x = rng_uniform(327, S3, -70000, 70000)
    half, back = hops.convert_roundtrip_f16(x, out_ld=4, out_c_off=1, out_fill=fill(hops), full=True)
    half, back = checked_dest(half, 1, 3, SENTINEL, "fp16 rows"), checked_dest(back, 1, 3, SENTINEL, "fp32 rows")
    with np.errstate(over="ignore"):
        want = x.astype(np.float16)
    assert np.array_equal(half, want) and np.array_equal(back, want.astype(np.float32))


# =============================================================================================================================================
# B4: the arms of one entry agree
# =============================================================================================================================================
PIXELS = (1, 5, 257)
CHANNELS = (1, 3, 4, 5, 8, 12, 16)


def layouts(c, v):
    """dense; a slice that keeps 16-byte alignment (v elements per 16 bytes); a slice at an odd offset of rows of odd length"""
    up = -(-c // v) * v
    return [{}, dict(in_ld=up + v, in_c_off=v, out_ld=up + 2 * v, out_c_off=v), dict(in_ld=c + 3, in_c_off=1, out_ld=c + 5, out_c_off=3)]


def run_layouts(hops, call, x, v, c_out=None, b_views=False):
    """call(x, **views) in every layout -> the destination slices, the gaps checked; all bit-identical"""
    c = x.shape[-1]
    outs = []
    for views in layouts(c, v):
        views = dict(views)
        if b_views and "in_ld" in views:
            views.update(b_ld=views["in_ld"], b_c_off=views["in_c_off"])
        full = call(x, out_fill=fill(hops), in_fill=fill(hops), full=True, **views)
        full = full.reshape(-1, full.shape[-1])
        outs.append(checked_dest(full, views.get("out_c_off", 0), c_out or c, SENTINEL, "layout %s" % (views,)))
        er.assert_arms_agree(outs[0], outs[-1], "layout %s vs dense" % (views,))
    return outs[0]


def small(seed, px, c, lo=0.25, hi=4.0, dtype=np.float32):
    return rng_uniform(seed + 31 * px + c, (1, 1, px, c), lo, hi).astype(dtype)


@pytest.mark.parametrize("px", PIXELS)
def test_arms_agree_f32(hops, px):
    for c in CHANNELS:
        x, y = small(400, px, c, -4, 4), small(401, px, c)
        x64, y64 = x.reshape(-1, c).astype(F64), y.reshape(-1, c).astype(F64)
        for kind in ("silu", "relu", "hardswish"):
            assert_activation32(run_layouts(hops, lambda t, **v: hops.activation(kind, t, **v), x, 4), er.activation_ref(kind, x64), "%s c=%d" % (kind, c))
        er.assert_ulp32(run_layouts(hops, lambda t, **v: hops.unary_op(7, t, **v), x, 4), er.unary_ref(7, x64), 4, "exp c=%d" % c)
        er.assert_bits32(run_layouts(hops, lambda t, **v: hops.unary_op(5, t, **v), y, 4), er.unary_ref(5, y64), "sqrt c=%d" % c)
        er.assert_bits32(run_layouts(hops, lambda t, **v: hops.binary_scalar(8, t, 1.75, **v), y, 4), er.binary_ref(8, y64, 1.75), "1.75 / x c=%d" % c)
        er.assert_ulp32(run_layouts(hops, lambda t, **v: hops.binary_scalar(6, t, 2.5, **v), y, 4), er.binary_ref(6, y64, 2.5), 4, "x ** 2.5 c=%d" % c)
        er.assert_bits32(run_layouts(hops, lambda t, **v: hops.binary_op(3, t, y, **v), x, 4, b_views=True), er.binary_ref(3, x64, y64), "div c=%d" % c)
        er.assert_ulp32(run_layouts(hops, lambda t, **v: hops.binary_op(10, t, y, **v), x, 4, b_views=True), er.binary_ref(10, x64, y64), 4, "atan2 c=%d" % c)
        assert np.array_equal(run_layouts(hops, lambda t, **v: hops.copy_channels(t, **v), x, 4), x.reshape(-1, c))
        m, var, g, b = (rng_uniform(410 + i + c, (c,), lo, hi) for i, (lo, hi) in enumerate(((-1, 1), (0.5, 2), (-2, 2), (-1, 1))))
        assert_parity(run_layouts(hops, lambda t, **v: hops.batchnorm2d(t, m, var, g, b, 1e-5, **v), x, 4), er.batchnorm_ref(x64, m, var, g, b, 1e-5), 1e-5, "bn c=%d" % c)
        col = x.reshape(1, px, 1, c)             # pools and upsample want a map: px x 1
        got = run_layouts(hops, lambda t, **v: hops.maxpool2d(t, (3, 1), (1, 1), (1, 0), **v), col, 4)
        assert np.array_equal(got, er.maxpool_ref(col, (3, 1), (1, 1), (1, 0)).reshape(-1, c)), "maxpool c=%d" % c
        got = run_layouts(hops, lambda t, **v: hops.upsample_nearest(t, 2.0, 2.0, **v), col, 4)
        assert np.array_equal(got, np.repeat(np.repeat(col, 2, 1), 2, 2).reshape(-1, c)), "upsample c=%d" % c
        pos = y.reshape(1, px, 1, c)             # (positive: the bar is relative to max|ref|)
        got = run_layouts(hops, lambda t, **v: hops.adaptive_avgpool2d(t, (1, 1), **v), pos, 4)
        ref = er.avgpool_ref(pos, (1, 1)).reshape(-1, c)
        assert np.abs(got - ref).max() <= 1e-6 * np.abs(ref).max(), "global avgpool c=%d" % c


@pytest.mark.parametrize("px", PIXELS)
def test_arms_agree_f16(hops, px):
    for c in CHANNELS:
        x, y = small(420, px, c, -4, 4, np.float16), small(421, px, c, dtype=np.float16)
        x64, y64 = x.reshape(-1, c).astype(F64), y.reshape(-1, c).astype(F64)
        for kind in ("silu", "relu", "leakyrelu"):
            bar = h_bar(kind in er.H_EXACT_ACT)
            er.assert_half(run_layouts(hops, lambda t, **v: hops.activation_f16(kind, t, SLOPE, **v), x, 8), er.activation_ref(kind, x64, F64(np.float32(SLOPE))), bar[0], "%s c=%d" % (kind, c))
        er.assert_half(run_layouts(hops, lambda t, **v: hops.unary_op_f16(7, t, **v), x, 8), er.unary_ref(7, x64), 1, "exp c=%d" % c)
        er.assert_half(run_layouts(hops, lambda t, **v: hops.unary_op_f16(5, t, **v), y, 8), er.unary_ref(5, y64), 0, "sqrt c=%d" % c)
        er.assert_half(run_layouts(hops, lambda t, **v: hops.binary_same_f16("mul", t, y, **v), x, 8, b_views=True), er.binary_ref(2, x64, y64), 0, "mul c=%d" % c)
        col = x.reshape(1, px, 1, c)
        got = run_layouts(hops, lambda t, **v: hops.maxpool2d_f16(t, (3, 1), (1, 1), (1, 0), **v), col, 8)
        assert np.array_equal(got, er.maxpool_ref(col, (3, 1), (1, 1), (1, 0), lowest=-er.H_MAX, dtype=np.float16).reshape(-1, c)), "maxpool c=%d" % c
        er.assert_half(run_layouts(hops, lambda t, **v: hops.adaptive_avgpool2d_f16(t, (1, 1), **v), col, 8), er.avgpool_ref(col, (1, 1)).reshape(-1, c), 1, "global avgpool c=%d" % c)
        z = small(422, px, c, -70000, 70000)
        with np.errstate(over="ignore"):
            want = z.reshape(-1, c).astype(np.float16)
        for views in layouts(c, 4):
            half, back = hops.convert_roundtrip_f16(z, out_fill=fill(hops), in_fill=fill(hops), full=True, **views)
            off = views.get("out_c_off", 0)
            assert np.array_equal(checked_dest(half.reshape(-1, half.shape[-1]), off, c, SENTINEL, "fp16 rows"), want)
            assert np.array_equal(checked_dest(back.reshape(-1, back.shape[-1]), off, c, SENTINEL, "fp32 rows"), want.astype(np.float32))


@pytest.mark.parametrize("op", [0, 1, 2, 3, 6, 10])
def test_channel_vector_and_general_broadcast_agree(hops, op):
    """[N,H,W,C] (op) [N or 1,1,1,C] through binary_chan_kernel (everything 16-byte aligned, c % 4 == 0) and through binary_bcast_kernel (the
    vector behind an odd offset), in both operand orders: with the vector FIRST the channel-vector kernel applies the operand-reversed code
    (binary_op_reversed), which for sub / div / pow / atan2 must be the other function, not the same one"""
    rev = er.BINARY_REVERSED[op]
    for n, vn, hw, c in ((2, 2, (3, 5), 8), (2, 1, (3, 5), 4), (1, 1, (2, 2), 12), (3, 3, (7, 1), 16)):
        a, b = rng_uniform(430 + c, (n,) + hw + (c,), 0.25, 4), rng_uniform(431 + c, (vn, 1, 1, c), 0.25, 4)
        a64, b64 = a.astype(F64), b.astype(F64)
        broken = dict(b_ld=c + 3, b_c_off=1)
        for code in (op, rev):
            # a (code) b: the vector is the second operand
            fast, slow = hops.binary_op(code, a, b), hops.binary_op(code, a, b, **broken)
            er.assert_arms_agree(fast, slow, "%s, vector second" % er.BINARY_NAMES[code])
            # b (code) a: the vector is the first operand (a's views are then the vector's: in_ld / in_c_off)
            fast_r, slow_r = hops.binary_op(code, b, a, a.shape), hops.binary_op(code, b, a, a.shape, in_ld=c + 3, in_c_off=1)
            er.assert_arms_agree(fast_r, slow_r, "%s, vector first" % er.BINARY_NAMES[code])
            for got, ref, what in ((fast, er.binary_ref(code, a64, b64), "a op b"), (fast_r, er.binary_ref(code, b64, a64), "b op a")):
                if code in er.BINARY_EXACT:
                    er.assert_bits32(got, np.broadcast_to(ref, a.shape), "%s %s" % (er.BINARY_NAMES[code], what))
                else:
                    er.assert_ulp32(got, np.broadcast_to(ref, a.shape), 4, "%s %s" % (er.BINARY_NAMES[code], what))
        # x (op) y == y (reversed op) x, bit for bit
        er.assert_arms_agree(hops.binary_op(op, a, b), hops.binary_op(rev, b, a, a.shape), "%s against its reversed code" % er.BINARY_NAMES[op])


# =============================================================================================================================================
# B5: pools, batch norm and linear against float64
# =============================================================================================================================================
@pytest.mark.parametrize("half", [False, True])
def test_maxpool_infinities_and_floor(hops, half):
    """A window that holds +inf returns +inf.  A window that holds ONLY -inf returns the lowest FINITE value of the storage type (-FLT_MAX, or
    -65504 with fp16 storage): the reference starts its running maximum at numeric_limits::lowest(), the oracle restates that, and so do the
    kernels -- the rule is the reference's, not IEEE's.  All-negative data with padding: a padded tap never wins.  NaN is left out of pool
    inputs on purpose: v_max drops a NaN operand, the reference's comparison keeps whichever came first, and no model feeds a pool NaN."""
    dt, lowest = (np.float16, -er.H_MAX) if half else (np.float32, -er.FLT_MAX)
    fn = hops.maxpool2d_f16 if half else hops.maxpool2d
    for c in (8, 16, 7, 3):
        x = rng_uniform(500 + c, (2, 9, 11, c), -9, -1).astype(dt)
        x[0, 2:7, 3:9, 0] = -np.inf                 # 5 x 6 block: 3 x 3 windows wholly inside it
        x[1, :3, :3, c - 1] = -np.inf               # a corner: the padded taps do not count either
        x[0, 4, 4, 1] = x[1, 8, 10, 2] = np.inf
        x[1, 5, 5, 0] = lowest                      # the floor itself as data
        for k, s, p in (((3, 3), (1, 1), (1, 1)), ((2, 2), (2, 2), (0, 0)), ((5, 5), (1, 1), (2, 2)), ((3, 3), (2, 2), (1, 1))):
            got = fn(x, k, s, p)
            ref = er.maxpool_ref(x, k, s, p, lowest=lowest)
            assert np.array_equal(got.astype(F64), ref), "maxpool k%s s%s p%s c=%d" % (k, s, p, c)
            if k == (3, 3) and s == (1, 1):
                assert got[0, 4, 5, 0] == dt(lowest) and got[1, 0, 0, c - 1] == dt(lowest) and np.isposinf(got[0, 3:6, 3:6, 1].astype(F64)).all()
            assert (got.astype(F64)[np.isfinite(ref)] < 0).all(), "all-negative data: a padded tap won"
    if half:                                         # every non-NaN pattern as pool data
        v = HALVES[~np.isnan(HALVES)]
        x = v[np.random.Generator(np.random.Philox(9)).permutation(v.size)][:63488].reshape(1, 32, 248, 8)
        assert np.array_equal(fn(x, (3, 3), (1, 1), (1, 1)).astype(F64), er.maxpool_ref(x, (3, 3), (1, 1), (1, 1), lowest=lowest))


AVG_MAPS = [((1, 1), [(1, 1)]), ((2, 3), [(1, 1), (2, 3), (1, 3)]), ((7, 7), [(1, 1), (7, 7)]), ((56, 56), [(1, 1), (28, 28), (8, 8)])]


@pytest.mark.parametrize("c", [1, 3, 8, 9, 100])
def test_avgpool_f32_vs_float64(hops, c):
    for (h, w), outs in AVG_MAPS:
        # (positive data: the bar is relative to max|ref|, which a mean of zero-centred data would leave near 0); the second: mean 1000, spread 1e-2
        for seed, lo, hi in ((510, 0.0, 2.0), (511, 1000 - 1e-2, 1000 + 1e-2)):
            x = rng_uniform(seed + c, (2, h, w, c), lo, hi)
            for out_hw in outs:
                got, ref = hops.adaptive_avgpool2d(x, out_hw), er.avgpool_ref(x, out_hw)
                e = np.abs(got - ref).max() / np.abs(ref).max()
                assert e <= 1e-6, "avgpool %dx%d -> %s c=%d [%g, %g): %.3g" % (h, w, out_hw, c, lo, hi, e)


@pytest.mark.parametrize("c", [1, 3, 8, 9, 100])
def test_avgpool_f16_vs_float64(hops, c):
    """within 1 fp16 ulp of the float64 mean rounded to fp16 -- also at +-65504, where the mean is an fp16 value and the fp32 sum is not"""
    worst = 0
    for (h, w), outs in AVG_MAPS:
        x = rng_uniform(520 + c, (2, h, w, c), -2, 2).astype(np.float16)
        big = np.full((2, h, w, c), 65504.0, np.float16)
        big[1] = -big[1]
        mixed = np.where(rng_uniform(521 + c, (2, h, w, c)) < 0.5, np.float16(65504), np.float16(-65504))
        for t in (x, big, mixed):
            for out_hw in outs:
                n, u = er.assert_half(hops.adaptive_avgpool2d_f16(t, out_hw), er.avgpool_ref(t, out_hw), 1, "avgpool f16 %dx%d -> %s c=%d" % (h, w, out_hw, c))
                worst = max(worst, u)
    record("fp16 avgpool c=%-3d worst %d ulp" % (c, worst))


@pytest.mark.parametrize("c", [1, 5, 8])
def test_batchnorm_edges_vs_float64(hops, c):
    x = rng_uniform(530 + c, (2, 5, 7, c), -3, 3)
    m, b = rng_uniform(531 + c, (c,), -1, 1), rng_uniform(532 + c, (c,), -1, 1)
    for var in (0.0, 1e-12, 1e6):
        for gamma in (rng_uniform(533 + c, (c,), 0.5, 2), np.zeros(c, np.float32), -rng_uniform(534 + c, (c,), 0.5, 2)):
            v = np.full(c, var, np.float32)
            got = hops.batchnorm2d(x, m, v, gamma, b, 1e-5)
            assert_parity(got, er.batchnorm_ref(x, m, v, gamma, b, 1e-5), 1e-5, "batchnorm c=%d var=%g gamma[0]=%g" % (c, var, gamma[0]))


@pytest.mark.parametrize("in_f", [1, 63, 64, 65, 129, 2048])
def test_linear_vs_float64(hops, in_f):
    for out_f in (1, 7, 1000):
        for rows in (1, 3):
            x, w, b = rng_uniform(540 + in_f, (rows, in_f), -1, 1), rng_uniform(541 + out_f, (out_f, in_f), -1, 1), rng_uniform(542, (out_f,), -1, 1)
            for bias in (b, None):
                assert_parity(hops.linear(x, w, bias), er.linear_ref(x, w, bias), what="linear %dx%d -> %d %s" % (rows, in_f, out_f, "bias" if bias is not None else "no bias"))
