"""CPU: the yardstick of tests/test_gpu_f16_rounding.py is itself on test here -- rne16 against an integer model of binary16 on every tie,
the bit-compare helper, the element-wise bound, and every exact-by-construction builder: each partial sum representable in fp32 (so the
expected half owes nothing to a kernel's accumulation order) and the value classes (subnormal, inf, tie) the GPU cases rely on."""
import numpy as np
import pytest

import f16_reference as fr

F64, F32 = np.float64, np.float32


def test_all_finite_halves():
    hv = fr.all_finite_halves()
    assert hv.size == 63488 and np.isfinite(hv).all() and len(np.unique(hv.view(np.uint16))) == 63488
    assert int(fr.is_subnormal16(hv).sum()) == 2046
    assert int((hv == 0).sum()) == 2
    t = fr.halves_tensor((2, 32, 16, 64))
    assert len(np.unique(t.view(np.uint16))) == 63488
    with pytest.raises(AssertionError):
        fr.halves_tensor((2, 31, 32, 31))


def test_rne16_is_the_integer_model_on_every_tie_and_its_neighbours():
    pos = np.unique(np.abs(fr.all_finite_halves().astype(F64)))    # (one zero)
    pos = np.concatenate([pos, [65536.0]])         # the half that would follow 65504: its midpoint, 65520, is the overflow threshold
    mid = (pos[:-1] + pos[1:]) / 2
    assert mid.size == 31744 and mid[-1] == 65520.0
    mid32 = mid.astype(F32)
    assert np.array_equal(mid32.astype(F64), mid)
    v = np.concatenate([mid32, np.nextafter(mid32, F32(0)), np.nextafter(mid32, F32(np.inf)),
                        np.array([65504.0, 65519.99, 65520.0, 2.0 ** -25, np.nextafter(F32(2.0 ** -25), F32(1)), 0.0, 2.0 ** -24, 2.0 ** -14, 1e-30, 3e38], F32)])
    v = np.concatenate([v, -v])
    want = fr.rne16_model_bits(v)
    assert np.array_equal(fr.rne16(v).view(np.uint16), want)                  # from float32
    assert np.array_equal(fr.rne16(v.astype(F64)).view(np.uint16), want)      # from float64: one rounding, not two
    # the ties go to the even neighbour, their fp32 neighbours to the near one
    lo, hi = fr.rne16(pos[:-1]).view(np.uint16), fr.rne16(pos[:-1]).view(np.uint16) + 1
    even = np.where(lo % 2 == 0, lo, hi)
    assert np.array_equal(want[:31744], even)
    assert np.array_equal(want[31744:2 * 31744], lo) and np.array_equal(want[2 * 31744:3 * 31744], hi)
    assert want[31743] == 0x7C00 and want[2 * 31744 - 1] == 0x7BFF             # 65520 -> inf, the fp32 below it -> 65504
    named = dict(zip([65504.0, 65519.99, 65520.0], fr.rne16(np.array([65504.0, 65519.99, 65520.0], F32)).view(np.uint16)))
    assert named == {65504.0: 0x7BFF, 65519.99: 0x7BFF, 65520.0: 0x7C00}
    tiny = np.array([2.0 ** -25, np.nextafter(F32(2.0 ** -25), F32(1))], F32)
    assert list(fr.rne16(tiny).view(np.uint16)) == [0, 1]                      # the tie under the smallest subnormal goes to (even) zero
    # every finite half is a fixed point of the model
    hv = fr.all_finite_halves()
    assert np.array_equal(fr.rne16_model_bits(hv.astype(F64)), hv.view(np.uint16))


def test_a_double_rounding_differs_from_rne16():
    """what the helper must be able to tell apart: float64 -> float32 -> fp16 is not float64 -> fp16"""
    v = 1.0 + 2.0 ** -11 + 2.0 ** -30
    assert fr.rne16(F64(v)).view(np.uint16) == 0x3C01 and F32(v).astype(np.float16).view(np.uint16) == 0x3C00


def test_assert_f16_store():
    v = np.array([1.0, 1.0 + 2.0 ** -11, -(1.0 + 3 * 2.0 ** -11), 65520.0, 2.0 ** -25, -2.0 ** -26, 3e-6, 0.0], F32)
    good = fr.rne16(v)
    fr.assert_f16_store(good, v, "rne")
    zeros = good.copy()
    zeros.view(np.uint16)[[4, 5, 7]] ^= 0x8000
    fr.assert_f16_store(zeros, v, "+0 and -0 are one class")
    for i, bits, why in ((1, 0x3C01, "tie rounded up"), (2, 0xBC01, "tie rounded toward zero"), (3, 0x7BFF, "no overflow at 65520"),
                         (6, 0x0000, "flushed subnormal"), (0, 0x3C01, "one ulp off")):
        bad = good.copy()
        bad.view(np.uint16)[i] = bits
        with pytest.raises(AssertionError) as ei:
            fr.assert_f16_store(bad, v, why)
        msg = str(ei.value)
        assert "1 of 8" in msg and "flat index %d" % i in msg and "0x%04x" % bits in msg and "0x%04x" % int(good.view(np.uint16)[i]) in msg
    with pytest.raises(AssertionError):
        fr.assert_f16_store(good.astype(F32), v, "dtype")


def test_f16_bound_terms():
    ref = np.array([0.0, 1.0, -1000.0, 3e-6], F64)
    a = 2e-5 * 1000.0
    b = fr.f16_bound(ref, a)
    assert np.array_equal(b, a + 2.0 ** -11 * (np.abs(ref) + a) + 2.0 ** -22 * np.abs(ref) + 2.0 ** -25)
    # an exact fp32 result (a = 0) stored with one nearest-even rounding is inside, one half ulp further is outside
    x = np.array([1.0 + 2.0 ** -11, 3.0 * 2.0 ** -25, 1000.3], F64)
    assert (np.abs(fr.rne16(x).astype(F64) - x) <= fr.f16_bound(x, 0.0)).all()
    assert np.abs(np.float16(1.0 + 2.0 ** -9) - x[0]) > fr.f16_bound(x[0], 0.0)
    # ... and the old bar is far wider at a typical element: max|ref| * 1e-3 against the bound at |ref| = 1
    assert fr.f16_bound(1.0, a) < 0.05 * 1e-3 * 1000.0
    fr.assert_f16_elementwise(fr.rne16(x), x, 0.0, "exact")
    with pytest.raises(AssertionError):
        fr.assert_f16_elementwise(np.array([1.0 + 2.0 ** -9, 0, 1000.5], np.float16), x, 0.0, "off")


@pytest.mark.parametrize("k", fr.SCALE_KS)
def test_scale_cases_value_classes(k):
    """x * 2^k over all finite halves: the product is exact in fp32 (the accumulator of a selector conv), and the classes of its rounding are
    the ones the GPU selector cases walk"""
    x = fr.all_finite_halves().astype(F64)
    y = x * 2.0 ** k
    assert fr.partial_sums_exact(y[:, None])
    r = fr.rne16(y)
    assert np.array_equal(r.view(np.uint16), fr.rne16_model_bits(y))
    with np.errstate(invalid="ignore"):
        inexact = r.astype(F64) != y
    got = (int(fr.is_subnormal16(r).sum()), int(inexact.sum()), int((r == 0).sum()), int(np.isinf(r).sum()))
    assert got == fr.SCALE_CLASSES[k]
    if k == 0:
        assert np.array_equal(r.view(np.uint16), fr.all_finite_halves().view(np.uint16))


def test_selector_builders():
    x = fr.halves_tensor((2, 31, 32, 32))
    for kh, s in ((1, 1), (3, 1), (3, 2), (5, 2)):
        src = fr.permutation(32, 5)
        w, ty, tx = fr.selector_weights(32, 32, kh, kh, -6, src)
        assert int((w != 0).sum()) == 32 and set(np.unique(w)) == {0.0, 2.0 ** -6}
        assert np.array_equal(w.astype(np.float16).astype(F32), w)
        assert sorted(np.flatnonzero(w.reshape(32, -1))) == sorted(np.arange(32) * 32 * kh * kh + src * kh * kh + ty * kh + tx)
        want = fr.selector_expected(x, src, ty, tx, -6, s, kh // 2, kh, kh)
        assert fr.partial_sums_exact(want[..., None])
        # the same conv in plain float64 loops over a corner of the output
        p = kh // 2
        xp = np.pad(x.astype(F64), ((0, 0), (p, p), (p, p), (0, 0)))
        for (n, oy, ox) in ((0, 0, 0), (1, want.shape[1] - 1, want.shape[2] - 1), (1, 3, 2)):
            patch = xp[n, oy * s:oy * s + kh, ox * s:ox * s + kh, :]                 # [kh, kw, ic]
            assert np.array_equal(np.einsum("yxc,ocyx->o", patch, w.astype(F64)), want[n, oy, ox])
    # borders of a padded selector are exact zeros
    src = np.arange(32)
    w, ty, tx = fr.selector_weights(32, 32, 3, 3, 0, src)
    want = fr.selector_expected(np.ones((1, 4, 4, 32), np.float16), src, ty, tx, 0, 1, 1, 3, 3)
    assert (want[0, 0, :, ty == 0] == 0).all() and (want[0, :, 0, tx == 0] == 0).all() and (want[0, 1:3, 1:3] == 1).all()


def test_tie_case_is_exact_and_every_expected_value_is_the_documented_neighbour():
    x, w, y, terms, s = fr.tie_case()
    assert x.shape == (2, 19, 128, 32) and x.dtype == np.float16 and w.shape == (24, 32, 1, 1)
    assert np.array_equal(w.astype(np.float16).astype(F32), w) and np.isfinite(x).all()
    assert not fr.is_subnormal16(x[..., :24]).any()
    assert fr.partial_sums_exact(terms)
    # the float64 sums are the conv of x and w
    assert np.array_equal(np.einsum("nhwc,oc->nhwo", x.astype(F64), w[:, :, 0, 0].astype(F64)), y)
    xa = np.stack([x[..., 3 * (o // 3)] for o in range(24)], -1)
    lo = xa.view(np.uint16).astype(np.int64)               # same sign, magnitude one step up = bits + 1 (exponent <= 14: never reaches inf)
    r = fr.rne16(y).view(np.uint16).astype(np.int64)
    assert np.array_equal(r, fr.rne16_model_bits(y).astype(np.int64))
    for o in range(24):
        if s[o] == 0:      # exact midpoints: 38912 ties in all, to the even neighbour
            assert np.array_equal(y[..., o], (xa[..., o].astype(F64) + (lo[..., o] + 1).astype(np.uint16).view(np.float16).astype(F64)) / 2)
            assert np.array_equal(r[..., o], np.where(lo[..., o] % 2 == 0, lo[..., o], lo[..., o] + 1))
        else:
            assert np.array_equal(r[..., o], lo[..., o] + (1 if s[o] > 0 else 0))
    ties = sum(int(np.prod(y.shape[:3])) for o in range(24) if s[o] == 0)
    assert ties == 38912
    up = int((r[..., s == 0] != lo[..., s == 0]).sum())
    assert up == 38912 // 2                                  # half of the ties go up, half down: a fixed direction fails one of them


def test_stem_tie_image():
    img = fr.stem_tie_image()
    assert img.dtype == F32 and img.shape == (2, 126, 252, 3) and np.abs(img).max() < 65520
    r = fr.rne16(img)
    assert np.isfinite(r).all()
    assert np.array_equal(r.view(np.uint16), fr.rne16_model_bits(img))
    exact = r.astype(F32) == img
    assert not exact.any()                                   # every pixel is rounded by the kernel's conversion
    d = np.abs(r.astype(F64) - img.astype(F64))
    b = r.view(np.uint16) & 0x7FFF
    ulp = np.where(b < 0x0400, 2.0 ** -24, 2.0 ** (((b >> 10) & 31).astype(F64) - 25))
    # a third of the values are exact ties (distance = half an ulp of the LOWER neighbour's binade), counted on the distinct values
    v = np.unique(img)
    rv = fr.rne16(v).astype(F64)
    with np.errstate(over="ignore"):
        nxt = np.nextafter(fr.rne16(v), np.float16(np.inf)).astype(F64)
        prv = np.nextafter(fr.rne16(v), np.float16(-np.inf)).astype(F64)
    tie = (np.abs(v - rv) == np.abs(v - nxt)) | (np.abs(v - rv) == np.abs(v - prv))
    assert int(tie.sum()) == 2 * 31743
    assert (d <= ulp).all()
    # products with the selector's 2^k are exact in fp32
    for k in (0, -14, 5):
        assert fr.partial_sums_exact((r.astype(F64) * 2.0 ** k)[..., None])


def test_epilogue_reference_rounds_in_fp32_and_only_the_store_in_fp16():
    acc = np.array([1.0, 2049.0 * 2.0 ** -11, -3.0, 2.0 ** -20], F64)
    bias = np.array([2.0 ** -24 + 2.0 ** -1, 0.0, 1.0, 0.0], F32)
    v = fr.epilogue_ref32(acc, bias)
    assert v.dtype == F32 and v[0] == F32(1.5)               # 1 + (0.5 + 2^-24): the fp32 add rounds (to even), float64 would not
    assert np.array_equal(fr.epilogue_ref32(acc, bias, "relu"), np.maximum(v, 0))
    lr = fr.epilogue_ref32(acc, bias, "leakyrelu", p=0.1)
    assert lr[2] == F32(-2.0) * F32(0.1) and lr[0] == v[0]
    res = np.array([1.0, -4.0, 0.5, 0.0], np.float16)
    assert np.array_equal(fr.epilogue_ref32(acc, bias, residual=res, act2="relu"), np.maximum(v + res.astype(F32), 0))
    with pytest.raises(AssertionError):
        fr.epilogue_ref32(np.array([1.0 + 2.0 ** -30]), None)


WIDE_SHAPES = [((2, 9, 9, 64), 96, 1, 1, 0, 1), ((2, 9, 9, 40), 72, 1, 1, 0, 1), ((2, 21, 19, 64), 96, 3, 2, 1, 1), ((2, 14, 18, 32), 32, 3, 1, 1, 1),
               ((2, 14, 18, 64), 64, 3, 1, 1, 1), ((2, 7, 9, 128), 128, 3, 1, 1, 1), ((2, 10, 10, 64), 64, 3, 1, 1, 2), ((2, 12, 12, 32), 32, 5, 1, 2, 1)]


@pytest.mark.parametrize("shape,oc,k,s,p,g", WIDE_SHAPES)
@pytest.mark.parametrize("bias", [False, True])
def test_wide_range_data_has_the_value_classes(orc, shape, oc, k, s, p, g, bias):
    """the float64 conv of the wide-range operands: at least 1 % subnormal halves and 1 % overflows among its outputs at every shape of the GPU
    file (which asserts the same on the kernel's own fp32 store), finite weights, a share of them subnormal halves"""
    x, w, b = fr.wide_range_case(1000 + oc + k, shape, oc, k, g, bias)
    assert x.dtype == np.float16 and np.isfinite(w).all() and np.array_equal(w.astype(np.float16).astype(F32), w)
    assert fr.is_subnormal16(w).mean() > 0.15
    ref = orc.conv2d(x.astype(F32), w, b, (s, s), (p, p), (1, 1), g, path="naive")
    sub, inf = fr.class_shares(ref)
    print("wide-range shares: subnormal %.4f inf %.4f" % (sub, inf))
    assert sub >= 0.0125 and inf >= 0.0125, (sub, inf)       # (a quarter above the 1 % the GPU test asks of the kernel's own values: the two differ only within 2e-5 of a class border)


def test_scaled_weights_of_the_fused_launch_cases():
    for lo in (fr.FUSED_MID_EXP, fr.FUSED_OUT_EXP):
        w, b = fr.scaled_weights(2, 128, 128, 1, lo, 0.15)
        assert w.shape == (128, 128, 1, 1) and b.shape == (128,) and b.dtype == F32
        assert np.isfinite(w).all() and np.array_equal(w.astype(np.float16).astype(F32), w)
        top, sc = np.abs(w).reshape(128, -1).max(1), 2.0 ** (lo + np.arange(128) % 32)
        assert (top <= 0.15 * sc * (1 + 2.0 ** -10) + 2.0 ** -25).all()      # (one rounding to a half: the smallest channels are subnormal or zero)
        assert (top[sc >= 2.0 ** -14] >= 0.1 * sc[sc >= 2.0 ** -14]).all()
        assert (np.abs(b) <= 0.5 * sc).all()
    # a 128-channel 1x1 over |x| <= 16 with the intermediate scale cannot overflow a half, whatever the signs
    assert 128 * 16 * 0.15 * 2.0 ** (fr.FUSED_MID_EXP + 31) + 0.5 * 2.0 ** (fr.FUSED_MID_EXP + 31) < 65504
