"""GPU: the STORED half of every fp16 convolution entry is one round-to-nearest-even of its fp32 result, bit for bit (fp32
epilogue, one RNE store, subnormal halves kept, overflow from 65520).  tests/test_gpu_f16.py holds these kernels to max|diff| / max|ref| <= 1e-3
on U(-1,1) data -- a store that truncates, rounds twice, flushes subnormal halves or overflows at the wrong threshold passes it.  Here:

  A  the fp16 store against rne16 of the kernel's OWN fp32 store (accumulation order drops out) on wide-range data -- output channels spread
     over 2^31, so a few per cent of the outputs are subnormal halves and a few per cent overflow -- through every epilogue, every tile
     variant and every special kernel form; the fused pair / triple launches (no fp32 store) against the launches they replace on the same
     kind of data;
  B  operands built so that every partial sum is exact in fp32 in any order (tests/f16_reference.py, pinned by
     tests/test_f16_rounding_cpu.py): all 63488 finite halves through selector convs times 2^0 / 2^-6 / 2^-14 / 2^5, every tie between two
     halves with its fp32 neighbours, and the epilogue order in float32 -- the expected half is plain float64 / float32 arithmetic rounded
     once, and owes nothing to a kernel.

Every mismatch count a case measures is printed as an `f16 store:` line (`pytest -s`)."""
import contextlib

import numpy as np
import pytest

import f16_reference as fr
from containment import checked_dest
from util import assert_exact, rng_uniform

pytestmark = pytest.mark.gpu

SENTINEL = 0x7B
F16_TILES = [0, 1, 2, 3, 7, 9, 10, 11]      # tests/test_gpu_f16.py F16_TILES
POLICY = None                               # no plan: the kernel form the launcher's policy picks
F64, F32 = np.float64, np.float32


@pytest.fixture(scope="module")
def hops(gpu):
    from simpleinfer_amd import hipops
    return hipops


def under(hops, mode):
    """mode: POLICY, a tile variant, or a dict of SiConvPlan fields"""
    if mode is POLICY:
        return contextlib.nullcontext()
    return hops.plan(**(mode if isinstance(mode, dict) else {"f16_tile": mode}))


def mode_id(mode):
    if mode is POLICY:
        return "policy"
    return "tile%d" % mode if not isinstance(mode, dict) else "-".join("%s%d" % kv for kv in mode.items())


def record(line):
    print("f16 store: " + line)


def check_store(got16, v, what):
    fr.assert_f16_store(got16, v, what)
    record("%-90s 0 of %d mismatches" % (what, got16.size))


# =============================================================================================================================================
# A: the store is ONE nearest-even rounding of the kernel's own fp32 result, on wide-range data
# =============================================================================================================================================
ALL_MODES = [POLICY] + F16_TILES
WIDE_CASES = [
    # shape NHWC, oc, k, s, p, groups, modes, kernel the policy must reach with an fp16 store (prefix of its name)
    ((2, 9, 9, 64), 96, 1, 1, 0, 1, ALL_MODES, "conv_igemm_f16"),                        # ragged 32-wide column block, M not a tile multiple
    ((2, 9, 9, 40), 72, 1, 1, 0, 1, ALL_MODES, "conv_igemm_f16"),                        # zero-padded K
    ((2, 21, 19, 64), 96, 3, 2, 1, 1, ALL_MODES, "conv_igemm_f16"),                      # generic tiles, borders
    ((2, 14, 18, 32), 32, 3, 1, 1, 1, ALL_MODES + [{"f16_s2c32": 0}], "conv_c32_patch_f16_kernel"),
    ((2, 14, 18, 64), 64, 3, 1, 1, 1, ALL_MODES + [{"f16_s2c32": 0}], "conv_igemm_f16"),   # ragged: the 64-channel patch form takes whole tiles only ...
    ((2, 8, 16, 64), 64, 3, 1, 1, 1, [POLICY, 0, {"f16_s2c32": 0}], "conv_c32_patch_f16_kernel"),   # ... so once more on whole tiles
    ((2, 7, 9, 128), 128, 3, 1, 1, 1, ALL_MODES + [{"f16_slab": 0}, {"f16_slab_w2": 0}], "conv3x3s1_slab_f16_kernel"),
    ((2, 10, 10, 64), 64, 3, 1, 1, 2, ALL_MODES, "conv_igemm_f16"),                      # grouped, 32 channels per group
    ((2, 12, 12, 32), 32, 5, 1, 2, 1, ALL_MODES, "conv_igemm_f16"),                      # 25 taps
]
WIDE_PARAMS = [pytest.param(c[:6], m, c[7], id="%s-%dto%d-k%ds%dg%d-%s" % ("x".join(map(str, c[0][:3])), c[0][3], c[1], c[2], c[3], c[5], mode_id(m)))
               for c in WIDE_CASES for m in c[6]]
_WIDE = {}


def wide_data(orc, case):
    """operands and the float64 conv of one wide-range case: computed once, shared by the modes, never written"""
    if case not in _WIDE:
        shape, oc, k, s, p, g = case
        x, w, b = fr.wide_range_case(1000 + oc + k, shape, oc, k, g, bias=True)
        sc = (2.0 ** (-18 + np.arange(oc) % 32)).astype(F32)
        refs = {bias: orc.conv2d(x.astype(F32), w, b if bias else None, (s, s), (p, p), (1, 1), g, path="naive").astype(F64) for bias in (False, True)}
        oh, ow = refs[True].shape[1:3]
        r = (rng_uniform(1003 + oc + k, (shape[0], oh, ow, oc), -4, 4) * sc).astype(np.float16)     # the shortcut, scaled like its channel
        for a in (x, w, b, r) + tuple(refs.values()):
            a.setflags(write=False)
        _WIDE[case] = (x, w, b, r, refs)
    return _WIDE[case]


@pytest.mark.parametrize("case,mode,kernel", WIDE_PARAMS)
def test_store_is_one_rne_of_the_fp32_result_on_wide_range_data(hops, orc, case, mode, kernel):
    shape, oc, k, s, p, g = case
    x, w, b, r, refs = wide_data(orc, case)
    assert np.isfinite(w).all() and np.isfinite(r).all()
    geo = ((s, s), (p, p), (1, 1), g)
    epilogues = [("plain, no bias", None, {}), ("plain", b, {}), ("silu", b, {"act1": "silu"}), ("silu + residual", b, {"act1": "silu", "residual": r}),
                 ("residual + relu", None, {"residual": r, "act2": "relu"}), ("hardswish", b, {"act1": "hardswish"}),
                 ("leakyrelu 0.1", b, {"act1": "leakyrelu", "act_param": 0.1})]
    with under(hops, mode):
        for name, bias, kw in epilogues:
            what = "%s, %s, %s" % (case, mode_id(mode), name)
            got16 = hops.conv2d_f16(x, w, bias, *geo, **kw)
            if mode is POLICY and name == "plain":
                assert hops.LAST_KERNEL_NAME["si_hip_conv2d_f16"].startswith(kernel), hops.LAST_KERNEL_NAME["si_hip_conv2d_f16"]
            got32 = hops.conv2d_f16(x, w, bias, *geo, out_f32=True, **kw)
            assert got32.dtype == F32 and np.isfinite(got32).all(), what
            check_store(got16, got32, what)
            if name.startswith("plain"):
                ref = refs[bias is not None]
                # the classes are there: subnormal halves and overflows, each at least 1 % of the kernel's own values
                sub, inf = fr.class_shares(got32)
                record("%-90s subnormal %.4f inf %.4f" % (what, sub, inf))
                assert sub >= 0.01 and inf >= 0.01, (what, sub, inf)
                # the project's fp32-out bar, per output channel (each one is a convolution of its own; they differ by 2^31 here)
                cmax = np.abs(ref).reshape(-1, oc).max(0)
                err = (np.abs(got32.astype(F64) - ref).reshape(-1, oc).max(0) / cmax).max()
                assert err <= 2e-5, "%s: fp32 store, worst channel max|diff| / max|ref| = %.3e" % (what, err)
            if name == "silu":    # into a channel slice of a wider row
                wide = hops.conv2d_f16(x, w, bias, *geo, out_ld=oc + 32, out_c_off=16, out_fill=hops.ByteFill(SENTINEL), full=True, **kw)
                check_store(checked_dest(wide, 16, oc, SENTINEL, what), got32, what + ", strided")


def finite_halves(a, what):
    assert a.dtype == np.float16 and np.isfinite(a).all(), "%s: an intermediate overflowed -- the case needs other scales" % what
    return a


def assert_classes(want, what):
    sub, inf = float(fr.is_subnormal16(want).mean()), float(np.isinf(want).mean())
    record("%-90s subnormal %.4f inf %.4f" % (what, sub, inf))
    assert sub >= 0.01 and inf >= 0.01 and not np.isnan(want).any(), (what, sub, inf)


def test_bottleneck_pair_same_bits_on_wide_range_data(hops):
    """si_hip_conv2d_pw_slab_f16 (SiLU hard-coded, no fp32 store): bit identity with its two launches, now with an intermediate that holds
    subnormal halves and an output that also overflows"""
    c = 128
    x = rng_uniform(1, (2, 7, 9, c), -16, 16).astype(np.float16)
    w0, b0 = fr.scaled_weights(2, c, c, 1, fr.FUSED_MID_EXP, 0.15)
    w1, b1 = fr.scaled_weights(4, c, c, 3, fr.FUSED_OUT_EXP, 0.2)
    r =(rng_uniform(9, (2, 7, 9, c), -100, 100) * 2.0 ** (fr.FUSED_OUT_EXP + np.arange(c) % 32)).astype(np.float16)
    mid = finite_halves(hops.conv2d_f16(x, w0, b0, act1="silu"), "1x1")
    assert fr.is_subnormal16(mid).mean() >= 0.01
    want = hops.conv2d_f16(mid, w1, b1, (1, 1), (1, 1), act1="silu", residual=finite_halves(r, "shortcut"))
    assert_classes(want, "bottleneck pair")
    assert_exact(hops.conv_pw_slab_f16(x, w0, b0, w1, b1, residual=r).view(np.uint16), want.view(np.uint16), "fused bottleneck pair vs two launches, wide-range data")


def test_c3_tail_same_bits_on_wide_range_data(hops):
    """si_hip_conv2d_pw_cv3_f16: pair -> concat -> cv3 in one launch, on wide-range data (both intermediates finite)"""
    c = 64
    x = rng_uniform(11, (2, 8, 16, c), -16, 16).astype(np.float16)
    z = rng_uniform(12, (2, 8, 16, c), -16, 16).astype(np.float16)
    w0, b0 = fr.scaled_weights(13, c, c, 1, fr.FUSED_MID_EXP, 0.15)
    w1, b1 = fr.scaled_weights(15, c, c, 3, fr.FUSED_MID_EXP, 0.1)
    w3, b3 = fr.scaled_weights(17, 2 * c, 2 * c, 1, fr.FUSED_OUT_EXP, 0.15)
    mid = finite_halves(hops.conv2d_f16(x, w0, b0, act1="silu"), "1x1")
    assert fr.is_subnormal16(mid).mean() >= 0.01
    y = finite_halves(hops.conv2d_f16(mid, w1, b1, (1, 1), (1, 1), act1="silu", residual=x), "3x3")
    assert_exact(hops.conv_pw_slab_f16(x, w0, b0, w1, b1, residual=x).view(np.uint16), y.view(np.uint16), "64-channel pair vs two launches, wide-range data")
    want = hops.conv2d_f16(np.concatenate([y, z], -1), w3, b3, act1="silu")
    assert_classes(want, "C3 tail")
    got = hops.conv_pw_cv3_f16(x, w0, b0, w1, b1, z, w3, b3, residual=x)
    assert_exact(got.view(np.uint16), want.view(np.uint16), "pair + concat + cv3 vs the launches it replaces, wide-range data")


def test_stem_pair_and_triple_same_bits_on_wide_range_data(hops):
    """si_hip_conv2d_stem_s2c32_f16 and si_hip_conv2d_stem_s2c32_pw_f16 against the launches they replace, on wide-range data"""
    x = rng_uniform(21, (1, 20, 24, 3), -16, 16)
    w0, b0 = fr.scaled_weights(22, 32, 3, 6, fr.FUSED_MID_EXP, 0.3)
    mid = finite_halves(hops.conv2d_f16(x, w0, b0, (2, 2), (2, 2), act1="silu"), "stem")
    assert fr.is_subnormal16(mid).mean() >= 0.01
    # the pair: the 3x3 stores the result
    w1, b1 = fr.scaled_weights(24, 64, 32, 3, fr.FUSED_OUT_EXP, 0.3)
    want = hops.conv2d_f16(mid, w1, b1, (2, 2), (1, 1), act1="silu")
    assert_classes(want, "stem pair")
    assert_exact(hops.conv_stem_s2c32_f16(x, w0, b0, w1, b1).view(np.uint16), want.view(np.uint16), "fused stem + conv vs the two launches, wide-range data")
    # the triple: the 3x3's output is an intermediate too
    w1, b1 = fr.scaled_weights(24, 64, 32, 3, fr.FUSED_MID_EXP, 0.3)
    w2, b2 = fr.scaled_weights(26, 64, 64, 1, fr.FUSED_OUT_EXP, 0.3)
    mid2 = finite_halves(hops.conv2d_f16(mid, w1, b1, (2, 2), (1, 1), act1="silu"), "3x3")
    assert fr.is_subnormal16(mid2).mean() >= 0.01
    want = hops.conv2d_f16(mid2, w2, b2, act1="silu")
    assert_classes(want, "stem triple")
    ya, yb = hops.conv_stem_s2c32_pw_f16(x, w0, b0, w1, b1, w2, b2, split_oc=32, out2_ld=64, out2_c_off=32)
    assert_exact(np.concatenate([ya, yb], -1).view(np.uint16), want.view(np.uint16), "fused stem + conv + 1x1 vs the three launches, wide-range data")
    assert_exact(hops.conv_stem_s2c32_pw_f16(x, w0, b0, w1, b1, w2, b2, split_oc=0).view(np.uint16), want.view(np.uint16), "... one destination")


# =============================================================================================================================================
# B: exact by construction
# =============================================================================================================================================
def check_epilogue_order(hops, run, acc, oc, what):
    """run(bias, **kw) -> stored halves of a conv whose accumulators are exactly `acc` (float64, representable in fp32): bias and shortcut are
    added in fp32 in the documented order, the activations are exact, only the store rounds to fp16"""
    bias = rng_uniform(31, (oc,), -2, 2)                                       # random fp32: 24 significant bits
    res = np.resize(fr.all_finite_halves()[::-1], acc.shape)                   # every finite half as the shortcut, against the grain of the input
    for name, kw in (("bias", {}), ("bias + relu", {"act1": "relu"}), ("bias + leakyrelu", {"act1": "leakyrelu", "act_param": 0.1}),
                     ("bias + residual + relu", {"residual": res, "act2": "relu"})):
        want32 = fr.epilogue_ref32(acc, bias, kw.get("act1", "none"), kw.get("residual"), kw.get("act2", "none"), kw.get("act_param", 0.0))
        check_store(run(bias, **kw), want32, "%s, %s" % (what, name))


@pytest.mark.parametrize("mode", ALL_MODES, ids=mode_id)
@pytest.mark.parametrize("k", fr.SCALE_KS)
@pytest.mark.parametrize("ic", [32, 40])
def test_selector_1x1_every_finite_half(hops, ic, k, mode):
    """w = P 2^k: k = 0 returns every half unchanged (the 2046 subnormal ones too), -14 walks gradual underflow at the store, +5 the overflow
    threshold; ic 40: zero-padded K"""
    x = fr.halves_tensor((2, 31, 32, 32) if ic == 32 else (2, 31, 26, 40))
    src = fr.permutation(ic, 40 + ic)
    w, ty, tx = fr.selector_weights(ic, ic, 1, 1, k, src)
    want = fr.selector_expected(x, src, ty, tx, k)
    what = "selector 1x1 ic %d k %d %s" % (ic, k, mode_id(mode))
    with under(hops, mode):
        got32 = hops.conv2d_f16(x, w, None, out_f32=True)
        assert np.array_equal(got32.astype(F64), want), what + ": the fp32 accumulator of a single exact product is not that product"
        got = hops.conv2d_f16(x, w, None)
        check_store(got, want, what)
        if k == 0:
            assert_exact(got.view(np.uint16) & 0x7FFF, x[..., src].view(np.uint16) & 0x7FFF, what + ": identity")
            assert int(fr.is_subnormal16(got).sum()) >= 2046
        if k in (0, -6) and mode in (POLICY, 0, 3):
            check_epilogue_order(hops, lambda b, **kw: hops.conv2d_f16(x, w, b, **kw), want, ic, what)


@pytest.mark.parametrize("mode", ALL_MODES, ids=mode_id)
def test_every_tie_and_its_fp32_neighbours(hops, mode):
    """three terms per output, exact in fp32 in any order: the midpoint between x_a and the next half (to the EVEN one), and one fp32 ulp to
    either side of it (to the near one), for every mantissa of exponent -4 .. 14; no bias (an accumulator may start from it)"""
    x, w, y, terms, s = fr.tie_case()
    with under(hops, mode):
        got32 = hops.conv2d_f16(x, w, None, out_f32=True)
        assert np.array_equal(got32.astype(F64), y), "ties %s: the fp32 accumulators are not the exact sums" % mode_id(mode)
        got = hops.conv2d_f16(x, w, None)
    for sv, name in ((0, "ties"), (1, "one fp32 ulp above the tie"), (-1, "one fp32 ulp below the tie")):
        check_store(np.ascontiguousarray(got[..., s == sv]), y[..., s == sv], "%s, %s" % (name, mode_id(mode)))


SPATIAL_CASES = [
    # shape, oc, k, s, modes, kernel under the policy
    ((2, 31, 32, 32), 32, 3, 1, [POLICY, 0, 3, 7], "conv_c32_patch_f16_kernel"),
    ((2, 31, 32, 32), 32, 3, 2, [POLICY, 0, 3, 7], "conv_c32_patch_f16_kernel"),
    ((2, 31, 32, 32), 64, 3, 2, [POLICY, 0], "conv_c32_patch_f16_kernel"),
    ((2, 32, 16, 64), 64, 3, 1, [POLICY, 0, 3], "conv_c32_patch_f16_kernel"),      # the 64-channel patch form: whole 4 x 16 tiles
    ((2, 32, 32, 64), 128, 3, 2, [POLICY, 0, 10], "conv_c32_patch_f16_kernel"),    # 64 -> 128 at stride 2
    ((2, 31, 16, 64), 64, 3, 2, [POLICY, 1, 2], "conv_igemm_f16"),
    ((2, 31, 8, 128), 128, 3, 1, [POLICY, 0, 9, 11, {"f16_slab_w2": 0}], "conv3x3s1_slab_f16_kernel"),
    ((2, 31, 32, 32), 32, 5, 1, [POLICY, 0, 3], "conv_igemm_f16"),
    ((2, 31, 32, 32), 32, 5, 2, [POLICY, 0, 3], "conv_igemm_f16"),
]


@pytest.mark.parametrize("shape,oc,kk,s,mode,kernel", [pytest.param(c[0], c[1], c[2], c[3], m, c[5], id="%dto%d-k%ds%d-%s" % (c[0][3], c[1], c[2], c[3], mode_id(m)))
                                                       for c in SPATIAL_CASES for m in c[4]])
def test_selector_spatial_every_finite_half(hops, shape, oc, kk, s, mode, kernel):
    """one non-zero tap 2^k per output channel (tap o % (kh kw), source channel from a permutation): borders are exact zeros, interior taps
    exact copies, through the generic tiles, the patch kernel and the slab kernel"""
    ic, p = shape[3], kk // 2
    x = fr.halves_tensor(shape)
    src = fr.permutation(ic, 50 + ic)[np.arange(oc) % ic]
    for k in fr.SCALE_KS:
        w, ty, tx = fr.selector_weights(oc, ic, kk, kk, k, src)
        want = fr.selector_expected(x, src, ty, tx, k, s, p, kk, kk)
        what = "selector %dx%d s%d %d -> %d k %d %s" % (kk, kk, s, ic, oc, k, mode_id(mode))
        with under(hops, mode):
            got = hops.conv2d_f16(x, w, None, (s, s), (p, p))
            if mode is POLICY:
                assert hops.LAST_KERNEL_NAME["si_hip_conv2d_f16"].startswith(kernel), hops.LAST_KERNEL_NAME["si_hip_conv2d_f16"]
            check_store(got, want, what)
            if k == -6 and mode in (POLICY, 0):     # (the patch and slab kernels carry epilogues of their own)
                check_epilogue_order(hops, lambda b, **kw: hops.conv2d_f16(x, w, b, (s, s), (p, p), **kw), want, oc, what)


@pytest.mark.parametrize("c,kk,s", [(8, 3, 1), (72, 3, 1), (8, 3, 2), (72, 3, 2), (8, 5, 2), (72, 5, 2)])
def test_depthwise_selector_every_finite_half(hops, c, kk, s):
    """si_hip_conv2d_depthwise_f16 (fp32 weights, fma chain in tap order): one tap 2^k per channel; the fma of an exact product into exact
    zeros is exact"""
    x = fr.halves_tensor((2, 31, 128, 8) if c == 8 else (2, 21, 21, 72))
    p, src = kk // 2, np.arange(c)
    for k in fr.SCALE_KS:
        w, ty, tx = fr.selector_weights(c, 1, kk, kk, k, np.zeros(c, np.int64))
        want = fr.selector_expected(x, src, ty, tx, k, s, p, kk, kk)
        what = "depthwise %dx%d s%d c %d k %d" % (kk, kk, s, c, k)
        check_store(hops.conv2d_f16(x, w, None, (s, s), (p, p), (1, 1), c), want, what)
        if k in (0, -6):
            check_epilogue_order(hops, lambda b, **kw: hops.conv2d_f16(x, w, b, (s, s), (p, p), (1, 1), c, **kw), want, c, what)


@pytest.mark.parametrize("kk,p,oc,first", [(6, 2, 64, 0), (6, 2, 64, 44), (3, 1, 32, 0)])
def test_stem_selector_on_fp32_ties(hops, kk, p, oc, first):
    """si_hip_conv2d_stem_f16 reads the fp32 image and rounds it to fp16 in the kernel: the image holds every tie between two halves and the
    fp32 value on either side, so that conversion is on test too; over the cases every (tap, channel) pair has an output channel"""
    img = fr.stem_tie_image()
    x16 = fr.rne16(img)
    q = (first + np.arange(oc)) % (3 * kk * kk)
    taps, src = q % (kk * kk), q // (kk * kk)
    for k in (0, -14, 5):
        w, ty, tx = fr.selector_weights(oc, 3, kk, kk, k, src, taps)
        want = fr.selector_expected(x16, src, ty, tx, k, 2, p, kk, kk)
        check_store(hops.conv2d_f16(img, w, None, (2, 2), (p, p)), want, "stem %dx%d s2 k %d" % (kk, kk, k))


@pytest.mark.parametrize("k", [0, -14])
def test_split_and_upcat_selectors(hops, k):
    """si_hip_conv2d_split_f16 and si_hip_conv2d_upcat_f16: one selector case each"""
    x = fr.halves_tensor((2, 31, 32, 32))
    sa, sb = fr.permutation(32, 61), fr.permutation(32, 62)
    (wa, ty, tx), (wb, _, _) = fr.selector_weights(32, 32, 1, 1, k, sa), fr.selector_weights(32, 32, 1, 1, k, sb)
    zero = np.zeros(32, F32)
    ya, yb = hops.conv2d_split_f16(x, wa, zero, wb, zero)
    check_store(ya, fr.selector_expected(x, sa, ty, tx, k), "split, first sibling, k %d" % k)
    check_store(yb, fr.selector_expected(x, sb, ty, tx, k), "split, second sibling, k %d" % k)
    # cat(upsample(low), skip): 32 + 64 channels; the skip tensor holds every finite half, the low one every eighth
    skip = fr.halves_tensor((2, 32, 16, 64))
    low = np.resize(fr.all_finite_halves()[::8], (2, 16, 8, 32))
    cat = np.concatenate([low.repeat(2, axis=1).repeat(2, axis=2), skip], -1)
    src = fr.permutation(96, 63)
    w, ty, tx = fr.selector_weights(96, 96, 1, 1, k, src)
    got = hops.conv2d_upcat_f16(low, skip, w, np.zeros(96, F32), (2.0, 2.0), True)
    check_store(got, fr.selector_expected(cat, src, ty, tx, k), "upcat, k %d" % k)
