"""GPU: rectangular kernels, strides, pads and dilations through every convolution family and the max pool, against torch float64
(tests/rect_reference.py).  Until this file every conv / depthwise / stem / fp16 / split / pool test passed (k, k), (s, s), (p, p), (d, d): a
swapped kh / kw, sh / sw, pt / pl or dh / dw anywhere in the kernels or their predicates would have passed the whole suite.

Per case: parity with the float64 reference at the project's "vs fp64" bar (2e-5 of max|ref|, plus the element-wise metric of
util.assert_parity); for the implicit-GEMM kernels bit equality with the oracle's fma chain (a tolerance turned into an equality: one wrong
border tap cannot hide), over every tile for the fast path; the kernel family the launch reports; batch invariance bit for bit.  Once per family
the fused epilogue and a strided view.  Every case has its twin with all axes swapped in the table.

Bars (none new): fp32 conv 2e-5 vs float64, the fused epilogue included (SiLU through the hardware's exp / rcp is good to about 1e-6 of its
argument: measured 7.5e-7 at worst); fp16 operands with fp32 out 2e-5, fp16 out F16_TOL; f32_split 2e-5; max and the chain: equality of bits."""
import ctypes as C

import numpy as np
import pytest

import rect_reference as rr
import util
from containment import checked_dest
from test_gpu_f16 import F16_TILES, F16_TOL, h
from test_gpu_tiles import ALL_TILES
from util import assert_exact, assert_parity

pytestmark = pytest.mark.gpu

SENTINEL = 0x7B
CONV_ENTRY = "si_hip_conv2d_f32"
_REF = {}   # case id -> (x, w, b, float64 reference): computed once, shared, never written


@pytest.fixture(scope="module")
def hops(gpu):
    from simpleinfer_amd import hipops
    yield hipops
    hipops.set_plan()


def case_ref(c):
    cid = rr.case_id(c)
    if cid not in _REF:
        x, w, b = rr.operands(c)
        ref = rr.conv2d_f64(x, w, b, c.s, c.p, c.d, c.g)
        for a in (x, w, b, ref):
            a.setflags(write=False)
        _REF[cid] = (x, w, b, ref)
    return _REF[cid]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint16)


def report(what, got, ref):
    print("%-90s max-based %.3e  element-wise %.3e" % (what, util.rel_err(got, ref), util.mixed_err(got, ref)))


def check_case(hops, orc, c, chain):
    """parity, family reached, the fma chain (implicit GEMM), batch invariance"""
    x, w, b, ref = case_ref(c)
    got = hops.conv2d(x, w, b, c.s, c.p, c.d, c.g)
    name = hops.LAST_KERNEL_NAME[CONV_ENTRY]
    report(rr.case_id(c) + " [" + name + "]", got, ref)
    assert c.kern in name, "%s ran %s, the table says %s" % (rr.case_id(c), name, c.kern)
    assert_parity(got, ref, 2e-5, what=rr.case_id(c))
    if chain:
        pred = orc.conv2d(x, w, b, c.s, c.p, c.d, c.g, path="chain")
        bad = int((bits(got) != bits(pred)).sum())
        assert bad == 0, "%s: %d of %d elements differ from the fma chain (max abs %.3e)" % (rr.case_id(c), bad, pred.size, float(np.abs(got - pred).max()))
    n = c.shape[0]
    if n > 1:
        one = hops.conv2d(x[n - 1:n], w, b, c.s, c.p, c.d, c.g)
        assert_exact(bits(one), bits(got[n - 1:n]), "%s: the last image alone" % rr.case_id(c))
    return got


def _param(*families):
    cases = rr.cases_of(*families)
    return pytest.mark.parametrize("c", cases, ids=rr.ids_of(cases))


@_param("igemm_fast")
def test_implicit_gemm_fast_path(hops, orc, c):
    """1x3 / 3x1, 1x7 / 7x1, 3x3 at one-axis strides and pads, dh != dw under the straight-line 3x3 mask, 64 taps (the mask's last bit) and 65
    (leaves the fast kernel): the default tile, then every tile, has the bits of the fma chain"""
    check_case(hops, orc, c, chain=True)
    if c.kern != rr.FAST:
        return
    x, w, b, _ = case_ref(c)
    pred = orc.conv2d(x, w, b, c.s, c.p, c.d, c.g, path="chain")
    try:
        for v in ALL_TILES:
            hops.set_plan(f32_tile=int(v))
            got = hops.conv2d(x, w, b, c.s, c.p, c.d, c.g)
            bad = int((bits(got) != bits(pred)).sum())
            assert bad == 0, "%s, tile variant %d: %d of %d elements differ from the fma chain" % (rr.case_id(c), v, bad, pred.size)
    finally:
        hops.set_plan()


@_param("igemm_padk")
def test_zero_padded_k_off_the_pointwise_path(hops, orc, c):
    """1x1 over 24 / 40 / 72 channels with a stride or a pad that differs between the axes: the PADK instantiation of the general form"""
    check_case(hops, orc, c, chain=True)
    assert "fast" in hops.LAST_KERNEL_NAME[CONV_ENTRY]


@_param("igemm_generic")
def test_generic_kernel(hops, orc, c):
    check_case(hops, orc, c, chain=True)


@_param("depthwise")
def test_depthwise(hops, orc, c):
    """the column kernel (kw, sw compile-time; kh, sh run-time) with kh != KW, the generic vector kernel under dh != dw, the scalar kernel"""
    check_case(hops, orc, c, chain=False)


@_param("grouped")
def test_merged_groups(hops, orc, c):
    """4 or 8 channels per group run as dense 32-channel super-groups with a block-diagonal weight image.  orc_conv2d_chain restates plain
    grouped convolutions (k = tap * icg + c), not this K order (k = tap * 32 + c with zeros between a group's channels), so the chain is run
    on the merged problem itself -- rr.merged_groups_dense; a zero weight leaves an accumulator as it is -- and must give the kernel's bits."""
    got = check_case(hops, orc, c, chain=False)
    x, w, b, _ = case_ref(c)
    dense, g2 = rr.merged_groups_dense(w, c.g)
    pred = orc.conv2d(x, dense, b, c.s, c.p, c.d, g2, path="chain")
    bad = int((bits(got) != bits(pred)).sum())
    assert bad == 0, "%s: %d of %d elements differ from the fma chain of the merged problem (max abs %.3e)" % (
        rr.case_id(c), bad, pred.size, float(np.abs(got - pred).max()))


@_param("stem")
def test_small_channel_stems(hops, orc, c):
    """6x7 / 7x6 and the other small-channel rows; the two square kernels at sh != sw must not take the rolling-window stem; a 9-element row
    taller than the stem kernel stages (7x3, 6x3 at sh = 2: si_conv_smallc_ok refuses sh + kh > 7) runs on the implicit GEMM"""
    check_case(hops, orc, c, chain=False)
    assert "stem_roll" not in hops.LAST_KERNEL_NAME[CONV_ENTRY]


# ---- once per family: fused epilogue and a strided view, on a rectangular case and its twin ------------------------------------------------------
# family -> (index of the case within its family, in_ld - ic, out_ld - oc, out_c_off)
VIEWS = {"igemm_fast": (4, 32, 16, 8), "igemm_padk": (0, 12, 8, 4), "igemm_generic": (0, 3, 4, 3), "depthwise": (0, 8, 16, 16), "grouped": (2, 32, 32, 16),
         "stem": (0, 1, 8, 4)}
VIEW_CASES = [c for fam, v in VIEWS.items() for c in (rr.cases_of(fam)[v[0]], [t for t in rr.cases_of(fam) if rr.key(t) == rr.key(rr.twin(rr.cases_of(fam)[v[0]]))][0])]


@pytest.mark.parametrize("c", VIEW_CASES, ids=rr.ids_of(VIEW_CASES))
def test_fused_epilogue_and_strided_view(hops, c):
    x, w, b, ref = case_ref(c)
    _, d_in, d_out, off = VIEWS[c.family]
    ic = c.shape[3]
    r = util.rng_uniform(rr.seed_of(c) + 3, ref.shape, -1, 1)
    got = hops.conv2d(x, w, b, c.s, c.p, c.d, c.g, act1="silu", residual=r, act2="relu")
    assert c.kern in hops.LAST_KERNEL_NAME[CONV_ENTRY]
    want = rr.epilogue_f64(ref, "silu", r, "relu")
    report(rr.case_id(c) + " silu + residual + relu", got, want)
    assert_parity(got, want, 2e-5, what=rr.case_id(c) + " fused epilogue")
    dense = hops.conv2d(x, w, b, c.s, c.p, c.d, c.g)
    wide = hops.conv2d(x, w, b, c.s, c.p, c.d, c.g, in_ld=ic + d_in, in_fill=np.nan, out_ld=c.oc + d_out, out_c_off=off,
                       out_fill=hops.ByteFill(SENTINEL), full=True)
    view = checked_dest(wide, off, c.oc, SENTINEL, rr.case_id(c) + " strided")
    assert_parity(view, ref, 2e-5, what=rr.case_id(c) + " strided view, NaN between the pixels' channels")
    if c.family != "stem":   # (a strided image takes the stem's element-wise loads; the arithmetic of the other families does not depend on the view)
        assert_exact(bits(view), bits(dense), rr.case_id(c) + ": strided view vs dense")


# ---- Winograd near-misses ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", [2, 4])
@pytest.mark.parametrize("pad", [(1, 0), (0, 1)])
def test_winograd_entry_points_refuse_unequal_pads(hops, pad, tile):
    """3x3 stride 1 over 32 -> 32 channels is Winograd's shape in everything but pt != pl: both entries refuse it, and si_hip_conv2d_f32 serves it
    (the same shapes are table cases of test_implicit_gemm_fast_path: correct, and on the fast implicit GEMM)"""
    c = [t for t in rr.cases_of("igemm_fast") if t.k == (3, 3) and t.p == pad and t.s == (1, 1) and t.d == (1, 1)][0]
    x, w, b, ref = case_ref(c)
    with pytest.raises(hops.HipError):
        hops.conv2d_winograd(x, w, b, pad, tile=tile)
    with pytest.raises(hops.HipError):
        hops.conv2d_wino23_split(x, w, b, pad)
    assert_parity(hops.conv2d(x, w, b, c.s, c.p), ref, 2e-5, what="pad %s through conv2d" % (pad,))
    assert rr.FAST in hops.LAST_KERNEL_NAME[CONV_ENTRY]
    # the control: the same tensors at pad (1, 1) ARE eligible
    assert_parity(hops.conv2d_winograd(x, w, b, (1, 1), tile=tile), rr.conv2d_f64(x, w, b, (1, 1), (1, 1)), what="pad (1, 1) is Winograd's")


# ---- fp16 storage --------------------------------------------------------------------------------------------------------------------------------
def f16_kind(hops, c):
    from simpleinfer_amd import _native
    n, ih, iw, ic = c.shape
    oh, ow = rr.out_hw(ih, iw, c.k, c.s, c.p, c.d)
    d = hops.SiConv2dDesc(n, ih, iw, ic, ic, oh, ow, c.oc, c.oc, c.k[0], c.k[1], c.s[0], c.s[1], c.d[0], c.d[1], c.p[0], c.p[1], c.g, 1, 0, 0, c.oc, 0, 0.0)
    return int(_native.hip().si_hip_conv2d_f16_supported(C.byref(d)))


def expected_f16_kind(c):
    """1 implicit GEMM, 2 stem, 3 depthwise, 0 none -- stated from the kernels' documented limits, not read back from the library"""
    if c.family == "stem":   # the instantiated kernel rows: kh 6 or 7 with ceil(kw * ic / 8) = 3, kh 3 with 2; stride <= 2
        return 2 if c.k in ((6, 7), (7, 6), (6, 6), (3, 3)) else 0
    if c.family == "depthwise":
        return 3 if c.shape[3] % 8 == 0 else 0
    return 1 if c.k[0] * c.k[1] <= 64 else 0     # fast / padk: ic % 8 == 0, ungrouped; the 64-bit tap mask


F16_CASES = rr.cases_of("igemm_fast", "igemm_padk", "depthwise", "stem")


@pytest.mark.parametrize("c", F16_CASES, ids=rr.ids_of(F16_CASES))
def test_conv_f16_on_rounded_operands(hops, c):
    """hops.conv2d_f16 on fp16-rounded operands against conv2d_f64 of the same rounded operands.  A case no fp16 kernel serves must be REFUSED
    (HipError) and is then held to the reference through the fp32 entry, which is where the engine runs it."""
    x, w, b = rr.operands(c, w_scale=0.3)
    xr, wr = h(x), h(w)
    ref = rr.conv2d_f64(xr, wr, b, c.s, c.p, c.d, c.g)
    kind = f16_kind(hops, c)
    assert kind == expected_f16_kind(c), (rr.case_id(c), kind)
    if kind == 0:
        with pytest.raises(hops.HipError):
            hops.conv2d_f16(xr, wr, b, c.s, c.p, c.d, c.g)
        assert_parity(hops.conv2d(xr, wr, b, c.s, c.p, c.d, c.g), ref, 2e-5, what=rr.case_id(c) + " refused by fp16, fp32 entry")
        return
    got = hops.conv2d_f16(xr, wr, b, c.s, c.p, c.d, c.g)
    assert got.dtype == np.float16
    report(rr.case_id(c) + " fp16 out (kind %d)" % kind, got.astype(np.float32), ref)
    assert_parity(got.astype(np.float32), ref, F16_TOL, what=rr.case_id(c) + " fp16 out")
    n = c.shape[0]
    if n > 1:
        assert_exact(bits(hops.conv2d_f16(xr[n - 1:n], wr, b, c.s, c.p, c.d, c.g)), bits(got[n - 1:n]), rr.case_id(c) + ": the last image alone")
    if kind != 1:
        return
    try:
        hops.set_plan(f16_tile=0)
        base = hops.conv2d_f16(xr, wr, b, c.s, c.p, c.d, c.g, out_f32=True)
        report(rr.case_id(c) + " fp32 out", base, ref)
        assert_parity(base, ref, 2e-5, what=rr.case_id(c) + " fp16 operands, fp32 out")
        for v in F16_TILES[1:]:
            hops.set_plan(f16_tile=int(v))
            got32 = hops.conv2d_f16(xr, wr, b, c.s, c.p, c.d, c.g, out_f32=True)
            bad = int((bits(got32) != bits(base)).sum())
            assert bad == 0, "%s: fp16 tile variant %d: %d of %d fp32 outputs differ from variant 0" % (rr.case_id(c), v, bad, base.size)
    finally:
        hops.set_plan()


def test_the_6x7_and_7x6_stems_are_fp16_stems(hops):
    for c in rr.cases_of("stem"):
        if c.k in ((6, 7), (7, 6)):
            assert f16_kind(hops, c) == 2, rr.case_id(c)


# ---- f32_split -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", rr.SPLIT3_CASES, ids=[rr.split3_id(c) for c in rr.SPLIT3_CASES])
def test_conv_split3(hops, c):
    """si_hip_conv2d_split3_f32 at the bar of test_conv_split3_vs_oracle_and_fp64 (2e-5 of the tensor's scale vs float64); the range flag stays 0"""
    shape, oc, k, s, p = c
    case = rr.Case("split3", shape, oc, k, s, p, (1, 1), 1, "", "")
    x, w, b = rr.operands(case, w_scale=0.2)
    ref = rr.conv2d_f64(x, w, b, s, p)
    got, flag = hops.conv2d_split3(x, w, b, s, p, return_flag=True)
    report("split3 " + rr.split3_id(c), got, ref)
    assert flag == 0
    assert_parity(got, ref, 2e-5, what="split3 " + rr.split3_id(c))
    n = shape[0]
    if n > 1:
        assert_exact(bits(hops.conv2d_split3(x[n - 1:n], w, b, s, p)), bits(got[n - 1:n]), "split3: the last image alone")


def test_conv_split3_refuses_33_taps(hops):
    x, w = util.rng_uniform(1, (1, 9, 12, 64), -1, 1), util.rng_uniform(2, (32, 64, 3, 11), -0.2, 0.2)
    with pytest.raises(hops.HipError):
        hops.conv2d_split3(x, w, None, (1, 1), (1, 5))


SPLIT_STEMS = [((2, 24, 32, 3), (6, 7), (2, 3)), ((2, 24, 32, 3), (7, 6), (3, 2)), ((2, 32, 24, 3), (7, 6), (3, 2)), ((2, 32, 24, 3), (6, 7), (2, 3))]


@pytest.mark.parametrize("shape,k,p", SPLIT_STEMS, ids=["%dx%d-k%dx%d" % (s[1], s[2], k[0], k[1]) for s, k, p in SPLIT_STEMS])
def test_stem_split3_6x7_and_7x6(hops, shape, k, p):
    """si_hip_conv2d_stem_split3_f32 takes dense image rows of whole 16-byte vectors (iw * 3 a multiple of 4): the table's 30-wide image is
    refused (and served by si_hip_conv2d_f32, test_small_channel_stems); 32- and 24-wide ones run here, at the fp32 bars"""
    case = rr.Case("stem", shape, 32, k, (2, 2), p, (1, 1), 1, "", "")
    x, w, b = rr.operands(case, w_scale=0.3)
    ref = rr.conv2d_f64(x, w, b, (2, 2), p)
    got, flag = hops.conv2d_stem_split3(x, w, b, (2, 2), p, return_flag=True)
    report("split stem %s" % (k,), got, ref)
    assert flag == 0 and got.dtype == np.float32
    assert_parity(got, ref, 2e-5, what="split stem %s" % (k,))
    assert_exact(bits(hops.conv2d_stem_split3(x[1:2], w, b, (2, 2), p)), bits(got[1:2]), "split stem: the last image alone")


def test_stem_split3_refuses_the_30_wide_table_image(hops):
    for c in rr.cases_of("stem"):
        if c.k in ((6, 7), (7, 6)) and (c.shape[2] * 3) % 4 != 0:
            x, w, b, ref = case_ref(c)
            with pytest.raises(hops.HipError):
                hops.conv2d_stem_split3(x, w, b, c.s, c.p)


# ---- max pool ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", rr.POOL_PARAMS, ids=[rr.pool_id(q) for q in rr.POOL_PARAMS])
@pytest.mark.parametrize("ch", [8, 6], ids=["c8_vector", "c6_scalar"])
def test_maxpool_rect_exact(hops, q, ch):
    """fp32 and fp16, bit for bit against torch on an all-negative tensor (a padded tap that took part would win), dense and through a strided
    view whose gaps hold a large finite number (it would win every max it reached)"""
    k, s, p, d = q
    x = rr.pool_input(ch)
    ref = rr.maxpool2d_f64(x, k, s, p, d)
    assert_exact(hops.maxpool2d(x, k, s, p, d).astype(np.float64), ref, "fp32 " + rr.pool_id(q))
    xh = h(x)
    refh = rr.maxpool2d_f64(xh, k, s, p, d)
    got = hops.maxpool2d_f16(xh, k, s, p, d)
    assert got.dtype == np.float16
    assert_exact(got.astype(np.float64), refh, "fp16 " + rr.pool_id(q))
    F = hops.ByteFill(SENTINEL)
    v32 = dict(in_ld=16, in_c_off=8, out_ld=24, out_c_off=12) if ch == 8 else dict(in_ld=9, in_c_off=3, out_ld=11, out_c_off=5)
    wide = hops.maxpool2d(x, k, s, p, d, in_fill=F, out_fill=F, full=True, **v32)
    assert_exact(checked_dest(wide, v32["out_c_off"], ch, SENTINEL, "fp32 strided").astype(np.float64), ref, "fp32 strided " + rr.pool_id(q))
    v16 = dict(in_ld=16, in_c_off=8, out_ld=32, out_c_off=16) if ch == 8 else dict(in_ld=9, in_c_off=3, out_ld=11, out_c_off=5)
    wide = hops.maxpool2d_f16(xh, k, s, p, d, in_fill=F, out_fill=F, full=True, **v16)
    assert_exact(checked_dest(wide, v16["out_c_off"], ch, SENTINEL, "fp16 strided").astype(np.float64), refh, "fp16 strided " + rr.pool_id(q))


# ---- engine: a graph whose layers are all rectangular --------------------------------------------------------------------------------------------
def _run_engine(si, pp, bp, x, **opts):
    e = si.Engine(**opts)
    e.load_model(pp, bp)
    (iname,), (oname,) = e.input_names(), e.output_names()
    e.input(iname, x)
    e.forward()
    return e, e.extract(oname)


def test_engine_rectangular_graph(gpu, tmp_path):
    """7x6 stride-2 RGB stem, 1x7, 7x1, 3x3 pad (1,0), 3x3 stride (1,2), depthwise 3x5 stride (2,1), 1x1 stride (2,1) over 24 channels, max pool
    (3,2) / (2,1), 1x1 head, against the same layers composed from conv2d_f64 / maxpool2d_f64 in float64.  fp32 at winograd 0 / 1 / 2 (no
    layer is Winograd-eligible: the same bits) and with f32_split at the fp32 graph bar of test_graph_parity_vs_oracle; fp16 storage at the bar
    of test_fp16_graph_vs_fp32_oracle."""
    import simpleinfer_amd as si
    from test_gpu_engine import F16_GRAPH_TOL
    mg = si.modelgen
    b = rr.build_rect_graph(mg)
    pp, bp = str(tmp_path / "rect.pnnx.param"), str(tmp_path / "rect.pnnx.bin")
    b.save(pp, bp)
    x = mg.synth_input((2, 48, 60, 3))
    ref = rr.eval_rect_graph(b, x)
    outs = {}
    for wino in (0, 1, 2):
        e, outs[wino] = _run_engine(si, pp, bp, x, winograd=wino)
        report("engine winograd=%d" % wino, outs[wino], ref)
        assert_parity(outs[wino], ref, what="rectangular graph, winograd=%d" % wino)
        kernels = [L["kernel"] for L in e.profile()]
        assert not any("wino" in k for k in kernels), kernels
    assert_exact(bits(outs[1]), bits(outs[0]), "winograd=1 vs 0")
    assert_exact(bits(outs[2]), bits(outs[0]), "winograd=2 vs 0")
    assert any(rr.SMALLC in k for k in kernels) and any(rr.FAST in k for k in kernels) and any(rr.dw_cols(5, 1) in k for k in kernels), kernels
    assert not any("stem_roll" in k for k in kernels), kernels
    # an image's bits do not depend on its batch
    bone = rr.build_rect_graph(mg, batch=1)
    pp1, bp1 = str(tmp_path / "rect1.pnnx.param"), str(tmp_path / "rect1.pnnx.bin")
    bone.save(pp1, bp1)
    _, one = _run_engine(si, pp1, bp1, x[1:2])
    assert_exact(bits(one), bits(outs[0][1:2]), "the second image alone")
    e, split = _run_engine(si, pp, bp, x, f32_split=1)
    report("engine f32_split", split, ref)
    assert_parity(split, ref, what="rectangular graph, f32_split")
    # the option did something: by the engine's own policy (K and output-channel thresholds of Conv2d::UseSplit3) the layers of this small graph
    # stay on their fp32 kernels except the 7x6 stem, which takes the split stem kernel (the split implicit GEMM is held at op level above)
    skernels = [L["kernel"] for L in e.profile()]
    assert "conv_stem_split_f32_kernel" in skernels, skernels
    assert not np.array_equal(bits(split), bits(outs[0])), "f32_split changed no bit"
    e, half = _run_engine(si, pp, bp, x, fp16=1)
    report("engine fp16", half, ref)
    assert half.dtype == np.float32
    assert_parity(half, ref, F16_GRAPH_TOL, what="rectangular graph, fp16 storage")
    assert any("f16" in L["kernel"] for L in e.profile()), e.profile()
