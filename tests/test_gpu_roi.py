"""GPU: the box-pooling kernel of include/si_roi.h, torchvision.ops.RoIAlign and torchvision.ops.roi_align.  Kernel: the case matrix of
tests/roi_reference.py against the restatement (float32 decisions, float64 sums), bit-exactness on dyadic cases and on samples that land
exactly on -1, 0, h - 1 and h, invalid boxes, independence of the rows, views under guard bands with every vector arm, three passes of the
grid-stride loop.  Layer and engine: the one-operator graph under both type strings, both toys in fp32 (also captured) and under fp16 storage,
the batch-split modes, refusals at load.  Every engine test fails without the layer (LoadModel rejects the types with kEmpty), every op-level
test without the kernel (the symbols are missing)."""
import numpy as np
import pytest

import containment as ct
import roi_reference as rr
import util
from ct_reference import _parse
from simpleinfer_amd import hipops, modelgen as mg
from simpleinfer_amd.engine import Engine, Status, StatusError

pytestmark = pytest.mark.gpu

FP16_EPS = 2.0 ** -11     # half an ulp of a round-to-nearest-even fp16 store, relative to the element


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype and got.dtype in (np.float32, np.float16), (what, got.shape, want.shape, got.dtype, want.dtype)
    u = np.uint32 if got.dtype == np.float32 else np.uint16
    bad = np.nonzero(got.view(u) != want.view(u))
    assert bad[0].size == 0, "%s: %d of %d elements differ in bits, first at %s" % (what, bad[0].size, got.size, tuple(int(b[0]) for b in bad))


def check(got, ref, what):
    """(test_gpu_grid.py's) the NaN positions equal the reference's; everything else at the fp32 bar of util.assert_parity -- for fp16 storage
    plus half an fp16 ulp of the element for the one rounding store.  Returns the max-based error."""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "%s: NaN masks differ (%d vs %d)" % (what, np.isnan(got).sum(), np.isnan(ref).sum())
    ok = np.isfinite(ref)
    assert np.isfinite(got[ok]).all(), what + ": a non-finite value where the reference is finite"
    g, r = np.where(ok, got, 0.0).astype(np.float64), np.where(ok, ref, 0.0)
    if got.dtype == np.float32:
        return util.assert_parity(g, r, what=what)
    scale = max(float(np.abs(r).max()), 1e-30)
    worst = float((np.abs(g - r) / (FP16_EPS * np.abs(r) + util.REL_TOL * scale)).max())
    assert worst <= 1.0, "%s: %.3f of the fp16 bound" % (what, worst)
    return util.rel_err(g, r)


def kernel():
    return hipops.LAST_KERNEL_NAME["si_hip_roi_align"]


# ---- the case matrix ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("c", rr.MATRIX_C)
def test_case_matrix_against_the_restatement(gpu, c, half):
    """x [2, c, 9, 11] x outputs (1,1) (2,3) (7,7) x sampling_ratio -1 0 1 2 3 x both `aligned` x scale 1 0.25 0.0625 x K 1 5 70: no case is
    skipped.  The reference of a combination is computed once for 70 boxes and 16 channels; rows and channels are independent, so every c
    and K is a slice of it, and x holds fp16 numbers, so both storage types share it."""
    dt = np.float16 if half else np.float32
    x = np.ascontiguousarray(rr.matrix_x()[..., :c]).astype(dt)
    worst, cases = 0.0, 0
    for out, ratio, aligned, scale in rr.matrix_params():
        ref, rois = rr.matrix_ref(out, ratio, aligned, scale), rr.matrix_rois(scale)
        for k in rr.MATRIX_K:
            got = hipops.roi_align(x, rois[:k], out, scale, ratio, aligned)
            what = "c %d %s out %s ratio %d aligned %d scale %g K %d" % (c, dt.__name__, out, ratio, aligned, scale, k)
            assert got.dtype == dt and kernel() == rr.expected_kernel(c, half), (what, kernel())
            worst = max(worst, check(got, ref[:k, :, :, :c], what))
            cases += 1
    assert cases == 90 * 3
    print("roi_align c %d %s: %d cases, worst max-based error %.3e" % (c, dt.__name__, cases, worst))


# ---- bit exactness ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("c", [4, 3, 8], ids=["c4", "c3", "c8"])
def test_dyadic_cases_bit_for_bit(gpu, c, half):
    """x holds small integers; scale 1, aligned=False: coordinates and weights are dyadic, every product and sum is exact in fp32, and the
    result is the reference's bit for bit"""
    dt = np.float16 if half else np.float32
    h, w = 9, 11
    x = np.floor(util.rng_uniform(111, (2, h, w, c), 0.0, 8.0)).astype(dt)
    # boxes [0, 0, 2 pw, 2 ph]: bins of 2 px; one sample per axis falls on pixel centres, two on halves
    for (ph, pw), ratio in (((3, 4), 1), ((3, 4), 2), ((4, 5), 2), ((1, 1), 2)):
        rois = np.asarray([[0, 0, 0, 2 * pw, 2 * ph], [1, 0, 0, 2 * pw, 2 * ph], [1, 1, 2, 1 + 2 * pw, 2 + 2 * ph]], np.float32)
        got = hipops.roi_align(x, rois, (ph, pw), 1.0, ratio, False)
        same_bits(got, rr.roi_align_ref(x, rois, (ph, pw), 1.0, ratio, False).astype(dt), "boxes of 2 px bins, %dx%d ratio %d" % (ph, pw, ratio))
    # 1 px bins, one sample each, from -1.5 to size + 0.5: the samples land on -1, 0, 1, .., h - 1, h exactly -- both are inside and clamp to
    # the border row; shifted by 2^-10 down (up) the first (last) sample is outside and the others blend with weights k / 1024
    e = 2.0 ** -10
    rois = np.asarray([[0, -1.5, -1.5, w + 0.5, h + 0.5], [1, -1.5 - e, -1.5 - e, w + 0.5 - e, h + 0.5 - e], [0, -1.5 + e, -1.5 + e, w + 0.5 + e, h + 0.5 + e],
                       [1, -1.5, -1.5 + e, w + 0.5, h + 0.5 + e]], np.float32)
    ref = rr.roi_align_ref(x, rois, (h + 2, w + 2), 1.0, 1, False)
    assert np.array_equal(ref[0, 0, 1:-1], x[0, 0].astype(np.float64)) and np.array_equal(ref[0, -1, 1:-1], x[0, -1].astype(np.float64))   # -1 and h: the border rows
    assert np.array_equal(ref[0, 1:-1, 0], x[0, :, 0].astype(np.float64)) and np.array_equal(ref[0, 0, 0], x[0, 0, 0].astype(np.float64))
    assert not ref[1, 0].any() and not ref[1, :, 0].any() and ref[1, -1].any()                 # just below -1: nothing; just below h: inside
    assert not ref[2, -1].any() and not ref[2, :, -1].any() and ref[2, 0].any()                # just above h: nothing; just above -1: inside
    got = hipops.roi_align(x, rois, (h + 2, w + 2), 1.0, 1, False)
    same_bits(got, ref.astype(dt), "samples on -1, 0, h - 1, h and one step beside them")
    # the same through adaptive sampling: bins of 1 px take ceil(1) = 1 sample
    same_bits(hipops.roi_align(x, rois[:1], (h + 2, w + 2), 1.0, 0, False), ref[:1].astype(dt), "adaptive, one sample per bin")


# ---- invalid boxes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,half", [(4, False), (5, False), (8, True), (6, True)], ids=["f32_vec4", "f32_scalar", "f16_vec8", "f16_vec2"])
def test_invalid_boxes_are_nan_rows_and_nothing_else_changes(gpu, c, half):
    dt = np.float16 if half else np.float32
    x = util.rng_uniform(121, (2, 7, 6, c), -1.0, 1.0).astype(dt)
    good = [[0, 1.0, 0.5, 5.0, 4.5], [1, -2.0, 1.0, 3.0, 8.0], [1, 0.0, 0.0, 6.0, 7.0]]
    bad = [[-1, 1, 1, 4, 3], [2, 1, 1, 4, 3], [0.5, 1, 1, 4, 3], [np.nan, 1, 1, 4, 3], [0, np.nan, 1, 4, 3], [1, 1, np.nan, 4, 3], [0, 1, 1, np.inf, 3],
           [1, 1, 1, 4, -np.inf], [0, -np.inf, 1, np.inf, 3]]
    rois = np.asarray([good[0]] + bad[:4] + [good[1]] + bad[4:] + [good[2]], np.float32)
    is_bad = np.asarray([False] + [True] * 4 + [False] + [True] * 5 + [False])
    for ratio, aligned in ((2, False), (0, True)):
        alone = hipops.roi_align(x, np.asarray(good, np.float32), (3, 2), 1.0, ratio, aligned)
        with hipops.guard_bands(0x7B) as g:                      # x and the boxes are held to their bytes, the bands around all three checked
            got = hipops.roi_align(x, rois, (3, 2), 1.0, ratio, aligned)
        assert g.checked == 3
        assert np.isnan(got[is_bad]).all(), (ratio, aligned)
        same_bits(got[~is_bad], alone, "the neighbours of the invalid rows, ratio %d aligned %d" % (ratio, aligned))
        check(got, rr.roi_align_ref(x, rois, (3, 2), 1.0, ratio, aligned), "invalid boxes against the restatement")


# ---- independence -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
def test_rows_are_independent_bit_for_bit(gpu, half):
    dt = np.float16 if half else np.float32
    x = np.ascontiguousarray(rr.matrix_x()[..., :8]).astype(dt)
    rois = rr.matrix_rois(0.25)
    for out, ratio, aligned in (((2, 3), 0, False), ((7, 7), 2, True)):
        base = hipops.roi_align(x, rois, out, 0.25, ratio, aligned)
        same_bits(hipops.roi_align(x, rois, out, 0.25, ratio, aligned), base, "two launches")
        perm = np.random.Generator(np.random.Philox(5)).permutation(len(rois))
        same_bits(hipops.roi_align(x, rois[perm], out, 0.25, ratio, aligned), base[perm], "permuted boxes")
        same_bits(hipops.roi_align(x, rois[17:18], out, 0.25, ratio, aligned), base[17:18], "one box alone")
        x2 = x.copy()
        x2[1] = -x2[1] + dt(0.5)
        other = hipops.roi_align(x2, rois, out, 0.25, ratio, aligned)
        on0 = rois[:, 0] == 0
        same_bits(other[on0], base[on0], "rows of image 0 after image 1 changed")
        assert not np.array_equal(other[~on0], base[~on0])
        # every vector arm of the type computes the same bits
        arms = set()
        for in_ld, out_ld in ((16, 24), (12, 8), (10, 8), (8, 18), (9, 8), (8, 11)):
            same_bits(hipops.roi_align(x, rois, out, 0.25, ratio, aligned, in_ld=in_ld, out_ld=out_ld, in_fill=np.nan), base, "in_ld %d out_ld %d" % (in_ld, out_ld))
            arms.add(kernel())
        assert arms == {rr.expected_kernel(v, half) for v in ((8, 4, 2, 1) if half else (4, 1))}, arms


# ---- views and containment ----------------------------------------------------------------------------------------------------
class RoiView:
    buffers = 3

    def __init__(self, vid, half, c, out, ratio, aligned, arm, rois_ld=None, **views):
        self.id, self.half, self.c, self.out, self.ratio, self.aligned, self.arm, self.rois_ld, self.views = vid, half, c, out, ratio, aligned, arm, rois_ld, views
        self.entry = "si_hip_roi_align_f16" if half else "si_hip_roi_align_f32"

    def operands(self):
        dt = np.float16 if self.half else np.float32
        rois = rr.matrix_rois(0.25)[:24].copy()
        rois[5] = [np.nan, 1, 1, 9, 9]              # an invalid row among them
        return util.rng_uniform(131, (2, 9, 11, self.c), -1.0, 1.0).astype(dt), rois

    def run(self, fill):
        x, rois = self.operands()
        full = hipops.roi_align(x, rois, self.out, 0.25, self.ratio, self.aligned, rois_ld=self.rois_ld, rois_fill=fill, in_fill=fill, out_fill=fill, full=True,
                                **self.views)
        assert kernel() == "roi_align_kernel<%s, %d>" % ("_Float16" if self.half else "float", self.arm), (self.id, kernel())
        return ct.Out("y", full, self.views.get("out_c_off", 0), self.c)

    def dense(self):
        x, rois = self.operands()
        return hipops.roi_align(x, rois, self.out, 0.25, self.ratio, self.aligned), rr.roi_align_ref(x, rois, self.out, 0.25, self.ratio, self.aligned)


VIEW_CASES = [
    RoiView("f32_vec4_slices", False, 8, (3, 2), 2, False, 4, rois_ld=8, in_ld=20, in_c_off=4, out_ld=24, out_c_off=12),
    RoiView("f32_misaligned_pointers", False, 8, (2, 3), 0, True, 1, rois_ld=7, in_ld=20, in_c_off=3, out_ld=24, out_c_off=12),     # x 12 bytes off: scalars
    RoiView("f32_scalar_last_slice", False, 5, (7, 7), -1, True, 1, rois_ld=5, in_ld=9, in_c_off=4, out_ld=7, out_c_off=2),
    RoiView("f16_vec8_slices", True, 8, (3, 2), 2, True, 8, rois_ld=6, in_ld=16, in_c_off=8, out_ld=32, out_c_off=16),
    RoiView("f16_vec4_by_pointer", True, 8, (2, 3), 0, False, 4, rois_ld=9, in_ld=16, in_c_off=8, out_ld=32, out_c_off=20),         # out 8 bytes off 16
    RoiView("f16_vec2", True, 6, (1, 1), 3, False, 2, rois_ld=11, in_ld=14, in_c_off=2, out_ld=22, out_c_off=4),
    RoiView("f16_scalar", True, 3, (2, 3), 1, True, 1, in_ld=11, in_c_off=5, out_ld=8, out_c_off=5),
]


@pytest.mark.parametrize("case", VIEW_CASES, ids=[c.id for c in VIEW_CASES])
def test_views_and_containment(gpu, case):
    del hipops.LAST_ENTRIES[:]
    dense, ref = case.dense()
    check(dense, ref, case.id + ", dense")
    plain = case.run(hipops.ByteFill(0x00))
    assert case.entry in hipops.LAST_ENTRIES, hipops.LAST_ENTRIES
    ct.assert_outside_fill(plain.full, plain.c_off, plain.c, 0x00, case.id + ", plain run")
    same_bits(plain.full[..., plain.c_off:plain.c_off + plain.c], dense, case.id + " against the dense run")
    for byte in ct.PATTERNS:      # 0xFF: the gaps between the channels and between the boxes hold NaN; 0x7B: a large finite sentinel
        with hipops.guard_bands(byte) as g:      # all bands and the inputs are compared when the block ends
            out = case.run(hipops.ByteFill(byte))
        what = "%s under 0x%02X" % (case.id, byte)
        assert g.checked == case.buffers, "%s: the guard saw %d buffers" % (what, g.checked)
        ct.assert_outside_fill(out.full, out.c_off, out.c, byte, what)             # every byte outside the output view unchanged
        same_bits(out.full[..., out.c_off:out.c_off + out.c], plain.full[..., plain.c_off:plain.c_off + plain.c], what)


def test_three_passes_of_the_grid_stride_loop(gpu):
    """fp16, c = 8: one item per bin, 2048 x 256 items per pass, 1100 boxes x 31 x 31 bins = 2.02 passes' worth: every lane goes round up to
    three times"""
    k, out = 1100, (31, 31)
    assert 2 * 2048 * 256 < k * out[0] * out[1] <= 3 * 2048 * 256
    x = util.rng_uniform(141, (2, 5, 6, 8), -1.0, 1.0).astype(np.float16)
    u = util.rng_uniform(142, (k, 4), 0.0, 1.0)
    rois = np.stack([np.arange(k) % 2, u[:, 0] * 8 - 2, u[:, 1] * 7 - 2, u[:, 0] * 8 - 2 + u[:, 2] * 6, u[:, 1] * 7 - 2 + u[:, 3] * 5], 1).astype(np.float32)
    got = hipops.roi_align(x, rois, out, 1.0, 1, True)
    assert kernel() == rr.expected_kernel(8, True)
    check(got, rr.roi_align_ref(x, rois, out, 1.0, 1, True), "three passes")


# ---- layer and engine ---------------------------------------------------------------------------------------------------------
def save(b, tmp_path, tag):
    pp, bp = str(tmp_path / (tag + ".pnnx.param")), str(tmp_path / (tag + ".pnnx.bin"))
    b.save(pp, bp)
    return pp, bp


def run_engine(b, tmp_path, xs, tag="m", forwards=1, **opts):
    """(engine, the list of the graph outputs as the engine stores them); xs: one array per graph input, in order"""
    pp, bp = save(b, tmp_path, tag)
    e = Engine(**opts)
    e.load_model(pp, bp)
    for name, x in zip(e.input_names(), xs):
        e.input(name, x)
    for _ in range(forwards):
        e.forward()
    return e, [e.extract(_parse(ln)[2][0]) for ln in b.lines if ln.startswith("pnnx.Output")]


def status_of_load(b, tmp_path, tag, **opts):
    pp, bp = save(b, tmp_path, tag)
    with pytest.raises(StatusError) as ei:
        Engine(**opts).load_model(pp, bp)
    return ei.value.status


@pytest.mark.parametrize("functional", [False, True], ids=["RoIAlign", "roi_align"])
def test_one_operator_graph(gpu, tmp_path, functional):
    x = util.rng_uniform(151, (2, 9, 11, 8), -1.0, 1.0)
    rois = rr.matrix_rois(0.25)[:20]
    b = mg.PnnxBuilder(seed=1)
    b.output(b.roi_align(b.input((2, 8, 9, 11)), b.input((20, 5)), (7, 5), 0.25, 2, True, functional=functional))
    eng, (got,) = run_engine(b, tmp_path, [x, rois])
    assert got.shape == (20, 7, 5, 8)
    check(got, rr.roi_align_ref(x, rois, (7, 5), 0.25, 2, True), "the layer")
    same_bits(got, hipops.roi_align(x, rois, (7, 5), 0.25, 2, True), "the layer against the op-level entry")
    (layer,) = [L for L in eng.profile() if L["type"] == rr.TYPES[int(functional)]]
    assert layer["kernel"] == "roi_align_kernel<float, 4>", layer
    assert layer["flops"] == (8.0 * 4 + 1.0) * got.size and layer["bytes"] == 4.0 * (x.size + rois.size + got.size), layer
    # adaptive sampling and the defaults pnnx leaves out
    b = mg.PnnxBuilder(seed=1)
    y = b.roi_align(b.input((2, 8, 9, 11)), b.input((20, 5)), 3, functional=functional)
    b.lines[-1] = " ".join(t for t in b.lines[-1].split() if not t.startswith(("aligned=", "sampling_ratio=", "spatial_scale=")))
    b.lines[-1] = b.lines[-1].replace("output_size=(3,3)", "output_size=3")
    b.output(y)
    big = rr.matrix_rois(1.0)[:20]
    _, (got,) = run_engine(b, tmp_path, [x, big], tag="defaults")
    same_bits(got, hipops.roi_align(x, big, 3, 1.0, -1, False), "output_size=3 and torchvision's defaults")


def toy_inputs(b):
    n, c, h, w = b.shapes["0"]
    return [mg.synth_input((n, h, w, c)), mg.toy_rois(b.shapes["1"][0], n, h, w)]


TOYS = {"box": mg.build_toy_box_head, "mask": mg.build_toy_mask_head}


@pytest.mark.parametrize("which", sorted(TOYS))
def test_toys_fp32(gpu, tmp_path, which):
    b = TOYS[which]()
    xs = toy_inputs(b)
    want = rr.eval_graph(b, xs)
    eng, got = run_engine(b, tmp_path, xs)
    assert len(got) == len(want) == (2 if which == "box" else 1)
    for g, w in zip(got, want):
        util.assert_parity(g, w, what="toy " + which)
    (layer,) = [L for L in eng.profile() if L["type"] in rr.TYPES]
    assert layer["kernel"] == "roi_align_kernel<float, 4>", layer
    _, cap = run_engine(b, tmp_path, xs, forwards=3, graph=1)
    for g, c in zip(got, cap):
        same_bits(c, g, which + ": graph=1 replay over three forwards")
    _, plain = run_engine(b, tmp_path, xs, fuse=0)
    for g, p in zip(got, plain):
        util.assert_parity(p, g, what=which + ", fuse=0")


@pytest.mark.parametrize("which", sorted(TOYS))
def test_toys_fp16_storage(gpu, tmp_path, which):
    """fp16=1: the features are a graph input and keep fp32, so the pooling runs on the fp32 kernel and a cast follows it; the boxes stay fp32.
    The error against float64 is at most 2x that of the fp16-storage emulation (weights, the inputs and every operator's output rounded to
    fp16, float64 arithmetic between): the bar of test_toys_fp16_storage of the other toys"""
    b = TOYS[which]()
    xs = toy_inputs(b)
    eng, got = run_engine(b, tmp_path, xs, fp16=1)
    (layer,) = [L for L in eng.profile() if L["type"] in rr.TYPES]
    assert layer["kernel"] == "roi_align_kernel<float, 4>", layer
    ref, emu = rr.eval_graph(b, xs), rr.eval_graph(b, xs, rnd=rr.round_f16)
    for g, r, m in zip(got, ref, emu):
        e_engine, e_emu = util.rel_err(g, r), util.rel_err(m, r)
        print("toy %s fp16 storage vs float64: engine %.3e, fp16 emulation %.3e" % (which, e_engine, e_emu))
        assert np.isfinite(g).all() and e_engine <= 2.0 * e_emu, (e_engine, e_emu)


def test_half_features_are_pooled_natively_with_fp32_boxes(gpu, tmp_path):
    """behind a conv the features are half under fp16=1 and the boxes, a graph input, fp32: the f16 entry, no cast around the pooling"""
    b = mg.PnnxBuilder(seed=2)
    feat, rois_in = b.input((2, 8, 20, 24)), b.input((6, 5))
    b.output(b.conv(b.roi_align(b.conv(feat, 16, 1), rois_in, 7, 0.25, 2, False), 8, 3, 1, 1))
    xs = [mg.synth_input((2, 20, 24, 8)), mg.toy_rois(6, 2, 20, 24)]
    eng, (got,) = run_engine(b, tmp_path, xs, fp16=1)
    (layer,) = [L for L in eng.profile() if L["type"] in rr.TYPES]
    assert layer["kernel"] == "roi_align_kernel<_Float16, 8>", layer
    (ref,), (emu,) = rr.eval_graph(b, xs), rr.eval_graph(b, xs, rnd=rr.round_f16)
    e_engine, e_emu = util.rel_err(got, ref), util.rel_err(emu, ref)
    print("conv -> RoIAlign -> conv, fp16 storage vs float64: engine %.3e, fp16 emulation %.3e" % (e_engine, e_emu))
    assert np.isfinite(got).all() and e_engine <= 2.0 * e_emu, (e_engine, e_emu)
    _, (f32,) = run_engine(b, tmp_path, xs)
    util.assert_parity(f32, ref, what="the same graph in fp32")


@pytest.mark.parametrize("boxes", [4, 6], ids=["K_eq_N", "K_ne_N"])
def test_batch_split_modes_leave_the_graph_uncut(gpu, tmp_path, boxes):
    """dimension 0 of the output counts boxes: host_slices=2 serves the graph unsliced with the unsplit bits and names the layer; streams=2 and
    a re-batch are refused at load -- also where the number of boxes equals the batch by coincidence"""
    b = mg.build_toy_box_head(batch=4, boxes=boxes)
    xs = toy_inputs(b)
    e0, base = run_engine(b, tmp_path, xs, host_slices=1, streams=1)
    for g, w in zip(base, rr.eval_graph(b, xs)):
        util.assert_parity(g, w, what="unsplit")
    e1, got = run_engine(b, tmp_path, xs, host_slices=2)
    sched = e1.schedule()
    assert sched["host_slices"] == 1 and sched["lanes"] == 1, sched
    assert any("roialign_0" in m and "count" in m and "boxes" in m for m in sched["batch_mixing"]), sched["batch_mixing"]
    for g, w in zip(got, base):
        same_bits(g, w, "host_slices=2")
    assert status_of_load(b, tmp_path, "streams", streams=2) == Status.kUnsupport
    assert status_of_load(b, tmp_path, "rebatch", batch=8) == Status.kUnsupport
    assert status_of_load(b, tmp_path, "rebatch_same", batch=4) == Status.kUnsupport


def test_refused_at_load(gpu, tmp_path):
    """the boxes as a list, rank-3 boxes, four columns, a wrong output: kUnsupport / kErrorShape with a logged reason; the process goes on"""
    def pool(x_shape, rois_shapes, out_shape, **params):
        b = mg.PnnxBuilder(seed=1)
        x = b.input(x_shape)
        rs = [b.input(s) for s in rois_shapes]
        y = b._new_operand(out_shape)
        p = dict(aligned=False, output_size=(3, 3), sampling_ratio=2, spatial_scale=1.0)
        p.update(params)
        b._emit(rr.TYPES[0], "roialign_0", [x] + rs, [y], p)
        b.output(y)
        return b

    assert status_of_load(pool((2, 8, 9, 11), [(3, 4), (2, 4)], (5, 8, 3, 3)), tmp_path, "list2") == Status.kUnsupport        # [boxes of image 0, of image 1]
    assert status_of_load(pool((1, 8, 9, 11), [(3, 4)], (3, 8, 3, 3)), tmp_path, "list1") == Status.kUnsupport                # a list of one [K, 4] tensor
    assert status_of_load(pool((2, 8, 9, 11), [(6, 4)], (6, 8, 3, 3)), tmp_path, "cols4") == Status.kUnsupport
    assert status_of_load(pool((2, 8, 9, 11), [(2, 3, 5)], (6, 8, 3, 3)), tmp_path, "rank3") == Status.kErrorShape
    assert status_of_load(pool((2, 8, 9, 11), [(6, 6)], (6, 8, 3, 3)), tmp_path, "cols6") == Status.kErrorShape
    assert status_of_load(pool((2, 8, 9, 11), [(6, 5)], (5, 8, 3, 3)), tmp_path, "out_k") == Status.kErrorShape
    assert status_of_load(pool((2, 8, 9, 11), [(6, 5)], (6, 7, 3, 3)), tmp_path, "out_c") == Status.kErrorShape
    assert status_of_load(pool((2, 8, 9, 11), [(6, 5)], (6, 8, 3, 4)), tmp_path, "out_w") == Status.kErrorShape
    assert status_of_load(pool((8, 9, 11), [(6, 5)], (6, 8, 3, 3)), tmp_path, "x_rank3") == Status.kErrorShape
    assert status_of_load(pool((2, 8, 9, 11), [(6, 5)], (6, 8, 3, 3), sampling_ratio=257), tmp_path, "ratio") == Status.kUnsupport
    bad = pool((2, 8, 9, 11), [(6, 5)], (6, 8, 3, 3))
    bad.lines = [ln.replace("output_size=(3,3)", "output_size=(3,3,3)") for ln in bad.lines]
    assert status_of_load(bad, tmp_path, "size3") == Status.kFail
    x, rois = util.rng_uniform(161, (2, 9, 11, 8), -1.0, 1.0), rr.matrix_rois(1.0)[:6]
    _, (got,) = run_engine(pool((2, 8, 9, 11), [(6, 5)], (6, 8, 3, 3)), tmp_path, [x, rois], tag="after")
    check(got, rr.roi_align_ref(x, rois, 3, 1.0, 2, False), "after the refusals")
