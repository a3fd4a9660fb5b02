"""GPU: bilinear upsample (si_hip_upsample_bilinear_f32 / _f16), nearest by size and the segmentation label map against the numpy
reference of tests/up_reference.py (pinned to torch by tests/test_upsample_cpu.py), and nn.Upsample / F.interpolate / F.upsample inside
the engine: one-op graphs, the bilinear toy U-Net and the toy segmentation net in fp32 and with fp16 storage, and the files it refuses."""
import os

import numpy as np
import pytest

import up_reference as ur
import util
from ct_reference import _parse, round_f16
from simpleinfer_amd import hipops, modelgen as mg
from simpleinfer_amd.engine import Engine, Status, StatusError

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "ops_golden.npz"))

HEAD_CASES = [(shape, ac, dict(out_hw=out_hw)) for _, shape, out_hw, ac in ur.LABEL_CASES]
OP_CASES = ([(s, ac, ur.form_args(s, f)) for s, ac, f in ur.BASE_CASES] +
            [(s, ac, dict(scale=2.0)) for s in ur.DECODER_SHAPES for ac in (False, True)] + HEAD_CASES +
            [((2, 9, 11, c), ac, dict(scale=2.0)) for c in (1, 3, 21, 255) for ac in (False, True)] +
            [((5, 6, 7, 12), False, dict(scale=2.0)), ((5, 6, 7, 21), True, dict(out_hw=(13, 9)))] +
            [(s, ac, kw) for s, kw in ur.EXTRA_CASES for ac in (False, True)])
OP_IDS = [ur.case_id(*c) for c in OP_CASES]


def fp16_bound(ref64, x):
    """half an fp16 ulp of the result (one round-to-nearest-even store) plus the fp32 blend error"""
    return 2.0 ** -11 * np.abs(ref64) + ur.blend_bound(x)


def check_f32(got, ref, x, what):
    assert got.dtype == np.float32 and got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), what
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print("%s: %.2f x 2^-24 max|x|" % (what, err / (ur.EPS * float(np.abs(x).max()))))
    assert err <= ur.blend_bound(x), "%s: max|diff| %.3e > %.3e" % (what, err, ur.blend_bound(x))


def check_f16(got, ref, x, what):
    assert got.dtype == np.float16 and got.shape == ref.shape, (what, got.shape, ref.shape)
    ratio = float((np.abs(got.astype(np.float64) - ref) / fp16_bound(ref, x)).max())
    print("%s: worst %.3f of the fp16 bound" % (what, ratio))
    assert ratio <= 1.0, "%s: %.3f of the fp16 bound" % (what, ratio)


# ---- op level -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,ac,kw", OP_CASES, ids=OP_IDS)
def test_bilinear_fp32(gpu, shape, ac, kw):
    x = ur.case_input(shape)
    check_f32(hipops.upsample_bilinear(x, align_corners=ac, **kw), ur.upsample_bilinear_ref(x, align_corners=ac, **kw), x, ur.case_id(shape, ac, kw))


@pytest.mark.parametrize("shape,ac,kw", OP_CASES, ids=OP_IDS)
def test_bilinear_fp16(gpu, shape, ac, kw):
    x = ur.case_input(shape, half=True)
    check_f16(hipops.upsample_bilinear(x, align_corners=ac, **kw), ur.upsample_bilinear_ref(x, align_corners=ac, **kw), x, ur.case_id(shape, ac, kw))


# (channels, input stride, output stride, channel offset): 16 bytes per lane in both types; 8- and 4-byte vectors for half; scalars
VIEWS = [(8, 16, 24, 8), (4, 12, 20, 4), (6, 14, 22, 2), (21, 29, 40, 12), (3, 11, 8, 5), (1, 9, 4, 3)]


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("c,in_ld,out_ld,off", VIEWS, ids=["c%d_ld%d_%d_off%d" % v for v in VIEWS])
def test_strided_views(gpu, c, in_ld, out_ld, off, half):
    """input at a wider pixel stride with NaN between the pixels' channels; output into channels [off, off + c) of a wider buffer filled with a
    sentinel: every channel outside the view keeps the sentinel bit for bit"""
    assert in_ld == c + 8
    x = ur.case_input((2, 7, 9, c), 5, half)
    sentinel = -1234.5
    for ac, kw in ((False, dict(scale=2.0)), (True, dict(out_hw=(10, 31)))):
        y = hipops.upsample_bilinear(x, align_corners=ac, in_ld=in_ld, in_fill=np.nan, out_ld=out_ld, out_c_off=off, out_fill=sentinel,
                                     full=True, **kw)
        ref = ur.upsample_bilinear_ref(x, align_corners=ac, **kw)
        (check_f16 if half else check_f32)(np.ascontiguousarray(y[..., off:off + c]), ref, x, "strided view c=%d" % c)
        outside = np.concatenate([y[..., :off], y[..., off + c:]], axis=-1)
        bits = np.uint16 if half else np.uint32
        assert np.array_equal(outside.view(bits), np.full(outside.shape, sentinel, x.dtype).view(bits))
        # ... and the view's values are the dense call's, bit for bit (the vector width may differ: the blend does not)
        dense = hipops.upsample_bilinear(x, align_corners=ac, **kw)
        util.assert_exact(np.ascontiguousarray(y[..., off:off + c]).view(bits), dense.view(bits), "strided vs dense")


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
def test_same_bits_twice(gpu, half):
    bits = np.uint16 if half else np.uint32
    for shape, ac, kw in (((2, 64, 64, 21), False, dict(out_hw=(512, 512))), ((2, 32, 32, 512), True, dict(scale=2.0))):
        x = ur.case_input(shape, 7, half)
        a = hipops.upsample_bilinear(x, align_corners=ac, **kw)
        b = hipops.upsample_bilinear(x, align_corners=ac, **kw)
        util.assert_exact(a.view(bits), b.view(bits), "two launches")


def test_nearest_by_size_is_exact(gpu):
    for shape in ur.BASE_SHAPES + [(2, 9, 11, 255), (1, 12, 9, 6)]:
        x = ur.case_input(shape, 2)
        for out_hw in (ur.form_args(shape, "size")["out_hw"], (shape[1] + 3, 2 * shape[2] + 1), (max(1, shape[1] // 2), max(1, shape[2] - 1))):
            got = hipops.upsample_nearest_size(x, out_hw)
            util.assert_exact(got.view(np.uint32), ur.upsample_nearest_ref(x, out_hw=out_hw).view(np.uint32), "nearest %s to %s" % (shape, out_hw))
    x = ur.case_input((2, 5, 6, 8), 3)
    got = hipops.upsample_nearest_size(x, (12, 7), in_ld=16, in_fill=np.nan)
    util.assert_exact(got.view(np.uint32), ur.upsample_nearest_ref(x, out_hw=(12, 7)).view(np.uint32), "strided input")


def test_nearest_by_scale_factor_still_matches_the_golden(gpu):
    util.assert_exact(hipops.upsample_nearest(GOLD["upsample2/x"], 2.0, 2.0), GOLD["upsample2/y"])


# ---- label map ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("case", ur.LABEL_CASES, ids=["seed%d" % c[0] for c in ur.LABEL_CASES])
def test_label_map(gpu, case, half):
    """the float64 argmax on every pixel outside the near-tie set, whose share is capped (tests/test_upsample_cpu.py counts it)"""
    seed, shape, out_hw, ac = case
    x = ur.label_logits(seed, shape, half)
    labels, near = ur.label_ref(x, out_hw, ac)
    assert near.mean() <= ur.LABEL_TIE_CAP
    got = hipops.segment_labels(x, out_hw, ac)
    assert got.dtype == np.uint8 and got.shape == labels.shape
    wrong = (got != labels) & ~near
    print("seed %d: %d near ties excluded, %d of them differ" % (seed, near.sum(), ((got != labels) & near).sum()))
    assert not wrong.any(), "%d pixels differ outside the near-tie set" % wrong.sum()
    # strided logits: the same labels, bit for bit
    util.assert_exact(hipops.segment_labels(x, out_hw, ac, in_ld=shape[3] + 8, in_fill=np.nan), got, "strided logits")
    # ... and they are the argmax of the copy kernel's own fp32 output (same device function; an fp16 store would round two classes together)
    if not half:
        up = hipops.upsample_bilinear(x, out_hw=out_hw, align_corners=ac)
        util.assert_exact(got, up.argmax(axis=-1).astype(np.uint8), "label map vs argmax of the upsampled logits")


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
def test_label_map_takes_the_lowest_class_on_a_tie(gpu, half):
    x = ur.label_logits(9, (2, 12, 10, 7), half)
    x[..., 5] = x[..., 2]           # two equal channels: every blend of them is equal too
    x[..., 2] += x.dtype.type(8.0)  # ... and they are the largest everywhere
    x[..., 5] = x[..., 2]
    for ac in (False, True):
        got = hipops.segment_labels(x, (50, 37), ac)
        assert (got == 2).all()
    one = hipops.segment_labels(x[..., :1], (20, 20))   # a single class
    assert (one == 0).all()
    wide = ur.label_logits(4, (1, 5, 5, 256), half)
    labels, near = ur.label_ref(wide, (23, 17), True)
    got = hipops.segment_labels(wide, (23, 17), True)
    assert np.array_equal(got[~near], labels[~near]) and got.max() > 127


# ---- engine ---------------------------------------------------------------------------------------------------------------------------
def save(b, tmp_path, tag="m"):
    pp, bp = str(tmp_path / (tag + ".pnnx.param")), str(tmp_path / (tag + ".pnnx.bin"))
    b.save(pp, bp)
    return pp, bp


def run_engine(pp, bp, x, **opts):
    e = Engine(**opts)
    e.load_model(pp, bp)
    e.input(e.input_names()[0], x)
    e.forward()
    return e, e.extract(e.output_names()[0])


def one_op(shape, emit):
    n, h, w, c = shape
    b = mg.PnnxBuilder(seed=5)
    b.output(emit(b, b.input((n, c, h, w))))
    return b


ONE_OP = {
    "upsample_bilinear_ac": ((2, 9, 7, 12), lambda b, x: b.upsample(x, 2.0, mode="bilinear", align_corners=True), dict(scale=2.0), True),
    "upsample_bilinear_noac_x3.7": ((1, 13, 9, 21), lambda b, x: b.upsample(x, 3.7, mode="bilinear", align_corners=False), dict(scale=3.7), False),
    "interpolate_size": ((2, 8, 8, 21), lambda b, x: b.interpolate(x, mode="bilinear", align_corners=False, size=(64, 61)), dict(out_hw=(64, 61)), False),
    "interpolate_scale": ((2, 8, 10, 16), lambda b, x: b.interpolate(x, scale=1.5, mode="bilinear", align_corners=False), dict(scale=1.5), False),
    "interpolate_recompute": ((1, 7, 30, 4), lambda b, x: b.interpolate(x, scale=3.7, mode="bilinear", recompute_scale_factor=True),
                              dict(out_hw=(25, 111)), False),
    "interpolate_none_ac": ((1, 6, 6, 8), lambda b, x: b.interpolate(x, scale=2.0, mode="bilinear"), dict(scale=2.0), False),
    "F_upsample": ((2, 6, 5, 8), lambda b, x: b.interpolate(x, scale=2.0, mode="bilinear", align_corners=True, functional="F.upsample"),
                   dict(scale=2.0), True),
}


@pytest.mark.parametrize("which", sorted(ONE_OP))
def test_engine_one_op_graph(gpu, tmp_path, which):
    """LoadModel -> Forward -> Extract reproduces the op-level result bit for bit (and the reference)"""
    shape, emit, kw, ac = ONE_OP[which]
    pp, bp = save(one_op(shape, emit), tmp_path)
    x = ur.case_input(shape, 9)
    e, got = run_engine(pp, bp, x)
    util.assert_exact(got.view(np.uint32), hipops.upsample_bilinear(x, align_corners=ac, **kw).view(np.uint32), "engine vs op level")
    check_f32(got, ur.upsample_bilinear_ref(x, align_corners=ac, **kw), x, which)
    kernels = [L["kernel"] for L in e.profile() if L["type"] in ur.RESIZE_TYPES]
    assert kernels == ["upsample_bilinear_kernel<float, %d>" % (4 if shape[3] % 4 == 0 else 1)], kernels


def test_engine_nearest_by_size(gpu, tmp_path):
    shape = (2, 6, 5, 8)
    x = ur.case_input(shape, 10)
    for tag, emit in (("module", lambda b, t: b.upsample(t, mode="nearest", size=(13, 9))),
                      ("functional", lambda b, t: b.interpolate(t, mode="nearest", size=(13, 9)))):
        pp, bp = save(one_op(shape, emit), tmp_path, tag)
        e, got = run_engine(pp, bp, x)
        util.assert_exact(got.view(np.uint32), ur.upsample_nearest_ref(x, out_hw=(13, 9)).view(np.uint32), tag)
        assert [L["kernel"] for L in e.profile() if L["type"] in ur.RESIZE_TYPES] == ["upsample_nearest"]
    # the scale-factor form keeps its result (the reference's rule) and its kernel name
    pp, bp = save(one_op(shape, lambda b, t: b.upsample(t, 2.0)), tmp_path, "scale")
    e, got = run_engine(pp, bp, x)
    util.assert_exact(got.view(np.uint32), hipops.upsample_nearest(x, 2.0, 2.0).view(np.uint32), "nearest by scale factor")
    assert [L["kernel"] for L in e.profile() if L["type"] == "nn.Upsample"] == ["upsample_nearest"]


TOY = {"unet_bilinear": lambda batch=2: mg.build_toy_unet(batch=batch, up="bilinear"), "segnet": lambda batch=2: mg.build_toy_segnet(batch=batch)}


def resize_lines(b):
    return [_parse(ln) for ln in b.lines if ln.split()[0] in ur.RESIZE_TYPES]


@pytest.mark.parametrize("which", sorted(TOY))
def test_toy_graph_fp32(gpu, tmp_path, which):
    b = TOY[which]()
    pp, bp = save(b, tmp_path, which)
    x = mg.synth_input((2, 64, 64, 3))
    e, got = run_engine(pp, bp, x)
    ref = ur.eval_graph(b, x)
    print("%s fp32: max-based %.3e, element-wise %.3e" % (which, util.rel_err(got, ref), util.mixed_err(got, ref)))
    util.assert_parity(got, ref, what=which + " fp32")
    prof = [L for L in e.profile() if L["type"] in ur.RESIZE_TYPES]
    assert len(prof) == len(resize_lines(b)) and all(L["kernel"].startswith("upsample_bilinear_kernel<float") for L in prof), prof
    # a captured graph replays the same bits
    _, g = run_engine(pp, bp, x, graph=1)
    util.assert_exact(g.view(np.uint32), got.view(np.uint32), "graph=1 vs eager")


def test_bilinear_output_is_aliased_into_its_concat(gpu, tmp_path):
    """a bilinear upsample whose sole consumer is a channel concat writes straight into the concat buffer, at a stride, bit for bit what the
    schedule without aliasing computes"""
    b = mg.PnnxBuilder(seed=3)
    x = b.input((2, 16, 12, 12))
    low = b.conv(x, 32, 3, 2, 1)
    skip = b.conv(x, 16, 1, 1, 0)
    up = b.upsample(low, 2.0, mode="bilinear", align_corners=False)
    b.output(b.conv(b.cat([skip, up]), 8, 3, 1, 1))
    pp, bp = save(b, tmp_path)
    xin = util.rng_uniform(4, (2, 12, 12, 16), -1.0, 1.0)
    e1, y1 = run_engine(pp, bp, xin)
    e0, y0 = run_engine(pp, bp, xin, alias_cat=0)
    assert up in e1.schedule()["alias"] and up not in e0.schedule()["alias"], (e1.schedule()["alias"], up)
    util.assert_exact(y1.view(np.uint32), y0.view(np.uint32), "alias_cat=1 vs 0")
    util.assert_parity(y1, ur.eval_graph(b, xin), what="bilinear into a concat")


def pan_graph(mode):
    """the YOLO-style top-down step: cat([upsample(low), skip]) read by a 1x1 conv"""
    b = mg.PnnxBuilder(seed=6)
    x = b.input((2, 32, 20, 20))
    low = b.conv(x, 64, 3, 2, 1)
    skip = b.conv(x, 32, 1, 1, 0)
    up = b.upsample(low, 2.0) if mode == "nearest" else b.upsample(low, 2.0, mode="bilinear", align_corners=False)
    b.output(b.conv(b.cat([up, skip]), 64, 1, 1, 0))
    return b


def test_only_nearest_by_scale_is_read_at_the_source(gpu, tmp_path):
    xin = util.rng_uniform(5, (2, 20, 20, 32), -1.0, 1.0)
    for mode in ("nearest", "bilinear"):
        b = pan_graph(mode)
        pp, bp = save(b, tmp_path, mode)
        e, y = run_engine(pp, bp, xin)
        s = e.schedule()
        if mode == "nearest":
            assert "upsample_0" in s["fused"] and not any(n.startswith("upsample") for n in s["run"]), s
        else:
            assert "upsample_0" not in s["fused"] and any(n.startswith("upsample_0") for n in s["run"]), s
            assert any(L["kernel"] == "upsample_bilinear_kernel<float, 4>" for L in e.profile())
        util.assert_parity(y, ur.eval_graph(b, xin), what="PAN step, " + mode)


@pytest.mark.parametrize("which", sorted(TOY))
def test_toy_graph_rebatch(gpu, tmp_path, which):
    """SetOption("batch", 5) on the batch-2 file: per image the same bits as batch-2 runs of the same images"""
    pp, bp = save(TOY[which](), tmp_path, which)
    x5 = util.rng_uniform(21, (5, 64, 64, 3), 0.0, 1.0)
    _, y5 = run_engine(pp, bp, x5, batch=5)
    xs = np.concatenate([x5, x5[:1]], 0)   # pairs (0, 1), (2, 3), (4, 0)
    for i in range(0, 6, 2):
        _, y2 = run_engine(pp, bp, xs[i:i + 2])
        for j in range(2):
            if i + j < 5:
                util.assert_exact(y5[i + j].view(np.uint32), y2[j].view(np.uint32), "image %d" % (i + j))


@pytest.mark.parametrize("which", sorted(TOY))
def test_toy_graph_fp16_storage(gpu, tmp_path, which):
    """fp16=1: the bilinear layers run the fp16 kernel on half tensors with no cast pair around them, and the error against fp64 is at most
    2x that of the fp16-storage emulation (weights, biases, the input and every layer's output rounded to fp16, fp64 arithmetic between)"""
    b = TOY[which]()
    pp, bp = save(b, tmp_path, which)
    x = mg.synth_input((2, 64, 64, 3))
    e, got = run_engine(pp, bp, x, fp16=1)
    prof = e.profile()
    ups = [L for L in prof if L["type"] in ur.RESIZE_TYPES]
    assert len(ups) == len(resize_lines(b)) and all(L["kernel"].startswith("upsample_bilinear_kernel<_Float16") for L in ups), ups
    names = [L["name"] for L in prof]
    for L in ups:   # (InsertFp32Fallbacks names its casts <layer>.in_to_f32.<k> / <layer>.out_to_f16.<k>)
        assert not any(n.startswith(L["name"] + ".in_to_f32") or n.startswith(L["name"] + ".out_to_f16") for n in names), names
    ref = ur.eval_graph(b, x)
    emu = ur.eval_graph(b, x, rnd=round_f16)
    e_engine, e_emu = util.rel_err(got, ref), util.rel_err(emu, ref)
    print("%s fp16 storage vs fp64: engine %.3e, fp16 emulation %.3e" % (which, e_engine, e_emu))
    assert np.isfinite(got).all()
    assert e_engine <= 2.0 * e_emu, (e_engine, e_emu)


def test_refusals_leave_the_process_usable(gpu, tmp_path):
    shape = (1, 6, 6, 8)

    def load(b, tag):
        pp, bp = save(b, tmp_path, tag)
        with pytest.raises(StatusError) as ei:
            Engine().load_model(pp, bp)
        return ei.value.status

    b = one_op(shape, lambda b, x: b.upsample(x, 2.0, mode="bilinear", align_corners=False))
    b.lines = [ln.replace("mode=bilinear", "mode=bicubic") for ln in b.lines]
    assert load(b, "bicubic") == Status.kUnsupport
    # an output shape that disagrees with size= / with floor(in * scale_factor)
    b = one_op(shape, lambda b, x: b.interpolate(x, mode="bilinear", align_corners=False, size=(20, 20)))
    b.lines = [ln.replace("(1,8,20,20)f32", "(1,8,20,21)f32") for ln in b.lines]
    assert load(b, "badsize") == Status.kErrorShape
    b = one_op(shape, lambda b, x: b.upsample(x, 1.5, mode="bilinear", align_corners=True))
    b.lines = [ln.replace("(1,8,9,9)f32", "(1,8,10,9)f32") for ln in b.lines]
    assert load(b, "badscale") == Status.kErrorShape
    b = one_op(shape, lambda b, x: b.upsample(x, mode="nearest", size=(9, 9)))
    b.lines = [ln.replace("(1,8,9,9)f32", "(1,8,9,8)f32") for ln in b.lines]
    assert load(b, "badnearest") == Status.kErrorShape
    # nearest has no align_corners=True (torch refuses it)
    b = one_op(shape, lambda b, x: b.upsample(x, 2.0, mode="nearest", align_corners=True))
    assert "align_corners=True mode=nearest" in "\n".join(b.lines)
    assert load(b, "nearest_ac") == Status.kUnsupport
    # F.interpolate on a rank-3 tensor
    b = mg.PnnxBuilder()
    x = b._new_operand((1, 8, 6))
    b._emit("pnnx.Input", "pnnx_input_0", [], [x])
    y = b._new_operand((1, 8, 12))
    b._emit("F.interpolate", "F_interpolate_0", [x], [y], dict(align_corners="None", mode="nearest", recompute_scale_factor="None",
                                                               scale_factor=(2.0,), size="None"))
    b.output(y)
    assert load(b, "rank3") == Status.kUnsupport
    # ... and the same process loads and runs a good model afterwards
    good_shape, emit, kw, ac = ONE_OP["interpolate_size"]
    pp, bp = save(one_op(good_shape, emit), tmp_path, "good")
    xin = ur.case_input(good_shape, 1)
    _, out = run_engine(pp, bp, xin)
    check_f32(out, ur.upsample_bilinear_ref(xin, align_corners=ac, **kw), xin, "after the refusals")
