"""GPU: the deformable-convolution kernel (include/si_deform.h) and torchvision.ops.DeformConv2d.  Kernel: every case of
tests/deform_reference.py against the float64 rule at the fp32 bar, the fused activations, special values, bit-for-bit independence, views
under guard bands.  Layer and engine: one-operator graphs with two and three graph inputs, both toys in fp32 and under fp16 storage, the fused
ReLU, the offset operand as a view, captured, re-batched, batch-split; refusals at load.  Every engine test fails without the layer (LoadModel
rejects the type with kEmpty), every op-level test without the kernel (the symbols are missing)."""
import numpy as np
import pytest

import containment as ct
import deform_reference as dr
import util
from ct_reference import _parse
from simpleinfer_amd import hipops, modelgen as mg
from simpleinfer_amd.engine import Engine, Status, StatusError

pytestmark = pytest.mark.gpu

VEC, SCALAR = "deform_conv_f32_kernel<true>", "deform_conv_f32_kernel<false>"
ARM = {1: VEC, 2: VEC, 3: SCALAR, 4: SCALAR, 5: SCALAR, 6: VEC, 7: SCALAR, 8: VEC, 9: SCALAR, 10: VEC}
CASE_IDS = ["%d_%s" % (i + 1, dr.case_id(c)) for i, c in enumerate(dr.CASES)]


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))
    assert bad[0].size == 0, "%s: %d of %d elements differ in bits, first at %s" % (what, bad[0].size, got.size, tuple(int(b[0]) for b in bad))


def run_op(c, ops, act="none", act_param=0.0, **views):
    x, off, m, w, b = ops
    return hipops.deform_conv2d(x, off, w, b, m, c[1], c[2], c[3], c[6], act, act_param, **views)


def parity_with_masks(got, ref, what):
    """the NaN and Inf positions equal the reference's, everything else at the fp32 bar"""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "%s: NaN masks differ (%d vs %d)" % (what, np.isnan(got).sum(), np.isnan(ref).sum())
    inf = np.isinf(ref)
    assert np.array_equal(got[inf], ref[inf].astype(np.float32)), what + ": Inf positions differ"
    ok = np.isfinite(ref)
    util.assert_parity(np.where(ok, got, 0.0), np.where(ok, ref, 0.0), what=what)


# ---- the kernel against float64 -----------------------------------------------------------------------------------------------
_REF = {}


def case_with_ref(index):
    """(case, operands, float64 reference), computed once and shared"""
    if index not in _REF:
        c = dr.CASES[index - 1]
        ops = dr.operands(c, seed=100 * index)
        ref = dr.run_ref(c, ops)
        ref.setflags(write=False)
        _REF[index] = (c, ops, ref)
    return _REF[index]


@pytest.mark.parametrize("index", range(1, len(dr.CASES) + 1), ids=CASE_IDS)
def test_cases_against_float64(gpu, index):
    c, ops, ref = case_with_ref(index)
    got = run_op(c, ops)
    assert hipops.LAST_KERNEL_NAME["si_hip_deform_conv2d"] == ARM[index]
    print("deform conv case %d: max-based %.3e, element-wise %.3e" % (index, util.rel_err(got, ref), util.mixed_err(got, ref)))
    util.assert_parity(got, ref, what="deform conv case %d" % index)


@pytest.mark.parametrize("act", sorted(a for a in hipops.ACT if a != "none"))
@pytest.mark.parametrize("index", [1, 4])
def test_fused_activations(gpu, index, act):
    c, ops, _ = case_with_ref(index)
    p = 0.1 if act == "leakyrelu" else 0.0
    util.assert_parity(run_op(c, ops, act, p), dr.run_ref(c, ops, act, p), what="case %d, %s" % (index, act))


# ---- special values -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", [4, 3], ids=["vector_arm", "scalar_arm"])
def test_boundary_coordinates(gpu, ci):
    """1x1 kernel: y = -1, y = H, x = W exactly, -0.5 and H - 0.5 (half the edge row), +-1e30 and +-Inf, integer positions on the last row"""
    h, w, co = 4, 5, 3
    x = util.rng_uniform(1, (1, h, w, ci), -1.0, 1.0)
    wt = util.rng_uniform(2, (co, ci, 1, 1), -1.0, 1.0)
    ho, wo = np.meshgrid(np.arange(h, dtype=np.float32), np.arange(w, dtype=np.float32), indexing="ij")
    zero = np.zeros((h, w), np.float32)
    settings = [("y = -1", -1 - ho, zero), ("y = H", h - ho, zero), ("x = W", zero, w - wo), ("x = -1", zero, -1 - wo), ("y = -0.5", -0.5 - ho, zero),
                ("y = H - 0.5", h - 0.5 - ho, zero), ("x = W - 0.5", zero, w - 0.5 - wo), ("integer", zero, zero), ("last row", h - 1 - ho, w - 1 - wo)]
    settings += [("dy %r" % v, zero + np.float32(v), zero) for v in (1e30, -1e30, np.inf, -np.inf)]
    settings += [("dx %r" % v, zero, zero + np.float32(v)) for v in (1e30, -1e30, np.inf, -np.inf)]
    for what, dy, dx in settings:
        off = np.stack([dy, dx], -1)[None].astype(np.float32)
        ref = dr.deform_conv2d_ref(x, off, wt)
        got = hipops.deform_conv2d(x, off, wt)
        assert hipops.LAST_KERNEL_NAME["si_hip_deform_conv2d"] == (VEC if ci == 4 else SCALAR)
        if not ref.any():
            assert not got.any(), what                  # out of range is exactly 0
        else:
            util.assert_parity(got, ref, what=what)


@pytest.mark.parametrize("index", [4, 10, 5])
def test_a_nan_offset_poisons_its_group_at_its_pixel(gpu, index):
    c, ops, _ = case_with_ref(index)
    x, off, m, w, b = ops
    taps, og = c[0][0] * c[0][1], c[7]
    off = off.copy()
    off[c[4][0] - 1, 1, 2, 2 * ((og - 1) * taps + taps // 2) + 1] = np.nan
    off[0, 0, 0, 0] = np.nan
    ref = dr.run_ref(c, (x, off, m, w, b))
    assert 0 < np.isnan(ref).sum() < ref.size // 4
    parity_with_masks(run_op(c, (x, off, m, w, b)), ref, "NaN offsets, case %d" % index)


@pytest.mark.parametrize("index", [1, 3])
def test_inf_in_x_under_a_zero_weight(gpu, index):
    """integer offsets: the three neighbours of the sampled pixel have weight 0 and are still multiplied where they are inside the image"""
    c, ops, _ = case_with_ref(index)
    x, off, m, w, b = ops
    x, off = x.copy(), np.round(off)
    x[0, 2, 3, 1] = np.inf
    x[0, 4, 2, 5] = -np.inf
    ref = dr.run_ref(c, (x, off, m, w, b))
    assert np.isnan(ref).any() and np.isfinite(ref).any()
    parity_with_masks(run_op(c, (x, off, m, w, b)), ref, "Inf in x, case %d" % index)


def test_independence_bit_for_bit(gpu):
    c, ops, _ = case_with_ref(10)
    x, off, m, w, b = ops
    full = run_op(c, ops)
    same_bits(run_op(c, ops), full, "two launches")
    for i in range(c[4][0]):       # M = 132: item 1 starts at row 44 of the first tile and item 2 spans the first two
        same_bits(run_op(c, (x[i:i + 1], off[i:i + 1], m[i:i + 1], w, b)), full[i:i + 1], "batch item %d alone" % i)


# ---- views and containment ----------------------------------------------------------------------------------------------------
class ViewCase:
    entries = ("si_hip_deform_conv2d_f32",)

    def __init__(self, vid, index, **views):
        self.id, self.index, self.views = vid, index, views

    def run(self, fill):
        c, ops, _ = case_with_ref(self.index)
        fills = dict(in_fill=fill, off_fill=fill, out_fill=fill)
        if ops[2] is not None:
            fills["mask_fill"] = fill
        full = run_op(c, ops, "silu", full=True, **fills, **self.views)
        return ct.Out("y", full, self.views.get("out_c_off", 0), c[5][1])


VIEW_CASES = [
    # the vector arm keeps its arm inside a wider row (a 16-byte aligned slice); offset, mask and out at odd element offsets
    ViewCase("dcnv2_vector_arm", 1, in_ld=24, in_c_off=4, off_ld=21, off_c_off=2, mask_ld=13, mask_c_off=3, out_ld=23, out_c_off=5),
    # ... and falls to the scalar arm on a slice that is not
    ViewCase("dcnv2_slice_off_16_bytes", 1, in_ld=19, in_c_off=3, off_ld=18, off_c_off=0, mask_ld=16, mask_c_off=7, out_ld=16, out_c_off=0),
    ViewCase("straddling_offset_groups", 4, in_ld=39, in_c_off=2, off_ld=40, off_c_off=4, mask_ld=19, mask_c_off=1, out_ld=8, out_c_off=3),
    ViewCase("dcnv1_one_past_a_tile", 3, in_ld=20, in_c_off=3, off_ld=5, off_c_off=3, out_ld=70, out_c_off=5),
    ViewCase("grouped_last_slices", 10, in_ld=48, in_c_off=8, off_ld=44, off_c_off=8, mask_ld=20, mask_c_off=2, out_ld=80, out_c_off=8),
    ViewCase("one_pixel", 6, in_ld=8, in_c_off=4, off_ld=19, off_c_off=1, out_ld=7, out_c_off=3),
]


@pytest.mark.parametrize("case", VIEW_CASES, ids=[c.id for c in VIEW_CASES])
def test_views_and_containment(gpu, case):
    del hipops.LAST_ENTRIES[:]
    c, ops, _ = case_with_ref(case.index)
    dense = run_op(c, ops, "silu")
    util.assert_parity(dense, dr.run_ref(c, ops, "silu"), what=case.id + ", dense")
    plain = case.run(hipops.ByteFill(0x00))
    assert set(case.entries) <= set(hipops.LAST_ENTRIES), hipops.LAST_ENTRIES
    vec = ARM[case.index] == VEC and case.views["in_ld"] % 4 == 0 and case.views["in_c_off"] % 4 == 0
    assert hipops.LAST_KERNEL_NAME["si_hip_deform_conv2d"] == (VEC if vec else SCALAR)
    ct.assert_outside_fill(plain.full, plain.c_off, plain.c, 0x00, case.id + ", plain run")
    check = same_bits if vec == (ARM[case.index] == VEC) else (lambda g, w, what: util.assert_parity(g, w, what=what))
    check(plain.full[..., plain.c_off:plain.c_off + plain.c], dense, case.id + " against the dense run")
    for byte in ct.PATTERNS:      # 0xFF: the gaps between the inputs' channels hold NaN; 0x7B: a large finite sentinel
        with hipops.guard_bands(byte) as g:      # all bands and the inputs are compared when the block ends
            out = case.run(hipops.ByteFill(byte))
        what = "%s under 0x%02X" % (case.id, byte)
        assert g.checked == 4 + (ops[2] is not None) + (ops[4] is not None), "%s: the guard saw %d buffers" % (what, g.checked)
        ct.assert_outside_fill(out.full, out.c_off, out.c, byte, what)             # every byte outside the output view unchanged
        same_bits(out.full[..., out.c_off:out.c_off + out.c], plain.full[..., plain.c_off:plain.c_off + plain.c], what)


# ---- layer and engine ---------------------------------------------------------------------------------------------------------
def save(b, tmp_path, tag):
    pp, bp = str(tmp_path / (tag + ".pnnx.param")), str(tmp_path / (tag + ".pnnx.bin"))
    b.save(pp, bp)
    return pp, bp


def run_engine(b, tmp_path, xs, tag="m", forwards=1, **opts):
    """(engine, the graph output as the engine stores it); xs: one array per graph input, in order"""
    pp, bp = save(b, tmp_path, tag)
    e = Engine(**opts)
    e.load_model(pp, bp)
    xs = xs if isinstance(xs, (list, tuple)) else [xs]
    for name, x in zip(e.input_names(), xs):
        e.input(name, x)
    for _ in range(forwards):
        e.forward()
    (out,) = [_parse(ln)[2][0] for ln in b.lines if ln.startswith("pnnx.Output")]
    return e, e.extract(out)


def nchw(shape_nhwc):
    n, h, w, c = shape_nhwc
    return (n, c, h, w)


def one_op(index, act=None, shapes=None):
    """the case as a graph whose operands are all graph inputs; shapes: NHWC overrides of (x, offset, mask) for the refusal tests"""
    c = dr.CASES[index - 1]
    k, s, p, d, (n, h, w), (ci, co), g, og, mask, bias = c
    x, off, m, _, _ = dr.operands(c, seed=100 * index)
    sh = [x.shape, off.shape] + ([m.shape] if mask else [])
    if shapes:
        sh = [o or v for o, v in zip(shapes, sh)]
    b = mg.PnnxBuilder(seed=index)
    ins = [b.input(nchw(v)) for v in sh]
    y = b.deform_conv(*ins, cout=co, k=k, s=s, p=p, d=d, groups=g, bias=bias)
    if act:
        y = getattr(b, act)(y)
    b.output(y)
    return b, [x, off] + ([m] if mask else [])


def layer_ref(b, xs, c, act="none"):
    name = [_parse(ln)[1] for ln in b.lines if ln.startswith(dr.TYPE)][0]
    return dr.deform_conv2d_ref(xs[0], xs[1], b.attrs[name + ".weight"], b.attrs.get(name + ".bias"), xs[2] if len(xs) == 3 else None, c[1], c[2], c[3],
                                c[6], act)


@pytest.mark.parametrize("index", [2, 1, 10, 5], ids=["two_inputs", "three_inputs", "grouped_three_inputs", "rect_two_inputs"])
def test_layer_in_a_one_operator_graph(gpu, tmp_path, index):
    b, xs = one_op(index)
    c = dr.CASES[index - 1]
    assert len(xs) == (3 if c[8] else 2)
    eng, got = run_engine(b, tmp_path, xs)
    util.assert_parity(got, layer_ref(b, xs, c), what="DeformConv2d layer, case %d" % index)
    name = [_parse(ln)[1] for ln in b.lines if ln.startswith(dr.TYPE)][0]
    same_bits(got, hipops.deform_conv2d(xs[0], xs[1], b.attrs[name + ".weight"], b.attrs.get(name + ".bias"), xs[2] if len(xs) == 3 else None, c[1],
                                        c[2], c[3], c[6]), "the layer against the op-level entry")
    (layer,) = [L for L in eng.profile() if L["type"] == dr.TYPE]
    assert layer["kernel"] == ARM[index], layer
    k, (ci, co), (n, oh, ow, _) = c[0], c[5], got.shape
    assert layer["flops"] == 2.0 * n * oh * ow * co * (ci // c[6]) * k[0] * k[1]
    assert layer["bytes"] == 4.0 * (sum(x.size for x in xs) + got.size + b.attrs[name + ".weight"].size + (co if c[9] else 0))


def test_relu_is_fused_into_the_epilogue(gpu, tmp_path):
    b, xs = one_op(1, act="relu")
    ref = layer_ref(b, xs, dr.CASES[0], "relu")
    e1, y1 = run_engine(b, tmp_path, xs, fuse=1)
    e0, y0 = run_engine(b, tmp_path, xs, fuse=0)
    util.assert_parity(y1, ref, what="fuse=1")
    util.assert_parity(y0, ref, what="fuse=0")
    assert "relu_0" in e1.schedule()["fused"] and "relu_0" not in e0.schedule()["fused"]
    p1, p0 = e1.profile(), e0.profile()
    assert len(p1) == len(p0) - 1, (p1, p0)
    assert any(L["type"] == dr.TYPE and L["kernel"] == VEC for L in p1), p1


TOYS = {"dcnv2": dict(mask=True), "dcnv1": dict(mask=False)}


def toy_input(b):
    n, c, h, w = b.shapes["0"]
    return mg.synth_input((n, h, w, c))


@pytest.mark.parametrize("which", sorted(TOYS))
def test_toys_fp32(gpu, tmp_path, which):
    b = mg.build_toy_dcn_head(**TOYS[which])
    x = toy_input(b)
    want = dr.eval_graph(b, x)
    eng, got = run_engine(b, tmp_path, x)
    util.assert_parity(got, want, what="toy " + which)
    prof = eng.profile()
    (layer,) = [L for L in prof if L["type"] == dr.TYPE]
    assert layer["kernel"] == VEC, layer
    assert "relu_0" in eng.schedule()["fused"] and not [L for L in prof if L["type"] == "nn.ReLU"]
    _, cap = run_engine(b, tmp_path, x, forwards=3, graph=1)
    same_bits(cap, got, which + ": graph=1 replay over three forwards")
    _, plain = run_engine(b, tmp_path, x, fuse=0, alias_split=0, alias_cat=0)
    util.assert_parity(plain, want, what="toy %s, fuse=0 alias_split=0" % which)


def test_the_offset_operand_is_a_view(gpu, tmp_path):
    """the DCNv2 toy: the 18 offset channels are read in place from the offset conv's 27-channel rows (pixel stride 27).  The 9 mask logits start
    72 bytes into the row, which the planner's 16-byte rule for views copies; a block whose pieces all start on 16 bytes launches nothing"""
    b = mg.build_toy_dcn_head()
    x = toy_input(b)
    want = dr.eval_graph(b, x)
    split = [_parse(ln) for ln in b.lines if ln.startswith("torch.split")][0]
    e1, y1 = run_engine(b, tmp_path, x, alias_split=1)
    e0, y0 = run_engine(b, tmp_path, x, alias_split=0)
    assert split[3][0] in e1.schedule()["alias"] and split[3][0] not in e0.schedule()["alias"]
    util.assert_parity(y1, want, what="offset as a view")
    util.assert_parity(y0, want, what="offset copied")
    # two deformable convs with two offset groups each on the halves of one 72-channel offset conv: both halves are views, no slice launch
    b2 = mg.PnnxBuilder(seed=2)
    f = b2.silu(b2.conv(b2.input((2, 3, 16, 16)), 16, 3, 2, 1))
    lo, hi = b2.chunk(b2.conv(f, 72, 3, 1, 1), 2, 1)
    b2.output(b2.conv(b2.add(b2.deform_conv(f, lo, cout=8, k=3, p=1), b2.deform_conv(f, hi, cout=8, k=3, p=1)), 8, 1))
    x2 = toy_input(b2)
    e2, y2 = run_engine(b2, tmp_path, x2, tag="halves", alias_split=1)
    (step,) = [L for L in e2.profile() if L["type"] == "torch.chunk"]
    assert step["kernel"] == "view" and {lo, hi} <= set(e2.schedule()["alias"]), (step, e2.schedule()["alias"])
    e3, y3 = run_engine(b2, tmp_path, x2, tag="halves", alias_split=0)
    (step,) = [L for L in e3.profile() if L["type"] == "torch.chunk"]
    assert step["kernel"] == "split_channels", step
    same_bits(y2, y3, "views against copies")          # (the kernel takes the same arm on either: the bits do not depend on the pixel stride)


def test_toy_rebatched(gpu, tmp_path):
    b2, b4 = mg.build_toy_dcn_head(batch=2), mg.build_toy_dcn_head(batch=4)
    x = toy_input(b4)
    _, want = run_engine(b4, tmp_path, x, tag="b4")
    eng, got = run_engine(b2, tmp_path, x, tag="b2", batch=4)
    same_bits(got, want, "batch=4 on the batch-2 file")
    dcn = [_parse(ln) for ln in b2.lines if ln.startswith(dr.TYPE)][0]
    assert eng.operand_shape(dcn[3][0])[0] == 4


@pytest.mark.parametrize("mode", ["host_slices2", "streams2"])
def test_toy_batch_split(gpu, tmp_path, mode):
    """as tests/test_gpu_batch_split.py for its toys: the split run has the bits of the unsplit one, and it really was split"""
    b = mg.build_toy_dcn_head(batch=4)
    x = toy_input(b)
    e0, base = run_engine(b, tmp_path, x, host_slices=1, streams=1)
    opts, slices, lanes = {"host_slices2": (dict(host_slices=2), 2, 1), "streams2": (dict(streams=2), 1, 2)}[mode]
    e1, got = run_engine(b, tmp_path, x, **opts)
    sched = e1.schedule()
    assert sched["batch_mixing"] == [] and sched["host_slices"] == slices and sched["lanes"] == lanes, sched
    same_bits(got, base, mode)


@pytest.mark.parametrize("which", sorted(TOYS))
def test_toys_fp16_storage(gpu, tmp_path, which):
    """fp16=1: the engine loads, the deformable conv runs its fp32 kernel between casts, and the error against float64 is at most 2x that of the
    fp16-storage emulation (weights, biases, the input and every layer's output rounded to fp16, float64 arithmetic between): the bar of
    test_toy_unet_fp16_storage"""
    b = mg.build_toy_dcn_head(**TOYS[which])
    x = toy_input(b)
    eng, got = run_engine(b, tmp_path, x, fp16=1)
    (layer,) = [L for L in eng.profile() if L["type"] == dr.TYPE]
    assert layer["kernel"] in (VEC, SCALAR), layer
    ref, emu = dr.eval_graph(b, x), dr.eval_graph(b, x, rnd=dr.round_f16)
    e_engine, e_emu = util.rel_err(got, ref), util.rel_err(emu, ref)
    print("toy %s fp16 storage vs float64: engine %.3e, fp16 emulation %.3e" % (which, e_engine, e_emu))
    assert np.isfinite(got).all()
    assert e_engine <= 2.0 * e_emu, (e_engine, e_emu)


def test_refused_at_load(gpu, tmp_path):
    """kErrorShape with a logged reason at LoadModel; the process goes on"""
    def load(b, tag):
        pp, bp = save(b, tmp_path, tag)
        with pytest.raises(StatusError) as ei:
            Engine().load_model(pp, bp)
        return ei.value.status

    # case 1: x [2, 8, 8, 16], offset [2, 8, 8, 18], mask [2, 8, 8, 9]
    assert load(one_op(1, shapes=[None, (2, 8, 8, 20), None])[0], "off_c") == Status.kErrorShape        # no multiple of 2 kh kw
    assert load(one_op(1, shapes=[None, (2, 8, 8, 54), (2, 8, 8, 27)])[0], "og") == Status.kErrorShape    # 3 offset groups, 16 channels
    assert load(one_op(1, shapes=[None, None, (2, 8, 8, 10)])[0], "mask_c") == Status.kErrorShape
    assert load(one_op(1, shapes=[None, (2, 7, 8, 18), None])[0], "off_h") == Status.kErrorShape
    assert load(one_op(1, shapes=[None, None, (2, 8, 7, 9)])[0], "mask_w") == Status.kErrorShape
    b, xs = one_op(1)
    b.lines = [" ".join(t for t in ln.split() if not t.startswith("stride=")) if ln.startswith(dr.TYPE) else ln for ln in b.lines]
    assert load(b, "missing") == Status.kFail
    b, xs = one_op(1)
    _, got = run_engine(b, tmp_path, xs)
    util.assert_parity(got, layer_ref(b, xs, dr.CASES[0]), what="after the refusals")
