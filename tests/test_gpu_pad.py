"""GPU: the explicit pads -- si_hip_pad2d_f32 / _f16 (include/si_pad.h) against the numpy index-map reference
(tests/pad_reference.py) by equality of BITS on random bit patterns: all four modes, vector and scalar forms, negative pads, the
constant, strided views under guard bands, determinism, the refusals; and the layers inside the engine: one-op graphs for the six
type strings and nn.Tanh, a pad feeding a concat, the toy CycleGAN generator in fp32, under graph capture, re-batched, and with
fp16 storage.  Every engine test fails without the layers (LoadModel rejects the types), every op-level test without the kernel
(the symbols are missing)."""
import ctypes as C

import numpy as np
import pytest

import containment as ct
import pad_reference as pr
import util
from ct_reference import _parse
from simpleinfer_amd import _native, hipops, modelgen as mg
from simpleinfer_amd.engine import Engine, Status, StatusError

pytestmark = pytest.mark.gpu

DTYPES = {"f32": np.float32, "f16": np.float16}


def bit_patterns(seed, shape, dtype):
    """random BITS viewed as the float type: NaNs of every payload, infinities, denormals and -0.0 are among them"""
    r = np.random.Generator(np.random.Philox(seed))
    if dtype == np.float32:
        return r.integers(0, 2 ** 32, shape, dtype=np.uint32).view(np.float32)
    return r.integers(0, 2 ** 16, shape, dtype=np.uint16).view(np.float16)


def form(dtype, vec):
    if dtype == np.float32:
        return "pad2d_kernel<float, 4>" if vec else "pad2d_kernel<float, 1>"
    return "pad2d_kernel<_Float16, 8>" if vec else "pad2d_kernel<_Float16, 1>"


def vectorised(c, dtype):
    return c % (16 // np.dtype(dtype).itemsize) == 0


# (NHWC shape, (l, r, t, b), modes or None: every mode the acceptance set has for it)
TABLE = [
    ((1, 1, 1, 4), (2, 1, 1, 2), None),               # a single pixel: constant and replicate (circular and reflect are over their limits)
    ((1, 1, 1, 4), (1, 1, 1, 1), ("circular",)),      # ... and circular at its limit, pad = size = 1
    ((1, 2, 2, 4), (1, 1, 1, 1), None),               # the largest legal reflect pad
    ((2, 5, 4, 8), (3, 0, 0, 4), None),
    ((2, 5, 4, 8), (1, 2, 0, 3), None),               # asymmetric, zero sides
    ((1, 4, 4, 4), (4, 4, 4, 4), ("circular", "constant", "replicate")),   # pad = size
    ((2, 6, 7, 3), (3, 3, 3, 3), None),               # scalar form, the RGB stem
    ((1, 9, 5, 21), (1, 2, 2, 1), None),              # scalar, odd c
    ((2, 8, 8, 12), (1, 1, 1, 1), None),              # fp16: c % 8 != 0, the scalar half form (fp32: vectors)
    ((3, 16, 16, 64), (1, 1, 1, 1), None),            # vector form, the residual-block case; 288 items per row: two workgroups
    ((1, 3, 40, 7), (2, 3, 1, 0), None),              # scalar form with 315 items per row: two workgroups, the second partly idle
    ((1, 11, 6, 8), (0, 0, 1, 1), None),              # 13 output rows: the last row group has one row
    ((2, 5, 4, 8), (-1, 2, -2, 1), ("constant",)),    # negative pads crop
    ((2, 5, 4, 8), (-1, 3, 1, -2), ("reflect",)),
    ((2, 5, 4, 8), (-3, 5, -4, 6), ("replicate",)),
    ((1, 4, 4, 4), (-1, -1, -1, -1), None),           # pure crop
    ((2, 5, 4, 8), (0, 0, 0, 0), None),               # a copy
]
CASES = [(s, p, m) for s, p, modes in TABLE for m in (modes or pr.MODES) if pr.accepts(s[1], s[2], p, m)]
assert all(pr.accepts(s[1], s[2], p, m) for s, p, modes in TABLE if modes for m in modes)


def case_id(c):
    s, p, m = c
    return "%dx%dx%dx%d_%s_%s" % (s + (m, "_".join(str(v).replace("-", "m") for v in p)))


FORMS_SEEN = set()


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_op_moves_the_bits_of_the_reference(gpu, case, dt):
    s, pads, mode = case
    dtype = DTYPES[dt]
    x = bit_patterns(17, s, dtype)
    got = hipops.pad2d(x, pads, mode, 1.5)
    kernel = hipops.LAST_KERNEL_NAME["si_hip_pad2d"]
    FORMS_SEEN.add(kernel)
    assert got.dtype == dtype
    assert kernel == form(dtype, vectorised(s[3], dtype)), kernel
    ct.assert_same_bits(got, pr.pad2d_ref(x, pads, mode, 1.5), "%s %s [%s]" % (case_id(case), dt, kernel))


def test_both_forms_ran(gpu):
    """the names reported over the case list include the vector and the scalar form of both types (runs after the parametrised test above,
    whose names it collects)"""
    if len(FORMS_SEEN) < 4:
        for dtype in DTYPES.values():
            for s in ((3, 16, 16, 64), (2, 6, 7, 3)):
                hipops.pad2d(bit_patterns(1, s, dtype), (1, 1, 1, 1), "reflect")
                FORMS_SEEN.add(hipops.LAST_KERNEL_NAME["si_hip_pad2d"])
    assert FORMS_SEEN == {form(d, v) for d in DTYPES.values() for v in (True, False)}, FORMS_SEEN


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("value", [1.5, -0.0, 0.1, float("inf")], ids=["1.5", "minus_zero", "0.1", "inf"])
@pytest.mark.parametrize("s", [(2, 5, 4, 8), (2, 6, 7, 3)], ids=["vector", "scalar"])
def test_constant_value(gpu, s, value, dt):
    """the constant arrives with its bits (the sign of -0.0); the fp16 entry rounds it once, to nearest even: 0.1 -> 0x2E66"""
    dtype = DTYPES[dt]
    x = bit_patterns(5, s, dtype)
    got = hipops.pad2d(x, (2, 1, 1, 2), "constant", value)
    ct.assert_same_bits(got, pr.pad2d_ref(x, (2, 1, 1, 2), "constant", value), "value %r" % value)
    want = np.float32(value) if dtype == np.float32 else np.float16(np.float32(value))
    corner = got[0, 0, 0, :]
    assert (corner.view(np.uint32 if dtype == np.float32 else np.uint16) == want.view(np.uint32 if dtype == np.float32 else np.uint16)).all(), corner
    if dtype == np.float16 and value == 0.1:
        assert int(want.view(np.uint16)) == 0x2E66
    if value == 0.0:
        assert np.signbit(corner).all()


# ---- views and containment: checks (a) - (d) of tests/test_gpu_containment.py ---------------------------------------------------------
class ViewCase:
    def __init__(self, cid, half, s, pads, mode, value, vec, **views):
        self.id, self.half, self.s, self.pads, self.mode, self.value, self.vec, self.views = cid, half, s, pads, mode, value, vec, views
        self.entries = ("si_hip_pad2d_f16" if half else "si_hip_pad2d_f32",)
        self.dtype = np.float16 if half else np.float32

    def input(self):
        return bit_patterns(23, self.s, self.dtype)

    def run(self, F):
        y = hipops.pad2d(self.input(), self.pads, self.mode, self.value, in_fill=F, out_fill=F, full=True, **self.views)
        return ct.Out("y", y, self.views.get("out_c_off", 0), self.s[3])


VIEW_CASES = []
for _half, _sfx in ((False, "f32"), (True, "f16")):
    VIEW_CASES += [
        # an input embedded at a channel offset of a wider buffer, an output slice of a wider buffer; 16-byte aligned on both sides
        ViewCase("vector_" + _sfx, _half, (2, 5, 4, 8), (1, 2, 1, 1), "reflect", 0.0, True, in_ld=24, in_c_off=8, out_ld=32, out_c_off=16),
        # odd offsets and strides, the constant among the outputs, a crop on two sides
        ViewCase("scalar_" + _sfx, _half, (2, 6, 7, 3), (-1, 2, 3, -2), "constant", 1.5, False, in_ld=5, in_c_off=2, out_ld=7, out_c_off=3),
        # a stride that forces the scalar form on vector-sized channels: in_ld = c + 1
        ViewCase("odd_stride_" + _sfx, _half, (1, 4, 4, 8), (4, 4, 4, 4), "circular", 0.0, False, in_ld=9, in_c_off=0, out_ld=16, out_c_off=8),
        # the input slice ends where its buffer ends
        ViewCase("last_slice_" + _sfx, _half, (1, 9, 5, 21), (1, 2, 2, 1), "replicate", 0.0, False, in_ld=29, in_c_off=8, out_ld=21, out_c_off=0),
    ]


@pytest.mark.parametrize("case", VIEW_CASES, ids=[c.id for c in VIEW_CASES])
def test_views_and_containment(gpu, case):
    del hipops.LAST_ENTRIES[:]
    plain = case.run(hipops.ByteFill(0x00))
    plain_kernel = hipops.LAST_KERNEL_NAME["si_hip_pad2d"]
    assert set(case.entries) <= set(hipops.LAST_ENTRIES), hipops.LAST_ENTRIES
    assert plain_kernel == form(case.dtype, case.vec), plain_kernel
    ct.assert_outside_fill(plain.full, plain.c_off, plain.c, 0x00, case.id + ", plain run")
    # the value too: nothing of the gaps between the input's pixels reached the output
    ct.assert_same_bits(plain.dest, pr.pad2d_ref(case.input(), case.pads, case.mode, case.value), case.id + " vs the reference")
    for byte in ct.PATTERNS:
        with hipops.guard_bands(byte) as g:      # (a) all bands and (d) the input are compared when the block ends
            out = case.run(hipops.ByteFill(byte))
        what = "%s under 0x%02X" % (case.id, byte)
        assert g.checked == 2, "%s: the guard saw %d buffers" % (what, g.checked)   # x, y
        assert hipops.LAST_KERNEL_NAME["si_hip_pad2d"] == plain_kernel, what
        ct.assert_outside_fill(out.full, out.c_off, out.c, byte, what)                              # (b)
        ct.assert_same_bits(out.dest, plain.dest, what + ": guarded + pattern-filled vs plain")    # (c)


# ---- determinism ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("s", [(3, 16, 16, 64), (2, 6, 7, 3)], ids=["vector", "scalar"])
def test_same_bits_twice(gpu, s, dt):
    x = bit_patterns(29, s, DTYPES[dt])
    ct.assert_same_bits(hipops.pad2d(x, (2, 1, 1, 2), "reflect"), hipops.pad2d(x, (2, 1, 1, 2), "reflect"), "two launches")


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("s", [(5, 16, 16, 64), (5, 6, 7, 3)], ids=["vector", "scalar"])
def test_batch_of_5_has_the_bits_of_single_images(gpu, s, dt):
    x = bit_patterns(31, s, DTYPES[dt])
    y5 = hipops.pad2d(x, (1, 2, 2, 1), "reflect")
    for i in range(5):
        ct.assert_same_bits(y5[i:i + 1], hipops.pad2d(x[i:i + 1], (1, 2, 2, 1), "reflect"), "image %d" % i)


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


def one_op_graph(s, *a, **kw):
    """input -> one pad (PnnxBuilder.pad's arguments) -> output, for an NHWC shape"""
    n, h, w, c = s
    b = mg.PnnxBuilder(seed=5)
    b.output(b.pad(b.input((n, c, h, w)), *a, **kw))
    return b


def test_refusals_leave_the_process_usable(gpu, tmp_path):
    x = bit_patterns(3, (1, 4, 4, 8), np.float32)
    with pytest.raises(hipops.HipError):
        hipops.pad2d(x, (4, 0, 0, 0), "reflect")                  # reflect with pad = size
    with pytest.raises(hipops.HipError):
        hipops.pad2d(x, (-1, 1, 0, 0), "circular")                # circular with a negative pad
    with pytest.raises(hipops.HipError):
        hipops.pad2d(bit_patterns(3, (1, 4, 4, 8), np.float16), (0, 0, 5, 0), "circular")
    d = hipops.pad2d_desc(x.shape, (1, 1, 1, 1), in_ld=7)          # ld < c (the wrapper would not build such a view: the entry itself)
    src, dst = hipops.DeviceBuffer(x.nbytes), hipops.DeviceBuffer(4 * x.nbytes)
    with pytest.raises(hipops.HipError):
        hipops._chk(_native.hip().si_hip_pad2d_f32(C.byref(d), src.ptr, dst.ptr, None), "si_hip_pad2d_f32")

    def load(b, tag):
        pp, bp = save(b, tmp_path, tag)
        with pytest.raises(StatusError) as ei:
            Engine().load_model(pp, bp)
        return ei.value.status

    s = (1, 4, 4, 8)
    assert load(one_op_graph(s, 4, "reflect"), "reflect_limit") == Status.kUnsupport               # a pad over the limit
    assert load(one_op_graph(s, (5, 0, 0, 0), "circular"), "circular_limit") == Status.kUnsupport
    assert load(one_op_graph(s, (-1, 1, 0, 0), "circular", functional=True), "circular_negative") == Status.kUnsupport
    b = one_op_graph(s, (1, 1, 1, 1), "constant", functional=True)
    b.lines = [ln.replace(" pad=(1,1,1,1) ", " pad=(1,1,1,1,0,0) ") for ln in b.lines]
    assert "pad=(1,1,1,1,0,0)" in b.lines[1] and load(b, "six_entries") == Status.kUnsupport      # channel padding
    b = one_op_graph(s, (1, 1, 1, 1), "reflect", functional=True)
    b.lines = [ln.replace(" mode=reflect ", " mode=symmetric ") for ln in b.lines]
    assert "mode=symmetric" in b.lines[1] and load(b, "unknown_mode") == Status.kUnsupport
    b = one_op_graph(s, (1, 1, 1, 1), "reflect")
    b.lines = [ln.replace(" padding=(1,1,1,1) ", " padding=(1,2,1,1) ") for ln in b.lines]
    assert "padding=(1,2,1,1)" in b.lines[1] and load(b, "shape") == Status.kErrorShape            # the file's output shape is not the rule's
    b = one_op_graph(s, (1, 1, 1, 1), "constant", 1.5)
    b.lines = [ln.replace(" value=%e " % 1.5, " ") for ln in b.lines]
    assert "value" not in b.lines[1] and load(b, "missing_value") == Status.kFail                  # a missing required key
    # ... and the same process loads and runs a good model afterwards
    b = one_op_graph(s, 3, "reflect")
    pp, bp = save(b, tmp_path, "good")
    _, out = run_engine(pp, bp, x)
    ct.assert_same_bits(out, pr.pad2d_ref(x, (3, 3, 3, 3), "reflect"), "good model after the refusals")


ONE_OP = {
    "ReflectionPad2d": ((2, 6, 7, 3), (3, "reflect"), {}),                                          # one int, the RGB stem, scalar form
    "ReplicationPad2d": ((3, 16, 16, 64), ((1, 2, 0, 3), "replicate"), {}),
    "ZeroPad2d": ((2, 5, 4, 8), ((1, 1, 2, 0),), {}),
    "ConstantPad2d": ((2, 5, 4, 8), ((-1, 2, -2, 1), "constant", 1.5), {}),
    "ConstantPad2d_int_value": ((1, 9, 5, 21), (2, "constant", -3), {}),
    "CircularPad2d": ((1, 4, 4, 4), (4, "circular"), {}),
    "F.pad_2_entries": ((2, 5, 4, 8), ((2, 3), "reflect"), dict(functional=True)),                  # W only
    "F.pad_4_entries": ((2, 5, 4, 8), ((1, 2, 0, 3), "replicate"), dict(functional=True)),
    "F.pad_value_none": ((2, 6, 7, 3), ((1, 0, 1, 0), "constant", None), dict(functional=True)),
    "F.pad_value": ((2, 5, 4, 8), ((0, 1, 0, 1), "constant", 0.1), dict(functional=True)),
    "F.pad_circular": ((1, 4, 4, 8), ((4, 0, 0, 4), "circular"), dict(functional=True)),
}


@pytest.mark.parametrize("which", sorted(ONE_OP))
def test_engine_one_op_graph(gpu, tmp_path, which):
    """LoadModel -> Forward -> Extract reproduces the op-level result bit for bit (and the reference)"""
    s, args, kw = ONE_OP[which]
    b = one_op_graph(s, *args, **kw)
    typ, _, _, _, prm = _parse(b.lines[1])
    assert typ == ("F.pad" if kw else "nn." + which.split("_")[0]), typ
    pads, mode, value = pr.pad_args(typ, prm)
    pp, bp = save(b, tmp_path)
    x = bit_patterns(9, s, np.float32)
    e, got = run_engine(pp, bp, x)
    op_level = hipops.pad2d(x, pads, mode, value)
    ct.assert_same_bits(got, op_level, "engine vs op level")
    ct.assert_same_bits(got, pr.pad2d_ref(x, pads, mode, value), "engine vs the reference")
    layers = [L for L in e.profile() if L["type"] in pr.PAD_TYPES]
    assert len(layers) == 1 and layers[0]["type"] == typ, layers
    assert layers[0]["kernel"] == hipops.pad2d_kernel_name(s, pads, mode) == form(np.float32, s[3] % 4 == 0), layers
    assert layers[0]["bytes"] == float(x.nbytes + got.nbytes), layers


@pytest.mark.parametrize("opts", [{}, dict(fp16=1)], ids=["fp32", "fp16_option"])
@pytest.mark.parametrize("s", [(2, 6, 7, 3), (1, 8, 8, 16)], ids=["scalar", "vector"])
def test_engine_tanh(gpu, tmp_path, s, opts):
    n, h, w, c = s
    b = mg.PnnxBuilder(seed=5)
    b.output(b.tanh(b.input((n, c, h, w))))
    pp, bp = save(b, tmp_path)
    x = util.rng_uniform(13, s, -4.0, 4.0)
    e, got = run_engine(pp, bp, x, **opts)
    util.assert_parity(got, np.tanh(x.astype(np.float64)), what="nn.Tanh %s" % (opts or "fp32"))
    layers = [L for L in e.profile() if L["type"] == "nn.Tanh"]
    assert len(layers) == 1 and layers[0]["kernel"] == "unary_kernel", layers


def test_pad_feeds_a_concat(gpu, tmp_path):
    """a U-Net level whose size is odd: the up-conv's 8 x 8 is padded (1, 0, 1, 0) to the skip's 9 x 9, then concatenated.  The pad
    writes into the concat buffer's channel slice (the alias the data-movement layers get)."""
    b = mg.PnnxBuilder(seed=7)
    x = b.input((2, 4, 9, 9))
    skip = b.relu(b.conv(x, 8, 3, 1, 1))
    down = b.relu(b.conv(skip, 16, 3, 2, 0))            # 4 x 4
    up = b.conv_transpose(down, 8, 2, 2, 0)             # 8 x 8
    padded = b.pad(up, (1, 0, 1, 0), "constant", None, functional=True)
    b.output(b.conv(b.cat([skip, padded]), 4, 1, 1, 0))
    pp, bp = save(b, tmp_path)
    xin = util.rng_uniform(15, (2, 9, 9, 4), -1.0, 1.0)
    e, got = run_engine(pp, bp, xin)
    util.assert_parity(got, pr.eval_graph(b, xin), what="pad -> cat")
    assert padded in e.schedule()["alias"], e.schedule()
    pads = [L for L in e.profile() if L["type"] == "F.pad"]
    assert len(pads) == 1 and pads[0]["kernel"] == "pad2d_kernel<float, 4>", pads


def pad_layers(prof):
    return [L for L in prof if L["type"] in pr.PAD_TYPES]


def test_toy_cyclegan_fp32(gpu, tmp_path):
    b = mg.build_toy_cyclegan()
    pp, bp = save(b, tmp_path)
    x = mg.synth_input((2, 32, 32, 3))
    e, got = run_engine(pp, bp, x)
    ref = pr.eval_graph(b, x)
    print("toy CycleGAN fp32: max-based %.3e, element-wise %.3e" % (util.rel_err(got, ref), util.mixed_err(got, ref)))
    util.assert_parity(got, ref, what="toy CycleGAN fp32")
    assert (np.abs(got) < 1.0).all()
    pads = pad_layers(e.profile())
    assert [L["kernel"] for L in pads] == ["pad2d_kernel<float, 1>"] + ["pad2d_kernel<float, 4>"] * 5, pads   # the RGB stem, then 32 / 8 channels
    assert [L["type"] for L in e.profile()].count("nn.Tanh") == 1
    # a captured graph replays the same bits
    _, g = run_engine(pp, bp, x, graph=1)
    util.assert_exact(g.view(np.uint32), got.view(np.uint32), "graph=1 vs eager")


def test_toy_cyclegan_rebatch(gpu, tmp_path):
    """SetOption("batch", 5) on the batch-2 file: per image the same bits as batch-2 runs of the same images"""
    b = mg.build_toy_cyclegan()
    pp, bp = save(b, tmp_path)
    x5 = util.rng_uniform(21, (5, 32, 32, 3), 0.0, 1.0)
    _, y5 = run_engine(pp, bp, x5, batch=5)
    xs = np.concatenate([x5, x5[:1]], 0)   # pairs (0, 1), (2, 3), (4, 0)
    for i in range(0, 6, 2):
        _, y2 = run_engine(pp, bp, xs[i:i + 2])
        for j in range(2):
            if i + j < 5:
                util.assert_exact(y5[i + j].view(np.uint32), y2[j].view(np.uint32), "image %d" % (i + j))


def test_toy_cyclegan_fp16_storage(gpu, tmp_path):
    """fp16=1: every pad and the tanh run the half kernels with no cast pair around them (the stem's pad reads the caller's fp32 tensor: the
    layer rounds it to half itself and pads in half; the RGB stem conv behind it has no fp16 kernel for a half input and runs in fp32 between
    casts of its own), and the error against fp64 is at most 2x that of the fp16-storage emulation (weights,
    biases, the input and every layer's output rounded to fp16, fp64 arithmetic between) -- the factor of test_toy_unet_fp16_storage"""
    b = mg.build_toy_cyclegan()
    pp, bp = save(b, tmp_path)
    x = mg.synth_input((2, 32, 32, 3))
    e, got = run_engine(pp, bp, x, fp16=1)
    prof = e.profile()
    pads, tanh = pad_layers(prof), [L for L in prof if L["type"] == "nn.Tanh"]
    assert [L["kernel"] for L in pads] == ["pad2d_kernel<_Float16, 1>"] + ["pad2d_kernel<_Float16, 8>"] * 5, pads
    assert len(tanh) == 1 and tanh[0]["kernel"] == "unary_h_kernel", tanh
    names = [L["name"] for L in prof]
    for L in pads + tanh:   # (InsertFp32Fallbacks names its casts <layer>.in_to_f32.<k> / <layer>.out_to_f16.<k>)
        assert not any(n.startswith(L["name"] + ".in_to_f32") or n.startswith(L["name"] + ".out_to_f16") for n in names), names
    ref = pr.eval_graph(b, x)
    emu = pr.eval_graph(b, x, rnd=pr.round_f16)
    e_engine, e_emu = util.rel_err(got, ref), util.rel_err(emu, ref)
    print("toy CycleGAN fp16 storage vs fp64: engine %.3e, fp16 emulation %.3e" % (e_engine, e_emu))
    assert np.isfinite(got).all()
    assert e_engine <= 2.0 * e_emu, (e_engine, e_emu)
