"""GPU: the sub-pixel super-resolution layers -- si_hip_pixel_shuffle_f32 / _f16 and si_hip_prelu_f32 / _f16 (include/si_superres.h)
against the numpy references (tests/superres_reference.py) by equality of BITS: the shuffle and the unshuffle on random bit
patterns in every form the header declares, strided views under guard bands, determinism; PReLU with shared and per-channel slopes,
special values, rank 2 and strided views; and the layers inside the engine: one-op graphs for the five type strings, a shuffle
that reads from one concat and writes into another, the three toy models (ESPCN, SRResNet, the Real-ESRGAN head) in fp32, under graph
capture, re-batched and with fp16 storage, and the Validate refusals.  Every engine test fails without the layers (LoadModel rejects
the types), every op-level test without the kernels (the symbols are missing)."""
import numpy as np
import pytest

import containment as ct
import superres_reference as sr
import util
from ct_reference import _parse
from simpleinfer_amd import hipops, modelgen as mg
from simpleinfer_amd.engine import Engine, Status, StatusError

pytestmark = pytest.mark.gpu

DTYPES = {"f32": np.float32, "f16": np.float16}
TNAME = {"f32": "float", "f16": "_Float16"}
VW = {"f32": 4, "f16": 8}


def bit_patterns(seed, shape, dtype):
    """random BITS viewed as the float type: NaNs of every payload, infinities, denormals and -0.0 are among them"""
    r = np.random.Generator(np.random.Philox(seed))
    if dtype == np.float32:
        return r.integers(0, 2 ** 32, shape, dtype=np.uint32).view(np.float32)
    return r.integers(0, 2 ** 16, shape, dtype=np.uint16).view(np.float16)


def form(dt, f):
    """f: "e" the element form, "v" the LDS form with channel vectors on the wide side, "s" the LDS form gathering single elements"""
    if f == "e":
        return "pixel_shuffle_elem<%s>" % TNAME[dt]
    return "pixel_shuffle_lds<%s, %d>" % (TNAME[dt], VW[dt] if f == "v" else 1)


ALL_FORMS = {form(dt, f) for dt in DTYPES for f in "evs"}

# (the DEEP tensor's NHWC shape [n, h, w, C r r], r, the form dense 16-byte aligned buffers take in fp32, in fp16).  The shuffle reads
# the deep tensor and writes the wide one [n, h r, w r, C]; the unshuffle runs the same row the other way and takes the same form.
TABLE = [
    ((1, 1, 1, 1), 1, "e", "e"),        # a single pixel; r = 1 is a copy
    ((1, 1, 1, 4), 2, "e", "e"),        # ... the wide row has 2 elements: no vector
    ((1, 1, 1, 9), 3, "e", "e"),
    ((1, 1, 1, 16), 4, "s", "e"),       # C = 1: the wide row is one fp32 vector
    ((1, 2, 3, 5), 1, "e", "e"),
    ((2, 3, 5, 16), 2, "v", "s"),       # C = 4: a channel vector in fp32, a dense row in fp16
    ((1, 2, 3, 27), 3, "e", "e"),       # odd everywhere: 81 elements per deep row
    ((1, 2, 2, 48), 4, "s", "s"),       # C = 3, r = 4
    ((2, 4, 6, 256), 2, "v", "v"),      # the SRResNet / EDSR upsampler, 256 -> 64; 6 pixels: fewer than a workgroup's run (16 / 32)
    ((1, 2, 40, 256), 2, "v", "v"),     # runs of 16 (fp32: 16 + 16 + 8) and 32 (fp16: 32 + 8): the last workgroup partly idle
    ((2, 3, 8, 48), 2, "v", "s"),       # C = 12: fp16 with C % 8 != 0
    ((1, 2, 16, 27), 3, "s", "s"),      # C = 3, r = 3: 16-byte vectors that straddle pixels on both sides
    ((1, 1, 344, 12), 2, "s", "s"),     # the 3 -> 12 unshuffle's row; fp32: a run of 336 pixels and one of 8
]


def case_id(c):
    s, r = c[0], c[1]
    return "%dx%dx%dx%d_r%d" % (s + (r,))


FORMS_SEEN = set()


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("inverse", [False, True], ids=["shuffle", "unshuffle"])
@pytest.mark.parametrize("case", TABLE, ids=case_id)
def test_op_moves_the_bits_of_the_reference(gpu, case, inverse, dt):
    deep, r = case[0], case[1]
    want_form = form(dt, case[2] if dt == "f32" else case[3])
    dtype = DTYPES[dt]
    s = sr.out_shape(deep, r) if inverse else deep
    x = bit_patterns(17, s, dtype)
    got = hipops.pixel_shuffle(x, r, inverse)
    kernel = hipops.LAST_KERNEL_NAME["si_hip_pixel_shuffle"]
    FORMS_SEEN.add(kernel)
    assert got.dtype == dtype
    assert kernel == want_form, kernel
    ct.assert_same_bits(got, sr.pixel_shuffle_ref(x, r, inverse), "%s %s %s [%s]" % (case_id(case), "unshuffle" if inverse else "shuffle", dt, kernel))


def test_all_forms_ran(gpu):
    """the names reported over the case list are exactly the forms the header declares (runs after the parametrised test above, whose
    names it collects)"""
    if FORMS_SEEN != ALL_FORMS:
        for dt, dtype in DTYPES.items():
            for case in TABLE:
                hipops.pixel_shuffle(bit_patterns(1, case[0], dtype), case[1])
                FORMS_SEEN.add(hipops.LAST_KERNEL_NAME["si_hip_pixel_shuffle"])
    assert FORMS_SEEN == ALL_FORMS, FORMS_SEEN


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("case", [TABLE[8], TABLE[11], TABLE[6]], ids=["vector", "straddling", "element"])
def test_same_bits_twice_and_round_trip(gpu, case, dt):
    deep, r = case[0], case[1]
    x = bit_patterns(29, deep, DTYPES[dt])
    y = hipops.pixel_shuffle(x, r)
    ct.assert_same_bits(y, hipops.pixel_shuffle(x, r), "two launches")
    ct.assert_same_bits(hipops.pixel_shuffle(y, r, True), x, "unshuffle of shuffle")


def test_batch_of_5_has_the_bits_of_single_images(gpu):
    x = bit_patterns(31, (5, 3, 8, 48), np.float16)
    y5 = hipops.pixel_shuffle(x, 2)
    for i in range(5):
        ct.assert_same_bits(y5[i:i + 1], hipops.pixel_shuffle(x[i:i + 1], 2), "image %d" % i)


# ---- views and containment: checks (a) - (d) of tests/test_gpu_containment.py ---------------------------------------------------------
class ShuffleView:
    """deep: the deep tensor's shape; the views are given for the deep and the wide side and land on the input or the output by direction"""

    def __init__(self, cid, half, inverse, deep, r, f, deep_view, wide_view):
        self.id = "%s_%s_%s" % ("unshuffle" if inverse else "shuffle", cid, "f16" if half else "f32")
        self.half, self.inverse, self.r, self.form = half, inverse, r, form("f16" if half else "f32", f)
        self.dtype = np.float16 if half else np.float32
        self.entries = ("si_hip_pixel_shuffle_f16" if half else "si_hip_pixel_shuffle_f32",)
        self.key = "si_hip_pixel_shuffle"
        self.s = sr.out_shape(deep, r) if inverse else deep
        iv, ov = (wide_view, deep_view) if inverse else (deep_view, wide_view)
        self.views = dict(in_ld=iv[0], in_c_off=iv[1], out_ld=ov[0], out_c_off=ov[1])
        self.buffers = 2   # x, y

    def input(self):
        return bit_patterns(23, self.s, self.dtype)

    def reference(self):
        return sr.pixel_shuffle_ref(self.input(), self.r, self.inverse)

    def run(self, F):
        y = hipops.pixel_shuffle(self.input(), self.r, self.inverse, in_fill=F, out_fill=F, full=True, **self.views)
        return ct.Out("y", y, self.views["out_c_off"], sr.out_shape(self.s, self.r, self.inverse)[3])


class PReluView:
    def __init__(self, cid, half, s, per_channel, vec, **views):
        self.id = "prelu_%s_%s" % (cid, "f16" if half else "f32")
        self.half, self.s, self.per_channel, self.views = half, s, per_channel, views
        self.dtype = np.float16 if half else np.float32
        self.form = "prelu_kernel<%s, %d>" % ("_Float16" if half else "float", (8 if half else 4) if vec else 1)
        self.entries = ("si_hip_prelu_f16" if half else "si_hip_prelu_f32",)
        self.key = "si_hip_prelu"
        self.buffers = 3   # the slopes, x, y

    def input(self):
        return util.rng_uniform(23, self.s, -4.0, 4.0).astype(self.dtype)

    def slope(self):
        return util.rng_uniform(7, (self.s[-1] if self.per_channel else 1,), 0.05, 0.4)

    def reference(self):
        return sr.prelu_ref(self.input(), self.slope())

    def run(self, F):
        y = hipops.prelu(self.input(), self.slope(), in_fill=F, out_fill=F, full=True, **self.views)
        return ct.Out("y", y, self.views.get("out_c_off", 0), self.s[-1])


VIEW_CASES = []
for _half in (False, True):
    for _inv in (False, True):
        VIEW_CASES += [
            # both tensors at a channel offset of a wider buffer, 16-byte aligned on both sides: the LDS form with channel vectors
            ShuffleView("vector", _half, _inv, (2, 3, 5, 32), 2, "v", (48, 16), (24, 8)),
            # odd offsets and strides
            ShuffleView("odd", _half, _inv, (1, 2, 3, 27), 3, "e", (29, 1), (5, 1)),
            # a stride c + 1 that forces the element form on vector-sized channels
            ShuffleView("odd_stride", _half, _inv, (1, 2, 4, 32), 2, "e", (33, 0), (16, 8)),
            # the wide tensor dense with C = 3 (vectors that straddle pixels run up to the buffer's last byte), the deep one a slice
            ShuffleView("straddling", _half, _inv, (1, 2, 16, 48), 4, "s", (64, 16), (None, 0)),
            # ... and both dense with nothing a multiple of the vector but the rows
            ShuffleView("dense_odd", _half, _inv, (1, 2, 16, 27), 3, "s", (None, 0), (None, 0)),
        ]
    VIEW_CASES += [
        PReluView("vector", _half, (2, 5, 4, 8), True, True, in_ld=24, in_c_off=8, out_ld=32, out_c_off=16),
        PReluView("scalar", _half, (2, 6, 7, 3), True, False, in_ld=5, in_c_off=2, out_ld=7, out_c_off=3),
        PReluView("odd_stride", _half, (1, 4, 4, 8), False, False, in_ld=9, in_c_off=0, out_ld=16, out_c_off=8),
        PReluView("rank2_last_slice", _half, (6, 21), True, False, in_ld=29, in_c_off=8, out_ld=21, out_c_off=0),
    ]


@pytest.mark.parametrize("case", VIEW_CASES, ids=[c.id for c in VIEW_CASES])
def test_views_and_containment(gpu, case):
    del hipops.LAST_ENTRIES[:]
    plain = case.run(hipops.ByteFill(0x00))
    plain_kernel = hipops.LAST_KERNEL_NAME[case.key]
    assert set(case.entries) <= set(hipops.LAST_ENTRIES), hipops.LAST_ENTRIES
    assert plain_kernel == case.form, plain_kernel
    ct.assert_outside_fill(plain.full, plain.c_off, plain.c, 0x00, case.id + ", plain run")
    # the value too: nothing of the gaps between the input's pixels reached the output
    ct.assert_same_bits(plain.dest, case.reference(), case.id + " vs the reference")
    for byte in ct.PATTERNS:
        with hipops.guard_bands(byte) as g:      # (a) all bands and (d) the input are compared when the block ends
            out = case.run(hipops.ByteFill(byte))
        what = "%s under 0x%02X" % (case.id, byte)
        assert g.checked == case.buffers, "%s: the guard saw %d buffers" % (what, g.checked)
        assert hipops.LAST_KERNEL_NAME[case.key] == plain_kernel, what
        ct.assert_outside_fill(out.full, out.c_off, out.c, byte, what)                              # (b)
        ct.assert_same_bits(out.dest, plain.dest, what + ": guarded + pattern-filled vs plain")    # (c)


# ---- PReLU ------------------------------------------------------------------------------------------------------------------------------
def prelu_input(seed, shape, dtype):
    """finite values in [-4, 4) with a -0.0, a +0.0, both infinities and a denormal among them"""
    x = util.rng_uniform(seed, shape, -4.0, 4.0).astype(dtype)
    flat = x.reshape(-1)
    tiny = np.finfo(dtype).smallest_subnormal
    for i, v in enumerate((-0.0, 0.0, np.inf, -np.inf, tiny, -tiny)):
        if 3 * i + 1 < flat.size:
            flat[3 * i + 1] = v
    return x


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("per_channel", [False, True], ids=["shared", "per_channel"])
@pytest.mark.parametrize("s", [(2, 3, 5, 1), (2, 6, 7, 3), (2, 5, 4, 8), (3, 9, 7, 64), (5, 64), (4, 3)],
                         ids=["c1", "c3", "c8", "c64", "rank2_c64", "rank2_c3"])
def test_prelu_bits(gpu, s, per_channel, dt):
    dtype = DTYPES[dt]
    x = prelu_input(41, s, dtype)
    slope = util.rng_uniform(43, (s[-1] if per_channel else 1,), 0.05, 0.4)
    got = hipops.prelu(x, slope)
    vec = s[-1] % VW[dt] == 0
    assert hipops.LAST_KERNEL_NAME["si_hip_prelu"] == "prelu_kernel<%s, %d>" % (TNAME[dt], VW[dt] if vec else 1)
    assert got.dtype == dtype and got.shape == x.shape
    ct.assert_same_bits(got, sr.prelu_ref(x, slope), "prelu %r %s" % (s, dt))
    ct.assert_same_bits(got, hipops.prelu(x, slope), "two launches")
    assert np.signbit(got.reshape(-1)[1]) and got.reshape(-1)[1] == 0     # -0.0 went through the multiply
    if x.size > 10:
        assert got.reshape(-1)[7] == np.inf and got.reshape(-1)[10] == -np.inf


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_prelu_keeps_nans(gpu, dt):
    dtype = DTYPES[dt]
    x = prelu_input(47, (1, 4, 4, 8), dtype)
    x.reshape(-1)[[0, 9, 77]] = np.nan
    got = hipops.prelu(x, [0.25])
    assert np.array_equal(np.isnan(got), np.isnan(x))
    ok = ~np.isnan(x)
    ct.assert_same_bits(got[ok], sr.prelu_ref(x, [0.25])[ok], "beside the NaNs")


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


def one_op_graph(s, op, *a, **kw):
    """input -> one layer (a PnnxBuilder method and its arguments) -> output, for an NHWC shape (or [N, F])"""
    b = mg.PnnxBuilder(seed=5)
    x = b.input((s[0], s[3], s[1], s[2]) if len(s) == 4 else s)
    b.output(getattr(b, op)(x, *a, **kw))
    return b


ONE_OP = {
    "nn.PixelShuffle": ((2, 4, 6, 256), "pixel_shuffle", (2,), {}, "pixel_shuffle_lds<float, 4>"),
    "nn.PixelShuffle_r3": ((1, 2, 3, 27), "pixel_shuffle", (3,), {}, "pixel_shuffle_elem<float>"),
    "F.pixel_shuffle": ((1, 2, 2, 48), "pixel_shuffle", (4,), dict(functional=True), "pixel_shuffle_lds<float, 1>"),
    "nn.PixelUnshuffle": ((1, 2, 688, 3), "pixel_unshuffle", (2,), {}, "pixel_shuffle_lds<float, 1>"),
    "F.pixel_unshuffle": ((2, 6, 10, 4), "pixel_unshuffle", (2,), dict(functional=True), "pixel_shuffle_lds<float, 4>"),
    "nn.PReLU": ((2, 5, 4, 8), "prelu", (1,), {}, "prelu_kernel<float, 4>"),
    "nn.PReLU_per_channel": ((2, 6, 7, 3), "prelu", (3,), {}, "prelu_kernel<float, 1>"),
}


@pytest.mark.parametrize("which", sorted(ONE_OP))
def test_engine_one_op_graph(gpu, tmp_path, which):
    """LoadModel -> Forward -> Extract reproduces the op-level result bit for bit (and the reference)"""
    s, op, args, kw, kernel = ONE_OP[which]
    b = one_op_graph(s, op, *args, **kw)
    typ, name, _, _, prm = _parse(b.lines[1])
    assert typ == which.split("_r3")[0].split("_per")[0], typ
    pp, bp = save(b, tmp_path)
    if typ == "nn.PReLU":
        x = prelu_input(9, s, np.float32)
        ref = sr.prelu_ref(x, b.attrs[name + ".weight"])
        op_level = hipops.prelu(x, b.attrs[name + ".weight"])
    else:
        x = bit_patterns(9, s, np.float32)
        ref = sr.pixel_shuffle_ref(x, sr.factor(typ, prm), typ in sr.UNSHUFFLE_TYPES)
        op_level = hipops.pixel_shuffle(x, sr.factor(typ, prm), typ in sr.UNSHUFFLE_TYPES)
    e, got = run_engine(pp, bp, x)
    ct.assert_same_bits(got, op_level, "engine vs op level")
    ct.assert_same_bits(got, ref, "engine vs the reference")
    layers = [L for L in e.profile() if L["type"] in sr.FIVE]
    assert len(layers) == 1 and layers[0]["type"] == typ, layers
    assert layers[0]["kernel"] == kernel, layers
    assert layers[0]["bytes"] == float(x.nbytes + got.nbytes), layers


def test_shuffle_between_two_concats(gpu, tmp_path):
    """the shuffle's input is a channel slice of one concat buffer (its producer writes there for the cat beside it) and its output a slice
    of another: both pixel strides are wider than the channels"""
    b = mg.PnnxBuilder(seed=7)
    x = b.input((2, 4, 6, 6))
    a1 = b.relu(b.conv(x, 16, 3, 1, 1))
    a2 = b.relu(b.conv(x, 16, 3, 1, 1))
    t = b.upsample(b.conv(b.cat([a1, a2]), 4, 3, 1, 1), 2.0)     # 12 x 12
    s = b.pixel_shuffle(a1, 2)                                    # 16 -> 4 channels at 12 x 12
    b.output(b.conv(b.cat([t, s]), 3, 3, 1, 1))
    pp, bp = save(b, tmp_path)
    xin = util.rng_uniform(15, (2, 6, 6, 4), -1.0, 1.0)
    e, got = run_engine(pp, bp, xin)
    util.assert_parity(got, sr.eval_graph(b, xin), what="cat -> shuffle -> cat")
    alias = e.schedule()["alias"]
    assert a1 in alias and s in alias, e.schedule()
    ps = [L for L in e.profile() if L["type"] == "nn.PixelShuffle"]
    assert len(ps) == 1 and ps[0]["kernel"] == "pixel_shuffle_lds<float, 4>", ps


TOYS = {
    "espcn_r2": (lambda: mg.build_toy_espcn(r=2), (2, 16, 16, 3)),
    "espcn_r3": (lambda: mg.build_toy_espcn(r=3), (2, 16, 16, 3)),
    "srresnet": (lambda: mg.build_toy_srresnet(), (2, 12, 12, 3)),
    "esrgan_head": (lambda: mg.build_toy_esrgan_head(), (2, 16, 16, 3)),
}


def new_layers(prof):
    return [L for L in prof if L["type"] in sr.FIVE]


@pytest.mark.parametrize("which", sorted(TOYS))
def test_toy_fp32_and_graph(gpu, tmp_path, which):
    build, s = TOYS[which]
    b = build()
    pp, bp = save(b, tmp_path)
    x = mg.synth_input(s)
    e, got = run_engine(pp, bp, x)
    ref = sr.eval_graph(b, x)
    print("toy %s fp32: max-based %.3e, element-wise %.3e" % (which, util.rel_err(got, ref), util.mixed_err(got, ref)))
    util.assert_parity(got, ref, what="toy %s fp32" % which)
    types = [ln.split()[0] for ln in b.lines]
    assert sorted(L["type"] for L in new_layers(e.profile())) == sorted(t for t in types if t in sr.FIVE)
    assert all(L["kernel"].startswith(("pixel_shuffle_", "prelu_kernel<float")) for L in new_layers(e.profile())), new_layers(e.profile())
    # a captured graph replays the same bits
    _, g = run_engine(pp, bp, x, graph=1)
    util.assert_exact(g.view(np.uint32), got.view(np.uint32), "graph=1 vs eager")


@pytest.mark.parametrize("which", sorted(TOYS))
def test_toy_rebatch(gpu, tmp_path, which):
    """SetOption("batch", 3) on the batch-2 file: per image the same bits as batch-2 runs of the same images"""
    build, s = TOYS[which]
    pp, bp = save(build(), tmp_path)
    x3 = util.rng_uniform(21, (3,) + s[1:], 0.0, 1.0)
    _, y3 = run_engine(pp, bp, x3, batch=3)
    xs = np.concatenate([x3, x3[:1]], 0)   # pairs (0, 1), (2, 0)
    for i in range(0, 4, 2):
        _, y2 = run_engine(pp, bp, xs[i:i + 2])
        for j in range(2):
            if i + j < 3:
                util.assert_exact(y3[i + j].view(np.uint32), y2[j].view(np.uint32), "image %d" % (i + j))


@pytest.mark.parametrize("which", sorted(TOYS))
def test_toy_fp16_storage(gpu, tmp_path, which):
    """fp16=1: the shuffles and PReLUs between half tensors run the half kernels with no cast pair around them (the Real-ESRGAN head's
    unshuffle reads the caller's fp32 tensor: the engine runs it in fp32 with its cast behind it), and the error against fp64 is at most
    2x that of the fp16-storage emulation (weights, biases, the input and every layer's output rounded to fp16, fp64 arithmetic
    between) -- the factor of test_toy_cyclegan_fp16_storage"""
    build, s = TOYS[which]
    b = build()
    pp, bp = save(b, tmp_path)
    x = mg.synth_input(s)
    e, got = run_engine(pp, bp, x, fp16=1)
    prof = e.profile()
    names = [L["name"] for L in prof]
    for L in new_layers(prof):
        if L["type"] == "nn.PixelUnshuffle" and which == "esrgan_head":
            continue
        assert "_Float16" in L["kernel"], L
        assert not any(n.startswith(L["name"] + ".in_to_f32") or n.startswith(L["name"] + ".out_to_f16") for n in names), names
    ref = sr.eval_graph(b, x)
    emu = sr.eval_graph(b, x, rnd=sr.round_f16)
    e_engine, e_emu = util.rel_err(got, ref), util.rel_err(emu, ref)
    print("toy %s fp16 storage vs fp64: engine %.3e, fp16 emulation %.3e" % (which, e_engine, e_emu))
    assert np.isfinite(got).all()
    assert e_engine <= 2.0 * e_emu, (e_engine, e_emu)


def raw_graph(in_shape, typ, out_shape, params, attrs=None):
    """input -> one line written as given (shapes as the file has them: NCHW) -> output"""
    b = mg.PnnxBuilder(seed=5)
    x = b.input(in_shape)
    y = b._new_operand(out_shape)
    b._emit(typ, "op_0", [x], [y], params, attrs or {})
    b.output(y)
    return b


def test_validate_refusals_leave_the_process_usable(gpu, tmp_path):
    def load(b, tag):
        pp, bp = save(b, tmp_path, tag)
        with pytest.raises(StatusError) as ei:
            Engine().load_model(pp, bp)
        return ei.value.status

    assert load(raw_graph((2, 16), "nn.PixelShuffle", (2, 16), dict(upscale_factor=2)), "rank2") == Status.kUnsupport
    assert load(raw_graph((2, 16, 3, 5), "nn.PixelShuffle", (2, 4, 6, 10), dict(upscale_factor=4)), "shape") == Status.kErrorShape
    assert load(raw_graph((2, 16, 3, 5), "F.pixel_shuffle", (2, 4, 6, 11), dict(upscale_factor=2)), "width") == Status.kErrorShape
    assert load(raw_graph((2, 18, 3, 5), "nn.PixelShuffle", (2, 4, 6, 10), dict(upscale_factor=2)), "channels") == Status.kErrorShape
    assert load(raw_graph((1, 3, 5, 6), "nn.PixelUnshuffle", (1, 12, 2, 3), dict(downscale_factor=2)), "indivisible") == Status.kErrorShape
    assert load(raw_graph((1, 3, 4, 6), "F.pixel_unshuffle", (1, 3, 4, 6), dict(downscale_factor=0)), "factor") == Status.kErrorShape
    assert load(raw_graph((2, 16, 3, 5), "nn.PixelShuffle", (2, 4, 6, 10), dict(scale=2)), "missing_key") == Status.kFail
    w4 = np.full(4, 0.25, np.float32)
    assert load(raw_graph((2, 8, 3, 5), "nn.PReLU", (2, 8, 3, 5), dict(num_parameters=4), dict(weight=w4)), "num_parameters") == Status.kErrorShape
    assert load(raw_graph((2, 8, 3, 5), "nn.PReLU", (2, 8, 3, 5), dict(num_parameters=8), dict(weight=w4)), "weights") == Status.kErrorShape
    assert load(raw_graph((2, 8, 3, 5), "nn.PReLU", (2, 8, 3, 5), dict(num_parameters=1)), "no_weight") == Status.kFail
    x = bit_patterns(3, (1, 4, 4, 8), np.float32)
    with pytest.raises(hipops.HipError):
        hipops.pixel_shuffle(x, 3)                              # 8 channels, r r = 9
    with pytest.raises(hipops.HipError):
        hipops.pixel_shuffle(x, 3, inverse=True)                # 4 x 4 pixels, r = 3
    with pytest.raises(hipops.HipError):
        hipops.prelu(x, [0.1, 0.2])                             # 2 slopes for 8 channels
    # ... and the same process loads and runs a good model afterwards
    pp, bp = save(one_op_graph((1, 4, 4, 8), "pixel_shuffle", 2), tmp_path, "good")
    _, out = run_engine(pp, bp, x)
    ct.assert_same_bits(out, sr.pixel_shuffle_ref(x, 2), "good model after the refusals")
