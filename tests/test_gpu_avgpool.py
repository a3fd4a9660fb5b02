"""GPU: the window means -- si_hip_avgpool2d_f32 / _f16 (include/si_pool.h).  The windowed form against the float32 / float16 emulation
of tests/pool_reference.py by equality of BITS (the emulation is pinned to torch's CPU kernels by tests/test_avgpool_cpu.py) and against
torch float64 at the project's bars; the cooperative form against torch float64; the form switch; determinism; strided views under guard
bands; the refusals; and the layers inside the engine: one-op graphs for the four type strings, a pool feeding a concat, the toy DenseNet /
Inception / ResNet-D classifier and the toy PSPNet in fp32, under graph capture, re-batched, and with fp16 storage.  Every engine test
fails without the layers (LoadModel rejects the types, Forward the non-divisible adaptive shapes), every op-level test without the
kernel (the symbols are missing)."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import containment as ct
import pool_reference as pl
import util
from ct_reference import _parse
from simpleinfer_amd import _native, hipops, modelgen as mg
from simpleinfer_amd.engine import Engine, Status, StatusError
from test_gpu_f16 import F16_TOL

pytestmark = pytest.mark.gpu

DTYPES = {"f32": np.float32, "f16": np.float16}
WIN, COOP = "avgpool2d_window_kernel", "avgpool2d_coop_kernel"
POOL_HEADER = os.path.join(os.path.dirname(ct.HEADER), "si_pool.h")
T = int(re.search(r"SI_AVGPOOL_COOP_TAPS = (\d+)", open(POOL_HEADER).read()).group(1))   # the form switch, in taps of the largest window
CMAX = 72   # the references are computed once at 72 channels: every channel is on its own, so the first c channels are the c-channel result


def kname(form, dtype, vec):
    if dtype == np.float32:
        return form + ("<float, 4>" if vec else "<float, 1>")
    return form + ("<_Float16, 8>" if vec else "<_Float16, 1>")


def vectorised(c, dtype):
    return c % (16 // np.dtype(dtype).itemsize) == 0


def as_kw(case):
    """a table row (k, s, p, ceil_mode, count_include_pad, divisor_override), or an adaptive output size (oh, ow)"""
    if len(case) == 2:
        return dict(adaptive=tuple(case))
    k, s, p, ce, cip, div = case
    return dict(k=k, s=s, p=p, ceil_mode=ce, count_include_pad=cip, divisor_override=div)


def cid(case):
    return "adaptive_%dx%d" % tuple(case) if len(case) == 2 else pl.case_id(case)


@functools.lru_cache(maxsize=None)
def data(shape3, dt, offset=0.0):
    x = (util.rng_uniform(41, shape3 + (CMAX,), -1.0, 1.0) + np.float32(offset)).astype(DTYPES[dt])
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def emulation(shape3, dt, case):
    return pl.avgpool2d_ref(data(shape3, dt), acc=np.float32, **as_kw(case))


@functools.lru_cache(maxsize=None)
def torch64(shape3, dt, case, offset=0.0):
    """torch float64 on the values the device sees (the half data widened)"""
    return pl.avgpool2d_f64_torch(data(shape3, dt, offset), **as_kw(case))


def run(x, case, **views):
    """the op on an NHWC array by a table row or an adaptive size; returns (result, kernel name)"""
    kw = as_kw(case)
    if "adaptive" in kw:
        y = hipops.adaptive_avgpool2d_general(x, kw["adaptive"], **views)
    else:
        y = hipops.avgpool2d(x, kw["k"], kw["s"], kw["p"], kw["ceil_mode"], kw["count_include_pad"], kw["divisor_override"], **views)
    return y, hipops.LAST_KERNEL_NAME["si_hip_avgpool2d"]


def expected_form(shape3, case):
    kw = as_kw(case)
    taps = pl.max_taps(shape3[1], shape3[2], adaptive=kw["adaptive"]) if "adaptive" in kw else pl.max_taps(
        shape3[1], shape3[2], kw["k"], kw["s"], kw["p"], kw["ceil_mode"])
    return COOP if taps >= T else WIN


FORMS_SEEN = set()
WORST = {}   # (form, dt) -> [max-based, element-wise] worst error against torch float64


def check(shape3, case, dt, c, offset=0.0):
    """one launch: the form the shape calls for; the windowed form holds the emulation's bits; both forms are within the bar of torch float64"""
    dtype = DTYPES[dt]
    x = np.ascontiguousarray(data(shape3, dt, offset)[..., :c])
    got, kernel = run(x, case)
    form = expected_form(shape3, case)
    FORMS_SEEN.add(kernel)
    what = "%s %s c=%d [%s]" % (cid(case), dt, c, kernel)
    assert got.dtype == dtype and kernel == kname(form, dtype, vectorised(c, dtype)), what
    ref = torch64(shape3, dt, case, offset)[..., :c]
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if form == WIN and offset == 0.0:
        ct.assert_same_bits(got, np.ascontiguousarray(emulation(shape3, dt, case)[..., :c]), what)
    e = util.assert_parity(got.astype(np.float64), ref, rel=util.REL_TOL if dt == "f32" else F16_TOL, what=what)
    w = WORST.setdefault((form, dt), [0.0, 0.0])
    w[0], w[1] = max(w[0], e), max(w[1], util.mixed_err(got.astype(np.float64), ref))


# ---- 1. the windowed form: equality of bits ----------------------------------------------------------------------------------------------
WINDOWED = [c for c in pl.TABLE_A if c[0] != (11, 14)] + pl.ADAPTIVE_A
CHANNELS = {"f32": (8, 6), "f16": (8, 12, 6)}   # vector and scalar forms (12 halves are no whole vector)


@pytest.mark.parametrize("case", WINDOWED, ids=cid)
def test_windowed_form_has_the_bits_of_the_rule(gpu, case):
    assert expected_form(pl.SHAPE_A, case) == WIN
    for dt in sorted(DTYPES):
        for c in CHANNELS[dt]:
            check(pl.SHAPE_A, case, dt, c)


def test_all_windowed_instantiations_ran(gpu):
    """(runs after the parametrised test above, whose names it collects)"""
    want = {kname(WIN, d, v) for d in DTYPES.values() for v in (True, False)}
    if not want <= FORMS_SEEN:
        for dt in DTYPES:
            for c in (8, 6):
                check(pl.SHAPE_A, pl.TABLE_A[0], dt, c)
    assert want <= FORMS_SEEN, FORMS_SEEN


# ---- 2. the cooperative form -------------------------------------------------------------------------------------------------------------
LARGE = [(pl.SHAPE_B, c) for c in pl.TABLE_B] + [(pl.SHAPE_A, c) for c in pl.TABLE_A if c[0] == (11, 14)] + [(pl.SHAPE_B, (2, 3)), (pl.SHAPE_B, (1, 2))]


@pytest.mark.parametrize("shape3,case", LARGE, ids=[cid(c) for _, c in LARGE])
def test_large_windows(gpu, shape3, case):
    """table B, the whole-map row of table A and the two coarse adaptive sizes: the form is the one the largest window's tap count calls for; a
    case under the threshold is held to the bits of the rule, the others to torch float64 at the fp32 / fp16 bar.  72 channels are more than one
    channel chunk of every instantiation."""
    for dt in sorted(DTYPES):
        for c in (8, 6, 72):
            check(shape3, case, dt, c)


def test_large_windows_on_offset_data(gpu):
    """30 + U[-1, 1): the mean is 30 times the spread, what is left of an error in the sum shows at once"""
    case = pl.TABLE_B[0]
    assert expected_form(pl.SHAPE_B, case) == COOP and expected_form(pl.SHAPE_B, (1, 2)) == COOP
    for dt in sorted(DTYPES):
        for c in (8, 6, 72):
            check(pl.SHAPE_B, case, dt, c, offset=30.0)
            check(pl.SHAPE_B, (1, 2), dt, c, offset=30.0)


def test_all_cooperative_instantiations_ran_and_the_worst_errors(gpu):
    want = {kname(COOP, d, v) for d in DTYPES.values() for v in (True, False)}
    if not want <= FORMS_SEEN:
        for dt in DTYPES:
            for c in (8, 6):
                check(pl.SHAPE_B, pl.TABLE_B[0], dt, c)
    assert want <= FORMS_SEEN, FORMS_SEEN
    for (form, dt), (e, m) in sorted(WORST.items()):
        print("%s %s vs torch float64: max-based %.3e, element-wise %.3e" % (form, dt, e, m))


# ---- 3. the switch ----------------------------------------------------------------------------------------------------------------------
def test_form_switch(gpu):
    name = hipops.avgpool2d_kernel_name
    names = [name((1, 40, 40, 8), k, 1, 0) for k in range(1, 41)]
    flips = [k for k in range(2, 41) if names[k - 1] != names[k - 2]]
    assert len(flips) == 1 and names[0] == kname(WIN, np.float32, True) and names[-1] == kname(COOP, np.float32, True), names
    kf = flips[0]
    assert kf * kf >= T >= 64 and (kf - 1) ** 2 < T, (kf, T)
    for k in (kf - 1, kf):
        for n in (1, 2, 7):
            assert name((n, 40, 40, 8), k, 1, 0) == names[k - 1] and name((n, 40, 40, 8), k, 5, 0, half=True).startswith(names[k - 1].split("<")[0])
    # one launch on each side (stride 5: 6 x 6 outputs)
    x = np.ascontiguousarray(data((1, 40, 40), "f32")[..., :8])
    below, nb = run(x, ((kf - 1, kf - 1), (5, 5), (0, 0), False, True, None))
    above, na = run(x, ((kf, kf), (5, 5), (0, 0), False, True, None))
    assert nb == kname(WIN, np.float32, True) and na == kname(COOP, np.float32, True), (nb, na)
    ct.assert_same_bits(below, pl.avgpool2d_ref(x, (kf - 1, kf - 1), (5, 5), acc=np.float32), "one tap row below the switch")
    util.assert_parity(above, pl.avgpool2d_f64_torch(x, (kf, kf), (5, 5)), what="at the switch")


# ---- 4. determinism ---------------------------------------------------------------------------------------------------------------------
BOTH_FORMS = [(pl.SHAPE_A, pl.TABLE_A[20]), (pl.SHAPE_B, pl.TABLE_B[4]), (pl.SHAPE_B, (1, 2))]   # k3 s1 p1 ceil; k17x19 p8x9; adaptive
assert BOTH_FORMS[0][1][0] == (3, 3) and BOTH_FORMS[1][1][0] == (17, 19)


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("shape3,case", BOTH_FORMS, ids=["windowed", "cooperative", "cooperative_adaptive"])
def test_same_bits_twice_and_per_image(gpu, shape3, case, dt):
    """two launches give the same bits; a batch of 5 gives the bits of its single images"""
    r = np.random.Generator(np.random.Philox(7))
    for c in (8, 6, 72):
        x = (r.random((5,) + shape3[1:] + (c,), dtype=np.float32) * 2 - 1).astype(DTYPES[dt])
        y5, k5 = run(x, case)
        assert k5.startswith(expected_form(shape3, case) + "<"), k5
        ct.assert_same_bits(y5, run(x, case)[0], "two launches, c=%d" % c)
        for i in range(5):
            y1, k1 = run(x[i:i + 1], case)
            assert k1 == k5
            ct.assert_same_bits(y5[i:i + 1], y1, "image %d, c=%d" % (i, c))


# ---- 5. views and containment: checks (a) - (d) of tests/test_gpu_containment.py ------------------------------------------------------------
class ViewCase:
    def __init__(self, vid, half, shape3, c, case, form, vec, **views):
        self.id, self.half, self.shape3, self.c, self.case, self.form, self.vec, self.views = vid, half, shape3, c, case, form, vec, views
        self.entries = ("si_hip_avgpool2d_f16" if half else "si_hip_avgpool2d_f32",)
        self.dt = "f16" if half else "f32"
        self.dtype = DTYPES[self.dt]

    def input(self):
        return np.ascontiguousarray(data(self.shape3, self.dt)[..., :self.c])

    def run(self, F):
        y, _ = run(self.input(), self.case, in_fill=F, out_fill=F, full=True, **self.views)
        return ct.Out("y", y, self.views.get("out_c_off", 0), self.c)


_W, _CO, _AD = pl.TABLE_A[22], pl.TABLE_B[5], (1, 2)   # k3 s1 p1 ceil, pad excluded; k17x19 s8x9 p8x9, pad excluded; adaptive 23 x 29 -> 1 x 2
VIEW_CASES = []
for _half, _sfx, _v in ((False, "f32", 4), (True, "f16", 8)):
    VIEW_CASES += [
        # an input embedded at a channel offset of a wider buffer, an output slice of a wider buffer; 16-byte aligned on both sides
        ViewCase("windowed_vector_" + _sfx, _half, pl.SHAPE_A, 8, _W, WIN, True, in_ld=24, in_c_off=8, out_ld=32, out_c_off=16),
        ViewCase("cooperative_vector_" + _sfx, _half, pl.SHAPE_B, 72, _CO, COOP, True, in_ld=88, in_c_off=8, out_ld=96, out_c_off=16),
        # odd offsets and strides
        ViewCase("windowed_scalar_" + _sfx, _half, pl.SHAPE_A, 6, _W, WIN, False, in_ld=9, in_c_off=2, out_ld=7, out_c_off=1),
        ViewCase("cooperative_scalar_" + _sfx, _half, pl.SHAPE_B, 72, _AD, COOP, False, in_ld=75, in_c_off=3, out_ld=77, out_c_off=2),
        # vector-sized channels and strides behind a pointer that is 8 bytes off a 16-byte boundary: the scalar form
        ViewCase("windowed_unaligned_" + _sfx, _half, pl.SHAPE_A, 8, _W, WIN, False, in_ld=16, in_c_off=_v // 2, out_ld=16, out_c_off=8),
        ViewCase("cooperative_unaligned_" + _sfx, _half, pl.SHAPE_B, 8, _CO, COOP, False, in_ld=16, in_c_off=0, out_ld=24, out_c_off=_v // 2),
        # the input slice ends where its buffer ends
        ViewCase("windowed_last_slice_" + _sfx, _half, pl.SHAPE_A, 6, pl.TABLE_A[12], WIN, False, in_ld=14, in_c_off=8, out_ld=6, out_c_off=0),
    ]


@pytest.mark.parametrize("case", VIEW_CASES, ids=[c.id for c in VIEW_CASES])
def test_views_and_containment(gpu, case):
    del hipops.LAST_ENTRIES[:]
    plain = case.run(hipops.ByteFill(0x00))
    plain_kernel = hipops.LAST_KERNEL_NAME["si_hip_avgpool2d"]
    assert set(case.entries) <= set(hipops.LAST_ENTRIES), hipops.LAST_ENTRIES
    assert plain_kernel == kname(case.form, case.dtype, case.vec), plain_kernel
    ct.assert_outside_fill(plain.full, plain.c_off, plain.c, 0x00, case.id + ", plain run")
    # the value too: nothing of the gaps between the input's pixels (NaN under 0xFF) reached the output
    dense, dense_kernel = run(case.input(), case.case)
    if dense_kernel == plain_kernel:   # (an unaligned view takes the scalar form, the dense array the vector form: the same bits only when windowed)
        ct.assert_same_bits(np.ascontiguousarray(plain.dest), dense, case.id + " vs the dense run")
    if case.form == WIN:
        ct.assert_same_bits(np.ascontiguousarray(plain.dest), np.ascontiguousarray(emulation(case.shape3, case.dt, case.case)[..., :case.c]),
                            case.id + " vs the rule")
    for byte in ct.PATTERNS:
        with hipops.guard_bands(byte) as g:      # (a) all bands and (d) the input are compared when the block ends
            out = case.run(hipops.ByteFill(byte))
        what = "%s under 0x%02X" % (case.id, byte)
        assert g.checked == 2, "%s: the guard saw %d buffers" % (what, g.checked)   # x, y
        assert hipops.LAST_KERNEL_NAME["si_hip_avgpool2d"] == plain_kernel, what
        ct.assert_outside_fill(out.full, out.c_off, out.c, byte, what)                              # (b)
        ct.assert_same_bits(out.dest, plain.dest, what + ": guarded + pattern-filled vs plain")    # (c)


# ---- engine helpers --------------------------------------------------------------------------------------------------------------------------
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


def one_op_graph(shape, adaptive=None, **kw):
    """input -> one pool -> output, for an NHWC shape"""
    n, h, w, c = shape
    b = mg.PnnxBuilder(seed=5)
    x = b.input((n, c, h, w))
    b.output(b.adaptive_avgpool(x, adaptive, **kw) if adaptive else b.avgpool(x, **kw))
    return b


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_process_usable(gpu, tmp_path):
    x = np.ascontiguousarray(data(pl.SHAPE_A, "f32")[..., :8])
    H = _native.hip()
    src, dst = hipops.DeviceBuffer(x.nbytes), hipops.DeviceBuffer(4 * x.nbytes)

    def entry(d):
        hipops._chk(H.si_hip_avgpool2d_f32(C.byref(d), src.ptr, dst.ptr, None), "si_hip_avgpool2d_f32")

    with pytest.raises(hipops.HipError):
        hipops.avgpool2d(x, 3, 2, 2)                                            # p > k / 2
    with pytest.raises(hipops.HipError):
        hipops.avgpool2d(x.astype(np.float16), (2, 3), 2, (1, 2))
    d = hipops.avgpool2d_desc(x.shape, 3, 2, 1, divisor_override=3)
    d.oh += 1                                                                   # divisor_override with oh off by one
    with pytest.raises(hipops.HipError):
        entry(d)
    with pytest.raises(hipops.HipError):
        entry(hipops.avgpool2d_desc(x.shape, 3, 2, 1, in_ld=7))                 # ld < c (the wrapper would not build such a view: the entry itself)
    for fn in ("si_hip_avgpool2d_f32", "si_hip_avgpool2d_f16"):
        for a, b in ((None, dst.ptr), (src.ptr, None)):                         # null pointers
            with pytest.raises(hipops.HipError):
                hipops._chk(getattr(H, fn)(C.byref(hipops.avgpool2d_desc(x.shape, 3, 2, 1)), a, b, None), fn)
    with pytest.raises(hipops.HipError):
        entry(hipops.adaptive_avgpool2d_desc(x.shape, (0, 3)))                  # adaptive with oh = 0

    def load(b, tag):
        pp, bp = save(b, tmp_path, tag)
        with pytest.raises(StatusError) as ei:
            Engine().load_model(pp, bp)
        return ei.value.status

    s = (2, 11, 14, 8)
    b = one_op_graph(s, k=3, s=2, p=1)
    b.lines = [ln.replace(" padding=(1,1) ", " padding=(2,2) ") for ln in b.lines]
    assert "padding=(2,2)" in b.lines[1] and load(b, "half_kernel") == Status.kUnsupport        # padding=(2,2) with kernel_size=(3,3)
    b = one_op_graph(s, k=3, s=2, p=1)
    b.lines = [ln.replace(" divisor_override=None ", " divisor_override=0 ") for ln in b.lines]
    assert "divisor_override=0" in b.lines[1] and load(b, "divisor_zero") == Status.kUnsupport
    b = one_op_graph(s, k=3, s=2, p=1)
    b.lines = [ln.replace(" ceil_mode=False ", " ceil_mode=True ") for ln in b.lines]              # 14 -> 7 (floor) but 8 (ceil): the file's shape is not the rule's
    assert "ceil_mode=True" in b.lines[1] and load(b, "shape") == Status.kErrorShape
    b = one_op_graph(s, k=3, s=2, p=1)
    b.lines = [ln.replace(" count_include_pad=True ", " ") for ln in b.lines]
    assert "count_include_pad" not in b.lines[1] and load(b, "missing_key") == Status.kFail        # a missing required key
    # ... and the same process launches, loads and runs afterwards
    ct.assert_same_bits(run(x, pl.TABLE_A[8])[0], np.ascontiguousarray(emulation(pl.SHAPE_A, "f32", pl.TABLE_A[8])[..., :8]), "good launch after the refusals")
    pp, bp = save(one_op_graph(s, k=3, s=2, p=1), tmp_path, "good")
    _, out = run_engine(pp, bp, x)
    ct.assert_same_bits(out, hipops.avgpool2d(x, 3, 2, 1), "good model after the refusals")


# ---- 7. engine ---------------------------------------------------------------------------------------------------------------------------
ONE_OP = {
    "nn.AvgPool2d_2x2": ("nn.AvgPool2d", (2, 12, 16, 16), dict(k=2), WIN),                                                            # the DenseNet transition
    "nn.AvgPool2d_inception": ("nn.AvgPool2d", (2, 11, 14, 8), dict(k=3, s=1, p=1, count_include_pad=False), WIN),
    "nn.AvgPool2d_resnet_d": ("nn.AvgPool2d", (2, 11, 15, 6), dict(k=2, s=2, ceil_mode=True, count_include_pad=False), WIN),          # odd map, scalar form
    "nn.AvgPool2d_divisor": ("nn.AvgPool2d", (2, 11, 14, 8), dict(k=(5, 3), s=(3, 2), p=(2, 1), divisor_override=3), WIN),
    "nn.AvgPool2d_lraspp": ("nn.AvgPool2d", (2, 23, 29, 72), dict(k=(20, 23), s=(3, 6)), COOP),                                       # a window over most of the map
    "F.avg_pool2d": ("F.avg_pool2d", (2, 11, 14, 8), dict(k=(3, 2), s=(3, 2), p=(0, 1), ceil_mode=True, functional=True), WIN),
    "nn.AdaptiveAvgPool2d_6x6_of_13": ("nn.AdaptiveAvgPool2d", (2, 13, 13, 16), dict(adaptive=(6, 6)), WIN),
    "nn.AdaptiveAvgPool2d_1x2_of_23x29": ("nn.AdaptiveAvgPool2d", (2, 23, 29, 8), dict(adaptive=(1, 2)), COOP),
    "nn.AdaptiveAvgPool2d_up": ("nn.AdaptiveAvgPool2d", (2, 11, 14, 8), dict(adaptive=(13, 20)), WIN),                                        # pooling up
    "F.adaptive_avg_pool2d": ("F.adaptive_avg_pool2d", (2, 11, 14, 6), dict(adaptive=(7, 7), functional=True), WIN),
}


@pytest.mark.parametrize("which", sorted(ONE_OP))
def test_engine_one_op_graph(gpu, tmp_path, which):
    """LoadModel -> Forward -> Extract reproduces the op-level result bit for bit and the torch float64 evaluation of the file"""
    want, s, kw, form = ONE_OP[which]
    b = one_op_graph(s, **kw)
    typ, _, _, _, prm = _parse(b.lines[1])
    assert typ == want, typ
    pp, bp = save(b, tmp_path)
    x = util.rng_uniform(9, s, -1.0, 1.0)
    e, got = run_engine(pp, bp, x)
    args = pl.pool_args(typ, prm)
    op_level, kernel = run(x, args["adaptive"] if "adaptive" in args else (args["k"], args["s"], args["p"], args["ceil_mode"],
                                                                            args["count_include_pad"], args["divisor_override"]))
    ct.assert_same_bits(got, op_level, "engine vs op level")
    util.assert_parity(got, pl.eval_graph(b, x), what=which)
    layers = [L for L in e.profile() if L["type"] in pl.POOL_TYPES]
    assert len(layers) == 1 and layers[0]["type"] == typ, layers
    assert layers[0]["kernel"] == kernel == kname(form, np.float32, s[3] % 4 == 0), (layers, kernel)


def test_divisible_adaptive_shapes_keep_their_kernels(gpu, tmp_path):
    """12 x 16 -> 3 x 4 and -> 1 x 1 run si_hip_adaptive_avgpool2d_f32 as before, with its bits"""
    s = (2, 12, 16, 8)
    x = util.rng_uniform(9, s, -1.0, 1.0)
    for o in ((3, 4), (1, 1)):
        pp, bp = save(one_op_graph(s, adaptive=o), tmp_path, "d%d" % o[0])
        e, got = run_engine(pp, bp, x)
        ct.assert_same_bits(got, hipops.adaptive_avgpool2d(x, o), "divisible %s" % (o,))
        assert [L["kernel"] for L in e.profile() if L["type"] == "nn.AdaptiveAvgPool2d"] == ["avgpool"]


def test_pool_feeds_a_concat(gpu, tmp_path):
    """the Inception pool branch without its 1x1 conv and a PSP-style non-divisible adaptive pool of the same size, both straight into the
    concat: they write into the concat buffer's channel slices (the alias the data-movement layers get) and read a strided view"""
    b = mg.PnnxBuilder(seed=7)
    x = b.input((2, 4, 13, 13))
    f = b.relu(b.conv(x, 16, 3, 1, 1))
    g = b.cat([b.relu(b.conv(f, 8, 1, 1, 0)), b.relu(b.conv(f, 8, 3, 1, 1))])       # g's operands are aliases: the pools read a 16-of-16 view
    p1 = b.avgpool(g, 3, 1, 1, count_include_pad=False)
    p2 = b.adaptive_avgpool(b.adaptive_avgpool(g, (6, 6)), (13, 13), functional=True)   # 13 -> 6 -> 13: both non-divisible
    b.output(b.conv(b.cat([g, p1, p2]), 4, 1, 1, 0))
    pp, bp = save(b, tmp_path)
    xin = util.rng_uniform(15, (2, 13, 13, 4), -1.0, 1.0)
    e, got = run_engine(pp, bp, xin)
    util.assert_parity(got, pl.eval_graph(b, xin), what="pools -> cat")
    alias = e.schedule()["alias"]
    assert p1 in alias and p2 in alias, e.schedule()
    pools = [L for L in e.profile() if L["type"] in pl.POOL_TYPES]
    assert [L["kernel"] for L in pools] == [kname(WIN, np.float32, True)] * 3, pools


def pool_layers(prof):
    return [L for L in prof if L["type"] in pl.POOL_TYPES]


TOYS = {
    # builder, NHWC input, fp32 kernels of the pool layers in file order ("avgpool": the divisible adaptive shapes' kernel family)
    "densenet": (mg.build_toy_densenet, (2, 33, 33, 3), [WIN + "<float, 4>"] * 3 + ["avgpool"]),
    "pspnet": (mg.build_toy_pspnet, (2, 52, 52, 3), ["avgpool"] + [WIN + "<float, 4>"] * 3),
}


@pytest.mark.parametrize("toy", sorted(TOYS))
def test_toy_model_fp32(gpu, tmp_path, toy):
    build, s, kernels = TOYS[toy]
    b = build()
    pp, bp = save(b, tmp_path)
    x = mg.synth_input(s)
    e, got = run_engine(pp, bp, x)
    ref = pl.eval_graph(b, x)
    print("toy %s fp32: max-based %.3e, element-wise %.3e" % (toy, util.rel_err(got, ref), util.mixed_err(got, ref)))
    util.assert_parity(got, ref, what="toy %s fp32" % toy)
    assert [L["kernel"] for L in pool_layers(e.profile())] == kernels, pool_layers(e.profile())
    # a captured graph replays the same bits
    _, g = run_engine(pp, bp, x, graph=1)
    util.assert_exact(g.view(np.uint32), got.view(np.uint32), "graph=1 vs eager")


@pytest.mark.parametrize("toy", sorted(TOYS))
def test_toy_model_rebatch(gpu, tmp_path, toy):
    """SetOption("batch", 5) on the batch-2 file: per image the same bits as batch-2 runs of the same images"""
    build, s, _ = TOYS[toy]
    pp, bp = save(build(), tmp_path)
    x5 = util.rng_uniform(21, (5,) + s[1:], 0.0, 1.0)
    _, y5 = run_engine(pp, bp, x5, batch=5)
    xs = np.concatenate([x5, x5[:1]], 0)   # pairs (0, 1), (2, 3), (4, 0)
    for i in range(0, 6, 2):
        _, y2 = run_engine(pp, bp, xs[i:i + 2])
        for j in range(2):
            if i + j < 5:
                util.assert_exact(y5[i + j].view(np.uint32), y2[j].view(np.uint32), "image %d" % (i + j))


@pytest.mark.parametrize("toy", sorted(TOYS))
def test_toy_model_fp16_storage(gpu, tmp_path, toy):
    """fp16=1: every pool layer runs its half kernel with no cast pair around it, and the error against fp64 is at most 2x that of the
    fp16-storage emulation (weights, the input and every layer's output rounded to fp16, fp64 arithmetic between) -- the factor of
    test_toy_cyclegan_fp16_storage"""
    build, s, kernels = TOYS[toy]
    b = build()
    pp, bp = save(b, tmp_path)
    x = mg.synth_input(s)
    e, got = run_engine(pp, bp, x, fp16=1)
    prof = e.profile()
    pools = pool_layers(prof)
    assert [L["kernel"] for L in pools] == [k.replace("<float, 4>", "<_Float16, 8>") for k in kernels], pools
    names = [L["name"] for L in prof]
    for L in pools:   # (InsertFp32Fallbacks names its casts <layer>.in_to_f32.<k> / <layer>.out_to_f16.<k>)
        assert not any(n.startswith(L["name"] + ".in_to_f32") or n.startswith(L["name"] + ".out_to_f16") for n in names), names
    ref = pl.eval_graph(b, x)
    emu = pl.eval_graph(b, x, rnd=pl.round_f16)
    e_engine, e_emu = util.rel_err(got, ref), util.rel_err(emu, ref)
    print("toy %s fp16 storage vs fp64: engine %.3e, fp16 emulation %.3e" % (toy, e_engine, e_emu))
    assert np.isfinite(got).all()
    assert e_engine <= 2.0 * e_emu, (e_engine, e_emu)
