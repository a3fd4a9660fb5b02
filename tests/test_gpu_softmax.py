"""GPU: softmax / log_softmax along one NHWC axis -- si_hip_softmax_f32 / _f16 (include/si_softmax.h).  Every form and instantiation
against torch float64 at the project's bars (util.REL_TOL for fp32, F16_TOL for fp16), the kernel name asserted each time; row sums;
stability under offsets and scales; torch's special values; determinism; strided views under guard bands; the refusals; and the layer
inside the engine: one-op graphs for the five type strings, a softmax reading a concat slice and one writing into a concat, the toy
classifier / segnet / U-Net with each head in fp32, under graph capture, re-batched, and with fp16 storage.  Every engine test fails
without the layer (LoadModel rejects the types), every op-level test without the kernel (the symbols are missing).

Every check prints its figures before it asserts (run with -s); the closing test of section 2 prints the worst max-based and element-wise
errors against torch float64 and the worst |row sum - 1| per form, dtype and function."""
import ctypes as C
import functools

import numpy as np
import pytest

import containment as ct
import softmax_reference as sr
import util
from ct_reference import _parse
from simpleinfer_amd import _native, hipops, modelgen as mg
from simpleinfer_amd.engine import Engine, Status, StatusError
from test_gpu_f16 import F16_TOL

pytestmark = pytest.mark.gpu

DTYPES = {"f32": np.float32, "f16": np.float16}
BAR = {"f32": util.REL_TOL, "f16": F16_TOL}
G, B = sr.header_enum("SI_SOFTMAX_GROUP_MAX_C"), sr.header_enum("SI_SOFTMAX_BLOCK_MAX_C")

SEEN = set()
WORST = {}   # (form, dt, log) -> [max-based, element-wise, row sum] worst error against torch float64


def vectorised(shape, dtype, **views):
    v = 16 // np.dtype(dtype).itemsize
    return all(int(k) % v == 0 for k in (shape[3], views.get("in_ld") or shape[3], views.get("out_ld") or shape[3], views.get("in_c_off", 0),
                                        views.get("out_c_off", 0)))


def run(x, axis, log=False, **views):
    y = hipops.softmax(x, axis, log, **views)
    return y, hipops.LAST_KERNEL_NAME["si_hip_softmax"]


@functools.lru_cache(maxsize=None)
def data(shape, dt, seed=41):
    x = util.rng_uniform(seed, shape, -4.0, 4.0).astype(DTYPES[dt])
    x.setflags(write=False)
    return x


def sums_to_one(got, axis, log, rel, what):
    g = np.asarray(got, np.float64)
    s = (np.exp(g) if log else g).sum(axis=axis)
    err = float(np.abs(s - 1.0).max())
    print("%s: worst |row sum - 1| = %.3e" % (what, err))
    assert err <= rel, "%s: a row sums to 1 within %.3e only (bar %.1e)" % (what, err, rel)
    return err


def check(x, axis, log, ref_of=None, what=""):
    """one launch: the kernel the shape calls for, within the bar of torch float64 (of `ref_of` if given, else of x itself), rows sum to 1"""
    dt = "f32" if x.dtype == np.float32 else "f16"
    got, kernel = run(x, axis, log)
    form = sr.expected_form(x.shape, axis)
    SEEN.add(kernel)
    what = "%s %s %s axis %d %s [%s]" % (what, "log_softmax" if log else "softmax", x.shape, axis, dt, kernel)
    assert got.dtype == x.dtype and got.shape == x.shape and kernel == sr.kname(form, x.dtype, vectorised(x.shape, x.dtype)), what
    ref = sr.softmax_f64_torch(x if ref_of is None else ref_of, axis, log)
    e = util.rel_err(got, ref) if np.isfinite(got).all() else float("nan")
    m = util.mixed_err(got, ref) if np.isfinite(got).all() else float("nan")
    print("%s: max-based %.3e, element-wise %.3e" % (what, e, m))
    util.assert_parity(got.astype(np.float64), ref, rel=BAR[dt], what=what)
    srr = sums_to_one(got, axis, log, BAR[dt], what)
    w = WORST.setdefault((form, dt, log), [0.0, 0.0, 0.0])
    w[0], w[1], w[2] = max(w[0], e), max(w[1], m), max(w[2], srr)
    return got


# ---- 1. the contiguous axis ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log", [False, True], ids=["softmax", "log_softmax"])
@pytest.mark.parametrize("c", sr.contig_c())
def test_contiguous_axis(gpu, c, log):
    """rows 1, 3 and 130 (one row, less than a group's share of a workgroup, more than one workgroup) of every channel count of the table,
    both dtypes: the form is the one the header's thresholds call for, the instantiation the one c allows"""
    for dt in sorted(DTYPES):
        for rows in sr.CONTIG_ROWS:
            check(data((rows, 1, 1, c), dt), 3, log)


def test_contiguous_axis_over_pixels(gpu):
    """the 21 classes of a segmentation head over a map: rows are pixels of a rank-4 tensor, more rows than one workgroup holds"""
    for dt in sorted(DTYPES):
        for log in (False, True):
            check(data((2, 9, 11, 21), dt), 3, log)
            check(data((2, 9, 11, 24), dt), 3, log)


# ---- 2. the strided axes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log", [False, True], ids=["softmax", "log_softmax"])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_strided_axes(gpu, axis, log):
    for shape in sr.STRIDED_SHAPES_F32:
        check(data(shape, "f32"), axis, log)
    for shape in sr.STRIDED_SHAPES_F16:
        check(data(shape, "f16"), axis, log)


def test_every_kernel_ran_and_the_worst_errors(gpu):
    """(runs after the parametrised tests above, whose names it collects)"""
    want = {sr.kname(f, d, v) for f in sr.FORMS for d in DTYPES.values() for v in (True, False)}
    if not want <= SEEN:
        for shape, axis in FORM_CASES:
            for dt in sorted(DTYPES):
                check(data(shape, dt), axis, False)
    assert want <= SEEN, sorted(want - SEEN)
    for (form, dt, log), (e, m, s) in sorted(WORST.items()):
        print("%s %s %s vs torch float64: max-based %.3e, element-wise %.3e, row sum %.3e" % (form, dt, "log_softmax" if log else "softmax", e, m, s))


# one (shape, axis) per form and instantiation: vector and scalar channel counts in both dtypes (a c of 6 or 21 is scalar in both; 8 and its
# multiples are vectors in both)
FORM_CASES = [((5, 1, 1, 21), 3), ((5, 1, 1, 64), 3), ((5, 1, 1, G + 1), 3), ((5, 1, 1, G + 8), 3), ((5, 1, 1, B + 5), 3), ((5, 1, 1, B + 8), 3),
              ((5, 5, 7, 8), 1), ((5, 5, 7, 6), 2), ((5, 1, 33, 8), 2), ((5, 12, 3, 6), 1)]
FORM_IDS = ["%s_c%d_axis%d" % (sr.expected_form(s, a), s[3], a) for s, a in FORM_CASES]


def test_form_cases_cover_every_kernel():
    names = {sr.kname(sr.expected_form(s, a), d, vectorised(s, d)) for s, a in FORM_CASES for d in DTYPES.values()}
    assert names == {sr.kname(f, d, v) for f in sr.FORMS for d in DTYPES.values() for v in (True, False)}


# ---- 3. stability ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,axis", FORM_CASES, ids=FORM_IDS)
def test_stability(gpu, shape, axis):
    """x + 100, x - 100: the result of x itself within the bar (softmax is invariant under a shift; the shifted input carries its own
    rounding of 100 + x, 4e-6, which the bar covers).  x * 1e30 and halves scaled to +-60000: torch float64 on the scaled values.  A kernel
    that does not subtract the maximum gives Inf / NaN here."""
    x = np.array(data(shape, "f32")) / np.float32(4)                  # U[-1, 1)
    for log in (False, True):
        for off in (100.0, -100.0):
            check((x + np.float32(off)).astype(np.float32), axis, log, ref_of=x, what="offset %+g" % off)
        check(x * np.float32(1e30), axis, log, what="scaled by 1e30")
    h = (x * np.float32(60000)).astype(np.float16)
    assert np.isfinite(h).all() and np.abs(h.astype(np.float32)).max() > 30000
    check(h, axis, False, what="halves at +-60000")
    # log_softmax of such rows is down to -120000, below the range of a half: the result must be the float64 value rounded to a half,
    # -inf where that is -inf, and within the bar where it is finite
    got, _ = run(h, axis, True)
    ref = sr.softmax_f64_torch(h, axis, True)
    with np.errstate(over="ignore"):
        inf = np.isinf(ref.astype(np.float16))
    assert not np.isnan(got).any() and np.array_equal(np.isneginf(got), inf), "halves at +-60000, log_softmax: -inf where float64 rounds to it"
    util.assert_parity(np.where(inf, 0.0, got.astype(np.float64)), np.where(inf, 0.0, ref), rel=F16_TOL, what="halves at +-60000, log_softmax")


# ---- 4. special values -----------------------------------------------------------------------------------------------------------------------
def with_special_rows(x, axis):
    """(x with the first 8 rows along `axis`, in the order of the other axes, replaced by sr.special_rows; its twin in which the four special
    rows 1, 3, 5, 6 keep x's own finite values: every other row is the same in both; the function that lists an array's rows)"""
    moved = np.moveaxis(np.array(x), axis, -1)
    rows = moved.reshape(-1, x.shape[axis]).copy()
    assert rows.shape[0] >= 8
    twin = rows.copy()
    rows[:8] = sr.special_rows(x.shape[axis], x.dtype)
    twin[[0, 2, 4, 7]] = rows[[0, 2, 4, 7]]
    back = lambda r: np.ascontiguousarray(np.moveaxis(r.reshape(moved.shape), -1, axis))
    return back(rows), back(twin), lambda y: np.moveaxis(np.asarray(y), axis, -1).reshape(rows.shape)


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("shape,axis", FORM_CASES, ids=FORM_IDS)
def test_special_values(gpu, shape, axis, dt):
    shape = (9,) + shape[1:] if axis == 3 else shape
    x, plain, rows_of = with_special_rows(data(shape, dt), axis)
    assert np.isfinite(plain).all()
    for log in (False, True):
        got, kernel = run(x, axis, log)
        assert kernel == sr.kname(sr.expected_form(shape, axis), x.dtype, vectorised(shape, x.dtype)), kernel
        ref = sr.softmax_f64_torch(x, axis, log)
        g, r, xr = rows_of(got), rows_of(ref), rows_of(x)
        what = "%s %s axis %d %s" % ("log_softmax" if log else "softmax", shape, axis, dt)
        assert np.array_equal(np.isnan(g), np.isnan(r)), what + ": NaN mask differs from torch's"
        assert np.isnan(g[[3, 5, 6]]).all() and not np.isnan(g[[0, 1, 2, 4, 7]]).any() and not np.isnan(g[8:]).any(), what
        minus = np.isneginf(xr[1])
        if minus.any():
            assert (g[1][minus] == (-np.inf if log else 0.0)).all(), what + ": -inf elements of a finite row"
        assert np.array_equal(np.isinf(g), np.isinf(r.astype(x.dtype))), what
        fin = np.isfinite(r.astype(x.dtype))
        util.assert_parity(np.where(fin, g.astype(np.float64), 0.0), np.where(fin, r, 0.0), rel=BAR[dt], what=what)
        # the neighbours: the bits of the launch whose rows 1, 3, 5 and 6 are finite (every other row is the same)
        p = rows_of(run(plain, axis, log)[0])
        keep = [0, 2, 4, 7] + list(range(8, g.shape[0]))
        ct.assert_same_bits(np.ascontiguousarray(g[keep]), np.ascontiguousarray(p[keep]), what + ": neighbouring rows")


# ---- 5. determinism --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("shape,axis", FORM_CASES, ids=FORM_IDS)
def test_same_bits_twice_and_per_image(gpu, shape, axis, dt):
    """two launches give the same bits; a batch of 5 gives the bits of its single images (the reduced axis is never the batch here)"""
    x = data(shape, dt, seed=7)
    assert shape[0] == 5 and axis != 0
    for log in (False, True):
        y5, k5 = run(x, axis, log)
        ct.assert_same_bits(y5, run(x, axis, log)[0], "two launches")
        for i in range(5):
            y1, k1 = run(x[i:i + 1], axis, log)
            assert k1 == k5
            ct.assert_same_bits(y5[i:i + 1], y1, "image %d" % i)


@pytest.mark.parametrize("c", [21, 64, G + 1, G + 8, B + 5, B + 8])
def test_a_row_alone_and_among_129_others(gpu, c):
    for dt in sorted(DTYPES):
        x = data((130, 1, 1, c), dt, seed=9)
        for log in (False, True):
            y, k = run(x, 3, log)
            for i in (0, 77, 129):
                y1, k1 = run(x[i:i + 1], 3, log)
                assert k1 == k
                ct.assert_same_bits(y[i:i + 1], y1, "row %d of 130, c=%d %s" % (i, c, dt))


# ---- 6. views and containment: checks (a) - (d) of tests/test_gpu_containment.py ----------------------------------------------------------------
class ViewCase:
    def __init__(self, vid, half, shape, axis, log, form, vec, **views):
        self.id, self.half, self.shape, self.axis, self.log, self.form, self.vec, self.views = vid, half, shape, axis, log, form, vec, views
        self.entries = ("si_hip_softmax_f16" if half else "si_hip_softmax_f32",)
        self.dt = "f16" if half else "f32"
        self.dtype = DTYPES[self.dt]
        self.c = shape[3]

    def input(self):
        return data(self.shape, self.dt)

    def run(self, F):
        y, _ = run(self.input(), self.axis, self.log, in_fill=F, out_fill=F, full=True, **self.views)
        return ct.Out("y", y, self.views.get("out_c_off", 0), self.c)


VIEW_CASES = []
for _half, _sfx, _v in ((False, "f32", 4), (True, "f16", 8)):
    VIEW_CASES += [
        # an input embedded at a channel offset of a wider buffer, an output slice of a wider buffer; 16-byte aligned on both sides
        ViewCase("group_vector_" + _sfx, _half, (2, 5, 7, 8), 3, False, "group", True, in_ld=24, in_c_off=8, out_ld=32, out_c_off=16),
        ViewCase("block_vector_" + _sfx, _half, (3, 1, 1, G + 8), 3, True, "block", True, in_ld=G + 24, in_c_off=8, out_ld=G + 16, out_c_off=8),
        ViewCase("block_online_vector_" + _sfx, _half, (3, 1, 1, B + 8), 3, False, "block_online", True, in_ld=B + 24, in_c_off=16, out_ld=B + 16, out_c_off=0),
        ViewCase("strided_vector_axis0_" + _sfx, _half, (2, 5, 7, 8), 0, True, "strided", True, in_ld=24, in_c_off=8, out_ld=32, out_c_off=16),
        ViewCase("strided_online_vector_axis2_" + _sfx, _half, (3, 1, 33, 8), 2, False, "strided_online", True, in_ld=16, in_c_off=8, out_ld=24, out_c_off=8),
        # odd offsets and strides
        ViewCase("group_scalar_" + _sfx, _half, (2, 5, 7, 6), 3, True, "group", False, in_ld=9, in_c_off=2, out_ld=7, out_c_off=1),
        ViewCase("block_scalar_" + _sfx, _half, (3, 1, 1, G + 1), 3, False, "block", False, in_ld=G + 4, in_c_off=3, out_ld=G + 3, out_c_off=1),
        ViewCase("block_online_scalar_" + _sfx, _half, (2, 1, 1, B + 5), 3, True, "block_online", False, in_ld=B + 9, in_c_off=3, out_ld=B + 7, out_c_off=2),
        ViewCase("strided_scalar_axis1_" + _sfx, _half, (2, 5, 7, 6), 1, False, "strided", False, in_ld=9, in_c_off=2, out_ld=7, out_c_off=1),
        ViewCase("strided_online_scalar_axis1_" + _sfx, _half, (2, 12, 3, 6), 1, True, "strided_online", False, in_ld=11, in_c_off=5, out_ld=9, out_c_off=0),
        ViewCase("strided_scalar_axis2_" + _sfx, _half, (2, 5, 7, 6), 2, True, "strided", False, in_ld=8, in_c_off=1, out_ld=6, out_c_off=0),
        # vector-sized channels and strides behind a pointer that is 8 bytes off a 16-byte boundary: the scalar instantiation
        ViewCase("group_unaligned_" + _sfx, _half, (2, 5, 7, 8), 3, False, "group", False, in_ld=16, in_c_off=_v // 2, out_ld=16, out_c_off=8),
        ViewCase("strided_online_unaligned_axis1_" + _sfx, _half, (2, 12, 3, 8), 1, False, "strided_online", False, in_ld=16, in_c_off=0, out_ld=24, out_c_off=_v // 2),
        # the input slice ends where its buffer ends
        ViewCase("group_last_slice_" + _sfx, _half, (2, 5, 7, 6), 3, False, "group", False, in_ld=14, in_c_off=8, out_ld=6, out_c_off=0),
    ]


def test_view_cases_cover_what_the_issue_lists():
    assert {c.half for c in VIEW_CASES} == {False, True} and {c.vec for c in VIEW_CASES} == {False, True}
    assert {c.axis for c in VIEW_CASES} == {0, 1, 2, 3} and {c.form for c in VIEW_CASES} == set(sr.FORMS)
    for c in VIEW_CASES:
        assert sr.expected_form(c.shape, c.axis) == c.form and vectorised(c.shape, c.dtype, **c.views) == c.vec, c.id
    assert any(c.c % (16 // np.dtype(c.dtype).itemsize) == 0 and not c.vec for c in VIEW_CASES)   # the misaligned base pointer


@pytest.mark.parametrize("case", VIEW_CASES, ids=[c.id for c in VIEW_CASES])
def test_views_and_containment(gpu, case):
    del hipops.LAST_ENTRIES[:]
    plain = case.run(hipops.ByteFill(0x00))
    plain_kernel = hipops.LAST_KERNEL_NAME["si_hip_softmax"]
    assert set(case.entries) <= set(hipops.LAST_ENTRIES), hipops.LAST_ENTRIES
    assert plain_kernel == sr.kname(case.form, case.dtype, case.vec), plain_kernel
    ct.assert_outside_fill(plain.full, plain.c_off, plain.c, 0x00, case.id + ", plain run")
    # the value too: nothing of the gaps between the input's pixels (NaN under 0xFF, the largest value under 0x7B) reached the output
    dense, dense_kernel = run(case.input(), case.axis, case.log)
    if dense_kernel == plain_kernel:
        ct.assert_same_bits(np.ascontiguousarray(plain.dest), dense, case.id + " vs the dense run")
    util.assert_parity(np.ascontiguousarray(plain.dest).astype(np.float64), sr.softmax_f64_torch(case.input(), case.axis, case.log), rel=BAR[case.dt],
                       what=case.id)
    for byte in ct.PATTERNS:
        with hipops.guard_bands(byte) as g:      # (a) all bands and (d) the input are compared when the block ends
            out = case.run(hipops.ByteFill(byte))
        what = "%s under 0x%02X" % (case.id, byte)
        assert g.checked == 2, "%s: the guard saw %d buffers" % (what, g.checked)   # x, y
        assert hipops.LAST_KERNEL_NAME["si_hip_softmax"] == plain_kernel, what
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


def emit(b, x, typ, dim):
    if typ == "nn.Softmax2d":
        return b.softmax2d(x)
    return b.softmax(x, dim, functional=typ.startswith("F."), log="og" in typ)


def one_op_graph(typ, shape_file, dim):
    """input -> one softmax -> output, for the file's (NCHW or [N, F]) shape"""
    b = mg.PnnxBuilder(seed=5)
    b.output(emit(b, b.input(shape_file), typ, dim))
    return b


def softmax_layers(prof):
    return [L for L in prof if L["type"] in sr.SOFTMAX_TYPES]


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_process_usable(gpu, tmp_path):
    x = np.array(data((2, 5, 7, 8), "f32"))
    H = _native.hip()
    src, dst = hipops.DeviceBuffer(x.nbytes), hipops.DeviceBuffer(x.nbytes)

    def entry(d, fn="si_hip_softmax_f32", a=None, b=None):
        hipops._chk(getattr(H, fn)(C.byref(d), src.ptr if a is None else a.value, dst.ptr if b is None else b.value, None), fn)

    with pytest.raises(hipops.HipError):
        hipops.softmax(x, 4)                                                    # axis outside 0 .. 3
    with pytest.raises(hipops.HipError):
        hipops.softmax(x.astype(np.float16), 2, log=2)                          # log outside 0 / 1
    with pytest.raises(hipops.HipError):
        entry(hipops.softmax_desc(x.shape, 3, in_ld=7))                         # ld < c (the wrapper would not build such a view: the entry itself)
    with pytest.raises(hipops.HipError):
        entry(hipops.softmax_desc((2, 0, 7, 8), 3))                             # a non-positive size
    for fn in ("si_hip_softmax_f32", "si_hip_softmax_f16"):
        for a, b in ((C.c_void_p(None), None), (None, C.c_void_p(None))):        # null pointers
            with pytest.raises(hipops.HipError):
                entry(hipops.softmax_desc(x.shape, 3), fn, a, b)
    with pytest.raises(hipops.HipError):
        entry(hipops.softmax_desc((1, 16384, 16384, 8), 3))                     # element offsets of 2^31

    def load(b, tag):
        pp, bp = save(b, tmp_path, tag)
        with pytest.raises(StatusError) as ei:
            Engine().load_model(pp, bp)
        return ei.value.status

    # an unsupported rank or dim is refused at LoadModel, with the message (the log names the dim and the shape), not at Forward
    assert load(one_op_graph("nn.Softmax", (2, 6, 5), 1), "rank3") == Status.kUnsupport
    assert load(one_op_graph("F.log_softmax", (2, 6, 5, 7), 4), "dim4") == Status.kUnsupport
    assert load(one_op_graph("nn.LogSoftmax", (2, 6, 5, 7), -5), "dim_minus5") == Status.kUnsupport
    assert load(one_op_graph("F.softmax", (3, 10), 2), "rank2_dim2") == Status.kUnsupport
    b = one_op_graph("nn.Softmax", (2, 6, 5, 7), 1)
    b.lines = [ln.replace(" dim=1 ", " ") for ln in b.lines]
    assert "dim=" not in b.lines[1] and load(b, "missing_key") == Status.kFail               # a missing required key
    b = one_op_graph("nn.Softmax", (2, 6, 5, 7), 1)
    b.lines = [ln.replace(" dim=1 ", " dim=1.5 ") for ln in b.lines]
    assert "dim=1.5" in b.lines[1] and load(b, "float_dim") == Status.kFail                  # a dim that is not an int
    # ... and the same process launches, loads and runs afterwards
    util.assert_parity(run(x, 3)[0], sr.softmax_f64_torch(x, 3), what="good launch after the refusals")
    pp, bp = save(one_op_graph("nn.Softmax", (2, 8, 5, 7), 1), tmp_path, "good")
    _, out = run_engine(pp, bp, x)
    ct.assert_same_bits(out, hipops.softmax(x, 3), "good model after the refusals")


# ---- 8. engine ---------------------------------------------------------------------------------------------------------------------------
ONE_OP = [(typ, (2, 6, 5, 7), dim) for typ in sr.SOFTMAX_TYPES if typ != "nn.Softmax2d" for dim in (1, 2, 3, -1, -3)]
ONE_OP += [("nn.Softmax2d", (2, 6, 5, 7), None), ("nn.Softmax2d", (2, 8, 40, 3), None)]
ONE_OP += [(typ, (2, 8, 40, 3), 2) for typ in ("nn.Softmax", "F.log_softmax")]                       # the online strided form, vectors
ONE_OP += [(typ, (3, 10), dim) for typ in sr.SOFTMAX_TYPES if typ != "nn.Softmax2d" for dim in (1, -1)]
ONE_OP += [("nn.Softmax", (3, 1000), 1), ("nn.LogSoftmax", (3, G + 8), -1), ("F.softmax", (3, 10), 0), ("F.log_softmax", (3, 10), -2)]


@pytest.mark.parametrize("typ,shape_file,dim", ONE_OP, ids=["%s_%s_dim%s" % (t, "x".join(map(str, s)), d) for t, s, d in ONE_OP])
def test_engine_one_op_graph(gpu, tmp_path, typ, shape_file, dim):
    """LoadModel -> Forward -> Extract reproduces the op-level result bit for bit and the torch float64 evaluation of the file"""
    b = one_op_graph(typ, shape_file, dim)
    assert _parse(b.lines[1])[0] == typ
    pp, bp = save(b, tmp_path)
    rank = len(shape_file)
    nhwc = (shape_file[0], shape_file[2], shape_file[3], shape_file[1]) if rank == 4 else shape_file
    x = util.rng_uniform(9, nhwc, -4.0, 4.0)
    e, got = run_engine(pp, bp, x)
    axis = sr.nhwc_axis(-3 if dim is None else dim, rank)
    x4 = x if rank == 4 else x.reshape(x.shape[0], 1, 1, x.shape[1])
    op_level, kernel = run(x4, axis, "og" in typ)
    ct.assert_same_bits(got, op_level.reshape(got.shape), "engine vs op level")
    util.assert_parity(got, sr.eval_graph(b, x), what="%s %s dim %s" % (typ, shape_file, dim))
    layers = softmax_layers(e.profile())
    assert len(layers) == 1 and layers[0]["type"] == typ, layers
    assert layers[0]["kernel"] == kernel == sr.kname(sr.expected_form(x4.shape, axis), np.float32, x4.shape[3] % 4 == 0), (layers, kernel)


def test_softmax_reads_a_concat_slice_and_writes_into_a_concat(gpu, tmp_path):
    """a and q are written into the concat buffer in place (aliases): the softmax over a and the log_softmax over q (along H) read 8 of 32
    channels at a pixel stride of 32, and both write their own slices of the same buffer"""
    b = mg.PnnxBuilder(seed=7)
    x = b.input((2, 4, 9, 11))
    f = b.relu(b.conv(x, 16, 3, 1, 1))
    a, q = b.relu(b.conv(f, 8, 1, 1, 0)), b.relu(b.conv(f, 8, 3, 1, 1))
    s1, s2 = b.softmax(a, 1), b.log_softmax(q, 2, functional=True)
    b.output(b.conv(b.cat([a, q, s1, s2]), 4, 1, 1, 0))
    pp, bp = save(b, tmp_path)
    xin = util.rng_uniform(15, (2, 9, 11, 4), -1.0, 1.0)
    e, got = run_engine(pp, bp, xin)
    util.assert_parity(got, sr.eval_graph(b, xin), what="softmax <-> cat")
    alias = e.schedule()["alias"]
    assert all(o in alias for o in (a, q, s1, s2)), e.schedule()
    assert [L["kernel"] for L in softmax_layers(e.profile())] == [sr.kname("group", np.float32, True), sr.kname("strided_online", np.float32, True)]


TOYS = {
    # builder, NHWC input, the NHWC axis of dim 1 and the fp32 form of the head
    "classifier": (mg.build_toy_classifier, (2, 32, 32, 3), "group<float, 1>"),      # [2, 10]
    "segnet": (mg.build_toy_segnet, (2, 64, 64, 3), "group<float, 1>"),              # 21 classes per pixel
    "unet": (mg.build_toy_unet, (2, 64, 64, 3), "group<float, 4>"),                  # 4 classes per pixel
}
HEADS = ("softmax", "log_softmax")


def head_kernel(toy):
    form, inst = TOYS[toy][2].split("<")
    return "softmax_%s_kernel<%s" % (form, inst)


@pytest.mark.parametrize("head", HEADS)
@pytest.mark.parametrize("toy", sorted(TOYS))
def test_toy_model_fp32(gpu, tmp_path, toy, head):
    build, s, _ = TOYS[toy]
    b = build(head=head)
    pp, bp = save(b, tmp_path)
    x = mg.synth_input(s)
    e, got = run_engine(pp, bp, x)
    ref = sr.eval_graph(b, x)
    print("toy %s %s fp32: max-based %.3e, element-wise %.3e" % (toy, head, util.rel_err(got, ref), util.mixed_err(got, ref)))
    util.assert_parity(got, ref, what="toy %s %s fp32" % (toy, head))
    sums_to_one(got, got.ndim - 1, head == "log_softmax", util.REL_TOL, "toy %s %s" % (toy, head))
    assert [L["kernel"] for L in softmax_layers(e.profile())] == [head_kernel(toy)], softmax_layers(e.profile())
    # a captured graph replays the same bits
    _, g = run_engine(pp, bp, x, graph=1)
    util.assert_exact(g.view(np.uint32), got.view(np.uint32), "graph=1 vs eager")


@pytest.mark.parametrize("toy", sorted(TOYS))
def test_toy_model_rebatch(gpu, tmp_path, toy):
    """SetOption("batch", 5) on the batch-2 file: per image the same bits as batch-2 runs of the same images"""
    build, s, _ = TOYS[toy]
    pp, bp = save(build(head="softmax"), tmp_path)
    x5 = util.rng_uniform(21, (5,) + s[1:], 0.0, 1.0)
    _, y5 = run_engine(pp, bp, x5, batch=5)
    xs = np.concatenate([x5, x5[:1]], 0)   # pairs (0, 1), (2, 3), (4, 0)
    for i in range(0, 6, 2):
        _, y2 = run_engine(pp, bp, xs[i:i + 2])
        for j in range(2):
            if i + j < 5:
                util.assert_exact(y5[i + j].view(np.uint32), y2[j].view(np.uint32), "image %d" % (i + j))


@pytest.mark.parametrize("head", HEADS)
@pytest.mark.parametrize("toy", sorted(TOYS))
def test_toy_model_fp16_storage(gpu, tmp_path, toy, head):
    """fp16=1: the head runs its half kernel with no cast pair around it, and the error against fp64 is at most 2x that of the
    fp16-storage emulation -- the factor of test_toy_cyclegan_fp16_storage.  The emulation rounds the weights, the input and every layer's
    output to fp16, fp64 arithmetic between, and here the graph output too: only Conv2d / Linear / Detect write an fp32 graph output from
    their own epilogue (the files of the sibling tests end in one of those); any other last layer -- this head -- stores halves, which an
    output cast widens (EngineImpl::InsertOutputCasts), so one rounding to fp16 is part of what fp16 storage means for these files."""
    build, s, _ = TOYS[toy]
    b = build(head=head)
    pp, bp = save(b, tmp_path)
    x = mg.synth_input(s)
    e, got = run_engine(pp, bp, x, fp16=1)
    prof = e.profile()
    heads = softmax_layers(prof)
    assert len(heads) == 1 and heads[0]["kernel"].startswith("softmax_group_kernel<_Float16, "), heads
    names = [L["name"] for L in prof]
    for L in heads:   # (InsertFp32Fallbacks names its casts <layer>.in_to_f32.<k> / <layer>.out_to_f16.<k>)
        assert not any(n.startswith(L["name"] + ".in_to_f32") or n.startswith(L["name"] + ".out_to_f16") for n in names), names
    ref = sr.eval_graph(b, x)
    emu = sr.round_f16(sr.eval_graph(b, x, rnd=sr.round_f16))
    e_engine, e_emu = util.rel_err(got, ref), util.rel_err(emu, ref)
    print("toy %s %s fp16 storage vs fp64: engine %.3e, fp16 emulation %.3e" % (toy, head, e_engine, e_emu))
    assert np.isfinite(got).all()
    assert e_engine <= 2.0 * e_emu, (e_engine, e_emu)
