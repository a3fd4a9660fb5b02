"""GPU: torch.sum / mean / amax / amin over NHWC axes -- si_hip_reduce_f32 / _f16 (include/si_reduce.h).  Integer data whose sums are exact in
any order (bit for bit, both dtypes: a dropped or doubled element shows at any length); every form and instantiation against torch float64
at the project's bars (util.REL_TOL for fp32, F16_TOL for fp16), the kernel name asserted each time; torch's special values in every lane
role; determinism and batch invariance; strided views under guard bands; the refusals; and the layer inside the engine: one-op graphs for
the four type strings, a reduction reading a concat slice and reductions writing into a concat, the toy timm head / CBAM / coordinate
attention / channels-first LayerNorm in fp32, under graph capture, re-batched, and with fp16 storage.  Every engine test fails without the
layer (LoadModel rejects the types), every op-level test without the kernels (the symbols are missing).

Every check prints its figures before it asserts (run with -s); the closing test of section 2 prints the worst max-based and element-wise
errors against torch float64 per form and dtype."""
import ctypes as C
import functools

import numpy as np
import pytest

import containment as ct
import reduce_reference as rr
import util
from ct_reference import _parse
from simpleinfer_amd import _native, hipops, modelgen as mg
from simpleinfer_amd.engine import Engine, Status, StatusError
from test_gpu_f16 import F16_TOL

pytestmark = pytest.mark.gpu

DTYPES = {"f32": np.float32, "f16": np.float16}
BAR = {"f32": util.REL_TOL, "f16": F16_TOL}
G = rr.header_enum("SI_REDUCE_GROUP_MAX_C")

SEEN = set()
WORST = {}   # (form, dt) -> [max-based, element-wise] worst error against torch float64


def run(x, op, axes, **views):
    y = hipops.reduce(x, op, axes, **views)
    return y, hipops.LAST_KERNEL_NAME["si_hip_reduce"]


@functools.lru_cache(maxsize=None)
def data(shape, dt, seed=41):
    """U[-1, 3): off zero mean, so a sum does not measure its own cancellation"""
    x = util.rng_uniform(seed, shape, -1.0, 3.0).astype(DTYPES[dt])
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def integers(shape, dt, seed=43):
    """integers in [-8, 8]: every partial sum of up to 25600 of them is an integer far below 2^24, exact in float32 in any order; the
    test checks the totals against the range in which a half holds them after one rounding"""
    r = np.random.Generator(np.random.Philox(seed))
    x = r.integers(-8, 9, shape).astype(DTYPES[dt])
    x.setflags(write=False)
    return x


def expected_kernel(shape, axes, dtype, **views):
    return rr.kname(rr.expected_form(shape, axes), dtype, rr.vectorised(shape, axes, dtype, **views))


CASE_GROUPS = {"masks": [(s, m) for s in rr.MASK_SHAPES for m in rr.MASKS], "coop": rr.coop_cases()}
CASE_GROUPS.update({"rows_c%d" % c: [((p, 1, 1, c), 8) for p in rr.ROW_PIXELS] for c in rr.row_c()})


# ---- 1. exact, order-independent ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", sorted(CASE_GROUPS))
def test_exact_on_integers(gpu, group):
    """sum: the integer sum bit for bit (fp16: rounded once to half); mean: np.float32(sum) / np.float32(count) bit for bit (fp16: that
    quotient rounded once); amax / amin on arbitrary data: numpy's bits"""
    for shape, axes in CASE_GROUPS[group]:
        count = rr.positions(shape, axes)
        for dt in sorted(DTYPES):
            x = integers(shape, dt)
            total = x.astype(np.int64).sum(axis=rr.mask_axes(axes), keepdims=True)
            assert np.abs(total).max() < 2 ** 15, "the totals fit a half and a float exactly enough to round once"
            want_sum = total.astype(np.float32)
            assert np.array_equal(want_sum.astype(np.int64), total)
            want_mean = want_sum / np.float32(count)
            assert want_mean.dtype == np.float32
            for op, want in (("sum", want_sum), ("mean", want_mean)):
                got, kernel = run(x, op, axes)
                what = "%s %s mask %d %s [%s]" % (op, shape, axes, dt, kernel)
                assert kernel == expected_kernel(shape, axes, x.dtype), what
                ct.assert_same_bits(got, want.astype(x.dtype), what)
            a = data(shape, dt)
            for op, fn in (("amax", np.max), ("amin", np.min)):
                got, kernel = run(a, op, axes)
                assert kernel == expected_kernel(shape, axes, a.dtype)
                ct.assert_same_bits(got, fn(a, axis=rr.mask_axes(axes), keepdims=True), "%s %s mask %d %s [%s]" % (op, shape, axes, dt, kernel))


# ---- 2. tolerance against torch float64 -----------------------------------------------------------------------------------------------------
def check(x, op, axes, what=""):
    dt = "f32" if x.dtype == np.float32 else "f16"
    got, kernel = run(x, op, axes)
    form = rr.expected_form(x.shape, axes)
    SEEN.add(kernel)
    what = "%s %s %s mask %d %s [%s]" % (what, op, x.shape, axes, dt, kernel)
    assert got.dtype == x.dtype and got.shape == rr.out_shape(x.shape, axes) and kernel == expected_kernel(x.shape, axes, x.dtype), what
    ref = rr.reduce_f64_torch(x, op, axes)
    e, m = util.rel_err(got, ref), util.mixed_err(got, ref)
    print("%s: max-based %.3e, element-wise %.3e" % (what, e, m))
    util.assert_parity(got.astype(np.float64), ref, rel=BAR[dt], what=what)
    w = WORST.setdefault((form, dt), [0.0, 0.0])
    w[0], w[1] = max(w[0], e), max(w[1], m)
    return got


@pytest.mark.parametrize("group", sorted(CASE_GROUPS))
def test_within_the_bar_of_torch_float64(gpu, group):
    for shape, axes in CASE_GROUPS[group]:
        for dt in sorted(DTYPES):
            for op in rr.OPS:
                check(data(shape, dt), op, axes)


# one (shape, mask) per form and instantiation: a c of 6 or 21 is scalar in both dtypes, 8 and its multiples are vectors in both
FORM_CASES = [((9, 1, 1, 21), 8), ((9, 1, 1, 64), 8), ((9, 1, 1, G + 1), 8), ((9, 1, 1, G + 8), 8), ((2, 5, 6, 8), 6), ((2, 5, 6, 6), 6),
              ((2, 9, 8, 8), 6), ((2, 9, 8, 6), 6), ((3, 4, 30, 8), 5), ((2, 70, 3, 6), 2)]
FORM_IDS = ["%s_c%d_mask%d" % (rr.expected_form(s, a), s[3], a) for s, a in FORM_CASES]
ALL_KERNELS = {rr.kname(f, d, v) for f in rr.FORMS for d in DTYPES.values() for v in (True, False)}


def test_form_cases_cover_every_kernel():
    assert {expected_kernel(s, a, d) for s, a in FORM_CASES for d in DTYPES.values()} == ALL_KERNELS


def test_every_kernel_ran_and_the_worst_errors(gpu):
    """(runs after the parametrised tests above, whose names it collects)"""
    if not ALL_KERNELS <= SEEN:
        for shape, axes in FORM_CASES:
            for dt in sorted(DTYPES):
                check(data(shape, dt), "mean", axes)
    assert ALL_KERNELS <= SEEN, sorted(ALL_KERNELS - SEEN)
    for (form, dt), (e, m) in sorted(WORST.items()):
        print("%s %s vs torch float64: max-based %.3e, element-wise %.3e" % (form, dt, e, m))


# ---- 3. special values -----------------------------------------------------------------------------------------------------------------------
def rows_view(shape, axes):
    """(to_rows, from_rows): an NHWC array as [reduced sets, positions in increasing (n, h, w, c) order] and back"""
    red = rr.mask_axes(axes)
    kept = tuple(a for a in range(4) if a not in red)
    perm = kept + red
    tshape = tuple(shape[a] for a in perm)
    k = int(np.prod([shape[a] for a in kept]))
    to_rows = lambda x: np.ascontiguousarray(np.transpose(np.asarray(x), perm)).reshape(k, -1)
    from_rows = lambda r: np.ascontiguousarray(np.transpose(r.reshape(tshape), np.argsort(perm)))
    return to_rows, from_rows


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("shape,axes", FORM_CASES, ids=FORM_IDS)
def test_special_values(gpu, shape, axes, dt):
    """rows 1, 3, 5, 6 of the first eight reduced sets: a NaN; one +inf; +inf and -inf; only -inf.  The special value sits once in the
    first, the middle and the last reduced position (the second infinity of row 5 at the other end or next to it).  Rows 0, 2, 4, 7 and all
    the others keep the bits of the launch in which the four rows are plain."""
    to_rows, from_rows = rows_view(shape, axes)
    plain = np.array(data(shape, dt))
    base = to_rows(plain)
    k, r = base.shape
    assert k >= 8
    out_rows = lambda y: np.asarray(y).reshape(-1) if axes == 8 else to_rows(np.broadcast_to(y, rr.out_shape(shape, axes))).reshape(k)
    plain_out = {op: run(plain, op, axes)[0] for op in rr.OPS}
    for at in sorted({0, r // 2, r - 1}):
        rows = base.copy()
        other = (at + 1) % r if r > 1 else at
        rows[1, at] = np.nan
        rows[3, at] = np.inf
        rows[5, at] = np.inf
        if r > 1:
            rows[5, r - 1 - at if r - 1 - at != at else other] = -np.inf
        rows[6, :] = -np.inf
        x = from_rows(rows)
        for op in rr.OPS:
            got, kernel = run(x, op, axes)
            assert kernel == expected_kernel(shape, axes, x.dtype), kernel
            g = out_rows(got).astype(np.float64)
            what = "%s %s mask %d %s, special value at position %d of %d" % (op, shape, axes, dt, at, r)
            assert np.isnan(g[1]), what + ": a NaN gives NaN"
            assert g[3] == np.inf if op != "amin" else np.isfinite(g[3]), what + ": one +inf"
            if r > 1:
                assert np.isnan(g[5]) if op in ("sum", "mean") else g[5] == (np.inf if op == "amax" else -np.inf), what + ": +inf and -inf"
            assert g[6] == -np.inf, what + ": only -inf"
            keep = [0, 2, 4, 7] + list(range(8, k))
            assert np.isfinite(g[keep]).all(), what
            ct.assert_same_bits(np.ascontiguousarray(out_rows(got)[keep]), np.ascontiguousarray(out_rows(plain_out[op])[keep]), what + ": neighbouring rows")
            ref = rr.reduce_f64_torch(x, op, axes)
            assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.isinf(got), np.isinf(ref.astype(x.dtype))), what + ": torch's masks"


# ---- 4. determinism and batch invariance -----------------------------------------------------------------------------------------------------
BATCH_CASES = [((3, 5, 7, 8), m) for m in (8, 2, 4, 6)] + [((3, 5, 7, 6), m) for m in (8, 2, 4, 6)]
BATCH_CASES += [((3, 5, 5, 8), 6), ((3, 8, 8, 8), 6), ((3, 9, 8, 6), 6), ((3, 70, 3, 8), 2), ((3, 1, 1, G + 8), 8), ((3, 1, 1, G + 1), 8)]


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("shape,axes", BATCH_CASES, ids=["%s_mask%d" % ("x".join(map(str, s)), a) for s, a in BATCH_CASES])
def test_same_bits_twice_and_per_image(gpu, shape, axes, dt):
    """two launches give the same bits; for a mask without n, image 1 of a batch of 3 has the bits of that image run alone.  (3, 5, 5, 8)
    over h and w has 25 positions per image and 75 in the batch: the form would change if n counted."""
    x = data(shape, dt, seed=7)
    assert shape[0] == 3 and not axes & 1
    for op in rr.OPS:
        y3, k3 = run(x, op, axes)
        ct.assert_same_bits(y3, run(x, op, axes)[0], "two launches")
        y1, k1 = run(x[1:2], op, axes)
        assert k1 == k3 == expected_kernel(shape, axes, x.dtype), (k1, k3)
        ct.assert_same_bits(y3[1:2], y1, "%s: image 1 of 3" % op)
    if axes != 8:   # with n reduced two launches still agree
        ct.assert_same_bits(run(x, "mean", axes | 1)[0], run(x, "mean", axes | 1)[0], "two launches, n reduced")


# ---- 5. views and containment: checks (a) - (d) of tests/test_gpu_containment.py --------------------------------------------------------------
class ViewCase:
    def __init__(self, vid, half, shape, axes, op, form, vec, **views):
        self.id, self.half, self.shape, self.axes, self.op, self.form, self.vec, self.views = vid, half, shape, axes, op, form, vec, views
        self.entries = ("si_hip_reduce_f16" if half else "si_hip_reduce_f32",)
        self.dt = "f16" if half else "f32"
        self.dtype = DTYPES[self.dt]
        self.oc = 1 if axes & 8 else shape[3]

    def input(self):
        return data(self.shape, self.dt)

    def run(self, F):
        y, _ = run(self.input(), self.op, self.axes, in_fill=F, out_fill=F, full=True, **self.views)
        return ct.Out("y", y, self.views.get("out_c_off", 0), self.oc)


VIEW_CASES = []
for _half, _sfx, _v in ((False, "f32", 4), (True, "f16", 8)):
    VIEW_CASES += [
        # an input embedded at a channel offset of a wider buffer, an output slice of a wider buffer; 16-byte aligned on both sides
        ViewCase("row_group_vector_" + _sfx, _half, (2, 5, 7, 8), 8, "mean", "row_group", True, in_ld=24, in_c_off=8, out_ld=3, out_c_off=1),
        ViewCase("row_block_vector_" + _sfx, _half, (3, 1, 1, G + 8), 8, "amax", "row_block", True, in_ld=G + 24, in_c_off=8, out_ld=5, out_c_off=4),
        ViewCase("col_lane_vector_hw_" + _sfx, _half, (2, 5, 6, 8), 6, "mean", "col_lane", True, in_ld=24, in_c_off=8, out_ld=32, out_c_off=16),
        ViewCase("col_lane_vector_n_" + _sfx, _half, (2, 5, 7, 8), 1, "sum", "col_lane", True, in_ld=16, in_c_off=8, out_ld=24, out_c_off=8),
        ViewCase("col_coop_vector_hw_" + _sfx, _half, (2, 9, 8, 8), 6, "mean", "col_coop", True, in_ld=24, in_c_off=16, out_ld=16, out_c_off=8),
        ViewCase("col_coop_vector_nw_" + _sfx, _half, (3, 4, 30, 8), 5, "amin", "col_coop", True, in_ld=16, in_c_off=0, out_ld=24, out_c_off=16),
        # odd offsets and strides
        ViewCase("row_group_scalar_" + _sfx, _half, (2, 5, 7, 6), 8, "sum", "row_group", False, in_ld=9, in_c_off=2, out_ld=2, out_c_off=1),
        ViewCase("row_block_scalar_" + _sfx, _half, (3, 1, 1, G + 1), 8, "mean", "row_block", False, in_ld=G + 4, in_c_off=3, out_ld=3, out_c_off=0),
        ViewCase("col_lane_scalar_h_" + _sfx, _half, (2, 5, 7, 6), 2, "amax", "col_lane", False, in_ld=9, in_c_off=2, out_ld=7, out_c_off=1),
        ViewCase("col_lane_scalar_w_" + _sfx, _half, (2, 5, 7, 6), 4, "mean", "col_lane", False, in_ld=8, in_c_off=1, out_ld=7, out_c_off=1),
        ViewCase("col_coop_scalar_hw_" + _sfx, _half, (2, 9, 8, 6), 6, "sum", "col_coop", False, in_ld=11, in_c_off=5, out_ld=9, out_c_off=0),
        ViewCase("col_coop_scalar_h_" + _sfx, _half, (2, 70, 3, 6), 2, "mean", "col_coop", False, in_ld=7, in_c_off=1, out_ld=8, out_c_off=2),
        # vector-sized channels and strides behind a pointer that is 8 bytes off a 16-byte boundary: the scalar instantiation
        ViewCase("row_group_unaligned_" + _sfx, _half, (2, 5, 7, 8), 8, "amin", "row_group", False, in_ld=16, in_c_off=_v // 2, out_ld=1, out_c_off=0),
        ViewCase("col_lane_unaligned_out_" + _sfx, _half, (2, 5, 6, 8), 6, "mean", "col_lane", False, in_ld=16, in_c_off=0, out_ld=24, out_c_off=_v // 2),
        ViewCase("col_coop_unaligned_in_" + _sfx, _half, (2, 9, 8, 8), 6, "amax", "col_coop", False, in_ld=16, in_c_off=_v // 2, out_ld=16, out_c_off=8),
        # the input slice ends where its buffer ends
        ViewCase("row_group_last_slice_" + _sfx, _half, (2, 5, 7, 6), 8, "mean", "row_group", False, in_ld=14, in_c_off=8, out_ld=1, out_c_off=0),
        ViewCase("col_lane_last_slice_" + _sfx, _half, (2, 5, 6, 6), 6, "mean", "col_lane", False, in_ld=14, in_c_off=8, out_ld=6, out_c_off=0),
    ]


def test_view_cases_cover_what_the_issue_lists():
    assert {c.half for c in VIEW_CASES} == {False, True}
    assert {(c.form, c.vec, c.half) for c in VIEW_CASES} == {(f, v, h) for f in rr.FORMS for v in (True, False) for h in (True, False)}
    assert {c.op for c in VIEW_CASES} == set(rr.OPS)
    for c in VIEW_CASES:
        assert rr.expected_form(c.shape, c.axes) == c.form and rr.vectorised(c.shape, c.axes, c.dtype, **c.views) == c.vec, c.id
        assert c.views["in_ld"] > c.shape[3] and (c.views["out_ld"] > c.oc or "last_slice" in c.id or "unaligned" in c.id), c.id
    assert any(c.shape[3] % (16 // np.dtype(c.dtype).itemsize) == 0 and not c.vec for c in VIEW_CASES)   # the misaligned base pointer


@pytest.mark.parametrize("case", VIEW_CASES, ids=[c.id for c in VIEW_CASES])
def test_views_and_containment(gpu, case):
    del hipops.LAST_ENTRIES[:]
    plain = case.run(hipops.ByteFill(0x00))
    plain_kernel = hipops.LAST_KERNEL_NAME["si_hip_reduce"]
    assert set(case.entries) <= set(hipops.LAST_ENTRIES), hipops.LAST_ENTRIES
    assert plain_kernel == rr.kname(case.form, case.dtype, case.vec), plain_kernel
    ct.assert_outside_fill(plain.full, plain.c_off, plain.c, 0x00, case.id + ", plain run")
    # the value too: nothing of the gaps between the input's pixels (NaN under 0xFF, the largest value under 0x7B) reached the output
    dense, dense_kernel = run(case.input(), case.op, case.axes)
    if dense_kernel == plain_kernel:
        ct.assert_same_bits(np.ascontiguousarray(plain.dest), dense, case.id + " vs the dense run")
    util.assert_parity(np.ascontiguousarray(plain.dest).astype(np.float64), rr.reduce_f64_torch(case.input(), case.op, case.axes), rel=BAR[case.dt],
                       what=case.id)
    for byte in ct.PATTERNS:
        with hipops.guard_bands(byte) as g:      # (a) all bands and (d) the input are compared when the block ends
            out = case.run(hipops.ByteFill(byte))
        what = "%s under 0x%02X" % (case.id, byte)
        assert g.checked == 2, "%s: the guard saw %d buffers" % (what, g.checked)   # x, y
        assert hipops.LAST_KERNEL_NAME["si_hip_reduce"] == plain_kernel, what
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


def one_op_graph(typ, shape_file, dim, keepdim):
    """input -> one reduction -> output, for the file's (NCHW or [N, F]) shape"""
    b = mg.PnnxBuilder(seed=5)
    b.output(getattr(b, typ.split(".")[1])(b.input(shape_file), dim, keepdim))
    return b


def reduce_layers(prof):
    return [L for L in prof if L["type"] in rr.REDUCE_TYPES]


def nhwc_of(shape_file):
    return (shape_file[0], shape_file[2], shape_file[3], shape_file[1]) if len(shape_file) == 4 else tuple(shape_file)


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_leave_the_process_usable(gpu, tmp_path):
    x = np.array(data((2, 5, 7, 8), "f32"))
    H = _native.hip()
    fill = np.full(x.shape, 7.25, np.float32)
    src, dst = hipops.DeviceBuffer.from_numpy(x), hipops.DeviceBuffer.from_numpy(fill, out=True)

    def entry(d, fn="si_hip_reduce_f32", a=None, b=None):
        return getattr(H, fn)(C.byref(d), src.ptr if a is None else a, dst.ptr if b is None else b, None)

    desc = hipops.reduce_desc
    bad_axes = desc(x.shape, "sum", 8)
    bad_axes.axes = 16
    bad_op = desc(x.shape, "sum", 8)
    bad_op.op = 4
    codes = [entry(bad_axes), entry(bad_op), entry(desc(x.shape, "mean", 8, in_ld=7)), entry(desc(x.shape, "mean", 6, out_ld=7)),
             entry(desc((2, 0, 7, 8), "mean", 6)), entry(desc(x.shape, "amax", 6), a=C.c_void_p(None)), entry(desc(x.shape, "amax", 6), b=C.c_void_p(None)),
             entry(desc(x.shape, "amax", 6), fn="si_hip_reduce_f16", a=C.c_void_p(None)), entry(desc(x.shape, "amax", 6), b=src.ptr),
             entry(desc(x.shape, "amin", 8), b=src.ptr + 20)]
    assert codes == [-1] * len(codes), codes
    codes = [entry(desc(x.shape, "sum", m)) for m in (9, 10, 12, 15)] + [entry(desc((1, 16384, 16384, 8), "sum", 8))]
    assert codes == [-2] * len(codes), codes
    ct.assert_same_bits(dst.to_numpy(x.shape, np.float32), fill, "the output buffer keeps its fill")
    with pytest.raises(hipops.HipError):
        hipops.reduce(x, "sum", 9)
    with pytest.raises(hipops.HipError):
        hipops.reduce(x.astype(np.float16), 5, 8)

    def load(b, tag):
        pp, bp = save(b, tmp_path, tag)
        with pytest.raises(StatusError) as ei:
            Engine().load_model(pp, bp)
        return ei.value.status

    # refused at LoadModel, with the reason in the log, not at the first Forward
    assert load(one_op_graph("torch.mean", (2, 6, 5, 7), 1, False), "keepdim_false_dim1") == Status.kUnsupport
    assert load(one_op_graph("torch.amax", (2, 6, 5, 7), (2,), False), "keepdim_false_dim2") == Status.kUnsupport
    assert load(one_op_graph("torch.sum", (3, 10), 1, False), "keepdim_false_rank2") == Status.kUnsupport
    assert load(one_op_graph("torch.sum", (2, 6, 5, 7), (1, 2), True), "mixed_mask") == Status.kUnsupport
    assert load(one_op_graph("torch.mean", (2, 6, 5, 7), (1, 2, 3), True), "mixed_mask_all") == Status.kUnsupport
    assert load(one_op_graph("torch.mean", (2, 6, 5), 1, True), "rank3") == Status.kUnsupport
    assert load(one_op_graph("torch.amin", (2, 6, 5, 7), 4, True), "dim4") == Status.kUnsupport
    b = one_op_graph("torch.mean", (2, 6, 5, 7), (2, 3), True)
    b.lines = [ln.replace(" dtype=None ", " dtype=torch.float ") for ln in b.lines]
    assert "dtype=torch.float" in b.lines[1] and load(b, "dtype") == Status.kUnsupport
    b = one_op_graph("torch.mean", (2, 6, 5, 7), (2, 3), True)
    b.lines = [ln.replace(" dim=(2,3) ", " ") for ln in b.lines]
    assert " dim=" not in b.lines[1] and load(b, "no_dim") == Status.kUnsupport                  # the reduction to a scalar
    b = one_op_graph("torch.mean", (2, 6, 5, 7), (2, 3), True)
    b.lines = [ln.replace("(2,6,1,1)f32", "(2,6,1,5)f32") for ln in b.lines]
    assert "(2,6,1,5)f32" in b.lines[1] and load(b, "wrong_shape") == Status.kErrorShape        # the file's output shape is not the rule's
    b = one_op_graph("torch.mean", (2, 6, 5, 7), (2, 3), True)
    b.lines = [ln.replace(" dim=(2,3) ", " dim=(2,-2) ") for ln in b.lines]
    assert load(b, "repeated_dim") == Status.kFail
    b = one_op_graph("torch.mean", (2, 6, 5, 7), 1, True)
    b.lines = [ln.replace(" dim=1 ", " dim=1.5 ") for ln in b.lines]
    assert "dim=1.5" in b.lines[1] and load(b, "float_dim") == Status.kFail
    # ... and the same process launches, loads and runs afterwards
    util.assert_parity(run(x, "mean", 6)[0], rr.reduce_f64_torch(x, "mean", 6), what="good launch after the refusals")
    pp, bp = save(one_op_graph("torch.mean", (2, 8, 5, 7), (2, 3), True), tmp_path, "good")
    _, out = run_engine(pp, bp, x)
    ct.assert_same_bits(out, hipops.reduce(x, "mean", 6), "good model after the refusals")


# ---- 7. engine ---------------------------------------------------------------------------------------------------------------------------
ONE_OP = [(typ, (2, 6, 5, 7), dim, True) for typ in rr.REDUCE_TYPES for dim in (1, (1,), (2, 3), (-1, -2))]
ONE_OP += [(rr.REDUCE_TYPES[i % 4], (2, 6, 5, 7), dim, True) for i, dim in enumerate((2, 3, -1, 0, -3, (0, 2, 3), (0, 3), (3, 2), (0,)))]
ONE_OP += [(typ, (2, 8, 5, 7), (2, 3), False) for typ in rr.REDUCE_TYPES] + [("torch.mean", (2, 8, 9, 8), (-1, -2), False)]
ONE_OP += [(typ, (3, 10), 1, True) for typ in rr.REDUCE_TYPES] + [("torch.sum", (3, 10), -1, True), ("torch.amin", (3, 10), 0, True), ("torch.mean", (3, 10), (-2,), True)]
ONE_OP += [("torch.mean", (3, G + 8), 1, True), ("torch.amax", (2, 8, 9, 8), (2, 3), True)]


def _one_op_id(t, s, d, k):
    return "%s_%s_dim%s_%s" % (t, "x".join(map(str, s)), "_".join(map(str, d)) if isinstance(d, tuple) else d, "keep" if k else "drop")


@pytest.mark.parametrize("typ,shape_file,dim,keepdim", ONE_OP, ids=[_one_op_id(*c) for c in ONE_OP])
def test_engine_one_op_graph(gpu, tmp_path, typ, shape_file, dim, keepdim):
    """LoadModel -> Forward -> Extract reproduces the op-level result bit for bit and the torch float64 evaluation of the file"""
    b = one_op_graph(typ, shape_file, dim, keepdim)
    assert _parse(b.lines[1])[0] == typ
    pp, bp = save(b, tmp_path)
    rank = len(shape_file)
    x = util.rng_uniform(9, nhwc_of(shape_file), -1.0, 3.0)
    e, got = run_engine(pp, bp, x)
    axes = rr.nhwc_mask(dim, rank)
    x4 = x if rank == 4 else x.reshape(x.shape[0], 1, 1, x.shape[1])
    op_level, kernel = run(x4, typ.split(".")[1], axes)
    ct.assert_same_bits(got, op_level.reshape(got.shape), "engine vs op level")
    ref = rr.eval_graph(b, x)
    assert got.shape == ref.shape == nhwc_of(b.shapes[_parse(b.lines[-1])[2][0]]), (got.shape, ref.shape)
    util.assert_parity(got, ref, what="%s %s dim %s" % (typ, shape_file, dim))
    layers = reduce_layers(e.profile())
    assert len(layers) == 1 and layers[0]["type"] == typ, layers
    assert layers[0]["kernel"] == kernel == expected_kernel(x4.shape, axes, np.float32), (layers, kernel)


def test_reductions_read_a_concat_slice_and_write_into_a_concat(gpu, tmp_path):
    """a and q are written into their concat buffer in place: the mean and the amax over (2, 3) of q read channels 8 .. 15 of 16 at a pixel
    stride of 16, and write channels 0 .. 7 and 8 .. 15 of the [N, 16, 1, 1] concat the squeeze-excite conv reads"""
    b = mg.PnnxBuilder(seed=7)
    x = b.input((2, 4, 9, 11))
    f = b.relu(b.conv(x, 16, 3, 1, 1))
    a, q = b.relu(b.conv(f, 8, 1, 1, 0)), b.relu(b.conv(f, 8, 3, 1, 1))
    y = b.conv(b.cat([a, q]), 8, 1, 1, 0)
    p1, p2 = b.mean(q, (2, 3), True), b.amax(q, (2, 3), True)
    b.output(b.conv(b.mul(y, b.sigmoid(b.conv(b.cat([p1, p2]), 8, 1))), 4, 1))
    pp, bp = save(b, tmp_path)
    xin = util.rng_uniform(15, (2, 9, 11, 4), -1.0, 1.0)
    e, got = run_engine(pp, bp, xin)
    util.assert_parity(got, rr.eval_graph(b, xin), what="reduce <-> cat")
    alias = e.schedule()["alias"]
    assert all(any(o in ln.split() for ln in alias) for o in (a, q, p1, p2)), e.schedule()
    assert [L["kernel"] for L in reduce_layers(e.profile())] == [rr.kname("col_coop", np.float32, True)] * 2
    _, g = run_engine(pp, bp, xin, graph=1)
    util.assert_exact(g.view(np.uint32), got.view(np.uint32), "graph=1 vs eager")


TOYS = {
    # builder, NHWC input, the fp32 kernels of the reduction layers in file order
    "timm_head": (mg.build_toy_timm_head, (2, 32, 32, 3), ["col_coop<float, 4>"]),
    "cbam": (mg.build_toy_cbam, (2, 16, 16, 3), ["col_coop<float, 4>", "col_coop<float, 4>", "row_group<float, 4>", "row_group<float, 4>"]),
    "coordatt": (mg.build_toy_coordatt, (2, 12, 20, 3), ["col_lane<float, 4>", "col_lane<float, 4>"]),
    "layernorm2d": (mg.build_toy_layernorm2d, (2, 16, 16, 3), ["row_group<float, 4>", "row_group<float, 4>"]),
}


def toy_kernels(toy, half=False):
    names = []
    for k in TOYS[toy][2]:
        form, inst = k.split("<")
        names.append("reduce_%s_kernel<%s" % (form, inst if not half else "_Float16, 8>"))
    return names


@pytest.mark.parametrize("toy", sorted(TOYS))
def test_toy_model_fp32(gpu, tmp_path, toy):
    build, s, _ = TOYS[toy]
    b = build()
    pp, bp = save(b, tmp_path)
    x = mg.synth_input(s)
    e, got = run_engine(pp, bp, x)
    ref = rr.eval_graph(b, x)
    print("toy %s fp32: max-based %.3e, element-wise %.3e" % (toy, util.rel_err(got, ref), util.mixed_err(got, ref)))
    util.assert_parity(got, ref, what="toy %s fp32" % toy)
    assert [L["kernel"] for L in reduce_layers(e.profile())] == toy_kernels(toy), reduce_layers(e.profile())
    # the schedule runs every reduction as a step of its own (none is fused away), and the profile names their reduce_* kernels
    ran = e.schedule()["run"]
    assert all(any(L["name"] in r.split() for r in ran) for L in reduce_layers(e.profile())), ran
    assert all(L["kernel"].startswith("reduce_") for L in reduce_layers(e.profile()))
    if toy == "timm_head":   # mean((2, 3)) hands its [N, C] to nn.Linear: no flatten, no copy, no cast in between
        types = [L["type"] for L in e.profile()]
        at = types.index("torch.mean")
        assert types[at + 1] == "nn.Linear" and len(types) == at + 2, types
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
    """fp16=1: every reduction runs its half kernel with no cast pair around it, and the result is within F16_TOL of the fp16-storage
    emulation: fp64 arithmetic, with the weights, the input and every operator's output -- those an expression lowers to included --
    rounded to fp16; the file's last layer (a conv or a linear) writes the fp32 graph output from its own epilogue."""
    build, s, _ = TOYS[toy]
    b = build()
    pp, bp = save(b, tmp_path)
    x = mg.synth_input(s)
    e, got = run_engine(pp, bp, x, fp16=1)
    prof = e.profile()
    layers = reduce_layers(prof)
    assert [L["kernel"] for L in layers] == toy_kernels(toy, half=True), layers
    names = [L["name"] for L in prof]
    for L in layers:   # (InsertFp32Fallbacks names its casts <layer>.in_to_f32.<k> / <layer>.out_to_f16.<k>)
        assert not any(n.startswith(L["name"] + ".in_to_f32") or n.startswith(L["name"] + ".out_to_f16") for n in names), names
    ref = rr.eval_graph(b, x)
    emu = rr.eval_graph(b, x, rnd=rr.round_f16)
    print("toy %s fp16 storage: vs the fp16 emulation max-based %.3e; vs fp64: engine %.3e, emulation %.3e" % (
        toy, util.rel_err(got, emu), util.rel_err(got, ref), util.rel_err(emu, ref)))
    assert np.isfinite(got).all()
    util.assert_parity(got, emu, rel=F16_TOL, what="toy %s fp16 storage vs the emulation" % toy)
