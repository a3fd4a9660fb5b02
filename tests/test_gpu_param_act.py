"""GPU: clamp / softplus / mish -- si_hip_param_act_f32 / _f16 (include/si_act.h) and the ParamActivation layer.  fp32 per op through the
three arms on special values, the band where an exponential overflows and a wide sweep (clamp bit for bit, softplus and mish within 4 ulp);
fp16 on every one of the 65536 bit patterns in the vector and the scalar arm; grid-stride launches of more than two passes with a
sentinel in the destination's gaps; strided views under guard bands; determinism; the refusals; and the layer inside the engine: one-op
graphs for the nine type strings, conv -> ReLU6 -> conv as three steps, a param_act between a chunk view and a concat, the functional
spellings of the existing activations against their nn.* twins, and the toy MobileNetV2 / CSP-Mish / clamp head in fp32, under graph
capture, re-batched and with fp16 storage.  Every engine test fails without the layer (LoadModel rejects the types), every op-level test
without the kernels (the symbols are missing).

Every check prints its figures before it asserts (run with -s)."""
import ctypes as C
import functools

import numpy as np
import pytest

import act_reference as ar
import containment as ct
import elementwise_reference as er
import util
from ct_reference import _parse
from simpleinfer_amd import _native, hipops, modelgen as mg
from simpleinfer_amd.engine import Engine, Status, StatusError
from test_gpu_f16 import F16_TOL

pytestmark = pytest.mark.gpu

INF = ar.INF
F64 = np.float64
SENTINEL = 0x7B            # 1.3e36 as fp32, 61280 as fp16
DTYPES = {"f32": np.float32, "f16": np.float16}
OP_PARAMS = {"clamp": ar.CLAMP_BOUNDS, "softplus": ar.SOFTPLUS_PARAMS, "mish": [(0.0, 0.0)]}
WORST = {}                 # (op, dtype) -> worst fp32 ulp, or (inputs that differ, worst fp16 ulp)


def record(line):
    print("param_act: " + line)


def run(x, op, p0=0.0, p1=0.0, **views):
    y = hipops.param_act(x, op, p0, p1, **views)
    return y, hipops.LAST_KERNEL_NAME["si_hip_param_act"]


@functools.lru_cache(maxsize=None)
def fp32_inputs():
    x = ar.fp32_inputs()
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def reference(op, p0, p1, which="f32"):
    """float64 reference of the shared inputs, computed once"""
    x = fp32_inputs() if which == "f32" else er.all_halves()
    r = ar.param_act_ref(op, x.astype(F64), p0, p1)
    r.setflags(write=False)
    return r


# ---- 1. fp32, per op, through the three arms ---------------------------------------------------------------------------------------------
ARMS32 = [("dense", 8, {}, True), ("vector", 8, dict(in_ld=16, in_c_off=8, out_ld=16, out_c_off=4), True), ("scalar", 7, {}, False)]


def through_the_arms(op, p0, p1):
    x = fp32_inputs()
    outs = []
    for arm, c, views, vec in ARMS32:
        t, n = er.as_rows(x, c, odd_pixels=True)
        y, kernel = run(t, op, p0, p1, **views)
        assert kernel == ar.kname(op, np.float32, vec), (arm, kernel)
        assert ar.vectorised(t.shape, np.float32, **views) == vec
        outs.append(y.reshape(-1)[:n])
        er.assert_arms_agree(outs[0], outs[-1], "%s(%g, %g) arm %s" % (op, p0, p1, arm))
    return outs[0]


@pytest.mark.parametrize("lo,hi", ar.CLAMP_BOUNDS, ids=["%g_%g" % b for b in ar.CLAMP_BOUNDS])
def test_fp32_clamp_is_exact(gpu, lo, hi):
    """a selection: the bits of the float64 rule rounded to fp32 (it never rounds), signs of zero included; NaN passes through"""
    got = through_the_arms("clamp", lo, hi)
    er.assert_bits32(got, reference("clamp", lo, hi), "clamp(%g, %g)" % (lo, hi))
    x = fp32_inputs()
    assert np.isnan(got[np.isnan(x)]).all()
    if (lo, hi) == (0.0, 6.0):
        z = got[(x == 0) & np.signbit(x)]
        assert z.size and np.signbit(z).all(), "-0.0 against lo = 0 stays -0.0"
    if lo > hi:
        assert (got[~np.isnan(x)] == np.float32(hi)).all(), "lo > hi gives hi everywhere"
    record("fp32 clamp(%g, %g): bit-exact on %d values" % (lo, hi, x.size))


@pytest.mark.parametrize("op,p0,p1", [("softplus",) + p for p in ar.SOFTPLUS_PARAMS] + [("mish", 0.0, 0.0)],
                         ids=["softplus_%g_%g" % p for p in ar.SOFTPLUS_PARAMS] + ["mish"])
def test_fp32_softplus_and_mish_within_4_ulp(gpu, op, p0, p1):
    got = through_the_arms(op, p0, p1)
    ref = reference(op, p0, p1)
    e = er.ulp32(got, ref)
    x = fp32_inputs()
    record("fp32 %s(%g, %g): worst %.3f ulp at x = %r on %d values" % (op, p0, p1, float(e.max()), x[int(np.argmax(e))], x.size))
    worst, _ = er.assert_ulp32(got, ref, 4, "%s(%g, %g)" % (op, p0, p1), band=True)
    WORST[(op, "f32")] = max(WORST.get((op, "f32"), 0.0), worst)
    # special values
    at = lambda v: got[np.flatnonzero(x == np.float32(v))[0]]
    assert np.isnan(got[np.isnan(x)]).all()
    if op == "softplus":
        assert at(INF) == INF and at(-INF) == 0
    else:
        assert at(INF) == INF and np.isnan(at(-INF))
    # the negative tail is there: not flushed to zero where the value is about e^x
    z = x.astype(F64) * (p0 if op == "softplus" else 1.0)
    tail = (z < -20) & (z > -80)
    assert tail.any() and (got[tail] != 0).all()


# ---- 2. fp16, all 65536 bit patterns, vector and scalar arm ---------------------------------------------------------------------------------
def halves_through_the_arms(op, p0, p1):
    h = er.all_halves()
    outs = []
    for c, vec in ((8, True), (7, False)):
        t, n = er.as_rows(h, c, odd_pixels=True)
        y, kernel = run(t, op, p0, p1)
        assert y.dtype == np.float16 and kernel == ar.kname(op, np.float16, vec), kernel
        outs.append(y.reshape(-1)[:n])
    er.assert_arms_agree(outs[0], outs[1], "%s(%g, %g) fp16 vector vs scalar" % (op, p0, p1))
    return outs[0]


@pytest.mark.parametrize("lo,hi", ar.CLAMP_BOUNDS_F16, ids=["%g_%g" % b for b in ar.CLAMP_BOUNDS_F16])
def test_fp16_clamp_is_exact(gpu, lo, hi):
    assert float(np.float16(lo)) == lo and float(np.float16(hi)) == hi, "bounds a half can hold"
    got = halves_through_the_arms("clamp", lo, hi)
    want = er.round_to(reference("clamp", lo, hi, "f16"), np.float16)
    ok = er.same_bits_or_nan(got, want)
    assert ok.all(), "clamp(%g, %g) fp16: %d of 65536 differ, first at pattern %d" % (lo, hi, int((~ok).sum()), int(np.flatnonzero(~ok)[0]))
    record("fp16 clamp(%g, %g): equal bits on all 65536 patterns" % (lo, hi))


@pytest.mark.parametrize("op,p0,p1", [("softplus",) + p for p in ar.SOFTPLUS_PARAMS] + [("mish", 0.0, 0.0)],
                         ids=["softplus_%g_%g" % p for p in ar.SOFTPLUS_PARAMS] + ["mish"])
def test_fp16_softplus_and_mish_within_1_ulp(gpu, op, p0, p1):
    got = halves_through_the_arms(op, p0, p1)
    ref = reference(op, p0, p1, "f16")
    d = er.half_ulp(got, ref)
    record("fp16 %s(%g, %g): %d of 65536 inputs differ from the reference rounded once, worst %d fp16 ulp" % (op, p0, p1, int((d > 0).sum()), int(d.max())))
    n, worst = er.assert_half(got, ref, 1, "%s(%g, %g) fp16" % (op, p0, p1), max_share=er.H_MISMATCH_SHARE)
    w = WORST.get((op, "f16"), (0, 0))
    WORST[(op, "f16")] = (max(w[0], n), max(w[1], worst))


def test_worst_errors(gpu):
    """(runs after the parametrised tests above, whose figures it collects)"""
    for (op, dt), w in sorted(WORST.items()):
        record("worst over the cases, %s %s: %s" % (op, dt, "%.3f fp32 ulp" % w if dt == "f32" else "%d inputs differ, %d fp16 ulp" % w))


# ---- 3. grid-stride: more than two passes, a ragged last one, a gap that holds a sentinel ------------------------------------------------------
V4 = (1, 1031, 1019, 4)
S3 = (1, 593, 593, 3)
GRID32 = [("dense", V4, dict(out_ld=4, out_c_off=0), True), ("vector", V4, dict(out_ld=8, out_c_off=4), True),
          ("scalar", S3[:3] + (7,), dict(out_ld=8, out_c_off=1), False)]
GRID16 = [("vector", V4[:3] + (8,), dict(out_ld=16, out_c_off=8), True), ("scalar", S3[:3] + (7,), dict(out_ld=8, out_c_off=1), False)]


def test_grid_stride_shapes_make_three_passes():
    ok = lambda n: n >= 2 * er.GRID_CAP + 1 and n % 256 != 0
    assert ok(V4[1] * V4[2]) and ok(S3[1] * S3[2] * 7)


@functools.lru_cache(maxsize=None)
def grid_input(shape, dt):
    x = util.rng_uniform(330, shape, -12, 12).astype(DTYPES[dt])
    x.setflags(write=False)
    return x


@pytest.mark.parametrize("op,p0,p1", [("clamp", -1.0, 1.0), ("mish", 0.0, 0.0)], ids=["clamp", "mish"])
@pytest.mark.parametrize("dt,arm,shape,views,vec", [("f32",) + g for g in GRID32] + [("f16",) + g for g in GRID16],
                         ids=["f32_" + g[0] for g in GRID32] + ["f16_" + g[0] for g in GRID16])
def test_grid_stride(gpu, dt, arm, shape, views, vec, op, p0, p1):
    x = grid_input(shape, dt)
    full, kernel = run(x, op, p0, p1, out_fill=hipops.ByteFill(SENTINEL), full=True, **views)
    assert kernel == ar.kname(op, x.dtype, vec), kernel
    got = ct.checked_dest(full, views["out_c_off"], shape[3], SENTINEL, "destination rows")
    ref = ar.param_act_ref(op, x.astype(F64), p0, p1)
    what = "grid-stride %s %s %s" % (op, dt, arm)
    if op == "clamp":
        assert er.same_bits_or_nan(got, er.round_to(ref, x.dtype)).all(), what
    elif dt == "f32":
        er.assert_ulp32(got, ref, 4, what, band=True)
    else:
        er.assert_half(got, ref, 1, what, max_share=er.H_MISMATCH_SHARE)


# ---- 4. views and containment: checks (a) - (d) of tests/test_gpu_containment.py --------------------------------------------------------------
class ViewCase:
    def __init__(self, vid, half, shape, op, params, vec, **views):
        self.id, self.half, self.shape, self.op, self.params, self.vec, self.views = vid, half, shape, op, params, vec, views
        self.entries = ("si_hip_param_act_f16" if half else "si_hip_param_act_f32",)
        self.dt = "f16" if half else "f32"
        self.dtype = DTYPES[self.dt]

    def input(self):
        x = util.rng_uniform(41, self.shape, -8.0, 8.0).astype(self.dtype)
        return x

    def run(self, F):
        y, _ = run(self.input(), self.op, *self.params, in_fill=F, out_fill=F, full=True, **self.views)
        return ct.Out("y", y, self.views.get("out_c_off", 0), self.shape[3])


VIEW_CASES = []
for _half, _sfx, _v in ((False, "f32", 4), (True, "f16", 8)):
    VIEW_CASES += [
        # an input embedded at a channel offset of a wider buffer, an output slice of a wider buffer; 16-byte aligned on both sides
        ViewCase("clamp_vector_" + _sfx, _half, (2, 5, 7, 8), "clamp", (0.0, 6.0), True, in_ld=24, in_c_off=8, out_ld=32, out_c_off=16),
        ViewCase("softplus_vector_" + _sfx, _half, (2, 5, 7, 16), "softplus", (1.0, 20.0), True, in_ld=32, in_c_off=16, out_ld=24, out_c_off=8),
        ViewCase("mish_vector_" + _sfx, _half, (2, 5, 7, 8), "mish", (0.0, 0.0), True, in_ld=16, in_c_off=8, out_ld=16, out_c_off=0),
        # odd offsets and strides
        ViewCase("clamp_scalar_" + _sfx, _half, (2, 5, 7, 6), "clamp", (-1.0, 1.0), False, in_ld=9, in_c_off=2, out_ld=11, out_c_off=5),
        ViewCase("softplus_scalar_" + _sfx, _half, (2, 5, 7, 7), "softplus", (2.0, 5.0), False, in_ld=8, in_c_off=1, out_ld=9, out_c_off=0),
        ViewCase("mish_scalar_" + _sfx, _half, (3, 1, 1, 21), "mish", (0.0, 0.0), False, in_ld=24, in_c_off=3, out_ld=22, out_c_off=1),
        # vector-sized channels and strides behind a pointer that is 8 bytes off a 16-byte boundary: the scalar instantiation
        ViewCase("clamp_unaligned_in_" + _sfx, _half, (2, 5, 7, 8), "clamp", (0.0, 6.0), False, in_ld=16, in_c_off=_v // 2, out_ld=16, out_c_off=8),
        ViewCase("mish_unaligned_out_" + _sfx, _half, (2, 5, 7, 8), "mish", (0.0, 0.0), False, in_ld=16, in_c_off=0, out_ld=24, out_c_off=_v // 2),
        # the input slice ends where its buffer ends; the destination is dense
        ViewCase("clamp_last_slice_" + _sfx, _half, (2, 5, 7, 6), "clamp", (-INF, 0.5), False, in_ld=14, in_c_off=8, out_ld=6, out_c_off=0),
        ViewCase("mish_last_slice_vector_" + _sfx, _half, (2, 5, 7, 8), "mish", (0.0, 0.0), True, in_ld=24, in_c_off=16, out_ld=8, out_c_off=0),
    ]


def test_view_cases_cover_every_instantiation():
    assert {(c.op, c.vec, c.half) for c in VIEW_CASES} == {(op, v, h) for op in ar.OPS for v in (True, False) for h in (True, False)}
    for c in VIEW_CASES:
        assert ar.vectorised(c.shape, c.dtype, **c.views) == c.vec, c.id
        assert c.views["in_ld"] > c.shape[3] and (c.views["out_ld"] > c.shape[3] or "last_slice" in c.id), c.id
    assert any(c.shape[3] % (16 // np.dtype(c.dtype).itemsize) == 0 and not c.vec for c in VIEW_CASES)   # the misaligned base pointer


def assert_at_the_bar(got, ref, op, dt, what):
    if op == "clamp":
        assert er.same_bits_or_nan(np.ascontiguousarray(got), er.round_to(ref, got.dtype)).all(), what
    elif dt == "f32":
        er.assert_ulp32(got, ref, 4, what, band=True)
    else:
        er.assert_half(got, ref, 1, what, max_share=None)


@pytest.mark.parametrize("case", VIEW_CASES, ids=[c.id for c in VIEW_CASES])
def test_views_and_containment(gpu, case):
    del hipops.LAST_ENTRIES[:]
    plain = case.run(hipops.ByteFill(0x00))
    plain_kernel = hipops.LAST_KERNEL_NAME["si_hip_param_act"]
    assert set(case.entries) <= set(hipops.LAST_ENTRIES), hipops.LAST_ENTRIES
    assert plain_kernel == ar.kname(case.op, case.dtype, case.vec), plain_kernel
    ct.assert_outside_fill(plain.full, plain.c_off, plain.c, 0x00, case.id + ", plain run")
    # the value too: nothing of the gaps between the input's pixels (NaN under 0xFF, a huge value under 0x7B) reached the output
    dense, _ = run(case.input(), case.op, *case.params)
    ct.assert_same_bits(np.ascontiguousarray(plain.dest), dense, case.id + " vs the dense run")
    assert_at_the_bar(np.ascontiguousarray(plain.dest), ar.param_act_ref(case.op, case.input().astype(F64), *case.params), case.op, case.dt, case.id)
    for byte in ct.PATTERNS:
        with hipops.guard_bands(byte) as g:      # (a) all bands and (d) the input are compared when the block ends
            out = case.run(hipops.ByteFill(byte))
        what = "%s under 0x%02X" % (case.id, byte)
        assert g.checked == 2, "%s: the guard saw %d buffers" % (what, g.checked)   # x, y
        assert hipops.LAST_KERNEL_NAME["si_hip_param_act"] == plain_kernel, what
        ct.assert_outside_fill(out.full, out.c_off, out.c, byte, what)                              # (b)
        ct.assert_same_bits(out.dest, plain.dest, what + ": guarded + pattern-filled vs plain")    # (c)


# ---- 5. determinism --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("c,views", [(8, {}), (8, dict(in_ld=16, in_c_off=8, out_ld=24, out_c_off=8)), (7, {}), (7, dict(in_ld=9, out_ld=8, out_c_off=1))],
                         ids=["dense", "vector", "scalar_dense", "scalar_rows"])
def test_same_bits_twice_and_per_row(gpu, c, views, dt):
    """two launches give the same bits; row 1 of a batch of 3 has the bits of that row run alone (the arm may differ: 35 x 7 elements fill
    no vector, 105 x 7 do not either, but 3 x 35 x 8 and 35 x 8 both do -- the arithmetic is the arm's in no case)"""
    x = util.rng_uniform(7, (3, 5, 7, c), -12.0, 12.0).astype(DTYPES[dt])
    for op, params in OP_PARAMS.items():
        p0, p1 = params[0]
        y3, _ = run(x, op, p0, p1, **views)
        ct.assert_same_bits(y3, run(x, op, p0, p1, **views)[0], "%s: two launches" % op)
        y1, _ = run(x[1:2], op, p0, p1, **views)
        ct.assert_same_bits(y3[1:2], y1, "%s: row 1 of 3" % op)


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


def nhwc_of(shape_file):
    return (shape_file[0], shape_file[2], shape_file[3], shape_file[1]) if len(shape_file) == 4 else tuple(shape_file)


def act_layers(prof):
    return [L for L in prof if L["type"] in ar.PARAM_TYPES]


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_leave_the_process_usable(gpu, tmp_path):
    x = util.rng_uniform(3, (2, 5, 7, 8), -8.0, 8.0)
    H = _native.hip()
    fill = np.full(x.shape, 7.25, np.float32)
    src, dst = hipops.DeviceBuffer.from_numpy(x), hipops.DeviceBuffer.from_numpy(fill, out=True)

    def entry(d, fn="si_hip_param_act_f32", a=None, b=None):
        return getattr(H, fn)(C.byref(d), src.ptr if a is None else a, dst.ptr if b is None else b, None)

    desc = hipops.param_act_desc
    nan = float("nan")
    zero_px = desc(x.shape, "mish")
    zero_px.pixels = 0
    codes = [entry(desc(x.shape, 3)), entry(desc(x.shape, -1)), entry(desc(x.shape, "clamp", 0, 6, in_ld=7)), entry(desc(x.shape, "clamp", 0, 6, out_ld=7)),
             entry(zero_px), entry(desc(x.shape, "clamp", nan, 6)), entry(desc(x.shape, "clamp", 0, nan)), entry(desc(x.shape, "softplus", 0, 20)),
             entry(desc(x.shape, "softplus", INF, 20)), entry(desc(x.shape, "softplus", nan, 20)), entry(desc(x.shape, "softplus", 1, nan)),
             entry(desc(x.shape, "mish"), a=C.c_void_p(None)), entry(desc(x.shape, "mish"), b=C.c_void_p(None)),
             entry(desc(x.shape, "mish"), fn="si_hip_param_act_f16", a=C.c_void_p(None)), entry(desc(x.shape, "mish"), b=src.ptr),
             entry(desc(x.shape, "mish"), b=src.ptr + 20), entry(desc(x.shape, "mish", in_ld=16, out_ld=16), b=src.ptr + 16)]
    assert codes == [-1] * len(codes), codes
    codes = [entry(desc((1 << 28, 8), "mish")), entry(desc((1 << 20, 8), "clamp", 0, 6, out_ld=1 << 11))]
    assert codes == [-2] * len(codes), codes
    ct.assert_same_bits(dst.to_numpy(x.shape, np.float32), fill, "the output buffer keeps its fill")
    with pytest.raises(hipops.HipError):
        hipops.param_act(x, 3)
    with pytest.raises(hipops.HipError):
        hipops.param_act(x.astype(np.float16), "softplus", 0.0, 20.0)

    def load(b, tag):
        pp, bp = save(b, tmp_path, tag)
        with pytest.raises(StatusError) as ei:
            Engine().load_model(pp, bp)
        return ei.value.status

    # refused at LoadModel, with the reason in the log, not at the first Forward
    assert load(ar.one_op_graph("torch.clamp"), "clamp_none_none") == Status.kUnsupport
    b = ar.one_op_graph("torch.clamp", min=0.0)
    b.lines = [ln.replace(" max=None ", " ").replace(" min=0.000000e+00 ", " ") for ln in b.lines]
    assert " min=" not in b.lines[1] and " max=" not in b.lines[1] and load(b, "clamp_no_keys") == Status.kUnsupport
    assert load(ar.one_op_graph("nn.Hardtanh", min_val=2.0, max_val=-2.0), "hardtanh_min_above_max") == Status.kFail
    assert load(ar.one_op_graph("F.hardtanh", min_val=2.0, max_val=-2.0), "f_hardtanh_min_above_max") == Status.kFail
    assert load(ar.one_op_graph("nn.Softplus", beta=0.0), "softplus_beta_0") == Status.kFail
    b = ar.one_op_graph("nn.Hardtanh")
    b.lines = [ln.replace(" min_val=-1.000000e+00 ", " min_val=(1,2) ") for ln in b.lines]
    assert "min_val=(1,2)" in b.lines[1] and load(b, "mistyped") == Status.kFail
    b = ar.one_op_graph("nn.Mish")
    b.lines = [ln.replace("#1=(2,8,5,7)f32", "#1=(2,8,5,6)f32") for ln in b.lines]
    assert "(2,8,5,6)f32" in b.lines[1] and load(b, "wrong_shape") == Status.kErrorShape
    # ... and the same process launches, loads and runs afterwards
    er.assert_bits32(run(x, "clamp", 0.0, 6.0)[0], ar.param_act_ref("clamp", x, 0.0, 6.0), "good launch after the refusals")
    pp, bp = save(ar.one_op_graph("nn.ReLU6"), tmp_path, "good")
    _, out = run_engine(pp, bp, x)
    ct.assert_same_bits(out, hipops.param_act(x, "clamp", 0.0, 6.0), "good model after the refusals")


# ---- 7. engine ---------------------------------------------------------------------------------------------------------------------------
ONE_OP = [("nn.ReLU6", {}), ("F.relu6", {}), ("nn.Hardtanh", {}), ("nn.Hardtanh", dict(min_val=-2.0, max_val=0.5)), ("F.hardtanh", dict(min_val=0.0, max_val=3.0)),
          ("torch.clamp", dict(min=0.1)), ("torch.clamp", dict(max=3.0)), ("torch.clamp", dict(min=-0.5, max=0.25)), ("nn.Softplus", {}),
          ("nn.Softplus", dict(beta=2.0, threshold=5.0)), ("F.softplus", dict(beta=0.5)), ("nn.Mish", {}), ("F.mish", {})]


def _one_op_id(t, p):
    return t + "".join("_%s%g" % kv for kv in sorted(p.items()))


@pytest.mark.parametrize("shape_file", [(2, 8, 5, 7), (2, 7, 5, 3), (3, 10)], ids=["c8", "c7", "rank2"])
@pytest.mark.parametrize("typ,params", ONE_OP, ids=[_one_op_id(*c) for c in ONE_OP])
def test_engine_one_op_graph(gpu, tmp_path, typ, params, shape_file):
    """LoadModel -> Forward -> Extract reproduces the op-level result bit for bit and the float64 evaluation of the file (clamp: exactly)"""
    b = ar.one_op_graph(typ, shape_file, **params)
    line = _parse(b.lines[1])
    assert line[0] == typ
    pp, bp = save(b, tmp_path)
    x = util.rng_uniform(9, nhwc_of(shape_file), -8.0, 8.0)
    e, got = run_engine(pp, bp, x)
    op, p0, p1 = ar.act_of_line(typ, line[4])
    op_level, kernel = run(x, op, p0, p1)
    assert kernel == ar.kname(op, np.float32, ar.vectorised(x.shape, np.float32))
    ct.assert_same_bits(got, op_level.reshape(got.shape), "engine vs op level")
    ref = ar.eval_graph(b, x)
    assert got.shape == ref.shape == x.shape
    if op == "clamp":
        er.assert_bits32(got, ref, "%s %s" % (typ, params))
        assert (got != x).any() and (got == x).any()          # the bounds cut some values and pass others
    else:
        util.assert_parity(got, ref, what="%s %s" % (typ, params))
    layers = act_layers(e.profile())
    assert len(layers) == 1 and layers[0]["type"] == typ and layers[0]["kernel"] == "param_act", layers


def test_relu6_between_two_convs_is_a_step_of_its_own(gpu, tmp_path):
    """conv -> ReLU6 -> conv: the activation is neither folded into the first convolution's epilogue nor dropped"""
    def graph(with_act):
        b = mg.PnnxBuilder(seed=11)
        x = b.conv(b.input((2, 4, 9, 11)), 16, 3, 1, 1)
        b.output(b.conv(b.relu6(x) if with_act else x, 8, 1))
        return b

    xin = util.rng_uniform(15, (2, 9, 11, 4), -6.0, 6.0)
    b = graph(True)
    e, got = run_engine(*save(b, tmp_path, "with"), xin)
    prof = e.profile()
    assert [L["type"] for L in prof] == ["nn.Conv2d", "nn.ReLU6", "nn.Conv2d"], prof
    assert prof[1]["kernel"] == "param_act" and not prof[0]["kernel"].startswith("param_act")
    assert not e.schedule()["fused"], e.schedule()
    ref = ar.eval_graph(b, xin)
    mid = ar.eval_graph(_cut(b, 1), xin)
    assert (mid > 6).any() and (mid < 0).any(), "the convolution's output reaches both bounds"
    util.assert_parity(got, ref, what="conv -> ReLU6 -> conv")
    plain = graph(False)
    assert all(np.array_equal(plain.attrs[k], b.attrs[k]) for k in plain.attrs)
    _, without = run_engine(*save(plain, tmp_path, "without"), xin)
    assert util.rel_err(got, without) > 1e-2, "the output differs from the graph without the activation"
    # an ActivationLayer in the same place IS folded: the plan of the existing types is what it was
    r = mg.PnnxBuilder(seed=11)
    x = r.conv(r.input((2, 4, 9, 11)), 16, 3, 1, 1)
    r.output(r.conv(r.relu(x), 8, 1))
    e2, _ = run_engine(*save(r, tmp_path, "relu"), xin)
    assert len(e2.schedule()["fused"]) == 1 and not any(L["kernel"] == "param_act" for L in e2.profile()), e2.schedule()


def _cut(b, n_ops):
    """the builder's graph up to and including operator line n_ops, its output made the graph output"""
    c = mg.PnnxBuilder(seed=b.seed)
    c.attrs, c.shapes = b.attrs, b.shapes
    c.lines = b.lines[:n_ops + 1] + ["pnnx.Output out 1 0 %s" % _parse(b.lines[n_ops])[3][0]]
    return c


def test_param_act_reads_a_chunk_view_and_writes_into_a_concat(gpu, tmp_path):
    """a and q are channel views of the convolution's 16 channels (torch.chunk launches nothing); mish reads q at a pixel stride of 16 from
    channel 8, ReLU6 reads a; both write their 8 channels into the concat buffer the last convolution reads"""
    b = mg.PnnxBuilder(seed=7)
    x = b.input((2, 4, 9, 11))
    f = b.conv(x, 16, 3, 1, 1)
    a, q = b.chunk(f, 2, 1)
    m, r = b.mish(q), b.relu6(a)
    b.output(b.conv(b.cat([m, r]), 4, 1))
    pp, bp = save(b, tmp_path)
    xin = util.rng_uniform(15, (2, 9, 11, 4), -6.0, 6.0)
    e, got = run_engine(pp, bp, xin)
    util.assert_parity(got, ar.eval_graph(b, xin), what="chunk -> param_act -> cat")
    alias = e.schedule()["alias"]
    assert all(any(o in ln.split() for ln in alias) for o in (a, q, m, r)), e.schedule()
    layers = act_layers(e.profile())
    assert [L["type"] for L in layers] == ["nn.Mish", "nn.ReLU6"] and all(L["kernel"] == "param_act" for L in layers)
    _, g = run_engine(pp, bp, xin, graph=1)
    util.assert_exact(g.view(np.uint32), got.view(np.uint32), "graph=1 vs eager")
    _, h = run_engine(pp, bp, xin, fp16=1)
    util.assert_parity(h, ar.eval_graph(b, xin, rnd=ar.round_f16), rel=F16_TOL, what="chunk -> param_act -> cat, fp16 storage")


def classifier(functional, batch=2, size=32):
    """build_toy_classifier's graph with every activation the project had before this feature, in either spelling"""
    b = mg.PnnxBuilder(0)
    x = b.input((batch, 3, size, size))
    x = b.hardswish(b.batchnorm(b.conv(x, 16, 3, 2, 1, bias=False)), functional)
    y = b.relu(b.conv(x, 16, 3, 1, 1, groups=16), functional)
    se = b.adaptive_avgpool(y, (1, 1))
    se = b.silu(b.conv(se, 8, 1), functional)
    se = b.hardsigmoid(b.conv(se, 16, 1), functional)
    y = b.mul(y, se)
    y = b.leaky_relu(b.conv(y, 16, 1), 0.1, functional)
    x = b.add(x, y)
    x = b.tanh(b.conv(x, 24, 3, 2, 1, groups=2), functional)
    x = b.sigmoid(b.conv(x, 24, 1), functional)
    x = b.flatten(b.adaptive_avgpool(x, (1, 1)))
    b.output(b.linear(x, 10))
    return b


@pytest.mark.parametrize("fp16", [0, 1], ids=["fp32", "fp16_storage"])
def test_functional_spellings_fuse_as_their_module_twins(gpu, tmp_path, fp16):
    """F.relu, F.silu, F.sigmoid, F.hardsigmoid, F.hardswish, F.leaky_relu, F.tanh: the same steps, the same kernels and the same bits as the
    nn.* graph -- the six ActivationLayers fold into their convolutions, tanh runs the unary kernel"""
    mod, fun = classifier(False), classifier(True)
    types = [_parse(ln)[0] for ln in fun.lines]
    assert [t for t in types if t in ar.FUNCTIONAL_TWINS] == ["F.hardswish", "F.relu", "F.silu", "F.hardsigmoid", "F.leaky_relu", "F.tanh", "F.sigmoid"]
    assert [ar.FUNCTIONAL_TWINS.get(t, t) for t in types] == [_parse(ln)[0] for ln in mod.lines]
    x = mg.synth_input((2, 32, 32, 3))
    opts = dict(fp16=1) if fp16 else {}
    em, ym = run_engine(*save(mod, tmp_path, "mod"), x, **opts)
    ef, yf = run_engine(*save(fun, tmp_path, "fun"), x, **opts)
    util.assert_exact(yf.view(np.uint32), ym.view(np.uint32), "functional vs module spelling")
    pm, pf = em.profile(), ef.profile()
    assert [(ar.FUNCTIONAL_TWINS.get(L["type"], L["type"]), L["kernel"]) for L in pf] == [(L["type"], L["kernel"]) for L in pm], (pf, pm)
    sm, sf = em.schedule(), ef.schedule()
    assert len(sf["run"]) == len(sm["run"]) and len(sf["fused"]) == len(sm["fused"]) and len(sf["alias"]) == len(sm["alias"])
    assert len(sf["fused"]) >= 1, sf                               # activations behind a convolution are folded into it ...
    tanh = [L for L in pf if L["type"] == "F.tanh"]
    assert len(tanh) == 1 and tanh[0]["kernel"] in ("unary_kernel", "unary_h_kernel"), pf     # ... and tanh, as nn.Tanh, is a step of its own
    if not fp16:
        util.assert_parity(yf, ar.eval_graph(fun, x), what="functional classifier")


TOYS = {
    # builder, NHWC input, the param_act layers in file order
    "mobilenetv2": (mg.build_toy_mobilenetv2, (2, 32, 32, 3), ["nn.ReLU6"] * 7),
    "csp_mish": (mg.build_toy_csp_mish, (2, 16, 16, 3), ["nn.Mish"] * 7),
    "clamp_head": (mg.build_toy_clamp_head, (2, 16, 16, 3), ["nn.Softplus", "torch.clamp"]),
}


@pytest.mark.parametrize("toy", sorted(TOYS))
def test_toy_model_fp32(gpu, tmp_path, toy):
    build, s, acts = TOYS[toy]
    b = build()
    pp, bp = save(b, tmp_path)
    x = mg.synth_input(s)
    e, got = run_engine(pp, bp, x)
    ref = ar.eval_graph(b, x)
    print("toy %s fp32: max-based %.3e, element-wise %.3e" % (toy, util.rel_err(got, ref), util.mixed_err(got, ref)))
    util.assert_parity(got, ref, what="toy %s fp32" % toy)
    layers = act_layers(e.profile())
    assert [L["type"] for L in layers] == acts and all(L["kernel"] == "param_act" for L in layers), layers
    ran = e.schedule()["run"]
    assert all(any(L["name"] in r.split() for r in ran) for L in layers), ran      # every one is a step of its own
    if toy == "mobilenetv2":
        fb = mg.build_toy_mobilenetv2(functional=True)
        _, f = run_engine(*save(fb, tmp_path, "functional"), x)
        util.assert_exact(f.view(np.uint32), got.view(np.uint32), "F.relu6 vs nn.ReLU6")
    # a captured graph replays the same bits
    _, g = run_engine(pp, bp, x, graph=1)
    util.assert_exact(g.view(np.uint32), got.view(np.uint32), "graph=1 vs eager")


@pytest.mark.parametrize("toy", sorted(TOYS))
def test_toy_model_rebatch(gpu, tmp_path, toy):
    """SetOption("batch", 3) on the batch-2 file: per image the same bits as batch-2 runs of the same images"""
    build, s, _ = TOYS[toy]
    pp, bp = save(build(), tmp_path)
    x3 = util.rng_uniform(21, (3,) + s[1:], 0.0, 1.0)
    _, y3 = run_engine(pp, bp, x3, batch=3)
    assert y3.shape[0] == 3
    for pair in ((0, 1), (2, 0)):
        _, y2 = run_engine(pp, bp, x3[list(pair)])
        for j, i in enumerate(pair):
            util.assert_exact(y3[i].view(np.uint32), y2[j].view(np.uint32), "image %d" % i)


@pytest.mark.parametrize("toy", sorted(TOYS))
def test_toy_model_fp16_storage(gpu, tmp_path, toy):
    """fp16=1: every param_act between two half tensors runs its half kernel with no cast pair around it (the clamp that writes the fp32
    graph output takes the engine's fp32 fallback), and the result is within F16_TOL of the fp16-storage emulation: fp64 arithmetic with the
    weights, the input and every operator's output rounded to fp16"""
    build, s, acts = TOYS[toy]
    b = build()
    pp, bp = save(b, tmp_path)
    x = mg.synth_input(s)
    e, got = run_engine(pp, bp, x, fp16=1)
    prof = e.profile()
    layers = act_layers(prof)
    assert [L["type"] for L in layers] == acts, layers
    names = [L["name"] for L in prof]
    last = _parse(b.lines[-2])[1]      # (a param_act that writes the fp32 graph output from a half input is the mixed pair: not judged here)
    for L in layers:   # (InsertFp32Fallbacks names its casts <layer>.in_to_f32.<k> / <layer>.out_to_f16.<k>)
        if L["name"] != last:
            assert not any(n.startswith(L["name"] + ".in_to_f32") or n.startswith(L["name"] + ".out_to_f16") for n in names), (L["name"], names)
    ref = ar.eval_graph(b, x)
    emu = ar.eval_graph(b, x, rnd=ar.round_f16)
    print("toy %s fp16 storage: vs the fp16 emulation max-based %.3e; vs fp64: engine %.3e, emulation %.3e" % (
        toy, util.rel_err(got, emu), util.rel_err(got, ref), util.rel_err(emu, ref)))
    assert np.isfinite(got).all()
    util.assert_parity(got, emu, rel=F16_TOL, what="toy %s fp16 storage vs the emulation" % toy)
