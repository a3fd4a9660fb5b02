"""GPU: arithmetic against graph constants -- si_hip_binary_const_f32 / _f16 (include/si_binary.h) against the numpy restatement of
tests/const_reference.py by equality of BITS (add / sub / mul / div and the reversed forms; a NaN by class, as everywhere in the suite: the
sign and payload of a generated NaN are the hardware's) and against the parent kernel si_hip_binary_f32 for pow / atan2: every broadcast
mask of the constant, one and two stages, both operand orders, both types, aligned and offset pointers, strides above the run, several
grid-stride passes, special values, views under guard bands, the form each launch reports.  Every test here fails without the kernel: the
symbols are missing."""
import numpy as np
import pytest

import const_reference as cr
import containment as ct
from elementwise_reference import same_bits_or_nan
from simpleinfer_amd import hipops

pytestmark = pytest.mark.gpu

DTYPES = {"f32": np.float32, "f16": np.float16}
TNAME = {np.float32: "float", np.float16: "_Float16"}
D3 = (1, 3, 4, 7, 8, 9, 32)
PIXELS = {1: (1, 1, 1), 5: (1, 1, 5), 64: (2, 4, 8), 257: (1, 257, 1)}


def values(seed, shape, dtype, lo=-4.0, hi=4.0):
    r = np.random.Generator(np.random.Philox(seed))
    return (lo + (hi - lo) * r.random(shape)).astype(dtype)


def assert_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    ok = same_bits_or_nan(got, want)
    if not ok.all():
        i = int(np.flatnonzero(~ok.reshape(-1))[0])
        raise AssertionError("%s: %d of %d elements differ in their bits; first at %s: got %r, want %r" % (
            what, int((~ok).sum()), ok.size, np.unravel_index(i, got.shape), got.reshape(-1)[i], want.reshape(-1)[i]))


def full_width(dtype):
    return 16 // np.dtype(dtype).itemsize


def kernel(dtype, vec, form):
    return "binary_const_kernel<%s, %d, %s>" % (TNAME[dtype], full_width(dtype) if vec else 1, form)


# how a case places its operands: the view hooks of the wrapper and the spare elements in front of the constants
def placements(d3, dtype):
    w = full_width(dtype)
    return [dict(),                                                         # dense, aligned
            dict(in_ld=d3 + w, out_ld=d3 + 2 * w, out_c_off=w),             # strides above the run, still 16-byte multiples
            dict(in_ld=d3 + 1, in_c_off=1, out_ld=d3 + 1, out_c_off=1),     # x and out offset by one element
            dict(c_off=1)]                                                  # the constants offset by one element


def vector_arm(d3, dtype, place):
    w = full_width(dtype)
    return d3 % w == 0 and place.get("in_ld", d3) % w == 0 and place.get("out_ld", d3) % w == 0 and place.get("in_c_off", 0) % w == 0 and \
        place.get("out_c_off", 0) % w == 0


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("pixels", sorted(PIXELS))
def test_every_mask_and_extent_has_the_bits_of_the_restatement(gpu, pixels, dt):
    """d3 x every broadcast mask of the first constant, a second constant of another mask in the two-stage launch, the six IEEE codes in
    both stages, the four placements rotated against the masks"""
    dtype = DTYPES[dt]
    for d3 in D3:
        s = PIXELS[pixels] + (d3,)
        x = values(d3 * 1000 + pixels, s, dtype)
        for m, mask in enumerate(cr.MASKS):
            place = placements(d3, dtype)[(m + m // 4) % 4]
            vec = vector_arm(d3, dtype, place)
            shapes = [cr.const_shape(s, mask), cr.const_shape(s, cr.MASKS[(5 * m + 3) % 16])]
            consts = [values(7 * m + k, cs, dtype, 0.25, 3.0) * dtype(1 - 2 * (k % 2)) for k, cs in enumerate(shapes)]
            ops = [cr.EXACT_OPS[m % 6], cr.EXACT_OPS[(m // 2 + 3) % 6]]
            for stages in (1, 2):
                what = "%s %s masks %s ops %s %s" % (s, dt, [mask, cr.MASKS[(5 * m + 3) % 16]][:stages], ops[:stages], place)
                got = hipops.binary_const(x, ops[:stages], consts[:stages], **place)
                name = hipops.LAST_KERNEL_NAME["si_hip_binary_const"]
                assert name == kernel(dtype, vec, cr.expected_form(s, shapes[:stages])), (what, name)
                assert_bits(got, cr.kernel_ref(x, ops[:stages], consts[:stages]), what + " [" + name + "]")


FORM_CONSTS = {"chan": (1, 1, 1, None), "pixel": (1, 5, 7, 1), "full": (3, 1, 7, None)}   # None: d3


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("form", sorted(FORM_CONSTS))
@pytest.mark.parametrize("arm", ["vector", "scalar"])
def test_every_code_in_every_form(gpu, arm, form, dt):
    """the six IEEE codes against the restatement and pow / atan2 (both orders) against the parent kernel si_hip_binary_f32 on the same
    operands -- for fp16 against its fp32 result rounded once"""
    dtype = DTYPES[dt]
    d3 = 32 if arm == "vector" else 9
    s = (3, 5, 7, d3)
    cs = tuple(d3 if v is None else v for v in FORM_CONSTS[form])
    x = values(41, s, dtype, 0.1, 3.0)
    x[0, 0, :, 0] *= -1                       # negative bases / arguments too
    c = values(42, cs, dtype, -2.0, 2.0)
    for op in cr.OPS:
        got = hipops.binary_const(x, [op], [c])
        assert hipops.LAST_KERNEL_NAME["si_hip_binary_const"] == kernel(dtype, arm == "vector", form)
        if op in cr.EXACT_OPS:
            want = cr.kernel_ref(x, [op], [c])
        else:
            want = hipops.binary_op(op, x.astype(np.float32), c.astype(np.float32)).reshape(s).astype(dtype)
        assert_bits(got, want, "op %d %s %s %s" % (op, form, arm, dt))


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_two_stages_have_the_bits_of_two_launches(gpu, dt):
    """x * scale + shift in one launch rounds as the two launches it replaces (no fma; under fp16 one rounding to half per stage), for every
    pair of the ten codes' representatives and every form"""
    dtype = DTYPES[dt]
    s = (3, 5, 7, 16)
    x = values(51, s, dtype, 0.1, 3.0)
    for form, fc in sorted(FORM_CONSTS.items()):
        cs = tuple(s[3] if v is None else v for v in fc)
        c0, c1 = values(52, cs, dtype, 0.3, 2.0), values(53, cs, dtype, -2.0, 2.0)
        for ops in ((2, 0), (2, 1), (3, 7), (8, 2), (0, 3), (6, 0), (2, 10), (9, 11)):
            both = hipops.binary_const(x, ops, [c0, c1])
            first = hipops.binary_const(x, ops[:1], [c0])
            assert_bits(both, hipops.binary_const(first, ops[1:], [c1]), "ops %s %s %s" % (ops, form, dt))


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("form", sorted(FORM_CONSTS))
def test_three_grid_stride_passes(gpu, form, dt):
    """grid_cap = 1: 256 lanes serve 840 (fp32 vectors), 420 (half vectors) and 3360 (scalar arm) items in 2 to 14 passes; in the chan form
    a pass is 32 runs of 8 pieces (fp32 vectors: 105 pixels, four passes, the last partly idle) or 8 runs of 32 elements (scalar arm)"""
    dtype = DTYPES[dt]
    s = (3, 5, 7, 32)
    cs = tuple(s[3] if v is None else v for v in FORM_CONSTS[form])
    x, c0, c1 = values(61, s, dtype), values(62, cs, dtype, 0.5, 2.0), values(63, cs, dtype)
    for place in (dict(), dict(in_ld=33, out_ld=35, out_c_off=2)):
        got = hipops.binary_const(x, [2, 0], [c0, c1], grid_cap=1, **place)
        assert hipops.LAST_KERNEL_NAME["si_hip_binary_const"] == kernel(dtype, not place, form)
        assert_bits(got, cr.kernel_ref(x, [2, 0], [c0, c1]), "%s %s %s" % (form, dt, place))
        assert_bits(got, hipops.binary_const(x, [2, 0], [c0, c1], **place), "capped vs uncapped")


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_special_values(gpu, dt):
    """every pair of ±0, ±Inf, NaN, subnormals, the ends of the finite range, 65504 with 15 and 16 (half: 65504 + 16 = 65520 rounds to Inf,
    65504 + 15 back to 65504) through add / sub / mul / div and the reversed forms; a division by zero gives the IEEE result (±Inf, NaN for
    0 / 0); vector and scalar arm"""
    dtype = DTYPES[dt]
    v = cr.special_values(dtype)
    v = np.concatenate([v, v[:32 - len(v)]])
    assert v.size == 32
    x = np.ascontiguousarray(np.broadcast_to(v[:, None], (1, 1, 32, 32)))
    for op in cr.EXACT_OPS:
        for place in (dict(), dict(in_ld=33, in_c_off=1)):
            got = hipops.binary_const(x, [op], [v.reshape(1, 1, 1, 32)], **place)
            assert_bits(got, cr.kernel_ref(x, [op], [v.reshape(1, 1, 1, 32)]), "op %d %s %s" % (op, dt, place))
    i0, i1, inf = int(np.flatnonzero(v == 0)[0]), int(np.flatnonzero(v == 1)[0]), int(np.flatnonzero(v == np.inf)[0])
    got = hipops.binary_const(x, [3], [v.reshape(1, 1, 1, 32)])[0, 0]
    assert got[i1, i0] == np.inf and np.isnan(got[i0, i0]) and got[i1, inf] == 0 and np.isnan(got[inf, inf])
    if dtype == np.float16:
        top, i15, i16 = int(np.flatnonzero(v == 65504)[0]), int(np.flatnonzero(v == 15)[0]), int(np.flatnonzero(v == 16)[0])
        got = hipops.binary_const(x, [0], [v.reshape(1, 1, 1, 32)])[0, 0]
        assert got[top, i15] == 65504 and got[top, i16] == np.inf
        # ... and the rounding happens after EACH stage: (65504 + 16) - 16 is Inf, not 65504
        two = hipops.binary_const(x, [0, 1], [v.reshape(1, 1, 1, 32), v.reshape(1, 1, 1, 32)])[0, 0]
        assert two[top, i16] == np.inf and two[top, i15] == 65504
        assert_bits(two, cr.kernel_ref(x, [0, 1], [v.reshape(1, 1, 1, 32)] * 2)[0, 0], "two stages on the special values")


# ---- views and containment: checks (a) - (d) of tests/test_gpu_containment.py ---------------------------------------------------------
class ViewCase:
    def __init__(self, cid, half, form, vec, s, **views):
        self.id, self.half, self.form, self.vec, self.s, self.views = cid, half, form, vec, s, views
        self.entries = ("si_hip_binary_const_f16" if half else "si_hip_binary_const_f32",)
        self.dtype = np.float16 if half else np.float32

    def operands(self):
        cs = tuple(self.s[3] if v is None else v for v in FORM_CONSTS[self.form])
        return values(71, self.s, self.dtype), [values(72, cs, self.dtype, 0.5, 2.0), values(73, cs, self.dtype)]

    def run(self, F):
        x, consts = self.operands()
        y = hipops.binary_const(x, [2, 0], consts, in_fill=F, out_fill=F, full=True, **self.views)
        return ct.Out("y", y, self.views.get("out_c_off", 0), self.s[3])


VIEW_CASES = []
for _half, _sfx, _w in ((False, "f32", 4), (True, "f16", 8)):
    for _form in sorted(FORM_CONSTS):
        VIEW_CASES += [
            # slices of wider rows at 16-byte aligned offsets; the input slice is the row's last
            ViewCase("%s_vector_%s" % (_form, _sfx), _half, _form, True, (3, 5, 7, 2 * _w), in_ld=4 * _w, in_c_off=2 * _w, out_ld=5 * _w, out_c_off=_w),
            # odd run, odd strides, odd offsets; the input slice ends where its buffer ends
            ViewCase("%s_scalar_%s" % (_form, _sfx), _half, _form, False, (3, 5, 7, 9), in_ld=14, in_c_off=5, out_ld=13, out_c_off=3),
        ]


@pytest.mark.parametrize("case", VIEW_CASES, ids=[c.id for c in VIEW_CASES])
def test_views_and_containment(gpu, case):
    del hipops.LAST_ENTRIES[:]
    plain = case.run(hipops.ByteFill(0x00))
    plain_kernel = hipops.LAST_KERNEL_NAME["si_hip_binary_const"]
    assert set(case.entries) <= set(hipops.LAST_ENTRIES), hipops.LAST_ENTRIES
    assert plain_kernel == kernel(case.dtype, case.vec, case.form), plain_kernel
    ct.assert_outside_fill(plain.full, plain.c_off, plain.c, 0x00, case.id + ", plain run")
    x, consts = case.operands()
    assert_bits(plain.dest, cr.kernel_ref(x, [2, 0], consts), case.id + " vs the restatement")
    for byte in ct.PATTERNS:
        with hipops.guard_bands(byte) as g:      # (a) all bands and (d) the inputs are compared when the block ends
            out = case.run(hipops.ByteFill(byte))
        what = "%s under 0x%02X" % (case.id, byte)
        assert g.checked == 4, "%s: the guard saw %d buffers" % (what, g.checked)   # x, c0, c1, y
        assert hipops.LAST_KERNEL_NAME["si_hip_binary_const"] == plain_kernel, what
        ct.assert_outside_fill(out.full, out.c_off, out.c, byte, what)                              # (b)
        ct.assert_same_bits(out.dest, plain.dest, what + ": guarded + pattern-filled vs plain")    # (c)


def test_refusals_leave_the_process_usable(gpu):
    x = values(81, (1, 3, 5, 8), np.float32)
    with pytest.raises(hipops.HipError):
        hipops.binary_const(x, [4], [np.ones((1, 1, 1, 8), np.float32)])          # max: no such code
    with pytest.raises(hipops.HipError):
        hipops.binary_const(x, [0], [np.ones((1, 1, 1, 8), np.float32)], in_ld=8, out_ld=8, grid_cap=-1)
    got = hipops.binary_const(x, [0], [np.ones((1, 1, 1, 8), np.float32)])
    assert_bits(got, x + np.float32(1), "after the refusals")


# ---- engine: pnnx.Attribute operands ------------------------------------------------------------------------------------------------------
# Every test below fails on an engine without graph constants: LoadModel stops at the first pnnx.Attribute (kEmpty: no such layer type).
import util  # noqa: E402
from ct_reference import _parse, round_f16  # noqa: E402
from simpleinfer_amd import modelgen as mg  # noqa: E402
from simpleinfer_amd.engine import Engine, Status, StatusError  # noqa: E402


def same_bits(got, want, what):
    outs = zip(got, want) if isinstance(got, list) else [(got, want)]
    for g, w in outs:
        ct.assert_same_bits(np.ascontiguousarray(g), np.ascontiguousarray(w), what)


def save(b, tmp_path, tag="m"):
    pp, bp = str(tmp_path / (tag + ".pnnx.param")), str(tmp_path / (tag + ".pnnx.bin"))
    b.save(pp, bp)
    return pp, bp


def run_engine(b, tmp_path, x, tag="m", forwards=1, **opts):
    """(engine, the graph output as the engine stores it -- a list when the graph has several)"""
    pp, bp = save(b, tmp_path, tag)
    e = Engine(**opts)
    e.load_model(pp, bp)
    (name,) = e.input_names()
    e.input(name, x)
    for _ in range(forwards):
        e.forward()
    # (by the engine's names: an expression's result is renamed by the lowering; sorted, which for these toys is the file's order)
    names = e.output_names()
    assert len(names) == sum(ln.startswith("pnnx.Output") for ln in b.lines), names
    outs = [e.extract(n) for n in names]
    return e, outs[0] if len(outs) == 1 else outs


def toy_input(b):
    n, c, h, w = b.shapes["0"]
    return mg.synth_input((n, h, w, c))


def parity(got, want, what, **kw):
    outs = zip(got, want) if isinstance(got, list) else [(got, want)]
    for i, (g, w) in enumerate(outs):
        util.assert_parity(g, w, what="%s, output %d" % (what, i), **kw)


TOYS = {
    "frozenbn": lambda **kw: mg.build_toy_frozenbn_block(**kw),
    "layer_scale": lambda **kw: mg.build_toy_layer_scale(**kw),
    "flow_const": lambda **kw: mg.build_toy_flow_warp_const(**kw),
    "pos_seq_first": lambda **kw: mg.build_toy_pos_embed(batch_first=False, **kw),
    "pos_batch_first": lambda **kw: mg.build_toy_pos_embed(batch_first=True, **kw),
    "fcos_scale": lambda **kw: mg.build_toy_fcos_scale(**kw),
}
# (toy: the BinaryOp steps of the default plan with the form each takes; the retired second stages)
PLANS = {
    "frozenbn": (["chan", "chan", None], ["add_1", "add_3"]),           # two x * scale + shift pairs, one launch each; the skip add is today's kernel
    "layer_scale": (["chan", None], []),
    "flow_const": (["full"], []),
    "pos_seq_first": (["full", None], []),
    "pos_batch_first": (["full", None], []),
    "fcos_scale": (["chan", "chan"], []),
}


def binary_steps(eng):
    return [L for L in eng.profile() if L["type"] == "BinaryOp"]


@pytest.mark.parametrize("which", sorted(TOYS))
def test_toys_fp32(gpu, tmp_path, which):
    b = TOYS[which]()
    x = toy_input(b)
    want = cr.eval_graph(b, x)
    eng, got = run_engine(b, tmp_path, x)
    parity(got, want, "toy " + which)
    assert eng.input_names() == ["0"], eng.input_names()                      # the constants are no inputs
    forms, fused = PLANS[which]
    steps = binary_steps(eng)
    assert [("binary_const_kernel" in L["kernel"], L["kernel"].split(", ")[-1].rstrip(">") if "binary_const_kernel" in L["kernel"] else None)
            for L in steps] == [(f is not None, f) for f in forms], steps
    sched = eng.schedule()
    assert sorted(n for n in sched["fused"] if n.startswith(("add_", "mul_"))) == fused, sched["fused"]
    assert not any(n.startswith("pnnx_attr") for n in sched["run"]), sched["run"]    # a constant has no step
    # graph=1 over three forwards, and the passes off: the same bits
    _, cap = run_engine(b, tmp_path, x, forwards=3, graph=1)
    same_bits(cap, got, which + ": graph=1 replay over three forwards")
    for opts in (dict(fuse_const=0), dict(fuse=0)):
        e0, plain = run_engine(b, tmp_path, x, **opts)
        same_bits(plain, got, "%s: %r" % (which, opts))
        assert not set(fused) & set(e0.schedule()["fused"]), (opts, e0.schedule()["fused"])
        assert set(fused) <= set(e0.schedule()["run"]), (opts, e0.schedule()["run"])


@pytest.mark.parametrize("which", sorted(TOYS))
def test_toys_fp16_storage(gpu, tmp_path, which):
    """fp16=1: the constants are held as halves and the constant form runs its fp16 kernels; the error against float64 is at most 2x that of
    the fp16-storage emulation (weights, biases, constants, the input and every operator's output rounded to fp16, float64 arithmetic
    between): the bar of the other toys' fp16 tests"""
    b = TOYS[which]()
    x = toy_input(b)
    eng, got = run_engine(b, tmp_path, x, fp16=1)
    ref, emu = cr.eval_graph(b, x), cr.eval_graph(b, x, rnd=round_f16)
    gl, rl, el = (v if isinstance(v, list) else [v] for v in (got, ref, emu))
    for g, r, e in zip(gl, rl, el):
        e_engine, e_emu = util.rel_err(g, r), util.rel_err(e, r)
        print("toy %s fp16 storage vs float64: engine %.3e, fp16 emulation %.3e" % (which, e_engine, e_emu))
        assert np.isfinite(g).all()
        assert e_engine <= 2.0 * e_emu, (e_engine, e_emu)
    assert any("binary_const_kernel<_Float16" in L["kernel"] for L in binary_steps(eng)), binary_steps(eng)
    e0, plain = run_engine(b, tmp_path, x, fp16=1, fuse_const=0)
    same_bits(plain, got, which + ": fp16, fuse_const=0")


@pytest.mark.parametrize("which", sorted(TOYS))
def test_toys_rebatched(gpu, tmp_path, which):
    """batch=4 from a file traced at 2: the constants keep their shapes (also dimension 0), everything else follows"""
    b2, b4 = TOYS[which](batch=2), TOYS[which](batch=4)
    x = toy_input(b4)
    eng, got = run_engine(b2, tmp_path, x, tag="b2", batch=4)
    parity(got, cr.eval_graph(b4, x), "batch=4 on the batch-2 file")
    _, want = run_engine(b4, tmp_path, x, tag="b4")
    same_bits(got, want, "batch=4 on the batch-2 file vs the batch-4 file")
    for ln in b2.lines:
        if ln.startswith("pnnx.Attribute"):
            r = _parse(ln)[3][0]
            stored = eng.operand_shape(r)
            assert int(np.prod(stored)) == int(np.prod(b2.shapes[r])), (r, stored)


@pytest.mark.parametrize("mode", ["host_slices2", "streams2"])
@pytest.mark.parametrize("which", sorted(TOYS))
def test_toys_batch_split(gpu, tmp_path, which, mode):
    """the split run has the bits of the unsplit one, and it really was split: no operator against a constant combines images"""
    b = TOYS[which](batch=4)
    x = toy_input(b)
    e0, base = run_engine(b, tmp_path, x, host_slices=1, streams=1)
    parity(base, cr.eval_graph(b, x), "unsplit")
    opts, slices, lanes = {"host_slices2": (dict(host_slices=2), 2, 1), "streams2": (dict(streams=2), 1, 2)}[mode]
    seq_first = which == "pos_seq_first"    # its graph output [L, N, E] carries the batch in dimension 1: never cut, with or without constants
    if seq_first and mode == "streams2":
        with pytest.raises(StatusError) as ei:
            run_engine(b, tmp_path, x, **opts)
        assert ei.value.status == Status.kUnsupport
        assert [m.split(" ")[0] for m in e0.schedule()["batch_mixing"]] == ["pnnx_output_0"], e0.schedule()
        return
    e1, got = run_engine(b, tmp_path, x, **opts)
    sched = e1.schedule()
    if seq_first:
        assert [m.split(" ")[0] for m in sched["batch_mixing"]] == ["pnnx_output_0"], sched
    else:
        assert sched["batch_mixing"] == [] and sched["host_slices"] == slices and sched["lanes"] == lanes, sched
    same_bits(got, base, mode)


def test_flow_warp_constant_has_the_bits_of_the_input_form(gpu, tmp_path):
    bc, bi = mg.build_toy_flow_warp_const(), mg.build_toy_flow_warp()
    x = toy_input(bc)
    _, got = run_engine(bc, tmp_path, x, tag="const")
    pp, bp = save(bi, tmp_path, "input")
    e = Engine()
    e.load_model(pp, bp)
    assert e.input_names() == ["0", "1"]
    e.input("0", x)
    e.input("1", mg.flow_base_grid(2, 24, 20))
    e.forward()
    same_bits(got, e.extract(e.output_names()[0]), "base grid as a constant vs as a graph input")


def test_a_constant_is_no_input(gpu, tmp_path):
    b = mg.build_toy_layer_scale()
    pp, bp = save(b, tmp_path)
    e = Engine()
    e.load_model(pp, bp)
    (attr,) = [_parse(ln)[3][0] for ln in b.lines if ln.startswith("pnnx.Attribute")]
    assert e.input_names() == ["0"] and attr not in e.input_names()
    with pytest.raises(StatusError) as ei:
        e._check("Input", e._L.si_engine_input(e._h, attr.encode(), np.zeros(24, np.float32).ctypes.data, 0))
    with pytest.raises(StatusError) as unknown:
        e._check("Input", e._L.si_engine_input(e._h, b"no_such_operand", np.zeros(24, np.float32).ctypes.data, 0))
    assert ei.value.status == unknown.value.status == Status.kFail


def test_refused_at_load(gpu, tmp_path):
    """each refusal returns its Status with the operator named in the log, and the process goes on"""
    def status(b, tag, patch_bin=None):
        pp, bp = save(b, tmp_path, tag)
        with pytest.raises(StatusError) as ei:
            Engine().load_model(pp, bp)
        return ei.value.status

    def one_const(shape=(1, 8, 1, 1), xshape=(2, 8, 5, 6)):
        b = mg.PnnxBuilder(seed=2)
        x = b.input(xshape)
        c = b.attribute(np.ones(shape, np.float32))
        return b, x, c

    # a type other than f32
    b, x, c = one_const()
    b.output(b.expression("mul(@0,@1)", [x, c]))
    b.lines = [ln.replace("@data=(1,8,1,1)f32", "@data=(1,8,1,1)i32").replace("#%s=(1,8,1,1)f32" % c, "#%s=(1,8,1,1)i32" % c) for ln in b.lines]
    assert status(b, "i32") == Status.kUnsupport
    # no data attribute
    b, x, c = one_const()
    b.output(b.expression("mul(@0,@1)", [x, c]))
    b.lines = [ln.replace(" @data=(1,8,1,1)f32", "") if ln.startswith("pnnx.Attribute") else ln for ln in b.lines]
    assert status(b, "nodata") == Status.kFail
    # a data size that is not the shape's
    b, x, c = one_const()
    b.output(b.expression("mul(@0,@1)", [x, c]))
    b.lines = [ln.replace("#%s=(1,8,1,1)f32" % c, "#%s=(1,4,1,1)f32" % c) for ln in b.lines]
    assert status(b, "size") == Status.kFail
    # an attribute whose output is a graph output directly
    b, x, c = one_const()
    b.output(b.relu(x))
    b.output(c)
    assert status(b, "output") == Status.kUnsupport
    # promoted rank above 4
    b = mg.PnnxBuilder(seed=2)
    x = b.view(b.input((2, 8, 5, 6)), (2, 2, 4, 5, 6))
    c = b.attribute(np.ones((4, 1, 1), np.float32))
    b.output(b.view(b.expression("mul(@0,@1)", [x, c]), (2, 8, 5, 6)))
    assert status(b, "rank5") == Status.kUnsupport
    # ... and the process goes on
    b = mg.build_toy_layer_scale()
    _, got = run_engine(b, tmp_path, toy_input(b), tag="after")
    parity(got, cr.eval_graph(b, toy_input(b)), "after the refusals")
