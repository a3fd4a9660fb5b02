"""GPU: torch.chunk / torch.split / Tensor.slice -- si_hip_slice_f32 / _f16 and si_hip_split_channels_f32 / _f16 (include/si_slice.h)
against the numpy rules (tests/slice_reference.py) by equality of BITS: every form the header declares on inputs that hold NaN payloads,
infinities, -0.0 and subnormals, strided views on both sides under guard bands, more than two grid-stride passes with a ragged last one; and
the layer inside the engine: one-op graphs for the three type strings and both Tensor.slice spellings, the four toy models (C2f, Focus,
Res2Net, Ghost) in fp32 and with fp16 storage under alias_split / alias_cat 1 and 0, and what the planner may and may not turn into a view.
Every engine test fails without the layers (LoadModel rejects the types with kEmpty: test_loads_chunk), every op-level test without the
kernels (the symbols are missing)."""
import ctypes as C

import numpy as np
import pytest

import containment as ct
import slice_reference as sl
import util
from ct_reference import _parse
from simpleinfer_amd import _native, hipops, modelgen as mg
from simpleinfer_amd.engine import Engine, Status, StatusError

pytestmark = pytest.mark.gpu

DTYPES = {"f32": np.float32, "f16": np.float16}
TNAME = {"f32": "float", "f16": "_Float16"}
VW = {"f32": 4, "f16": 8}
ALL = slice(None)


def bit_patterns(seed, shape, dtype):
    """random BITS viewed as the float type, with a quiet and a signalling NaN that carry payloads, both infinities, -0.0, +0.0 and the
    smallest and largest subnormals planted at the front"""
    r = np.random.Generator(np.random.Philox(seed))
    if dtype == np.float32:
        x = r.integers(0, 2 ** 32, shape, dtype=np.uint32)
        special = [0x7FC12345, 0xFF800001, 0x7F800000, 0xFF800000, 0x80000000, 0x00000000, 0x00000001, 0x807FFFFF]
    else:
        x = r.integers(0, 2 ** 16, shape, dtype=np.uint16)
        special = [0x7E55, 0xFC01, 0x7C00, 0xFC00, 0x8000, 0x0000, 0x0001, 0x83FF]
    flat = x.reshape(-1)
    step = max(flat.size // len(special), 1)
    for i, v in enumerate(special):
        flat[(i * step) % flat.size] = v
    return x.view(dtype)


def slice_form(dt, f):
    return "slice_vec<%s, %d>" % (TNAME[dt], VW[dt]) if f == "v" else "slice_elem<%s>" % TNAME[dt]


def split_form(dt, f):
    return "split_vec<%s, %d>" % (TNAME[dt], VW[dt]) if f == "v" else "split_elem<%s>" % TNAME[dt]


ALL_FORMS = {f(dt, k) for f in (slice_form, split_form) for dt in DTYPES for k in "ve"}


def ch(*a):
    return (ALL, ALL, ALL, slice(*a))


# (id, NHWC shape, index, the form dense 16-byte aligned buffers take in fp32, in fp16)
SLICE_TABLE = [
    ("c16_4to12", (2, 5, 6, 16), ch(4, 12), "v", "e"),
    ("c16_8to16", (2, 5, 6, 16), ch(8, 16), "v", "v"),
    ("c12_3to10", (2, 5, 6, 12), ch(3, 10), "e", "e"),
    ("c12_1_step2", (2, 5, 6, 12), ch(1, None, 2), "e", "e"),
    ("focus_00", (2, 8, 10, 3), (ALL, slice(0, None, 2), slice(0, None, 2), ALL), "e", "e"),
    ("focus_10", (2, 8, 10, 3), (ALL, slice(1, None, 2), slice(0, None, 2), ALL), "e", "e"),
    ("focus_01", (2, 8, 10, 3), (ALL, slice(0, None, 2), slice(1, None, 2), ALL), "e", "e"),
    ("focus_11", (2, 8, 10, 3), (ALL, slice(1, None, 2), slice(1, None, 2), ALL), "e", "e"),
    ("h1to4_w2to7", (2, 7, 9, 8), (ALL, slice(1, 4), slice(2, 7), ALL), "v", "v"),
    ("n1to2", (3, 4, 4, 8), (slice(1, 2), ALL, ALL, ALL), "v", "v"),
]

# (id, NHWC shape, widths, form in fp32, in fp16); 10 pieces: more than SI_SPLIT_MAX, the launcher loops
SPLIT_TABLE = [
    ("24_8_8_8", (2, 5, 6, 24), (8, 8, 8), "v", "v"),
    ("24_4_20", (2, 5, 6, 24), (4, 20), "v", "e"),
    ("24_5_7_12", (2, 5, 6, 24), (5, 7, 12), "e", "e"),
    ("40_10x4", (2, 3, 3, 40), (4,) * 10, "v", "e"),
]

FORMS_SEEN = set()


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("case", SLICE_TABLE, ids=[c[0] for c in SLICE_TABLE])
def test_slice_moves_the_bits_of_the_rule(gpu, case, dt):
    cid, s, index, f32, f16 = case
    x = bit_patterns(17, s, DTYPES[dt])
    got = hipops.slice(x, index)
    kernel = hipops.LAST_KERNEL_NAME["si_hip_slice"]
    FORMS_SEEN.add(kernel)
    assert kernel == slice_form(dt, f32 if dt == "f32" else f16), kernel
    ct.assert_same_bits(got, np.ascontiguousarray(x[index]), "%s %s [%s]" % (cid, dt, kernel))
    ct.assert_same_bits(got, hipops.slice(x, index), "two launches")


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("case", SPLIT_TABLE, ids=[c[0] for c in SPLIT_TABLE])
def test_split_moves_the_bits_of_the_rule(gpu, case, dt):
    cid, s, widths, f32, f16 = case
    x = bit_patterns(19, s, DTYPES[dt])
    got = hipops.split_channels(x, widths)
    kernel = hipops.LAST_KERNEL_NAME["si_hip_split_channels"]
    FORMS_SEEN.add(kernel)
    assert kernel == split_form(dt, f32 if dt == "f32" else f16), kernel
    want = sl.split_ref(x, widths, 1)
    assert len(got) == len(want) == len(widths)
    for i, (g, w) in enumerate(zip(got, want)):
        ct.assert_same_bits(g, w, "%s %s piece %d [%s]" % (cid, dt, i, kernel))


def test_all_forms_ran(gpu):
    """the names reported over the two tables are exactly the forms the header declares (runs after the parametrised tests above, whose
    names it collects)"""
    if FORMS_SEEN != ALL_FORMS:
        for dt, dtype in DTYPES.items():
            for _, s, index, _, _ in SLICE_TABLE:
                hipops.slice(bit_patterns(1, s, dtype), index)
                FORMS_SEEN.add(hipops.LAST_KERNEL_NAME["si_hip_slice"])
            for _, s, widths, _, _ in SPLIT_TABLE:
                hipops.split_channels(bit_patterns(1, s, dtype), widths)
                FORMS_SEEN.add(hipops.LAST_KERNEL_NAME["si_hip_split_channels"])
    assert FORMS_SEEN == ALL_FORMS, FORMS_SEEN


def test_overlapping_and_partial_destinations(gpu):
    """the offsets need not tile the input: two overlapping ranges and an untouched tail"""
    x = bit_patterns(23, (2, 3, 5, 16), np.float32)
    a, b = hipops.split_channels(x, (8, 4), offsets=(0, 4))
    ct.assert_same_bits(a, np.ascontiguousarray(x[..., 0:8]), "range 0")
    ct.assert_same_bits(b, np.ascontiguousarray(x[..., 4:8]), "range 1")


@pytest.mark.parametrize("kernel", ["slice", "split"])
def test_grid_stride_passes_with_a_ragged_last_one(gpu, kernel):
    """2 x 1031 x 511 x 8 fp32 through the vec form: 2 107 364 vectors for at most 524 288 lanes -- four full passes and a fifth of 10 212"""
    s = (2, 1031, 511, 8)
    assert 4 * 524288 < s[0] * s[1] * s[2] * 2 < 5 * 524288
    x = bit_patterns(29, s, np.float32)
    if kernel == "slice":
        got = [hipops.slice(x, ch(0, 8), out_fill=hipops.ByteFill(0x7B))]
        assert hipops.LAST_KERNEL_NAME["si_hip_slice"] == "slice_vec<float, 4>"
        want = [x]
    else:
        got = hipops.split_channels(x, (4, 4), out_fill=hipops.ByteFill(0x7B))
        assert hipops.LAST_KERNEL_NAME["si_hip_split_channels"] == "split_vec<float, 4>"
        want = [np.ascontiguousarray(x[..., :4]), np.ascontiguousarray(x[..., 4:])]
    for g, w in zip(got, want):
        ct.assert_same_bits(g, w, "%s over five passes" % kernel)


# ---- views and containment: checks (a) - (d) of tests/test_gpu_containment.py ---------------------------------------------------------
class SliceView:
    def __init__(self, cid, half, s, index, f, **views):
        self.id = "slice_%s_%s" % (cid, "f16" if half else "f32")
        self.half, self.s, self.index, self.views = half, s, index, views
        self.dtype = np.float16 if half else np.float32
        self.form = slice_form("f16" if half else "f32", f)
        self.entries = ("si_hip_slice_f16" if half else "si_hip_slice_f32",)
        self.key = "si_hip_slice"
        self.buffers = 2   # x, y

    def input(self):
        return bit_patterns(31, self.s, self.dtype)

    def reference(self):
        return [np.ascontiguousarray(self.input()[self.index])]

    def run(self, F):
        y = hipops.slice(self.input(), self.index, in_fill=F, out_fill=F, full=True, **self.views)
        return [ct.Out("y", y, self.views.get("out_c_off", 0), self.reference()[0].shape[-1])]


class SplitView:
    def __init__(self, cid, half, s, widths, f, **views):
        self.id = "split_%s_%s" % (cid, "f16" if half else "f32")
        self.half, self.s, self.widths, self.views = half, s, widths, views
        self.dtype = np.float16 if half else np.float32
        self.form = split_form("f16" if half else "f32", f)
        self.entries = ("si_hip_split_channels_f16" if half else "si_hip_split_channels_f32",)
        self.key = "si_hip_split_channels"
        self.buffers = 1 + len(widths)   # x and every destination

    def input(self):
        return bit_patterns(37, self.s, self.dtype)

    def reference(self):
        return sl.split_ref(self.input(), self.widths, 1)

    def run(self, F):
        ys = hipops.split_channels(self.input(), self.widths, in_fill=F, out_fill=F, full=True, **self.views)
        offs = self.views.get("out_c_offs") or [0] * len(self.widths)
        return [ct.Out("y%d" % i, y, offs[i], self.widths[i]) for i, y in enumerate(ys)]


VIEW_CASES = []
for _half in (False, True):
    _e = 2 if _half else 1   # elements in 4 bytes: a pointer that far into a row is 4 bytes off a 16-byte boundary
    VIEW_CASES += [
        # both tensors at 16-byte aligned channel offsets of wider rows: the vec forms
        SliceView("vector", _half, (2, 5, 6, 32), ch(8, 24), "v", in_ld=48, in_c_off=16, out_ld=32, out_c_off=16),
        SliceView("vector_hw", _half, (2, 7, 9, 8), (ALL, slice(1, 4), slice(2, 7), ALL), "v", in_ld=24, in_c_off=8, out_ld=16, out_c_off=8),
        # a stride of c + 1 forces the element form on vector-sized channels
        SliceView("odd_stride", _half, (1, 4, 5, 16), ch(8, 16), "e", in_ld=17, in_c_off=0, out_ld=9, out_c_off=1),
        # vector-sized everything, but both pointers 4 bytes off a 16-byte boundary
        SliceView("off_4_bytes", _half, (2, 3, 5, 16), ch(8, 16), "e", in_ld=24, in_c_off=_e, out_ld=16, out_c_off=_e),
        # a Focus slice of an RGB image held in rows of 4, written into its 3 channels of the 12-channel concat
        SliceView("focus", _half, (2, 8, 10, 3), (ALL, slice(1, None, 2), slice(1, None, 2), ALL), "e", in_ld=4, in_c_off=1, out_ld=12, out_c_off=9),
        # a channel step
        SliceView("channel_step", _half, (2, 3, 5, 12), ch(1, None, 3), "e", in_ld=13, in_c_off=1, out_ld=7, out_c_off=2),
        SplitView("vector", _half, (2, 5, 6, 24), (8, 8, 8), "v", in_ld=32, in_c_off=8, out_lds=(16, 24, 16), out_c_offs=(8, 16, 0)),
        SplitView("off_4_bytes", _half, (2, 5, 6, 24), (8, 16), "e", in_ld=32, in_c_off=_e, out_lds=(16, 24), out_c_offs=(_e, 8)),
        SplitView("odd", _half, (2, 5, 6, 24), (5, 7, 12), "e", in_ld=29, in_c_off=3, out_lds=(9, 8, 13), out_c_offs=(2, 0, 1)),
        SplitView("ten_pieces", _half, (2, 3, 3, 80), (8,) * 10, "v", in_ld=88, in_c_off=8, out_lds=(16,) * 10, out_c_offs=(8, 0) * 5),
    ]


@pytest.mark.parametrize("case", VIEW_CASES, ids=[c.id for c in VIEW_CASES])
def test_views_and_containment(gpu, case):
    del hipops.LAST_ENTRIES[:]
    plain = case.run(hipops.ByteFill(0x00))
    plain_kernel = hipops.LAST_KERNEL_NAME[case.key]
    assert set(case.entries) <= set(hipops.LAST_ENTRIES), hipops.LAST_ENTRIES
    assert plain_kernel == case.form, plain_kernel
    for out, ref in zip(plain, case.reference()):
        ct.assert_outside_fill(out.full, out.c_off, out.c, 0x00, case.id + ", plain run")
        # the value too: nothing of the gaps between the input's pixels reached the output
        ct.assert_same_bits(out.dest, ref, "%s %s vs the rule" % (case.id, out.name))
    for byte in ct.PATTERNS:
        with hipops.guard_bands(byte) as g:      # (a) all bands and (d) the input are compared when the block ends
            outs = case.run(hipops.ByteFill(byte))
        what = "%s under 0x%02X" % (case.id, byte)
        assert g.checked == case.buffers, "%s: the guard saw %d buffers" % (what, g.checked)
        assert hipops.LAST_KERNEL_NAME[case.key] == plain_kernel, what
        for out, p in zip(outs, plain):
            ct.assert_outside_fill(out.full, out.c_off, out.c, byte, what)                          # (b)
            ct.assert_same_bits(out.dest, p.dest, what + ": guarded + pattern-filled vs plain")    # (c)


# ---- engine ---------------------------------------------------------------------------------------------------------------------------
def save(b, tmp_path, tag="m"):
    pp, bp = str(tmp_path / (tag + ".pnnx.param")), str(tmp_path / (tag + ".pnnx.bin"))
    b.save(pp, bp)
    return pp, bp


def graph_outputs(b):
    return [_parse(ln)[2][0] for ln in b.lines if ln.startswith("pnnx.Output")]


def run_engine(b, tmp_path, x, tag="m", **opts):
    """(engine, the graph's outputs in the order of its pnnx.Output lines)"""
    pp, bp = save(b, tmp_path, tag)
    e = Engine(**opts)
    e.load_model(pp, bp)
    e.input(e.input_names()[0], x)
    e.forward()
    return e, [e.extract(name) for name in graph_outputs(b)]


def new_layers(prof):
    return [L for L in prof if L["type"] in sl.THREE]


def one_op_graph(s, op, *a, **kw):
    """input -> one chunk / split / slice (a PnnxBuilder method and its arguments) -> one output per piece, for an NHWC shape (or [N, F])"""
    b = mg.PnnxBuilder(seed=5)
    x = b.input((s[0], s[3], s[1], s[2]) if len(s) == 4 else s)
    ys = getattr(b, op)(x, *a, **kw)
    for y in ([ys] if isinstance(ys, str) else ys):
        b.output(y)
    return b


def test_loads_chunk(gpu, tmp_path):
    """a torch.chunk graph loads and runs (without the layer LoadModel fails with kEmpty: the type is not registered)"""
    b = one_op_graph((2, 4, 6, 8), "chunk", 2, 1)
    x = bit_patterns(9, (2, 4, 6, 8), np.float32)
    e, got = run_engine(b, tmp_path, x)
    assert len(got) == 2
    for g, w in zip(got, sl.chunk_ref(x, 2, 1)):
        ct.assert_same_bits(g, w, "torch.chunk")
    layers = new_layers(e.profile())
    assert len(layers) == 1 and layers[0]["type"] == "torch.chunk" and layers[0]["kernel"] == "split_channels", layers
    assert layers[0]["flops"] == 0.0


ONE_OP = {
    "chunk_uneven_3_of_8": ((2, 4, 6, 8), "chunk", (3, 1), {}, "split_channels"),
    "chunk_negative_dim": ((2, 4, 6, 8), "chunk", (2, -3), {}, "split_channels"),
    "chunk_h": ((2, 5, 6, 8), "chunk", (2, 2), {}, "slice"),
    "chunk_rank2": ((3, 20), "chunk", (3, 1), {}, "split_channels"),
    "split_int_short_tail": ((2, 4, 6, 10), "split", (4, 1), {}, "split_channels"),
    "split_sections": ((2, 4, 6, 24), "split", ((5, 7, 12), 1), {}, "split_channels"),
    "split_w": ((2, 4, 7, 8), "split", ((2, 5), 3), {}, "slice"),
    "split_n": ((3, 4, 4, 8), "split", (1, 0), {}, "slice"),
    "slice_channels": ((2, 4, 6, 16), "slice", (1, 4, 12, 1), {}, "split_channels"),
    "slice_negative": ((2, 4, 6, 16), "slice", (1, -12, -3, 2), {}, "slice"),
    "slice_open_end": ((2, 7, 6, 8), "slice", (2, 3, None, 1), {}, "slice"),
    "slice_none_end": ((2, 7, 6, 8), "slice", (-1, 1, "None", 2), {}, "slice"),
    "slice_int64_end": ((2, 7, 6, 8), "slice", (3, 2, 9223372036854775807, 1), {}, "slice"),
    "slice_many_axes": ((2, 7, 9, 8), "slice", ((2, 3, 1), (1, 2, 0), (4, 7, None), (1, 1, 1)), {}, "slice"),
    "slice_focus": ((2, 8, 10, 3), "slice", ((2, 3), (1, 0), (None, None), (2, 2)), {}, "slice"),
    "slice_rank2": ((3, 20), "slice", (1, 5, -5, 1), {}, "split_channels"),
}


@pytest.mark.parametrize("which", sorted(ONE_OP))
def test_engine_one_op_graph(gpu, tmp_path, which):
    """LoadModel -> Forward -> Extract reproduces the rule bit for bit, for every output of the operator"""
    s, op, args, kw, kernel = ONE_OP[which]
    b = one_op_graph(s, op, *args, **kw)
    typ, _, _, _, prm = _parse(b.lines[1])
    x = bit_patterns(9, s, np.float32)
    want = sl.apply_line(typ, prm, x)
    e, got = run_engine(b, tmp_path, x)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        ct.assert_same_bits(g, w, "%s output %d" % (which, i))
    layers = new_layers(e.profile())
    assert len(layers) == 1 and layers[0]["type"] == typ and layers[0]["kernel"] == kernel, layers
    assert e.schedule()["alias"] == [], "a piece of a graph input that is a graph output is never a view"


TOYS = {
    "c2f": (lambda: mg.build_toy_c2f(), (2, 16, 16, 16)),
    "focus": (lambda: mg.build_toy_focus(), (2, 16, 16, 3)),
    "res2net": (lambda: mg.build_toy_res2net_block(), (2, 12, 12, 3)),
    "ghost": (lambda: mg.build_toy_ghost(), (2, 16, 16, 16)),
}
PLANS = [(1, 1), (1, 0), (0, 1), (0, 0)]
REFS = {}


def toy(which):
    """(builder, input, fp64 reference, fp16-storage emulation): computed once, shared by the tests below"""
    if which not in REFS:
        build, s = TOYS[which]
        b = build()
        x = mg.synth_input(s)
        REFS[which] = (b, x, sl.eval_graph(b, x), sl.eval_graph(b, x, rnd=sl.round_f16))
    return REFS[which]


@pytest.mark.parametrize("plan", PLANS, ids=["split%d_cat%d" % p for p in PLANS])
@pytest.mark.parametrize("which", sorted(TOYS))
def test_toy_fp32(gpu, tmp_path, which, plan):
    b, x, ref, _ = toy(which)
    e, (got,) = run_engine(b, tmp_path, x, alias_split=plan[0], alias_cat=plan[1])
    print("toy %s fp32 %r: max-based %.3e, element-wise %.3e" % (which, plan, util.rel_err(got, ref), util.mixed_err(got, ref)))
    util.assert_parity(got, ref, what="toy %s fp32 alias_split=%d alias_cat=%d" % ((which,) + plan))
    types = [ln.split()[0] for ln in b.lines]
    assert sorted(L["type"] for L in new_layers(e.profile())) == sorted(t for t in types if t in sl.THREE)
    assert all(L["kernel"] in ("view", "split_channels", "slice") for L in new_layers(e.profile())), new_layers(e.profile())
    if plan == (1, 1):
        _, (g,) = run_engine(b, tmp_path, x, graph=1)      # a captured graph replays the same bits
        util.assert_exact(g.view(np.uint32), got.view(np.uint32), "graph=1 vs eager")


@pytest.mark.parametrize("plan", PLANS, ids=["split%d_cat%d" % p for p in PLANS])
@pytest.mark.parametrize("which", sorted(TOYS))
def test_toy_fp16_storage(gpu, tmp_path, which, plan):
    """fp16=1: the error against fp64 is at most 2x that of the fp16-storage emulation (weights, biases, the input and every layer's output
    rounded to fp16, fp64 arithmetic between) -- the factor of tests/test_gpu_superres.py"""
    b, x, ref, emu = toy(which)
    e, (got,) = run_engine(b, tmp_path, x, fp16=1, alias_split=plan[0], alias_cat=plan[1])
    e_engine, e_emu = util.rel_err(got, ref), util.rel_err(emu, ref)
    print("toy %s fp16 storage %r vs fp64: engine %.3e, fp16 emulation %.3e" % (which, plan, e_engine, e_emu))
    assert np.isfinite(got).all()
    assert e_engine <= 2.0 * e_emu, (e_engine, e_emu)


def chunk_step(e):
    (L,) = [L for L in e.profile() if L["type"] == "torch.chunk"]
    return L


def test_c2f_chunk_is_a_view(gpu, tmp_path):
    b, x, ref, _ = toy("c2f")
    chunk = [_parse(ln) for ln in b.lines if ln.startswith("torch.chunk")][0]
    e, (got,) = run_engine(b, tmp_path, x, alias_split=1)
    assert chunk_step(e)["kernel"] == "view", chunk_step(e)
    alias = e.schedule()["alias"]
    assert set(chunk[3]) <= set(alias), (chunk[3], alias)
    e0, (got0,) = run_engine(b, tmp_path, x, alias_split=0)
    assert chunk_step(e0)["kernel"] == "split_channels", chunk_step(e0)
    util.assert_parity(got, ref, what="c2f, views")
    util.assert_parity(got0, ref, what="c2f, copies")
    # the fp16 halves sit at 0 and 32 bytes: views too
    eh, _ = run_engine(b, tmp_path, x, fp16=1)
    assert chunk_step(eh)["kernel"] == "view" and set(chunk[3]) <= set(eh.schedule()["alias"])


def test_alias_of_an_alias(gpu, tmp_path):
    """a conv output feeds a chunk AND a concat: the operand lives in the concat buffer, and the chunk's views hang off that buffer at the
    summed channel offset with the concat's pixel stride"""
    b = mg.PnnxBuilder(seed=7)
    x = b.input((2, 8, 10, 10))
    first = x
    for _ in range(4):
        first = mg._Conv(b, first, 16, 3)        # in front of X in the concat: X's offset there is 16 channels
    X = b.conv(x, 32, 1)
    y0, y1 = b.chunk(X, 2, 1)
    assert [X, y0, y1] == ["9", "10", "11"]      # the views' names sort BEFORE their parent's: they are bound first, and only to a root can they be
    p, q = mg._Conv(b, y0, 16, 3), mg._Conv(b, y1, 16, 1)
    b.output(mg._Conv(b, b.cat([first, X, p, q], 1), 8, 1))
    xin = util.rng_uniform(15, (2, 10, 10, 8), -1.0, 1.0)
    ref = sl.eval_graph(b, xin)
    for opts in (dict(), dict(arena=0), dict(alias_cat=0), dict(alias_split=0)):
        e, (got,) = run_engine(b, tmp_path, xin, **opts)
        util.assert_parity(got, ref, what="chunk + cat of one conv output %r" % opts)
        alias = e.schedule()["alias"]
        if not opts or "arena" in opts:
            assert {X, y0, y1, first, p, q} <= set(alias), alias
            assert chunk_step(e)["kernel"] == "view"
    # a chunk of a chunk: views of views
    b2 = mg.PnnxBuilder(seed=8)
    x2 = b2.input((2, 8, 6, 6))
    a0, a1 = b2.chunk(mg._Conv(b2, x2, 32, 1), 2, 1)
    c0, c1 = b2.chunk(a1, 2, 1)
    b2.output(mg._Conv(b2, b2.cat([mg._Conv(b2, c1, 8, 3), mg._Conv(b2, a0, 8, 1), mg._Conv(b2, c0, 8, 1)], 1), 8, 1))
    xin2 = util.rng_uniform(16, (2, 6, 6, 8), -1.0, 1.0)
    e2, (got2,) = run_engine(b2, tmp_path, xin2, tag="m2")
    util.assert_parity(got2, sl.eval_graph(b2, xin2), what="chunk of a chunk")
    assert {a0, a1, c0, c1} <= set(e2.schedule()["alias"]), e2.schedule()
    assert [L["kernel"] for L in new_layers(e2.profile())] == ["view", "view"]


def test_a_view_keeps_its_buffer_alive(gpu, tmp_path):
    """the second half of a chunk is read eight steps after the first: with the arena on, the input's buffer must not be handed to any of
    the convs in between"""
    b = mg.PnnxBuilder(seed=9)
    x = b.input((2, 8, 12, 12))
    y0, y1 = b.chunk(mg._Conv(b, x, 32, 1), 2, 1)
    t = y0
    for _ in range(8):
        t = mg._Conv(b, t, 16, 3)
    b.output(b.conv(b.add(t, y1), 8, 1))
    xin = util.rng_uniform(17, (2, 12, 12, 8), -1.0, 1.0)
    ref = sl.eval_graph(b, xin)
    e, (got,) = run_engine(b, tmp_path, xin, arena=1)
    assert {y0, y1} <= set(e.schedule()["alias"]) and chunk_step(e)["kernel"] == "view"
    assert e.schedule()["arena_bytes"] < e.schedule()["per_operand_bytes"], "the arena shares nothing: the test shows nothing"
    util.assert_parity(got, ref, what="late reader of a view, arena on")
    _, (got0,) = run_engine(b, tmp_path, xin, arena=0)
    util.assert_exact(got.view(np.uint32), got0.view(np.uint32), "arena on vs one allocation per operand")


def test_what_is_not_aliased(gpu, tmp_path):
    # a chunk of the graph input
    b = mg.PnnxBuilder(seed=10)
    x = b.input((2, 16, 8, 8))
    y0, y1 = b.chunk(x, 2, 1)
    b.output(b.conv(b.cat([mg._Conv(b, y0, 8, 3), mg._Conv(b, y1, 8, 3)], 1), 8, 1))
    xin = util.rng_uniform(18, (2, 8, 8, 16), -1.0, 1.0)
    e, (got,) = run_engine(b, tmp_path, xin, tag="input")
    assert not {y0, y1} & set(e.schedule()["alias"]) and chunk_step(e)["kernel"] == "split_channels", e.schedule()
    util.assert_parity(got, sl.eval_graph(b, xin), what="chunk of the graph input")
    # fp16 storage, 4 channels per half: the second half starts 8 bytes into the pixel
    b = mg.PnnxBuilder(seed=11)
    x = b.input((2, 8, 8, 8))
    y0, y1 = b.chunk(mg._Conv(b, x, 8, 3), 2, 1)
    b.output(b.conv(b.cat([mg._Conv(b, y0, 8, 3), mg._Conv(b, y1, 8, 3)], 1), 8, 1))
    xin = util.rng_uniform(19, (2, 8, 8, 8), -1.0, 1.0)
    e, (got,) = run_engine(b, tmp_path, xin, tag="half", fp16=1)
    alias = e.schedule()["alias"]
    assert y0 in alias and y1 not in alias and chunk_step(e)["kernel"] == "split_channels", e.schedule()
    ref = sl.eval_graph(b, xin)
    assert util.rel_err(got, ref) <= 2.0 * util.rel_err(sl.eval_graph(b, xin, rnd=sl.round_f16), ref)
    e32, _ = run_engine(b, tmp_path, xin, tag="half")          # fp32: 16 bytes, a view
    assert {y0, y1} <= set(e32.schedule()["alias"])
    # a chunk behind a flatten whose pieces feed nn.Linear: rank 2, and Linear takes dense rows
    b = mg.PnnxBuilder(seed=12)
    x = b.input((3, 8, 6, 6))
    f = b.flatten(b.adaptive_avgpool(mg._Conv(b, x, 32, 3)))
    y0, y1 = b.chunk(f, 2, 1)
    b.output(b.linear(y0, 5))
    b.output(b.linear(y1, 7))
    xin = util.rng_uniform(20, (3, 6, 6, 8), -1.0, 1.0)
    e, got = run_engine(b, tmp_path, xin, tag="linear")
    assert not {y0, y1} & set(e.schedule()["alias"]) and chunk_step(e)["kernel"] == "split_channels", e.schedule()
    for g, r in zip(got, sl.eval_graph(b, xin)):
        util.assert_parity(g, r, what="chunk -> Linear")


def raw_graph(in_shape, typ, out_shapes, params):
    """input -> one line written as given (shapes as the file has them: NCHW) -> outputs"""
    b = mg.PnnxBuilder(seed=5)
    x = b.input(in_shape)
    ys = [b._new_operand(s) for s in out_shapes]
    b._emit(typ, "op_0", [x], ys, params)
    for y in ys:
        b.output(y)
    return b


def test_validate_refusals_leave_the_process_usable(gpu, tmp_path):
    def load(b, tag):
        pp, bp = save(b, tmp_path, tag)
        with pytest.raises(StatusError) as ei:
            Engine().load_model(pp, bp)
        return ei.value.status

    s = (2, 8, 4, 6)
    half = (2, 4, 4, 6)
    assert load(raw_graph(s, "torch.chunk", [half, half, half], dict(chunks=3, dim=1)), "count") == Status.kErrorShape       # the rule: 3 + 3 + 2
    assert load(raw_graph(s, "torch.chunk", [half, (2, 3, 4, 6)], dict(chunks=2, dim=1)), "shape") == Status.kErrorShape
    assert load(raw_graph(s, "torch.chunk", [half, half], dict(chunks=0, dim=1)), "zero") == Status.kErrorShape
    assert load(raw_graph(s, "torch.chunk", [half, half], dict(chunks=2)), "missing_key") == Status.kFail
    assert load(raw_graph(s, "torch.chunk", [half, half], dict(chunks=2, dim=4)), "dim") == Status.kUnsupport
    assert load(raw_graph((2, 8, 6), "torch.chunk", [(2, 4, 6), (2, 4, 6)], dict(chunks=2, dim=1)), "rank3") == Status.kUnsupport
    assert load(raw_graph((4, 8), "torch.chunk", [(2, 8), (2, 8)], dict(chunks=2, dim=0)), "rank2_dim0") == Status.kUnsupport
    assert load(raw_graph(s, "torch.split", [half, half], dict(dim=1, split_size_or_sections=(4, 3))), "sum") == Status.kErrorShape
    assert load(raw_graph(s, "torch.split", [half, half], dict(dim=1, split_size_or_sections=(8, 0))), "empty_section") == Status.kErrorShape
    assert load(raw_graph(s, "Tensor.slice", [half], dict(dim=1, start=6, end=2, step=1)), "empty") == Status.kErrorShape
    assert load(raw_graph(s, "Tensor.slice", [half], dict(dim=1, start=0, end=8, step=0)), "step0") == Status.kErrorShape
    assert load(raw_graph(s, "Tensor.slice", [half], dict(dim=1, start=0, end=8, step=-1)), "negative_step") == Status.kErrorShape
    assert load(raw_graph(s, "Tensor.slice", [half], dict(dim=1, start=0, end=5, step=1)), "slice_shape") == Status.kErrorShape
    assert load(raw_graph(s, "Tensor.slice", [half], dict(dims=(1, 2), starts=(0,), ends=(4, 4), steps=(1, 1))), "lists") == Status.kFail
    x = bit_patterns(3, (1, 4, 4, 8), np.float32)
    with pytest.raises(hipops.HipError):
        hipops.slice(x, ch(8, 8))                                # empty
    d = hipops.slice_desc(x.shape, ch(0, 8))
    d.oc = 9                                                     # one channel past the input
    assert _native.hip().si_hip_slice_f32(C.byref(d), 256, 256, None) == -1
    # ... and the same process loads and runs a good model afterwards
    _, got = run_engine(one_op_graph((1, 4, 4, 8), "chunk", 2, 1), tmp_path, x, tag="good")
    for g, w in zip(got, sl.chunk_ref(x, 2, 1)):
        ct.assert_same_bits(g, w, "good model after the refusals")
