"""CPU: clamp / softplus / mish (include/si_act.h) -- the numpy rule of tests/act_reference.py pinned to torch float64 on special values, a wide
sweep and all 65536 halves; the float32 emulation of the kernel's formulas under the GPU file's bars, and the naive log(1 + exp) forms
above them (the control: the bar sees the negative tail); the C-ABI (exported, bound under its own table, absent from include/si_hip.h,
every compute entry driven by the GPU file's view cases); the registry; what the entries decide without a device (every refusal by
return code, the kernel name by descriptor, strides and pointer alignment); the builder's lines and the three toy models.  (What LoadModel
refuses needs an engine, hence a device: tests/test_gpu_param_act.py.)"""
import ctypes as C
import re

import numpy as np
import pytest

import act_reference as ar
import containment as ct
import elementwise_reference as er
from ct_reference import _parse
from simpleinfer_amd import _native, engine, hipops, modelgen as mg

INF = ar.INF
ULP_BAR = 4          # the GPU file's fp32 bar for softplus and mish (er.assert_ulp32)


def _inputs():
    halves = er.all_halves().astype(np.float64)
    return {"special": er.special_f32().astype(np.float64), "sweep": er.wide_sweep("any").astype(np.float64), "halves": halves}


def _same_values(got, ref, what):
    """equal as float64 values (zeros by value: torch's sign of a zero is its vector unit's, not a rule), NaN where the other has NaN"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), what + ": NaN masks differ"
    ok = ~np.isnan(ref)
    assert np.array_equal(got[ok], ref[ok]), what


def _close_values(got, ref, what, ulps=8):
    """two float64 statements of one smooth function: NaN and infinity masks equal, the rest within a few float64 ulps (+ a denormal)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), what + ": NaN masks differ"
    inf = np.isinf(ref)
    assert np.array_equal(got[inf], ref[inf]) and not np.isinf(got[~inf & ~np.isnan(ref)]).any(), what + ": infinities differ"
    fin = np.isfinite(ref)
    bound = ulps * np.finfo(np.float64).eps * np.abs(ref[fin]) + 1e-300
    bad = np.abs(got[fin] - ref[fin]) > bound
    assert not bad.any(), "%s: %d elements differ, first %r vs %r" % (what, int(bad.sum()), got[fin][bad][0], ref[fin][bad][0])


def test_reference_equals_torch_float64():
    pytest.importorskip("torch")
    for tag, x in _inputs().items():
        for lo, hi in [(0.0, 6.0), (-1.0, 1.0), (-INF, 0.5), (0.1, INF), (-2.5, 3.0)]:     # F.relu6, F.hardtanh, torch.clamp with each bound None
            _same_values(ar.param_act_ref("clamp", x, lo, hi), ar.param_act_torch("clamp", x, lo, hi), "clamp(%g, %g) on %s" % (lo, hi, tag))
        import torch
        t = torch.from_numpy(x)
        _same_values(ar.param_act_ref("clamp", x, 0.0, 6.0), torch.nn.functional.relu6(t).numpy(), "F.relu6 on " + tag)
        _same_values(ar.param_act_ref("clamp", x, -1.0, 1.0), torch.nn.functional.hardtanh(t).numpy(), "F.hardtanh on " + tag)
        for beta in (1.0, 0.5, 2.0):
            for threshold in (20.0, 5.0):
                _close_values(ar.param_act_ref("softplus", x, beta, threshold), ar.param_act_torch("softplus", x, beta, threshold),
                              "softplus(beta %g, threshold %g) on %s" % (beta, threshold, tag))
        _close_values(ar.param_act_ref("mish", x), ar.param_act_torch("mish", x), "mish on " + tag)


def test_reference_special_values_and_signs_of_zero():
    f = lambda op, v, *p: ar.param_act_ref(op, np.array([v], np.float64), *p)[0]
    assert np.isnan(f("clamp", np.nan, 0, 6)) and np.isnan(f("softplus", np.nan, 1, 20)) and np.isnan(f("mish", np.nan))
    assert f("softplus", -INF, 1, 20) == 0 and f("softplus", INF, 1, 20) == INF and f("mish", INF) == INF and np.isnan(f("mish", -INF))
    z = f("clamp", -0.0, 0.0, 6.0)
    assert z == 0 and np.signbit(z)                                   # -0.0 is not below the bound 0: it stays
    assert f("clamp", 7.0, 2.0, -2.0) == -2.0 and f("clamp", -7.0, 2.0, -2.0) == -2.0 and f("clamp", 0.0, 2.0, -2.0) == -2.0    # lo > hi: hi everywhere
    assert not np.signbit(f("clamp", -1.0, 0.0, 6.0)) and np.signbit(f("clamp", -1.0, -0.0, 0.0))
    assert f("clamp", -INF, -INF, 0.5) == -INF and f("clamp", INF, 0.1, INF) == INF


def test_the_bars_can_be_met_and_see_the_tail():
    """the kernel's formulas in numpy float32 stay under the fp32 bar; log(1 + exp) does not (it returns 0 where the value is e^z).  Rounded
    to half, the float32 formulas differ from the float64 reference rounded once on a handful of the 65536 inputs."""
    x = ar.fp32_inputs()
    worst = {}
    for beta, threshold in ar.SOFTPLUS_PARAMS:
        ref = ar.param_act_ref("softplus", x, beta, threshold)
        w, _ = er.assert_ulp32(ar.softplus_f32(x, beta, threshold), ref, ULP_BAR, "softplus emulation", band=True)
        worst["softplus"] = max(worst.get("softplus", 0.0), w)
        with pytest.raises(AssertionError):
            er.assert_ulp32(ar.softplus_f32(x, beta, threshold, naive=True), ref, ULP_BAR, "naive softplus", band=True)
    ref = ar.param_act_ref("mish", x)
    worst["mish"], _ = er.assert_ulp32(ar.mish_f32(x), ref, ULP_BAR, "mish emulation", band=True)
    with pytest.raises(AssertionError):
        er.assert_ulp32(ar.mish_f32(x, naive=True), ref, ULP_BAR, "naive mish", band=True)
    print("float32 emulation, worst ulp: softplus %.2f, mish %.2f" % (worst["softplus"], worst["mish"]))
    assert worst["softplus"] <= 3.0 and worst["mish"] <= 3.0       # measured 2.04 / 2.56 with numpy's primitives: room for 1-ulp device functions
    # the naive forms are 100 % off in the tail
    tail = x[(x < -20) & (x > -80)]
    assert (ar.softplus_f32(tail, naive=True) == 0).all() and (ar.param_act_ref("softplus", tail, 1, 20) > 0).all()
    h = er.all_halves()
    n_sp, w_sp = er.assert_half(ar.softplus_f32(h.astype(np.float32)).astype(np.float16), ar.param_act_ref("softplus", h, 1, 20), 1, "softplus halves")
    n_mi, w_mi = er.assert_half(ar.mish_f32(h.astype(np.float32)).astype(np.float16), ar.param_act_ref("mish", h), 1, "mish halves")
    print("rounded to half: softplus differs on %d inputs, mish on %d" % (n_sp, n_mi))
    assert n_sp <= 4 and n_mi <= 4
    for lo, hi in ar.CLAMP_BOUNDS:
        er.assert_bits32(ar.clamp_f32(x, lo, hi), ar.param_act_ref("clamp", x, lo, hi), "clamp(%g, %g) emulation" % (lo, hi))


def _declared(path):
    src = open(path).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    names = []
    for m in re.finditer(r"\b(si_[a-z0-9_]+)\s*\(", src):
        if m.group(1) not in names:
            names.append(m.group(1))
    return names


def test_act_header_is_exported_and_bound(native_libs):
    H, _ = native_libs
    declared = _declared(ar.HEADER)
    assert declared == ["si_hip_param_act_f32", "si_hip_param_act_f16", "si_hip_param_act_kernel_name"]
    assert sorted(H._si_act_signatures) == sorted(declared)
    others = [v for k, v in vars(H).items() if re.fullmatch(r"_si_[a-z_]*signatures", k) and k != "_si_act_signatures"]
    assert len(others) >= 8
    for other in others:
        assert not set(declared) & set(other)
    raw = C.CDLL(_native.LIB_HIP_PATH)   # a handle of its own: nothing but the dynamic symbol table answers
    missing = [name for name in declared if not hasattr(raw, name)]
    assert not missing, missing
    # the Python structure has the header's fields in the header's order, and their C types
    text = open(ar.HEADER).read()
    m = re.search(r"typedef struct SiParamActDesc \{(.*?)\} SiParamActDesc;", text, flags=re.S)
    body = re.sub(r"/\*.*?\*/", " ", m.group(1), flags=re.S)
    fields = [(decl.strip().split(None, 1)[0], f.strip()) for decl in body.split(";") if decl.strip() for f in decl.strip().split(None, 1)[1].split(",")]
    ctype = {"int": C.c_int, "float": C.c_float, "size_t": C.c_size_t}
    assert [(ctype[t], n) for t, n in fields] == [(t, n) for n, t in _native.SiParamActDesc._fields_], fields
    enum = lambda name: int(re.search(r"\b%s\s*=\s*(-?\d+)" % name, text).group(1))
    assert [enum("SI_PACT_" + k.upper()) for k in ar.OPS] == [hipops.PARAM_ACT_OPS[k] for k in ar.OPS] == [ar.OP_CODE[k] for k in ar.OPS] == [0, 1, 2]
    assert enum("SI_PACT_MISH_CUT") == ar.MISH_CUT


def test_si_hip_header_declares_none_of_them():
    text = open(ct.HEADER).read()
    for name in _declared(ar.HEADER):
        assert name not in text, name
    assert "SiParamActDesc" not in text and "si_hip_param_act" not in text


def test_registry_lists_the_new_type_strings(native_libs):
    types = engine.registry_types()
    for t in ar.PARAM_TYPES + tuple(ar.FUNCTIONAL_TWINS):
        assert t in types, t
    assert len(ar.PARAM_TYPES) == 9 and len(ar.FUNCTIONAL_TWINS) == 7
    for t in ("nn.GELU", "nn.ELU", "nn.ChannelShuffle", "nn.Dropout", "nn.Softmin", "F.softmin", "nn.AdaptiveMaxPool2d", "torch.max", "torch.argmax",
              "torch.prod", "torch.tensor_split", "torch.unbind", "Tensor.select", "Tensor.narrow", "Tensor.clamp_"):
        assert t not in types, t


def test_every_compute_entry_of_the_act_header_is_driven():
    """the rule of tests/test_containment_cpu.py for include/si_hip.h, applied to include/si_act.h and the view cases of the GPU file"""
    import test_gpu_param_act as tp
    entries = [n for n in ct.header_functions(ar.HEADER) if not ct.is_exempt(n)]
    assert entries == ["si_hip_param_act_f32", "si_hip_param_act_f16"]
    driven = {e for c in tp.VIEW_CASES for e in c.entries}
    assert set(entries) <= driven, sorted(set(entries) - driven)
    assert driven <= set(ct.header_functions(ar.HEADER)), "a case names an entry the header does not declare"


BADARG, UNSUPPORTED = -1, -2


def test_abi_without_a_device(native_libs):
    """refusals happen before any device call (the pointers are compared, never followed)"""
    H, _ = native_libs
    src, dst = C.c_void_p(1 << 20), C.c_void_p(1 << 40)
    shape = (2, 5, 7, 8)
    desc = hipops.param_act_desc
    nan = float("nan")
    for fn in ("si_hip_param_act_f32", "si_hip_param_act_f16"):
        esize = 4 if fn.endswith("f32") else 2

        def call(d, a=src, b=dst):
            return getattr(H, fn)(C.byref(d), a, b, None)

        assert getattr(H, fn)(None, src, dst, None) == BADARG               # null descriptor
        assert call(desc(shape, "clamp", 0, 6), a=None) == BADARG           # null pointers
        assert call(desc(shape, "mish"), b=None) == BADARG
        for field, values in (("pixels", (0,)), ("c", (0, -1)), ("in_ld", (0, -8)), ("out_ld", (0, -8))):   # zero or negative sizes
            for value in values:
                bad = desc(shape, "clamp", 0, 6)
                setattr(bad, field, value)
                assert call(bad) == BADARG, (field, value)
        assert call(desc(shape, "clamp", 0, 6, in_ld=7)) == BADARG          # ld < c
        assert call(desc(shape, "clamp", 0, 6, out_ld=7)) == BADARG
        for op in (-1, 3):                                                  # op outside 0 .. 2
            assert call(desc(shape, op)) == BADARG, op
        assert call(desc(shape, "clamp", nan, 6)) == BADARG and call(desc(shape, "clamp", 0, nan)) == BADARG      # a NaN bound
        for beta in (0.0, -0.0, INF, -INF, nan):                            # beta zero or non-finite
            assert call(desc(shape, "softplus", beta, 20)) == BADARG, beta
        assert call(desc(shape, "softplus", 1, nan)) == BADARG              # a NaN threshold
        # overlapping in / out: the same pointer, an output inside the input, windows of one pixel grid that meet, strides that differ
        assert call(desc(shape, "mish"), a=src, b=src) == BADARG
        assert call(desc(shape, "mish"), a=src, b=C.c_void_p(src.value + 5 * esize)) == BADARG
        assert call(desc(shape, "mish", in_ld=16, out_ld=16), a=src, b=C.c_void_p(src.value + 4 * esize)) == BADARG   # channels 4 .. 11 meet 0 .. 7
        assert call(desc(shape, "mish", in_ld=8, out_ld=16), a=C.c_void_p(src.value + 8 * esize), b=src) == BADARG    # strides differ: the spans decide
        assert call(desc((1 << 20, 8), "mish", out_ld=1 << 11)) == UNSUPPORTED      # element offsets of 2^31, on the output side alone
        assert call(desc((1 << 28, 8), "clamp", 0, 6)) == UNSUPPORTED
        assert call(desc((1 << 32, 1), "clamp", 0, 6)) == UNSUPPORTED               # 2^32 pixels


def test_what_is_accepted_is_named(native_libs):
    """the other side of the refusals, by the name query (which runs the same check and launches nothing): infinite clamp bounds, lo > hi,
    a negative beta, an infinite threshold, any p0 / p1 for mish, and two channel slices of one buffer that do not meet"""
    name = hipops.param_act_kernel_name
    shape = (2, 5, 7, 8)
    for p in ((-INF, INF), (2.0, -2.0), (-INF, 0.5), (0.1, INF)):
        assert name(shape, "clamp", *p) == ar.kname("clamp", np.float32, True), p
    for p in ((-1.0, 20.0), (1.0, INF), (1.0, -INF), (1e-30, 20.0)):
        assert name(shape, "softplus", *p) == ar.kname("softplus", np.float32, True), p
    assert name(shape, "mish", float("nan"), float("nan")) == ar.kname("mish", np.float32, True)
    assert name((1 << 27, 8), "mish") == ar.kname("mish", np.float32, True) and name((1 << 28, 8), "mish") == "none"


def test_kernel_name_follows_the_descriptor_the_strides_and_the_pointers(native_libs):
    H, _ = native_libs
    name, K = hipops.param_act_kernel_name, ar.kname
    f32, f16 = np.float32, np.float16
    for op, p in (("clamp", (0, 6)), ("softplus", (1, 20)), ("mish", (0, 0))):
        assert name((2, 5, 7, 8), op, *p) == K(op, f32, True) and name((2, 5, 7, 8), op, *p, half=True) == K(op, f16, True)
        assert name((1, 1, 9, 7), op, *p) == K(op, f32, False) and name((1, 1, 9, 7), op, *p, half=True) == K(op, f16, False)   # 63 elements
    # the dense arm: an odd c still takes the vectors when the whole tensor fills them
    assert name((2, 5, 8, 7), "mish") == K("mish", f32, True) and name((2, 5, 8, 7), "mish", half=True) == K("mish", f16, True)      # 560 elements
    assert name((1, 5, 4, 7), "mish") == K("mish", f32, True) and name((1, 5, 4, 7), "mish", half=True) == K("mish", f16, False)     # 140: 4 | 140, 8 does not
    assert name((2, 5, 7, 12), "mish", half=True) == K("mish", f16, True)            # 840 elements, c % 8 != 0: dense
    # inside strided rows: c and both strides
    assert name((2, 5, 7, 8), "clamp", 0, 6, in_ld=16, out_ld=24) == K("clamp", f32, True)
    assert name((2, 5, 7, 8), "clamp", 0, 6, in_ld=16, out_ld=16, half=True) == K("clamp", f16, True)
    assert name((2, 5, 7, 8), "clamp", 0, 6, in_ld=9) == K("clamp", f32, False)      # a stride that is no multiple of the vector
    assert name((2, 5, 7, 8), "clamp", 0, 6, out_ld=10) == K("clamp", f32, False)
    assert name((2, 5, 7, 12), "clamp", 0, 6, in_ld=16, out_ld=16, half=True) == K("clamp", f16, False)   # c % 8 != 0 in rows
    assert name((2, 5, 8, 7), "clamp", 0, 6, in_ld=8) == K("clamp", f32, False)      # odd c in rows
    # the pointers' alignment, either side
    d = hipops.param_act_desc((2, 5, 7, 8), "clamp", 0, 6)
    q = lambda a, b, half: H.si_hip_param_act_kernel_name(C.byref(d), C.c_void_p(a), C.c_void_p(b), half).decode()
    assert q(256, 512, 0) == K("clamp", f32, True) and q(260, 512, 0) == K("clamp", f32, False) and q(256, 520, 0) == K("clamp", f32, False)
    assert q(256, 512, 1) == K("clamp", f16, True) and q(264, 512, 1) == K("clamp", f16, False) and q(256, 514, 1) == K("clamp", f16, False)
    # refused descriptors
    assert name((2, 5, 7, 8), 3) == "none" and name((2, 5, 7, 8), "clamp", 0, 6, in_ld=7) == "none" and name((2, 5, 7, 8), "softplus", 0, 20) == "none"
    assert name((2, 5, 7, 8), "clamp", float("nan"), 1) == "none"
    assert H.si_hip_param_act_kernel_name(None, C.c_void_p(256), C.c_void_p(256), 0) == b"none"
    # the reference's rule is the library's, on the whole case table of the GPU file
    import test_gpu_param_act as tp
    for c in tp.VIEW_CASES:
        views = {k: v for k, v in c.views.items() if k in ("in_ld", "out_ld")}
        if c.views.get("in_c_off", 0) % (16 // np.dtype(c.dtype).itemsize) == 0 and c.views.get("out_c_off", 0) % (16 // np.dtype(c.dtype).itemsize) == 0:
            assert name(c.shape, c.op, *c.params, half=c.half, **views) == K(c.op, c.dtype, c.vec), c.id
        assert ar.vectorised(c.shape, c.dtype, **c.views) == c.vec, c.id


# ---- the builder ---------------------------------------------------------------------------------------------------------------------------
def test_builder_emits_pnnx_keys():
    b = mg.PnnxBuilder(seed=1)
    x = b.input((2, 6, 5, 7))
    outs = [b.relu6(x), b.relu6(x, functional=True), b.hardtanh(x), b.hardtanh(x, -2.0, 0.5, functional=True), b.clamp(x, 0.0, 1.0), b.clamp(x, min=0.1),
            b.clamp(x, max=3.0), b.softplus(x), b.softplus(x, 0.5, 5.0, functional=True), b.mish(x), b.mish(x, functional=True)]
    parsed = [_parse(ln) for ln in b.lines[1:]]
    assert [p[0] for p in parsed] == ["nn.ReLU6", "F.relu6", "nn.Hardtanh", "F.hardtanh", "torch.clamp", "torch.clamp", "torch.clamp", "nn.Softplus",
                                      "F.softplus", "nn.Mish", "F.mish"]
    assert parsed[0][4] == parsed[1][4] == parsed[9][4] == parsed[10][4] == {}
    num = lambda p, k: float(p[4][k])
    assert (num(parsed[2], "min_val"), num(parsed[2], "max_val")) == (-1.0, 1.0) and (num(parsed[3], "min_val"), num(parsed[3], "max_val")) == (-2.0, 0.5)
    assert (num(parsed[4], "min"), num(parsed[4], "max")) == (0.0, 1.0)
    assert parsed[5][4]["max"] == "None" and abs(num(parsed[5], "min") - 0.1) < 1e-7 and parsed[6][4]["min"] == "None" and num(parsed[6], "max") == 3.0
    assert (num(parsed[7], "beta"), num(parsed[7], "threshold")) == (1.0, 20.0) and (num(parsed[8], "beta"), num(parsed[8], "threshold")) == (0.5, 5.0)
    assert all(b.shapes[o] == (2, 6, 5, 7) for o in outs) and not b.attrs
    assert [ar.act_of_line(p[0], p[4])[0] for p in parsed] == ["clamp"] * 7 + ["softplus"] * 2 + ["mish"] * 2


def test_existing_activation_methods_keep_their_default_output():
    """functional= is new on the existing methods: without it they write the lines they always wrote (pinned here by text, and by the hash
    of a builder's whole output in tests/test_groupnorm_cpu.py); with it the F.* spelling and the same keys"""
    b = mg.PnnxBuilder(seed=1)
    x = b.input((2, 6, 5, 7))
    for method in ("silu", "relu", "sigmoid", "hardsigmoid", "hardswish", "tanh"):
        getattr(b, method)(x)
    b.leaky_relu(x, 0.1)
    want = ["nn.SiLU silu_0", "nn.ReLU relu_0", "nn.Sigmoid sigmoid_0", "nn.Hardsigmoid hsigmoid_0", "nn.Hardswish hswish_0", "nn.Tanh tanh_0",
            "nn.LeakyReLU leakyrelu_0"]
    assert [" ".join(ln.split()[:2]) for ln in b.lines[1:]] == want
    assert b.lines[-1].split()[6] == "negative_slope=1.000000e-01" and all(len(ln.split()) == 8 for ln in b.lines[1:-1])
    f = mg.PnnxBuilder(seed=1)
    x = f.input((2, 6, 5, 7))
    for method in ("relu", "silu", "sigmoid", "hardsigmoid", "hardswish"):
        getattr(f, method)(x, functional=True)
    f.leaky_relu(x, 0.1, functional=True)
    f.tanh(x, functional=True)
    assert [ln.split()[0] for ln in f.lines[1:]] == list(ar.FUNCTIONAL_TWINS)
    assert f.lines[-2].split()[6] == "negative_slope=1.000000e-01"
    # a whole model of the existing builders is the text it was
    text = "\n".join(mg.build_toy_classifier().lines)
    assert "F." not in text and text.count("nn.Hardswish") == 1 and text.count("nn.ReLU ") == 2 and text.count("nn.Hardsigmoid") == 1


TOYS = {
    # builder, the activation lines in file order, the output's shape in the file
    "mobilenetv2": (mg.build_toy_mobilenetv2, ["nn.ReLU6"] * 7, (2, 10)),
    "csp_mish": (mg.build_toy_csp_mish, ["nn.Mish"] * 7, (2, 16, 8, 8)),
    "clamp_head": (mg.build_toy_clamp_head, ["nn.Softplus", "torch.clamp"], (2, 8, 16, 16)),
}


@pytest.mark.parametrize("toy", sorted(TOYS))
def test_toy_builders(toy):
    pytest.importorskip("torch")
    build, acts, oshape = TOYS[toy]
    b = build()
    parsed = [_parse(ln) for ln in b.lines]
    types = [p[0] for p in parsed]
    assert [t for t in types if t in ar.PARAM_TYPES] == acts
    assert types[0] == "pnnx.Input" and types[-1] == "pnnx.Output" and b.shapes[parsed[-1][2][0]] == oshape
    if toy == "mobilenetv2":
        assert types.count("nn.Conv2d") == 10 and types.count("pnnx.Expression") == 2 and types[-2] == "nn.Linear"     # two of three blocks add
        depthwise = [p for p in parsed if p[0] == "nn.Conv2d" and int(p[4]["groups"]) > 1]
        assert len(depthwise) == 3 and all(p[4]["groups"] == p[4]["in_channels"] == p[4]["out_channels"] for p in depthwise)
        fb = mg.build_toy_mobilenetv2(functional=True)
        assert [_parse(ln)[0] for ln in fb.lines].count("F.relu6") == 7
    if toy == "csp_mish":
        assert types.count("nn.Conv2d") == 7 and types.count("torch.cat") == 1
        for i, t in enumerate(types):
            if t == "nn.Conv2d":
                assert types[i + 1] == "nn.Mish", (i, types)
    if toy == "clamp_head":
        assert types[1:4] == ["nn.Conv2d", "nn.Softplus", "torch.clamp"]
        assert parsed[3][4]["max"] == "None" and abs(float(parsed[3][4]["min"]) - 0.1) < 1e-7
    n, c, h, w = b.shapes["0"]
    x = mg.synth_input((n, h, w, c))
    y = ar.eval_graph(b, x)
    assert y.shape == (oshape if len(oshape) == 2 else (oshape[0], oshape[2], oshape[3], oshape[1])) and np.isfinite(y).all() and np.abs(y).max() > 1e-3
    e = ar.eval_graph(b, x, rnd=ar.round_f16)
    assert np.isfinite(e).all() and np.abs(e - y).max() / np.abs(y).max() < 2e-2     # the fp16-storage emulation stays near the exact evaluation
    if toy == "clamp_head":
        assert y.min() >= float(np.float32(0.1)) and (y > 0.2).any()
    if toy == "mobilenetv2":      # ReLU6 does something on this input: both bounds are reached in front of some activation
        cut = mg.build_toy_mobilenetv2()
        first = _parse(cut.lines[1])[3][0]
        cut.lines = cut.lines[:2] + ["pnnx.Output out 1 0 %s" % first]
        z = ar.eval_graph(cut, x)
        assert (z < 0).any() and (z > 0).any()
