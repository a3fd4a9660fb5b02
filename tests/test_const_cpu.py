"""CPU: graph constants and the constant-operand kernel's host side -- the builder's pnnx.Attribute lines and the five toys' operator sequences;
the float64 evaluation of tests/const_reference.py pinned to a torch float64 restatement; the numpy restatement of the kernel against
float64 arithmetic rounded once; the loader / writer round trip (Graph::save keeps attributes with their bytes, the re-batching rewrite
leaves them alone); the C-ABI of include/si_binary.h (exported, bound under its own table, absent from include/si_hip.h, the structure's
fields, every compute entry driven by a view case of the GPU file); every refusal by return code, without a launch; and two stand-alone C++
programs under AddressSanitizer and UBSan: the plan arithmetic (tests/cpp/test_binary_plan.cpp over csrc/hip/binary_plan.h) and the batch
rule for constants (tests/cpp/test_batch_rule_const.cpp)."""
import ctypes as C
import os
import re
import subprocess
import zipfile

import numpy as np
import pytest

import const_reference as cr
import containment as ct
from ct_reference import _ints, _parse
from simpleinfer_amd import _native, engine, hipops, modelgen as mg

BADARG, UNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def native_libs():
    try:
        return _native.hip(), _native.host()
    except _native.NativeLibraryMissing as e:   # build() has not run
        pytest.fail(str(e))


TOYS = [(mg.build_toy_frozenbn_block, {}), (mg.build_toy_layer_scale, {}), (mg.build_toy_flow_warp_const, {}), (mg.build_toy_pos_embed, {}),
        (mg.build_toy_pos_embed, dict(batch_first=True)), (mg.build_toy_fcos_scale, {})]


def toy_input(b):
    n, c, h, w = b.shapes["0"]
    return mg.synth_input((n, h, w, c))


def _types(b):
    return [ln.split()[0] for ln in b.lines]


# ---- the builder ------------------------------------------------------------------------------------------------------------------------
def test_attribute_lines():
    b = mg.PnnxBuilder(seed=1)
    x = b.input((2, 8, 5, 6))
    c = b.attribute(np.arange(8, dtype=np.float32).reshape(1, 8, 1, 1))
    g = b.attribute(np.ones((8, 1, 1)), name="gamma")
    assert b.lines[1] == "pnnx.Attribute pnnx_attr_0 0 1 %s @data=(1,8,1,1)f32 #%s=(1,8,1,1)f32" % (c, c)
    assert b.lines[2] == "pnnx.Attribute gamma 0 1 %s @data=(8,1,1)f32 #%s=(8,1,1)f32" % (g, g)
    assert b.shapes[c] == (1, 8, 1, 1) and b.shapes[g] == (8, 1, 1)
    assert b.attrs["pnnx_attr_0.data"].dtype == np.float32 and np.array_equal(b.attrs["pnnx_attr_0.data"].reshape(-1), np.arange(8))
    assert b.attrs["gamma.data"].dtype == np.float32      # (a float64 array is stored as fp32)
    assert x == "0" and (c, g) == ("1", "2")


def test_toy_operator_sequences():
    b = mg.build_toy_frozenbn_block()
    assert _types(b) == ["pnnx.Input", "nn.Conv2d", "nn.ReLU", "nn.Conv2d", "pnnx.Attribute", "pnnx.Attribute", "pnnx.Expression", "nn.ReLU", "nn.Conv2d",
                         "pnnx.Attribute", "pnnx.Attribute", "pnnx.Expression", "pnnx.Expression", "nn.ReLU", "pnnx.Output"]
    assert [_parse(ln)[4]["expr"] for ln in b.lines if ln.startswith("pnnx.Expression")] == ["add(mul(@0,@1),@2)"] * 2 + ["add(@0,@1)"]
    assert {b.shapes[_parse(ln)[3][0]] for ln in b.lines if ln.startswith("pnnx.Attribute")} == {(1, 16, 1, 1)}
    b = mg.build_toy_layer_scale()
    (attr,) = [_parse(ln) for ln in b.lines if ln.startswith("pnnx.Attribute")]
    assert b.shapes[attr[3][0]] == (24, 1, 1)
    (expr,) = [_parse(ln) for ln in b.lines if ln.startswith("pnnx.Expression") and "mul" in ln]
    assert expr[2][0] == attr[3][0] and len(b.shapes[expr[2][1]]) == 4      # the constant on the left, rank 3 against rank 4
    b = mg.build_toy_flow_warp_const()
    assert _types(b).count("pnnx.Input") == 1 and mg.build_toy_flow_warp.__call__()._n_operand == b._n_operand
    (attr,) = [_parse(ln) for ln in b.lines if ln.startswith("pnnx.Attribute")]
    assert b.shapes[attr[3][0]] == (1, 2, 24, 20)
    assert np.array_equal(b.attrs[attr[1] + ".data"].transpose(0, 2, 3, 1), mg.flow_base_grid(1, 24, 20))
    for batch_first, shape in ((False, (16, 1, 32)), (True, (1, 16, 32))):
        b = mg.build_toy_pos_embed(batch_first=batch_first)
        (attr,) = [_parse(ln) for ln in b.lines if ln.startswith("pnnx.Attribute")]
        assert b.shapes[attr[3][0]] == shape and "nn.MultiheadAttention" in _types(b)
    b = mg.build_toy_fcos_scale()
    assert _types(b).count("pnnx.Attribute") == 2 == _types(b).count("pnnx.Output")
    assert {b.shapes[_parse(ln)[3][0]] for ln in b.lines if ln.startswith("pnnx.Attribute")} == {(1,)}
    assert [_parse(ln)[4]["expr"] for ln in b.lines if ln.startswith("pnnx.Expression")] == ["exp(mul(@0,@1))"] * 2


# ---- the float64 evaluation against torch ------------------------------------------------------------------------------------------------
def eval_graph_torch(builder, x_nhwc):
    """the toys restated with torch's own float64 modules and functions, operator by operator"""
    import torch
    F = torch.nn.functional
    t64 = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64)))
    vals, results = {}, []
    for typ, name, ins, outs, prm in (_parse(ln) for ln in builder.lines):
        a = lambda k: t64(builder.attrs["%s.%s" % (name, k)])
        if typ == "pnnx.Input":
            vals[outs[0]] = t64(x_nhwc).permute(0, 3, 1, 2)
            continue
        if typ == "pnnx.Attribute":
            vals[outs[0]] = a("data")
            continue
        if typ == "pnnx.Output":
            r = vals[ins[0]]
            results.append(np.ascontiguousarray((r.permute(0, 2, 3, 1) if r.ndim == 4 else r).numpy()))
            continue
        x = vals[ins[0]]
        if typ == "nn.Conv2d":
            y = F.conv2d(x, a("weight"), a("bias") if prm["bias"] == "True" else None, _ints(prm["stride"]), _ints(prm["padding"]), _ints(prm["dilation"]),
                         int(prm["groups"]))
        elif typ == "nn.ReLU":
            y = F.relu(x)
        elif typ == "nn.SiLU":
            y = F.silu(x)
        elif typ == "nn.Tanh":
            y = torch.tanh(x)
        elif typ == "torch.flatten":
            y = torch.flatten(x, int(prm["start_dim"]))
        elif typ == "Tensor.permute":
            y = x.permute(*_ints(prm["dims"]))
        elif typ == "nn.Linear":
            y = F.linear(x, a("weight"), a("bias") if prm["bias"] == "True" else None)
        elif typ == "pnnx.Expression":
            v = [vals[i] for i in ins]
            y = {"add(mul(@0,@1),@2)": lambda: torch.add(torch.mul(v[0], v[1]), v[2]), "add(@0,@1)": lambda: torch.add(v[0], v[1]),
                 "mul(@0,@1)": lambda: torch.mul(v[0], v[1]), "exp(mul(@0,@1))": lambda: torch.exp(torch.mul(v[0], v[1]))}[prm["expr"]]()
        elif typ == "nn.MultiheadAttention":
            m = torch.nn.MultiheadAttention(int(prm["embed_dim"]), int(prm["num_heads"]), bias=True, batch_first=prm["batch_first"] == "True", dtype=torch.float64).eval()
            with torch.no_grad():
                m.in_proj_weight.copy_(a("in_proj_weight")); m.in_proj_bias.copy_(a("in_proj_bias"))
                m.out_proj.weight.copy_(a("out_proj.weight")); m.out_proj.bias.copy_(a("out_proj.bias"))
                y = m(x, x, x, need_weights=False)[0]
        elif typ == "F.grid_sample":
            y = F.grid_sample(x, vals[ins[1]], mode=prm["mode"], padding_mode=prm["padding_mode"], align_corners=prm["align_corners"] == "True")
        else:
            raise NotImplementedError(typ)
        assert tuple(y.shape) == tuple(builder.shapes[outs[0]]), (typ, name, tuple(y.shape))
        vals[outs[0]] = y
    return results[0] if len(results) == 1 else results


@pytest.mark.parametrize("toy", range(len(TOYS)), ids=[f.__name__ + ("_bf" if kw else "") for f, kw in TOYS])
def test_float64_evaluation_against_torch(toy):
    build, kw = TOYS[toy]
    b = build(**kw)
    x = toy_input(b)
    got, want = cr.eval_graph(b, x), eval_graph_torch(b, x)
    got, want = (v if isinstance(v, list) else [v] for v in (got, want))
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.shape == w.shape and g.dtype == np.float64
        err = float(np.abs(g - w).max() / max(np.abs(w).max(), 1e-30))
        assert err <= 1e-12, (build.__name__, err)
    # the constants matter: without them the result is another one
    if build is mg.build_toy_layer_scale:
        b.attrs["pnnx_attr_0.data"] = b.attrs["pnnx_attr_0.data"] * 2
        assert np.abs(cr.eval_graph(b, x) - got[0]).max() > 1e-3


def test_eval_expr():
    a, c = np.arange(6, dtype=np.float64).reshape(1, 2, 3, 1) + 1, np.asarray([2.0, 4.0]).reshape(2, 1, 1)
    assert np.array_equal(cr.eval_expr("add(mul(@0,@1),@2)", [a, c, c]), a * c + c)
    assert np.array_equal(cr.eval_expr("sub(@1,div(@0,2.0))", [a, c]), c - a / 2.0)
    assert np.array_equal(cr.eval_expr("exp(neg(@0))", [a]), np.exp(-a))


# ---- the kernel's restatement ------------------------------------------------------------------------------------------------------------
def test_kernel_restatement_rounds_once_per_stage():
    r = np.random.Generator(np.random.Philox(5))
    x32 = (r.random((2, 3, 5, 8)) * 8 - 4).astype(np.float32)
    c32, k32 = (r.random((1, 1, 1, 8)) * 2 + 0.5).astype(np.float32), (r.random((1, 3, 1, 1)) * 2 - 1).astype(np.float32)
    # fp32: every IEEE code is the float64 operation rounded once (24-bit operands: the float64 result of + - * is exact, / is correctly rounded twice
    # without a double-rounding case at 53 >= 2 * 24 + 2 bits)
    for op in cr.EXACT_OPS:
        want = cr.stage_f32(op, x32.astype(np.float64), c32.astype(np.float64))
        assert np.array_equal(cr.kernel_ref(x32, [op], [c32]), np.asarray(want, np.float64).astype(np.float32)), op
    # two stages are two one-stage calls, in both types
    for dt in (np.float32, np.float16):
        x, c, k = x32.astype(dt), c32.astype(dt), k32.astype(dt)
        for ops in ((2, 0), (3, 7), (8, 1)):
            two = cr.kernel_ref(x, ops, [c, k])
            assert two.dtype == dt and np.array_equal(two, cr.kernel_ref(cr.kernel_ref(x, ops[:1], [c]), ops[1:], [k])), (dt, ops)
    # fp16: the intermediate is a half -- 65504 + 16 overflows before the subtraction brings it back
    top, s16 = np.full((1, 1, 1, 1), 65504, np.float16), np.full((1, 1, 1, 1), 16, np.float16)
    assert np.isinf(cr.kernel_ref(top, [0, 1], [s16, s16])).all() and cr.kernel_ref(top.astype(np.float32), [0, 1], [s16.astype(np.float32)] * 2)[0, 0, 0, 0] == 65504
    assert cr.kernel_ref(top, [0], [np.full((1, 1, 1, 1), 15, np.float16)])[0, 0, 0, 0] == 65504
    # the reversed codes are the codes with the operands exchanged
    for op in cr.OPS:
        assert np.array_equal(cr.stage_f32(cr.REVERSED[op], x32, c32), cr.stage_f32(op, np.broadcast_to(c32, x32.shape), x32), equal_nan=True), op
    assert cr.expected_form((2, 3, 5, 8), [(1, 1, 1, 8)]) == "chan" and cr.expected_form((2, 3, 5, 8), [(1, 3, 5, 1)]) == "pixel"
    assert cr.expected_form((2, 3, 5, 8), [(1, 1, 1, 8), (2, 1, 1, 1)]) == "full" and cr.expected_form((2, 3, 5, 8), [(1, 1, 1, 1)]) == "chan"
    assert len(cr.MASKS) == 16 and cr.const_shape((2, 3, 5, 8), (0, 1, 0, 1)) == (1, 3, 1, 8)


# ---- loader and writer -------------------------------------------------------------------------------------------------------------------
def _dump(tmp_path, pp, bp, tag, expand=False):
    out = str(tmp_path / (tag + ".dump"))
    engine.pnnx_dump(pp, bp, expand, out)
    return open(out).read()


def test_loader_round_trip_and_rebatch(native_libs, tmp_path):
    b = mg.build_toy_frozenbn_block()
    pp, bp = str(tmp_path / "m.pnnx.param"), str(tmp_path / "m.pnnx.bin")
    b.save(pp, bp)
    first = _dump(tmp_path, pp, bp, "first")
    assert first.count("op pnnx.Attribute ") == 4 and first.count("attr data type=1 shape=1,16,1,1, bytes=64") == 4
    # Graph::save keeps the attributes with their bytes: the dump of the rewritten pair (checksums of the data included) is the first one
    pp2, bp2 = str(tmp_path / "r.pnnx.param"), str(tmp_path / "r.pnnx.bin")
    engine.pnnx_save(pp, bp, pp2, bp2)
    assert _dump(tmp_path, pp2, bp2, "second") == first
    with zipfile.ZipFile(bp2) as z:
        assert z.read("pnnx_attr_0.data") == b.attrs["pnnx_attr_0.data"].astype("<f4").tobytes()
    # with the expressions lowered: BinaryOps that read the attributes' operands
    lowered = _dump(tmp_path, pp, bp, "lowered", expand=True)
    assert lowered.count("op BinaryOp ") == 5 and "pnnx.Expression" not in lowered and lowered.count("op pnnx.Attribute ") == 4
    # the re-batching rewrite: every operand follows but the constants, whose shapes and bytes stay
    pp4, bp4 = str(tmp_path / "b4.pnnx.param"), str(tmp_path / "b4.pnnx.bin")
    engine.pnnx_save(pp, bp, pp4, bp4, batch=4)
    want = mg.build_toy_frozenbn_block(batch=4)
    ppw, bpw = str(tmp_path / "w.pnnx.param"), str(tmp_path / "w.pnnx.bin")
    want.save(ppw, bpw)
    assert _dump(tmp_path, pp4, bp4, "rebatched") == _dump(tmp_path, ppw, bpw, "built_at_4")
    # ... also a constant whose dimension 0 equals the traced batch
    b = mg.PnnxBuilder(seed=3)
    x = b.input((2, 2, 4, 4))
    b.output(b.expression("add(@0,@1)", [x, b.attribute(np.ones((2, 1, 1), np.float32))]))
    b.save(pp, bp)
    engine.pnnx_save(pp, bp, pp4, bp4, batch=4)
    text = _dump(tmp_path, pp4, bp4, "chan2")
    assert "operand 0 type=1 shape=4,2,4,4," in text and "operand 1 type=1 shape=2,1,1," in text and "operand 2 type=1 shape=4,2,4,4," in text, text


def test_attribute_is_no_layer_type(native_libs):
    assert "pnnx.Attribute" not in engine.registry_types()     # a constant has no layer: the engine binds it as an operand


# ---- the C-ABI ---------------------------------------------------------------------------------------------------------------------------
def test_binary_header_is_exported_and_bound(native_libs):
    H, _ = native_libs
    declared = ct.header_functions(cr.HEADER)
    assert declared == cr.ENTRIES
    assert sorted(H._si_binary_signatures) == sorted(declared)
    others = [getattr(H, n) for n in dir(H) if re.fullmatch(r"_si_\w*signatures", n) and n != "_si_binary_signatures"]
    assert len(others) >= 15
    for other in others:
        assert not set(declared) & set(other)
    raw = C.CDLL(_native.LIB_HIP_PATH)   # a handle of its own: nothing but the dynamic symbol table answers
    missing = [name for name in declared if not hasattr(raw, name)]
    assert not missing, missing
    # the Python structure has the header's fields in the header's order, with the header's types
    m = re.search(r"typedef struct SiBinaryDesc \{(.*?)\} SiBinaryDesc;", open(cr.HEADER).read(), flags=re.S)
    body = re.sub(r"/\*.*?\*/", " ", m.group(1), flags=re.S)
    fields = []
    for names in re.findall(r"\bint\s+([^;]+);", body):
        for n in names.split(","):
            arr = re.fullmatch(r"\s*(\w+)\[(\d+)\]\s*", n)
            fields.append((arr.group(1), C.c_int * int(arr.group(2))) if arr else (n.strip(), C.c_int))
    assert [(n, t._length_ if hasattr(t, "_length_") else 0) for n, t in fields] == \
        [(n, t._length_ if hasattr(t, "_length_") else 0) for n, t in _native.SiBinaryDesc._fields_], fields
    assert C.sizeof(_native.SiBinaryDesc) == 4 * (4 + 2 + 1 + 2 + 4 + 4 + 1)


def test_si_hip_header_declares_none_of_them():
    text = open(ct.HEADER).read()
    for name in cr.ENTRIES:
        assert name not in text, name
    assert "SiBinaryDesc" not in text and "si_hip_binary_const" not in text
    # the existing entries stay declared where they were
    for name in ("si_hip_binary_f32", "si_hip_binary_scalar_f32", "si_hip_binary_same_f16", "si_hip_binary_bcast_f16"):
        assert name in text, name


def test_every_compute_entry_of_the_binary_header_is_driven():
    """the rule of tests/test_containment_cpu.py for include/si_hip.h, applied to include/si_binary.h and the view cases of the GPU file"""
    import test_gpu_const as tc
    entries = [n for n in ct.header_functions(cr.HEADER) if not ct.is_exempt(n)]
    assert entries == ["si_hip_binary_const_f32", "si_hip_binary_const_f16"]
    driven = {e for c in tc.VIEW_CASES for e in c.entries}
    assert set(entries) <= driven, sorted(set(entries) - driven)
    assert driven <= set(ct.header_functions(cr.HEADER)), "a case names an entry the header does not declare"
    # every form and both arms of both types have a case
    assert {(c.half, c.form, c.vec) for c in tc.VIEW_CASES} == {(h, f, v) for h in (False, True) for f in ("chan", "pixel", "full") for v in (False, True)}


def test_abi_without_a_device(native_libs):
    """refusals happen before any device call: the addresses are made up, so a launch on them could not succeed"""
    H, _ = native_libs
    P = [C.c_void_p((j + 1) << 24) for j in range(4)]   # x, c0, c1, out: 16-byte aligned, 16 MiB apart

    def desc(n=1, **kw):
        d = hipops.binary_const_desc((2, 5, 7, 8), [2, 0][:n], [(1, 1, 1, 8), (1, 5, 7, 1)][:n])
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    for fn, half in (("si_hip_binary_const_f32", 0), ("si_hip_binary_const_f16", 1)):
        def call(d, p=P):
            return getattr(H, fn)(C.byref(d) if d is not None else None, p[0], p[1], p[2], p[3], None)

        def refused(d, code, what="", p=P):
            assert call(d, p) == code, (fn, what, call(d, p))
            assert H.si_hip_binary_const_kernel_name(C.byref(d) if d is not None else None, p[0], p[1], p[2], p[3], half) == b"none", (fn, what)

        refused(None, BADARG, "null descriptor")
        for j in (0, 1, 3):
            refused(desc(), BADARG, "null pointer %d" % j, [None if i == j else P[i] for i in range(4)])
        refused(desc(2), BADARG, "two stages without c1", [P[0], P[1], None, P[3]])
        for stages in (0, 3, -1):
            refused(desc(stages=stages), BADARG, "stages %d" % stages)
        for i in range(4):
            for v in (0, -1):
                d = desc()
                d.d[i] = v
                refused(d, BADARG, "extent %d = %d" % (i, v))
        refused(desc(x_ld=7), BADARG, "x_ld below the run")
        refused(desc(out_ld=7), BADARG, "out_ld below the run")
        refused(desc(grid_cap=-1), BADARG, "negative cap")
        d = desc()
        d.c0_stride[1] = -8
        refused(d, BADARG, "negative stride")
        for op in (4, 5, 12, -1):
            d = desc()
            d.op[0] = op
            refused(d, UNSUPPORTED, "code %d" % op)
            d = desc(2)
            d.op[1] = op
            refused(d, UNSUPPORTED, "second code %d" % op)
        # beyond 31 bits: x, out, a constant
        d = desc()
        d.d[0], d.d[1], d.d[2] = 1 << 10, 1 << 10, 1 << 8
        refused(d, BADARG, "2^28 pixels of 8")
        d = desc(x_ld=1 << 26)
        refused(d, BADARG, "x stride")
        d = desc()
        d.c0_stride[0] = 1 << 30
        d.c0_stride[2] = 1 << 28
        refused(d, BADARG, "constant offsets")
        # what is accepted names its kernel: the form by the strides, the arm by the pointers
        t = "_Float16, 8" if half else "float, 4"
        name = lambda d, p=P: H.si_hip_binary_const_kernel_name(C.byref(d), p[0], p[1], p[2], p[3], half).decode()
        assert name(desc()) == "binary_const_kernel<%s, chan>" % t
        assert name(desc(2)) == "binary_const_kernel<%s, full>" % t
        odd = [C.c_void_p(P[0].value + (2 if half else 4))] + P[1:]
        assert name(desc(), odd) == "binary_const_kernel<%s, 1, chan>" % ("_Float16" if half else "float")


# ---- stand-alone programs under the sanitizers ---------------------------------------------------------------------------------------------
SANITIZE = ["-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]      # the runtimes inside the program: it starts the same under any environment


def _stand_alone(tmp_path, source, includes, ok):
    exe = str(tmp_path / os.path.splitext(source)[0])
    subprocess.check_call(["g++", "-std=c++17", "-O0", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined"] + SANITIZE +
                          ["-I" + i for i in includes] + [os.path.join(cr.ROOT, "tests", "cpp", source), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and ok in r.stdout and "runtime error" not in r.stderr, r.stdout[-4000:] + r.stderr[-4000:]


def test_plan_arithmetic_stand_alone_under_sanitizers(tmp_path):
    hip_dir = os.path.join(cr.ROOT, "simpleinfer_amd", "csrc", "hip")
    _stand_alone(tmp_path, "test_binary_plan.cpp", [hip_dir, os.path.join(cr.ROOT, "include")], "binary plan ok")
    # the kernel files use that header, and the header nothing of HIP beyond the C-ABI's types
    assert '#include "binary_plan.h"' in open(os.path.join(hip_dir, "binary_const.hip")).read()
    assert '#include "binary_plan.h"' in open(os.path.join(hip_dir, "ops.hip")).read()
    text = re.sub(r"//[^\n]*", "", open(os.path.join(hip_dir, "binary_plan.h")).read())
    assert "hip_runtime" not in text and "__global__" not in text and "__device__" not in text


def test_batch_rule_for_constants_stand_alone_under_sanitizers(tmp_path):
    _stand_alone(tmp_path, "test_batch_rule_const.cpp", [os.path.join(cr.ROOT, "simpleinfer_amd", "csrc", "host")], "const rule ok")
