"""CPU: nn.Conv1d and the temporal convolution kernels' host side -- the numpy rule of tests/conv1d_reference.py pinned to torch float64 on
every case (padding='same' with an even and an odd d (K - 1) among them); the builder's lines and both toys' operator sequences and float64
evaluation; the registry; the C-ABI of include/si_conv1d.h (exported, bound under its own table, absent from include/si_hip.h, the
structure's fields, every compute entry driven by a view case of the GPU file); what is decided without a device: every refusal by return
code, the weight images against a numpy statement of the lane order; and two stand-alone C++ programs under AddressSanitizer and UBSan: the
plan arithmetic (tests/cpp/test_conv1d_plan.cpp over csrc/hip/conv1d_plan.h) and the batch rule's kSpatial row on rank-3 operands
(tests/cpp/test_batch_rule_conv1d.cpp)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import containment as ct
import conv1d_reference as cr
from ct_reference import _parse
from simpleinfer_amd import _native, engine, hipops, modelgen as mg

BADARG, UNSUPPORTED = -1, -2
ALL_CASES = cr.CASES + cr.F16_CASES[-4:-3] + cr.SAME_CASES


@pytest.mark.parametrize("case", ALL_CASES, ids=[cr.case_id(c) for c in ALL_CASES])
def test_rule_equals_torch(case):
    pytest.importorskip("torch")
    n, c, l, oc, k, s, p, d, g = case
    for bias in (True, False):
        x, w, b = cr.operands(case, seed=3, bias=bias)
        got, ref = cr.conv1d_ref(x, w, b, s, p, d, g), cr.conv1d_torch(x, w, b, s, p, d, g)
        assert got.shape == ref.shape == (n, oc, cr.out_len(l, k, s, p, d)), (got.shape, ref.shape)
        assert np.abs(got - ref).max() <= 1e-12, (case, bias, np.abs(got - ref).max())


def test_same_pads_one_more_on_the_right():
    assert cr.pads(4, "same", 1) == (1, 2) and cr.pads(3, "same", 3) == (3, 3) and cr.pads(2, "same", 3) == (1, 2) and cr.pads(5, "valid") == (0, 0)
    assert hipops.conv1d_pads(4, "same", 1) == (1, 2) and hipops.conv1d_pads(3, "same", 4) == (4, 4) and hipops.conv1d_pads(7, 3) == (3, 3)
    for case in ALL_CASES:
        n, c, l, oc, k, s, p, d, g = case
        assert hipops.conv1d_out_len(l, k, s, p, d) == cr.out_len(l, k, s, p, d)
        dsc = hipops.conv1d_desc(n, c, l, oc, k, s, p, d, g)
        assert (dsc.lo, dsc.pad_left) == (cr.out_len(l, k, s, p, d), cr.pads(k, p, d, s)[0])
        assert (dsc.x_sc, dsc.x_sn, dsc.y_sc, dsc.y_sn) == (l, c * l, dsc.lo, oc * dsc.lo)


def test_the_fp16_restatement_rounds_the_operands_only():
    case = cr.DENSE_CASES[3]
    x, w, b = cr.operands(case, seed=5)
    n, c, l, oc, k, s, p, d, g = case
    exact = cr.conv1d_ref(x, w, b, s, p, d, g)
    half = cr.conv1d_ref(x, w, b, s, p, d, g, rnd=cr.round_f16)
    same = cr.conv1d_ref(cr.round_f16(x), cr.round_f16(w), b, s, p, d, g)
    assert np.array_equal(half, same) and 0.0 < np.abs(half - exact).max() < 1e-2


def test_builder_lines_parse_back():
    b = mg.PnnxBuilder(seed=1)
    x = b.input((2, 16, 50))
    y = b.conv1d(x, 32, 11, 2, 5)
    z = b.conv1d(y, 32, 33, 1, "same", groups=32, bias=False)
    v = b.conv1d(z, 8, 4, 1, "valid", d=3)
    u = b.conv1d(b.input((16, 50)), 4, 3, padding_mode="reflect")
    parsed = [_parse(ln) for ln in b.lines if ln.startswith("nn.Conv1d")]
    assert [p[0] for p in parsed] == ["nn.Conv1d"] * 4
    assert parsed[0][4] == dict(bias="True", dilation="(1)", groups="1", in_channels="16", kernel_size="(11)", out_channels="32", padding="(5)",
                                padding_mode="zeros", stride="(2)")
    assert parsed[1][4]["padding"] == "same" and parsed[1][4]["groups"] == "32" and parsed[1][4]["bias"] == "False"
    assert parsed[2][4]["padding"] == "valid" and parsed[2][4]["dilation"] == "(3)" and parsed[3][4]["padding_mode"] == "reflect"
    assert b.shapes[y] == (2, 32, 25) and b.shapes[z] == (2, 32, 25) and b.shapes[v] == (2, 8, 16) and b.shapes[u] == (4, 50)
    n0, n1 = parsed[0][1], parsed[1][1]
    assert b.attrs[n0 + ".weight"].shape == (32, 16, 11) and b.attrs[n0 + ".bias"].shape == (32,)
    assert b.attrs[n1 + ".weight"].shape == (32, 1, 33) and n1 + ".bias" not in b.attrs


def _types(b):
    return [_parse(ln)[0] for ln in b.lines]


def test_toys_have_the_expected_operator_sequences():
    block = ["nn.Conv1d", "nn.Conv1d", "nn.ReLU", "nn.Conv1d", "pnnx.Expression", "nn.ReLU"]
    b = mg.build_toy_quartznet()
    assert _types(b) == ["pnnx.Input", "nn.Conv1d", "nn.ReLU"] + block * 2 + ["nn.Conv1d", "nn.ReLU", "nn.Conv1d", "pnnx.Output"]
    convs = [_parse(ln) for ln in b.lines if ln.startswith("nn.Conv1d")]
    assert b.shapes["0"] == (2, 16, 64) and len(b.shapes["0"]) == 3
    assert convs[0][4]["kernel_size"] == "(11)" and convs[0][4]["stride"] == "(2)"
    assert convs[1][4]["kernel_size"] == "(33)" and convs[1][4]["groups"] == convs[1][4]["in_channels"] == convs[1][4]["out_channels"] == "32"
    assert convs[2][4]["kernel_size"] == "(1)" and convs[3][4]["kernel_size"] == "(1)"
    assert convs[7][4]["dilation"] == "(2)" and convs[7][4]["padding"] == "same" and convs[8][4]["out_channels"] == "12"
    x = np.random.Generator(np.random.Philox(1)).uniform(-1, 1, (2, 16, 64)).astype(np.float32)
    (y,) = cr.eval_graph(b, x)
    assert y.shape == (2, 12, 32) and np.isfinite(y).all() and np.abs(y).max() > 1e-3
    (yh,) = cr.eval_graph(b, x, rnd=cr.round_f16)
    assert 0.0 < np.abs(yh - y).max() < 2e-2 * np.abs(y).max()

    g = mg.build_toy_conv_gru()
    assert _types(g) == ["pnnx.Input", "nn.Conv1d", "nn.Hardtanh", "nn.Conv1d", "nn.Hardtanh", "Tensor.permute", "nn.GRU", "nn.Linear", "pnnx.Output"]
    perm = _parse([ln for ln in g.lines if ln.startswith("Tensor.permute")][0])
    assert perm[4]["dims"] == "(2,0,1)" and g.shapes[perm[2][0]] == (2, 16, 13) and g.shapes[perm[3][0]] == (13, 2, 16)
    x = np.random.Generator(np.random.Philox(2)).uniform(-1, 1, (2, 8, 50)).astype(np.float32)
    (y,) = cr.eval_graph(g, x)
    assert y.shape == (13, 2, 9) and np.isfinite(y).all()
    # the evaluator's convolution is torch's, operator by operator
    torch = pytest.importorskip("torch")
    name = _parse(g.lines[1])[1]
    want = torch.nn.functional.conv1d(torch.from_numpy(x.astype(np.float64)), torch.from_numpy(g.attrs[name + ".weight"].astype(np.float64)),
                                      torch.from_numpy(g.attrs[name + ".bias"].astype(np.float64)), 2, 5).clamp(0.0, 20.0).numpy()
    two = mg.PnnxBuilder(seed=0)
    two.output(two.hardtanh(two.conv1d(two.input((2, 8, 50)), 16, 11, 2, 5), 0.0, 20.0))
    assert np.abs(cr.eval_graph(two, x)[0] - want).max() <= 1e-12


def test_registry_lists_the_type(native_libs):
    types = engine.registry_types()
    assert "nn.Conv1d" in types
    for absent in ("F.conv1d", "nn.ConvTranspose1d", "nn.BatchNorm1d", "nn.MaxPool1d", "nn.AdaptiveAvgPool1d", "nn.Conv3d"):
        assert absent not in types, absent


def _declared(path):
    src = open(path).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    names = []
    for m in re.finditer(r"\b(si_[a-z0-9_]+)\s*\(", src):
        if m.group(1) not in names:
            names.append(m.group(1))
    return names


def test_conv1d_header_is_exported_and_bound(native_libs):
    H, _ = native_libs
    declared = _declared(cr.HEADER)
    assert declared == cr.ENTRIES
    assert sorted(H._si_conv1d_signatures) == sorted(declared)
    for other in (H._si_signatures, H._si_norm_signatures, H._si_pad_signatures, H._si_pool_signatures, H._si_softmax_signatures, H._si_superres_signatures,
                  H._si_slice_signatures, H._si_reduce_signatures, H._si_act_signatures, H._si_permute_signatures, H._si_attention_signatures,
                  H._si_deform_signatures, H._si_grid_signatures, H._si_roi_signatures, H._si_rnn_signatures, H._si_binary_signatures):
        assert not set(declared) & set(other)
    raw = C.CDLL(_native.LIB_HIP_PATH)   # a handle of its own: nothing but the dynamic symbol table answers
    missing = [name for name in declared if not hasattr(raw, name)]
    assert not missing, missing
    # the Python structure has the header's fields in the header's order, with the header's types
    ctypes_of = {"int": C.c_int, "long long": C.c_longlong, "float": C.c_float}
    fields = [(n, ctypes_of[typ]) for n, typ in cr.header_fields()]
    assert fields == list(_native.SiConv1dDesc._fields_), fields
    assert [n for n, _ in fields] == ["n", "c", "l", "oc", "lo", "k", "stride", "dilation", "pad_left", "groups", "x_sn", "x_sc", "y_sn", "y_sc", "act",
                                      "act_param"]
    # the header states the contract
    text = open(cr.HEADER).read()
    for phrase in ("Reduction order", "depend on that item's data alone", "Nothing beyond the extents is read or written",
                   "safe inside a captured graph", "never allocate", "the right pad is implied by lo"):
        assert phrase in text, phrase


def test_si_hip_header_declares_none_of_them():
    text = open(ct.HEADER).read()
    for name in cr.ENTRIES:
        assert name not in text, name
    assert "SiConv1dDesc" not in text and "si_hip_conv1d" not in text


def test_every_compute_entry_of_the_conv1d_header_is_driven():
    """the rule of tests/test_containment_cpu.py for include/si_hip.h, applied to include/si_conv1d.h and the view cases of the GPU file"""
    import test_gpu_conv1d as tc
    entries = [n for n in ct.header_functions(cr.HEADER) if not ct.is_exempt(n)]
    assert entries == ["si_hip_conv1d_f32", "si_hip_conv1d_f16", "si_hip_conv1d_weight_bytes", "si_hip_conv1d_pack_weights_f32",
                       "si_hip_conv1d_pack_weights_f16"]
    driven = {e for c in tc.VIEW_CASES for e in c.entries}
    assert set(entries) <= driven, sorted(set(entries) - driven)
    assert driven <= set(ct.header_functions(cr.HEADER)), "a case names an entry the header does not declare"
    # every form in both types is among the view cases
    names = {cr.kname(c.case, c.dtype) for c in tc.VIEW_CASES}
    assert names == {"conv1d_%s_kernel<%s>" % (f, t) for f in ("dense", "depthwise") for t in ("float", "_Float16")}


def test_the_kernel_file_uses_neither_a_magic_division_nor_umulhi():
    hip_dir = os.path.join(cr.ROOT, "simpleinfer_amd", "csrc", "hip")
    src = open(os.path.join(hip_dir, "conv1d.hip")).read()
    assert "si_fast_div(" not in src and "__umulhi" not in src
    assert '#include "conv1d_plan.h"' in src
    assert "hip" not in re.sub(r"//[^\n]*", "", open(os.path.join(hip_dir, "conv1d_plan.h")).read()).lower()


def test_abi_refusals_without_a_launch(native_libs):
    """every refusal happens before any device call: the addresses are made up, 16-byte aligned and 16 MiB apart"""
    H, _ = native_libs
    X, W, B, Y = (C.c_void_p((j + 1) << 24) for j in range(4))

    def desc(n=2, c=8, l=33, oc=24, k=5, s=2, p=2, d=1, g=1, **kw):
        return hipops.conv1d_desc(n, c, l, oc, k, s, p, d, g, **kw)

    for fn, half in (("si_hip_conv1d_f32", 0), ("si_hip_conv1d_f16", 1)):
        def call(dd, x=X, w=W, b=B, y=Y):
            return getattr(H, fn)(C.byref(dd), x, w, b, y, None)

        def name(dd, x=X, y=Y):
            return H.si_hip_conv1d_kernel_name(C.byref(dd), x, y, half)

        def refused(dd, code, what=""):
            assert call(dd) == code, (fn, what, call(dd))
            assert name(dd) == b"none", (fn, what)

        assert getattr(H, fn)(None, X, W, B, Y, None) == BADARG                                  # null descriptor
        assert call(desc(), x=None) == BADARG and call(desc(), w=None) == BADARG and call(desc(), y=None) == BADARG
        assert name(desc(), x=None) == b"none" and name(desc(), y=None) == b"none" and H.si_hip_conv1d_kernel_name(None, X, Y, half) == b"none"
        for field in ("n", "c", "l", "oc", "lo", "k", "stride", "dilation", "groups"):           # non-positive sizes
            for value in (0, -1):
                bad = desc()
                setattr(bad, field, value)
                refused(bad, BADARG, (field, value))
        bad = desc()
        bad.pad_left = -1
        refused(bad, BADARG, "negative pad")
        refused(desc(c=8, oc=24, g=3), BADARG, "groups do not divide c")
        refused(desc(c=9, oc=25, g=3), BADARG, "groups do not divide oc")
        # lo against torch's formula: 17 is what pad 2 gives, 16 what the left pad alone gives, 18 a larger right pad; 15 and 0 fit no right pad
        for lo, ok in ((17, True), (16, True), (18, True), (15, False), (1, False)):
            dd = desc(lo=lo)
            assert (name(dd) != b"none") == ok, (fn, lo)
            if not ok:
                refused(dd, BADARG, ("lo", lo))
        assert name(desc(l=8, k=11, s=1, p=5)) != b"none"                                        # K > L with enough padding
        # strides below the row width, batch items that share a row
        for field, value in (("x_sc", 32), ("y_sc", 16), ("x_sn", 8 * 33 - 1), ("y_sn", 24 * 17 - 1), ("x_sn", -264), ("y_sc", -17)):
            bad = desc()
            setattr(bad, field, value)
            refused(bad, BADARG, (field, value))
        wide = desc(x_sc=40, x_sn=12 * 40, y_sc=20, y_sn=30 * 20)                                # a channel slice and a crop are fine
        assert name(wide) != b"none"
        # y overlapping x, the image or the bias
        es = 2 if half else 4
        assert call(desc(), y=X) == BADARG and call(desc(), y=W) == BADARG and call(desc(), y=B) == BADARG
        assert call(desc(), y=C.c_void_p(X.value + 2 * 8 * 33 * es - es)) == BADARG              # y starts on x's last element
        assert call(desc(), x=C.c_void_p(Y.value + 64)) == BADARG
        # element offsets beyond 31 bits; grid extents; a span beyond the LDS
        refused(desc(n=3, x_sn=1 << 30), UNSUPPORTED, "x offsets")
        refused(desc(n=3, y_sn=1 << 30), UNSUPPORTED, "y offsets")
        refused(desc(x_sc=1 << 31, x_sn=1 << 34), UNSUPPORTED, "a stride beyond 31 bits")
        refused(desc(n=65536, c=1, l=1, oc=1, k=1, s=1, p=0), UNSUPPORTED, "batch beyond a grid's z")
        refused(desc(n=1, c=8, l=100000, oc=8, k=3, s=1, p=0, d=30000), UNSUPPORTED, "a span beyond the LDS")
        assert name(desc()) == cr.kname((2, 8, 33, 24, 5, 2, 2, 1, 1), np.float16 if half else np.float32).encode()
        dw = (2, 8, 40, 8, 33, 1, 16, 1, 8)
        assert name(desc(*dw)) == cr.kname(dw, np.float16 if half else np.float32).encode()
        # the image functions look at the filter alone
        filt = hipops.conv1d_desc(1, 8, 1, 24, 5, lo=1)
        filt.n = filt.l = filt.lo = filt.stride = filt.dilation = 0
        assert H.si_hip_conv1d_weight_bytes(C.byref(filt), half) == 2 * (1 if half else 2) * 5 * 64 * (16 if half else 4)
        assert H.si_hip_conv1d_weight_bytes(None, half) == 0
        for field in ("c", "oc", "k", "groups"):
            bad = hipops.conv1d_desc(1, 8, 1, 24, 5, lo=1)
            setattr(bad, field, 0)
            assert H.si_hip_conv1d_weight_bytes(C.byref(bad), half) == 0, field
            pack = getattr(H, "si_hip_conv1d_pack_weights_" + ("f16" if half else "f32"))
            assert pack(C.byref(bad), X, Y) == BADARG, field
    # fp16 alone: the divisibility rule of the dense form, an image off 16 bytes, a row off 2 bytes
    d12 = desc(c=12)
    assert H.si_hip_conv1d_f16(C.byref(d12), X, W, B, Y, None) == UNSUPPORTED and H.si_hip_conv1d_kernel_name(C.byref(d12), X, Y, 1) == b"none"
    assert H.si_hip_conv1d_kernel_name(C.byref(d12), X, Y, 0) == b"conv1d_dense_kernel<float>"
    assert H.si_hip_conv1d_weight_bytes(C.byref(d12), 1) == 0 and H.si_hip_conv1d_weight_bytes(C.byref(d12), 0) > 0
    g2 = desc(c=16, g=2)
    assert H.si_hip_conv1d_kernel_name(C.byref(g2), X, Y, 1) == b"conv1d_dense_kernel<_Float16>"
    assert H.si_hip_conv1d_kernel_name(C.byref(desc(c=16, oc=24, g=4)), X, Y, 1) == b"none"
    assert H.si_hip_conv1d_f16(C.byref(desc()), X, C.c_void_p(W.value + 8), B, Y, None) == UNSUPPORTED
    assert H.si_hip_conv1d_kernel_name(C.byref(desc()), C.c_void_p(X.value + 1), Y, 1) == b"none"
    assert H.si_hip_conv1d_kernel_name(C.byref(desc()), C.c_void_p(X.value + 2), Y, 1) == b"conv1d_dense_kernel<_Float16>"
    assert H.si_hip_conv1d_kernel_name(C.byref(desc()), C.c_void_p(X.value + 2), Y, 0) == b"none"


def test_weight_images_against_the_lane_order(native_libs):
    """dense: lane 16 g + x of (group, tile, channel step q, tap k) holds w[16 tile + x][4 q + g][k] (fp32) or [32 q + 8 g ..][k] (fp16);
    filters and channels beyond the group's are zeros, and every weight is there once.  depthwise: the filters as they are"""
    r = np.random.Generator(np.random.Philox(9))
    for oc, cg, k, groups in ((5, 3, 3, 1), (24, 8, 5, 1), (40, 24, 3, 1), (18, 4, 3, 3), (8, 1, 5, 4), (64, 64, 1, 1), (17, 33, 2, 1), (32, 40, 2, 2)):
        w = r.uniform(-1, 1, (oc, cg, k)).astype(np.float32)
        img = hipops.conv1d_pack_weights(w, groups)
        want = cr.dense_image(w, groups, False)
        assert img.size == want.size and np.array_equal(img.reshape(want.shape), want), (oc, cg, k, groups)
        assert np.count_nonzero(img) == np.count_nonzero(w)
        if cg % 8 == 0:
            img16 = hipops.conv1d_pack_weights(w, groups, half=True)
            want16 = cr.dense_image(w, groups, True)
            assert img16.dtype == np.float16 and img16.size == want16.size and np.array_equal(img16.reshape(want16.shape), want16), (oc, cg, k, groups)
        else:
            with pytest.raises(hipops.HipError):
                hipops.conv1d_pack_weights(w, groups, half=True)
    w = r.uniform(-1, 1, (16, 1, 87)).astype(np.float32)
    assert np.array_equal(hipops.conv1d_pack_weights(w, 16), w.reshape(-1))
    assert np.array_equal(hipops.conv1d_pack_weights(w, 16, half=True), w.reshape(-1).astype(np.float16))


SANITIZE = ["-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]      # the runtimes inside the program: it starts the same under any environment


def _stand_alone(tmp_path, source, include, ok):
    exe = str(tmp_path / os.path.splitext(source)[0])
    subprocess.check_call(["g++", "-std=c++17", "-O0", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined"] + SANITIZE +
                          ["-I" + include, os.path.join(cr.ROOT, "tests", "cpp", source), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and ok in r.stdout and "runtime error" not in r.stderr, r.stdout[-4000:] + r.stderr[-4000:]


def test_plan_arithmetic_stand_alone_under_sanitizers(tmp_path):
    _stand_alone(tmp_path, "test_conv1d_plan.cpp", os.path.join(cr.ROOT, "simpleinfer_amd", "csrc", "hip"), "conv1d plan ok")


def test_batch_rule_on_rank_3_operands_stand_alone_under_sanitizers(tmp_path):
    _stand_alone(tmp_path, "test_batch_rule_conv1d.cpp", os.path.join(cr.ROOT, "simpleinfer_amd", "csrc", "host"), "conv1d rule ok")
