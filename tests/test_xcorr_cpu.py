"""CPU: F.conv2d with a tensor filter and the cross-correlation kernels' host side -- the numpy rule of tests/xcorr_reference.py pinned to torch
float64 on every case (padding='same' with odd totals among them); the builder's lines, the toys' operator sequences and their float64
evaluation; the registry; the C-ABI of include/si_xcorr.h (exported, bound under its own table, absent from include/si_hip.h, the
structure's fields, every compute entry driven by a view case of the GPU file); every refusal by return code, without a launch; the
lowering of a constant filter to nn.Conv2d, checked on the written graph; and two stand-alone C++ programs under AddressSanitizer and UBSan:
the plan arithmetic (tests/cpp/test_xcorr_plan.cpp over csrc/hip/xcorr_plan.h) and the batch rule's family kXcorr
(tests/cpp/test_batch_rule_xcorr.cpp)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import containment as ct
import xcorr_reference as xr
from ct_reference import _parse
from simpleinfer_amd import _native, engine, hipops, modelgen as mg

BADARG, UNSUPPORTED = -1, -2
SAME_CASES = [(2, 3, 7, 9, 4, 4, 2, 1, "same", 1, 1), (1, 4, 9, 9, 4, 2, 5, 1, "same", 3, 2), (1, 2, 7, 7, 2, 5, 3, 1, "valid", 1, 1)]
ALL_CASES = xr.CASES + xr.F16_CASES[-9:-7] + SAME_CASES


@pytest.mark.parametrize("case", ALL_CASES, ids=[xr.case_id(c) for c in ALL_CASES])
def test_rule_equals_torch(case):
    pytest.importorskip("torch")
    n, c, h, wd, oc, kh, kw, s, p, d, g = case
    for bias in (True, False):
        x, w, b = xr.operands(case, seed=3, bias=bias)
        got, ref = xr.conv2d_ref(x, w, b, s, p, d, g), xr.conv2d_torch(x, w, b, s, p, d, g)
        assert got.shape == ref.shape == (n, oc) + xr.out_hw(h, wd, kh, kw, s, p, d), (got.shape, ref.shape)
        assert np.abs(got - ref).max() <= 1e-12, (case, bias, np.abs(got - ref).max())
    if xr.is_depthwise(case):
        # per-sample: the sandwich of views around groups = N C, in torch
        z = xr.templates(case, seed=3)
        want = xr.conv2d_torch(x.reshape(1, n * c, h, wd), z.reshape(n * c, 1, kh, kw), None, s, p, d, n * c).reshape(got.shape)
        assert np.abs(xr.per_sample_ref(x, z, None, s, p, d) - want).max() <= 1e-12


def test_pads_and_descriptor_defaults():
    assert xr.pads(4, 2, "same") == ((1, 2), (0, 1)) and xr.pads(3, 3, "same", 2) == ((2, 2), (2, 2)) and xr.pads(5, 5, "valid") == ((0, 0), (0, 0))
    assert hipops.xcorr_pads(4, 2, "same") == ((1, 2), (0, 1)) and hipops.xcorr_pads(3, 3, (2, 1)) == ((2, 2), (1, 1))
    for case in ALL_CASES:
        n, c, h, wd, oc, kh, kw, s, p, d, g = case
        assert hipops.xcorr_out_hw(h, wd, kh, kw, s, p, d) == xr.out_hw(h, wd, kh, kw, s, p, d)
        dsc = hipops.xcorr_desc(n, h, wd, c, oc, kh, kw, s, p, d, g)
        (pt, _), (pl, _) = xr.pads(kh, kw, p, d, s)
        assert (dsc.ho, dsc.wo) == xr.out_hw(h, wd, kh, kw, s, p, d) and (dsc.pad_top, dsc.pad_left) == (pt, pl)
        assert (dsc.x_sp, dsc.x_sh, dsc.x_sn) == (c, wd * c, h * wd * c) and (dsc.y_sp, dsc.y_sh, dsc.y_sn) == (oc, dsc.wo * oc, dsc.ho * dsc.wo * oc)
        if xr.is_depthwise(case):
            assert (dsc.w_sc, dsc.w_sp, dsc.w_sh, dsc.w_sn, dsc.per_sample) == (kh * kw, 1, kw, 0, 0)
            ps = hipops.xcorr_desc(n, h, wd, c, oc, kh, kw, s, p, d, g, per_sample=True)
            assert (ps.w_sc, ps.w_sp, ps.w_sh, ps.w_sn, ps.per_sample) == (1, c, kw * c, kh * kw * c, 1)
        elif g == 1:     # (a grouped case of the list is there for the rule against torch alone: no kernel serves it)
            assert (dsc.w_sc, dsc.w_sp, dsc.w_sh, dsc.w_sn, dsc.per_sample) == (1, c, kw * c, kh * kw * c, 0)


def test_the_fp16_restatement_rounds_the_operands_only():
    case = xr.DENSE_CASES[6]
    x, w, b = xr.operands(case, seed=5)
    n, c, h, wd, oc, kh, kw, s, p, d, g = case
    exact = xr.conv2d_ref(x, w, b, s, p, d, g)
    half = xr.conv2d_ref(x, w, b, s, p, d, g, rnd=xr.round_f16)
    same = xr.conv2d_ref(xr.round_f16(x), xr.round_f16(w), b, s, p, d, g)
    assert np.array_equal(half, same) and 0.0 < np.abs(half - exact).max() < 1e-2


def test_builder_lines_parse_back():
    b = mg.PnnxBuilder(seed=1)
    x, w = b.input((2, 8, 16, 16)), b.input((6, 8, 3, 5))
    y = b.conv2d_functional(x, w)
    z = b.conv2d_functional(x, w, b.attribute(np.zeros(6, np.float32)), stride=(2, 1), padding=(1, 2), dilation=2)
    v = b.conv2d_functional(x, b.attribute(np.zeros((8, 1, 4, 2), np.float32)), padding="same", groups=8)
    u = b.conv2d_functional(x, w, padding="valid")
    parsed = [_parse(ln) for ln in b.lines if ln.startswith("F.conv2d")]
    assert [p[0] for p in parsed] == ["F.conv2d"] * 4
    assert parsed[0][2] == [x, w] and parsed[0][4] == dict(bias="None", stride="(1,1)", padding="(0,0)", dilation="(1,1)", groups="1")
    assert len(parsed[1][2]) == 3 and "bias" not in parsed[1][4]
    assert parsed[1][4] == dict(stride="(2,1)", padding="(1,2)", dilation="(2,2)", groups="1")
    assert parsed[2][4]["padding"] == "same" and parsed[2][4]["groups"] == "8" and parsed[3][4]["padding"] == "valid"
    assert b.shapes[y] == (2, 6, 14, 12) and b.shapes[z] == (2, 6, 7, 12) and b.shapes[v] == (2, 8, 16, 16) and b.shapes[u] == (2, 6, 14, 12)


def _types(b):
    return [_parse(ln)[0] for ln in b.lines]


def _inputs(b, seed):
    r = np.random.Generator(np.random.Philox(seed))
    return [r.uniform(-1, 1, b.shapes[_parse(ln)[3][0]]).astype(np.float32) for ln in b.lines if ln.startswith("pnnx.Input")]


def test_toys_have_the_expected_operator_sequences():
    stack = ["nn.Conv2d", "nn.ReLU", "nn.Conv2d"]
    b = mg.build_toy_siamfc()
    assert _types(b) == ["pnnx.Input", "pnnx.Input"] + stack * 2 + ["F.conv2d", "pnnx.Output"]
    (fc,) = [_parse(ln) for ln in b.lines if ln.startswith("F.conv2d")]
    assert b.shapes[fc[2][0]] == (1, 16, 29, 29) and b.shapes[fc[2][1]] == (1, 16, 13, 13) and b.shapes[fc[3][0]] == (1, 1, 17, 17)
    b = mg.build_toy_siamrpn()
    assert _types(b) == ["pnnx.Input", "pnnx.Input"] + stack * 2 + ["Tensor.view", "F.conv2d", "nn.ReLU", "pnnx.Output"]
    (fc,) = [_parse(ln) for ln in b.lines if ln.startswith("F.conv2d")]
    assert b.shapes[fc[2][1]] == (10, 8, 4, 4) and b.shapes[fc[3][0]] == (1, 10, 13, 13)
    for n in (1, 2):
        b = mg.build_toy_siamrpnpp(batch=n)
        assert _types(b) == ["pnnx.Input", "pnnx.Input"] + stack * 2 + ["Tensor.view", "Tensor.view", "F.conv2d", "Tensor.view", "nn.Conv2d", "pnnx.Output"]
        (fc,) = [_parse(ln) for ln in b.lines if ln.startswith("F.conv2d")]
        assert b.shapes[fc[2][0]] == (1, 8 * n, 15, 15) and b.shapes[fc[2][1]] == (8 * n, 1, 7, 7) and fc[4]["groups"] == str(8 * n)
        views = [_parse(ln) for ln in b.lines if ln.startswith("Tensor.view")]
        assert b.shapes[views[2][3][0]] == (n, 8, 9, 9)
    b = mg.build_toy_dynamic_head()
    assert _types(b) == ["pnnx.Input", "nn.Conv2d", "nn.ReLU", "nn.AdaptiveAvgPool2d", "nn.Conv2d", "Tensor.view", "F.conv2d", "nn.Sigmoid", "pnnx.Output"]
    b = mg.build_toy_dynamic_head(batch=2, constant=True)
    assert _types(b) == ["pnnx.Input", "nn.Conv2d", "nn.ReLU", "pnnx.Attribute", "Tensor.view", "F.conv2d", "nn.Sigmoid", "pnnx.Output"]
    b = mg.build_toy_blurpool()
    assert _types(b) == ["pnnx.Input", "nn.Conv2d", "nn.ReLU", "pnnx.Attribute", "F.conv2d", "nn.Conv2d", "pnnx.Output"]
    (fc,) = [_parse(ln) for ln in b.lines if ln.startswith("F.conv2d")]
    assert fc[4] == dict(bias="None", stride="(2,2)", padding="(1,1)", dilation="(1,1)", groups="8") and b.shapes[fc[3][0]] == (2, 8, 8, 8)
    blur = b.attrs[_parse([ln for ln in b.lines if ln.startswith("pnnx.Attribute")][0])[1] + ".data"]
    assert blur.shape == (8, 1, 3, 3) and np.array_equal(blur[3, 0] * 16, [[1, 2, 1], [2, 4, 2], [1, 2, 1]])
    # every toy evaluates in float64, and its fp16 emulation stays close
    for build in (mg.build_toy_siamfc, mg.build_toy_siamrpn, mg.build_toy_siamrpnpp, mg.build_toy_dynamic_head, mg.build_toy_blurpool):
        b = build()
        xs = _inputs(b, 1)
        (y,) = xr.eval_graph(b, xs)
        assert np.isfinite(y).all() and np.abs(y).max() > 1e-3
        (yh,) = xr.eval_graph(b, xs, rnd=xr.round_f16)
        assert 0.0 < np.abs(yh - y).max() < 2e-2 * np.abs(y).max()


def test_the_evaluator_is_torch_operator_by_operator():
    torch = pytest.importorskip("torch")
    F = torch.nn.functional
    b = mg.build_toy_siamrpnpp(batch=2)
    z, x = _inputs(b, 2)
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    convs = [_parse(ln)[1] for ln in b.lines if ln.startswith("nn.Conv2d")]
    wb = lambda i: (t(b.attrs[convs[i] + ".weight"]), t(b.attrs[convs[i] + ".bias"]))
    fz = F.conv2d(F.relu(F.conv2d(t(z), *wb(0))), *wb(1))
    fx = F.conv2d(F.relu(F.conv2d(t(x), *wb(2))), *wb(3))
    y = F.conv2d(fx.view(1, 16, 15, 15), fz.view(16, 1, 7, 7), groups=16).view(2, 8, 9, 9)
    want = F.conv2d(y, *wb(4)).numpy()
    assert np.abs(xr.eval_graph(b, [z, x])[0] - want).max() <= 1e-12


def test_registry_lists_the_type(native_libs):
    types = engine.registry_types()
    assert "F.conv2d" in types
    for absent in ("F.conv1d", "F.conv_transpose2d", "F.linear", "nn.Conv3d", "pnnx.Attribute", "torch.matmul", "nn.LayerNorm"):
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


def test_xcorr_header_is_exported_and_bound(native_libs):
    H, _ = native_libs
    declared = _declared(xr.HEADER)
    assert declared == xr.ENTRIES
    assert sorted(H._si_xcorr_signatures) == sorted(declared)
    for other in (H._si_signatures, H._si_norm_signatures, H._si_pad_signatures, H._si_pool_signatures, H._si_softmax_signatures, H._si_superres_signatures,
                  H._si_slice_signatures, H._si_reduce_signatures, H._si_act_signatures, H._si_permute_signatures, H._si_attention_signatures,
                  H._si_deform_signatures, H._si_grid_signatures, H._si_roi_signatures, H._si_rnn_signatures, H._si_binary_signatures,
                  H._si_conv1d_signatures):
        assert not set(declared) & set(other)
    raw = C.CDLL(_native.LIB_HIP_PATH)   # a handle of its own: nothing but the dynamic symbol table answers
    missing = [name for name in declared if not hasattr(raw, name)]
    assert not missing, missing
    # the Python structure has the header's fields in the header's order, with the header's types
    ctypes_of = {"int": C.c_int, "long long": C.c_longlong, "float": C.c_float}
    fields = [(n, ctypes_of[typ]) for n, typ in xr.header_fields()]
    assert fields == list(_native.SiXcorrDesc._fields_), fields
    assert [n for n, _ in fields] == ["n", "h", "w", "c", "oc", "ho", "wo", "kh", "kw", "stride_h", "stride_w", "dilation_h", "dilation_w", "pad_top",
                                      "pad_left", "groups", "x_sn", "x_sh", "x_sp", "w_sn", "w_sh", "w_sp", "w_sc", "y_sn", "y_sh", "y_sp",
                                      "per_sample", "act", "act_param"]
    # the header states the contract
    text = open(xr.HEADER).read()
    for phrase in ("Reduction order", "depend on image n alone", "Nothing outside the extents is read or written", "safe inside a captured graph",
                   "never allocate", "no pack step", "the far pads are implied by ho / wo"):
        assert phrase in text, phrase


def test_si_hip_header_declares_none_of_them():
    text = open(ct.HEADER).read()
    for name in xr.ENTRIES:
        assert name not in text, name
    assert "SiXcorrDesc" not in text and "si_hip_xcorr" not in text


def test_every_compute_entry_of_the_xcorr_header_is_driven():
    """the rule of tests/test_containment_cpu.py for include/si_hip.h, applied to include/si_xcorr.h and the view cases of the GPU file"""
    import test_gpu_xcorr as tx
    entries = [n for n in ct.header_functions(xr.HEADER) if not ct.is_exempt(n)]
    assert entries == ["si_hip_xcorr_f32", "si_hip_xcorr_f16"]
    driven = {e for c in tx.VIEW_CASES for e in c.entries}
    assert set(entries) <= driven, sorted(set(entries) - driven)
    assert driven <= set(ct.header_functions(xr.HEADER)), "a case names an entry the header does not declare"
    # every form in both types and both addressings is among the view cases
    names = {(xr.kname(c.case, c.dtype, depthwise=c.per_sample or xr.is_depthwise(c.case)), c.per_sample) for c in tx.VIEW_CASES}
    assert names == {("xcorr_%s_kernel<%s>" % (f, t), ps) for f, ps in (("dense", False), ("depthwise", False), ("depthwise", True))
                     for t in ("float", "_Float16")}


def test_the_plan_header_needs_no_device_and_there_is_no_pack_entry():
    hip_dir = os.path.join(xr.ROOT, "simpleinfer_amd", "csrc", "hip")
    src = open(os.path.join(hip_dir, "xcorr.hip")).read()
    assert '#include "xcorr_plan.h"' in src and "hipMalloc" not in src and "__shared__" not in src
    plan = re.sub(r"//[^\n]*", "", open(os.path.join(hip_dir, "xcorr_plan.h")).read())
    assert "hip" not in plan.lower() and set(re.findall(r"#include\s+[<\"]([^>\"]+)[>\"]", plan)) == {"cstdint"}
    assert not [n for n in xr.ENTRIES if "pack" in n or "weight" in n or "workspace" in n]


def test_abi_refusals_without_a_launch(native_libs):
    """every refusal happens before any device call: the addresses are made up, 16-byte aligned and 16 MiB apart"""
    H, _ = native_libs
    X, W, B, Y = (C.c_void_p((j + 1) << 24) for j in range(4))

    def desc(n=2, h=9, w=11, c=8, oc=24, kh=3, kw=3, s=2, p=1, d=1, g=1, **kw_):
        return hipops.xcorr_desc(n, h, w, c, oc, kh, kw, s, p, d, g, **kw_)

    for fn, half in (("si_hip_xcorr_f32", 0), ("si_hip_xcorr_f16", 1)):
        def call(dd, x=X, w=W, b=B, y=Y):
            return getattr(H, fn)(C.byref(dd), x, w, b, y, None)

        def name(dd, x=X, w=W, y=Y):
            return H.si_hip_xcorr_kernel_name(C.byref(dd), x, w, y, half)

        def refused(dd, code, what=""):
            assert call(dd) == code, (fn, what, call(dd))
            assert name(dd) == b"none", (fn, what)

        sfx = "_Float16" if half else "float"
        assert name(desc()) == ("xcorr_dense_kernel<%s>" % sfx).encode()
        assert name(desc(c=8, oc=8, g=8)) == ("xcorr_depthwise_kernel<%s>" % sfx).encode()
        assert name(desc(c=8, oc=8, g=8, per_sample=True)) == ("xcorr_depthwise_kernel<%s>" % sfx).encode()
        assert name(desc(c=1, oc=1)) == ("xcorr_depthwise_kernel<%s>" % sfx).encode()
        assert getattr(H, fn)(None, X, W, B, Y, None) == BADARG                                  # null descriptor
        assert call(desc(), x=None) == BADARG and call(desc(), w=None) == BADARG and call(desc(), y=None) == BADARG
        assert name(desc(), x=None) == b"none" and name(desc(), w=None) == b"none" and name(desc(), y=None) == b"none"
        assert H.si_hip_xcorr_kernel_name(None, X, W, Y, half) == b"none"
        for field in ("n", "h", "w", "c", "oc", "ho", "wo", "kh", "kw", "stride_h", "stride_w", "dilation_h", "dilation_w", "groups"):   # non-positive sizes
            for value in (0, -1):
                bad = desc()
                setattr(bad, field, value)
                refused(bad, BADARG, (field, value))
        for field in ("pad_top", "pad_left"):
            bad = desc()
            setattr(bad, field, -1)
            refused(bad, BADARG, "negative " + field)
        # ho / wo against torch's formula (h = 9, pad 1, k = 3, stride 2): 5 is what pad 1 gives, 4 what the near pad alone gives, 6 a larger
        # far pad; 3 and 1 fit no far pad
        for ho, ok in ((5, True), (4, True), (6, True), (3, False), (1, False)):
            dd = desc(ho=ho)
            dd.y_sn = dd.ho * dd.y_sh
            assert (name(dd) != b"none") == ok, (fn, ho)
            if not ok:
                refused(dd, BADARG, ("ho", ho))
        refused(desc(wo=4), BADARG, "wo")
        assert name(desc(h=3, w=3, kh=5, kw=5, s=1, p=2)) != b"none"                              # a kernel larger than the unpadded image
        refused(desc(h=3, w=3, kh=5, kw=5, s=1, p=0), BADARG, "a kernel larger than the padded image: torch's extent is 0")
        # negative strides; strides of y that let two elements share an address
        for field, value in (("x_sn", -1), ("x_sh", -88), ("w_sp", -8), ("w_sc", -1), ("y_sp", 23), ("y_sh", 6 * 24 - 1), ("y_sn", 5 * 6 * 24 - 1),
                             ("y_sn", -720)):
            bad = desc()
            setattr(bad, field, value)
            refused(bad, BADARG, (field, value))
        wide = desc(x_sp=12, x_sh=14 * 12, x_sn=9 * 14 * 12, y_sp=32, y_sh=8 * 32, y_sn=5 * 8 * 32, w_sp=16, w_sh=4 * 16, w_sn=3 * 4 * 16)
        assert name(wide) != b"none"                                                             # channel slices and gapped rows are fine
        # y overlapping x, the filter or the bias
        es = 2 if half else 4
        assert call(desc(), y=X) == BADARG and call(desc(), y=W) == BADARG and call(desc(), y=B) == BADARG
        assert call(desc(), y=C.c_void_p(X.value + 2 * 9 * 11 * 8 * es - es)) == BADARG           # y starts on x's last element
        assert call(desc(), x=C.c_void_p(Y.value + 64)) == BADARG
        # element offsets beyond 31 bits; grid extents; other group counts; per-sample filters without the depthwise form
        refused(desc(n=3, x_sn=1 << 30), UNSUPPORTED, "x offsets")
        refused(desc(n=3, y_sn=1 << 30), UNSUPPORTED, "y offsets")
        refused(desc(w_sn=1 << 27), UNSUPPORTED, "filter offsets")
        refused(desc(x_sp=1 << 31, x_sh=1 << 35, x_sn=1 << 39), UNSUPPORTED, "a stride beyond 31 bits")
        refused(desc(n=65536, h=1, w=1, c=1, oc=3, kh=1, kw=1, s=1, p=0), UNSUPPORTED, "batch beyond a grid's z")
        refused(desc(c=8, oc=8, g=2), UNSUPPORTED, "groups 2 of 8")
        refused(desc(c=8, oc=16, g=8), UNSUPPORTED, "a channel multiplier")
        refused(desc(per_sample=True), UNSUPPORTED, "per-sample dense")
        # pointers off their element
        assert name(desc(), x=C.c_void_p(X.value + 1)) == b"none" and call(desc(), w=C.c_void_p(W.value + 1)) == UNSUPPORTED
    # fp16 alone: the divisibility rule of the dense form
    d12 = desc(c=12)
    assert H.si_hip_xcorr_f16(C.byref(d12), X, W, B, Y, None) == UNSUPPORTED and H.si_hip_xcorr_kernel_name(C.byref(d12), X, W, Y, 1) == b"none"
    assert H.si_hip_xcorr_kernel_name(C.byref(d12), X, W, Y, 0) == b"xcorr_dense_kernel<float>"
    assert H.si_hip_xcorr_kernel_name(C.byref(desc(c=12, oc=12, g=12)), X, W, Y, 1) == b"xcorr_depthwise_kernel<_Float16>"
    assert H.si_hip_xcorr_kernel_name(C.byref(desc()), C.c_void_p(X.value + 2), W, Y, 1) == b"xcorr_dense_kernel<_Float16>"
    assert H.si_hip_xcorr_kernel_name(C.byref(desc()), C.c_void_p(X.value + 2), W, Y, 0) == b"none"


def test_constant_filter_is_lowered_to_conv2d_on_the_graph(native_libs, tmp_path):
    """what LoadModel does to the graph, checked on the written file without a device: build_toy_blurpool holds an nn.Conv2d operator with the
    blur filter as its weight and no F.conv2d; a tensor filter, a constant with another reader and an asymmetric 'same' stay as they are"""
    def lowered(b, tag):
        pp, bp = str(tmp_path / (tag + ".pnnx.param")), str(tmp_path / (tag + ".pnnx.bin"))
        op, ob = str(tmp_path / (tag + ".out.param")), str(tmp_path / (tag + ".out.bin"))
        b.save(pp, bp)
        engine.pnnx_save(pp, bp, op, ob, expand=True)
        return [ln.split() for ln in open(op).read().splitlines()[2:]]

    b = mg.build_toy_blurpool()
    ops = lowered(b, "blur")
    assert [o[0] for o in ops] == ["pnnx.Input", "nn.Conv2d", "nn.ReLU", "nn.Conv2d", "nn.Conv2d", "pnnx.Output"]
    conv = ops[3]
    params = dict(tok.split("=", 1) for tok in conv if "=" in tok and tok[0] not in "@#$")
    assert params == dict(bias="False", dilation="(1,1)", groups="8", in_channels="8", kernel_size="(3,3)", out_channels="8", padding="(1,1)",
                          padding_mode="zeros", stride="(2,2)"), params
    assert "@weight=(8,1,3,3)f32" in conv and conv[2:4] == ["1", "1"]
    # ... with a constant bias
    c = mg.PnnxBuilder(seed=2)
    x = c.input((2, 4, 9, 9))
    c.output(c.conv2d_functional(x, c.attribute(np.ones((6, 4, 3, 3), np.float32)), c.attribute(np.arange(6, dtype=np.float32)), padding="same"))
    ops = lowered(c, "bias")
    assert [o[0] for o in ops] == ["pnnx.Input", "nn.Conv2d", "pnnx.Output"] and "bias=True" in ops[1] and "@bias=(6)f32" in ops[1]
    # what stays: a filter with a second reader, an odd 'same' total, a tensor filter
    c = mg.PnnxBuilder(seed=2)
    x = c.input((2, 4, 9, 9))
    k = c.attribute(np.ones((4, 4, 3, 3), np.float32))
    c.output(c.conv2d_functional(c.conv2d_functional(x, k, padding=1), k, padding=1))
    assert [o[0] for o in lowered(c, "shared")] == ["pnnx.Input", "pnnx.Attribute", "F.conv2d", "F.conv2d", "pnnx.Output"]
    c = mg.PnnxBuilder(seed=2)
    c.output(c.conv2d_functional(c.input((2, 4, 9, 9)), c.attribute(np.ones((4, 4, 4, 2), np.float32)), padding="same"))
    assert [o[0] for o in lowered(c, "odd_same")] == ["pnnx.Input", "pnnx.Attribute", "F.conv2d", "pnnx.Output"]
    assert "F.conv2d" in [o[0] for o in lowered(mg.build_toy_siamfc(), "siamfc")]
    assert "F.conv2d" in [o[0] for o in lowered(mg.build_toy_dynamic_head(batch=2, constant=True), "derived")]


SANITIZE = ["-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]      # the runtimes inside the program: it starts the same under any environment


def _stand_alone(tmp_path, source, include, ok):
    exe = str(tmp_path / os.path.splitext(source)[0])
    subprocess.check_call(["g++", "-std=c++17", "-O0", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined"] + SANITIZE +
                          ["-I" + include, os.path.join(xr.ROOT, "tests", "cpp", source), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and ok in r.stdout and "runtime error" not in r.stderr, r.stdout[-4000:] + r.stderr[-4000:]


def test_plan_arithmetic_stand_alone_under_sanitizers(tmp_path):
    _stand_alone(tmp_path, "test_xcorr_plan.cpp", os.path.join(xr.ROOT, "simpleinfer_amd", "csrc", "hip"), "xcorr plan ok")


def test_batch_rule_for_tensor_filters_stand_alone_under_sanitizers(tmp_path):
    _stand_alone(tmp_path, "test_batch_rule_xcorr.cpp", os.path.join(xr.ROOT, "simpleinfer_amd", "csrc", "host"), "xcorr rule ok")
