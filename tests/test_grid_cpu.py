"""CPU: F.grid_sample / F.affine_grid and the host side of include/si_grid.h -- the numpy rule of tests/grid_reference.py pinned to torch in
float64 (coordinates in float64) and, with its fp32 coordinates, held to torch's fp32 CPU result on bilinear; the special values of the rule;
the builder's lines, both toys' operator sequences and their float64 evaluation; the registry and the batch rule; the C-ABI (exported, bound
under its own table, absent from include/si_hip.h, the structures' fields, every compute entry driven by a view case of the GPU file); and what
is decided without a device: every refusal by return code, the kernel name by c, strides, alignment, grid source and type.  (LoadModel creates
the device context first, so the layers' refusals are held in tests/test_gpu_grid.py.)"""
import ctypes as C
import os
import re
import subprocess
import warnings

import numpy as np
import pytest

import containment as ct
import grid_reference as gr
import util
from ct_reference import _parse
from simpleinfer_amd import _native, engine, hipops, modelgen as mg

BADARG, UNSUPPORTED = -1, -2
SIZES = [((1, 1), (3, 2)), ((1, 6), (4, 5)), ((7, 1), (2, 3)), ((5, 4), (6, 7)), ((9, 11), (13, 17))]   # (h, w) of x, (ho, wo)


def _torch_sample(x_nhwc, grid, mode, pad, ac, dtype):
    import torch
    X = torch.from_numpy(np.ascontiguousarray(np.asarray(x_nhwc, dtype).transpose(0, 3, 1, 2)))
    y = torch.nn.functional.grid_sample(X, torch.from_numpy(np.asarray(grid, dtype)), mode=mode, padding_mode=pad, align_corners=ac)
    return y.numpy().transpose(0, 2, 3, 1)


@pytest.mark.parametrize("ac", [False, True], ids=["noac", "ac"])
@pytest.mark.parametrize("pad", gr.PADDINGS)
@pytest.mark.parametrize("mode", gr.MODES)
def test_rule_with_float64_coordinates_equals_torch(mode, pad, ac):
    pytest.importorskip("torch")
    worst = 0.0
    for k, ((h, w), (ho, wo)) in enumerate(SIZES):
        x = util.rng_uniform(10 + k, (2, h, w, 3), -1.0, 1.0).astype(np.float64)
        grid = gr.make_grid(20 + k, 2, ho, wo).astype(np.float64)          # out to +-2.5
        assert np.abs(grid).max() == 2.5
        got = gr.grid_sample_ref(x, grid, mode, pad, ac, coords64=True)
        want = _torch_sample(x, grid, mode, pad, ac, np.float64)
        worst = max(worst, float(np.abs(got - want).max()))
    print("%s %s ac=%d: %.3e" % (mode, pad, ac, worst))
    assert worst <= 1e-9, worst


@pytest.mark.parametrize("ac", [False, True], ids=["noac", "ac"])
def test_affine_rule_with_float64_coordinates_equals_torch(ac):
    torch = pytest.importorskip("torch")
    for k, (h, w) in enumerate([(1, 1), (1, 5), (4, 1), (6, 7), (13, 17)]):
        theta = util.rng_uniform(30 + k, (3, 2, 3), -1.5, 1.5).astype(np.float64)
        got = gr.affine_grid_ref(theta, (h, w), ac, coords64=True)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)       # (torch's note on unit-size grids under align_corners: the case is meant)
            want = torch.nn.functional.affine_grid(torch.from_numpy(theta), (3, 2, h, w), align_corners=ac).numpy()
        assert got.shape == want.shape == (3, h, w, 2)
        assert np.abs(got - want).max() <= 1e-9, (h, w, np.abs(got - want).max())
        # the fp32 rule (the kernel's base coordinates and fused multiply-adds) differs from it by fp32 rounding alone
        g32 = gr.affine_grid_ref(theta.astype(np.float32), (h, w), ac)
        assert g32.dtype == np.float32 and np.abs(g32 - got).max() <= 4 * 2.0 ** -24 * 5.5, np.abs(g32 - got).max()


@pytest.mark.parametrize("ac", [False, True], ids=["noac", "ac"])
@pytest.mark.parametrize("pad", gr.PADDINGS)
def test_fp32_coordinates_against_torch_fp32_on_bilinear(pad, ac):
    """bilinear is continuous in the coordinate, so the rule on its fp32 coordinates and torch's fp32 CPU kernel (which may contract or reorder)
    agree at the fp32 bar"""
    pytest.importorskip("torch")
    for k, ((h, w), (ho, wo)) in enumerate(SIZES):
        x = util.rng_uniform(40 + k, (2, h, w, 5), -1.0, 1.0)
        grid = gr.make_grid(50 + k, 2, ho, wo)
        got = gr.grid_sample_ref(x, grid, "bilinear", pad, ac)
        want = _torch_sample(x, grid, "bilinear", pad, ac, np.float32)
        util.assert_parity(got, want, what="%s ac=%d %dx%d" % (pad, ac, h, w))


def _one(x_hw, gy, gx, mode="bilinear", pad="zeros", ac=True):
    """x [h, w] sampled at one PIXEL position (gy, gx), given through the align_corners=True normalisation of sizes (5, 5): exact arithmetic"""
    x = np.asarray(x_hw, np.float32).reshape(1, 5, 5, 1)
    grid = np.asarray([[[[gx / 2.0 - 1.0, gy / 2.0 - 1.0]]]], np.float32)
    return gr.grid_sample_ref(x, grid, mode, pad, ac)[0, 0, 0, 0]


def test_special_values_follow_the_rule():
    x = np.arange(1, 26, dtype=np.float64).reshape(5, 5)
    # zeros padding: -1 and size are outside, -0.5 and size - 0.5 carry half the edge
    assert _one(x, -1.0, 2.0) == 0.0 and _one(x, 5.0, 2.0) == 0.0 and _one(x, 2.0, 5.0) == 0.0
    assert _one(x, -0.5, 2.0) == 0.5 * x[0, 2] and _one(x, 4.5, 2.0) == 0.5 * x[4, 2] and _one(x, 2.0, 4.5) == 0.5 * x[2, 4]
    for v in (1e30, -1e30, np.inf, -np.inf):
        for mode in gr.MODES:
            assert _one(x, v, 2.0, mode) == 0.0 and _one(x, 2.0, v, mode) == 0.0, (v, mode)
            assert _one(x, v, 2.0, mode, "border") == (x[4, 2] if v > 0 else x[0, 2]), (v, mode)
            assert np.isfinite(_one(x, v, 2.0, mode, "reflection")), (v, mode)
    # NaN: zeros padding gives NaN; border and reflection clip it to pixel 0
    for mode in gr.MODES:
        assert np.isnan(_one(x, np.nan, 2.0, mode)) and np.isnan(_one(x, 2.0, np.nan, mode))
        assert _one(x, np.nan, 2.0, mode, "border") == x[0, 2] and _one(x, np.nan, 2.0, mode, "reflection") == x[0, 2]
    # border and reflection
    assert _one(x, -1.0, 2.0, pad="border") == x[0, 2] and _one(x, 5.5, 3.0, pad="border") == x[4, 3]
    assert _one(x, -1.0, 2.0, pad="reflection") == x[1, 2] and _one(x, 5.0, 2.0, pad="reflection") == x[3, 2] and _one(x, 9.0, 2.0, pad="reflection") == x[1, 2]
    # nearest: half to even
    assert _one(x, 0.5, 2.0, "nearest") == x[0, 2] and _one(x, 1.5, 2.0, "nearest") == x[2, 2] and _one(x, 2.5, 2.0, "nearest") == x[2, 2]
    assert _one(x, 2.0, 3.5, "nearest") == x[2, 4] and _one(x, 2.0, 4.5, "nearest") == x[2, 4] and _one(x, 2.0, -0.5, "nearest") == x[2, 0]
    # Inf in x under a weight of 0: at an integer position the three neighbours have weight 0 and are multiplied where they are inside
    xi = x.copy()
    xi[2, 2] = np.inf
    assert np.isnan(_one(xi, 1.0, 1.0)) and np.isnan(_one(xi, 2.0, 1.0)) and np.isinf(_one(xi, 2.0, 2.0)) and _one(xi, 3.0, 3.0) == x[3, 3]
    xi = x.copy()
    xi[4, 4] = np.inf
    assert np.isinf(_one(xi, 4.0, 4.0)) and np.isinf(_one(xi, 9.0, 9.0, pad="border"))      # the last pixel: its neighbours outside are never read
    # reflection over a single pixel (a zero span)
    one = np.full((1, 1, 1, 2), 7.0, np.float32)
    g = np.asarray([[[[0.3, -2.0]]]], np.float32)
    assert np.array_equal(gr.grid_sample_ref(one, g, "bilinear", "reflection", True), one)
    assert np.array_equal(gr.grid_sample_ref(one, g, "nearest", "reflection", False), one)


def test_case_table_covers_every_value():
    rows = gr.CASES
    assert len(rows) == 24 and len({gr.case_id(r) for r in rows}) == 24
    assert {(r["half"], r["mode"], r["pad"], r["ac"]) for r in rows} == {(hf, m, p, a) for hf in (False, True) for m in gr.MODES for p in gr.PADDINGS
                                                                         for a in (False, True)}
    assert {r["c"] for r in rows} == {1, 2, 3, 4, 5, 8, 12, 20} and {r["n"] for r in rows} == {1, 3}
    assert {r["hw"] for r in rows} == {(1, 1), (1, 6), (7, 2), (9, 11)} and {r["out"] for r in rows} == {(2, 2), (5, 1), (13, 17)}
    for half in (False, True):
        sub = [r for r in rows if r["half"] == half]
        assert {r["c"] for r in sub} == {1, 2, 3, 4, 5, 8, 12, 20} and {r["hw"] for r in sub} == {(1, 1), (1, 6), (7, 2), (9, 11)}, half
        assert {gr.expected_kernel(r["c"], half) for r in sub} == {gr.expected_kernel(c, half) for c in ((8, 4, 2, 1) if half else (4, 1))}


# ---- graphs -----------------------------------------------------------------------------------------------------------------
def _types(b):
    return [_parse(ln)[0] for ln in b.lines]


def test_builder_lines_parse_back():
    b = mg.PnnxBuilder(seed=1)
    x, g, t = b.input((2, 5, 9, 7)), b.input((2, 4, 3, 2)), b.input((2, 2, 3))
    y = b.grid_sample(x, g, "nearest", "reflection", True)
    p = _parse(b.lines[-1])
    assert p[0] == gr.SAMPLE and p[2] == [x, g] and p[3] == [y] and p[4] == dict(align_corners="True", mode="nearest", padding_mode="reflection")
    assert b.shapes[y] == (2, 5, 4, 3)
    y2 = b.grid_sample(x, g, align_corners=None)
    assert _parse(b.lines[-1])[4] == dict(align_corners="None", mode="bilinear", padding_mode="zeros") and b.shapes[y2] == (2, 5, 4, 3)
    a = b.affine_grid(t, (2, 5, 6, 8), align_corners=False)
    p = _parse(b.lines[-1])
    assert p[0] == gr.AFFINE and p[2] == [t] and p[3] == [a] and p[4] == dict(align_corners="False", size="(2,5,6,8)") and b.shapes[a] == (2, 6, 8, 2)


def test_toys_have_the_expected_operator_sequence():
    b = mg.build_toy_stn()
    assert _types(b) == ["pnnx.Input", "nn.Conv2d", "nn.ReLU", "nn.MaxPool2d", "nn.Conv2d", "nn.AdaptiveAvgPool2d", "torch.flatten", "nn.Linear",
                         "Tensor.view", gr.AFFINE, gr.SAMPLE, "nn.Conv2d", "pnnx.Output"]
    lines = [_parse(ln) for ln in b.lines]
    lin, view, aff, smp = lines[7], lines[8], lines[9], lines[10]
    assert np.array_equal(b.attrs[lin[1] + ".bias"], [1, 0, 0, 0, 1, 0]) and view[4]["shape"] == "(2,2,3)"
    assert aff[4] == dict(align_corners="False", size="(2,3,32,32)") and aff[2] == view[3]
    assert smp[2] == [lines[0][3][0], aff[3][0]] and smp[4] == dict(align_corners="False", mode="bilinear", padding_mode="zeros")
    assert b.shapes[aff[3][0]] == (2, 32, 32, 2) and b.shapes[smp[3][0]] == (2, 3, 32, 32) and b.shapes[lines[-1][2][0]] == (2, 8, 32, 32)

    f = mg.build_toy_flow_warp()
    assert _types(f) == ["pnnx.Input", "pnnx.Input", "nn.Conv2d", "nn.Conv2d", "nn.Tanh", "pnnx.Expression", "Tensor.permute", gr.SAMPLE, "nn.Conv2d",
                         "pnnx.Output"]
    lines = [_parse(ln) for ln in f.lines]
    add, perm, smp = lines[5], lines[6], lines[7]
    assert f.shapes[lines[0][3][0]] == (2, 3, 24, 20) and f.shapes[lines[1][3][0]] == (2, 2, 24, 20)
    assert add[2] == [lines[1][3][0], lines[4][3][0]] and perm[4]["dims"] == "(0,2,3,1)" and f.shapes[perm[3][0]] == (2, 24, 20, 2)
    assert smp[2] == [lines[2][3][0], perm[3][0]] and smp[4] == dict(align_corners="True", mode="bilinear", padding_mode="border")
    assert mg.build_toy_stn(batch=3, size=16).shapes["0"] == (3, 3, 16, 16)


def test_toys_evaluate_in_float64():
    b = mg.build_toy_stn()
    x = mg.synth_input((2, 32, 32, 3))
    y = gr.eval_graph(b, x)
    assert y.shape == (2, 32, 32, 8) and np.isfinite(y).all()
    yh = gr.eval_graph(b, x, rnd=gr.round_f16)
    assert 0.0 < np.abs(yh - y).max() < 5e-2 * np.abs(y).max()
    # with a zero localisation weight theta is the identity and the sampler returns the image
    ident = mg.build_toy_stn()
    (lin,) = [_parse(ln)[1] for ln in ident.lines if ln.startswith("nn.Linear")]
    ident.attrs[lin + ".weight"][:] = 0.0
    tail = mg.PnnxBuilder(seed=0)
    tail.output(tail.conv(tail.input((2, 3, 32, 32)), 8, 3, 1, 1, name=[_parse(ln)[1] for ln in ident.lines if ln.startswith("nn.Conv2d")][-1]))
    assert np.abs(gr.eval_graph(ident, x) - gr.eval_graph(tail, x)).max() <= 1e-12

    f = mg.build_toy_flow_warp()
    img, base = mg.synth_input((2, 24, 20, 3)), mg.flow_base_grid(2, 24, 20)
    y = gr.eval_graph(f, [img, base])
    assert y.shape == (2, 24, 20, 8) and np.isfinite(y).all()
    assert 0.0 < np.abs(gr.eval_graph(f, [img, base], rnd=gr.round_f16) - y).max() < 5e-2 * np.abs(y).max()
    # the base grid alone is the identity warp under align_corners=True
    xs = util.rng_uniform(3, (2, 24, 20, 4), -1.0, 1.0)
    assert np.abs(gr.grid_sample_ref(xs, base, "bilinear", "border", True) - xs).max() <= 2e-5


def test_registry_lists_both_types(native_libs):
    assert {gr.SAMPLE, gr.AFFINE} <= set(engine.registry_types())


def test_batch_rule_has_a_row_for_both(tmp_path):
    """the stand-alone program of tests/cpp (its own table, the graphs, FollowBatchAxis) with the two type strings as its registry list"""
    host = os.path.join(gr.ROOT, "simpleinfer_amd", "csrc", "host")
    exe = str(tmp_path / "test_batch_rule")
    subprocess.check_call(["g++", "-std=c++17", "-O0", "-I" + host, os.path.join(gr.ROOT, "tests", "cpp", "test_batch_rule.cpp"), "-o", exe])
    r = subprocess.run([exe, gr.SAMPLE, gr.AFFINE], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "batch rule ok" in r.stdout and "2 registry types" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    r = subprocess.run([exe, gr.SAMPLE, "F.grid_sample_3d"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "[F.grid_sample_3d]" in r.stdout, r.stdout[-2000:]


# ---- C-ABI ------------------------------------------------------------------------------------------------------------------
def _declared(path):
    src = open(path).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    names = []
    for m in re.finditer(r"\b(si_[a-z0-9_]+)\s*\(", src):
        if m.group(1) not in names:
            names.append(m.group(1))
    return names


def test_grid_header_is_exported_and_bound(native_libs):
    H, _ = native_libs
    declared = _declared(gr.HEADER)
    assert sorted(declared) == sorted(gr.ENTRIES)
    assert sorted(H._si_grid_signatures) == sorted(declared)
    for other in (H._si_signatures, H._si_norm_signatures, H._si_pad_signatures, H._si_pool_signatures, H._si_softmax_signatures, H._si_permute_signatures,
                  H._si_attention_signatures, H._si_deform_signatures):
        assert not set(declared) & set(other)
    raw = C.CDLL(_native.LIB_HIP_PATH)   # a handle of its own: nothing but the dynamic symbol table answers
    missing = [name for name in declared if not hasattr(raw, name)]
    assert not missing, missing
    # the Python structures have the header's fields in the header's order, with the header's types
    ctypes_of = {"int": C.c_int, "long long": C.c_longlong}
    for struct in (_native.SiGridSampleDesc, _native.SiAffineGridDesc):
        m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct.__name__, struct.__name__), open(gr.HEADER).read(), flags=re.S)
        body = re.sub(r"/\*.*?\*/", " ", m.group(1), flags=re.S)
        fields = [(n.strip(), ctypes_of[typ]) for typ, names in re.findall(r"\b(int|long long)\s+([^;]+);", body) for n in names.split(",")]
        assert fields == list(struct._fields_), fields


def test_si_hip_header_declares_none_of_them():
    text = open(ct.HEADER).read()
    for name in gr.ENTRIES:
        assert name not in text, name
    assert "SiGridSampleDesc" not in text and "SiAffineGridDesc" not in text and "grid_sample" not in text and "affine_grid" not in text


def test_every_compute_entry_of_the_grid_header_is_driven():
    """the rule of tests/test_containment_cpu.py for include/si_hip.h, applied to include/si_grid.h and the view cases of the GPU file"""
    import test_gpu_grid as tg
    entries = [n for n in ct.header_functions(gr.HEADER) if not ct.is_exempt(n)]
    assert sorted(entries) == ["si_hip_affine_grid_f16", "si_hip_affine_grid_f32", "si_hip_grid_sample_f16", "si_hip_grid_sample_f32"]
    driven = {e for c in tg.VIEW_CASES for e in c.entries}
    assert set(entries) <= driven, sorted(set(entries) - driven)
    assert driven <= set(ct.header_functions(gr.HEADER)), "a case names an entry the header does not declare"


# ---- host decisions -----------------------------------------------------------------------------------------------------------
def _desc(**kw):
    args = dict(x_shape=(2, 9, 11, 8), out_hw=(13, 17))
    args.update(kw)
    return hipops.grid_sample_desc(**args)


def test_sampler_refusals_without_a_device(native_libs):
    """refusals happen before any device call"""
    H, _ = native_libs
    P = [C.c_void_p((j + 1) << 28) for j in range(3)]   # x, grid, out: 256 MiB apart

    def check(d, code, p=P, what=""):
        for half, fn in ((0, H.si_hip_grid_sample_f32), (1, H.si_hip_grid_sample_f16)):
            got = fn(C.byref(d) if d is not None else None, p[0], p[1], p[2], None)
            assert got == code, (what, half, got)
            assert H.si_hip_grid_sample_kernel_name(C.byref(d) if d is not None else None, p[0], p[1], p[2], half) == b"none", (what, half)

    check(None, BADARG, what="null descriptor")
    assert H.si_hip_grid_sample_kernel_name(C.byref(_desc()), P[0], P[1], P[2], 0) == b"grid_sample_kernel<float, 4, pair>"
    for j in range(3):
        check(_desc(), BADARG, [None if i == j else P[i] for i in range(3)], "null pointer %d" % j)
        check(_desc(theta=True), BADARG, [None if i == j else P[i] for i in range(3)], "null pointer %d, theta" % j)
    for field in ("n", "c", "h", "w", "ho", "wo"):
        for value in (0, -1):
            bad = _desc()
            setattr(bad, field, value)
            check(bad, BADARG, what=(field, value))
    for field, value in (("in_ld", 7), ("out_ld", 7), ("in_ld", -8), ("mode", 3), ("mode", -1), ("padding_mode", 3), ("padding_mode", -1), ("grid_source", 2),
                         ("grid_source", -1), ("spatial_dims", 1), ("spatial_dims", 4), ("gs_n", -2), ("gs_h", -1), ("gs_w", -2), ("gs_k", -1)):
        bad = _desc()
        setattr(bad, field, value)
        check(bad, BADARG, what=(field, value))
    neg = _desc(theta=True)                                   # (the strides are not looked at with theta)
    neg.gs_n = neg.gs_k = -5
    assert H.si_hip_grid_sample_kernel_name(C.byref(neg), P[0], P[1], P[2], 0) == b"grid_sample_kernel<float, 4, theta>"
    # the output's extent intersecting x, the grid, theta
    check(_desc(), BADARG, [P[0], P[1], P[0]], "out == x")
    check(_desc(), BADARG, [P[0], P[1], C.c_void_p(P[0].value + 64)], "out inside x")
    check(_desc(), BADARG, [P[0], P[1], C.c_void_p(P[0].value - 64)], "x inside out")
    check(_desc(), BADARG, [P[0], P[1], P[1]], "out == grid")
    check(_desc(), BADARG, [P[0], P[1], C.c_void_p(P[1].value - 2 * 13 * 17 * 8 * 2 + 2)], "the grid's first element is the output's last (fp16 extent)")
    check(_desc(theta=True), BADARG, [P[0], P[1], C.c_void_p(P[1].value + 8)], "out inside theta")
    ok = [P[0], P[1], C.c_void_p(P[1].value - 2 * 13 * 17 * 8 * 4)]          # the output ends where the grid starts
    assert H.si_hip_grid_sample_kernel_name(C.byref(_desc()), ok[0], ok[1], ok[2], 0) != b"none"
    # what the kernel does not have: bicubic, 5-D
    bad = _desc()
    bad.mode = hipops.GRID_MODE["bicubic"]
    check(bad, UNSUPPORTED, what="bicubic")
    check(_desc(spatial_dims=3), UNSUPPORTED, what="5-D")
    # beyond 31 bits: element offsets of x, out and the grid; sizes beyond 2^24 (they are used as floats)
    far = [C.c_void_p((j + 1) << 44) for j in range(3)]
    for field, value in (("in_ld", 1 << 30), ("out_ld", 1 << 30), ("gs_n", 1 << 31), ("gs_h", 1 << 28), ("gs_w", 1 << 27), ("gs_k", 1 << 31)):
        bad = _desc()
        setattr(bad, field, value)
        check(bad, UNSUPPORTED, far, what=field)
    fits = _desc()
    fits.gs_n = 1 << 30                                       # (n = 2: the last element lies at 2^30 + ..., within 31 bits)
    assert H.si_hip_grid_sample_kernel_name(C.byref(fits), far[0], far[1], far[2], 0) != b"none"
    check(hipops.grid_sample_desc((1 << 15, 256, 256, 1), (1, 1)), UNSUPPORTED, far, "2^31 input pixels")
    check(hipops.grid_sample_desc((1 << 15, 1, 1, 1), (256, 256)), UNSUPPORTED, far, "2^31 output pixels")
    check(hipops.grid_sample_desc((1, 1, (1 << 24) + 1, 1), (1, 1)), UNSUPPORTED, far, "w beyond 2^24")
    assert H.si_hip_grid_sample_kernel_name(C.byref(hipops.grid_sample_desc((1, 1, 1 << 24, 1), (1, 1))), far[0], far[1], far[2], 0) != b"none"


def test_affine_refusals_without_a_device(native_libs):
    H, _ = native_libs
    P = [C.c_void_p((j + 1) << 28) for j in range(2)]
    D = _native.SiAffineGridDesc

    def check(d, code, p=P, what=""):
        for half, fn in ((0, H.si_hip_affine_grid_f32), (1, H.si_hip_affine_grid_f16)):
            assert fn(C.byref(d) if d is not None else None, p[0], p[1], None) == code, (what, half)
            assert H.si_hip_affine_grid_kernel_name(C.byref(d) if d is not None else None, p[0], p[1], half) == b"none", (what, half)

    assert H.si_hip_affine_grid_kernel_name(C.byref(D(2, 5, 7, 0, 0)), P[0], P[1], 0) == b"affine_grid_kernel<float>"
    assert H.si_hip_affine_grid_kernel_name(C.byref(D(2, 5, 7, 9, 1)), P[0], P[1], 1) == b"affine_grid_kernel<_Float16>"
    check(None, BADARG, what="null descriptor")
    check(D(2, 5, 7, 0, 0), BADARG, [None, P[1]], "null theta")
    check(D(2, 5, 7, 0, 0), BADARG, [P[0], None], "null out")
    for bad in (D(0, 5, 7, 0, 0), D(2, 0, 7, 0, 0), D(2, 5, -1, 0, 0), D(2, 5, 7, 4, 0), D(2, 5, 7, -5, 0)):
        check(bad, BADARG, what=[getattr(bad, f) for f, _ in D._fields_])
    check(D(2, 5, 7, 0, 0), BADARG, [P[0], P[0]], "out == theta")
    check(D(2, 5, 7, 0, 0), BADARG, [P[0], C.c_void_p(P[0].value - 8)], "theta inside out")
    far = [C.c_void_p((j + 1) << 44) for j in range(2)]
    check(D(2, 5, 7, 1 << 30, 0), UNSUPPORTED, far, "out_ld")
    check(D(1 << 15, 1 << 10, 1 << 10, 0, 0), UNSUPPORTED, far, "2^35 elements")
    check(D(1, (1 << 24) + 1, 1, 0, 0), UNSUPPORTED, far, "h beyond 2^24")


def test_kernel_name_by_channels_strides_alignment_source_and_type(native_libs):
    name = hipops.grid_sample_kernel_name
    xs = lambda c: (2, 9, 11, c)
    for half in (False, True):
        for c in (1, 2, 3, 4, 5, 8, 12, 20):
            for source, kw in (("pair", {}), ("theta", dict(theta=True)), ("strided", dict(grid_strides=(2 * 17 * 13, 1, 2 * 13, 13)))):
                assert name(xs(c), (13, 17), half, **kw) == gr.expected_kernel(c, half, source), (half, c, source)
    f32 = lambda vw, src="pair": "grid_sample_kernel<float, %d, %s>" % (vw, src)
    f16 = lambda vw, src="pair": "grid_sample_kernel<_Float16, %d, %s>" % (vw, src)
    # pixel strides
    assert name(xs(8), (13, 17), in_ld=12, out_ld=16) == f32(4) and name(xs(8), (13, 17), in_ld=10) == f32(1) and name(xs(8), (13, 17), out_ld=9) == f32(1)
    assert [name(xs(8), (13, 17), True, in_ld=ld) for ld in (16, 12, 10, 9)] == [f16(8), f16(4), f16(2), f16(1)]
    assert [name(xs(8), (13, 17), True, out_ld=ld) for ld in (24, 20, 18, 11)] == [f16(8), f16(4), f16(2), f16(1)]
    # pointer alignment of x / out
    assert [name(xs(8), (13, 17), align=a) for a in (16, 8, 4)] == [f32(4), f32(1), f32(1)]
    assert [name(xs(8), (13, 17), True, align=a) for a in (16, 8, 4, 2)] == [f16(8), f16(4), f16(2), f16(1)]
    # the grid source: one load for both coordinates needs gs_k == 1, even strides and a pointer aligned to the pair
    inplace = (13 * 17 * 6, 17 * 6, 6, 1)
    assert name(xs(8), (13, 17), grid_strides=inplace) == f32(4) and name(xs(8), (13, 17), True, grid_strides=inplace) == f16(8)
    assert name(xs(8), (13, 17), grid_strides=(13 * 17 * 5, 17 * 5, 5, 1)) == f32(4, "strided")            # an odd pixel stride
    assert name(xs(8), (13, 17), grid_strides=inplace, grid_align=4) == f32(4, "strided")                    # fp32 pair: 8 bytes
    assert name(xs(8), (13, 17), True, grid_strides=inplace, grid_align=4) == f16(8)                         # fp16 pair: 4 bytes
    assert name(xs(8), (13, 17), True, grid_strides=inplace, grid_align=2) == f16(8, "strided")
    assert name(xs(8), (13, 17), grid_strides=(13 * 17 * 6, 17 * 6, 6, 2)) == f32(4, "strided")
    assert name(xs(3), (13, 17), theta=True, grid_align=2) == f32(1, "theta")                               # (theta has no alignment rule)
