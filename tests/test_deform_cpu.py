"""CPU: torchvision.ops.DeformConv2d and the deformable-conv kernel's host side -- the numpy rule of tests/deform_reference.py pinned to an
independent float64 restatement on torch (F.grid_sample per tap, an einsum) and, at zero offsets, to a float64 conv2d; special values; the
builder's line and the toy's operator sequence; the registry; the C-ABI of include/si_deform.h (exported, bound under its own table, absent from
include/si_hip.h, the structure's fields, every compute entry driven by a view case of the GPU file); and what is decided without a device:
every refusal by return code, the kernel name by alignment arm.  (LoadModel creates the device context first, so the layer's kErrorShape cases
are held in tests/test_gpu_deform.py.)"""
import ctypes as C
import re

import numpy as np
import pytest

import containment as ct
import deform_reference as dr
from ct_reference import _parse
from simpleinfer_amd import _native, engine, hipops, modelgen as mg

BADARG, UNSUPPORTED = -1, -2


def _close(got, ref, what, tol=1e-12):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = np.abs(got - ref).max() / max(1.0, np.abs(ref).max())
    assert err <= tol, "%s: %.3e" % (what, err)
    return err


@pytest.mark.parametrize("index", [1, 4, 5, 3, 10, 8])
def test_rule_equals_the_grid_sample_restatement(index):
    """on the reference's own fp32 coordinates the two agree to float64 rounding; with the coordinates summed in float64 on the torch side they
    differ by the fp32 rounding of the coordinate alone (1e-7 to 3e-7 on unit-scale data)"""
    pytest.importorskip("torch")
    c = dr.CASES[index - 1]
    x, off, m, w, b = dr.operands(c, seed=10 * index)
    ref = dr.deform_conv2d_ref(x, off, w, b, m, c[1], c[2], c[3], c[6])
    assert np.isfinite(ref).all()
    same = dr.deform_conv2d_grid_sample(x, off, w, b, m, c[1], c[2], c[3], c[6])
    _close(ref, same, "case %d, fp32 coordinates" % index)
    wide = dr.deform_conv2d_grid_sample(x, off, w, b, m, c[1], c[2], c[3], c[6], coords64=True)
    e = np.abs(ref - wide).max() / max(1.0, np.abs(ref).max())
    print("case %d: rule vs float64 coordinates %.3e" % (index, e))
    assert e <= 5e-6, e


@pytest.mark.parametrize("index", [1, 4, 5, 10])
def test_zero_offsets_and_mask_one_are_a_convolution(index):
    torch = pytest.importorskip("torch")
    c = dr.CASES[index - 1]
    x, off, m, w, b = dr.operands(c, seed=3)
    ones = None if m is None else np.ones_like(m)
    got = dr.deform_conv2d_ref(x, np.zeros_like(off), w, b, ones, c[1], c[2], c[3], c[6])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64)))
    want = torch.nn.functional.conv2d(t(x.transpose(0, 3, 1, 2)), t(w), None if b is None else t(b), c[1], c[2], c[3], c[6]).numpy().transpose(0, 2, 3, 1)
    _close(got, want, "case %d at zero offsets" % index)


def _one_tap(x_hw, dy, dx, h=4, w=5, mask=None):
    """1x1 kernel, weight 1, one channel: the output is the sample of x (an [h, w] array) at (ho + dy, wo + dx)"""
    x = np.asarray(x_hw, np.float32).reshape(1, h, w, 1)
    off = np.zeros((1, h, w, 2), np.float32)
    off[..., 0], off[..., 1] = dy, dx
    return dr.deform_conv2d_ref(x, off, np.ones((1, 1, 1, 1), np.float32), None, mask)[0, :, :, 0]


def test_special_values_follow_the_rule():
    h, w = 4, 5
    x = np.arange(1, h * w + 1, dtype=np.float64).reshape(h, w)
    ho, wo = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    # y = -1, y = H, x = W exactly -> 0
    assert np.array_equal(_one_tap(x, -1.0 - ho, 0.0), np.zeros((h, w)))
    assert np.array_equal(_one_tap(x, float(h) - ho, 0.0), np.zeros((h, w)))
    assert np.array_equal(_one_tap(x, 0.0, float(w) - wo), np.zeros((h, w)))
    # y = -0.5 and y = H - 0.5: half the weight of the edge row
    assert np.array_equal(_one_tap(x, -0.5 - ho, 0.0), 0.5 * np.broadcast_to(x[0], (h, w)))
    assert np.array_equal(_one_tap(x, h - 0.5 - ho, 0.0), 0.5 * np.broadcast_to(x[h - 1], (h, w)))
    # +-1e30 and +-Inf -> 0
    for v in (1e30, -1e30, np.inf, -np.inf):
        assert np.array_equal(_one_tap(x, v, 0.0), np.zeros((h, w))), v
        assert np.array_equal(_one_tap(x, 0.0, v), np.zeros((h, w))), v
    # an integer coordinate on the last row / column reads that pixel alone
    assert np.array_equal(_one_tap(x, 0.0, 0.0), x)
    # Inf in x under a zero weight: (ho, wo) = (1, 1) samples at an integer position, so its lower-right neighbours have weight 0; they are inside, so
    # they are multiplied -- 0 * Inf is NaN, as in torch
    xi = x.copy()
    xi[2, 2] = np.inf
    got = _one_tap(xi, 0.0, 0.0)
    want = np.zeros((h, w), bool)
    want[1:3, 1:3] = True           # every pixel whose 2x2 footprint holds (2, 2)
    assert np.array_equal(np.isnan(got) | np.isinf(got), want) and np.isinf(got[2, 2]) and np.isnan(got[1, 1])
    # the last row / column: the neighbour outside the image is never read
    xi = x.copy()
    xi[h - 1, w - 1] = np.inf
    assert np.isinf(_one_tap(xi, 0.0, 0.0)[h - 1, w - 1])


def test_a_nan_offset_poisons_its_offset_group_at_its_pixel_alone():
    for index in (4, 10, 5):
        c = dr.CASES[index - 1]
        k, s, p, d, (n, hh, ww), (ci, co), groups, og, _, _ = c
        x, off, m, w, b = dr.operands(c, seed=5)
        clean = dr.deform_conv2d_ref(x, off, w, b, m, s, p, d, groups)
        taps = k[0] * k[1]
        g, t, pix = og - 1, taps // 2, (n - 1, 1, 2)
        off = off.copy()
        off[pix + (2 * (g * taps + t) + 1,)] = np.nan                     # the dx of one tap of one offset group at one pixel
        got = dr.deform_conv2d_ref(x, off, w, b, m, s, p, d, groups)
        # the output channels fed by that offset group: those of the weight groups that hold one of its input channels
        cpo, cg, cog = ci // og, ci // groups, co // groups
        fed = np.zeros(co, bool)
        for ch in range(g * cpo, (g + 1) * cpo):
            fed[(ch // cg) * cog:(ch // cg + 1) * cog] = True
        want = np.zeros(got.shape, bool)
        want[pix] = fed
        assert np.array_equal(np.isnan(got), want), index
        assert np.array_equal(got[~want], clean[~want]), index


def test_builder_line_parses_back():
    b = mg.PnnxBuilder(seed=1)
    x, off, m = b.input((2, 8, 9, 7)), b.input((2, 36, 5, 4)), b.input((2, 18, 5, 4))
    y1 = b.deform_conv(x, off, m, cout=12, k=3, s=2, p=1, groups=2)
    y2 = b.deform_conv(x, off, cout=6, k=3, s=2, p=1, bias=False)
    p1, p2 = _parse(b.lines[-2]), _parse(b.lines[-1])
    assert p1[0] == p2[0] == dr.TYPE == "torchvision.ops.DeformConv2d"
    assert p1[2] == [x, off, m] and p2[2] == [x, off] and len(p1[3]) == len(p2[3]) == 1
    assert p1[4] == dict(bias="True", dilation="(1,1)", groups="2", in_channels="8", kernel_size="(3,3)", out_channels="12", padding="(1,1)", stride="(2,2)")
    assert p2[4] == dict(p1[4], bias="False", groups="1", out_channels="6")
    assert b.shapes[y1] == (2, 12, 5, 4) and b.shapes[y2] == (2, 6, 5, 4)
    assert b.attrs[p1[1] + ".weight"].shape == (12, 4, 3, 3) and b.attrs[p1[1] + ".bias"].shape == (12,)
    assert b.attrs[p2[1] + ".weight"].shape == (6, 8, 3, 3) and p2[1] + ".bias" not in b.attrs
    # rectangular everything
    b3 = mg.PnnxBuilder()
    y3 = b3.deform_conv(b3.input((1, 4, 9, 7)), b3.input((1, 12, 9, 4)), cout=4, k=(3, 2), s=(1, 2), p=(2, 1), d=(2, 1))
    assert b3.shapes[y3] == (1, 4, 9, 4) and _parse(b3.lines[-1])[4]["kernel_size"] == "(3,2)"


def _types(b):
    return [_parse(ln)[0] for ln in b.lines]


def test_toys_have_the_expected_operator_sequence():
    b = mg.build_toy_dcn_head()
    assert _types(b) == ["pnnx.Input", "nn.Conv2d", "nn.SiLU", "nn.Conv2d", "torch.split", "nn.Sigmoid", dr.TYPE, "nn.ReLU", "nn.Conv2d", "pnnx.Output"]
    lines = [_parse(ln) for ln in b.lines]
    split, sig, dcn = lines[4], lines[5], lines[6]
    assert split[4]["split_size_or_sections"] == "(18,9)" and [b.shapes[o][1] for o in split[3]] == [18, 9]
    assert dcn[2] == [lines[2][3][0], split[3][0], sig[3][0]]             # (x, offset: the first piece, mask: the sigmoid of the second)
    assert dcn[4]["in_channels"] == "16" and dcn[4]["out_channels"] == "24" and dcn[4]["kernel_size"] == "(3,3)" and dcn[4]["padding"] == "(1,1)"
    assert b.shapes["0"] == (2, 3, 32, 32) and b.shapes[dcn[3][0]] == (2, 24, 16, 16) and b.shapes[lines[-1][2][0]] == (2, 8, 16, 16)
    y = dr.eval_graph(b, mg.synth_input((2, 32, 32, 3)))
    assert y.shape == (2, 16, 16, 8) and np.isfinite(y).all()
    v1 = mg.build_toy_dcn_head(mask=False)
    assert _types(v1) == ["pnnx.Input", "nn.Conv2d", "nn.SiLU", "nn.Conv2d", dr.TYPE, "nn.ReLU", "nn.Conv2d", "pnnx.Output"]
    d1 = _parse(v1.lines[4])
    assert len(d1[2]) == 2 and v1.shapes[d1[2][1]] == (2, 18, 16, 16)
    y1 = dr.eval_graph(v1, mg.synth_input((2, 32, 32, 3)))
    assert y1.shape == (2, 16, 16, 8) and np.isfinite(y1).all()
    # the fp16 emulation moves the result by rounding alone
    yh = dr.eval_graph(b, mg.synth_input((2, 32, 32, 3)), rnd=dr.round_f16)
    assert 0.0 < np.abs(yh - y).max() < 5e-2 * np.abs(y).max()
    assert mg.build_toy_dcn_head(batch=3, size=16).shapes["0"] == (3, 3, 16, 16)


def test_registry_lists_deform_conv(native_libs):
    assert dr.TYPE in engine.registry_types()


def _declared(path):
    src = open(path).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    names = []
    for m in re.finditer(r"\b(si_[a-z0-9_]+)\s*\(", src):
        if m.group(1) not in names:
            names.append(m.group(1))
    return names


def test_deform_header_is_exported_and_bound(native_libs):
    H, _ = native_libs
    declared = _declared(dr.HEADER)
    assert declared == dr.ENTRIES
    assert sorted(H._si_deform_signatures) == sorted(declared)
    for other in (H._si_signatures, H._si_norm_signatures, H._si_pad_signatures, H._si_pool_signatures, H._si_softmax_signatures, H._si_permute_signatures,
                  H._si_attention_signatures):
        assert not set(declared) & set(other)
    raw = C.CDLL(_native.LIB_HIP_PATH)   # a handle of its own: nothing but the dynamic symbol table answers
    missing = [name for name in declared if not hasattr(raw, name)]
    assert not missing, missing
    # the Python structure has the header's fields in the header's order, with the header's types
    m = re.search(r"typedef struct SiDeformConv2dDesc \{(.*?)\} SiDeformConv2dDesc;", open(dr.HEADER).read(), flags=re.S)
    body = re.sub(r"/\*.*?\*/", " ", m.group(1), flags=re.S)
    ctypes_of = {"int": C.c_int, "float": C.c_float}
    fields = [(n.strip(), ctypes_of[typ]) for typ, names in re.findall(r"\b(int|float)\s+([^;]+);", body) for n in names.split(",")]
    assert fields == list(_native.SiDeformConv2dDesc._fields_), fields


def test_si_hip_header_declares_none_of_them():
    text = open(ct.HEADER).read()
    for name in dr.ENTRIES:
        assert name not in text, name
    assert "SiDeformConv2dDesc" not in text and "deform" not in text.lower()


def test_every_compute_entry_of_the_deform_header_is_driven():
    """the rule of tests/test_containment_cpu.py for include/si_hip.h, applied to include/si_deform.h and the view cases of the GPU file"""
    import test_gpu_deform as td
    entries = [n for n in ct.header_functions(dr.HEADER) if not ct.is_exempt(n)]
    assert entries == ["si_hip_deform_conv2d_f32"]
    driven = {e for c in td.VIEW_CASES for e in c.entries}
    assert set(entries) <= driven, sorted(set(entries) - driven)
    assert driven <= set(ct.header_functions(dr.HEADER)), "a case names an entry the header does not declare"


def _desc(c=dr.CASES[0], **kw):
    k, s, p, d, (n, h, w), (ci, co), g, og, mask, bias = c
    oh, ow = dr.out_hw(h, w, k, s, p, d)
    return hipops.deform_conv2d_desc((n, h, w, ci), (n, oh, ow, 2 * og * k[0] * k[1]), (co, ci // g) + tuple(k), mask, bias, s, p, d, g, **kw)


def test_abi_without_a_device(native_libs):
    """refusals happen before any device call"""
    H, _ = native_libs
    P = [C.c_void_p((j + 1) << 24) for j in range(6)]   # x, offset, mask, weight, bias, out: 16-byte aligned, 16 MiB apart
    fn = H.si_hip_deform_conv2d_f32

    def call(d, p=P):
        return fn(C.byref(d), p[0], p[1], p[2], p[3], p[4], p[5], None)

    def name(d, p=P):
        return H.si_hip_deform_conv2d_kernel_name(C.byref(d), p[0], p[1], p[2], p[5])

    def refused(d, code, p=P, what="", named=True):
        assert call(d, p) == code, (what, call(d, p))
        if named:
            assert name(d, p) == b"none", what

    assert fn(None, P[0], P[1], P[2], P[3], P[4], P[5], None) == BADARG and H.si_hip_deform_conv2d_kernel_name(None, P[0], P[1], P[2], P[5]) == b"none"
    ok = _desc()
    assert ok.has_mask == 1 and ok.has_bias == 1 and name(ok) == b"deform_conv_f32_kernel<true>"
    for j in (0, 1, 2, 5):                                                                 # null tensors
        refused(_desc(), BADARG, [None if i == j else P[i] for i in range(6)], "null %d" % j)
    for j in (3, 4):                                                                       # null weight / bias (the name does not look at them)
        refused(_desc(), BADARG, [None if i == j else P[i] for i in range(6)], "null %d" % j, named=False)
    v1 = _desc(dr.CASES[1])                                                                # without mask and bias both may be null
    assert v1.has_mask == 0 and v1.has_bias == 0 and name(v1, [P[0], P[1], None, P[3], None, P[5]]) == b"deform_conv_f32_kernel<true>"
    for field in ("n", "ih", "iw", "ic", "oc", "oh", "ow", "kh", "kw", "sh", "sw", "dh", "dw", "groups", "offset_groups"):   # non-positive sizes
        for value in (0, -1):
            bad = _desc()
            setattr(bad, field, value)
            refused(bad, BADARG, what=(field, value))
    for field in ("ph", "pw"):
        bad = _desc()
        setattr(bad, field, -1)
        refused(bad, BADARG, what=field)
    for field, value in (("groups", 3), ("offset_groups", 3)):                             # Cin % groups, Cout % groups, Cin % offset_groups
        bad = _desc(off_ld=1024, mask_ld=1024)
        setattr(bad, field, value)
        refused(bad, BADARG, what=field)
    bad = _desc(dr.CASES[3])                                                               # 36 -> 5: groups = 2 divides Cin, not Cout
    bad.groups = 2
    refused(bad, BADARG, what="Cout % groups")
    for field, value in (("in_ld", 15), ("out_ld", 15), ("off_ld", 17), ("mask_ld", 8)):   # a stride below its channel count
        bad = _desc()
        setattr(bad, field, value)
        refused(bad, BADARG, what=field)
    v1.mask_ld = 0                                                                         # (not looked at without a mask)
    assert name(v1, [P[0], P[1], None, P[3], None, P[5]]) != b"none"
    for field in ("oh", "ow"):                                                             # an output size off the formula
        bad = _desc()
        setattr(bad, field, getattr(bad, field) + 1)
        refused(bad, BADARG, what=field)
    # out intersecting an input: the same address, and an output that starts inside the input
    for j in range(3):
        refused(_desc(), BADARG, P[:5] + [P[j]], "out == input %d" % j)
    refused(_desc(), BADARG, P[:5] + [C.c_void_p(P[0].value + 64)], "out inside x")
    refused(_desc(), BADARG, P[:5] + [C.c_void_p(P[0].value - 64)], "x inside out")
    # an activation that does not exist; element offsets and a workgroup count beyond 31 bits
    bad = _desc()
    bad.act = 7
    refused(bad, UNSUPPORTED, what="act")
    far = [C.c_void_p((j + 1) << 40) for j in range(6)]
    for field in ("in_ld", "out_ld", "off_ld", "mask_ld"):
        bad = _desc()
        setattr(bad, field, 1 << 30)
        refused(bad, UNSUPPORTED, far, what=field)
    big = hipops.deform_conv2d_desc((1 << 15, 256, 256, 1), (1 << 15, 256, 256, 2), (1, 1, 1, 1))       # 2^31 pixels: the pixel index itself
    refused(big, UNSUPPORTED, far, what="pixels")
    # weight helpers: sizes alone
    assert H.si_hip_deform_conv2d_weight_elems(C.byref(_desc())) == 9 * 16 * 16
    assert H.si_hip_deform_conv2d_weight_elems(C.byref(_desc(dr.CASES[2]))) == 65 * 20         # 17 channels padded to 20
    assert H.si_hip_deform_conv2d_weight_elems(None) == 0
    bad = _desc()
    bad.groups = 3
    assert H.si_hip_deform_conv2d_weight_elems(C.byref(bad)) == 0
    assert H.si_hip_deform_conv2d_pack_weight_host(C.byref(bad), P[0], P[1]) == BADARG
    assert H.si_hip_deform_conv2d_pack_weight_host(C.byref(_desc()), None, P[1]) == BADARG


def test_packed_weight_layout(native_libs):
    """[Cout][Cin/groups][kh][kw] -> [kh][kw][Cout][Cin/groups rounded up to 4], the padding zero"""
    c = dr.CASES[4]
    w = dr.operands(c)[3]
    packed = hipops.deform_conv2d_pack(_desc(c), w)
    assert np.array_equal(packed.reshape(3, 2, 8, 4), w.transpose(2, 3, 0, 1))
    c = dr.CASES[2]
    w = dr.operands(c)[3]
    packed = hipops.deform_conv2d_pack(_desc(c), w).reshape(1, 1, 65, 20)
    assert np.array_equal(packed[..., :17], w.transpose(2, 3, 0, 1)) and not packed[..., 17:].any()


def test_kernel_name_follows_the_alignment_arm(native_libs):
    vec, scalar = "deform_conv_f32_kernel<true>", "deform_conv_f32_kernel<false>"

    def name(index, **kw):
        k, s, p, d, (n, h, w), (ci, co), g, og, mask, _ = dr.CASES[index - 1]
        oh, ow = dr.out_hw(h, w, k, s, p, d)
        return hipops.deform_conv2d_kernel_name((n, h, w, ci), (n, oh, ow, 2 * og * k[0] * k[1]), (co, ci // g) + tuple(k), mask, s, p, d, g, **kw)

    want = {1: vec, 2: vec, 3: scalar, 4: scalar, 5: scalar, 6: vec, 7: scalar, 8: vec, 9: scalar, 10: vec}
    # 3: Cin = 17; 4: 18 channels per offset group; 5: 2 channels per offset group; 7, 9: Cin = 3, 1
    assert {i: name(i) for i in want} == want
    assert name(1, in_ld=20) == vec and name(1, in_ld=18) == scalar              # a pixel stride off 16 bytes
    assert name(1, align=260) == scalar and name(1, align=272) == vec            # a pointer off 16 bytes
    assert name(10, in_ld=44) == vec
