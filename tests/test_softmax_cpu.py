"""CPU: nn.Softmax / nn.LogSoftmax / nn.Softmax2d / F.softmax / F.log_softmax -- the numpy rule of tests/softmax_reference.py pinned to
torch float64 on every case table, special values included (NaN positions as a mask); the builder's lines for the five spellings and
the toy builders' heads; the C-ABI of include/si_softmax.h (exported, bound under its own table, absent from include/si_hip.h, every
compute entry driven by the GPU file's view cases); the registry; and what the entries decide without a device: the refusals by return
code and the kernel form by c, the strides, the pointers' alignment and the header's thresholds."""
import ctypes as C
import re

import numpy as np
import pytest

import containment as ct
import softmax_reference as sr
import util
from ct_reference import _parse
from simpleinfer_amd import _native, engine, hipops, modelgen as mg

G, B, RA = sr.header_enum("SI_SOFTMAX_GROUP_MAX_C"), sr.header_enum("SI_SOFTMAX_BLOCK_MAX_C"), sr.header_enum("SI_SOFTMAX_STRIDED_REG_A")


def _same_with_nan_mask(got, ref, what):
    assert got.shape == ref.shape and got.dtype == ref.dtype == np.float64, what
    assert np.array_equal(np.isnan(got), np.isnan(ref)), what + ": NaN masks differ"
    ok = ~np.isnan(ref)
    inf = ok & np.isinf(ref)
    assert np.array_equal(got[inf], ref[inf]), what + ": infinities differ"
    fin = ok & ~inf
    # the two float64 statements differ by the order of a few roundings: 64 ulp of the largest value, and exact zeros where torch has them
    assert np.abs(got[fin] - ref[fin]).max(initial=0.0) <= 64 * np.finfo(np.float64).eps * max(1.0, np.abs(ref[fin]).max(initial=0.0)), what
    assert np.array_equal(got[fin] == 0.0, ref[fin] == 0.0), what + ": exact zeros differ"


@pytest.mark.parametrize("log", [False, True], ids=["softmax", "log_softmax"])
def test_rule_equals_torch_float64(log):
    pytest.importorskip("torch")
    for c in sr.contig_c():
        x = util.rng_uniform(3, (3, 1, 1, c), -4.0, 4.0)
        _same_with_nan_mask(sr.softmax_ref(x, 3, log), sr.softmax_f64_torch(x, 3, log), "c=%d" % c)
    for shape in sr.STRIDED_SHAPES_F32 + sr.STRIDED_SHAPES_F16:
        x = util.rng_uniform(4, shape, -4.0, 4.0)
        for axis in (0, 1, 2):
            _same_with_nan_mask(sr.softmax_ref(x, axis, log), sr.softmax_f64_torch(x, axis, log), "%s axis %d" % (shape, axis))
    # stability: offsets, 1e30, halves at +-60000
    x = util.rng_uniform(5, (3, 1, 1, 21), -1.0, 1.0)
    for t in (x + np.float32(100), x - np.float32(100), x * np.float32(1e30), (x * 60000).astype(np.float16)):
        got = sr.softmax_ref(t, 3, log)
        _same_with_nan_mask(got, sr.softmax_f64_torch(t, 3, log), "stability")
        assert np.isfinite(got).all()


@pytest.mark.parametrize("log", [False, True], ids=["softmax", "log_softmax"])
def test_special_values_follow_torch(log):
    pytest.importorskip("torch")
    for c in (1, 2, 5, 21, 64):
        for dtype in (np.float32, np.float16):
            x = sr.special_rows(c, dtype).reshape(8, 1, 1, c)
            got, ref = sr.softmax_ref(x, 3, log), sr.softmax_f64_torch(x, 3, log)
            _same_with_nan_mask(got, ref, "c=%d" % c)
            rows = got.reshape(8, c)
            assert np.isnan(rows[[3, 5, 6]]).all() and np.isfinite(rows[[0, 2, 4, 7]]).all(), c
            minus = np.isneginf(x.reshape(8, c)[1])
            assert (rows[1][minus] == (-np.inf if log else 0.0)).all() and np.isfinite(rows[1][~minus]).all(), c
            # the same rows along a strided axis: [1, 8 rows, c positions, 1 channel] reduced over w
            xs = np.ascontiguousarray(x.reshape(1, 8, c, 1))
            _same_with_nan_mask(sr.softmax_ref(xs, 2, log), sr.softmax_f64_torch(xs, 2, log), "strided c=%d" % c)


def test_builder_emits_torch_keys():
    b = mg.PnnxBuilder(seed=1)
    x = b.input((2, 6, 5, 7))
    outs = [b.softmax(x, 1), b.log_softmax(x, -1), b.softmax2d(x), b.softmax(x, 2, functional=True), b.log_softmax(x, -3, functional=True)]
    parsed = [_parse(ln) for ln in b.lines[1:]]
    assert [p[0] for p in parsed] == list(sr.SOFTMAX_TYPES)
    assert [p[4] for p in parsed] == [dict(dim="1"), dict(dim="-1"), {}, dict(dim="2"), dict(dim="-3")]
    assert all(b.shapes[o] == (2, 6, 5, 7) for o in outs) and not b.attrs
    assert [sr.nhwc_axis(d, 4) for d in (0, 1, 2, 3, -1, -2, -3, -4)] == [0, 3, 1, 2, 2, 1, 3, 0]
    assert [sr.nhwc_axis(d, 2) for d in (0, 1, -1, -2)] == [0, 3, 3, 0]


@pytest.mark.parametrize("build", [mg.build_toy_classifier, mg.build_toy_segnet, mg.build_toy_unet], ids=lambda f: f.__name__)
def test_toy_builders_heads(build):
    pytest.importorskip("torch")
    plain, explicit = build(), build(head=None)
    assert plain.lines == explicit.lines and sorted(plain.attrs) == sorted(explicit.attrs)
    for k in plain.attrs:
        ct.assert_same_bits(plain.attrs[k], explicit.attrs[k], k)
    n, c, h, w = plain.shapes["0"]
    x = mg.synth_input((n, h, w, c))
    base = sr.eval_graph(plain, x)
    for head, typ in (("softmax", "nn.Softmax"), ("log_softmax", "nn.LogSoftmax")):
        b = build(head=head)
        # the head is one more line in front of the output; everything before it is the headless file, byte for byte
        assert b.lines[:-2] == plain.lines[:-1] and sorted(b.attrs) == sorted(plain.attrs)
        typ_, _, ins, outs, prm = _parse(b.lines[-2])
        assert typ_ == typ and prm == dict(dim="1") and _parse(b.lines[-1])[2] == outs and ins == _parse(plain.lines[-1])[2]
        y = sr.eval_graph(b, x)
        assert y.shape == base.shape
        np.testing.assert_allclose(y, sr.softmax_ref(base, base.ndim - 1, head == "log_softmax"), rtol=0, atol=1e-12)
    with pytest.raises(AssertionError):
        build(head="softmin")


def _declared(path):
    src = open(path).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    names = []
    for m in re.finditer(r"\b(si_[a-z0-9_]+)\s*\(", src):
        if m.group(1) not in names:
            names.append(m.group(1))
    return names


def test_softmax_header_is_exported_and_bound(native_libs):
    H, _ = native_libs
    declared = _declared(sr.HEADER)
    assert declared == ["si_hip_softmax_f32", "si_hip_softmax_f16", "si_hip_softmax_kernel_name"]
    assert sorted(H._si_softmax_signatures) == sorted(declared)
    for other in (H._si_signatures, H._si_norm_signatures, H._si_pad_signatures, H._si_pool_signatures):
        assert not set(declared) & set(other)
    raw = C.CDLL(_native.LIB_HIP_PATH)   # a handle of its own: nothing but the dynamic symbol table answers
    missing = [name for name in declared if not hasattr(raw, name)]
    assert not missing, missing
    # the Python structure has the header's fields in the header's order
    m = re.search(r"typedef struct SiSoftmaxDesc \{(.*?)\} SiSoftmaxDesc;", open(sr.HEADER).read(), flags=re.S)
    body = re.sub(r"/\*.*?\*/", " ", m.group(1), flags=re.S)
    fields = [f.strip() for decl in body.split(";") if decl.strip() for f in decl.strip().split(None, 1)[1].split(",")]
    assert fields == [f[0] for f in _native.SiSoftmaxDesc._fields_], fields
    assert 64 <= G < B and RA >= 1


def test_si_hip_header_declares_none_of_them():
    text = open(ct.HEADER).read()
    for name in _declared(sr.HEADER):
        assert name not in text, name
    assert "SiSoftmaxDesc" not in text and "softmax" not in text.lower()


def test_registry_lists_the_five_type_strings(native_libs):
    types = engine.registry_types()
    for t in sr.SOFTMAX_TYPES:
        assert t in types, t
    assert "nn.Softmin" not in types and "F.softmin" not in types


def test_every_compute_entry_of_the_softmax_header_is_driven():
    """the rule of tests/test_containment_cpu.py for include/si_hip.h, applied to include/si_softmax.h and the view cases of the GPU file"""
    import test_gpu_softmax as ts
    entries = [n for n in ct.header_functions(sr.HEADER) if not ct.is_exempt(n)]
    assert entries == ["si_hip_softmax_f32", "si_hip_softmax_f16"]
    driven = {e for c in ts.VIEW_CASES for e in c.entries}
    assert set(entries) <= driven, sorted(set(entries) - driven)
    assert driven <= set(ct.header_functions(sr.HEADER)), "a case names an entry the header does not declare"


BADARG, UNSUPPORTED = -1, -2


def test_abi_without_a_device(native_libs):
    """refusals happen before any device call (the pointers are never looked at)"""
    H, _ = native_libs
    dummy = C.c_void_p(256)
    shape = (2, 5, 7, 8)
    desc = hipops.softmax_desc
    for fn in ("si_hip_softmax_f32", "si_hip_softmax_f16"):
        def call(d, src=dummy, dst=dummy):
            return getattr(H, fn)(C.byref(d), src, dst, None)

        assert getattr(H, fn)(None, dummy, dummy, None) == BADARG          # null descriptor
        assert call(desc(shape, 3), src=None) == BADARG                    # null pointers
        assert call(desc(shape, 3), dst=None) == BADARG
        for field in ("n", "h", "w", "c"):                                 # non-positive sizes
            for value in (0, -1):
                bad = desc(shape, 3)
                setattr(bad, field, value)
                assert call(bad) == BADARG, (field, value)
        assert call(desc(shape, 3, in_ld=7)) == BADARG                     # ld < c
        assert call(desc(shape, 1, out_ld=4)) == BADARG
        for axis in (-1, 4):                                               # axis outside 0 .. 3
            bad = desc(shape, 3)
            bad.axis = axis
            assert call(bad) == BADARG, axis
        for log in (-1, 2):                                                # log outside 0 / 1
            bad = desc(shape, 3)
            bad.log = log
            assert call(bad) == BADARG, log
        assert call(desc((1, 16384, 16384, 8), 3)) == UNSUPPORTED          # element offsets of 2^31
        assert call(desc((1, 1, 1 << 20, 8), 2, out_ld=1 << 11)) == UNSUPPORTED   # ... on the output side alone
        assert call(desc((65536, 65536, 1, 1), 0)) == UNSUPPORTED          # 2^32 pixels


def test_kernel_form_follows_channels_strides_pointers_and_thresholds(native_libs):
    H, _ = native_libs
    name, K = hipops.softmax_kernel_name, sr.kname
    f32, f16 = np.float32, np.float16
    assert name((2, 5, 7, 8), 3) == K("group", f32, True)
    assert name((2, 5, 7, 8), 3, half=True) == K("group", f16, True)
    assert name((2, 5, 7, 6), 3) == K("group", f32, False)
    assert name((2, 5, 7, 12), 3) == K("group", f32, True)
    assert name((2, 5, 7, 12), 3, half=True) == K("group", f16, False)      # c % 8 != 0
    assert name((2, 5, 7, 8), 3, in_ld=9) == K("group", f32, False)         # a stride that is no multiple of the vector
    assert name((2, 5, 7, 8), 3, out_ld=10) == K("group", f32, False)
    assert name((2, 5, 7, 8), 3, in_ld=16, out_ld=24) == K("group", f32, True)
    # the two thresholds of the contiguous axis, never a function of the row count
    for n in (1, 3, 130):
        for half in (False, True):
            dt = f16 if half else f32
            assert name((n, 1, 1, G), 3, half) == K("group", dt, True)
            assert name((n, 1, 1, G + 1), 3, half) == K("block", dt, False)
            assert name((n, 1, 1, G + 8), 3, half) == K("block", dt, True)
            assert name((n, 1, 1, B), 3, half) == K("block", dt, True)
            assert name((n, 1, 1, B + 1), 3, half) == K("block_online", dt, False)
            assert name((n, 1, 1, B + 4), 3, half) == K("block_online", dt, not half)
            assert name((n, 1, 1, B + 8), 3, half) == K("block_online", dt, True)
    # the strided axes: the axis length against the register threshold
    for axis, at, above in ((0, (RA, 3, 4, 8), (RA + 1, 3, 4, 8)), (1, (2, RA, 4, 8), (2, RA + 1, 4, 8)), (2, (2, 3, RA, 6), (2, 3, RA + 1, 6))):
        vec = at[3] % 4 == 0
        assert name(at, axis) == K("strided", f32, vec) and name(above, axis) == K("strided_online", f32, vec), axis
        assert name(at, axis, half=True) == K("strided", f16, at[3] % 8 == 0)
    assert name((7, 40, 3, 4), 1) == name((1, 40, 3, 4), 1) == K("strided_online", f32, True)     # n does not enter (axis != 0)
    assert name((1, 1, 1, 10), 0) == K("strided", f32, False)                                        # a rank-2 [N, F] tensor over dim 0
    d = hipops.softmax_desc((2, 5, 7, 8), 3)
    assert H.si_hip_softmax_kernel_name(C.byref(d), C.c_void_p(260), C.c_void_p(256), 0) == K("group", f32, False).encode()   # a pointer off 16 bytes
    assert H.si_hip_softmax_kernel_name(C.byref(d), C.c_void_p(256), C.c_void_p(264), 1) == K("group", f16, False).encode()
    d = hipops.softmax_desc((2, 5, 7, 8), 1)
    assert H.si_hip_softmax_kernel_name(C.byref(d), C.c_void_p(256), C.c_void_p(264), 0) == K("strided", f32, False).encode()
    assert name((2, 5, 7, 8), 4) == "none" and name((2, 5, 7, 8), 3, in_ld=7) == "none"
    assert H.si_hip_softmax_kernel_name(None, C.c_void_p(256), C.c_void_p(256), 0) == b"none"
    for shape in sr.STRIDED_SHAPES_F32:
        for axis in (0, 1, 2, 3):
            assert name(shape, axis).startswith("softmax_%s_kernel<" % sr.expected_form(shape, axis))
