"""CPU: nn.PixelShuffle / nn.PixelUnshuffle / nn.PReLU -- the numpy references pinned to torch bit for bit, the builder's lines and
the three toy models, the C-ABI of include/si_superres.h (exported, bound under its own table, absent from include/si_hip.h, every
compute entry driven by the GPU file's view cases), the registry, and what the entries decide without a device: the refusals by
return code and the kernel form of every row of the GPU case table."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import containment as ct
import superres_reference as sr
from ct_reference import _parse
from simpleinfer_amd import _native, engine, hipops, modelgen as mg

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "si_superres.h")


def _bits(shape, seed):
    r = np.random.Generator(np.random.Philox(seed))
    return r.integers(0, 2 ** 32, shape, dtype=np.uint32).view(np.float32)


@pytest.mark.parametrize("r", [1, 2, 3, 4])
@pytest.mark.parametrize("c", [1, 3, 4])
def test_reference_equals_torch_bit_for_bit(c, r):
    """random bit patterns (NaN payloads, -0.0, denormals), n = 2, h != w"""
    torch = pytest.importorskip("torch")
    F = torch.nn.functional
    x = _bits((2, 3, 5, c * r * r), 3 + c + 10 * r)
    t = torch.from_numpy(x).permute(0, 3, 1, 2).contiguous()
    want = F.pixel_shuffle(t, r).permute(0, 2, 3, 1).contiguous().numpy()
    got = sr.pixel_shuffle_ref(x, r)
    assert got.shape == want.shape == (2, 3 * r, 5 * r, c)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    back = sr.pixel_shuffle_ref(got, r, inverse=True)
    assert np.array_equal(back.view(np.uint32), x.view(np.uint32))                      # unshuffle of shuffle is the identity
    wantu = F.pixel_unshuffle(torch.from_numpy(got).permute(0, 3, 1, 2).contiguous(), r).permute(0, 2, 3, 1).contiguous().numpy()
    assert np.array_equal(back.view(np.uint32), wantu.view(np.uint32))
    h = got.view(np.uint16)[..., :got.shape[-1]].view(np.float16)                       # the gather is the same for every dtype
    assert np.array_equal(sr.pixel_shuffle_ref(sr.pixel_shuffle_ref(h, r, True), r).view(np.uint16), h.view(np.uint16))


def test_rule_on_one_pixel():
    x = np.arange(8, dtype=np.float32).reshape(1, 1, 1, 8)           # C = 2, r = 2: channel c r r + i r + j
    y = sr.pixel_shuffle_ref(x, 2)
    assert y.shape == (1, 2, 2, 2)
    assert y[0, :, :, 0].tolist() == [[0, 1], [2, 3]] and y[0, :, :, 1].tolist() == [[4, 5], [6, 7]]
    assert sr.out_shape((2, 6, 4, 3), 2, inverse=True) == (2, 3, 2, 12)
    with pytest.raises(AssertionError):
        sr.out_shape((1, 5, 4, 3), 2, inverse=True)


def _finite_input(shape, seed):
    r = np.random.Generator(np.random.Philox(seed))
    x = ((r.random(shape, dtype=np.float32) - np.float32(0.5)) * np.float32(8.0)).astype(np.float32)
    flat = x.reshape(-1)
    flat[1], flat[4], flat[7] = -0.0, 0.0, np.float32(1e-42)
    return x


@pytest.mark.parametrize("per_channel", [False, True], ids=["shared", "per_channel"])
@pytest.mark.parametrize("c", [1, 3, 8])
def test_prelu_reference_equals_torch_bit_for_bit(c, per_channel):
    torch = pytest.importorskip("torch")
    x = _finite_input((2, 3, 5, c), 11 + c)
    r = np.random.Generator(np.random.Philox(5))
    slope = (np.float32(0.05) + np.float32(0.35) * r.random(c if per_channel else 1, dtype=np.float32)).astype(np.float32)
    want = torch.nn.functional.prelu(torch.from_numpy(x).permute(0, 3, 1, 2).contiguous(), torch.from_numpy(slope))
    want = want.permute(0, 2, 3, 1).contiguous().numpy()
    got = sr.prelu_ref(x, slope)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.signbit(got.reshape(-1)[1]) and got.reshape(-1)[1] == 0       # -0.0 goes through the multiply
    # rank 2
    x2 = x.reshape(-1, c)
    want2 = torch.nn.functional.prelu(torch.from_numpy(x2), torch.from_numpy(slope)).numpy()
    assert np.array_equal(sr.prelu_ref(x2, slope).view(np.uint32), want2.view(np.uint32))
    # fp16: the fp32 product rounded once
    h = x.astype(np.float16)
    hf = h.astype(np.float32)
    once = np.where(hf > 0, hf, (slope * hf).astype(np.float32)).astype(np.float16)
    assert np.array_equal(sr.prelu_ref(h, slope).view(np.uint16), once.view(np.uint16))
    assert sr.prelu_ref(h, slope).dtype == np.float16
    nan = sr.prelu_ref(np.array([[np.nan, -np.inf, np.inf]], np.float32), [0.25])
    assert np.isnan(nan[0, 0]) and nan[0, 1] == -np.inf and nan[0, 2] == np.inf


def test_builder_emits_torch_keys():
    b = mg.PnnxBuilder(seed=1)
    x = b.input((2, 36, 6, 4))
    outs = [b.pixel_shuffle(x, 2), b.pixel_shuffle(x, 3, functional=True), b.pixel_unshuffle(x, 2), b.pixel_unshuffle(x, 1, functional=True),
            b.prelu(x), b.prelu(x, 36), b.leaky_relu(x, 0.2)]
    parsed = [_parse(ln) for ln in b.lines[1:]]
    assert [p[0] for p in parsed] == ["nn.PixelShuffle", "F.pixel_shuffle", "nn.PixelUnshuffle", "F.pixel_unshuffle", "nn.PReLU", "nn.PReLU",
                                      "nn.LeakyReLU"]
    assert [p[4] for p in parsed] == [dict(upscale_factor="2"), dict(upscale_factor="3"), dict(downscale_factor="2"), dict(downscale_factor="1"),
                                      dict(num_parameters="1"), dict(num_parameters="36"), dict(negative_slope="%e" % 0.2)]
    assert [b.shapes[o] for o in outs] == [(2, 9, 12, 8), (2, 4, 18, 12), (2, 144, 3, 2), (2, 36, 6, 4), (2, 36, 6, 4), (2, 36, 6, 4), (2, 36, 6, 4)]
    assert sorted(b.attrs) == ["prelu_0.weight", "prelu_1.weight"]
    assert b.attrs["prelu_0.weight"].shape == (1,) and b.attrs["prelu_1.weight"].shape == (36,)
    for w in b.attrs.values():
        assert w.dtype == np.float32 and (w >= 0.05).all() and (w < 0.4).all()
    assert "@weight=(36)f32" in b.lines[6]
    for typ, _, _, _, prm in parsed[:4]:   # the reference reads every line the builder writes
        assert sr.factor(typ, prm) in (1, 2, 3)
    with pytest.raises(AssertionError):
        b.pixel_shuffle(x, 5)
    with pytest.raises(AssertionError):
        b.pixel_unshuffle(x, 4)
    with pytest.raises(AssertionError):
        b.prelu(x, 4)


def _count(b):
    types = [ln.split()[0] for ln in b.lines]
    return {t: types.count(t) for t in set(types)}


def test_toy_espcn():
    for r in (2, 3):
        b = mg.build_toy_espcn(r=r)
        assert _count(b) == {"pnnx.Input": 1, "nn.Conv2d": 3, "nn.Tanh": 2, "nn.PixelShuffle": 1, "pnnx.Output": 1}
        assert [ln.split()[0] for ln in b.lines][-2:] == ["nn.PixelShuffle", "pnnx.Output"]
        convs = [_parse(ln)[4] for ln in b.lines if ln.startswith("nn.Conv2d")]
        assert [c["kernel_size"] for c in convs] == ["(5,5)", "(3,3)", "(3,3)"] and convs[-1]["out_channels"] == str(3 * r * r)
        y = sr.eval_graph(b, mg.synth_input((2, 16, 16, 3)))
        assert y.shape == (2, 16 * r, 16 * r, 3) and y.dtype == np.float64 and np.isfinite(y).all() and np.abs(y).max() > 0.01


def test_toy_srresnet():
    b = mg.build_toy_srresnet()
    assert _count(b) == {"pnnx.Input": 1, "nn.Conv2d": 9, "nn.PReLU": 5, "nn.BatchNorm2d": 5, "pnnx.Expression": 3, "nn.PixelShuffle": 2,
                         "nn.Tanh": 1, "pnnx.Output": 1}
    types = [ln.split()[0] for ln in b.lines]
    assert types[1:3] == ["nn.Conv2d", "nn.PReLU"] and types[-3:] == ["nn.Conv2d", "nn.Tanh", "pnnx.Output"]
    convs = [_parse(ln)[4] for ln in b.lines if ln.startswith("nn.Conv2d")]
    assert convs[0]["kernel_size"] == convs[-1]["kernel_size"] == "(9,9)"
    counts = sorted(int(_parse(ln)[4]["num_parameters"]) for ln in b.lines if ln.startswith("nn.PReLU"))
    assert counts == [1, 1, 1, 16, 16]                                     # shared and per-channel slopes both occur
    i = types.index("nn.PixelShuffle")
    assert types[i - 1] == "nn.Conv2d" and types[i + 1] == "nn.PReLU"       # conv -> PixelShuffle(2) -> PReLU
    y = sr.eval_graph(b, mg.synth_input((2, 12, 12, 3)))
    assert y.shape == (2, 48, 48, 3) and np.isfinite(y).all() and (np.abs(y) < 1.0).all() and np.abs(y).max() > 0.01
    emu = sr.eval_graph(b, mg.synth_input((2, 12, 12, 3)), rnd=sr.round_f16)
    assert 0 < np.abs(emu - y).max() < 0.05                                 # the fp16-storage emulation differs, a little


def test_toy_esrgan_head():
    b = mg.build_toy_esrgan_head()
    assert [ln.split()[0] for ln in b.lines] == ["pnnx.Input", "nn.PixelUnshuffle", "nn.Conv2d", "nn.LeakyReLU", "nn.Upsample", "nn.Conv2d",
                                                 "pnnx.Output"]
    assert b.shapes["1"] == (2, 12, 8, 8)
    y = sr.eval_graph(b, mg.synth_input((2, 16, 16, 3)))
    assert y.shape == (2, 16, 16, 3) and np.isfinite(y).all() and np.abs(y).max() > 0.01


def _declared(path):
    src = open(path).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    names = []
    for m in re.finditer(r"\b(si_[a-z0-9_]+)\s*\(", src):
        if m.group(1) not in names:
            names.append(m.group(1))
    return names


def test_header_is_exported_and_bound(native_libs):
    H, _ = native_libs
    declared = _declared(HEADER)
    assert declared == ["si_hip_pixel_shuffle_f32", "si_hip_pixel_shuffle_f16", "si_hip_pixel_shuffle_kernel_name", "si_hip_prelu_f32",
                        "si_hip_prelu_f16", "si_hip_prelu_kernel_name"]
    assert sorted(H._si_superres_signatures) == sorted(declared)
    for other in (H._si_signatures, H._si_norm_signatures, H._si_pad_signatures, H._si_pool_signatures, H._si_softmax_signatures):
        assert not set(declared) & set(other)
    raw = C.CDLL(_native.LIB_HIP_PATH)   # a handle of its own: nothing but the dynamic symbol table answers
    missing = [name for name in declared if not hasattr(raw, name)]
    assert not missing, missing
    for name in declared:
        assert getattr(H, name).argtypes is not None
    # the Python structure has the header's fields in the header's order
    m = re.search(r"typedef struct SiPixelShuffleDesc \{(.*?)\} SiPixelShuffleDesc;", open(HEADER).read(), flags=re.S)
    body = re.sub(r"/\*.*?\*/", " ", m.group(1), flags=re.S)
    fields = [f.strip() for decl in body.split(";") if decl.strip() for f in decl.strip().split(None, 1)[1].split(",")]
    assert fields == [f[0] for f in _native.SiPixelShuffleDesc._fields_], fields


def test_si_hip_header_declares_none_of_them():
    text = open(ct.HEADER).read()
    for name in _declared(HEADER):
        assert name not in text, name
    assert "si_hip_pixel_shuffle" not in text and "prelu" not in text.lower()


def test_registry_lists_the_five_type_strings(native_libs):
    types = engine.registry_types()
    for t in sr.FIVE:
        assert t in types, t
    assert "nn.GELU" not in types and "nn.ELU" not in types and "nn.ChannelShuffle" not in types


def test_every_compute_entry_of_the_superres_header_is_driven():
    """the rule of tests/test_containment_cpu.py for include/si_hip.h, applied to include/si_superres.h and the view cases of the GPU file"""
    import test_gpu_superres as tg
    entries = [n for n in ct.header_functions(HEADER) if not ct.is_exempt(n)]
    assert entries == ["si_hip_pixel_shuffle_f32", "si_hip_pixel_shuffle_f16", "si_hip_prelu_f32", "si_hip_prelu_f16"]
    driven = {e for c in tg.VIEW_CASES for e in c.entries}
    assert set(entries) <= driven, sorted(set(entries) - driven)
    assert driven <= set(ct.header_functions(HEADER)), "a case names an entry the header does not declare"
    # shuffle, unshuffle and PReLU each have aligned, odd and forced-element views in both types
    ids = {c.id for c in tg.VIEW_CASES}
    for sfx in ("f32", "f16"):
        for op in ("shuffle", "unshuffle", "prelu"):
            for kind in ("vector", "odd_stride"):
                assert "%s_%s_%s" % (op, kind, sfx) in ids


BADARG, UNSUPPORTED = -1, -2


def test_shuffle_abi_without_a_device(native_libs):
    """refusals happen before any device call (the pointers are never looked at)"""
    H, _ = native_libs
    dummy = C.c_void_p(256)
    deep, wide = (2, 3, 5, 16), (2, 6, 10, 4)
    desc = hipops.pixel_shuffle_desc
    for fn in ("si_hip_pixel_shuffle_f32", "si_hip_pixel_shuffle_f16"):
        def call(d, src=dummy, dst=dummy):
            return getattr(H, fn)(C.byref(d), src, dst, None)

        def changed(shape, factor, inverse, **fields):
            d = desc(shape, factor, inverse)
            for k, v in fields.items():
                setattr(d, k, v)
            return call(d)

        assert getattr(H, fn)(None, dummy, dummy, None) == BADARG
        assert call(desc(deep, 2), src=None) == BADARG
        assert call(desc(deep, 2), dst=None) == BADARG
        assert call(desc(deep, 2, in_ld=15)) == BADARG                     # ld < c
        assert call(desc(deep, 2, out_ld=3)) == BADARG
        assert call(desc(wide, 2, True, in_ld=3)) == BADARG
        assert call(desc(wide, 2, True, out_ld=15)) == BADARG
        for field in ("n", "ih", "iw", "ic", "oh", "ow", "oc"):            # non-positive sizes
            assert changed(deep, 2, False, **{field: 0}) == BADARG, field
            assert changed(wide, 2, True, **{field: -1}) == BADARG, field
        assert changed(deep, 2, False, r=0) == BADARG                      # r < 1
        assert changed(wide, 2, True, r=-2) == BADARG
        assert changed(deep, 2, False, oc=5, out_ld=5) == BADARG           # ic != oc r r
        assert changed(deep, 2, False, oh=7) == BADARG                     # oh != ih r
        assert changed(deep, 2, False, ow=9) == BADARG
        assert changed(deep, 2, False, r=4) == BADARG                      # the shapes are r = 2's
        assert changed(wide, 2, True, oc=12) == BADARG                     # the inverse: oc != ic r r
        assert changed(wide, 2, True, oh=2) == BADARG
        assert changed(wide, 2, True, ow=6) == BADARG
        assert call(desc((2, 7, 10, 4), 2, True)) == BADARG                # ih % r
        assert call(desc((2, 6, 9, 4), 2, True)) == BADARG                 # iw % r
        assert call(desc((65536, 2, 2, 4), 2)) == UNSUPPORTED              # n > 65535
        assert call(desc((4096, 512, 512, 4), 2)) == UNSUPPORTED           # n * oh * ow = 2^32
        assert call(desc((1, 8192, 8192, 32), 2)) == UNSUPPORTED           # element offsets of 2^31
        assert call(desc((1, 16384, 16384, 8), 2, True)) == UNSUPPORTED    # ... on the inverse's input


def test_prelu_abi_without_a_device(native_libs):
    H, _ = native_libs
    p = C.c_void_p(256)
    for fn in (H.si_hip_prelu_f32, H.si_hip_prelu_f16):
        assert fn(None, 10, 8, 8, p, 1, p, 8, None) == BADARG
        assert fn(p, 10, 8, 8, None, 1, p, 8, None) == BADARG
        assert fn(p, 10, 8, 8, p, 1, None, 8, None) == BADARG
        assert fn(p, 0, 8, 8, p, 1, p, 8, None) == BADARG                  # no pixels
        assert fn(p, 10, 0, 8, p, 1, p, 8, None) == BADARG
        assert fn(p, 10, 8, 7, p, 1, p, 8, None) == BADARG                 # ld < c
        assert fn(p, 10, 8, 8, p, 1, p, 7, None) == BADARG
        for count in (0, 2, 4, 9, -1):
            assert fn(p, 10, 8, 8, p, count, p, 8, None) == BADARG         # neither 1 nor c
        assert fn(p, 2 ** 28, 8, 8, p, 8, p, 8, None) == UNSUPPORTED       # element offsets of 2^31
        assert fn(p, 2 ** 27, 8, 8, p, 1, p, 16, None) == UNSUPPORTED
    name = hipops.prelu_kernel_name
    assert name((2, 5, 4, 8)) == name((2, 5, 4, 8), 8) == "prelu_kernel<float, 4>"
    assert name((2, 5, 4, 8), half=True) == "prelu_kernel<_Float16, 8>"
    assert name((2, 5, 4, 12), half=True) == "prelu_kernel<_Float16, 1>"
    assert name((2, 6, 7, 3)) == "prelu_kernel<float, 1>" and name((5, 64)) == "prelu_kernel<float, 4>"
    assert name((2, 5, 4, 8), in_ld=9) == "prelu_kernel<float, 1>" and name((2, 5, 4, 8), out_ld=24) == "prelu_kernel<float, 4>"
    assert name((2, 5, 4, 8), 3) == "none" and name((2, 5, 4, 8), in_ld=7) == "none"
    assert H.si_hip_prelu_kernel_name(C.c_void_p(260), 10, 8, 8, 1, C.c_void_p(256), 8, 0) == b"prelu_kernel<float, 1>"   # a pointer off 16 bytes


def test_kernel_form_of_every_row_of_the_gpu_table(native_libs):
    import test_gpu_superres as tg
    H, _ = native_libs
    name = hipops.pixel_shuffle_kernel_name
    seen = set()
    for deep, r, f32, f16 in tg.TABLE:
        wide = sr.out_shape(deep, r)
        for half, f in ((False, f32), (True, f16)):
            want = tg.form("f16" if half else "f32", f)
            assert name(deep, r, False, half) == want, (deep, r, half)
            assert name(wide, r, True, half) == want, (wide, r, half)
            seen.add(want)
    assert seen == tg.ALL_FORMS                                            # the table reaches every form the header declares
    text = open(HEADER).read()
    for form in tg.ALL_FORMS | {"prelu_kernel<T, V>", "prelu_kernel<T, 1>"}:
        assert form.replace("float", "T").replace("_Float16", "T").replace("4>", "V>").replace("8>", "V>") in text, form
    # strides and pointers
    assert name((2, 4, 6, 256), 2, in_ld=260, out_ld=72) == "pixel_shuffle_lds<float, 4>"
    assert name((2, 4, 6, 256), 2, in_ld=257) == "pixel_shuffle_elem<float>"
    assert name((2, 4, 6, 256), 2, out_ld=65) == "pixel_shuffle_elem<float>"
    assert name((2, 4, 6, 256), 2, half=True, out_ld=68) == "pixel_shuffle_elem<_Float16>"      # 68 % 8
    assert name((1, 2, 2, 48), 4, out_ld=4) == "pixel_shuffle_elem<float>"                      # C = 3 in a stride of 4: not dense
    assert name((1, 2, 2, 4096), 2) == "pixel_shuffle_elem<float>"                              # a deep pixel above 2 KiB
    assert name((1, 2, 2, 512), 2) == "pixel_shuffle_lds<float, 4>" and name((1, 2, 2, 1024), 2, half=True) == "pixel_shuffle_lds<_Float16, 8>"
    d = hipops.pixel_shuffle_desc((2, 4, 6, 256), 2)
    assert H.si_hip_pixel_shuffle_kernel_name(C.byref(d), C.c_void_p(260), C.c_void_p(256), 0) == b"pixel_shuffle_elem<float>"
    assert H.si_hip_pixel_shuffle_kernel_name(C.byref(d), C.c_void_p(256), C.c_void_p(264), 1) == b"pixel_shuffle_elem<_Float16>"
    # a descriptor the launch would refuse
    assert name((2, 7, 10, 4), 2, True) == "none" and name((2, 4, 6, 256), 2, in_ld=255) == "none"
    assert H.si_hip_pixel_shuffle_kernel_name(None, C.c_void_p(256), C.c_void_p(256), 0) == b"none"
