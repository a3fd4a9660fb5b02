"""CPU: the explicit pads and nn.Tanh -- the numpy index-map reference pinned to torch.nn.functional.pad bit for bit on the accepted
set, the builder's lines and the toy CycleGAN generator, the C-ABI of include/si_pad.h (exported, bound under its own table, absent
from include/si_hip.h, every compute entry driven by the GPU file's view cases), the registry, and what the entries decide
without a device: the refusals by return code and the kernel form."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import containment as ct
import pad_reference as pr
from ct_reference import _parse
from simpleinfer_amd import engine, hipops, modelgen as mg

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PAD_HEADER = os.path.join(ROOT, "include", "si_pad.h")
SIX = ("nn.ReflectionPad2d", "nn.ReplicationPad2d", "nn.ZeroPad2d", "nn.ConstantPad2d", "nn.CircularPad2d", "F.pad")


def _bits_input(h, w, seed):
    """(1, h, w, 2) float32 from random finite values with a -0.0, an infinity and a NaN with a payload among them where there is room"""
    r = np.random.Generator(np.random.Philox(seed))
    x = (r.random((1, h, w, 2), dtype=np.float32) - np.float32(0.5)).astype(np.float32)
    flat = x.reshape(-1).view(np.uint32)
    for i, bits in enumerate((0x80000000, 0x7F800000, 0x7FC12345, 0x00000001)):
        if 2 * i + 1 < flat.size:
            flat[2 * i + 1] = bits
    return x


@pytest.mark.parametrize("hw", [(1, 1), (2, 3), (5, 4)], ids=["1x1", "2x3", "5x4"])
@pytest.mark.parametrize("mode", pr.MODES)
def test_reference_equals_torch_bit_for_bit(mode, hw):
    """every (l, r, t, b) in [-2, 4]^4 the predicate accepts: torch raises on none of them and gives the reference's bits"""
    torch = pytest.importorskip("torch")
    F = torch.nn.functional
    h, w = hw
    x = _bits_input(h, w, 3)
    t = torch.from_numpy(x).permute(0, 3, 1, 2).contiguous()
    checked = 0
    for pads in itertools.product(range(-2, 5), repeat=4):
        if not pr.accepts(h, w, pads, mode):
            continue
        ref = pr.pad2d_ref(x, pads, mode, 1.5)
        got = (F.pad(t, pads, mode, 1.5) if mode == "constant" else F.pad(t, pads, mode)).permute(0, 2, 3, 1).contiguous().numpy()
        assert got.shape == ref.shape, (pads, got.shape, ref.shape)
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (mode, hw, pads)
        checked += 1
    print("%s %dx%d: %d pad tuples accepted and compared" % (mode, h, w, checked))
    assert checked >= {"constant": 1, "replicate": 1, "reflect": 1, "circular": 1}[mode]
    if hw == (5, 4):
        assert checked > 200, checked


def test_predicate_edges():
    assert pr.accepts(4, 4, (3, 3, 3, 3), "reflect") and not pr.accepts(4, 4, (4, 0, 0, 0), "reflect")
    assert pr.accepts(4, 4, (4, 4, 4, 4), "circular") and not pr.accepts(4, 4, (5, 0, 0, 0), "circular")
    assert not pr.accepts(4, 4, (-1, 1, 0, 0), "circular")
    assert pr.accepts(5, 4, (-3, 5, -4, 6), "replicate") and not pr.accepts(5, 4, (-4, 5, 0, 0), "replicate")
    assert not pr.accepts(5, 4, (-5, 6, 0, 0), "constant") and not pr.accepts(5, 4, (-2, -2, 0, 0), "constant")
    # the rule itself on one row: a b c d
    x = np.arange(4, dtype=np.float32).reshape(1, 1, 4, 1)
    row = lambda *a: pr.pad2d_ref(x, *a).reshape(-1).tolist()
    assert row((2, 3, 0, 0), "reflect") == [2, 1, 0, 1, 2, 3, 2, 1, 0]
    assert row((2, 3, 0, 0), "replicate") == [0, 0, 0, 1, 2, 3, 3, 3, 3]
    assert row((2, 3, 0, 0), "circular") == [2, 3, 0, 1, 2, 3, 0, 1, 2]
    assert row((2, -1, 0, 0), "constant", 7.0) == [7, 7, 0, 1, 2]
    assert row((-1, 2, 0, 0), "reflect") == [1, 2, 3, 2, 1]


def test_builder_emits_torch_keys():
    b = mg.PnnxBuilder(seed=1)
    x = b.input((2, 6, 5, 7))
    outs = [b.pad(x, 2, "reflect"), b.pad(x, (1, 2, 0, 3), "replicate"), b.pad(x, (1, 1, 1, 1)), b.pad(x, (1, 0, 2, 0), "constant", 1.5),
            b.pad(x, 1, "constant", 2), b.pad(x, (5, 7, 0, 0), "circular"), b.pad(x, (1, 2), "reflect", functional=True),
            b.pad(x, (1, 2, 3, 4), "constant", None, functional=True), b.pad(x, (-1, 2, 0, 0), "constant", 0.5, functional=True), b.tanh(x)]
    parsed = [_parse(ln) for ln in b.lines[1:]]
    assert [p[0] for p in parsed] == ["nn.ReflectionPad2d", "nn.ReplicationPad2d", "nn.ZeroPad2d", "nn.ConstantPad2d", "nn.ConstantPad2d",
                                      "nn.CircularPad2d", "F.pad", "F.pad", "F.pad", "nn.Tanh"]
    assert [p[4] for p in parsed] == [dict(padding="2"), dict(padding="(1,2,0,3)"), dict(padding="(1,1,1,1)"),
                                      dict(padding="(1,0,2,0)", value="%e" % 1.5), dict(padding="1", value="2"), dict(padding="(5,7,0,0)"),
                                      dict(mode="reflect", pad="(1,2)", value="None"), dict(mode="constant", pad="(1,2,3,4)", value="None"),
                                      dict(mode="constant", pad="(-1,2,0,0)", value="%e" % 0.5), {}]
    assert [b.shapes[o] for o in outs] == [(2, 6, 9, 11), (2, 6, 8, 10), (2, 6, 7, 9), (2, 6, 7, 8), (2, 6, 7, 9), (2, 6, 5, 19), (2, 6, 5, 10),
                                          (2, 6, 12, 10), (2, 6, 5, 8), (2, 6, 5, 7)]
    assert not b.attrs
    for typ, _, _, _, prm in parsed[:-1]:   # the reference reads every line the builder writes
        pads, mode, value = pr.pad_args(typ, prm)
        assert len(pads) == 4 and mode in pr.MODES and isinstance(value, float)


def test_toy_cyclegan():
    b = mg.build_toy_cyclegan()
    types = [ln.split()[0] for ln in b.lines]
    want = {"pnnx.Input": 1, "nn.ReflectionPad2d": 6, "nn.Conv2d": 8, "nn.InstanceNorm2d": 9, "nn.ReLU": 7, "pnnx.Expression": 2,
            "nn.ConvTranspose2d": 2, "nn.Tanh": 1, "pnnx.Output": 1}
    assert {t: types.count(t) for t in set(types)} == want
    assert types[1] == "nn.ReflectionPad2d" and types[-4:] == ["nn.ReflectionPad2d", "nn.Conv2d", "nn.Tanh", "pnnx.Output"]
    assert not any(k.startswith("in_") for k in b.attrs)   # InstanceNorm2d without affine
    convs = [_parse(ln)[4] for ln in b.lines if ln.startswith("nn.Conv2d")]
    assert [c["padding"] for c in convs] == ["(0,0)", "(1,1)", "(1,1)"] + ["(0,0)"] * 5   # the padded convs themselves pad nothing
    x = mg.synth_input((2, 32, 32, 3))
    y = pr.eval_graph(b, x)
    assert y.shape == (2, 32, 32, 3) and y.dtype == np.float64 and np.isfinite(y).all()
    assert (np.abs(y) < 1.0).all() and np.abs(y).max() > 0.01
    # the pad mode reaches every explicit pad; more blocks add four lines of each kind per pair
    z = mg.build_toy_cyclegan(batch=1, size=16, blocks=3, pad="replicate")
    types = [ln.split()[0] for ln in z.lines]
    assert types.count("nn.ReplicationPad2d") == 8 and "nn.ReflectionPad2d" not in types
    assert np.isfinite(pr.eval_graph(z, mg.synth_input((1, 16, 16, 3)))).all()


def _declared(path):
    src = open(path).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    names = []
    for m in re.finditer(r"\b(si_[a-z0-9_]+)\s*\(", src):
        if m.group(1) not in names:
            names.append(m.group(1))
    return names


def test_pad_header_is_exported_and_bound(native_libs):
    H, _ = native_libs
    declared = _declared(PAD_HEADER)
    assert declared == ["si_hip_pad2d_f32", "si_hip_pad2d_f16", "si_hip_pad2d_kernel_name"]
    assert sorted(H._si_pad_signatures) == sorted(declared)
    assert not set(declared) & set(H._si_signatures) and not set(declared) & set(H._si_norm_signatures)
    from simpleinfer_amd import _native
    raw = C.CDLL(_native.LIB_HIP_PATH)   # a handle of its own: nothing but the dynamic symbol table answers
    missing = [name for name in declared if not hasattr(raw, name)]
    assert not missing, missing
    for name in declared:
        assert getattr(H, name).argtypes is not None
    # the Python structure has the header's fields in the header's order
    m = re.search(r"typedef struct SiPad2dDesc \{(.*?)\} SiPad2dDesc;", open(PAD_HEADER).read(), flags=re.S)
    body = re.sub(r"/\*.*?\*/", " ", m.group(1), flags=re.S)
    fields = [f.strip() for decl in body.split(";") if decl.strip() for f in decl.strip().split(None, 1)[1].split(",")]
    assert fields == [f[0] for f in _native.SiPad2dDesc._fields_], fields


def test_si_hip_header_declares_none_of_them():
    text = open(ct.HEADER).read()
    for name in _declared(PAD_HEADER):
        assert name not in text, name
    assert "pad2d" not in text.lower()


def test_registry_lists_the_pads_and_tanh(native_libs):
    types = engine.registry_types()
    for t in SIX + ("nn.Tanh",):
        assert t in types, t
    assert "nn.GELU" not in types and "nn.Dropout" not in types and "nn.ReflectionPad1d" not in types


def test_every_compute_entry_of_the_pad_header_is_driven():
    """the rule of tests/test_containment_cpu.py for include/si_hip.h, applied to include/si_pad.h and the view cases of the GPU file"""
    import test_gpu_pad as tp
    entries = [n for n in ct.header_functions(PAD_HEADER) if not ct.is_exempt(n)]
    assert entries == ["si_hip_pad2d_f32", "si_hip_pad2d_f16"]
    driven = {e for c in tp.VIEW_CASES for e in c.entries}
    assert set(entries) <= driven, sorted(set(entries) - driven)
    assert driven <= set(ct.header_functions(PAD_HEADER)), "a case names an entry the header does not declare"


BADARG, UNSUPPORTED = -1, -2


def test_abi_without_a_device(native_libs):
    """refusals happen before any device call (the pointers are never looked at)"""
    H, _ = native_libs
    dummy = C.c_void_p(256)
    shape = (2, 5, 4, 8)

    for fn in ("si_hip_pad2d_f32", "si_hip_pad2d_f16"):
        def call(d, src=dummy, dst=dummy):
            return getattr(H, fn)(C.byref(d), src, dst, None)

        assert getattr(H, fn)(None, dummy, dummy, None) == BADARG
        assert call(hipops.pad2d_desc(shape, (1, 1, 1, 1)), src=None) == BADARG
        assert call(hipops.pad2d_desc(shape, (1, 1, 1, 1)), dst=None) == BADARG
        assert call(hipops.pad2d_desc(shape, (1, 1, 1, 1), in_ld=7)) == BADARG                 # ld < c
        assert call(hipops.pad2d_desc(shape, (1, 1, 1, 1), out_ld=4)) == BADARG
        bad = hipops.pad2d_desc(shape, (1, 1, 1, 1))
        bad.mode = 4
        assert call(bad) == BADARG
        bad.mode = -1
        assert call(bad) == BADARG
        bad = hipops.pad2d_desc(shape, (1, 1, 1, 1))
        bad.oh += 1                                                                            # oh inconsistent with the pads
        assert call(bad) == BADARG
        bad = hipops.pad2d_desc(shape, (1, 1, 1, 1))
        bad.ow -= 1
        assert call(bad) == BADARG
        assert call(hipops.pad2d_desc(shape, (-2, -2, 0, 0))) == BADARG                        # ow = 0: a non-positive size
        bad = hipops.pad2d_desc(shape, (0, 0, 0, 0))
        bad.c = 0
        assert call(bad) == BADARG
        assert call(hipops.pad2d_desc(shape, (4, 0, 0, 0), "reflect")) == UNSUPPORTED          # reflect with pad = size (iw = 4)
        assert call(hipops.pad2d_desc(shape, (0, 0, 0, 5), "reflect")) == UNSUPPORTED          # ... and in H (ih = 5)
        assert call(hipops.pad2d_desc(shape, (-1, 2, 0, 0), "circular")) == UNSUPPORTED        # circular with a negative pad
        assert call(hipops.pad2d_desc(shape, (5, 0, 0, 0), "circular")) == UNSUPPORTED         # circular with pad = size + 1
        assert call(hipops.pad2d_desc(shape, (0, 0, 6, 0), "circular")) == UNSUPPORTED
        for mode in ("constant", "replicate"):
            assert call(hipops.pad2d_desc(shape, (-4, 5, 0, 0), mode)) == UNSUPPORTED          # a crop that leaves nothing
            assert call(hipops.pad2d_desc(shape, (0, 0, 2, -5), mode)) == UNSUPPORTED
        assert call(hipops.pad2d_desc((65536, 128, 128, 8), (64, 64, 0, 0))) == UNSUPPORTED    # n > 65535, n * oh * ow = 2^31
        assert call(hipops.pad2d_desc((4096, 512, 512, 8), (512, 0, 0, 0))) == UNSUPPORTED     # n * oh * ow = 2^31
        assert call(hipops.pad2d_desc((1, 16384, 16384, 8), (0, 0, 0, 0))) == UNSUPPORTED      # element offsets of 2^31


def test_kernel_form_follows_channels_strides_and_pointers(native_libs):
    H, _ = native_libs
    name = hipops.pad2d_kernel_name
    assert name((3, 16, 16, 64), (1, 1, 1, 1), "reflect") == "pad2d_kernel<float, 4>"
    assert name((3, 16, 16, 64), (1, 1, 1, 1), "reflect", half=True) == "pad2d_kernel<_Float16, 8>"
    assert name((2, 6, 7, 3), (3, 3, 3, 3), "reflect") == "pad2d_kernel<float, 1>"             # the RGB stem
    assert name((1, 9, 5, 21), (1, 2, 2, 1), "replicate") == "pad2d_kernel<float, 1>"
    assert name((2, 8, 8, 12), (1, 1, 1, 1)) == "pad2d_kernel<float, 4>"
    assert name((2, 8, 8, 12), (1, 1, 1, 1), half=True) == "pad2d_kernel<_Float16, 1>"         # c % 8 != 0
    assert name((2, 5, 4, 8), (1, 1, 1, 1), in_ld=9) == "pad2d_kernel<float, 1>"               # a stride that is no multiple of the vector
    assert name((2, 5, 4, 8), (1, 1, 1, 1), out_ld=10) == "pad2d_kernel<float, 1>"
    assert name((2, 5, 4, 8), (1, 1, 1, 1), in_ld=16, out_ld=24) == "pad2d_kernel<float, 4>"
    assert name((2, 5, 4, 8), (1, 1, 1, 1), half=True, in_ld=12) == "pad2d_kernel<_Float16, 1>"
    d = hipops.pad2d_desc((2, 5, 4, 8), (1, 1, 1, 1))
    assert H.si_hip_pad2d_kernel_name(C.byref(d), C.c_void_p(260), C.c_void_p(256), 0) == b"pad2d_kernel<float, 1>"   # a pointer off 16 bytes
    assert H.si_hip_pad2d_kernel_name(C.byref(d), C.c_void_p(256), C.c_void_p(264), 1) == b"pad2d_kernel<_Float16, 1>"
    # a descriptor the launch would refuse
    assert name((2, 5, 4, 8), (4, 0, 0, 0), "reflect") == "none"
    assert name((2, 5, 4, 8), (-1, 1, 0, 0), "circular") == "none"
    assert name((2, 5, 4, 8), (1, 1, 1, 1), in_ld=7) == "none"
    assert H.si_hip_pad2d_kernel_name(None, C.c_void_p(256), C.c_void_p(256), 0) == b"none"
