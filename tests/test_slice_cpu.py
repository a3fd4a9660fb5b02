"""CPU: torch.chunk / torch.split / Tensor.slice -- the numpy rules pinned to torch on CPU bit for bit, the builder's lines and the four toy
models, the C-ABI of include/si_slice.h (exported, bound under its own table, absent from include/si_hip.h, every compute entry driven by
the GPU file's view cases), the registry, and what the entries decide without a device: the refusals by return code and the kernel form
of every row of the GPU case tables."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import containment as ct
import slice_reference as sl
from ct_reference import _parse
from simpleinfer_amd import _native, engine, hipops, modelgen as mg

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "si_slice.h")
ALL = slice(None)


def _bits(shape, seed):
    r = np.random.Generator(np.random.Philox(seed))
    return r.integers(0, 2 ** 32, shape, dtype=np.uint32).view(np.float32)


def _nchw(x):
    torch = pytest.importorskip("torch")
    return torch.from_numpy(x).permute(0, 3, 1, 2).contiguous() if x.ndim == 4 else torch.from_numpy(x)


def _nhwc(t):
    return (t.permute(0, 2, 3, 1) if t.dim() == 4 else t).contiguous().numpy()


def _same(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for g, w in zip(got, want):
        w = _nhwc(w)
        assert g.shape == w.shape and g.flags.c_contiguous, (g.shape, w.shape)
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32))


@pytest.mark.parametrize("dim", [0, 1, 2, 3, -1, -3])
def test_chunk_and_split_rules_equal_torch_bit_for_bit(dim):
    """random bit patterns (NaN payloads, -0.0, denormals); among the cases the uneven chunks=3 of 8 channels, which gives 3 + 3 + 2, a
    chunk count that gives fewer pieces than asked for, and an int split_size with a short tail"""
    torch = pytest.importorskip("torch")
    x = _bits((4, 5, 6, 8), 3 + dim)       # NHWC; NCHW (4, 8, 5, 6)
    t = _nchw(x)
    for chunks in (1, 2, 3, 4, 5, 8, 9):
        _same(sl.chunk_ref(x, chunks, dim), torch.chunk(t, chunks, dim))
    size = t.shape[dim]
    for ss in (1, 2, 3, size - 1, size, size + 3):
        if ss >= 1:
            _same(sl.split_ref(x, ss, dim), torch.split(t, ss, dim))
    _same(sl.split_ref(x, [1, size - 1], dim), torch.split(t, [1, size - 1], dim))
    assert [p.shape[3] for p in sl.chunk_ref(x, 3, 1)] == [3, 3, 2]
    assert [p.shape[3] for p in sl.chunk_ref(x, 5, 1)] == [2, 2, 2, 2]             # ceil(8 / 5) = 2: four pieces, not five
    assert [p.shape[3] for p in sl.split_ref(x, 3, 1)] == [3, 3, 2]
    x2 = _bits((5, 21), 9)
    _same(sl.chunk_ref(x2, 4, 1), torch.chunk(torch.from_numpy(x2), 4, 1))
    _same(sl.split_ref(x2, [5, 16], -1), torch.split(torch.from_numpy(x2), [5, 16], -1))
    with pytest.raises(AssertionError):
        sl.split_ref(x, [3, 4], 1)


def test_slice_rule_equals_python_slicing_on_torch():
    pytest.importorskip("torch")
    x = _bits((3, 7, 9, 8), 21)
    t = _nchw(x)                           # (3, 8, 7, 9)
    E = sl.OPEN_END
    _same([sl.slice_ref(x, 1, 2, 6, 1)], [t[:, 2:6]])
    _same([sl.slice_ref(x, 1, -6, -1, 2)], [t[:, -6:-1:2]])                         # negative indices wrap
    _same([sl.slice_ref(x, 1, 1, E, 3)], [t[:, 1::3]])                              # pnnx's open end
    _same([sl.slice_ref(x, 2, 0, 100, 1)], [t[:, :, 0:100]])                        # an end past the size
    _same([sl.slice_ref(x, -1, -100, None, 2)], [t[..., -100::2]])                  # a start before the beginning
    _same([sl.slice_ref(x, 0, 1, 2, 1)], [t[1:2]])
    _same([sl.slice_ref(x, (2, 3), (1, 0), (E, E), (2, 2))], [t[..., 1::2, 0::2]])  # a Focus slice
    _same([sl.slice_ref(x, (1, 3, 2), (4, 2, 1), (8, 7, 4), (1, 1, 1))], [t[:, 4:8, 1:4, 2:7]])
    x2 = _bits((4, 20), 22)
    _same([sl.slice_ref(x2, 1, 5, -5, 1)], [_nchw(x2)[:, 5:-5]])
    h = x.view(np.uint16)[..., :8].view(np.float16)                                 # the index is the same for every dtype
    assert np.array_equal(sl.slice_ref(h, 1, 2, 6, 1).view(np.uint16), h[..., 2:6].view(np.uint16))
    assert sl.nhwc_axis(1, 4) == 3 and sl.nhwc_axis(-1, 4) == 2 and sl.nhwc_axis(2, 4) == 1 and sl.nhwc_axis(1, 2) == 1


def test_builder_emits_pnnx_keys():
    b = mg.PnnxBuilder(seed=1)
    x = b.input((2, 8, 6, 4))
    outs = [b.chunk(x, 3, 1), b.split(x, 3, 1), b.split(x, (5, 3), -3), b.chunk(x, 2, 2)]
    s1 = b.slice(x, 1, 2, 6, 1)
    s2 = b.slice(x, (2, 3), (1, 0), (None, None), (2, 2))
    s3 = b.slice(x, -1, -3, "None", 1)
    parsed = [_parse(ln) for ln in b.lines[1:]]
    assert [p[0] for p in parsed] == ["torch.chunk", "torch.split", "torch.split", "torch.chunk", "Tensor.slice", "Tensor.slice", "Tensor.slice"]
    assert [p[4] for p in parsed] == [dict(chunks="3", dim="1"), dict(dim="1", split_size_or_sections="3"),
                                      dict(dim="-3", split_size_or_sections="(5,3)"), dict(chunks="2", dim="2"),
                                      dict(dim="1", end="6", start="2", step="1"),
                                      dict(dims="(2,3)", ends="(2147483647,2147483647)", starts="(1,0)", steps="(2,2)"),
                                      dict(dim="-1", end="None", start="-3", step="1")]
    assert [[b.shapes[o] for o in os_] for os_ in outs] == [[(2, 3, 6, 4), (2, 3, 6, 4), (2, 2, 6, 4)], [(2, 3, 6, 4), (2, 3, 6, 4), (2, 2, 6, 4)],
                                                           [(2, 5, 6, 4), (2, 3, 6, 4)], [(2, 8, 3, 4), (2, 8, 3, 4)]]
    assert [b.shapes[o] for o in (s1, s2, s3)] == [(2, 4, 6, 4), (2, 8, 3, 2), (2, 8, 6, 3)]
    assert [len(p[3]) for p in parsed] == [3, 3, 2, 2, 1, 1, 1]                       # one output operand per piece on the line
    xv = _bits((2, 6, 4, 8), 5)
    for typ, _, _, os_, prm in parsed:                                               # the reference reads every line the builder writes
        ys = sl.apply_line(typ, prm, xv)
        assert [(y.shape[0], y.shape[3], y.shape[1], y.shape[2]) for y in ys] == [b.shapes[o] for o in os_]
    with pytest.raises(AssertionError):
        b.split(x, (5, 4), 1)
    with pytest.raises(AssertionError):
        b.slice(x, 1, 6, 2, 1)


def _types(b):
    return [ln.split()[0] for ln in b.lines]


def _count(b):
    t = _types(b)
    return {k: t.count(k) for k in set(t)}


def test_toy_c2f():
    for n in (1, 2):
        b = mg.build_toy_c2f(n=n)
        assert _count(b) == {"pnnx.Input": 1, "nn.Conv2d": 2 + 2 * n, "nn.SiLU": 2 + 2 * n, "torch.chunk": 1, "pnnx.Expression": n, "torch.cat": 1,
                             "pnnx.Output": 1}
        t = _types(b)
        assert t[1:4] == ["nn.Conv2d", "nn.SiLU", "torch.chunk"] and t[-4:] == ["torch.cat", "nn.Conv2d", "nn.SiLU", "pnnx.Output"]
        chunk = [_parse(ln) for ln in b.lines if ln.startswith("torch.chunk")][0]
        cat = [_parse(ln) for ln in b.lines if ln.startswith("torch.cat")][0]
        assert chunk[4] == dict(chunks="2", dim="1") and cat[2][:2] == chunk[3] and len(cat[2]) == 2 + n     # both halves lead the concat
        assert [b.shapes[o] for o in chunk[3]] == [(2, 16, 16, 16)] * 2 and b.shapes[cat[3][0]] == (2, 16 * (2 + n), 16, 16)
        y = sl.eval_graph(b, mg.synth_input((2, 16, 16, 16)))
        assert y.shape == (2, 16, 16, 32) and y.dtype == np.float64 and np.isfinite(y).all() and np.abs(y).max() > 0.01
    emu = sl.eval_graph(b, mg.synth_input((2, 16, 16, 16)), rnd=sl.round_f16)
    assert 0 < np.abs(emu - y).max() < 0.05                                           # the fp16-storage emulation differs, a little


def test_toy_focus():
    b = mg.build_toy_focus()
    assert _types(b) == ["pnnx.Input"] + ["Tensor.slice"] * 4 + ["torch.cat", "nn.Conv2d", "nn.SiLU", "pnnx.Output"]
    prm = [_parse(ln)[4] for ln in b.lines if ln.startswith("Tensor.slice")]
    assert [p["starts"] for p in prm] == ["(0,0)", "(1,0)", "(0,1)", "(1,1)"]          # YOLOv5's order: x[..., i::2, j::2]
    assert all(p["dims"] == "(2,3)" and p["steps"] == "(2,2)" for p in prm)
    assert b.shapes["1"] == (2, 3, 8, 8) and b.shapes["5"] == (2, 12, 8, 8)
    x = mg.synth_input((2, 16, 16, 3))
    parts = [sl.apply_line("Tensor.slice", p, x)[0] for p in prm]
    assert np.array_equal(parts[1], x[:, 1::2, 0::2, :]) and np.array_equal(parts[2], x[:, 0::2, 1::2, :])
    y = sl.eval_graph(b, x)
    assert y.shape == (2, 8, 8, 16) and np.isfinite(y).all() and np.abs(y).max() > 0.01


def test_toy_res2net_block():
    b = mg.build_toy_res2net_block()
    assert _count(b) == {"pnnx.Input": 1, "nn.Conv2d": 6, "nn.ReLU": 6, "torch.split": 1, "pnnx.Expression": 3, "torch.cat": 1, "pnnx.Output": 1}
    split = [_parse(ln) for ln in b.lines if ln.startswith("torch.split")][0]
    cat = [_parse(ln) for ln in b.lines if ln.startswith("torch.cat")][0]
    assert split[4] == dict(dim="1", split_size_or_sections="8") and len(split[3]) == 4
    assert [b.shapes[o] for o in split[3]] == [(2, 8, 12, 12)] * 4
    assert cat[2][-1] == split[3][-1] and not set(cat[2][:-1]) & set(split[3])         # the last piece passes through, the others go through convs
    y = sl.eval_graph(b, mg.synth_input((2, 12, 12, 3)))
    assert y.shape == (2, 12, 12, 32) and np.isfinite(y).all() and np.abs(y).max() > 0.01


def test_toy_ghost():
    b = mg.build_toy_ghost()
    assert _types(b) == ["pnnx.Input", "nn.Conv2d", "nn.ReLU", "nn.Conv2d", "nn.ReLU", "torch.cat", "Tensor.slice", "pnnx.Output"]
    convs = [_parse(ln)[4] for ln in b.lines if ln.startswith("nn.Conv2d")]
    assert convs[0]["out_channels"] == convs[1]["out_channels"] == convs[1]["groups"] == "14" and convs[1]["kernel_size"] == "(3,3)"
    assert _parse(b.lines[-2])[4] == dict(dim="1", end="27", start="0", step="1")      # out[:, :oup] of 28 channels
    y = sl.eval_graph(b, mg.synth_input((2, 16, 16, 16)))
    assert y.shape == (2, 16, 16, 27) and np.isfinite(y).all() and y.min() >= 0 and y.max() > 0.01


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
    assert declared == ["si_hip_slice_f32", "si_hip_slice_f16", "si_hip_slice_kernel_name", "si_hip_split_channels_f32",
                        "si_hip_split_channels_f16", "si_hip_split_channels_kernel_name"]
    assert sorted(H._si_slice_signatures) == sorted(declared)
    for other in (H._si_signatures, H._si_norm_signatures, H._si_pad_signatures, H._si_pool_signatures, H._si_softmax_signatures,
                  H._si_superres_signatures):
        assert not set(declared) & set(other)
    raw = C.CDLL(_native.LIB_HIP_PATH)   # a handle of its own: nothing but the dynamic symbol table answers
    missing = [name for name in declared if not hasattr(raw, name)]
    assert not missing, missing
    for name in declared:
        assert getattr(H, name).argtypes is not None
    # the Python structure has the header's fields in the header's order, the two arrays with their lengths
    text = open(HEADER).read()
    m = re.search(r"typedef struct SiSliceDesc \{(.*?)\} SiSliceDesc;", text, flags=re.S)
    body = re.sub(r"/\*.*?\*/", " ", m.group(1), flags=re.S)
    fields = [f.strip() for decl in body.split(";") if decl.strip() for f in decl.strip().split(None, 1)[1].split(",")]
    have = ["%s[%d]" % (n, t._length_) if hasattr(t, "_length_") else n for n, t in _native.SiSliceDesc._fields_]
    assert fields == have, fields
    assert C.sizeof(_native.SiSliceDesc) == 18 * 4
    assert int(re.search(r"#define SI_SPLIT_MAX (\d+)", text).group(1)) == 8


def test_si_hip_header_declares_none_of_them():
    text = open(ct.HEADER).read()
    for name in _declared(HEADER):
        assert name not in text, name
    assert "si_hip_slice" not in text and "split_channels" not in text


def test_registry_lists_the_three_type_strings(native_libs):
    types = engine.registry_types()
    for t in sl.THREE:
        assert t in types, t
    for t in ("nn.GELU", "nn.ELU", "nn.ChannelShuffle", "nn.Dropout", "nn.Softmin", "nn.AdaptiveMaxPool2d", "torch.tensor_split", "torch.unbind",
              "Tensor.select", "Tensor.narrow"):
        assert t not in types, t


def test_every_compute_entry_of_the_slice_header_is_driven():
    """the rule of tests/test_containment_cpu.py for include/si_hip.h, applied to include/si_slice.h and the view cases of the GPU file"""
    import test_gpu_slice as tg
    entries = [n for n in ct.header_functions(HEADER) if not ct.is_exempt(n)]
    assert entries == ["si_hip_slice_f32", "si_hip_slice_f16", "si_hip_split_channels_f32", "si_hip_split_channels_f16"]
    driven = {e for c in tg.VIEW_CASES for e in c.entries}
    assert set(entries) <= driven, sorted(set(entries) - driven)
    assert driven <= set(ct.header_functions(HEADER)), "a case names an entry the header does not declare"
    # the slice and the split each have aligned, 4-bytes-off and odd views in both types
    ids = {c.id for c in tg.VIEW_CASES}
    for sfx in ("f32", "f16"):
        for cid in ("slice_vector", "slice_odd_stride", "slice_off_4_bytes", "slice_focus", "split_vector", "split_off_4_bytes", "split_odd"):
            assert "%s_%s" % (cid, sfx) in ids
    for c in tg.VIEW_CASES:                # every view is a real one: a stride wider than the channels on both sides
        if isinstance(c, tg.SliceView):
            assert c.views["in_ld"] > c.s[3] and c.views["out_ld"] > c.reference()[0].shape[3], c.id
        else:
            assert c.views["in_ld"] > c.s[3] and all(ld > w for ld, w in zip(c.views["out_lds"], c.widths)), c.id


BADARG, UNSUPPORTED = -1, -2


def test_slice_abi_without_a_device(native_libs):
    """refusals happen before any device call (the pointers are never looked at)"""
    H, _ = native_libs
    dummy = C.c_void_p(256)
    s = (2, 7, 9, 16)
    index = (ALL, slice(1, 6, 2), slice(2, 9), slice(4, 12))
    for fn in ("si_hip_slice_f32", "si_hip_slice_f16"):
        def call(d, src=dummy, dst=dummy):
            return getattr(H, fn)(C.byref(d), src, dst, None)

        def changed(idx=index, shape=s, **fields):
            d = hipops.slice_desc(shape, idx)
            for k, v in fields.items():
                if isinstance(v, tuple):
                    getattr(d, k)[v[0]] = v[1]
                else:
                    setattr(d, k, v)
            return call(d)

        assert getattr(H, fn)(None, dummy, dummy, None) == BADARG
        assert call(hipops.slice_desc(s, index), src=None) == BADARG
        assert call(hipops.slice_desc(s, index), dst=None) == BADARG
        assert call(hipops.slice_desc(s, index, in_ld=15)) == BADARG       # ld < c
        assert call(hipops.slice_desc(s, index, out_ld=7)) == BADARG
        for field in ("n", "ih", "iw", "ic", "on", "oh", "ow", "oc"):       # non-positive sizes
            assert changed(**{field: 0}) == BADARG, field
            assert changed(**{field: -1}) == BADARG, field
        for a in range(4):
            assert changed(step=(a, 0)) == BADARG                           # a step below 1
            assert changed(step=(a, -1)) == BADARG
            assert changed(start=(a, -1)) == BADARG                         # a start before the input
            assert changed(start=(a, s[a])) == BADARG                       # ... and behind it
        assert changed(oh=4) == BADARG                                      # 1 + 3 * 2 = 7: one row past the input
        assert changed(ow=8) == BADARG                                      # 2 + 7 = 9
        assert changed(oc=13, out_ld=13) == BADARG                          # 4 + 12 = 16
        assert changed(on=3) == BADARG
        assert changed(step=(3, 2)) == BADARG                               # 4 + 7 * 2 = 18
        assert changed(step=(1, 3)) == BADARG                               # 1 + 2 * 3 = 7
        assert call(hipops.slice_desc((65536, 2, 2, 4), (ALL,))) == UNSUPPORTED               # n > 65535
        assert call(hipops.slice_desc((4096, 1024, 512, 4), (ALL,))) == UNSUPPORTED           # n h w = 2^31
        assert call(hipops.slice_desc((1, 8192, 8192, 32), (ALL,))) == UNSUPPORTED            # element offsets of 2^31
        assert call(hipops.slice_desc((1, 8192, 8192, 32), ch_first(4))) == UNSUPPORTED       # ... on the input alone
        assert call(hipops.slice_desc((1, 8192, 8192, 16), (ALL,), out_ld=32)) == UNSUPPORTED  # ... on the output alone
    name = hipops.slice_kernel_name
    assert name(s, index) == "slice_vec<float, 4>" and name(s, index, half=True) == "slice_elem<_Float16>"
    assert name(s, index, in_ld=15) == "none" and name(s, (ALL, ALL, ALL, slice(0, 16)), out_ld=15) == "none"
    assert H.si_hip_slice_kernel_name(None, dummy, dummy, 0) == b"none"


def ch_first(c):
    return (ALL, ALL, ALL, slice(0, c))


def test_split_abi_without_a_device(native_libs):
    H, _ = native_libs

    def call(fn, pixels=60, c=24, in_ld=24, widths=(8, 16), offsets=(0, 8), out_lds=(8, 16), src=256, dsts=None, k=None, null=None):
        n = len(widths)
        ia = lambda v: (C.c_int * n)(*v)
        args = [C.c_void_p(src), pixels, c, in_ld, n if k is None else k, ia(offsets), ia(widths), (C.c_void_p * n)(*(dsts or [256] * n)), ia(out_lds)]
        if null is not None:
            args[null] = None
        return fn(*(args + [None]))

    for fn in (H.si_hip_split_channels_f32, H.si_hip_split_channels_f16):
        assert call(fn, src=None) == BADARG
        for slot in (5, 6, 7, 8):                                           # the four arrays
            assert call(fn, null=slot) == BADARG, slot
        assert call(fn, dsts=[256, None]) == BADARG
        assert call(fn, pixels=0) == BADARG
        assert call(fn, c=0) == BADARG and call(fn, c=-3) == BADARG
        assert call(fn, in_ld=23) == BADARG                                 # ld < c
        assert call(fn, k=0) == BADARG and call(fn, k=-1) == BADARG         # K < 1
        assert call(fn, widths=(8, 0)) == BADARG and call(fn, widths=(-8, 16)) == BADARG
        assert call(fn, offsets=(-1, 8)) == BADARG
        assert call(fn, offsets=(0, 9)) == BADARG                           # 9 + 16 > 24
        assert call(fn, out_lds=(8, 15)) == BADARG                          # out_ld < width
        assert call(fn, pixels=2 ** 31) == UNSUPPORTED
        assert call(fn, pixels=2 ** 27) == UNSUPPORTED                      # 2^27 * 24 element offsets
        assert call(fn, pixels=2 ** 26, out_lds=(8, 32)) == UNSUPPORTED     # ... on one destination alone
        assert call(fn, pixels=2 ** 27, c=8, in_ld=8, widths=(8, 8), offsets=(0, 0), out_lds=(8, 8)) == UNSUPPORTED   # the launch's items: 2^27 * 16
    name = hipops.split_channels_kernel_name
    assert name((2, 5, 6, 24), (8, 16)) == "split_vec<float, 4>" and name((2, 5, 6, 24), (8, 16), half=True) == "split_vec<_Float16, 8>"
    assert name((2, 5, 6, 24), (8, 16), in_ld=25) == "split_elem<float>" and name((2, 5, 6, 24), (8, 16), out_lds=(8, 17)) == "split_elem<float>"
    assert name((2, 5, 6, 24), (8, 8), offsets=(0, 12), half=True) == "split_elem<_Float16>"       # an offset that is no multiple of 8
    assert name((2, 5, 6, 24), (8, 17)) == "none" and name((2, 5, 6, 24), (8, 16), in_ld=23) == "none"
    n2 = (C.c_int * 2)
    off4 = H.si_hip_split_channels_kernel_name(C.c_void_p(256), 60, 24, 24, 2, n2(0, 8), n2(8, 16), (C.c_void_p * 2)(256, 260), n2(8, 16), 0)
    assert off4 == b"split_elem<float>"                                     # ONE destination 4 bytes off: the whole split goes by elements
    assert H.si_hip_split_channels_kernel_name(C.c_void_p(264), 60, 24, 24, 2, n2(0, 8), n2(8, 16), (C.c_void_p * 2)(256, 256), n2(8, 16), 1) == b"split_elem<_Float16>"


def test_kernel_form_of_every_row_of_the_gpu_tables(native_libs):
    import test_gpu_slice as tg
    seen = set()
    for _, s, index, f32, f16 in tg.SLICE_TABLE:
        for half, f in ((False, f32), (True, f16)):
            want = tg.slice_form("f16" if half else "f32", f)
            assert hipops.slice_kernel_name(s, index, half) == want, (s, index, half)
            seen.add(want)
    for _, s, widths, f32, f16 in tg.SPLIT_TABLE:
        for half, f in ((False, f32), (True, f16)):
            want = tg.split_form("f16" if half else "f32", f)
            assert hipops.split_channels_kernel_name(s, widths, half=half) == want, (s, widths, half)
            seen.add(want)
    assert seen == tg.ALL_FORMS and len(seen) == 8                          # the tables reach every form the header declares
    text = open(HEADER).read()
    for form in tg.ALL_FORMS:
        assert form.replace("float", "T").replace("_Float16", "T").replace("4>", "V>").replace("8>", "V>") in text, form
    # the grid-stride case of the GPU file and the view cases take the forms they name
    assert hipops.slice_kernel_name((2, 1031, 511, 8), ch_first(8)) == "slice_vec<float, 4>"
    for c in tg.VIEW_CASES:
        v = c.views
        if isinstance(c, tg.SliceView):
            d = hipops.slice_desc(c.s, c.index, v["in_ld"], v["out_ld"])
            es = 2 if c.half else 4
            got = _native.hip().si_hip_slice_kernel_name(C.byref(d), C.c_void_p(256 + es * v["in_c_off"]), C.c_void_p(256 + es * v["out_c_off"]), int(c.half))
            assert got.decode() == c.form, c.id


def test_out_of_range_integers_in_a_param_file_do_not_throw(native_libs, tmp_path):
    """Parameter::parse_from_string saturates: an int64 open end (or any integer beyond 32 bits, in a list too) is a value, never an exception
    through the C-ABI; the loader is exercised through si_pnnx_save, which needs no device"""
    b = mg.PnnxBuilder(seed=1)
    x = b.input((2, 8, 6, 4))
    b.output(b.slice(x, 1, 2, 9223372036854775807, 1))
    b.output(b.slice(x, (2, 3), (1, 0), (99999999999999999999, 4294967296), (1, 1)))
    y = b._new_operand((2, 8, 6, 4))
    b._emit("Tensor.slice", "op_neg", [x], [y], dict(dim=1, start=-99999999999, end=4294967295, step=1))
    b.output(y)
    pp, bp = str(tmp_path / "m.param"), str(tmp_path / "m.bin")
    b.save(pp, bp)
    op, ob = str(tmp_path / "o.param"), str(tmp_path / "o.bin")
    engine.pnnx_save(pp, bp, op, ob)
    lines = [_parse(ln) for ln in open(op).read().splitlines()[2:]]
    prm = [p for t, _, _, _, p in lines if t == "Tensor.slice"]
    assert prm[0]["end"] == "2147483647" and prm[1]["ends"] == "(2147483647,2147483647)"
    assert prm[2]["start"] == "-2147483648" and prm[2]["end"] == "2147483647"
