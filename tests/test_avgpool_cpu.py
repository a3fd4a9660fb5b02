"""CPU: nn.AvgPool2d and the general nn.AdaptiveAvgPool2d -- the numpy rule of tests/pool_reference.py pinned to torch: float64 exactly,
the float32 / float16 emulations of the windowed kernel's arithmetic to the BITS of torch's fp32 / half CPU kernels, the output-size
rule over a grid; the builder's lines and the two toy models; the C-ABI of include/si_pool.h (exported, bound under its own table,
absent from include/si_hip.h, every compute entry driven by the GPU file's view cases); the registry; and what the entries decide
without a device: the refusals by return code, the kernel form and the form switch."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import containment as ct
import pool_reference as pl
import util
from ct_reference import _parse
from simpleinfer_amd import _native, engine, hipops, modelgen as mg

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
POOL_HEADER = os.path.join(ROOT, "include", "si_pool.h")
FOUR = ("nn.AvgPool2d", "F.avg_pool2d", "nn.AdaptiveAvgPool2d", "F.adaptive_avg_pool2d")


def _args(case):
    k, s, p, ce, cip, div = case
    return dict(k=k, s=s, p=p, ceil_mode=ce, count_include_pad=cip, divisor_override=div)


def _x(shape3, c, seed=3, dtype=np.float64):
    return util.rng_uniform(seed, (shape3[0], shape3[1], shape3[2], c), -1.0, 1.0).astype(dtype)


@pytest.mark.parametrize("table", ["A", "B"])
def test_rule_equals_torch_float64_exactly(table):
    pytest.importorskip("torch")
    cases, shape, c = (pl.TABLE_A, pl.SHAPE_A, 8) if table == "A" else (pl.TABLE_B, pl.SHAPE_B, 6)
    x = _x(shape, c)
    for case in cases:
        ref, got = pl.avgpool2d_f64_torch(x, **_args(case)), pl.avgpool2d_ref(x, **_args(case))
        assert got.dtype == np.float64 and got.shape == ref.shape, (case, got.shape, ref.shape)
        ct.assert_same_bits(got, ref, "table %s %s" % (table, pl.case_id(case)))


def test_adaptive_rule_equals_torch_float64_exactly():
    pytest.importorskip("torch")
    # (8 channels: whole vectors of torch's channels_last kernel on any CPU, whose lanes add in the rule's order)
    for shape, outs, c in ((pl.SHAPE_A, pl.ADAPTIVE_A, 8), (pl.SHAPE_B, pl.ADAPTIVE_B, 8)):
        x = _x(shape, c)
        for o in outs:
            ct.assert_same_bits(pl.avgpool2d_ref(x, adaptive=o), pl.avgpool2d_f64_torch(x, adaptive=o), "adaptive %s -> %s" % (shape[1:], o))


@pytest.mark.parametrize("dt", ["f32", "f16"])
def test_emulation_has_the_bits_of_torchs_cpu_kernels(dt):
    """sequential float32 adds from +0, one division, (half: one rounding): torch's fp32 and half CPU kernels do exactly this on table A and
    the 11 x 14 adaptive list (channels_last tensors, the layout of this project) -- the rule the GPU tests hold the windowed form to"""
    pytest.importorskip("torch")
    dtype = np.float32 if dt == "f32" else np.float16
    x = _x(pl.SHAPE_A, 8, 5, dtype)
    for case in pl.TABLE_A:
        got = pl.avgpool2d_ref(x, acc=np.float32, **_args(case))
        assert got.dtype == dtype
        ct.assert_same_bits(got, pl.avgpool2d_torch(x, **_args(case)), "%s %s" % (dt, pl.case_id(case)))
    for o in pl.ADAPTIVE_A:
        if o == (1, 1):
            continue   # torch turns this one into mean(), a different order of additions
        ct.assert_same_bits(pl.avgpool2d_ref(x, adaptive=o, acc=np.float32), pl.avgpool2d_torch(x, adaptive=o), "%s adaptive %s" % (dt, o))


def test_output_size_rule_matches_torch():
    torch = pytest.importorskip("torch")
    F = torch.nn.functional
    checked = 0
    for i in range(1, 13):
        t = torch.zeros(1, 1, i, 1)
        for k in range(1, 6):
            for s in range(1, 5):
                for p in range(0, k // 2 + 1):
                    if i + 2 * p - k < 0:
                        continue
                    for ce in (False, True):
                        got = F.avg_pool2d(t, (k, 1), (s, 1), (p, 0), ce).shape[2]
                        assert pl.out_size(i, k, s, p, ce) == got == hipops.avgpool_out_size(i, k, s, p, ce) == mg.PnnxBuilder.avgpool_out_size(
                            i, k, s, p, ce), (i, k, s, p, ce, got)
                        assert len(pl.windows(i, k, s, p, ce)) == got
                        checked += 1
    assert checked > 900, checked
    assert pl.out_size(5, 2, 3, 1, True) == 2 and pl.out_size(5, 2, 3, 1, False) == 2   # the decrement: ceil alone would give 3
    assert pl.out_size(15, 2, 2, 0, True) == 8 and pl.out_size(15, 2, 2, 0, False) == 7


def test_windows_by_hand():
    assert pl.windows(5, 3, 2, 1) == [(0, 2, 3), (1, 4, 3), (3, 5, 3)]
    assert pl.windows(5, 2, 2, 0, True) == [(0, 2, 2), (2, 4, 2), (4, 5, 1)]          # the ceil window is cut at i + p
    assert pl.windows(4, 3, 2, 1, True) == [(0, 2, 3), (1, 4, 3), (3, 4, 2)]          # ... its padded extent too: b = min(a + k, i + p)
    assert pl.adaptive_windows(13, 6) == [(0, 3, 3), (2, 5, 3), (4, 7, 3), (6, 9, 3), (8, 11, 3), (10, 13, 3)]
    assert pl.adaptive_windows(5, 3) == [(0, 2, 2), (1, 4, 3), (3, 5, 2)]
    assert pl.adaptive_windows(2, 5) == [(0, 1, 1), (0, 1, 1), (0, 2, 2), (1, 2, 1), (1, 2, 1)]   # pooling up
    x = np.arange(5, dtype=np.float64).reshape(1, 1, 5, 1)
    row = lambda **kw: pl.avgpool2d_ref(x, **kw).reshape(-1).tolist()
    assert row(k=(1, 3), s=(1, 2), p=(0, 1)) == [1 / 3, 2.0, 7 / 3]
    assert row(k=(1, 3), s=(1, 2), p=(0, 1), count_include_pad=False) == [0.5, 2.0, 3.5]
    assert row(k=(1, 3), s=(1, 2), p=(0, 1), divisor_override=2) == [0.5, 3.0, 3.5]


def test_builder_emits_torch_keys():
    b = mg.PnnxBuilder(seed=1)
    x = b.input((2, 6, 11, 14))
    outs = [b.avgpool(x, 2), b.avgpool(x, 3, 1, 1, count_include_pad=False), b.avgpool(x, 2, 2, 0, ceil_mode=True, count_include_pad=False),
            b.avgpool(x, (5, 3), (3, 2), (2, 1), divisor_override=3, functional=True), b.avgpool(x, 2, 3, 1, ceil_mode=True),
            b.adaptive_avgpool(x, (5, 3)), b.adaptive_avgpool(x, (7, 7), functional=True)]
    parsed = [_parse(ln) for ln in b.lines[1:]]
    assert [p[0] for p in parsed] == ["nn.AvgPool2d", "nn.AvgPool2d", "nn.AvgPool2d", "F.avg_pool2d", "nn.AvgPool2d", "nn.AdaptiveAvgPool2d",
                                      "F.adaptive_avg_pool2d"]
    assert parsed[0][4] == dict(ceil_mode="False", count_include_pad="True", divisor_override="None", kernel_size="(2,2)", padding="(0,0)",
                                stride="(2,2)")
    assert parsed[3][4] == dict(ceil_mode="False", count_include_pad="True", divisor_override="3", kernel_size="(5,3)", padding="(2,1)",
                                stride="(3,2)")
    assert parsed[2][4]["ceil_mode"] == "True" and parsed[2][4]["count_include_pad"] == "False"
    assert parsed[5][4] == dict(output_size="(5,3)") and parsed[6][4] == dict(output_size="(7,7)")
    assert [b.shapes[o] for o in outs] == [(2, 6, 5, 7), (2, 6, 11, 14), (2, 6, 6, 7), (2, 6, 4, 7), (2, 6, 4, 5), (2, 6, 5, 3), (2, 6, 7, 7)]
    assert not b.attrs
    for typ, _, _, _, prm in parsed:   # the reference reads every line the builder writes
        assert pl.pool_args(typ, prm)


def _counts(b):
    types = [ln.split()[0] for ln in b.lines]
    return {t: types.count(t) for t in set(types)}


def test_toy_densenet():
    b = mg.build_toy_densenet()
    assert _counts(b) == {"pnnx.Input": 1, "nn.Conv2d": 11, "nn.BatchNorm2d": 3, "nn.ReLU": 10, "torch.cat": 3, "nn.AvgPool2d": 3,
                          "pnnx.Expression": 1, "nn.AdaptiveAvgPool2d": 1, "torch.flatten": 1, "nn.Linear": 1, "pnnx.Output": 1}
    pools = [_parse(ln) for ln in b.lines if ln.startswith("nn.AvgPool2d")]
    args = [pl.pool_args(p[0], p[4]) for p in pools]
    assert [(a["k"], a["s"], a["p"], a["ceil_mode"], a["count_include_pad"]) for a in args] == [
        ((2, 2), (2, 2), (0, 0), False, True), ((3, 3), (1, 1), (1, 1), False, False), ((2, 2), (2, 2), (0, 0), True, False)]
    assert [(b.shapes[p[2][0]][2:], b.shapes[p[3][0]][2:]) for p in pools] == [((31, 31), (15, 15)), ((15, 15), (15, 15)), ((15, 15), (8, 8))]
    x = mg.synth_input((2, 33, 33, 3))
    y = pl.eval_graph(b, x)
    assert y.shape == (2, 10) and y.dtype == np.float64 and np.isfinite(y).all() and np.abs(y).max() > 0.01
    assert pl.eval_graph(mg.build_toy_densenet(batch=1, size=21), mg.synth_input((1, 21, 21, 3))).shape == (1, 10)


def test_toy_pspnet():
    b = mg.build_toy_pspnet()
    assert _counts(b) == {"pnnx.Input": 1, "nn.Conv2d": 8, "nn.ReLU": 7, "nn.AdaptiveAvgPool2d": 4, "F.interpolate": 5, "torch.cat": 1,
                          "pnnx.Output": 1}
    pools = [_parse(ln) for ln in b.lines if ln.startswith("nn.AdaptiveAvgPool2d")]
    assert [b.shapes[p[3][0]] for p in pools] == [(2, 32, 1, 1), (2, 32, 2, 2), (2, 32, 3, 3), (2, 32, 6, 6)]
    assert all(b.shapes[p[2][0]] == (2, 32, 13, 13) for p in pools)
    x = mg.synth_input((2, 52, 52, 3))
    y = pl.eval_graph(b, x)
    assert y.shape == (2, 52, 52, 5) and y.dtype == np.float64 and np.isfinite(y).all() and np.abs(y).max() > 0.01
    emu = pl.eval_graph(b, x, rnd=pl.round_f16)
    assert 0 < util.rel_err(emu, y) < 1e-2


def _declared(path):
    src = open(path).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    names = []
    for m in re.finditer(r"\b(si_[a-z0-9_]+)\s*\(", src):
        if m.group(1) not in names:
            names.append(m.group(1))
    return names


def test_pool_header_is_exported_and_bound(native_libs):
    H, _ = native_libs
    declared = _declared(POOL_HEADER)
    assert declared == ["si_hip_avgpool2d_f32", "si_hip_avgpool2d_f16", "si_hip_avgpool2d_kernel_name"]
    assert sorted(H._si_pool_signatures) == sorted(declared)
    for other in (H._si_signatures, H._si_norm_signatures, H._si_pad_signatures):
        assert not set(declared) & set(other)
    raw = C.CDLL(_native.LIB_HIP_PATH)   # a handle of its own: nothing but the dynamic symbol table answers
    missing = [name for name in declared if not hasattr(raw, name)]
    assert not missing, missing
    # the Python structure has the header's fields in the header's order
    m = re.search(r"typedef struct SiAvgPool2dDesc \{(.*?)\} SiAvgPool2dDesc;", open(POOL_HEADER).read(), flags=re.S)
    body = re.sub(r"/\*.*?\*/", " ", m.group(1), flags=re.S)
    fields = [f.strip() for decl in body.split(";") if decl.strip() for f in decl.strip().split(None, 1)[1].split(",")]
    assert fields == [f[0] for f in _native.SiAvgPool2dDesc._fields_], fields
    m = re.search(r"SI_AVGPOOL_COOP_TAPS = (\d+)", open(POOL_HEADER).read())
    assert int(m.group(1)) >= 64   # every window of up to 49 taps keeps the windowed form and torch's bits


def test_si_hip_header_declares_none_of_them():
    text = open(ct.HEADER).read()
    for name in _declared(POOL_HEADER):
        assert name not in text, name
    assert "SiAvgPool2dDesc" not in text


def test_registry_lists_the_four_type_strings(native_libs):
    types = engine.registry_types()
    for t in FOUR:
        assert t in types, t
    assert "nn.AdaptiveMaxPool2d" not in types and "nn.LPPool2d" not in types and "nn.AvgPool1d" not in types and "nn.AvgPool3d" not in types


def test_every_compute_entry_of_the_pool_header_is_driven():
    """the rule of tests/test_containment_cpu.py for include/si_hip.h, applied to include/si_pool.h and the view cases of the GPU file"""
    import test_gpu_avgpool as tp
    entries = [n for n in ct.header_functions(POOL_HEADER) if not ct.is_exempt(n)]
    assert entries == ["si_hip_avgpool2d_f32", "si_hip_avgpool2d_f16"]
    driven = {e for c in tp.VIEW_CASES for e in c.entries}
    assert set(entries) <= driven, sorted(set(entries) - driven)
    assert driven <= set(ct.header_functions(POOL_HEADER)), "a case names an entry the header does not declare"


BADARG, UNSUPPORTED = -1, -2


def test_abi_without_a_device(native_libs):
    """refusals happen before any device call (the pointers are never looked at)"""
    H, _ = native_libs
    dummy = C.c_void_p(256)
    shape = (2, 11, 14, 8)
    desc, adesc = hipops.avgpool2d_desc, hipops.adaptive_avgpool2d_desc
    for fn in ("si_hip_avgpool2d_f32", "si_hip_avgpool2d_f16"):
        def call(d, src=dummy, dst=dummy):
            return getattr(H, fn)(C.byref(d), src, dst, None)

        assert getattr(H, fn)(None, dummy, dummy, None) == BADARG
        assert call(desc(shape, 3, 2, 1), src=None) == BADARG
        assert call(desc(shape, 3, 2, 1), dst=None) == BADARG
        assert call(desc(shape, 3, 2, 1, in_ld=7)) == BADARG                       # ld < c
        assert call(desc(shape, 3, 2, 1, out_ld=4)) == BADARG
        assert call(desc(shape, 3, 2, 2)) == UNSUPPORTED                           # p > k / 2
        assert call(desc(shape, (2, 3), 2, (1, 2))) == UNSUPPORTED
        for field, value in (("kh", 0), ("sw", 0), ("pt", -1), ("c", 0), ("n", 0)):
            bad = desc(shape, 3, 2, 1)
            setattr(bad, field, value)
            assert call(bad) == BADARG, field
        # k3 s2 p1 on 11 x 14: oh = 6 with either rounding, ow = 7 (floor) or 8 (ceil); anything else is refused, with a divisor_override too
        for ce in (False, True):
            good = desc(shape, 3, 2, 1, ceil_mode=ce, divisor_override=3)
            assert (good.oh, good.ow) == (6, 8 if ce else 7)
            for oh, ow in ((5, good.ow), (7, good.ow), (6, 6), (6, 9)):
                bad = desc(shape, 3, 2, 1, ceil_mode=ce, divisor_override=3)
                bad.oh, bad.ow = oh, ow
                assert call(bad) == BADARG, (ce, oh, ow)
        bad = desc((2, 5, 5, 8), 2, 3, 1, ceil_mode=True)
        assert (bad.oh, bad.ow) == (2, 2)
        bad.oh = 3                                                                 # ceil without the decrement
        assert call(bad) == BADARG
        assert call(desc((2, 4, 14, 8), 5, 1, 0)) == BADARG                        # the kernel does not fit: oh = 0
        bad = adesc(shape, (0, 3))
        assert call(bad) == BADARG                                                 # adaptive with oh = 0
        assert call(adesc((65536, 8, 8, 8), (3, 3))) == UNSUPPORTED                # n > 65535
        assert call(adesc((1, 16384, 16384, 8), (3, 3))) == UNSUPPORTED            # element offsets of 2^31
        assert call(adesc((1, 40000, 2, 1), (60000, 1))) == UNSUPPORTED            # ih * oh does not fit 31 bits
        assert call(desc((4096, 512, 512, 8), 1, 1, 0)) == UNSUPPORTED             # n * oh * ow = 2^30 pixels of 8: offsets of 2^33


WIN, COOP = "avgpool2d_window_kernel", "avgpool2d_coop_kernel"


def test_kernel_form_follows_channels_strides_and_pointers(native_libs):
    H, _ = native_libs
    name = hipops.avgpool2d_kernel_name
    s = (2, 11, 14, 8)
    assert name(s, 3, 2, 1) == WIN + "<float, 4>"
    assert name(s, 3, 2, 1, half=True) == WIN + "<_Float16, 8>"
    assert name((2, 11, 14, 6), 3, 2, 1) == WIN + "<float, 1>"
    assert name((2, 11, 14, 12), 3, 2, 1) == WIN + "<float, 4>"
    assert name((2, 11, 14, 12), 3, 2, 1, half=True) == WIN + "<_Float16, 1>"      # c % 8 != 0
    assert name(s, 3, 2, 1, in_ld=9) == WIN + "<float, 1>"                         # a stride that is no multiple of the vector
    assert name(s, 3, 2, 1, out_ld=10) == WIN + "<float, 1>"
    assert name(s, 3, 2, 1, in_ld=16, out_ld=24) == WIN + "<float, 4>"
    assert name(s, adaptive=(5, 3)) == WIN + "<float, 4>"
    assert name((2, 23, 29, 8), (20, 23), (3, 6), 0) == COOP + "<float, 4>"
    assert name((2, 23, 29, 6), (20, 23), (3, 6), 0, half=True) == COOP + "<_Float16, 1>"
    assert name((2, 23, 29, 8), adaptive=(1, 2), half=True) == COOP + "<_Float16, 8>"
    d = hipops.avgpool2d_desc(s, 3, 2, 1)
    assert H.si_hip_avgpool2d_kernel_name(C.byref(d), C.c_void_p(260), C.c_void_p(256), 0) == (WIN + "<float, 1>").encode()   # a pointer off 16 bytes
    assert H.si_hip_avgpool2d_kernel_name(C.byref(d), C.c_void_p(256), C.c_void_p(264), 1) == (WIN + "<_Float16, 1>").encode()
    assert name(s, 3, 2, 2) == "none" and name(s, 3, 2, 1, in_ld=7) == "none"
    assert H.si_hip_avgpool2d_kernel_name(None, C.c_void_p(256), C.c_void_p(256), 0) == b"none"


def test_form_switch_is_the_largest_windows_tap_count(native_libs):
    """cooperative exactly when the largest clipped window of the launch has SI_AVGPOOL_COOP_TAPS taps or more -- checked against the
    window lists of the reference over the tables, the adaptive lists and a grid of (i, k, s, p) -- and never a function of n"""
    T = int(re.search(r"SI_AVGPOOL_COOP_TAPS = (\d+)", open(POOL_HEADER).read()).group(1))
    name = hipops.avgpool2d_kernel_name
    for shape, cases in ((pl.SHAPE_A, pl.TABLE_A), (pl.SHAPE_B, pl.TABLE_B)):
        for k, s, p, ce, _, _ in cases:
            want = COOP if pl.max_taps(shape[1], shape[2], k, s, p, ce) >= T else WIN
            for n in (1, 2, 7):
                assert name((n, shape[1], shape[2], 8), k, s, p, ce).startswith(want + "<"), (k, s, p, ce, n)
    for ih, iw in ((11, 14), (23, 29), (65, 65), (13, 13), (40, 37)):
        for o in pl.ADAPTIVE_A + pl.ADAPTIVE_B + [(2, 2), (3, 3), (6, 6), (64, 3), (66, 1)]:
            want = COOP if pl.max_taps(ih, iw, adaptive=o) >= T else WIN
            assert name((1, ih, iw, 8), adaptive=o).startswith(want + "<"), (ih, iw, o)
    # one axis against the reference's window list: with a kernel of `rows` rows on a map of `rows` rows every window has rows * (its extent
    # along W) taps, so the form at rows = ceil(T / ext) and one row less tells whether the entry found the largest extent
    for i in range(1, 13):
        for k in range(1, 6):
            for s in range(1, 5):
                for p in range(0, k // 2 + 1):
                    if i + 2 * p - k < 0:
                        continue
                    for ce in (False, True):
                        ext = max(hi - lo for lo, hi, _ in pl.windows(i, k, s, p, ce))
                        for rows in (-(-T // ext), -(-T // ext) - 1):   # rows * ext >= T, and just below
                            if rows >= 1:
                                got = name((1, rows, i, 8), (rows, k), (1, s), (0, p), ce)
                                assert got.startswith((COOP if rows * ext >= T else WIN) + "<"), (i, k, s, p, ce, rows, ext, got)
    names = [name((1, 40, 40, 8), k, 1, 0) for k in range(1, 41)]
    flips = [k for k in range(2, 41) if names[k - 1] != names[k - 2]]
    assert len(flips) == 1 and flips[0] ** 2 >= T > (flips[0] - 1) ** 2 and T >= 64, (flips, T)
    assert names[0] == WIN + "<float, 4>" and names[-1] == COOP + "<float, 4>"
