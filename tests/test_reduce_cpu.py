"""CPU: torch.mean / torch.sum / torch.amax / torch.amin -- the numpy rule of tests/reduce_reference.py pinned to torch float64 for every op
and every supported mask (NaN positions as a mask); the builder's lines and the four toy models; the C-ABI of include/si_reduce.h
(exported, bound under its own table, absent from include/si_hip.h, every compute entry driven by the GPU file's view cases); the
registry; and what the entries decide without a device: the refusals by return code and the kernel form by the descriptor, the strides,
the pointers' alignment and the header's switch values.  (What LoadModel refuses needs an engine, hence a device: tests/test_gpu_reduce.py.)"""
import ctypes as C
import re

import numpy as np
import pytest

import containment as ct
import reduce_reference as rr
import util
from ct_reference import _parse
from simpleinfer_amd import _native, engine, hipops, modelgen as mg

G = rr.header_enum("SI_REDUCE_GROUP_MAX_C")
MINP, MAXO = rr.header_enum("SI_REDUCE_COOP_MIN_POSITIONS"), rr.header_enum("SI_REDUCE_COOP_MAX_OUTPUTS")


def _same_with_nan_mask(got, ref, what):
    assert got.shape == ref.shape and got.dtype == ref.dtype == np.float64, what
    assert np.array_equal(np.isnan(got), np.isnan(ref)), what + ": NaN masks differ"
    ok = ~np.isnan(ref)
    inf = ok & np.isinf(ref)
    assert np.array_equal(got[inf], ref[inf]), what + ": infinities differ"
    fin = ok & ~inf
    # the two float64 statements differ by the order of at most 70 additions: 4096 ulp of the largest value is far above that
    bound = 4096 * np.finfo(np.float64).eps * max(1.0, np.abs(ref[fin]).max(initial=0.0))
    assert np.abs(got[fin] - ref[fin]).max(initial=0.0) <= bound, what


@pytest.mark.parametrize("op", rr.OPS)
def test_rule_equals_torch_float64(op):
    pytest.importorskip("torch")
    for shape, masks in (((2, 5, 7, 6), rr.MASKS), ((3, 1, 1, 4), (8, 1))):      # NHWC, and the rank-2 [3, 4] over dim 1 and dim 0
        x = util.rng_uniform(3, shape, -1.0, 3.0)
        for axes in masks:
            got = rr.reduce_ref(x, op, axes)
            assert got.shape == rr.out_shape(shape, axes)
            _same_with_nan_mask(got, rr.reduce_f64_torch(x, op, axes), "%s %s mask %d" % (op, shape, axes))
            if op in ("amax", "amin"):
                assert np.array_equal(got, rr.reduce_f64_torch(x, op, axes))
        # special values: a NaN, one +inf, +inf with -inf, all -inf -- one per channel 0 .. 3 of pixel rows along every mask
        s = x.copy()
        s[0, 0, 0, 0] = np.nan
        s[-1, -1, -1, 1] = np.inf
        s[0, 0, 0, 2], s[-1, -1, -1, 2] = np.inf, -np.inf
        s[..., 3] = -np.inf
        for axes in masks:
            got, ref = rr.reduce_ref(s, op, axes), rr.reduce_f64_torch(s, op, axes)
            _same_with_nan_mask(got, ref, "special values, %s mask %d" % (op, axes))
            assert np.isnan(got).any() and np.isinf(got).any()


def test_masks_follow_the_softmax_axis_rule():
    assert [rr.nhwc_mask(d, 4) for d in (0, 1, 2, 3, -1, -2, -3, -4)] == [1, 8, 2, 4, 4, 2, 8, 1]
    assert rr.nhwc_mask((2, 3), 4) == rr.nhwc_mask((-1, -2), 4) == 6 and rr.nhwc_mask((1,), 4) == 8 and rr.nhwc_mask((0, 2, 3), 4) == 7
    assert [rr.nhwc_mask(d, 2) for d in (0, 1, -1, -2)] == [1, 8, 8, 1]
    with pytest.raises(AssertionError):
        rr.nhwc_mask((2, -2), 4)


def test_builder_emits_torch_keys():
    b = mg.PnnxBuilder(seed=1)
    x = b.input((2, 6, 5, 7))
    outs = [b.mean(x, (2, 3)), b.mean(x, (2, 3), True), b.sum(x, 1, True), b.amax(x, (1,), True), b.amin(x, -1, True), b.mean(x, (-1, -2), True),
            b.amax(x, 0, True), b.sum(x, 1)]
    parsed = [_parse(ln) for ln in b.lines[1:]]
    assert [p[0] for p in parsed] == ["torch.mean", "torch.mean", "torch.sum", "torch.amax", "torch.amin", "torch.mean", "torch.amax", "torch.sum"]
    assert [p[4]["dim"] for p in parsed] == ["(2,3)", "(2,3)", "1", "(1)", "-1", "(-1,-2)", "0", "1"]
    assert [p[4]["keepdim"] for p in parsed] == ["False", "True", "True", "True", "True", "True", "True", "False"]
    assert all(("dtype" in p[4]) == (p[0] in ("torch.mean", "torch.sum")) and p[4].get("dtype", "None") == "None" for p in parsed)
    assert [b.shapes[o] for o in outs] == [(2, 6), (2, 6, 1, 1), (2, 1, 5, 7), (2, 1, 5, 7), (2, 6, 5, 1), (2, 6, 1, 1), (1, 6, 5, 7), (2, 5, 7)]
    assert not b.attrs
    y = b.input((3, 10))
    assert b.shapes[b.mean(y, 1, True)] == (3, 1) and b.shapes[b.amax(y, 0, True)] == (1, 10)


TOYS = {
    # builder, the reduction lines in file order as (type, dim, keepdim), the output's shape (NCHW in the file)
    "timm_head": (mg.build_toy_timm_head, [("torch.mean", "(2,3)", "False")], (2, 10)),
    "cbam": (mg.build_toy_cbam, [("torch.mean", "(2,3)", "True"), ("torch.amax", "(2,3)", "True"), ("torch.mean", "1", "True"),
                                 ("torch.amax", "1", "True")], (2, 8, 16, 16)),
    "coordatt": (mg.build_toy_coordatt, [("torch.mean", "3", "True"), ("torch.mean", "2", "True")], (2, 8, 12, 20)),
    "layernorm2d": (mg.build_toy_layernorm2d, [("torch.mean", "1", "True"), ("torch.mean", "(1)", "True")], (2, 8, 16, 16)),
}


@pytest.mark.parametrize("toy", sorted(TOYS))
def test_toy_builders(toy):
    pytest.importorskip("torch")
    build, reductions, oshape = TOYS[toy]
    b = build()
    parsed = [_parse(ln) for ln in b.lines]
    assert [(p[0], p[4]["dim"], p[4]["keepdim"]) for p in parsed if p[0] in rr.REDUCE_TYPES] == reductions
    assert parsed[0][0] == "pnnx.Input" and parsed[-1][0] == "pnnx.Output" and b.shapes[parsed[-1][2][0]] == oshape
    assert parsed[-2][0] in ("nn.Conv2d", "nn.Linear")     # (an fp32 graph output from the layer's own epilogue under fp16 storage)
    types = [p[0] for p in parsed]
    if toy == "cbam":
        assert types.count("nn.Conv2d") == 7 and types.count("torch.cat") == 1 and types.count("nn.Sigmoid") == 2 and types.count("pnnx.Expression") == 3
        for k in ("mlp0_", "mlp1_"):
            ct.assert_same_bits(b.attrs[k + "avg.weight"], b.attrs[k + "max.weight"], "the shared MLP")
    if toy == "layernorm2d":
        assert [p[4]["expr"] for p in parsed if p[0] == "pnnx.Expression"] == ["sub(@0,@1)", "square(@0)", "div(@0,sqrt(add(@1,1e-06)))"]
    n, c, h, w = b.shapes["0"]
    x = mg.synth_input((n, h, w, c))
    y = rr.eval_graph(b, x)
    assert y.shape == (oshape if len(oshape) == 2 else (oshape[0], oshape[2], oshape[3], oshape[1])) and np.isfinite(y).all() and np.abs(y).max() > 1e-3
    e = rr.eval_graph(b, x, rnd=rr.round_f16)
    assert np.isfinite(e).all() and util.rel_err(e, y) < 2e-2       # the fp16-storage emulation stays near the exact evaluation
    if toy == "layernorm2d":    # the normalised map in front of the last conv has mean 0 and variance 1 over the channels
        cut = mg.build_toy_layernorm2d()
        cut.lines = cut.lines[:-2] + ["pnnx.Output out 1 0 %s" % _parse(cut.lines[-2])[2][0]]
        z = rr.eval_graph(cut, x)
        assert np.abs(z.mean(axis=3)).max() < 1e-9 and np.abs((z * z).mean(axis=3) - 1.0).max() < 1e-3


def _declared(path):
    src = open(path).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    names = []
    for m in re.finditer(r"\b(si_[a-z0-9_]+)\s*\(", src):
        if m.group(1) not in names:
            names.append(m.group(1))
    return names


def test_reduce_header_is_exported_and_bound(native_libs):
    H, _ = native_libs
    declared = _declared(rr.HEADER)
    assert declared == ["si_hip_reduce_f32", "si_hip_reduce_f16", "si_hip_reduce_kernel_name"]
    assert sorted(H._si_reduce_signatures) == sorted(declared)
    for other in (H._si_signatures, H._si_norm_signatures, H._si_pad_signatures, H._si_pool_signatures, H._si_softmax_signatures,
                  H._si_superres_signatures, H._si_slice_signatures):
        assert not set(declared) & set(other)
    raw = C.CDLL(_native.LIB_HIP_PATH)   # a handle of its own: nothing but the dynamic symbol table answers
    missing = [name for name in declared if not hasattr(raw, name)]
    assert not missing, missing
    # the Python structure has the header's fields in the header's order
    text = open(rr.HEADER).read()
    m = re.search(r"typedef struct SiReduceDesc \{(.*?)\} SiReduceDesc;", text, flags=re.S)
    body = re.sub(r"/\*.*?\*/", " ", m.group(1), flags=re.S)
    fields = [f.strip() for decl in body.split(";") if decl.strip() for f in decl.strip().split(None, 1)[1].split(",")]
    assert fields == [f[0] for f in _native.SiReduceDesc._fields_], fields
    assert [rr.header_enum("SI_REDUCE_" + k.upper()) for k in rr.OPS] == [hipops.REDUCE_OPS[k] for k in rr.OPS] == [0, 1, 2, 3]
    assert [rr.header_enum("SI_REDUCE_AXIS_" + k) for k in "NHWC"] == [1, 2, 4, 8]
    parts, slots = rr.header_enum("SI_REDUCE_COOP_PARTS"), rr.header_enum("SI_REDUCE_COOP_SLOTS")
    assert G >= 64 and parts * slots <= 1024 and (parts * slots) % 64 == 0 and MINP >= 1 and MAXO >= 1


def test_si_hip_header_declares_none_of_them():
    text = open(ct.HEADER).read()
    for name in _declared(rr.HEADER):
        assert name not in text, name
    assert "SiReduceDesc" not in text and "si_hip_reduce" not in text


def test_registry_lists_the_four_type_strings(native_libs):
    types = engine.registry_types()
    for t in rr.REDUCE_TYPES:
        assert t in types, t
    for t in ("torch.max", "torch.argmax", "torch.prod", "nn.AdaptiveMaxPool2d", "nn.GELU", "nn.ELU", "nn.ChannelShuffle", "nn.Dropout", "nn.Softmin"):
        assert t not in types, t


def test_every_compute_entry_of_the_reduce_header_is_driven():
    """the rule of tests/test_containment_cpu.py for include/si_hip.h, applied to include/si_reduce.h and the view cases of the GPU file"""
    import test_gpu_reduce as tr
    entries = [n for n in ct.header_functions(rr.HEADER) if not ct.is_exempt(n)]
    assert entries == ["si_hip_reduce_f32", "si_hip_reduce_f16"]
    driven = {e for c in tr.VIEW_CASES for e in c.entries}
    assert set(entries) <= driven, sorted(set(entries) - driven)
    assert driven <= set(ct.header_functions(rr.HEADER)), "a case names an entry the header does not declare"


BADARG, UNSUPPORTED = -1, -2


def test_abi_without_a_device(native_libs):
    """refusals happen before any device call (the pointers are compared, never followed)"""
    H, _ = native_libs
    src, dst = C.c_void_p(1 << 20), C.c_void_p(1 << 40)
    shape = (2, 5, 7, 8)
    desc = hipops.reduce_desc
    for fn in ("si_hip_reduce_f32", "si_hip_reduce_f16"):
        esize = 4 if fn.endswith("f32") else 2

        def call(d, a=src, b=dst):
            return getattr(H, fn)(C.byref(d), a, b, None)

        assert getattr(H, fn)(None, src, dst, None) == BADARG               # null descriptor
        assert call(desc(shape, "sum", 8), a=None) == BADARG                # null pointers
        assert call(desc(shape, "sum", 6), b=None) == BADARG
        for field in ("n", "h", "w", "c"):                                  # non-positive sizes
            for value in (0, -1):
                bad = desc(shape, "mean", 6)
                setattr(bad, field, value)
                assert call(bad) == BADARG, (field, value)
        assert call(desc(shape, "mean", 8, in_ld=7)) == BADARG              # in_ld < c
        assert call(desc(shape, "mean", 6, in_ld=7)) == BADARG
        assert call(desc(shape, "mean", 6, out_ld=7)) == BADARG             # out_ld < the output's channels: c when c is kept ...
        bad = desc(shape, "mean", 8)
        bad.out_ld = 0
        assert call(bad) == BADARG                                          # ... 1 when it is reduced
        for axes in (0, -1, 16, 24):                                        # axes outside 1 .. 15
            bad = desc(shape, "sum", 8)
            bad.axes = axes
            assert call(bad) == BADARG, axes
        for op in (-1, 4):                                                  # op outside 0 .. 3
            bad = desc(shape, "sum", 8)
            bad.op = op
            assert call(bad) == BADARG, op
        # overlapping in / out: the same pointer, an output inside the input, an input inside the output's rows
        assert call(desc(shape, "amax", 6), a=src, b=src) == BADARG
        assert call(desc(shape, "amax", 8), a=src, b=C.c_void_p(src.value + 5 * esize)) == BADARG
        assert call(desc(shape, "amax", 2, in_ld=16, out_ld=16), a=src, b=C.c_void_p(src.value + 4 * esize)) == BADARG   # channels 4 .. 11 meet 0 .. 7
        assert call(desc(shape, "amax", 1, in_ld=8, out_ld=16), a=C.c_void_p(src.value + 8 * esize), b=src) == BADARG    # strides differ: the spans decide
        for axes in (9, 10, 12, 15):                                        # the channel axis together with another
            assert call(desc(shape, "sum", axes)) == UNSUPPORTED, axes
        assert call(desc((1, 16384, 16384, 8), "sum", 8)) == UNSUPPORTED    # element offsets of 2^31
        assert call(desc((1, 1, 1 << 20, 8), "sum", 1, out_ld=1 << 11)) == UNSUPPORTED   # ... on the output side alone
        assert call(desc((65536, 65536, 1, 1), "sum", 1)) == UNSUPPORTED    # 2^32 pixels


def test_kernel_form_follows_the_descriptor_the_pointers_and_the_switches(native_libs):
    H, _ = native_libs
    name, K = hipops.reduce_kernel_name, rr.kname
    f32, f16 = np.float32, np.float16
    for op in rr.OPS:       # the op does not enter
        assert name((2, 5, 7, 8), op, 8) == K("row_group", f32, True)
        assert name((2, 5, 6, 8), op, 6, half=True) == K("col_lane", f16, True)
    assert name((2, 5, 7, 6), "sum", 8) == K("row_group", f32, False)
    assert name((2, 5, 7, 12), "sum", 8) == K("row_group", f32, True)
    assert name((2, 5, 7, 12), "sum", 8, half=True) == K("row_group", f16, False)      # c % 8 != 0
    assert name((2, 5, 7, 8), "sum", 8, in_ld=9) == K("row_group", f32, False)         # a stride that is no multiple of the vector
    assert name((2, 5, 7, 8), "sum", 8, out_ld=3) == K("row_group", f32, True)         # the row forms store single elements: out_ld does not enter
    assert name((2, 5, 6, 8), "sum", 6, out_ld=10) == K("col_lane", f32, False)        # the col forms store vectors
    assert name((2, 5, 6, 8), "sum", 6, in_ld=16, out_ld=24) == K("col_lane", f32, True)
    # the row switch, never a function of the pixel count
    for n in rr.ROW_PIXELS:
        for half in (False, True):
            dt = f16 if half else f32
            assert name((n, 1, 1, G), "mean", 8, half) == K("row_group", dt, True)
            assert name((n, 1, 1, G + 1), "mean", 8, half) == K("row_block", dt, False)
            assert name((n, 1, 1, G + 8), "mean", 8, half) == K("row_block", dt, True)
            assert name((n, 1, 1, 4099), "mean", 8, half) == K("row_block", dt, False)
    # the col switch: positions, and outputs per image; n enters only when it is reduced
    assert name((1, 1, MINP - 1, 8), "mean", 6) == K("col_lane", f32, True) and name((1, 1, MINP, 8), "mean", 6) == K("col_coop", f32, True)
    assert name((3, 5, 5, 8), "mean", 6) == name((1, 5, 5, 8), "mean", 6) == name((64, 5, 5, 8), "mean", 6) == K("col_lane", f32, True)
    assert name((3, 5, 5, 8), "mean", 7) == K("col_coop", f32, True)                    # 75 positions: n is reduced
    assert name((1, 8, 8, MAXO), "amax", 6) == K("col_coop", f32, True) and name((1, 8, 8, MAXO + 4), "amax", 6) == K("col_lane", f32, True)
    assert name((64, 8, 8, MAXO), "amax", 6) == K("col_coop", f32, True)              # a kept n is never counted among the outputs
    assert name((1, 2, MINP, MAXO // 2), "amax", 4) == K("col_coop", f32, True) and name((1, 3, MINP, MAXO // 2), "amax", 4) == K("col_lane", f32, True)
    assert name((1, 1, 1, 10), "sum", 1) == K("col_lane", f32, False)                   # a rank-2 [N, F] tensor over dim 0
    d = hipops.reduce_desc((2, 5, 7, 8), "sum", 8)
    q = lambda a, b, half: H.si_hip_reduce_kernel_name(C.byref(d), C.c_void_p(a), C.c_void_p(b), half).decode()
    assert q(260, 256, 0) == K("row_group", f32, False) and q(256, 260, 0) == K("row_group", f32, True)    # a pointer off 16 bytes: the input's only
    assert q(264, 256, 1) == K("row_group", f16, False)
    d = hipops.reduce_desc((2, 5, 7, 8), "sum", 2)
    assert q(256, 264, 0) == K("col_lane", f32, False) and q(264, 256, 0) == K("col_lane", f32, False) and q(256, 512, 0) == K("col_lane", f32, True)
    assert name((2, 5, 7, 8), "sum", 16) == "none" and name((2, 5, 7, 8), "sum", 8, in_ld=7) == "none" and name((2, 5, 7, 8), "sum", 9) == "none"
    assert name((2, 5, 7, 8), 4, 8) == "none"
    assert H.si_hip_reduce_kernel_name(None, C.c_void_p(256), C.c_void_p(256), 0) == b"none"
    # the whole case table of the GPU file
    for shape in rr.MASK_SHAPES:
        for axes in rr.MASKS:
            for dt in (f32, f16):
                assert name(shape, "sum", axes, dt == f16) == K(rr.expected_form(shape, axes), dt, rr.vectorised(shape, axes, dt)), (shape, axes)
    for c in rr.row_c():
        for dt in (f32, f16):
            assert name((3, 1, 1, c), "amin", 8, dt == f16) == K(rr.expected_form((3, 1, 1, c), 8), dt, rr.vectorised((3, 1, 1, c), 8, dt)), c
    forms = set()
    for shape, axes in rr.coop_cases():
        for dt in (f32, f16):
            assert name(shape, "mean", axes, dt == f16) == K(rr.expected_form(shape, axes), dt, rr.vectorised(shape, axes, dt)), (shape, axes)
        forms.add((rr.expected_form(shape, axes), rr.positions(shape, axes) - MINP))
    assert {("col_lane", -1), ("col_coop", 0), ("col_coop", 1)} <= forms and ("col_lane", 0) in forms     # ... and the outputs rule at the positions switch itself
