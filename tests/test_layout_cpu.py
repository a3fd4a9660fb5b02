"""CPU: Tensor.permute / reshape / view / torch.transpose / squeeze / unsqueeze / contiguous -- the layout algebra (include/si_layout.h) against
numpy by brute force, the idioms with their exact nests, its refusals, the builder's lines and toy models, the C-ABI of include/si_permute.h
(exported, bound under its own table, what it decides without a device) and the registry."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import layout_reference as lr
from ct_reference import _parse
from simpleinfer_amd import _native, engine, hipops, modelgen as mg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "si_permute.h")
LAYOUT_HEADER = os.path.join(ROOT, "include", "si_layout.h")
OK, ERROR_SHAPE, UNSUPPORT = 0, 3, 5
BADARG, UNSUPPORTED = -1, -2


def header_int(name, path=HEADER):
    return int(re.search(r"#define %s (\d+)" % name, open(path).read()).group(1))


def _check(in_shape, ops):
    """the plan of a chain against numpy's element order; returns what the plan is"""
    oshape, want = lr.expected_gather(in_shape, ops)
    rc, view, dims, st = hipops.layout_plan(in_shape, ops, oshape)
    assert rc in (OK, UNSUPPORT), (rc, in_shape, ops)              # (a chain numpy serves never has a wrong shape)
    if rc == UNSUPPORT and not dims:
        return "refused"                                           # a non-dividing boundary
    got = np.arange(want.size) if view else lr.nest_gather(dims, st)
    assert np.array_equal(got, want), (in_shape, ops, view, dims, st)
    assert all(d > 1 for d in dims) and all(s > 0 for s in st)
    assert view == (len(dims) == 0 or (len(dims) == 1 and st[0] == 1))
    for k in range(len(dims) - 1):                                 # neighbours are merged wherever they can be
        assert st[k] != dims[k + 1] * st[k + 1], (dims, st)
    assert (rc == UNSUPPORT) == (len(dims) > 4)
    return "view" if view else "nest%d" % len(dims)


@pytest.mark.parametrize("seed", [11, 12, 13, 14])
def test_algebra_equals_numpy_on_random_chains(native_libs, seed):
    """1000 seeded chains per case of rank 2 - 4 with extents from {1, 2, 3, 4, 6}: every chain the rule serves reproduces numpy's element order"""
    rng = np.random.Generator(np.random.Philox(seed))
    kinds = {}
    for _ in range(1000):
        in_shape, ops = lr.random_chain(rng, int(rng.integers(2, 5)))
        k = _check(in_shape, ops)
        kinds[k] = kinds.get(k, 0) + 1
    assert kinds.get("view", 0) > 300 and kinds.get("nest2", 0) + kinds.get("nest3", 0) + kinds.get("nest4", 0) > 200, kinds
    assert 50 < kinds.get("refused", 0) < 400, kinds


N, C_, H, W = 2, 12, 5, 7
IDIOMS = [
    # (input, chain, view, dims, in_stride)
    ("ssd", (N, C_, H, W), [("permute", (0, 2, 3, 1)), ("view", (N, -1, 4))], True, [N * H * W * C_], [1]),
    ("pool_1x1_view", (N, C_, 1, 1), [("view", (N, -1))], True, [N * C_], [1]),
    ("view_n_c_hw", (N, C_, H, W), [("view", (N, C_, -1))], False, [N, C_, H * W], [H * W * C_, 1, C_]),
    ("view_n_flat", (N, C_, H, W), [("view", (N, -1))], False, [N, C_, H * W], [H * W * C_, 1, C_]),
    ("permute_021", (N, H * W, C_), [("permute", (0, 2, 1))], False, [N, C_, H * W], [H * W * C_, 1, C_]),
    ("permute_0231", (N, C_, H, W), [("permute", (0, 2, 3, 1))], False, [N, W * C_, H], [H * W * C_, 1, W * C_]),
    ("permute_0312", (N, C_, H, W), [("permute", (0, 3, 1, 2))], False, [N, C_, H * W], [H * W * C_, 1, C_]),
    # the raw YOLOv5 head, na = 3, no = 4: runs of `no`; three dimensions for one image, the batch in front of them otherwise
    ("yolov5_raw_n1", (1, C_, H, W), [("view", (1, 3, 4, H, W)), ("permute", (0, 1, 3, 4, 2)), ("view", (1, -1, 4))], False,
     [3, H * W, 4], [4, C_, 1]),
    ("yolov5_raw", (N, C_, H, W), [("view", (N, 3, 4, H, W)), ("permute", (0, 1, 3, 4, 2)), ("view", (N, -1, 4))], False,
     [N, 3, H * W, 4], [H * W * C_, 4, C_, 1]),
    # channel shuffle, g = 3: the batch merges into the pixels
    ("channel_shuffle", (N, C_, H, W), [("view", (N, 3, 4, H, W)), ("transpose", (1, 2)), ("view", (N, C_, H, W))], False,
     [N * H * W, 4, 3], [C_, 1, 4]),
]


@pytest.mark.parametrize("case", IDIOMS, ids=[c[0] for c in IDIOMS])
def test_idioms_have_these_exact_nests(native_libs, case):
    _, in_shape, ops, view, dims, st = case
    oshape, _ = lr.expected_gather(in_shape, ops)
    assert hipops.layout_plan(in_shape, ops, oshape) == (OK, view, dims, st)
    assert _check(in_shape, ops) == ("view" if view else "nest%d" % len(dims))
    if not view:                                                   # the form the kernel takes for the nest
        want = "rows" if st[-1] == 1 else "tile"
        name = hipops.permute_kernel_name(hipops.permute_desc(dims, st, form=want))
        assert name.startswith("permute_%s<float" % want), name
        assert hipops.permute_kernel_name(hipops.permute_desc(dims, st, form="rows" if want == "tile" else "tile")) == "none"


def test_pixel_stride_and_squeeze_rules(native_libs):
    # a strided rank-4 input is never a view: the rows of C channels are gathered out of rows of ld
    assert hipops.layout_plan((N, C_, H, W), [("permute", (0, 2, 3, 1)), ("view", (N, -1, 4))], in_ld=16) == (OK, False, [N * H * W, C_], [16, 1])
    assert hipops.layout_plan((N, C_, H, W), [("contiguous", ())], (N, C_, H, W)) == (OK, True, [N * H * W * C_], [1])
    assert hipops.layout_plan((N, 1, H, W), [("squeeze", 1)], (N, H, W))[:2] == (OK, True)
    assert hipops.layout_plan((N, C_, H, W), [("squeeze", 1)], (N, C_, H, W))[:2] == (OK, True)    # torch: a dimension that is not 1 stays
    assert hipops.layout_plan((N, H, W), [("unsqueeze", 1)], (N, 1, H, W))[:2] == (OK, True)
    assert hipops.layout_plan((N, H, W), [("unsqueeze", -1)], (N, H, W, 1)) == (OK, False, [N, W, H], [H * W, 1, W])
    assert hipops.layout_plan((N, C_), [("transpose", (0, 1))], (C_, N)) == (OK, False, [C_, N], [1, C_])
    assert hipops.layout_plan((N, C_), [("transpose", (-1, -2))], (C_, N)) == (OK, False, [C_, N], [1, C_])
    assert hipops.layout_plan((1, 1, 1), [("view", (1,))], (1,)) == (OK, True, [], [])
    # dimensions that are contiguous with each other are one run: a boundary may fall wherever a divisor of the run allows
    assert hipops.layout_plan((4, 3), [("view", (6, 2))], (6, 2)) == (OK, True, [12], [1])
    assert hipops.layout_plan((3, 4), [("transpose", (0, 1)), ("view", (6, 2))])[0] == UNSUPPORT      # (a transposed [4, 3] is no run)
    assert hipops.layout_plan((2, 6, 1, 1), [("view", (4, 3))], (4, 3)) == (OK, True, [12], [1])


def test_refusals(native_libs):
    # a boundary that falls inside the stored channel dimension and does not divide it
    assert hipops.layout_plan((2, 12, 5, 8), [("view", (2, 8, -1))])[0] == UNSUPPORT
    assert hipops.layout_plan((2, 12, 5, 8), [("view", (2, 6, -1))])[0] == OK                       # ... one that divides is served
    # a copy of five loop dimensions: the nest is reported (and is right), the status says it is not served
    ops = [("view", (2, 2, 3, 4, 6)), ("permute", (0, 1, 2, 4, 3)), ("view", (4, 3, 6, 4))]
    rc, view, dims, st = hipops.layout_plan((2, 6, 4, 6), ops, (4, 3, 6, 4))
    assert (rc, view, dims, st) == (UNSUPPORT, False, [2, 2, 6, 4, 3], [144, 3, 6, 36, 1])
    assert _check((2, 6, 4, 6), ops) == "nest5"
    # tensors of rank > 4 exist only inside a chain
    assert hipops.layout_plan((2, 12, 5, 7), [("view", (2, 3, 4, 5, 7))], (2, 3, 4, 5, 7))[0] == UNSUPPORT
    assert hipops.layout_plan((2, 3, 4, 5, 7), [("view", (2, 12, 5, 7))], (2, 12, 5, 7))[0] == UNSUPPORT
    # parameters that disagree with the operand
    assert hipops.layout_plan((2, 12, 5, 7), [("permute", (0, 2, 3, 1)), ("view", (2, -1, 4))], (2, 104, 4))[0] == ERROR_SHAPE
    assert hipops.layout_plan((2, 12, 5, 7), [("view", (2, 13, -1))])[0] == ERROR_SHAPE
    assert hipops.layout_plan((2, 12, 5, 7), [("view", (2, -1, -1))])[0] == ERROR_SHAPE
    assert hipops.layout_plan((2, 12, 5, 7), [("view", (2, 0, 420))])[0] == ERROR_SHAPE
    assert hipops.layout_plan((2, 12, 5, 7), [("permute", (0, 2, 1))])[0] == ERROR_SHAPE
    assert hipops.layout_plan((2, 12, 5, 7), [("permute", (0, 2, 2, 1))])[0] == ERROR_SHAPE
    assert hipops.layout_plan((2, 12, 5, 7), [("transpose", (1, 4))])[0] == ERROR_SHAPE
    assert hipops.layout_plan((2, 12, 5, 7), [("squeeze", 4)])[0] == ERROR_SHAPE
    assert hipops.layout_plan((2, 12, 5, 7), [("unsqueeze", 5)])[0] == ERROR_SHAPE
    assert hipops.layout_plan((2, 12, 5, 7), [("permute", (0, 2, 3, 1))], (2, 5, 12, 7))[0] == ERROR_SHAPE
    assert hipops.layout_plan((2, 12, 5, 7), [], in_ld=8)[0] == ERROR_SHAPE                        # a pixel stride below the channels


def test_builder_emits_pnnx_keys():
    b = mg.PnnxBuilder(seed=1)
    x = b.input((2, 8, 6, 4))
    outs = [b.permute(x, (0, 2, 3, 1)), b.permute(x, (0, -1, 1, 2), functional=True), b.reshape(x, (2, -1, 4)), b.view(x, (2, 192)),
            b.transpose(x, 1, -1), b.squeeze(b.unsqueeze(x, 1), 1), b.squeeze(x, 1), b.contiguous(x)]
    parsed = [_parse(ln) for ln in b.lines[1:]]
    assert [p[0] for p in parsed] == ["Tensor.permute", "torch.permute", "Tensor.reshape", "Tensor.view", "torch.transpose", "torch.unsqueeze",
                                      "torch.squeeze", "torch.squeeze", "Tensor.contiguous"]
    assert [p[4] for p in parsed] == [dict(dims="(0,2,3,1)"), dict(dims="(0,-1,1,2)"), dict(shape="(2,-1,4)"), dict(shape="(2,192)"),
                                      dict(dim0="1", dim1="-1"), dict(dim="1"), dict(dim="1"), dict(dim="1"), {}]
    assert [b.shapes[o] for o in outs] == [(2, 6, 4, 8), (2, 4, 8, 6), (2, 48, 4), (2, 192), (2, 4, 6, 8), (2, 8, 6, 4), (2, 8, 6, 4), (2, 8, 6, 4)]
    assert b.shapes[parsed[5][3][0]] == (2, 1, 8, 6, 4)
    xv = np.arange(2 * 8 * 6 * 4, dtype=np.float32).reshape(2, 8, 6, 4)
    for typ, _, ins, os_, prm in parsed:                            # the reference reads every line the builder writes
        if ins == ["0"]:
            assert lr.apply_op(xv, *lr.line_op(typ, prm)).shape == b.shapes[os_[0]]
    with pytest.raises(AssertionError):
        b.view(x, (2, 5, -1))
    with pytest.raises(AssertionError):
        b.permute(x, (0, 1, 1, 2))


def _types(b):
    return [ln.split()[0] for ln in b.lines]


def _lines(b, typ):
    return [_parse(ln) for ln in b.lines if ln.split()[0] == typ]


def test_toy_ssd_head():
    b = mg.build_toy_ssd_head()
    t = _types(b)
    assert t.count("Tensor.permute") == t.count("Tensor.view") == 4 and t.count("torch.cat") == 3 and t.count("nn.Sigmoid") == 1
    assert t[-5:] == ["torch.cat", "torch.cat", "nn.Sigmoid", "torch.cat", "pnnx.Output"]
    assert all(p[4] == dict(dims="(0,2,3,1)") for p in _lines(b, "Tensor.permute"))
    assert [p[4]["shape"] for p in _lines(b, "Tensor.view")] == ["(2,-1,4)", "(2,-1,3)"] * 2
    assert [b.shapes[p[3][0]] for p in _lines(b, "Tensor.view")] == [(2, 128, 4), (2, 128, 3), (2, 32, 4), (2, 32, 3)]
    cats = _lines(b, "torch.cat")
    assert [c[4]["dim"] for c in cats] == ["1", "1", "2"] and [b.shapes[c[3][0]] for c in cats] == [(2, 160, 4), (2, 160, 3), (2, 160, 7)]
    for p in _lines(b, "Tensor.permute"):                           # every permute -> view pair is the identity on the conv's bytes
        n, c, h, w = b.shapes[p[2][0]]
        k = 4 if c == 8 else 3
        assert hipops.layout_plan((n, c, h, w), [("permute", (0, 2, 3, 1)), ("view", (n, -1, k))], (n, h * w * c // k, k))[:2] == (OK, True)
    y = lr.eval_graph(b, mg.synth_input((2, 32, 32, 3)))
    assert y.shape == (2, 160, 7) and np.isfinite(y).all() and (y[..., 4:] > 0).all() and (y[..., 4:] < 1).all() and y[..., :4].min() < 0


def test_toy_anchorfree_head():
    b = mg.build_toy_anchorfree_head()
    assert _types(b)[-6:] == ["Tensor.view", "nn.Conv2d", "Tensor.view", "torch.cat", "Tensor.permute", "pnnx.Output"]
    assert [p[4]["shape"] for p in _lines(b, "Tensor.view")] == ["(2,32,-1)"] * 2
    assert [b.shapes[p[3][0]] for p in _lines(b, "Tensor.view")] == [(2, 32, 256), (2, 32, 64)]
    assert _lines(b, "torch.cat")[0][4] == dict(dim="2") and _lines(b, "Tensor.permute")[0][4] == dict(dims="(0,2,1)")
    y = lr.eval_graph(b, mg.synth_input((2, 64, 64, 3)))
    assert y.shape == (2, 320, 32) and np.isfinite(y).all() and np.abs(y).max() > 0.01


def test_toy_yolov5_raw_head():
    b = mg.build_toy_yolov5_raw_head()
    assert _types(b)[-7:] == ["nn.Conv2d", "Tensor.view", "Tensor.permute", "Tensor.view", "nn.Sigmoid", "torch.cat", "pnnx.Output"]
    views = _lines(b, "Tensor.view")
    assert [p[4]["shape"] for p in views] == ["(2,3,7,8,8)", "(2,-1,7)", "(2,3,7,4,4)", "(2,-1,7)"]
    assert all(p[4] == dict(dims="(0,1,3,4,2)") for p in _lines(b, "Tensor.permute"))
    assert [len(b.shapes[p[3][0]]) for p in views] == [5, 3, 5, 3]                                 # the rank-5 route
    y = lr.eval_graph(b, mg.synth_input((2, 32, 32, 3)))
    assert y.shape == (2, 240, 7) and (y > 0).all() and (y < 1).all()


@pytest.mark.parametrize("pool", [1, 2])
def test_toy_view_classifier(pool):
    b = mg.build_toy_view_classifier(pool=pool)
    f = mg.build_toy_view_classifier(pool=pool, flatten=True)
    assert _types(b)[-4:] == ["nn.AdaptiveAvgPool2d", "Tensor.view", "nn.Linear", "pnnx.Output"]
    assert _types(f)[-4:] == ["nn.AdaptiveAvgPool2d", "torch.flatten", "nn.Linear", "pnnx.Output"]
    assert _lines(b, "Tensor.view")[0][4] == dict(shape="(2,-1)") and b.shapes[_lines(b, "Tensor.view")[0][3][0]] == (2, 32 * pool * pool)
    x = mg.synth_input((2, 32, 32, 3))
    y = lr.eval_graph(b, x)
    assert y.shape == (2, 10) and np.array_equal(y, lr.eval_graph(f, x))                           # the same model, written two ways
    plan = hipops.layout_plan((2, 32, pool, pool), [("view", (2, -1))], (2, 32 * pool * pool))
    assert plan == ((OK, True, [64], [1]) if pool == 1 else (OK, False, [2, 32, 4], [128, 1, 32]))


def test_toy_channel_shuffle():
    b = mg.build_toy_channel_shuffle()
    assert _types(b) == ["pnnx.Input", "nn.Conv2d", "nn.ReLU", "nn.Conv2d", "nn.ReLU", "Tensor.view", "torch.transpose", "Tensor.view", "nn.Conv2d",
                         "pnnx.Output"]
    assert [p[4] for p in _lines(b, "Tensor.view")] == [dict(shape="(2,3,8,16,16)"), dict(shape="(2,24,16,16)")]
    assert _lines(b, "torch.transpose")[0][4] == dict(dim0="1", dim1="2")
    x = np.arange(2 * 24 * 4, dtype=np.float32).reshape(2, 24, 2, 2)
    ops = [("view", (2, 3, 8, 2, 2)), ("transpose", (1, 2)), ("view", (2, 24, 2, 2))]
    import torch
    want = torch.nn.functional.channel_shuffle(torch.from_numpy(x), 3).numpy()
    assert np.array_equal(lr.apply_ops(x, ops), want)


def test_tap_rule_of_the_graph_runner():
    """the taps are the arithmetic a movement operator reads and the arithmetic on moved data; with them the runner needs nothing else"""
    b = mg.build_toy_ssd_head()
    taps = lr.tap_operands(b)
    assert len(taps) == 5 and b.shapes[taps[-1]] == (2, 160, 3)
    x = mg.synth_input((2, 32, 32, 3))
    p = lr.probe_builder(b, taps)
    assert _types(p)[-5:] == ["pnnx.Output"] * 5 and _types(b).count("pnnx.Output") == 1
    exact = {}
    for r in taps:                                                  # (stand-in for an engine: float32 roundings of the float64 runner)
        q = lr.probe_builder(b, [r])
        exact[r] = lr.eval_graph(q, x).astype(np.float32)
    y = lr.eval_graph(b, x, taps=exact)
    assert y.dtype == np.float32 and np.array_equal(y[..., 4:], exact[taps[-1]])
    assert np.abs(y - lr.eval_graph(b, x)).max() < 1e-5


# ---- the C-ABI ------------------------------------------------------------------------------------------------------------
def _declared(path):
    src = open(path).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    names = []
    for m in re.finditer(r"\b(si_[a-z0-9_]+)\s*\(", src):
        if m.group(1) not in names:
            names.append(m.group(1))
    return names


def test_headers_are_exported_and_bound(native_libs):
    H, L = native_libs
    declared = _declared(HEADER)
    assert declared == ["si_hip_permute_f32", "si_hip_permute_f16", "si_hip_permute_kernel_name"]
    assert sorted(H._si_permute_signatures) == sorted(declared)
    for other in (H._si_signatures, H._si_slice_signatures, H._si_reduce_signatures, H._si_act_signatures, H._si_pad_signatures):
        assert not set(declared) & set(other)
    raw = C.CDLL(_native.LIB_HIP_PATH)
    assert not [n for n in declared if not hasattr(raw, n)]
    assert "si_hip_permute" not in open(os.path.join(ROOT, "include", "si_hip.h")).read()
    text = open(HEADER).read()
    m = re.search(r"typedef struct SiPermuteDesc \{(.*?)\} SiPermuteDesc;", text, flags=re.S)
    body = re.sub(r"/\*.*?\*/", " ", m.group(1), flags=re.S)
    fields = [f.strip() for decl in body.split(";") if decl.strip() for f in decl.strip().rsplit(None, 1)[1].split(",")]
    have = ["%s[%d]" % (n, t._length_) if hasattr(t, "_length_") else n for n, t in _native.SiPermuteDesc._fields_]
    assert fields == have, fields
    assert C.sizeof(_native.SiPermuteDesc) == 64
    assert [header_int("SI_PERMUTE_FORM_" + k.upper()) for k in ("auto", "rows", "tile", "elem")] == [hipops.PERMUTE_FORMS[k] for k in
                                                                                                   ("auto", "rows", "tile", "elem")]
    assert header_int("SI_PERMUTE_TILE") == 64 and 1 <= header_int("SI_PERMUTE_TILE_MIN") <= 64
    assert header_int("SI_PERMUTE_TILE_MAX_BLOCKS") >= 256 and header_int("SI_PERMUTE_MAX_BLOCKS") >= 256
    # the host side
    assert _declared(LAYOUT_HEADER) == ["si_layout_plan"] == sorted(L._si_layout_signatures)
    assert hasattr(C.CDLL(_native.LIB_HOST_PATH), "si_layout_plan")
    assert [header_int("SI_LAYOUT_" + k.upper(), LAYOUT_HEADER) for k in ("permute", "reshape", "transpose", "squeeze", "unsqueeze")] == [
        hipops.LAYOUT_OPS[k] for k in ("permute", "reshape", "transpose", "squeeze", "unsqueeze")]
    assert header_int("SI_LAYOUT_IDENTITY", LAYOUT_HEADER) == hipops.LAYOUT_OPS["contiguous"]
    assert header_int("SI_LAYOUT_MAX_NEST", LAYOUT_HEADER) == 8 == len(_native.SiLayoutNest().dims)


def test_permute_abi_without_a_device(native_libs):
    """refusals happen before any device call (the pointers are never looked at), and the form follows from the descriptor alone"""
    H, _ = native_libs
    dummy = C.c_void_p(256)
    for fn in (H.si_hip_permute_f32, H.si_hip_permute_f16):
        def call(d, src=dummy, dst=dummy):
            return fn(C.byref(d), src, dst, None)

        good = lambda **kw: hipops.permute_desc((3, 5, 16), (80, 1, 5), **kw)
        assert fn(None, dummy, dummy, None) == BADARG
        assert call(good(), src=None) == BADARG and call(good(), dst=None) == BADARG
        for rank in (0, -1, 5):
            d = good()
            d.rank = rank
            assert call(d) == BADARG
        for k in range(3):
            for v in (0, -1):
                d = good()
                d.dims[k] = v
                assert call(d) == BADARG
                d = good()
                d.in_stride[k] = v
                assert call(d) == BADARG
        assert call(good(out_ld=15)) == BADARG
        assert call(good(form=4)) == BADARG and call(good(form=-1)) == BADARG
        assert call(good(form="rows")) == BADARG                                                    # the innermost stride is 5
        assert call(hipops.permute_desc((3, 5, 16), (80, 16, 1), form="tile")) == BADARG              # nothing to transpose
        assert call(hipops.permute_desc((3, 16), (7, 3), form="tile")) == BADARG                      # no loop dimension of stride 1
        # offsets and counts beyond 31 bits
        assert call(hipops.permute_desc((2, 4), (2 ** 31, 1))) == UNSUPPORTED
        assert call(hipops.permute_desc((3, 2 ** 30), (1, 3))) == UNSUPPORTED
        assert call(hipops.permute_desc((2 ** 16, 2 ** 16), (1, 1))) == UNSUPPORTED
        assert call(hipops.permute_desc((2 ** 20, 4), (4, 1), out_ld=2 ** 12)) == UNSUPPORTED
    tmin = header_int("SI_PERMUTE_TILE_MIN")
    name = hipops.permute_kernel_name
    assert name(hipops.permute_desc((3, 5, 16), (80, 16, 1))) == "permute_rows<float, 4>"
    assert name(hipops.permute_desc((3, 5, 16), (80, 16, 1)), half=True) == "permute_rows<_Float16, 8>"
    assert name(hipops.permute_desc((3, 5, 12), (80, 16, 1)), half=True) == "permute_rows<_Float16, 1>"
    assert name(hipops.permute_desc((3, 5, 16), (80, 16, 1)), src_align=260) == "permute_rows<float, 1>"
    assert name(hipops.permute_desc((3, 5, 16), (80, 16, 1)), dst_align=264) == "permute_rows<float, 1>"
    assert name(hipops.permute_desc((3, 5, 16), (80, 18, 1))) == "permute_rows<float, 1>"
    assert name(hipops.permute_desc((3, 5, 16), (80, 16, 1), out_ld=18)) == "permute_rows<float, 1>"
    assert name(hipops.permute_desc((3, 5, 6), (80, 16, 1))) == "permute_rows<float, 1>"
    assert name(hipops.permute_desc((3, tmin, tmin), (640, 1, tmin))) == "permute_tile<float>"
    assert name(hipops.permute_desc((3, tmin, tmin), (640, 1, tmin)), half=True) == "permute_tile<_Float16>"
    assert name(hipops.permute_desc((3, tmin - 1, tmin), (640, 1, tmin))) == "permute_elem<float>"
    assert name(hipops.permute_desc((3, tmin, tmin - 1), (640, 1, tmin))) == "permute_elem<float>"
    assert name(hipops.permute_desc((3, 2, 2), (640, 1, 2), form="tile")) == "permute_tile<float>"
    assert name(hipops.permute_desc((3, 16), (7, 3))) == "permute_elem<float>"
    assert name(hipops.permute_desc((3, 16), (7, 3)), half=True) == "permute_elem<_Float16>"
    assert name(hipops.permute_desc((3, 16), (7, 3), out_ld=2)) == "none"


def test_permute_ref_is_the_descriptor_in_numpy():
    src = np.arange(2 * 5 * 3, dtype=np.float32)
    got = hipops.permute_ref(src, hipops.permute_desc((2, 3, 5), (15, 1, 3), out_ld=6), out_fill=-1.0)
    want = np.full((6, 6), -1.0, np.float32)
    want[:, :5] = src.reshape(2, 5, 3).transpose(0, 2, 1).reshape(6, 5)
    assert np.array_equal(got, want)


def test_registry_lists_the_layout_type_strings(native_libs):
    types = engine.registry_types()
    assert len(lr.LAYOUT_TYPES) == 8
    for t in lr.LAYOUT_TYPES:
        assert t in types, t
    for t in lr.ABSENT_TYPES + ("nn.ChannelShuffle", "nn.GELU", "nn.ELU", "nn.Dropout", "nn.Softmin", "F.softmin", "nn.AdaptiveMaxPool2d",
                                "torch.max", "torch.argmax", "torch.prod", "torch.tensor_split", "torch.unbind", "Tensor.select",
                                "Tensor.narrow", "Tensor.clamp_", "nn.LPPool2d", "nn.AvgPool1d", "nn.AvgPool3d", "nn.ReflectionPad1d"):
        assert t not in types, t
