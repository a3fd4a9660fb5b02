"""CPU: nn.LSTM / nn.GRU and the step kernel's host side -- the numpy rule of tests/rnn_reference.py pinned to torch float64 (1 and 2
layers, both directions, both batch_first settings, bias on and off); the builders' lines for both output arities and the toy's operator
sequence; the registry; the C-ABI of include/si_rnn.h (exported, bound under its own table, absent from include/si_hip.h, the structure's
fields, every compute entry driven by a view case of the GPU file); what is decided without a device: every refusal by return code, the
buffer sizes, the W_hh image; and two stand-alone C++ programs under AddressSanitizer and UBSan: the plan arithmetic
(tests/cpp/test_rnn_plan.cpp over csrc/hip/rnn_plan.h) and the batch rule of the family kRecurrent (tests/cpp/test_batch_rule_rnn.cpp)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import containment as ct
import rnn_reference as rr
from ct_reference import _parse
from simpleinfer_amd import _native, engine, hipops, modelgen as mg

BADARG, UNSUPPORTED = -1, -2
CELLS = ("lstm", "gru")


@pytest.mark.parametrize("batch_first", [False, True], ids=["seq_first", "batch_first"])
@pytest.mark.parametrize("dirs", [1, 2])
@pytest.mark.parametrize("layers", [1, 2])
@pytest.mark.parametrize("cell", CELLS)
def test_rule_equals_torch(cell, layers, dirs, batch_first):
    pytest.importorskip("torch")
    for bias, (t, n, i, h) in ((True, (7, 3, 5, 6)), (False, (4, 2, 8, 9)), (True, (1, 1, 3, 1))):
        w = rr.make_weights(cell, i, h, layers, dirs, bias, seed=3)
        x = rr.sequence(4, t, n, i, batch_first=batch_first)
        got, ref = rr.rnn_ref(cell, x, w, batch_first), rr.rnn_torch(cell, x, w, batch_first)
        for a, b, what in zip(got, ref, ("y", "h_n", "c_n")):
            if b is None:
                assert a is None and cell == "gru"
                continue
            assert a.shape == b.shape, (what, a.shape, b.shape)
            assert np.abs(a - b).max() <= 1e-12, (cell, layers, dirs, batch_first, bias, what, np.abs(a - b).max())


def test_rounding_restatement_rounds_only_what_is_stored():
    """with rnd=round_f16 every value of y is a half, the states follow y, and the result moves by rounding alone"""
    for cell in CELLS:
        w = rr.make_weights(cell, 8, 16, 2, 2, True, seed=5)
        x = rr.round_f16(rr.sequence(6, 5, 3, 8))
        y, h_n, c_n = rr.rnn_ref(cell, x, w, rnd=rr.round_f16)
        exact = rr.rnn_ref(cell, x, w)[0]
        assert np.array_equal(y, y.astype(np.float16).astype(np.float64))
        assert np.array_equal(h_n[2], y[-1, :, :16]) and np.array_equal(h_n[3], y[0, :, 16:])
        assert 0.0 < np.abs(y - exact).max() < 2e-2


def test_builder_lines_parse_back():
    b = mg.PnnxBuilder(seed=1)
    x = b.input((7, 2, 24))
    y = b.lstm(x, 16)
    y2, h_n, c_n = b.lstm(x, 8, num_layers=2, bias=False, bidirectional=True, states=True)
    g = b.gru(x, 12, bidirectional=True)
    g2, gh = b.gru(b.input((2, 7, 24)), 8, num_layers=3, batch_first=True, states=True)
    parsed = [_parse(ln) for ln in b.lines if ln.startswith(("nn.LSTM", "nn.GRU"))]
    assert [p[0] for p in parsed] == ["nn.LSTM", "nn.LSTM", "nn.GRU", "nn.GRU"]
    assert [len(p[2]) for p in parsed] == [1, 1, 1, 1] and [len(p[3]) for p in parsed] == [1, 3, 1, 2]
    assert parsed[0][4] == dict(batch_first="False", bias="True", bidirectional="False", dropout="0.000000e+00", hidden_size="16", input_size="24",
                                num_layers="1", proj_size="0")
    assert parsed[1][4]["num_layers"] == "2" and parsed[1][4]["bidirectional"] == "True" and parsed[1][4]["bias"] == "False"
    assert "proj_size" not in parsed[2][4] and parsed[3][4]["batch_first"] == "True"
    assert b.shapes[y] == (7, 2, 16) and b.shapes[y2] == (7, 2, 16) and b.shapes[h_n] == b.shapes[c_n] == (4, 2, 8)
    assert b.shapes[g] == (7, 2, 24) and b.shapes[g2] == (2, 7, 8) and b.shapes[gh] == (3, 2, 8)
    n0, n1, n2 = parsed[0][1], parsed[1][1], parsed[2][1]
    assert b.attrs[n0 + ".weight_ih_l0"].shape == (64, 24) and b.attrs[n0 + ".weight_hh_l0"].shape == (64, 16)
    assert b.attrs[n0 + ".bias_ih_l0"].shape == b.attrs[n0 + ".bias_hh_l0"].shape == (64,)
    assert n0 + ".weight_ih_l0_reverse" not in b.attrs
    assert b.attrs[n1 + ".weight_ih_l1_reverse"].shape == (32, 16) and b.attrs[n1 + ".weight_hh_l1"].shape == (32, 8) and n1 + ".bias_ih_l0" not in b.attrs
    assert b.attrs[n2 + ".weight_ih_l0_reverse"].shape == (36, 24) and b.attrs[n2 + ".bias_hh_l0_reverse"].shape == (36,)
    # what the engine refuses is still written: proj_size, initial states as further inputs
    b2 = mg.PnnxBuilder()
    x = b2.input((7, 2, 24))
    h0 = b2.input((1, 2, 16))
    b2.lstm(x, 16, proj_size=4)
    b2.lstm(x, 16, initial=(h0, h0))
    p = [_parse(ln) for ln in b2.lines[-2:]]
    assert p[0][4]["proj_size"] == "4" and len(p[1][2]) == 3


def _types(b):
    return [_parse(ln)[0] for ln in b.lines]


def test_toy_crnn_has_the_expected_operator_sequence():
    pytest.importorskip("torch")
    stage = ["nn.Conv2d", "nn.ReLU", "nn.MaxPool2d"]
    for cell, typ in (("lstm", "nn.LSTM"), ("gru", "nn.GRU")):
        for batch_first in (False, True):
            b = mg.build_toy_crnn(cell=cell, batch_first=batch_first)
            assert _types(b) == ["pnnx.Input"] + stage * 3 + ["torch.flatten", "Tensor.permute", typ, "nn.Linear", "pnnx.Output"]
            rec = _parse([ln for ln in b.lines if ln.startswith(typ)][0])
            perm = _parse([ln for ln in b.lines if ln.startswith("Tensor.permute")][0])
            assert perm[4]["dims"] == ("(0,2,1)" if batch_first else "(2,0,1)")
            assert rec[4]["num_layers"] == "2" and rec[4]["bidirectional"] == "True" and rec[4]["hidden_size"] == "32" and rec[4]["input_size"] == "32"
            assert b.shapes[rec[2][0]] == ((2, 10, 32) if batch_first else (10, 2, 32))
            assert b.shapes[rec[3][0]] == ((2, 10, 64) if batch_first else (10, 2, 64))
            (y,) = rr.eval_graph(b, mg.synth_input((2, 16, 40, 3)))
            assert y.shape == ((2, 10, 11) if batch_first else (10, 2, 11)) and np.isfinite(y).all()
    b = mg.build_toy_crnn(states=True)
    assert _types(b)[-5:] == ["nn.LSTM", "nn.Linear", "pnnx.Output", "nn.Linear", "pnnx.Output"]
    y, hcls = rr.eval_graph(b, mg.synth_input((2, 16, 40, 3)))
    assert y.shape == (10, 2, 11) and hcls.shape == (4, 2, 11)
    # the fp16 emulation moves the result by rounding alone
    (yh,) = rr.eval_graph(mg.build_toy_crnn(), mg.synth_input((2, 16, 40, 3)), rnd=rr.round_f16)
    (ye,) = rr.eval_graph(mg.build_toy_crnn(), mg.synth_input((2, 16, 40, 3)))
    assert 0.0 < np.abs(yh - ye).max() < 2e-2 * np.abs(ye).max()


def test_registry_lists_both_types(native_libs):
    types = engine.registry_types()
    assert "nn.LSTM" in types and "nn.GRU" in types
    for absent in ("nn.RNN", "nn.LSTMCell", "nn.GRUCell"):
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


def test_rnn_header_is_exported_and_bound(native_libs):
    H, _ = native_libs
    declared = _declared(rr.HEADER)
    assert declared == rr.ENTRIES
    assert sorted(H._si_rnn_signatures) == sorted(declared)
    for other in (H._si_signatures, H._si_norm_signatures, H._si_pad_signatures, H._si_pool_signatures, H._si_softmax_signatures, H._si_superres_signatures,
                  H._si_slice_signatures, H._si_reduce_signatures, H._si_act_signatures, H._si_permute_signatures, H._si_attention_signatures,
                  H._si_deform_signatures, H._si_grid_signatures, H._si_roi_signatures):
        assert not set(declared) & set(other)
    raw = C.CDLL(_native.LIB_HIP_PATH)   # a handle of its own: nothing but the dynamic symbol table answers
    missing = [name for name in declared if not hasattr(raw, name)]
    assert not missing, missing
    # the Python structure has the header's fields in the header's order, with the header's types
    m = re.search(r"typedef struct SiRnnDesc \{(.*?)\} SiRnnDesc;", open(rr.HEADER).read(), flags=re.S)
    body = re.sub(r"/\*.*?\*/", " ", m.group(1), flags=re.S)
    ctypes_of = {"int": C.c_int, "long long": C.c_longlong, "float": C.c_float}
    fields = [(n.strip(), ctypes_of[typ]) for typ, names in re.findall(r"\b(int|long long|float)\s+([^;]+);", body) for n in names.split(",")]
    assert fields == list(_native.SiRnnDesc._fields_), fields
    assert rr.header_enum("SI_RNN_LSTM") == 0 and rr.header_enum("SI_RNN_GRU") == 1 == hipops.RNN_CELLS["gru"]
    assert rr.header_enum("SI_RNN_TILE_ROWS") == 16 and rr.header_enum("SI_RNN_BLOCK_UNITS") == 64 and rr.header_enum("SI_RNN_MAX_HIDDEN") == 2048
    assert (rr.header_enum("SI_RNN_WS_GATES"), rr.header_enum("SI_RNN_WS_STATE"), rr.header_enum("SI_RNN_WS_WHH")) == (0, 1, 2)
    # the header pins the bias order of the projection
    text = open(rr.HEADER).read()
    assert "LSTM b_ih + b_hh for every gate" in text and "b_ih ALONE for n" in text


def test_si_hip_header_declares_none_of_them():
    text = open(ct.HEADER).read()
    for name in rr.ENTRIES:
        assert name not in text, name
    assert "SiRnnDesc" not in text and "si_hip_rnn" not in text


def test_every_compute_entry_of_the_rnn_header_is_driven():
    """the rule of tests/test_containment_cpu.py for include/si_hip.h, applied to include/si_rnn.h and the view cases of the GPU file"""
    import test_gpu_rnn as tr
    entries = [n for n in ct.header_functions(rr.HEADER) if not ct.is_exempt(n)]
    assert entries == ["si_hip_rnn_layer_f32", "si_hip_rnn_layer_f16", "si_hip_rnn_pack_whh_f32", "si_hip_rnn_pack_whh_f16"]
    driven = {e for c in tr.VIEW_CASES for e in c.entries}
    assert set(entries) <= driven, sorted(set(entries) - driven)
    assert driven <= set(ct.header_functions(rr.HEADER)), "a case names an entry the header does not declare"


def test_abi_without_a_device(native_libs):
    """refusals happen before any device call.  Every descriptor here has step0 == t, and the accepted calls pass no state output: a call
    that is accepted has then nothing to launch and returns 0 without touching the (made-up) addresses"""
    H, _ = native_libs
    P = [C.c_void_p((j + 1) << 24) for j in range(6)]   # gates, whh, y, c, h_n, c_n: 16-byte aligned, 16 MiB apart
    bhn = C.c_void_p(7 << 24)

    def desc(cell="lstm", t=5, batch=3, input_size=8, hidden=16, dirs=2, **kw):
        return hipops.rnn_desc(cell, t, batch, input_size, hidden, dirs, step0=t, **kw)

    for fn, half in (("si_hip_rnn_layer_f32", 0), ("si_hip_rnn_layer_f16", 1)):
        def call(d, p=P):
            return getattr(H, fn)(C.byref(d), p[0], p[1], bhn, p[2], p[3], p[4], p[5], None)

        def accepted(d, p=P):
            return getattr(H, fn)(C.byref(d), p[0], p[1], bhn, p[2], p[3], None, None, None) == 0

        def name(d, p=P):
            return H.si_hip_rnn_kernel_name(C.byref(d), p[0], p[2], half)

        def refused(d, code, what=""):
            p = P if d.cell == 0 else P[:5] + [None]
            assert call(d, p) == code, (fn, what, call(d, p))
            assert name(d) == b"none", (fn, what)
            for which in range(3):
                assert H.si_hip_rnn_workspace_bytes(C.byref(d), which, half) == 0, (fn, what, which)

        assert getattr(H, fn)(None, P[0], P[1], bhn, P[2], P[3], P[4], P[5], None) == BADARG                 # null descriptor
        for j in (0, 1, 2, 3):                                                                                  # null gates / image / y / c
            assert call(desc(), [None if i == j else P[i] for i in range(6)]) == BADARG, j
        assert accepted(desc("gru"), [P[0], P[1], P[2], None, None, None])                                      # a GRU has no c ...
        assert call(desc("gru"), P) == BADARG                                                                   # ... and no c_n
        assert accepted(desc())                                                                                 # the states are optional
        for field in ("t", "batch", "input", "hidden", "dirs"):                                                  # non-positive sizes
            for value in (0, -1):
                bad = desc()
                setattr(bad, field, value)
                refused(bad, BADARG, (field, value))
        for field, value in (("dirs", 3), ("cell", 2), ("cell", -1), ("step0", -1), ("step0", 6)):
            bad = desc()
            setattr(bad, field, value)
            refused(bad, BADARG, (field, value))
        for field, width in (("x_st", 8), ("x_sb", 8), ("g_st", 128), ("g_sb", 128), ("y_st", 32), ("y_sb", 32)):   # strides below the row width
            bad = desc()
            setattr(bad, field, width - 8)
            refused(bad, BADARG, field)
        bad = desc()
        bad.y_st = -32
        refused(bad, BADARG, "negative stride")
        bad = desc()                      # rows of y that share elements: (s = 1, b = 0) on (s = 0, b = 1)
        bad.y_st = bad.y_sb = 32
        refused(bad, BADARG, "interleaved rows of y")
        assert accepted(desc(batch_first=True)) and accepted(desc())                                            # both dense orders
        # y intersecting the gates, the image, c, h_n, c_n: the same address, and a y that starts inside the gates
        for j in (0, 1, 3, 4, 5):
            p = list(P)
            p[2] = P[j]
            assert call(desc(), p) == BADARG, "y == buffer %d" % j
        p = list(P)
        p[2] = C.c_void_p(P[0].value + 64)
        assert call(desc(), p) == BADARG, "y inside the gates"
        # offsets beyond 31 bits; hidden above the limit
        refused(desc(x_ld=1 << 30), UNSUPPORTED, "x offsets")
        refused(desc(t=1 << 12, g_ld=1 << 20), UNSUPPORTED, "gate offsets")
        refused(desc(batch=1 << 12, t=4, y_ld=1 << 18, batch_first=True), UNSUPPORTED, "y offsets")
        refused(desc(hidden=2056), UNSUPPORTED, "hidden above 2048")
        for cell in CELLS:
            assert name(desc(cell)) == rr.kname(cell, np.float16 if half else np.float32).encode()
    # fp16 alone: hidden % 8, input % 8, a stride or a pointer off 16 bytes
    def call16(d, p=P):
        return (H.si_hip_rnn_layer_f16(C.byref(d), p[0], p[1], bhn, p[2], p[3], p[4], p[5], None), H.si_hip_rnn_kernel_name(C.byref(d), p[0], p[2], 1))

    assert call16(desc(hidden=20)) == (UNSUPPORTED, b"none")
    assert call16(desc(input_size=5)) == (UNSUPPORTED, b"none")
    assert call16(desc(y_ld=36)) == (UNSUPPORTED, b"none") and call16(desc(g_ld=132)) == (UNSUPPORTED, b"none")
    for j in (0, 1, 2, 4, 5):
        off = [C.c_void_p(P[i].value + (8 if i == j else 0)) for i in range(6)]
        assert H.si_hip_rnn_layer_f16(C.byref(desc()), off[0], off[1], bhn, off[2], off[3], off[4], off[5], None) == UNSUPPORTED, j
    d = desc(hidden=20, input_size=5)                  # the same descriptors are fine in fp32, at any address
    assert H.si_hip_rnn_kernel_name(C.byref(d), C.c_void_p(P[0].value + 4), P[2], 0) == b"rnn_step_kernel<float, 4>"
    assert H.si_hip_rnn_layer_f32(C.byref(d), C.c_void_p(P[0].value + 4), P[1], bhn, P[2], P[3], None, None, None) == 0
    assert H.si_hip_rnn_kernel_name(None, P[0], P[2], 0) == b"none" and H.si_hip_rnn_kernel_name(C.byref(d), None, P[2], 0) == b"none"


def test_workspace_sizes_and_the_whh_image(native_libs):
    H, _ = native_libs
    d = hipops.rnn_desc("lstm", 26, 32, 512, 256, 2)
    assert H.si_hip_rnn_workspace_bytes(C.byref(d), 0, 0) == 26 * 32 * 2 * 4 * 256 * 4
    assert H.si_hip_rnn_workspace_bytes(C.byref(d), 0, 1) == 26 * 32 * 2 * 4 * 256 * 2
    assert H.si_hip_rnn_workspace_bytes(C.byref(d), 1, 0) == H.si_hip_rnn_workspace_bytes(C.byref(d), 1, 1) == 2 * 32 * 256 * 4
    assert H.si_hip_rnn_workspace_bytes(C.byref(d), 2, 0) == 2 * 4 * 256 * 256 * 4 and H.si_hip_rnn_workspace_bytes(C.byref(d), 3, 0) == 0
    g = hipops.rnn_desc("gru", 26, 32, 512, 256, 2)
    assert H.si_hip_rnn_workspace_bytes(C.byref(g), 1, 0) == 0 and H.si_hip_rnn_workspace_bytes(C.byref(g), 2, 1) == 2 * 3 * 256 * 256 * 2
    # the image: lane 16 g + x of (direction, tile, k step, gate) holds W[gate H + 16 tile + x][4 s + g] (fp32) or [32 s + 8 g ..] (fp16);
    # units and k beyond H are zeros, and every weight is there once
    for cell in CELLS:
        ng = rr.GATES[cell]
        for hidden in (1, 15, 17, 40):
            w = rr.make_weights(cell, 8, hidden, 1, 2, False, seed=hidden)
            w_hh = np.stack([w[0][0][1], w[0][1][1]])
            dd = hipops.rnn_desc(cell, 1, 1, 8, hidden, 2)
            tiles = (hidden + 15) // 16
            img = hipops.rnn_pack_whh(dd, w_hh)
            ks = (hidden + 3) // 4
            img = img.reshape(2, tiles, ks, ng, 4, 16)          # [dir][tile][s][gate][g][x]
            full = np.zeros((2, ng, tiles * 16, ks * 4), np.float32)
            full[:, :, :hidden, :hidden] = w_hh.reshape(2, ng, hidden, hidden)
            want = full.reshape(2, ng, tiles, 16, ks, 4).transpose(0, 2, 4, 1, 5, 3)
            assert np.array_equal(img, want), (cell, hidden)
            if hidden % 8 == 0:
                img16 = hipops.rnn_pack_whh(dd, w_hh, half=True)
                ks16 = (hidden + 31) // 32
                img16 = img16.reshape(2, tiles, ks16, ng, 4, 16, 8)   # [dir][tile][s][gate][g][x][j]
                full16 = np.zeros((2, ng, tiles * 16, ks16 * 32), np.float16)
                full16[:, :, :hidden, :hidden] = w_hh.reshape(2, ng, hidden, hidden).astype(np.float16)
                want16 = full16.reshape(2, ng, tiles, 16, ks16, 4, 8).transpose(0, 2, 4, 1, 5, 3, 6)
                assert np.array_equal(img16, want16), (cell, hidden)
    with pytest.raises(hipops.HipError):
        hipops.rnn_pack_whh(hipops.rnn_desc("lstm", 1, 1, 8, 20, 1), np.zeros((1, 80, 20), np.float32), half=True)


def test_projection_bias_order():
    """the one fp32 sum the header pins, in hipops and in the restatement"""
    r = np.random.Generator(np.random.Philox(9))
    for cell in CELLS:
        g = rr.GATES[cell] * 6
        b_ih, b_hh = r.uniform(-1, 1, g).astype(np.float32), r.uniform(-1, 1, g).astype(np.float32)
        bias, b_hn = hipops.rnn_projection_bias(cell, b_ih, b_hh)
        rb, rh = rr.projection_bias(cell, b_ih, b_hh)
        assert np.array_equal(bias, rb) and bias.dtype == np.float32
        if cell == "lstm":
            assert b_hn is None and rh is None and np.array_equal(bias, b_ih + b_hh)
        else:
            assert np.array_equal(b_hn, rh) and np.array_equal(b_hn, b_hh[12:]) and np.array_equal(bias[12:], b_ih[12:]) and np.array_equal(bias[:12], (b_ih + b_hh)[:12])


SANITIZE = ["-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]      # the runtimes inside the program: it starts the same under any environment


def _stand_alone(tmp_path, source, include, ok):
    exe = str(tmp_path / os.path.splitext(source)[0])
    subprocess.check_call(["g++", "-std=c++17", "-O0", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined"] + SANITIZE +
                          ["-I" + include, os.path.join(rr.ROOT, "tests", "cpp", source), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and ok in r.stdout and "runtime error" not in r.stderr, r.stdout[-4000:] + r.stderr[-4000:]


def test_plan_arithmetic_stand_alone_under_sanitizers(tmp_path):
    hip_dir = os.path.join(rr.ROOT, "simpleinfer_amd", "csrc", "hip")
    _stand_alone(tmp_path, "test_rnn_plan.cpp", hip_dir, "rnn plan ok")
    # the kernel file uses that header, and the header nothing of HIP
    assert '#include "rnn_plan.h"' in open(os.path.join(hip_dir, "rnn.hip")).read()
    assert "hip" not in re.sub(r"//[^\n]*", "", open(os.path.join(hip_dir, "rnn_plan.h")).read()).lower()


def test_batch_rule_for_both_types_stand_alone_under_sanitizers(tmp_path):
    _stand_alone(tmp_path, "test_batch_rule_rnn.cpp", os.path.join(rr.ROOT, "simpleinfer_amd", "csrc", "host"), "rnn rule ok")
