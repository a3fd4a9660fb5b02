"""CPU: nn.MultiheadAttention and the attention kernel's host side -- the numpy rule of tests/attention_reference.py pinned to torch float64
(nn.MultiheadAttention with 1, 2 and 3 inputs, both batch_first settings, lq != lk; F.scaled_dot_product_attention on the GPU file's case
table; special values, NaN positions as a mask); the builder's line and the two toys' operator sequences; the registry; the C-ABI of
include/si_attention.h (exported, bound under its own table, absent from include/si_hip.h, the structure's fields, every compute entry driven
by a view case of the GPU file); and what is decided without a device: every refusal by return code, the kernel name by d, type and
alignment.  (LoadModel creates the device context first, so the layer's kUnsupport / kFail cases are held in tests/test_gpu_attention.py.)"""
import ctypes as C
import re

import numpy as np
import pytest

import attention_reference as ar
import containment as ct
from ct_reference import _parse
from simpleinfer_amd import _native, engine, hipops, modelgen as mg

BADARG, UNSUPPORTED = -1, -2


def _same_with_nan_mask(got, ref, what, tol=1e-12):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), what + ": NaN masks differ"
    ok = ~np.isnan(ref)
    assert np.abs(got[ok] - ref[ok]).max(initial=0.0) <= tol * max(1.0, np.abs(ref[ok]).max(initial=0.0)), what


def _weights(e, bias=True, seed=5):
    r = np.random.Generator(np.random.Philox(seed))
    a = np.sqrt(3.0 / e)
    w_in, w_out = r.uniform(-a, a, (3 * e, e)), r.uniform(-a, a, (e, e))
    return (w_in, r.uniform(-0.1, 0.1, 3 * e) if bias else None, w_out, r.uniform(-0.1, 0.1, e) if bias else None)


@pytest.mark.parametrize("batch_first", [False, True], ids=["seq_first", "batch_first"])
@pytest.mark.parametrize("n_in", [1, 2, 3])
def test_rule_equals_torch_multihead_attention(n_in, batch_first):
    pytest.importorskip("torch")
    for e, heads, lq, lk, batch, bias in ((24, 3, 7, 7, 2, True), (32, 4, 5, 9, 3, False), (8, 1, 1, 4, 1, True), (20, 5, 17, 3, 2, True)):
        if n_in == 1:
            lk = lq
        w = _weights(e, bias)
        xs = [ar.tokens(3, lq, batch, e, batch_first=batch_first)] + [ar.tokens(4 + j, lk, batch, e, batch_first=batch_first) for j in range(n_in - 1)]
        got = ar.mha_ref(xs, *w, heads, batch_first)
        _same_with_nan_mask(got, ar.mha_torch(xs, *w, heads, batch_first), "E=%d heads=%d lq=%d lk=%d" % (e, heads, lq, lk))


def test_rule_equals_torch_sdpa_on_the_case_table():
    pytest.importorskip("torch")
    cases = ar.kernel_cases(ar.D_F32)
    assert {c[1] for c in cases} == set(ar.LENGTHS) == {c[2] for c in cases}
    assert {(c[1] % 64, c[2] % 64) for c in cases} == {(a % 64, b % 64) for a in ar.LENGTHS for b in ar.LENGTHS}
    for d, lq, lk, heads, batch in cases[::3]:
        q, k, v = ar.tokens(1, lq, batch, heads * d), ar.tokens(2, lk, batch, heads * d), ar.tokens(3, lk, batch, heads * d)
        for bf in (False, True):
            qq, kk, vv = (np.ascontiguousarray(t.transpose(1, 0, 2)) if bf else t for t in (q, k, v))
            _same_with_nan_mask(ar.attention_ref(qq, kk, vv, heads, batch_first=bf), ar.sdpa_torch(qq, kk, vv, heads, batch_first=bf),
                                "d=%d lq=%d lk=%d" % (d, lq, lk))
    # a scale of its own
    q, k, v = ar.tokens(1, 5, 2, 12), ar.tokens(2, 9, 2, 12), ar.tokens(3, 9, 2, 12)
    _same_with_nan_mask(ar.attention_ref(q, k, v, 3, scale=0.37), ar.sdpa_torch(q, k, v, 3, scale=0.37), "scale")


def test_special_values_follow_torch():
    pytest.importorskip("torch")
    heads, d, lq, lk, batch = 2, 4, 6, 70, 2
    base = [ar.tokens(s, l, batch, heads * d) for s, l in ((1, lq), (2, lk), (3, lk))]
    # large magnitudes stay finite: the maximum is subtracted
    big = [base[0] * np.float32(60), base[1] * np.float32(60), base[2]]
    got = ar.attention_ref(*big, heads)
    assert np.isfinite(got).all()
    _same_with_nan_mask(got, ar.sdpa_torch(*big, heads), "large scores", tol=1e-9)
    for which, pos in (("q", (3, 1, 5)), ("k", (40, 0, 2)), ("v", (66, 1, 1))):
        q, k, v = (t.copy() for t in base)
        {"q": q, "k": k, "v": v}[which][pos] = np.nan
        got, ref = ar.attention_ref(q, k, v, heads), ar.sdpa_torch(q, k, v, heads)
        _same_with_nan_mask(got, ref, "NaN in " + which)
        nan = np.isnan(got)
        s, b, col = pos
        h = col // d
        want = np.zeros_like(nan)
        if which == "q":
            want[s, b, h * d:(h + 1) * d] = True          # its own row of its own head
        elif which == "k":
            want[:, b, h * d:(h + 1) * d] = True          # every row of that (batch, head)
        else:
            want[:, b, col] = True                        # that column of that (batch, head)
        assert np.array_equal(nan, want), which
    # lk = 1: the softmax is 1 and the output is V's only row
    q, k, v = ar.tokens(1, 5, 2, 8), ar.tokens(2, 1, 2, 8), ar.tokens(3, 1, 2, 8)
    assert np.array_equal(ar.attention_ref(q, k, v, 2), np.broadcast_to(v.astype(np.float64), (5, 2, 8)))


def test_builder_line_parses_back():
    b = mg.PnnxBuilder(seed=1)
    q, k = b.input((7, 2, 24)), b.input((9, 2, 24))
    outs = [b.multihead_attention(q, num_heads=3), b.multihead_attention(q, k, num_heads=4, bias=False),
            b.multihead_attention(q, k, k, num_heads=2, batch_first=True, add_bias_kv=True, add_zero_attn=True, kdim=16, vdim=12)]
    parsed = [_parse(ln) for ln in b.lines[2:]]
    assert [p[0] for p in parsed] == ["nn.MultiheadAttention"] * 3
    assert [len(p[2]) for p in parsed] == [1, 2, 3] and all(len(p[3]) == 1 for p in parsed)
    common = dict(embed_dim="24", kdim="24", vdim="24", add_bias_kv="False", add_zero_attn="False", batch_first="False")
    assert parsed[0][4] == dict(common, num_heads="3", bias="True")
    assert parsed[1][4] == dict(common, num_heads="4", bias="False")
    assert parsed[2][4] == dict(embed_dim="24", kdim="16", vdim="12", add_bias_kv="True", add_zero_attn="True", batch_first="True", num_heads="2",
                                bias="True")
    assert all(b.shapes[o] == (7, 2, 24) for o in outs)
    n0, n1 = parsed[0][1], parsed[1][1]
    assert b.attrs[n0 + ".in_proj_weight"].shape == (72, 24) and b.attrs[n0 + ".out_proj.weight"].shape == (24, 24)
    assert b.attrs[n0 + ".in_proj_bias"].shape == (72,) and b.attrs[n0 + ".out_proj.bias"].shape == (24,)
    assert n1 + ".in_proj_bias" not in b.attrs and n1 + ".out_proj.bias" not in b.attrs
    # the weights as a second output
    b2 = mg.PnnxBuilder()
    x = b2.input((2, 7, 24))
    b2.multihead_attention(x, num_heads=3, batch_first=True, need_weights=True)
    typ, _, ins, outs2, _ = _parse(b2.lines[-1])
    assert len(ins) == 1 and len(outs2) == 2 and b2.shapes[outs2[1]] == (2, 7, 7)
    # nn.Linear over the last dimension of a rank-3 operand; the rank-2 line is what it was
    b3 = mg.PnnxBuilder()
    y = b3.linear(b3.input((5, 2, 24)), 16)
    assert b3.shapes[y] == (5, 2, 16) and _parse(b3.lines[-1])[4] == dict(bias="True", in_features="24", out_features="16")


def _types(b):
    return [_parse(ln)[0] for ln in b.lines]


def test_toys_have_the_expected_operator_sequence():
    pytest.importorskip("torch")
    b = mg.build_toy_c3tr()
    layer = ["nn.Linear"] * 3 + ["nn.MultiheadAttention", "pnnx.Expression", "nn.Linear", "nn.Linear", "pnnx.Expression"]
    assert _types(b) == (["pnnx.Input", "nn.Conv2d", "nn.SiLU", "nn.Conv2d", "nn.SiLU", "torch.flatten", "Tensor.permute", "nn.Linear", "pnnx.Expression"]
                         + layer * 2 + ["Tensor.permute", "Tensor.reshape", "nn.Conv2d", "nn.SiLU", "pnnx.Output"])
    mha = [_parse(ln) for ln in b.lines if ln.startswith("nn.MultiheadAttention")]
    assert all(len(m[2]) == 3 and m[4]["num_heads"] == "4" and m[4]["batch_first"] == "False" and m[4]["embed_dim"] == "32" for m in mha)
    assert all(b.shapes[m[3][0]] == (64, 2, 32) for m in mha)                       # [L, N, E]
    lin = [_parse(ln) for ln in b.lines if ln.startswith("nn.Linear")]
    assert [m[4]["bias"] for m in lin] == ["True"] + ["False"] * 10
    assert _parse(b.lines[5])[4] == dict(end_dim="-1", start_dim="2")
    y = ar.eval_graph(b, mg.synth_input((2, 32, 32, 3)))
    assert y.shape == (2, 8, 8, 32) and np.isfinite(y).all()

    h = mg.build_toy_mhsa_head()
    assert _types(h) == ["pnnx.Input", "nn.Conv2d", "nn.ReLU", "nn.Conv2d", "nn.ReLU", "Tensor.permute", "Tensor.view", "nn.MultiheadAttention",
                         "Tensor.permute", "Tensor.view", "torch.mean", "nn.Linear", "pnnx.Output"]
    m = _parse([ln for ln in h.lines if ln.startswith("nn.MultiheadAttention")][0])
    assert len(m[2]) == 1 and m[4]["batch_first"] == "True" and m[4]["num_heads"] == "3" and h.shapes[m[3][0]] == (2, 64, 24)
    y = ar.eval_graph(h, mg.synth_input((2, 16, 16, 3)))
    assert y.shape == (2, 10) and np.isfinite(y).all()
    # the fp16 emulation moves the result by rounding alone
    yh = ar.eval_graph(h, mg.synth_input((2, 16, 16, 3)), rnd=ar.round_f16)
    assert 0.0 < np.abs(yh - y).max() < 2e-2 * np.abs(y).max()


def test_registry_lists_multihead_attention(native_libs):
    types = engine.registry_types()
    assert "nn.MultiheadAttention" in types
    for t in ar.ABSENT_TYPES:
        assert t not in types, t


def _declared(path):
    src = open(path).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    names = []
    for m in re.finditer(r"\b(si_[a-z0-9_]+)\s*\(", src):
        if m.group(1) not in names:
            names.append(m.group(1))
    return names


def test_attention_header_is_exported_and_bound(native_libs):
    H, _ = native_libs
    declared = _declared(ar.HEADER)
    assert declared == ar.ENTRIES
    assert sorted(H._si_attention_signatures) == sorted(declared)
    for other in (H._si_signatures, H._si_norm_signatures, H._si_pad_signatures, H._si_pool_signatures, H._si_softmax_signatures, H._si_permute_signatures):
        assert not set(declared) & set(other)
    raw = C.CDLL(_native.LIB_HIP_PATH)   # a handle of its own: nothing but the dynamic symbol table answers
    missing = [name for name in declared if not hasattr(raw, name)]
    assert not missing, missing
    # the Python structure has the header's fields in the header's order, with the header's types
    m = re.search(r"typedef struct SiAttentionDesc \{(.*?)\} SiAttentionDesc;", open(ar.HEADER).read(), flags=re.S)
    body = re.sub(r"/\*.*?\*/", " ", m.group(1), flags=re.S)
    ctypes_of = {"int": C.c_int, "long long": C.c_longlong, "float": C.c_float}
    fields = [(n.strip(), ctypes_of[typ]) for typ, names in re.findall(r"\b(int|long long|float)\s+([^;]+);", body) for n in names.split(",")]
    assert fields == list(_native.SiAttentionDesc._fields_), fields
    assert ar.header_enum("SI_ATTENTION_BLOCK_Q") == 64 and ar.header_enum("SI_ATTENTION_TILE_K") == 64 and ar.header_enum("SI_ATTENTION_MAX_D") == 128


def test_si_hip_header_declares_none_of_them():
    text = open(ct.HEADER).read()
    for name in ar.ENTRIES:
        assert name not in text, name
    assert "SiAttentionDesc" not in text and "attention" not in text.lower()


def test_every_compute_entry_of_the_attention_header_is_driven():
    """the rule of tests/test_containment_cpu.py for include/si_hip.h, applied to include/si_attention.h and the view cases of the GPU file"""
    import test_gpu_attention as ta
    entries = [n for n in ct.header_functions(ar.HEADER) if not ct.is_exempt(n)]
    assert entries == ["si_hip_attention_f32", "si_hip_attention_f16"]
    driven = {e for c in ta.VIEW_CASES for e in c.entries}
    assert set(entries) <= driven, sorted(set(entries) - driven)
    assert driven <= set(ct.header_functions(ar.HEADER)), "a case names an entry the header does not declare"


def test_abi_without_a_device(native_libs):
    """refusals happen before any device call"""
    H, _ = native_libs
    P = [C.c_void_p(1 << 20), C.c_void_p(2 << 20), C.c_void_p(3 << 20), C.c_void_p(4 << 20)]   # 16-byte aligned, 1 MiB apart
    desc = hipops.attention_desc
    for fn, half in (("si_hip_attention_f32", 0), ("si_hip_attention_f16", 1)):
        def call(d, p=P):
            return getattr(H, fn)(C.byref(d), p[0], p[1], p[2], p[3], None)

        def name(d, p=P):
            return H.si_hip_attention_kernel_name(C.byref(d), p[0], p[1], p[2], p[3], half)

        def refused(d, code, p=P, what=""):
            assert call(d, p) == code, (fn, what, call(d, p))
            assert name(d, p) == b"none", (fn, what)

        assert getattr(H, fn)(None, P[0], P[1], P[2], P[3], None) == BADARG                  # null descriptor
        for j in range(4):                                                                     # null pointers
            refused(desc(2, 3, 5, 7, 8), BADARG, [None if i == j else P[i] for i in range(4)], "null %d" % j)
        for field in ("batch", "heads", "lq", "lk", "d"):                                      # non-positive sizes
            for value in (0, -1):
                bad = desc(2, 3, 5, 7, 8)
                setattr(bad, field, value)
                refused(bad, BADARG, what=(field, value))
        for field in ("q_ss", "k_ss", "v_ss", "o_ss"):                                         # a sequence stride below heads * d
            bad = desc(1, 3, 5, 7, 8)
            setattr(bad, field, 16)
            refused(bad, BADARG, what=field)
        bad = desc(2, 3, 5, 7, 8)
        bad.q_sb = -8
        refused(bad, BADARG, what="negative stride")
        # output rows that share elements: batch 2, lq 2 with o_sb = o_ss = heads * d puts (b = 1, s = 0) on (b = 0, s = 1)
        bad = desc(2, 3, 2, 7, 8)
        bad.o_sb = bad.o_ss = 24
        refused(bad, BADARG, what="interleaved output rows")
        ok = desc(2, 3, 2, 7, 8, batch_first=True)       # both dense orders are fine
        assert call(ok) not in (BADARG, UNSUPPORTED) and call(desc(2, 3, 2, 7, 8)) not in (BADARG, UNSUPPORTED)
        # o intersecting an input: the same address, and an output that starts inside v
        for j in range(3):
            refused(desc(2, 3, 5, 7, 8), BADARG, [P[i] for i in range(3)] + [P[j]], "o == input %d" % j)
        refused(desc(2, 3, 5, 7, 8), BADARG, [P[0], P[1], P[2], C.c_void_p((3 << 20) + 64)], "o inside v")
        # offsets beyond 31 bits; d above the limit
        refused(desc(3, 1, 5, 7, 8, q_ld=1 << 30), UNSUPPORTED, what="q offsets")
        refused(desc(2, 1, 4, 1 << 20, 8, out_ld=1 << 29, batch_first=True), UNSUPPORTED, what="o offsets")
        refused(desc(1, 1, 5, 7, 136), UNSUPPORTED, what="d > 128")
        ok = desc(2, 3, 5, 7, 8)
        assert name(ok) == ar.kname(8, np.float16 if half else np.float32).encode()
    # fp16 alone: d % 8, a stride or a pointer off 16 bytes
    def call16(d, p=P):
        return H.si_hip_attention_f16(C.byref(d), p[0], p[1], p[2], p[3], None), H.si_hip_attention_kernel_name(C.byref(d), p[0], p[1], p[2], p[3], 1)

    assert call16(desc(2, 3, 5, 7, 12)) == (UNSUPPORTED, b"none")
    assert call16(desc(2, 3, 5, 7, 8, k_ld=28)) == (UNSUPPORTED, b"none")
    for j in range(4):
        assert call16(desc(2, 3, 5, 7, 8), [C.c_void_p(P[i].value + (8 if i == j else 0)) for i in range(4)]) == (UNSUPPORTED, b"none"), j
    d = desc(2, 3, 5, 7, 12)                       # the same descriptors are fine in fp32, at any address
    assert H.si_hip_attention_kernel_name(C.byref(d), C.c_void_p(P[0].value + 4), P[1], P[2], P[3], 0) == b"attention_kernel<float, 16>"
    assert H.si_hip_attention_kernel_name(None, P[0], P[1], P[2], P[3], 0) == b"none"


def test_kernel_name_follows_head_dim_and_type(native_libs):
    for d in range(1, 129):
        assert hipops.attention_kernel_name(d) == ar.kname(d, np.float32), d
        assert hipops.attention_kernel_name(d, half=True) == (ar.kname(d, np.float16) if d % 8 == 0 else "none"), d
    assert {hipops.attention_kernel_name(d) for d in ar.D_F32} == {"attention_kernel<float, %d>" % p for p in (16, 32, 64, 128)}
    assert {hipops.attention_kernel_name(d, True) for d in ar.D_F16} == {"attention_kernel<_Float16, %d>" % p for p in (32, 64, 128)}
    assert hipops.attention_kernel_name(129) == "none" and hipops.attention_kernel_name(64, heads=6) == "attention_kernel<float, 64>"
    assert hipops.attention_kernel_name(64, half=True, align=264) == "none" and hipops.attention_kernel_name(64, align=260) == "attention_kernel<float, 64>"
