"""GPU: the fused attention kernel (include/si_attention.h) and nn.MultiheadAttention.  Kernel: fp32 and fp16 against float64 on the case
table of tests/attention_reference.py, the online-softmax cases, special values, bit-for-bit independence, views under guard bands.  Layer and
engine: one-operator graphs for every input count and both batch_first settings, the two toys in fp32 and fp16 storage, re-batched (both), captured,
unfused, their profiles; the fp32 fallback; nn.Linear on rank 3."""
import numpy as np
import pytest

import attention_reference as ar
import containment as ct
import util
from ct_reference import _parse
from simpleinfer_amd import hipops, modelgen as mg
from simpleinfer_amd.engine import Engine, Status, StatusError

pytestmark = pytest.mark.gpu

F32, F16 = np.float32, np.float16


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    w = np.uint32 if got.dtype.itemsize == 4 else np.uint16
    bad = np.nonzero(got.view(w) != want.view(w))
    assert bad[0].size == 0, "%s: %d of %d elements differ in bits, first at %s" % (what, bad[0].size, got.size, tuple(int(b[0]) for b in bad))


def qkv(seed, lq, lk, batch, e, dtype=F32, lo=-1.0, hi=1.0, batch_first=False):
    return tuple(ar.tokens(seed + j, l, batch, e, lo, hi, batch_first, dtype) for j, l in enumerate((lq, lk, lk)))


# ---- the kernel against float64 -----------------------------------------------------------------------------------------------
def half_bar(mag, ref):
    """per element: 2^-10 sum_j p_j |v_j| + 2^-11 |ref| -- twice the budget of rounding P to fp16, plus the final rounding"""
    return 2.0 ** -10 * mag + 2.0 ** -11 * np.abs(ref)


@pytest.mark.parametrize("d", ar.D_F32)
def test_fp32_against_float64(gpu, d):
    """assert_parity at the fp32 bar, and the maximum error held to 8x that of torch's CPU fp32 scaled_dot_product_attention on the same
    inputs (the margin: the hardware exp2 against libm, the folded scale multiply, one rescale rounding per key tile)"""
    pytest.importorskip("torch")
    worst = (0.0, 0.0)
    for dd, lq, lk, heads, batch in [c for c in ar.kernel_cases(ar.D_F32) if c[0] == d]:
        q, k, v = qkv(100 + lq + 7 * lk, lq, lk, batch, heads * d)
        ref = ar.attention_ref(q, k, v, heads)
        got = hipops.attention(q, k, v, heads)
        what = "d=%d lq=%d lk=%d heads=%d batch=%d" % (d, lq, lk, heads, batch)
        assert hipops.LAST_KERNEL_NAME["si_hip_attention"] == ar.kname(d, F32), what
        err = float(np.abs(got.astype(np.float64) - ref).max())
        cpu = float(np.abs(ar.sdpa_torch(q, k, v, heads, dtype=F32) - ref).max())
        print("attention fp32 %s: kernel %.3e, torch CPU fp32 %.3e" % (what, err, cpu))
        worst = max(worst, (err, cpu))
        util.assert_parity(got, ref, what="attention fp32 " + what)
        assert err <= 8.0 * cpu, "%s: kernel error %.3e above 8 x %.3e" % (what, err, cpu)
    print("attention fp32 family d=%d: worst kernel error %.3e (torch CPU fp32 on that case %.3e)" % ((d,) + worst))


@pytest.mark.parametrize("d", ar.D_F16)
def test_fp16_against_float64(gpu, d):
    worst = 0.0
    for dd, lq, lk, heads, batch in [c for c in ar.kernel_cases(ar.D_F16) if c[0] == d]:
        q, k, v = qkv(200 + lq + 7 * lk, lq, lk, batch, heads * d, F16)
        ref, mag = ar.attention_parts(q, k, v, heads)
        got = hipops.attention(q, k, v, heads)
        what = "d=%d lq=%d lk=%d heads=%d batch=%d" % (d, lq, lk, heads, batch)
        assert got.dtype == F16 and hipops.LAST_KERNEL_NAME["si_hip_attention"] == ar.kname(d, F16), what
        ratio = float((np.abs(got.astype(np.float64) - ref) / half_bar(mag, ref)).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, "%s: %.3f of the per-element bar" % (what, ratio)
    print("attention fp16 family d=%d: worst error %.3f of the per-element bar" % (d, worst))


def _online_case(kind, dtype, lk=200, lq=16, d=8):
    """scores that rise with j (the maximum in the last tile), fall with j, or spike once in the middle tile: score(i, j) = a_i * level(j // 8)
    * amp - 0.375 * (j % 8), levels in [-1, 1] on plateaus of 8 keys.  Raw scores reach +-200 in fp32 and +-60000, the fp16 range, in halves;
    the terms are exact in fp32 up to the fp16 range, so the reference's scores are the kernel's;
    rows with a_i < 0 see the mirrored pattern, rows with a small a_i a gentle softmax.  V = I columns: column c collects the keys j = c mod 8,
    one of every plateau, so every column holds a key of the row's top plateau (an output made of nothing but weights below fp16's 2^-24
    would measure P's underflow, not the recurrence) and every output row sums to 1."""
    j = np.arange(lk)
    m, nm = j // 8, lk // 8
    level = {"rising": m / (nm - 1) * 2.0 - 1.0, "falling": 1.0 - m / (nm - 1) * 2.0, "spike": np.where(m == nm // 2, 1.0, -1.0 + 0.01 * (m % 5))}[kind]
    a = np.array([10, -10, 7, -7, 3, -3, 1, -1, 0.3, -0.3, 0.05, -0.05, 0.01, -0.01, 0, 2], np.float64)[:lq]
    amp = 20.0 if dtype == F32 else 250.0
    if dtype == F16:
        a = a * 24.0
    q, k, v = np.zeros((lq, 1, d)), np.zeros((lk, 1, d)), np.zeros((lk, 1, d))
    q[:, 0, 0], q[:, 0, 1] = a, 1.0
    k[:, 0, 0], k[:, 0, 1] = level * amp, -0.375 * (j % 8)
    v[j, 0, j % d] = 1.0
    return q.astype(dtype), k.astype(dtype), v.astype(dtype)


@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("kind", ["rising", "falling", "spike"])
def test_online_softmax_cases(gpu, kind, dtype):
    q, k, v = _online_case(kind, dtype)
    raw = (q.astype(np.float64)[:, 0] @ k.astype(np.float64)[:, 0].T)
    assert (199.0 if dtype == F32 else 59000.0) <= np.abs(raw).max() <= 65504.0
    top = raw.argmax(1)
    assert {"rising": (top >= 192).any(), "falling": (top < 64).any(), "spike": ((top >= 64) & (top < 128)).any()}[kind]
    ref, mag = ar.attention_parts(q, k, v, 1, scale=1.0)
    got = hipops.attention(q, k, v, 1, scale=1.0).astype(np.float64)
    assert np.isfinite(got).all(), kind
    if dtype == F32:
        util.assert_parity(got, ref, what="online " + kind)
        assert np.abs(got.sum(-1) - 1.0).max() <= 1e-5, kind
    else:
        ratio = float((np.abs(got - ref) / half_bar(mag, ref)).max())
        print("online %s fp16: %.3f of the per-element bar" % (kind, ratio))
        assert ratio <= 1.0, kind
        assert np.abs(got.sum(-1) - 1.0).max() <= 2.0 ** -9, kind


@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
def test_identical_keys_give_the_mean_of_v(gpu, dtype):
    lq, lk, batch, heads, d = 17, 129, 2, 3, 8
    q, _, v = qkv(5, lq, lk, batch, heads * d, dtype)
    k = np.broadcast_to(ar.tokens(9, 1, batch, heads * d, dtype=dtype), (lk, batch, heads * d)).copy()
    got = hipops.attention(q, k, v, heads).astype(np.float64)
    mean = np.broadcast_to(v.astype(np.float64).mean(0), got.shape)
    if dtype == F32:
        util.assert_parity(got, mean, what="identical keys")
    else:
        assert (np.abs(got - mean) <= half_bar(np.abs(v.astype(np.float64)).mean(0), mean)).all()


# ---- special values ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
def test_nan_rules(gpu, dtype):
    pytest.importorskip("torch")
    heads, d, lq, lk, batch = 2, 8, 70, 130, 2
    base = qkv(31, lq, lk, batch, heads * d, dtype)
    for which, pos in (("q", (66, 1, 13)), ("k", (129, 0, 2)), ("k", (3, 1, 9)), ("v", (70, 1, 1)), ("v", (0, 0, 15))):
        q, k, v = (t.copy() for t in base)
        {"q": q, "k": k, "v": v}[which][pos] = np.nan
        ref = ar.sdpa_torch(q, k, v, heads)
        got = hipops.attention(q, k, v, heads).astype(np.float64)
        what = "NaN in %s%r" % (which, pos)
        assert np.isnan(ref).any() and np.array_equal(np.isnan(got), np.isnan(ref)), what
        ok = ~np.isnan(ref)
        assert np.abs(got[ok] - ref[ok]).max() <= (1e-5 if dtype == F32 else 2e-3), what


def test_one_key_returns_v_bit_for_bit(gpu):
    for d, heads, batch, lq in ((20, 3, 2, 70), (64, 1, 1, 5), (1, 1, 2, 17)):
        q, k, v = qkv(41, lq, 1, batch, heads * d)
        same_bits(hipops.attention(q, k, v, heads), np.broadcast_to(v, q.shape), "lk = 1, d = %d" % d)


def test_large_finite_inputs_stay_finite(gpu):
    q, k, v = qkv(43, 20, 150, 1, 16, lo=-30.0, hi=30.0)
    got = hipops.attention(q, k, v, 2, scale=1.0)
    assert np.isfinite(got).all()
    util.assert_parity(got, ar.attention_ref(q, k, v, 2, scale=1.0), what="scores to +-7000")


# ---- independence, bit for bit ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,d", [(F32, 20), (F32, 64), (F16, 16), (F16, 64)], ids=["f32_d20", "f32_d64", "f16_d16", "f16_d64"])
def test_independence_bit_for_bit(gpu, dtype, d):
    heads, batch, lq, lk = 3, 2, 81, 131
    e = heads * d
    q, k, v = qkv(51, lq, lk, batch, e, dtype)
    full = hipops.attention(q, k, v, heads)
    same_bits(hipops.attention(q, k, v, heads), full, "two launches")
    for b in range(batch):
        same_bits(hipops.attention(q[:, b:b + 1], k[:, b:b + 1], v[:, b:b + 1], heads), full[:, b:b + 1], "batch item %d alone" % b)
    nan = hipops.ByteFill(0xFF)
    for h in range(heads):
        # heads = 1 on a column slice of rows of E elements: the other heads' columns hold NaN on the input side and stay untouched on the output side
        sl = slice(h * d, (h + 1) * d)
        one = hipops.attention(q[..., sl], k[..., sl], v[..., sl], 1, in_ld=e, in_c_off=h * d, in_fill=nan, out_ld=e, out_c_off=h * d, out_fill=nan)
        same_bits(one, full[..., sl], "head %d alone" % h)
    for i in (0, 15, 16, 63, 64, 80):
        same_bits(hipops.attention(q[i:i + 1], k, v, heads), full[i:i + 1], "query row %d alone" % i)
    for cut in (1, 37, 64):
        same_bits(np.concatenate([hipops.attention(q[:cut], k, v, heads), hipops.attention(q[cut:], k, v, heads)]), full, "lq split at %d" % cut)
    t = lambda a: np.ascontiguousarray(a.transpose(1, 0, 2))
    same_bits(t(hipops.attention(t(q), t(k), t(v), heads, batch_first=True)), full, "batch-first strides")
    same_bits(hipops.attention(q, k, v, heads, packed=False, in_ld=e + 24, in_c_off=8, out_ld=e + 8, out_c_off=8), full, "wider rows")


# ---- views and containment ----------------------------------------------------------------------------------------------------
class ViewCase:
    def __init__(self, vid, half, lq, lk, heads, d, batch, batch_first, packed, **views):
        self.id, self.half, self.packed, self.views = vid, half, packed, views
        self.lq, self.lk, self.heads, self.d, self.batch, self.batch_first = lq, lk, heads, d, batch, batch_first
        self.entries = ("si_hip_attention_f16" if half else "si_hip_attention_f32",)
        self.dtype = F16 if half else F32

    def operands(self):
        return qkv(61, self.lq, self.lk, self.batch, self.heads * self.d, self.dtype, batch_first=self.batch_first)

    def run(self, fill):
        q, k, v = self.operands()
        e = self.heads * self.d
        full = hipops.attention(q, k, v, self.heads, batch_first=self.batch_first, packed=self.packed, in_fill=fill, out_fill=fill, full=True, **self.views)
        return ct.Out("o", full, self.views.get("out_c_off", 0), e)


VIEW_CASES = []
for _half, _sfx in ((False, "f32"), (True, "f16")):
    VIEW_CASES += [
        # q | k | v as the neighbouring slices of ONE [rows, ld >= 3E] buffer (the layer's workspace), o a slice of a wider row; one short of and
        # one past a tile on both sides
        ViewCase("packed_63_" + _sfx, _half, 63, 63, 3, 16, 2, False, True, in_ld=3 * 48 + 16, in_c_off=8, out_ld=72, out_c_off=16),
        ViewCase("packed_65_batch_first_" + _sfx, _half, 65, 65, 2, 8, 2, True, True, in_ld=3 * 16 + 8, in_c_off=0, out_ld=40, out_c_off=8),
        # three buffers of their own, lq past and lk short of a tile, and the other way round
        ViewCase("slices_65_63_" + _sfx, _half, 65, 63, 3, 8, 2, False, False, in_ld=40, in_c_off=16, out_ld=32, out_c_off=8),
        ViewCase("slices_63_65_" + _sfx, _half, 63, 65, 1, 64, 1, True, False, in_ld=80, in_c_off=8, out_ld=72, out_c_off=0),
    ]
VIEW_CASES += [
    # fp32 alone: a head dim that is no multiple of 4 at odd offsets (nothing is vectorised, nothing may be rounded up)
    ViewCase("odd_d_f32", False, 65, 65, 3, 5, 2, False, True, in_ld=50, in_c_off=3, out_ld=19, out_c_off=1),
]


@pytest.mark.parametrize("case", VIEW_CASES, ids=[c.id for c in VIEW_CASES])
def test_views_and_containment(gpu, case):
    del hipops.LAST_ENTRIES[:]
    q, k, v = case.operands()
    dense = hipops.attention(q, k, v, case.heads, batch_first=case.batch_first)
    plain = case.run(hipops.ByteFill(0x00))
    assert set(case.entries) <= set(hipops.LAST_ENTRIES), hipops.LAST_ENTRIES
    assert hipops.LAST_KERNEL_NAME["si_hip_attention"] == ar.kname(case.d, case.dtype)
    ct.assert_outside_fill(plain.full, plain.c_off, plain.c, 0x00, case.id + ", plain run")
    same_bits(plain.full[..., plain.c_off:plain.c_off + plain.c], dense, case.id + " against the dense run")
    for byte in ct.PATTERNS:
        with hipops.guard_bands(byte) as g:      # all bands and the inputs are compared when the block ends
            out = case.run(hipops.ByteFill(byte))
        what = "%s under 0x%02X" % (case.id, byte)
        assert g.checked == (2 if case.packed else 4), "%s: the guard saw %d buffers" % (what, g.checked)
        ct.assert_outside_fill(out.full, out.c_off, out.c, byte, what)
        same_bits(out.full[..., out.c_off:out.c_off + out.c], dense, what)


# ---- layer and engine ---------------------------------------------------------------------------------------------------------
def save(b, tmp_path, tag):
    pp, bp = str(tmp_path / (tag + ".pnnx.param")), str(tmp_path / (tag + ".pnnx.bin"))
    b.save(pp, bp)
    return pp, bp


def graph_outputs(b):
    return [_parse(ln)[2][0] for ln in b.lines if ln.startswith("pnnx.Output")]


def run_engine(b, tmp_path, xs, tag="m", forwards=1, **opts):
    """(engine, the graph output as the engine stores it); xs: one array per graph input, in order"""
    pp, bp = save(b, tmp_path, tag)
    e = Engine(**opts)
    e.load_model(pp, bp)
    xs = xs if isinstance(xs, (list, tuple)) else [xs]
    for name, x in zip(e.input_names(), xs):
        e.input(name, x)
    for _ in range(forwards):
        e.forward()
    (out,) = graph_outputs(b)
    return e, e.extract(out)


def one_op(shapes, **kw):
    b = mg.PnnxBuilder(seed=3)
    xs = [b.input(s) for s in shapes]
    b.output(b.multihead_attention(*xs, **kw))
    return b


def mha_weights(b):
    name = [_parse(ln)[1] for ln in b.lines if ln.startswith("nn.MultiheadAttention")][0]
    a = lambda k: b.attrs.get("%s.%s" % (name, k))
    return a("in_proj_weight"), a("in_proj_bias"), a("out_proj.weight"), a("out_proj.bias")


def composition(xs, w, heads, batch_first):
    """the layer's three stages through the op-level entries: conv 1x1 per input (the row blocks of in_proj_weight that input feeds), the
    attention kernel, conv 1x1"""
    w_in, b_in, w_out, b_out = w
    e = w_out.shape[0]
    blocks = {1: [(0, 3 * e)], 2: [(0, e), (e, 3 * e)], 3: [(0, e), (e, 2 * e), (2 * e, 3 * e)]}[len(xs)]
    cols = []
    for x, (lo, hi) in zip(xs, blocks):
        y = hipops.conv2d(x.reshape(-1, 1, 1, e), w_in[lo:hi].reshape(hi - lo, e, 1, 1), None if b_in is None else b_in[lo:hi])
        cols += [y.reshape(x.shape[:2] + (hi - lo,))[..., j * e:(j + 1) * e] for j in range((hi - lo) // e)]
    att = hipops.attention(cols[0], cols[1], cols[2], heads, batch_first=batch_first)
    return hipops.conv2d(att.reshape(-1, 1, 1, e), w_out.reshape(e, e, 1, 1), b_out).reshape(att.shape)


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "no_bias"])
@pytest.mark.parametrize("batch_first", [False, True], ids=["seq_first", "batch_first"])
@pytest.mark.parametrize("n_in", [1, 2, 3])
def test_layer_in_a_one_operator_graph(gpu, tmp_path, n_in, batch_first, bias):
    e, heads, lq, lk, batch = 40, 5, 70, (70 if n_in == 1 else 33), 2
    shape = lambda l: (batch, l, e) if batch_first else (l, batch, e)
    b = one_op([shape(lq)] + [shape(lk)] * (n_in - 1), num_heads=heads, batch_first=batch_first, bias=bias)
    xs = [ar.tokens(70 + j, lq if j == 0 else lk, batch, e, batch_first=batch_first) for j in range(n_in)]
    eng, got = run_engine(b, tmp_path, xs)
    w = mha_weights(b)
    util.assert_parity(got, ar.mha_ref(xs, *w, heads, batch_first), what="MHA layer, %d inputs" % n_in)
    same_bits(got, composition(xs, w, heads, batch_first), "MHA layer against conv2d -> attention -> conv2d")
    (layer,) = [L for L in eng.profile() if L["type"] == "nn.MultiheadAttention"]
    assert layer["kernel"] == ar.kname(e // heads, F32)
    rows_q, rows_k = batch * lq, batch * lk
    assert layer["flops"] == 2.0 * e * e * (2 * rows_q + 2 * rows_k) + 4.0 * batch * heads * lq * lk * (e // heads)
    _, cap = run_engine(b, tmp_path, xs, forwards=3, graph=1)
    same_bits(cap, got, "captured replay")


TOYS = {"c3tr": (mg.build_toy_c3tr, 2), "mhsa_head": (mg.build_toy_mhsa_head, 1)}


def toy_input(b):
    n, c, h, w = b.shapes["0"]
    return mg.synth_input((n, h, w, c))


@pytest.mark.parametrize("which", sorted(TOYS))
def test_toys_fp32(gpu, tmp_path, which):
    build, n_mha = TOYS[which]
    b = build()
    x = toy_input(b)
    want = ar.eval_graph(b, x)
    eng, got = run_engine(b, tmp_path, x)
    util.assert_parity(got, want, what="toy " + which)
    prof = eng.profile()
    mha = [L for L in prof if L["type"] == "nn.MultiheadAttention"]
    assert len(mha) == n_mha and all(L["kernel"] == "attention_kernel<float, 16>" for L in mha), mha
    if which == "mhsa_head":
        views = [L for L in prof if L["type"] in ("Tensor.view", "Tensor.permute")]
        assert views and all(L["kernel"] == "view" for L in views), views     # permute -> view on either side of the layer moves nothing
    _, cap = run_engine(b, tmp_path, x, forwards=3, graph=1)
    same_bits(cap, got, which + " captured")
    _, plain = run_engine(b, tmp_path, x, fuse=0, alias_view=0)
    same_bits(plain, got, which + " fuse=0 alias_view=0")


@pytest.mark.parametrize("which", sorted(TOYS))
def test_toys_fp16_storage(gpu, tmp_path, which):
    """the engine's error against plain float64 held to 4x the error of the float64 emulation that rounds to fp16 wherever the engine stores
    a half tensor (the margin: one rounding that may land one ulp either way at each of those stores)"""
    build, n_mha = TOYS[which]
    b = build()
    x = toy_input(b)
    exact, emulated = ar.eval_graph(b, x), ar.eval_graph(b, x, rnd=ar.round_f16)
    eng, got = run_engine(b, tmp_path, x, fp16=1)
    scale = np.abs(exact).max()
    err, emu = np.abs(got - exact).max() / scale, np.abs(emulated - exact).max() / scale
    print("toy %s fp16 storage: engine %.3e, emulation %.3e (max|d| / max|ref| against float64)" % (which, err, emu))
    mha = [L for L in eng.profile() if L["type"] == "nn.MultiheadAttention"]
    assert len(mha) == n_mha and all(L["kernel"] == "attention_kernel<_Float16, 32>" for L in mha), mha
    assert np.isfinite(got).all() and err <= 4.0 * emu, (err, emu)
    _, cap = run_engine(b, tmp_path, x, forwards=3, graph=1, fp16=1)
    same_bits(cap, got, which + " fp16 captured")


@pytest.mark.parametrize("fp16", [0, 1])
@pytest.mark.parametrize("which", sorted(TOYS))
def test_toys_rebatched(gpu, tmp_path, which, fp16):
    """SetOption("batch", 3) on the file traced at batch 2 gives the bits of the file built at batch 3, in both batch_first settings: the
    batch is dimension 0 of the MHSA head's [N, L, E] tokens and dimension 1 of C3TR's [L, N, E] tokens, where the engine's rewrite follows
    it through flatten(2) -> permute(2, 0, 1), the Linears, the attention layers and the adds, and back through permute(1, 2, 0) -> reshape"""
    build = TOYS[which][0]
    b2, b3 = build(batch=2), build(batch=3)
    x = toy_input(b3)
    _, want = run_engine(b3, tmp_path, x, tag="b3", fp16=fp16)
    eng, got = run_engine(b2, tmp_path, x, tag="b2", batch=3, fp16=fp16)
    same_bits(got, want, which + " batch=3")
    if which == "c3tr":
        mha = [_parse(ln) for ln in b2.lines if ln.startswith("nn.MultiheadAttention")][0]
        assert b2.shapes[mha[3][0]] == (64, 2, 32) and eng.operand_shape(mha[3][0]) == (64, 3, 32)


def test_rebatch_refuses_what_it_cannot_follow(gpu, tmp_path):
    """a seq-first token tensor as a graph input: dimension 0 is L, the re-batch cannot know where N is -- kUnsupport at LoadModel with the
    reason logged, instead of a rewritten sequence length; batch_first tokens as a graph input re-batch, and L == the traced batch stays L"""
    b = one_op([(7, 2, 24)], num_heads=3)
    pp, bp = save(b, tmp_path, "seq_first_input")
    with pytest.raises(StatusError) as ei:
        Engine(batch=5).load_model(pp, bp)
    assert ei.value.status == Status.kUnsupport
    _, got = run_engine(b, tmp_path, ar.tokens(1, 7, 2, 24))                      # ... and loads without the option
    assert got.shape == (7, 2, 24)
    b2, b3 = (one_op([(n, 2, 24)], num_heads=3, batch_first=True) for n in (2, 3))   # [N, L = 2, E]: L equals the traced batch
    x = ar.tokens(2, 2, 3, 24, batch_first=True)
    _, want = run_engine(b3, tmp_path, x, tag="bf3")
    _, got = run_engine(b2, tmp_path, x, tag="bf2", batch=3)
    assert got.shape == (3, 2, 24)
    same_bits(got, want, "batch_first tokens as the graph input, batch=3")


def test_flatten_of_a_map_under_fp16_storage(gpu, tmp_path):
    """torch.flatten of a map with H W > 1 has no half path: under fp16 storage it runs in fp32 between casts (it used to fail at Forward)"""
    b = mg.build_toy_view_classifier(pool=2, flatten=True)
    x = toy_input(b)
    _, f32 = run_engine(b, tmp_path, x)
    eng, got = run_engine(b, tmp_path, x, fp16=1)
    assert np.isfinite(got).all() and np.abs(got - f32).max() <= 2e-2 * np.abs(f32).max()
    (flat,) = [L for L in eng.profile() if L["type"] == "torch.flatten"]
    assert flat["kernel"] == "nhwc_to_nchw"
    _, view = run_engine(mg.build_toy_view_classifier(pool=2), tmp_path, x, tag="view", fp16=1)     # the same model through Tensor.view
    assert np.abs(got - view).max() <= 2e-2 * np.abs(f32).max()


def test_fp16_fallback_for_dims_off_eight(gpu, tmp_path):
    """E = 20 / head dim 4 (and E = 24 / head dim 12) under fp16 storage: HalfStorageOk refuses, the layer runs in fp32 between casts"""
    for e, heads in ((20, 5), (24, 2)):
        b = mg.PnnxBuilder(seed=4)
        x0 = b.input((2, 3, 8, 8))
        t = b.view(b.permute(b.relu(b.conv(x0, e, 3, 1, 1)), (0, 2, 3, 1)), (2, -1, e))
        t = b.multihead_attention(t, num_heads=heads, batch_first=True)
        b.output(b.relu(b.conv(b.view(b.permute(t, (0, 2, 1)), (2, e, 8, 8)), 8, 1)))
        x = toy_input(b)
        exact = ar.eval_graph(b, x)
        eng, got = run_engine(b, tmp_path, x, fp16=1)
        (layer,) = [L for L in eng.profile() if L["type"] == "nn.MultiheadAttention"]
        assert layer["kernel"] == ar.kname(e // heads, F32), layer
        assert np.abs(got - exact).max() <= 2e-2 * np.abs(exact).max()


# ---- nn.Linear on rank 3 ------------------------------------------------------------------------------------------------------
def linear_graph(shape, out_f, bias=True):
    b = mg.PnnxBuilder(seed=6)
    b.output(b.linear(b.input(shape), out_f, bias=bias))
    return b


def test_linear_on_rank3_fp32(gpu, tmp_path):
    for shape, out_f, bias in (((33, 2, 24), 40, True), ((2, 65, 7), 5, False), ((1, 1, 16), 16, True)):
        b = linear_graph(shape, out_f, bias)
        x = ar.tokens(80, shape[0], shape[1], shape[2])
        name = _parse(b.lines[1])[1]
        w, bi = b.attrs[name + ".weight"].astype(np.float64), b.attrs[name + ".bias"].astype(np.float64)
        eng, got = run_engine(b, tmp_path, x)
        assert got.shape == shape[:2] + (out_f,)
        util.assert_parity(got, x.astype(np.float64) @ w.T + (bi if bias else 0.0), what="Linear on %r" % (shape,))
        # the folded rank-2 problem: same bits, same kernel
        b2 = linear_graph((shape[0] * shape[1], shape[2]), out_f, bias)
        eng2, got2 = run_engine(b2, tmp_path, x.reshape(-1, shape[2]), tag="r2")
        same_bits(got.reshape(got2.shape), got2, "rank 3 against the folded rank 2")
        same_bits(got2, hipops.conv2d(x.reshape(-1, 1, 1, shape[2]), b.attrs[name + ".weight"].reshape(out_f, shape[2], 1, 1),
                                      b.attrs[name + ".bias"] if bias else None).reshape(got2.shape), "rank-2 Linear against conv2d 1x1")
        k3, k2 = ([L["kernel"] for L in e_.profile() if L["type"] == "nn.Linear"] for e_ in (eng, eng2))
        assert k3 == k2 and len(k3) == 1, (k3, k2)


def test_linear_on_rank3_fp16(gpu, tmp_path):
    """between two elementwise layers, so that its operands are stored as halves"""
    b = mg.PnnxBuilder(seed=7)
    y = b.linear(b.relu(b.input((33, 2, 24))), 40)
    b.output(b.relu(y))
    x = ar.tokens(81, 33, 2, 24)
    name = [_parse(ln)[1] for ln in b.lines if ln.startswith("nn.Linear")][0]
    w, bi = b.attrs[name + ".weight"].astype(np.float64), b.attrs[name + ".bias"].astype(np.float64)
    r = ar.round_f16
    want = np.maximum(r(np.maximum(x.astype(np.float64), 0)) @ r(w).T + bi, 0)
    eng, got = run_engine(b, tmp_path, x, fp16=1)
    assert np.abs(got - want).max() <= 2.0 ** -9 * np.abs(want).max()
    # the folded rank-2 graph under fp16 storage: the same native half kernel (no fp32 fallback, no casts around the layer), the same bits
    b2 = mg.PnnxBuilder(seed=7)
    b2.output(b2.relu(b2.linear(b2.relu(b2.input((66, 24))), 40)))
    eng2, got2 = run_engine(b2, tmp_path, x.reshape(66, 24), tag="r2", fp16=1)
    same_bits(got.reshape(66, 40), got2, "rank-3 fp16 Linear against the folded rank 2")
    k3, k2 = ([L["kernel"] for L in e_.profile() if L["type"] == "nn.Linear"] for e_ in (eng, eng2))
    assert k3 == k2 and len(k3) == 1, (k3, k2)
    assert [L["type"] for L in eng.profile()] == [L["type"] for L in eng2.profile()]


def test_refused_at_load(gpu, tmp_path):
    """kUnsupport with a logged reason at LoadModel, kFail for a missing key; the process goes on"""
    def load(b, tag):
        pp, bp = save(b, tmp_path, tag)
        with pytest.raises(StatusError) as ei:
            Engine().load_model(pp, bp)
        return ei.value.status

    assert load(one_op([(7, 2, 24)], num_heads=3, add_bias_kv=True), "bias_kv") == Status.kUnsupport
    assert load(one_op([(7, 2, 24)], num_heads=3, add_zero_attn=True), "zero_attn") == Status.kUnsupport
    assert load(one_op([(7, 2, 24)], num_heads=3, kdim=16), "kdim") == Status.kUnsupport
    assert load(one_op([(7, 2, 24)], num_heads=3, vdim=16), "vdim") == Status.kUnsupport
    assert load(one_op([(7, 2, 24)], num_heads=5), "heads") == Status.kUnsupport
    assert load(one_op([(3, 1, 272)], num_heads=2), "wide") == Status.kUnsupport
    b = one_op([(7, 2, 24)], num_heads=3, need_weights=True)          # the attention weights as a second output operand
    assert len(_parse(b.lines[-2])[3]) == 2 and load(b, "weights") == Status.kUnsupport
    b = mg.PnnxBuilder(seed=3)                                          # attn_mask: a fourth input operand
    xs = [b.input((7, 2, 24)) for _ in range(3)] + [b.input((7, 7))]
    b.multihead_attention(*xs[:3], num_heads=3)
    toks = b.lines[-1].split()
    toks[2] = "4"
    toks.insert(7, xs[3])
    b.lines[-1] = " ".join(toks + ["#%s=(7,7)f32" % xs[3]])
    b.output(_parse(b.lines[-1])[3][0])
    assert len(_parse(b.lines[-2])[2]) == 4 and load(b, "mask") == Status.kUnsupport
    for drop in ("num_heads=", "batch_first=", "kdim=", "@in_proj_weight=", "@out_proj.bias="):
        b = one_op([(7, 2, 24)], num_heads=3)
        b.lines[-2] = " ".join(t for t in b.lines[-2].split() if not t.startswith(drop))
        assert load(b, "missing") == Status.kFail, drop
    b = one_op([(7, 2, 24)], num_heads=3)
    x = ar.tokens(1, 7, 2, 24)
    _, got = run_engine(b, tmp_path, x)
    util.assert_parity(got, ar.mha_ref([x], *mha_weights(b), 3), what="after the refusals")
