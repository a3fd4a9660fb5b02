"""GPU: the recurrent step kernel (include/si_rnn.h) and nn.LSTM / nn.GRU.  Kernel: fp32 against float64 with torch's CPU fp32 modules as
the yardstick, fp16 storage against the rounding restatement of tests/rnn_reference.py, the bit-for-bit invariants (batch item alone, prefix
and suffix of the sequence, directions apart, batch_first, states, two runs, a continued call), saturated gates, the NaN rule, T = 1 on
poisoned workspaces, views under guard bands.  Layer and engine: one-operator graphs against the op-level composition, build_toy_crnn in
every variant in fp32 and under fp16 storage, captured, re-batched, batch-split, and the kUnsupport paths.

Shapes are small: T <= 12, N in {1, 2, 16, 17}, I in {5, 8, 32}, H in {1, 15, 16, 20, 33, 64, 136} and one case of H = 256."""
import numpy as np
import pytest

import containment as ct
import rnn_reference as rr
import util
from ct_reference import _parse
from simpleinfer_amd import hipops, modelgen as mg
from simpleinfer_amd.engine import Engine, Status, StatusError

pytestmark = pytest.mark.gpu

F32, F16 = np.float32, np.float16
CELLS = ("lstm", "gru")
RUN = {"lstm": hipops.lstm, "gru": hipops.gru}


def record(line):
    print("rnn: " + line)


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    w = np.uint32 if got.dtype.itemsize == 4 else np.uint16
    bad = np.nonzero(got.view(w) != want.view(w))
    assert bad[0].size == 0, "%s: %d of %d elements differ in bits, first at %s" % (what, bad[0].size, got.size, tuple(int(b[0]) for b in bad))


# ---- accuracy -------------------------------------------------------------------------------------------------------------------
# (H, N, I, T, dirs, layers): every H of the table, every N, every I; one block, a ragged block, more than one block of units and of rows
F32_CASES = [(1, 1, 5, 3, 1, 1), (15, 2, 8, 12, 2, 1), (16, 16, 32, 5, 2, 2), (20, 17, 5, 7, 2, 1), (33, 17, 8, 12, 1, 2), (64, 16, 32, 6, 2, 1),
             (136, 2, 8, 4, 2, 1), (256, 17, 32, 3, 2, 1)]
FLOOR = 2.0 ** -20   # 8 ulp at 1: outputs lie in (-1, 1)


@pytest.mark.parametrize("case", F32_CASES, ids=["H%d_N%d_I%d_T%d_D%d_L%d" % c for c in F32_CASES])
@pytest.mark.parametrize("cell", CELLS)
def test_fp32_against_float64(gpu, cell, case):
    """max abs error of y (and of h_n), and of c_n relative to max(1, |c|), against float64; the yardstick is the error of torch's own CPU
    fp32 module on the same data, which the kernel may exceed 4 times (another reduction order, the device's sigmoid / tanh), floor 2^-20"""
    pytest.importorskip("torch")
    hid, n, i, t, dirs, layers = case
    w = rr.make_weights(cell, i, hid, layers, dirs, True, seed=hid)
    x = rr.sequence(100 + hid, t, n, i)
    ref = rr.rnn_ref(cell, x, w)
    cpu = rr.rnn_torch(cell, x, w, dtype=F32)
    got = RUN[cell](x, w, want_state=True)
    assert hipops.LAST_KERNEL_NAME["si_hip_rnn"] == rr.kname(cell, F32)
    for j, what in enumerate(("y", "h_n", "c_n")[:len(got)]):
        scale = np.maximum(1.0, np.abs(ref[j])) if what == "c_n" else 1.0
        err = float((np.abs(got[j].astype(np.float64) - ref[j]) / scale).max())
        yard = float((np.abs(cpu[j] - ref[j]) / scale).max())
        bar = max(4.0 * yard, FLOOR)
        record("fp32 %s H=%d N=%d I=%d T=%d D=%d L=%d %s: kernel %.3e, torch CPU fp32 %.3e, ratio %.2f, bar %.3e" % (
            cell, hid, n, i, t, dirs, layers, what, err, yard, err / yard if yard else 0.0, bar))
        assert np.isfinite(got[j]).all() and err <= bar, (what, err, yard)


F16_CASES = [(16, 16, 32, 5, 2, 2), (64, 17, 8, 12, 2, 1), (136, 2, 8, 4, 2, 1), (256, 17, 32, 3, 2, 1), (16, 1, 8, 12, 1, 1)]
# The fp16 bar: |got - restatement| <= 1 fp16 ulp of the restatement's value (a store that lands on the other side of a tie; ulp of v:
# 2^(floor(log2 |v|) - 10), at least 2^-24) + the propagated effect of such 1-ulp differences in earlier steps, in the layer below and in the
# stored gates, which is absolute: a gate of magnitude 1 .. 4 moves by 2^-10 .. 2^-9, h by 2^-11, whatever the size of the value they end in.
# That second term is MEASURED, in units of 2^-11 (the ulp of the largest outputs, |y| < 1): the worst case of this table on the GPU is
# MEASURED_PROPAGATED (GRU, H = 64, T = 12; at most 0.6 % of the elements of a case differ from the restatement at all, by up to 81 of
# their own ulps where the value is tiny), and the bar is four times that: 2^-13 absolute beyond the one ulp.
MEASURED_PROPAGATED = 0.0625
F16_PROPAGATED_BAR = 4.0 * MEASURED_PROPAGATED


def ulp16(ref):
    ref = np.asarray(ref, np.float64)
    with np.errstate(divide="ignore"):
        e = np.floor(np.log2(np.abs(ref)))
    return 2.0 ** (np.maximum(e, -14.0) - 10.0)


@pytest.mark.parametrize("case", F16_CASES, ids=["H%d_N%d_I%d_T%d_D%d_L%d" % c for c in F16_CASES])
@pytest.mark.parametrize("cell", CELLS)
def test_fp16_against_the_rounding_restatement(gpu, cell, case):
    hid, n, i, t, dirs, layers = case
    w = rr.make_weights(cell, i, hid, layers, dirs, True, seed=hid)
    x = rr.sequence(200 + hid, t, n, i, dtype=F16)
    ref = rr.rnn_ref(cell, x, w, rnd=rr.round_f16)
    got = RUN[cell](x, w, want_state=True)
    assert got[0].dtype == F16 and hipops.LAST_KERNEL_NAME["si_hip_rnn"] == rr.kname(cell, F16)
    worst = []
    for j, what in enumerate(("y", "h_n", "c_n")[:len(got)]):
        want = rr.round_f16(ref[j]) if what == "c_n" else ref[j]      # (c_n is c rounded to the storage type)
        d = np.abs(got[j].astype(np.float64) - want)
        own = float((d / ulp16(want)).max())
        prop = float(((d - ulp16(want)) / 2.0 ** -11).max())
        off = float((d > 0).mean())
        record("fp16 %s H=%d N=%d I=%d T=%d D=%d L=%d %s: %.1f %% of the elements off the restatement, worst %.2f of its own ulp; beyond one own ulp "
               "%.3f x 2^-11" % (cell, hid, n, i, t, dirs, layers, what, 100.0 * off, own, prop))
        assert np.isfinite(got[j]).all(), what
        worst.append((prop, what))
    assert max(worst)[0] <= F16_PROPAGATED_BAR, worst


# ---- bit-for-bit invariants -------------------------------------------------------------------------------------------------------
def flip(a):
    return np.ascontiguousarray(a[::-1])


@pytest.mark.parametrize("dtype,hid,i", [(F32, 20, 5), (F32, 136, 8), (F16, 16, 8), (F16, 136, 32)], ids=["f32_H20", "f32_H136", "f16_H16", "f16_H136"])
@pytest.mark.parametrize("cell", CELLS)
def test_invariants_bit_for_bit(gpu, cell, dtype, hid, i):
    t, n = 9, 17
    w = rr.make_weights(cell, i, hid, 1, 2, True, seed=7)
    fwd, rev = [[w[0][0]]], [[w[0][1]]]
    x = rr.sequence(31, t, n, i, dtype=dtype)
    run = RUN[cell]
    full = run(x, w, want_state=True)
    y = full[0]
    again = run(x, w, want_state=True)
    for a, b, what in zip(full, again, ("y", "h_n", "c_n")):
        same_bits(a, b, "two runs, " + what)
    # a batch item alone: the first and the last of the first tile, the only one of the second
    for b in (0, 15, 16):
        same_bits(run(x[:, b:b + 1], w), y[:, b:b + 1], "batch item %d alone" % b)
    # the directions apart: the reverse direction on its own is the forward kernel on the mirrored sequence
    yf = run(x, fwd)
    yr = flip(run(flip(x), rev))
    same_bits(np.concatenate([yf, yr], axis=2), y, "bidirectional against forward | reverse")
    # a prefix of the sequence in the forward direction, a suffix in the reverse direction
    for cut in (1, 4, 8):
        same_bits(run(x[:cut], fwd), y[:cut, :, :hid], "forward y[:%d] against a run of length %d" % (cut, cut))
        same_bits(run(x[t - cut:], w)[..., hid:], y[t - cut:, :, hid:], "reverse y[%d:] against a run on the last %d steps" % (t - cut, cut))
    # batch_first is seq-first on the transposed data
    tr = lambda a: np.ascontiguousarray(a.transpose(1, 0, 2))
    bf = run(tr(x), w, batch_first=True, want_state=True)
    same_bits(tr(bf[0]), y, "batch_first y")
    for a, b, what in zip(bf[1:], full[1:], ("h_n", "c_n")):
        same_bits(a, b, "batch_first " + what)
    # h_n is the last forward row and the first reverse row of y
    same_bits(full[1][0], y[t - 1, :, :hid], "h_n forward")
    same_bits(full[1][1], y[0, :, hid:], "h_n reverse")


@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("cell", CELLS)
def test_a_continued_call_equals_one_call(gpu, cell, dtype):
    """step0: a forward layer of 9 steps as one call, and as steps 0 .. 3 (a call of length 4) followed by a call with step0 = 4 on the y
    and the c buffer the first one left -- the same bits; the rows the second call does not own start as NaN bytes"""
    t, n, hid, cut = 9, 3, 24, 4
    w = rr.make_weights(cell, 8, hid, 1, 1, True, seed=9)
    w_hh = np.stack([d[1] for d in w[0]])
    b_hn = np.stack([d[3][2 * hid:] for d in w[0]]) if cell == "gru" else None
    gates = rr.sequence(32, t, n, rr.GATES[cell] * hid, dtype=dtype)
    one = hipops.rnn_layer(cell, gates, w_hh, b_hn, want_state=True, return_c=True)
    y4, c4 = hipops.rnn_layer(cell, gates[:cut], w_hh, b_hn, return_c=True)
    same_bits(y4, one[0][:cut], "the first %d steps" % cut)
    y0 = hipops._full((t, n, hid), dtype, hipops.ByteFill(0xFF))
    y0[:cut] = y4
    two = hipops.rnn_layer(cell, gates, w_hh, b_hn, step0=cut, resume=(y0, c4), want_state=True, return_c=True)
    assert len(two) == len(one)
    for a, b in zip(two, one):
        if a is not None or b is not None:
            same_bits(a, b, "continued call")


# ---- edge cases -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("big", [100.0, 1e4])
@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
def test_saturated_gates_are_exact(gpu, dtype, big):
    """pre-activations of +-100 / +-1e4 (W_hh = 0: the gates are the pre-activations): sigmoid reads exactly 1 / 0, nothing is NaN.
    LSTM unit kinds: A all gates +big: c_1 = 1, c_2 = 2 exactly; B i = -big: c stays 0, h = 0.  GRU: A z = +big: h = h_prev = 0 exactly;
    B z = r = -big, n's gate 0.5: r = 0 exactly wipes the huge b_hn, h = tanh(0.5)"""
    t, n, hid = 2, 3, 8
    # LSTM
    g = np.full((t, n, 4, hid), big, np.float64)
    g[:, :, 0, 4:] = -big                       # units 4..7: i = -big
    got = hipops.rnn_layer("lstm", g.reshape(t, n, 4 * hid).astype(dtype), np.zeros((1, 4 * hid, hid), F32), want_state=True, return_c=True)
    y, h_n, c_n, c = got
    assert all(np.isfinite(a).all() for a in got)
    assert np.array_equal(c[0, :, :4], np.full((n, 4), 2.0, F32)) and np.array_equal(c[0, :, 4:], np.zeros((n, 4), F32))
    assert np.array_equal(c_n.astype(F32), c) and np.array_equal(y[:, :, 4:], np.zeros((t, n, 4), dtype))
    assert np.abs(y[:, :, :4].astype(np.float64) - np.tanh([[[1.0]], [[2.0]]])).max() <= (2.0 ** -20 if dtype == F32 else 2.0 ** -11)
    # GRU
    g = np.zeros((t, n, 3, hid), np.float64)
    g[:, :, 1, :4] = big                        # units 0..3: z = 1
    g[:, :, 0, 4:] = g[:, :, 1, 4:] = -big      # units 4..7: r = z = 0
    g[:, :, 2, :] = 0.5
    b_hn = np.full((1, hid), 1e30, F32)
    y, h_n = hipops.rnn_layer("gru", g.reshape(t, n, 3 * hid).astype(dtype), np.zeros((1, 3 * hid, hid), F32), b_hn, want_state=True)
    assert np.isfinite(y).all() and np.isfinite(h_n).all()
    assert np.array_equal(y[:, :, :4], np.zeros((t, n, 4), dtype))
    assert np.abs(y[:, :, 4:].astype(np.float64) - np.tanh(0.5)).max() <= (2.0 ** -20 if dtype == F32 else 2.0 ** -11)


@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("cell", CELLS)
def test_nan_rule(gpu, cell, dtype):
    """a NaN in x[s, b, :] makes item b NaN from s onward in the forward direction and from s backward in the reverse direction; every
    other element keeps the bits of the clean run"""
    t, n, i, hid = 8, 17, 8, 16
    w = rr.make_weights(cell, i, hid, 1, 2, True, seed=11)
    x = rr.sequence(41, t, n, i, dtype=dtype)
    clean = RUN[cell](x, w)
    for s, b in ((3, 16), (0, 2), (7, 15)):
        xn = x.copy()
        xn[s, b, 5] = np.nan
        got = RUN[cell](xn, w)
        want = np.zeros(got.shape, bool)
        want[s:, b, :hid] = True
        want[:s + 1, b, hid:] = True
        assert np.array_equal(np.isnan(got), want), "NaN at (%d, %d): the NaN mask is not the rule's" % (s, b)
        same_bits(np.where(want, 0, got).astype(dtype), np.where(want, 0, clean).astype(dtype), "NaN at (%d, %d): the other elements" % (s, b))


@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("cell", CELLS)
def test_one_step_reads_nothing_stale(gpu, cell, dtype):
    """T = 1: the product is skipped; y, the states and the c buffer start as NaN bytes and the result is the restatement's"""
    n, i, hid = 17, 8, 24
    w = rr.make_weights(cell, i, hid, 2, 2, True, seed=13)
    x = rr.sequence(51, 1, n, i, dtype=dtype)
    got = RUN[cell](x, w, want_state=True, out_fill=hipops.ByteFill(0xFF))
    ref = rr.rnn_ref(cell, x, w, rnd=rr.round_f16 if dtype == F16 else None)
    for a, b, what in zip(got, ref, ("y", "h_n", "c_n")):
        assert np.isfinite(a).all(), what
        assert np.abs(a.astype(np.float64) - b).max() <= (2.0 ** -18 if dtype == F32 else 2.0 ** -9), what


# ---- views and containment ----------------------------------------------------------------------------------------------------
class ViewCase:
    def __init__(self, vid, cell, half, t, n, hid, dirs, batch_first, **views):
        self.id, self.cell, self.half, self.views = vid, cell, half, views
        self.t, self.n, self.hid, self.dirs, self.batch_first = t, n, hid, dirs, batch_first
        sfx = "f16" if half else "f32"
        self.entries = ("si_hip_rnn_layer_" + sfx, "si_hip_rnn_pack_whh_" + sfx)
        self.dtype = F16 if half else F32

    def operands(self):
        w = rr.make_weights(self.cell, 8, self.hid, 1, self.dirs, True, seed=17)
        gates = rr.sequence(61, self.t, self.n, self.dirs * rr.GATES[self.cell] * self.hid, batch_first=self.batch_first, dtype=self.dtype)
        b_hn = np.stack([d[3][2 * self.hid:] for d in w[0]]) if self.cell == "gru" else None
        return gates, np.stack([d[1] for d in w[0]]), b_hn

    def run(self, fill, **more):
        gates, w_hh, b_hn = self.operands()
        v = dict(self.views, **more)
        return hipops.rnn_layer(self.cell, gates, w_hh, b_hn, batch_first=self.batch_first, want_state=True, g_fill=fill, out_fill=fill, full=True, **v)


VIEW_CASES = []
for _half, _sfx in ((False, "f32"), (True, "f16")):
    VIEW_CASES += [
        # gates and y as column slices of wider rows, one row past a tile of batch rows; both cells, both orders
        ViewCase("lstm_slices_" + _sfx, "lstm", _half, 5, 17, 24, 2, False, g_ld=2 * 4 * 24 + 16, g_c_off=8, out_ld=64, out_c_off=8),
        ViewCase("gru_batch_first_" + _sfx, "gru", _half, 6, 3, 72, 1, True, g_ld=3 * 72 + 8, g_c_off=0, out_ld=88, out_c_off=16),
    ]
VIEW_CASES += [
    # fp32 alone: H that is no multiple of 4 at odd offsets (nothing is vectorised, nothing may be rounded up)
    ViewCase("lstm_odd_f32", "lstm", False, 4, 2, 15, 2, False, g_ld=2 * 4 * 15 + 3, g_c_off=1, out_ld=37, out_c_off=3),
    ViewCase("gru_odd_f32", "gru", False, 3, 17, 33, 2, True, g_ld=2 * 3 * 33 + 5, g_c_off=2, out_ld=71, out_c_off=5),
]


@pytest.mark.parametrize("case", VIEW_CASES, ids=[c.id for c in VIEW_CASES])
def test_views_and_containment(gpu, case):
    del hipops.LAST_ENTRIES[:]
    gates, w_hh, b_hn = case.operands()
    dense = hipops.rnn_layer(case.cell, gates, w_hh, b_hn, batch_first=case.batch_first, want_state=True)
    plain = case.run(hipops.ByteFill(0x00))
    assert set(case.entries) <= set(hipops.LAST_ENTRIES), hipops.LAST_ENTRIES
    assert hipops.LAST_KERNEL_NAME["si_hip_rnn"] == rr.kname(case.cell, case.dtype)
    yw, off = case.dirs * case.hid, case.views["out_c_off"]
    ct.assert_outside_fill(plain[0], off, yw, 0x00, case.id + ", plain run")
    same_bits(plain[0][..., off:off + yw], dense[0], case.id + " against the dense run")
    for byte in ct.PATTERNS:
        with hipops.guard_bands(byte) as g:      # all bands and the inputs (gates, image, b_hn) are compared when the block ends
            out = case.run(hipops.ByteFill(byte))
        what = "%s under 0x%02X" % (case.id, byte)
        # the image, the gates, y, h_n and c, c_n (LSTM) or b_hn (GRU)
        assert g.checked == (6 if case.cell == "lstm" else 5), "%s: the guard saw %d buffers" % (what, g.checked)
        ct.assert_outside_fill(out[0], off, yw, byte, what)
        same_bits(out[0][..., off:off + yw], dense[0], what)
        for a, b, name in zip(out[1:], dense[1:], ("h_n", "c_n")):
            same_bits(a, b, what + ", " + name)


# ---- layer and engine ---------------------------------------------------------------------------------------------------------
def save(b, tmp_path, tag):
    pp, bp = str(tmp_path / (tag + ".pnnx.param")), str(tmp_path / (tag + ".pnnx.bin"))
    b.save(pp, bp)
    return pp, bp


def graph_outputs(b):
    return [_parse(ln)[2][0] for ln in b.lines if ln.startswith("pnnx.Output")]


def run_engine(b, tmp_path, x, tag="m", forwards=1, **opts):
    """(engine, the graph outputs in file order, as the engine stores them)"""
    pp, bp = save(b, tmp_path, tag)
    e = Engine(**opts)
    e.load_model(pp, bp)
    e.input(e.input_names()[0], x)
    for _ in range(forwards):
        e.forward()
    return e, [e.extract(o) for o in graph_outputs(b)]


def status_of_load(b, tmp_path, tag, **opts):
    pp, bp = save(b, tmp_path, tag)
    try:
        Engine(**opts).load_model(pp, bp)
    except StatusError as ex:
        return ex.status
    return Status.kSuccess


@pytest.mark.parametrize("states", [False, True], ids=["y", "y_states"])
@pytest.mark.parametrize("batch_first", [False, True], ids=["seq_first", "batch_first"])
@pytest.mark.parametrize("cell", CELLS)
def test_layer_in_a_one_operator_graph(gpu, tmp_path, cell, batch_first, states):
    """two layers, both directions: the layer against float64, and bit for bit against the op-level chain conv2d -> rnn_layer per layer"""
    t, n, i, hid = 7, 3, 12, 20
    b = mg.PnnxBuilder(seed=3)
    x0 = b.input((n, t, i) if batch_first else (t, n, i))
    outs = (b.lstm if cell == "lstm" else b.gru)(x0, hid, num_layers=2, bidirectional=True, batch_first=batch_first, states=states)
    for o in (outs if states else (outs,)):
        b.output(o)
    name = [_parse(ln)[1] for ln in b.lines if ln.startswith(("nn.LSTM", "nn.GRU"))][0]
    w = rr.builder_weights(b, name, cell, 2, 2, True)
    x = rr.sequence(70, t, n, i, batch_first=batch_first)
    eng, got = run_engine(b, tmp_path, x)
    ref = rr.rnn_ref(cell, x, w, batch_first)
    chain = RUN[cell](x, w, batch_first=batch_first, want_state=True)
    for g, r, c, what in zip(got, ref, chain, ("y", "h_n", "c_n")):
        assert np.abs(g.astype(np.float64) - r).max() <= 2e-5, what
        same_bits(g, c, "layer against the op-level chain, " + what)
    (layer,) = [L for L in eng.profile() if L["type"] in ("nn.LSTM", "nn.GRU")]
    assert layer["kernel"] == rr.kname(cell, F32)
    gh = 2 * rr.GATES[cell] * hid
    assert layer["flops"] == 2.0 * t * n * gh * (i + hid) + 2.0 * t * n * gh * (2 * hid + hid)
    _, cap = run_engine(b, tmp_path, x, forwards=3, graph=1)
    for g, c in zip(got, cap):
        same_bits(c, g, "captured replay")


TOYS = [("lstm", False, False), ("lstm", True, False), ("gru", False, False), ("gru", True, False), ("lstm", False, True)]
TOY_IDS = ["%s_%s%s" % (c, "batch_first" if bf else "seq_first", "_states" if st else "") for c, bf, st in TOYS]


def toy_input(b):
    n, c, h, w = b.shapes["0"]
    return mg.synth_input((n, h, w, c))


@pytest.mark.parametrize("toy", TOYS, ids=TOY_IDS)
def test_toy_crnn_fp32(gpu, tmp_path, toy):
    cell, batch_first, states = toy
    b = mg.build_toy_crnn(cell=cell, batch_first=batch_first, states=states)
    x = toy_input(b)
    want = rr.eval_graph(b, x)
    eng, got = run_engine(b, tmp_path, x)
    assert len(got) == len(want) == (2 if states else 1)
    for g, r in zip(got, want):
        util.assert_parity(g, r, what="toy crnn " + str(toy))
    rec = [L for L in eng.profile() if L["type"] in ("nn.LSTM", "nn.GRU")]
    assert len(rec) == 1 and rec[0]["kernel"] == rr.kname(cell, F32), rec
    _, cap = run_engine(b, tmp_path, x, forwards=3, graph=1)
    for g, c in zip(got, cap):
        same_bits(c, g, "toy crnn captured")


@pytest.mark.parametrize("toy", TOYS, ids=TOY_IDS)
def test_toy_crnn_fp16_storage(gpu, tmp_path, toy):
    """the engine's error against plain float64 held to 4x the error of the float64 emulation that rounds to fp16 wherever the engine stores
    a half tensor (the margin: one rounding that may land one ulp either way at each of those stores)"""
    cell, batch_first, states = toy
    b = mg.build_toy_crnn(cell=cell, batch_first=batch_first, states=states)
    x = toy_input(b)
    exact, emulated = rr.eval_graph(b, x), rr.eval_graph(b, x, rnd=rr.round_f16)
    eng, got = run_engine(b, tmp_path, x, fp16=1)
    for g, ex, em in zip(got, exact, emulated):
        scale = np.abs(ex).max()
        err, emu = np.abs(g - ex).max() / scale, np.abs(em - ex).max() / scale
        record("toy crnn %s fp16 storage: engine %.3e, emulation %.3e (max|d| / max|ref| against float64)" % (toy, err, emu))
        assert np.isfinite(g).all() and err <= 4.0 * emu, (err, emu)
    rec = [L for L in eng.profile() if L["type"] in ("nn.LSTM", "nn.GRU")]
    assert len(rec) == 1 and rec[0]["kernel"] == rr.kname(cell, F16), rec
    _, cap = run_engine(b, tmp_path, x, forwards=3, graph=1, fp16=1)
    for g, c in zip(got, cap):
        same_bits(c, g, "toy crnn fp16 captured")


@pytest.mark.parametrize("fp16", [0, 1])
@pytest.mark.parametrize("batch_first", [False, True], ids=["seq_first", "batch_first"])
@pytest.mark.parametrize("cell", CELLS)
def test_toy_crnn_rebatched(gpu, tmp_path, cell, batch_first, fp16):
    """SetOption("batch", 5) on the file traced at batch 2 gives the bits of the file built at batch 5: the batch is followed through
    flatten(2) -> permute into dimension 1 (or 0) of the tokens, through the recurrent operator and the Linear"""
    b2, b5 = (mg.build_toy_crnn(batch=n, cell=cell, batch_first=batch_first) for n in (2, 5))
    x = toy_input(b5)
    _, want = run_engine(b5, tmp_path, x, tag="b5", fp16=fp16)
    eng, got = run_engine(b2, tmp_path, x, tag="b2", batch=5, fp16=fp16)
    same_bits(got[0], want[0], "toy crnn batch=5")
    y = [_parse(ln) for ln in b2.lines if ln.startswith(("nn.LSTM", "nn.GRU"))][0][3][0]
    assert eng.operand_shape(y) == ((5, 10, 64) if batch_first else (10, 5, 64))


@pytest.mark.parametrize("cell", CELLS)
def test_toy_crnn_batch_split(gpu, tmp_path, cell):
    """the y-only, batch_first toy (its output carries the batch in dimension 0) re-batched to 8 and cut by host_slices and by streams: the
    bits of the unsplit run -- a batch item's bits do not depend on the batch or on its place in a tile"""
    b = mg.build_toy_crnn(batch=2, cell=cell, batch_first=True)
    x = mg.synth_input((8, 16, 40, 3))
    eng, base = run_engine(b, tmp_path, x, batch=8, host_slices=1, streams=1)
    sched = eng.schedule()
    assert sched["batch_mixing"] == [] and sched["host_slices"] == 1 and sched["lanes"] == 1, sched
    for opts, slices, lanes in ((dict(host_slices=2), 2, 1), (dict(host_slices=4), 4, 1), (dict(streams=2), 1, 2)):
        eng, got = run_engine(b, tmp_path, x, batch=8, **opts)
        sched = eng.schedule()
        assert sched["batch_mixing"] == [] and sched["host_slices"] == slices and sched["lanes"] == lanes, (opts, sched)
        same_bits(got[0], base[0], "toy crnn split %r" % (opts,))
    # the seq-first toy's output carries the batch in dimension 1: a slab of images is no slab of that buffer, and the graph is served unsplit
    eng, _ = run_engine(mg.build_toy_crnn(batch=2, cell=cell), tmp_path, x, tag="seq", batch=8, host_slices=2)
    sched = eng.schedule()
    assert sched["host_slices"] == 1 and len(sched["batch_mixing"]) == 1 and "pnnx_output" in sched["batch_mixing"][0], sched


def test_states_rebatch_follows_dimension_one(gpu, tmp_path):
    """the 3-output form re-batched: the state outputs [layers * dirs, N, H] have dimension 1 rewritten, also where layers * dirs equals the
    traced batch"""
    b2, b3 = (mg.build_toy_crnn(batch=n, layers=1, states=True) for n in (2, 3))
    x = toy_input(b3)
    _, want = run_engine(b3, tmp_path, x, tag="b3")
    eng, got = run_engine(b2, tmp_path, x, tag="b2", batch=3)
    rec = [_parse(ln) for ln in b2.lines if ln.startswith("nn.LSTM")][0]
    assert b2.shapes[rec[3][1]] == (2, 2, 32) and eng.operand_shape(rec[3][1]) == (2, 3, 32)
    for g, w in zip(got, want):
        same_bits(g, w, "states, batch=3")


def test_refused_with_a_status(gpu, tmp_path):
    """kUnsupport with a logged reason at LoadModel; the process goes on"""
    def one(cell="lstm", hidden=16, in_f=8, **kw):
        b = mg.PnnxBuilder(seed=3)
        x = b.input((7, 2, in_f))
        h0 = [b.input((1, 2, hidden)) for _ in range(kw.pop("n_initial", 0))]
        b.output((b.lstm if cell == "lstm" else b.gru)(x, hidden, initial=h0, **kw))
        return b

    assert status_of_load(one(proj_size=1), tmp_path, "proj") == Status.kUnsupport
    assert status_of_load(one(n_initial=2), tmp_path, "h0c0") == Status.kUnsupport
    assert status_of_load(one("gru", n_initial=1), tmp_path, "h0") == Status.kUnsupport
    # fp16 storage with H = 20: between two elementwise layers, so that the operator's operands are halves
    for cell in CELLS:
        b = mg.PnnxBuilder(seed=3)
        y = (b.lstm if cell == "lstm" else b.gru)(b.relu(b.input((7, 2, 8))), 20)
        b.output(b.relu(y))
        assert status_of_load(b, tmp_path, "h20" + cell, fp16=1) == Status.kUnsupport
        assert status_of_load(b, tmp_path, "h20f32" + cell) == Status.kSuccess            # ... and loads without the option
    for drop in ("hidden_size=", "bidirectional=", "@weight_hh_l0=", "@bias_ih_l0="):
        b = one()
        b.lines[-2] = " ".join(tok for tok in b.lines[-2].split() if not tok.startswith(drop))
        assert status_of_load(b, tmp_path, "missing") == Status.kFail, drop
    b = one()
    x = rr.sequence(1, 7, 2, 8)
    name = _parse(b.lines[-2])[1]
    _, got = run_engine(b, tmp_path, x)
    assert np.abs(got[0] - rr.rnn_ref("lstm", x, rr.builder_weights(b, name, "lstm", 1, 1, True))[0]).max() <= 2e-5, "after the refusals"
