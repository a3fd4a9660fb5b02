"""GPU: the temporal convolution kernels (include/si_conv1d.h) and nn.Conv1d.  Kernels: fp32 against float64 at the project's fp32 bar, fp16
storage against the rounding restatement of tests/conv1d_reference.py at the fp16 bar, exact checks on integer-valued data (bit for bit, both
types, a permutation matrix as the K = 1 weight), every fused activation, the bit-for-bit invariants (a batch item alone, a subset of the
filters, two runs), the NaN rule, views under guard bands.  Layer and engine: a one-operator graph with a rank-3 graph input, both toys in
fp32 and under fp16 storage, captured, re-batched and batch-split, the fused activations, the fp32 fallback of a layer that breaks the fp16
rule, and the refusals at LoadModel.

Shapes are the case list of tests/conv1d_reference.py: the smallest at which each mechanism can fail."""
import numpy as np
import pytest

import conv1d_reference as cr
import containment as ct
import util
from ct_reference import _parse
from simpleinfer_amd import hipops, modelgen as mg
from simpleinfer_amd.engine import Engine, Status, StatusError
from test_gpu_f16 import F16_TOL

pytestmark = pytest.mark.gpu

F32, F16 = np.float32, np.float16
ACTS = ("relu", "silu", "sigmoid", "hardsigmoid", "hardswish", "leakyrelu")


def record(line):
    print("conv1d: " + line)


def same_bits(got, want, what):
    ct.assert_same_bits(np.ascontiguousarray(got), np.ascontiguousarray(want), what)


def run(case, x, w, b, **kw):
    n, c, l, oc, k, s, p, d, g = case
    return hipops.conv1d(x, w, b, s, p, d, g, **kw)


def ref(case, x, w, b, **kw):
    n, c, l, oc, k, s, p, d, g = case
    return cr.conv1d_ref(x, w, b, s, p, d, g, **kw)


# ---- accuracy -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cr.CASES, ids=[cr.case_id(c) for c in cr.CASES])
def test_fp32_against_float64(gpu, case):
    x, w, b = cr.operands(case)
    got = run(case, x, w, b)
    assert hipops.LAST_KERNEL_NAME["si_hip_conv1d"] == cr.kname(case, F32)
    want = ref(case, x, w, b)
    assert got.shape == want.shape and got.dtype == F32
    record("fp32 %s: max|d| / max|ref| = %.3e" % (cr.case_id(case), util.rel_err(got, want)))
    util.assert_parity(got, want, util.REL_TOL, what="conv1d fp32 " + cr.case_id(case))
    # without a bias
    util.assert_parity(run(case, x, w, None), ref(case, x, w, None), util.REL_TOL, what="conv1d fp32, no bias, " + cr.case_id(case))


@pytest.mark.parametrize("case", cr.F16_CASES, ids=[cr.case_id(c) for c in cr.F16_CASES])
def test_fp16_against_the_rounding_restatement(gpu, case):
    x, w, b = cr.operands(case, dtype=F16)
    got = run(case, x, w, b)
    assert got.dtype == F16 and hipops.LAST_KERNEL_NAME["si_hip_conv1d"] == cr.kname(case, F16)
    want = ref(case, x, w, b, rnd=cr.round_f16)
    record("fp16 %s: max|d| / max|ref| = %.3e" % (cr.case_id(case), util.rel_err(got.astype(F32), want)))
    util.assert_parity(got.astype(F32), want, F16_TOL, what="conv1d fp16 " + cr.case_id(case))


# ---- exact checks -----------------------------------------------------------------------------------------------------------------
def integer_operands(case, seed):
    """operands that are small integers with every partial sum below 2^11 in magnitude: exact in fp32 and in fp16, whatever the order"""
    n, c, l, oc, k, s, p, d, g = case
    r = np.random.Generator(np.random.Philox(seed))
    terms = (c // g) * k
    hi = 3 if terms * 9 + 8 < 2048 else 1
    x = r.integers(-hi, hi + 1, (n, c, l)).astype(F32)
    w = r.integers(-hi, hi + 1, (oc, c // g, k)).astype(F32)
    b = r.integers(-8, 9, oc).astype(F32)
    assert terms * hi * hi + 8 < 2048
    return x, w, b


EXACT_CASES = [cr.DENSE_CASES[1], cr.DENSE_CASES[2], cr.DENSE_CASES[7], cr.DENSE_CASES[10], cr.DENSE_CASES[11]] + cr.DEPTHWISE_CASES


@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("case", EXACT_CASES, ids=[cr.case_id(c) for c in EXACT_CASES])
def test_integer_data_is_exact(gpu, case, dtype):
    if dtype == F16 and not cr.is_depthwise(case) and (case[1] // case[8]) % 8 != 0:
        case = (case[0], 8 * case[8]) + case[2:]     # the same mechanism at C / g = 8
    x, w, b = integer_operands(case, 5)
    got = run(case, x.astype(dtype), w, b)
    want = ref(case, x, w, b)
    assert np.abs(want).max() < 2048
    same_bits(got, want.astype(dtype), "integer data, " + cr.case_id(case))


@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
def test_permutation_matrix_as_the_weight(gpu, dtype):
    """K = 1 with an asymmetric permutation matrix: y[n, o, l] = x[n, perm[o], l] bit for bit -- a swapped row / column or a wrong lane map
    cannot pass.  24 channels: one and a half tiles on both sides; 70 positions: a tile and a ragged one"""
    c, l = 24, 70
    r = np.random.Generator(np.random.Philox(3))
    perm = r.permutation(c)
    assert not np.array_equal(np.argsort(perm), perm), "the permutation must not be its own inverse"
    w = np.zeros((c, c, 1), F32)
    w[np.arange(c), perm, 0] = 1.0
    x = r.uniform(-1, 1, (2, c, l)).astype(F32).astype(dtype)
    got = hipops.conv1d(x, w)
    assert hipops.LAST_KERNEL_NAME["si_hip_conv1d"] == "conv1d_dense_kernel<%s>" % ("float" if dtype == F32 else "_Float16")
    same_bits(got, x[:, perm, :], "permutation weight")


# ---- activations ------------------------------------------------------------------------------------------------------------------
ACT_CASES = [cr.DENSE_CASES[2], cr.DEPTHWISE_CASES[0]]


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("case", ACT_CASES, ids=[cr.case_id(c) for c in ACT_CASES])
def test_every_fused_activation(gpu, case, act):
    x, w, b = cr.operands(case, seed=2)
    x = x * 4.0     # (both sides of every clamp)
    got = run(case, x, w, b, act=act, act_param=0.1)
    want = ref(case, x, w, b, act=act, act_param=0.1)
    util.assert_parity(got, want, util.REL_TOL, what="conv1d %s %s" % (act, cr.case_id(case)))
    got16 = run(case, x.astype(F16), w, b, act=act, act_param=0.1)
    want16 = ref(case, x.astype(F16), w, b, act=act, act_param=0.1, rnd=cr.round_f16)
    util.assert_parity(got16.astype(F32), want16, F16_TOL, what="conv1d fp16 %s %s" % (act, cr.case_id(case)))


# ---- bit-for-bit invariants -------------------------------------------------------------------------------------------------------
INVARIANT_CASES = [(3, 8, 33, 24, 5, 2, 2, 1, 1), (3, 64, 70, 40, 3, 1, 1, 1, 1), (3, 16, 21, 24, 3, 1, 0, 2, 2), (3, 8, 40, 8, 33, 1, 16, 1, 8)]


@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("case", INVARIANT_CASES, ids=[cr.case_id(c) for c in INVARIANT_CASES])
def test_invariants_bit_for_bit(gpu, case, dtype):
    n, c, l, oc, k, s, p, d, g = case
    x, w, b = cr.operands(case, seed=7, dtype=dtype)
    y = run(case, x, w, b, act="silu")
    same_bits(run(case, x, w, b, act="silu"), y, "two runs")
    for i in range(n):
        same_bits(run((1,) + case[1:], x[i:i + 1], w, b, act="silu"), y[i:i + 1], "batch item %d alone" % i)
    if not cr.is_depthwise(case):
        # a subset of the filters: whole groups dropped from the end would change the input too, so the subset keeps every group and
        # takes the first `keep` filters of each
        ocg = oc // g
        for keep in (1, ocg - 3, ocg // 2):
            rows = np.concatenate([np.arange(gi * ocg, gi * ocg + keep) for gi in range(g)])
            sub = hipops.conv1d(x, w[rows], b[rows], s, p, d, g, act="silu")
            same_bits(sub, y[:, rows], "the first %d filters of each group" % keep)
        # ... and filters picked from the middle, which land in other lanes and other tiles
        if g == 1:
            rows = np.arange(5, oc, 3)
            same_bits(hipops.conv1d(x, w[rows], b[rows], s, p, d, g, act="silu"), y[:, rows], "every third filter")
    else:
        rows = np.arange(2, 7)
        sub = hipops.conv1d(x[:, rows], w[rows], b[rows], s, p, d, len(rows), act="silu")
        same_bits(sub, y[:, rows], "five channels of the depthwise filter bank")


# ---- NaN rule ---------------------------------------------------------------------------------------------------------------------
NAN_CASES = [(3, 8, 33, 24, 5, 2, 2, 1, 1), (2, 16, 40, 12, 3, 1, "same", 4, 2), (2, 8, 40, 8, 33, 1, 16, 1, 8)]


@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("case", NAN_CASES, ids=[cr.case_id(c) for c in NAN_CASES])
def test_nan_rule(gpu, case, dtype):
    """one NaN in x[n, c, l] makes NaN exactly the outputs of its item and group whose window covers l, as in the float64 reference; every
    other element keeps the bits of the clean run"""
    n, c, l, oc, k, s, p, d, g = case
    x, w, b = cr.operands(case, seed=11, dtype=dtype)
    clean = run(case, x, w, b)
    for ni, ci, li in ((0, 0, 0), (n - 1, c - 1, l - 1), (1, c // 2, l // 2)):
        xn = x.copy()
        xn[ni, ci, li] = np.nan
        got = run(case, xn, w, b)
        want = np.isnan(ref(case, xn.astype(np.float64), w, b))
        assert want.any() and not want.all()
        assert np.array_equal(np.isnan(got), want), "NaN at (%d, %d, %d): the NaN mask is not the reference's" % (ni, ci, li)
        same_bits(np.where(want, 0, got).astype(dtype), np.where(want, 0, clean).astype(dtype), "NaN at (%d, %d, %d): the other elements" % (ni, ci, li))


@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("case", [cr.DENSE_CASES[6], cr.DENSE_CASES[3], cr.DEPTHWISE_CASES[2]], ids=cr.case_id)
def test_the_padding_region_is_never_read(gpu, case, dtype):
    """x is an L-crop of a wider tensor whose other positions hold NaN: where the zero padding lies, memory holds NaN, and the result is the
    dense run's, bit for bit"""
    if dtype == F16 and not cr.is_depthwise(case) and (case[1] // case[8]) % 8 != 0:
        case = (case[0], 8 * case[8]) + case[2:]     # the same mechanism at C / g = 8
    x, w, b = cr.operands(case, seed=13, dtype=dtype)
    dense = run(case, x, w, b)
    pad = 96
    got = run(case, x, w, b, in_ld=case[2] + 2 * pad, in_l_off=pad, in_fill=hipops.ByteFill(0xFF))
    assert np.isfinite(got).all()
    same_bits(got, dense, "NaN around the crop")


# ---- views and containment ----------------------------------------------------------------------------------------------------
class ViewCase:
    def __init__(self, vid, case, half, **views):
        self.id, self.case, self.half, self.views = vid, case, half, views
        sfx = "f16" if half else "f32"
        self.entries = ("si_hip_conv1d_" + sfx, "si_hip_conv1d_pack_weights_" + sfx, "si_hip_conv1d_weight_bytes")
        self.dtype = F16 if half else F32

    def operands(self):
        return cr.operands(self.case, seed=17, dtype=self.dtype)

    def run(self, fill, **more):
        x, w, b = self.operands()
        return run(self.case, x, w, b, act="relu", in_fill=fill, out_fill=fill, full=True, **dict(self.views, **more))


VIEW_CASES = []
for _half, _sfx in ((False, "f32"), (True, "f16")):
    VIEW_CASES += [
        # x and y as channel slices and L-crops of wider tensors: dense, grouped dense, depthwise; aligned windows
        ViewCase("dense_" + _sfx, (2, 8, 33, 24, 5, 2, 2, 1, 1), _half, in_c_total=12, in_c_off=4, in_ld=48, in_l_off=8, out_c_total=32, out_c_off=8,
                 out_ld=32, out_l_off=8),
        ViewCase("grouped_" + _sfx, (2, 16, 21, 18, 3, 3, 0, 2, 2), _half, in_c_total=16, in_c_off=0, in_ld=24, in_l_off=3, out_c_total=20, out_c_off=1,
                 out_ld=9, out_l_off=1),
        ViewCase("depthwise_" + _sfx, (2, 8, 40, 8, 33, 1, 16, 1, 8), _half, in_c_total=9, in_c_off=1, in_ld=41, in_l_off=1, out_c_total=10, out_c_off=2,
                 out_ld=47, out_l_off=5),
    ]
VIEW_CASES += [
    # fp32 alone: nothing divides, odd offsets everywhere
    ViewCase("dense_odd_f32", (1, 3, 17, 5, 3, 1, 1, 1, 1), False, in_c_total=5, in_c_off=1, in_ld=23, in_l_off=5, out_c_total=7, out_c_off=1, out_ld=19,
             out_l_off=1),
    # fp16 alone: rows that are not 16-byte aligned
    ViewCase("dense_unaligned_f16", (1, 8, 17, 5, 3, 1, 1, 1, 1), True, in_c_total=9, in_c_off=1, in_ld=19, in_l_off=1, out_c_total=6, out_c_off=1,
             out_ld=21, out_l_off=3),
]


def outside_window(full, case, views, byte, what):
    """every byte of the wide destination outside the window [:, c_off : c_off + OC, l_off : l_off + Lo] equals the fill"""
    n, c, l, oc, k, s, p, d, g = case
    lo = cr.out_len(l, k, s, p, d)
    bad = (ct._bits(full) != np.uint8(byte)).any(axis=-1)
    bad[:, views["out_c_off"]:views["out_c_off"] + oc, views["out_l_off"]:views["out_l_off"] + lo] = False
    assert not bad.any(), "%s: %d elements outside the window differ from the fill 0x%02X, first at %s" % (
        what, int(bad.sum()), byte, tuple(int(i[0]) for i in np.nonzero(bad)))
    return np.ascontiguousarray(full[:, views["out_c_off"]:views["out_c_off"] + oc, views["out_l_off"]:views["out_l_off"] + lo])


@pytest.mark.parametrize("case", VIEW_CASES, ids=[c.id for c in VIEW_CASES])
def test_views_and_containment(gpu, case):
    del hipops.LAST_ENTRIES[:]
    x, w, b = case.operands()
    dense = run(case.case, x, w, b, act="relu")
    name = hipops.LAST_KERNEL_NAME["si_hip_conv1d"]
    assert name == cr.kname(case.case, case.dtype)
    plain = case.run(hipops.ByteFill(0x00))
    assert set(case.entries) <= set(hipops.LAST_ENTRIES), hipops.LAST_ENTRIES
    assert hipops.LAST_KERNEL_NAME["si_hip_conv1d"] == name
    same_bits(outside_window(plain, case.case, case.views, 0x00, case.id + ", plain run"), dense, case.id + " against the dense run")
    for byte in ct.PATTERNS:
        with hipops.guard_bands(byte) as g:      # all bands and the inputs (image, x, bias) are compared when the block ends
            out = case.run(hipops.ByteFill(byte))
        what = "%s under 0x%02X" % (case.id, byte)
        assert g.checked == 4, "%s: the guard saw %d buffers" % (what, g.checked)
        same_bits(outside_window(out, case.case, case.views, byte, what), dense, what)


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


def frames(shape, seed=1):
    r = np.random.Generator(np.random.Philox(seed))
    return r.uniform(-1, 1, shape).astype(F32)


ONE_OP = [(2, 8, 33, 24, 5, 2, 2, 1, 1), (1, 16, 40, 32, 3, 1, "same", 4, 1), (1, 8, 20, 8, 4, 1, "same", 1, 1), (2, 12, 21, 18, 3, 3, 0, 2, 3),
          (2, 8, 40, 8, 33, 1, 16, 1, 8), (2, 6, 30, 4, 3, 1, "valid", 1, 1)]


@pytest.mark.parametrize("case", ONE_OP, ids=[cr.case_id(c) for c in ONE_OP])
def test_layer_in_a_one_operator_graph(gpu, tmp_path, case):
    """a rank-3 graph input: the layer against float64, bit for bit against the op-level call, and a captured replay"""
    n, c, l, oc, k, s, p, d, g = case
    b = mg.PnnxBuilder(seed=3)
    b.output(b.conv1d(b.input((n, c, l)), oc, k, s, p, d, groups=g))
    name = [_parse(ln)[1] for ln in b.lines if ln.startswith("nn.Conv1d")][0]
    w, bias = b.attrs[name + ".weight"], b.attrs[name + ".bias"]
    x = frames((n, c, l))
    eng, (got,) = run_engine(b, tmp_path, x)
    util.assert_parity(got, cr.conv1d_ref(x, w, bias, s, p, d, g), util.REL_TOL, what="layer " + cr.case_id(case))
    same_bits(got, hipops.conv1d(x, w, bias, s, p, d, g), "layer against the op-level call")
    (layer,) = [L for L in eng.profile() if L["type"] == "nn.Conv1d"]
    assert layer["kernel"] == cr.kname(case, F32)
    assert layer["flops"] == 2.0 * got.size * (c // g) * k
    _, (cap,) = run_engine(b, tmp_path, x, forwards=3, graph=1)
    same_bits(cap, got, "captured replay")


TOYS = {"quartznet": mg.build_toy_quartznet, "conv_gru": mg.build_toy_conv_gru}


def toy_input(b, batch=None):
    n, c, t = b.shapes["0"]
    return frames((batch or n, c, t), seed=5)


@pytest.mark.parametrize("toy", sorted(TOYS))
def test_toys_fp32(gpu, tmp_path, toy):
    b = TOYS[toy]()
    x = toy_input(b)
    (want,) = cr.eval_graph(b, x)
    eng, (got,) = run_engine(b, tmp_path, x)
    util.assert_parity(got, want, what="toy " + toy)
    kernels = [L["kernel"] for L in eng.profile() if L["type"] == "nn.Conv1d"]
    if toy == "quartznet":
        assert kernels.count("conv1d_depthwise_kernel<float>") == 2 and kernels.count("conv1d_dense_kernel<float>") == 7, kernels
    else:
        assert kernels == ["conv1d_dense_kernel<float>"] * 2, kernels
    _, (cap,) = run_engine(b, tmp_path, x, forwards=3, graph=1)
    same_bits(cap, got, "toy %s captured" % toy)
    # the fused activations: nn.ReLU behind a Conv1d is the conv's epilogue (nn.Hardtanh is a parametrised activation, which no epilogue
    # of the project folds in: it stays a step of its own), and the fused schedule gives the bits of fuse=0
    fused = eng.schedule()["fused"]
    relus = [_parse(ln) for ln in b.lines if ln.startswith("nn.ReLU")]
    behind_conv = [r[1] for r in relus if any(_parse(ln)[3] == r[2] for ln in b.lines if ln.startswith("nn.Conv1d"))]
    assert set(behind_conv) <= set(fused), (behind_conv, fused)
    if toy == "quartznet":
        assert len(behind_conv) == 4
    _, (plain,) = run_engine(b, tmp_path, x, fuse=0)
    same_bits(plain, got, "toy %s, fuse=0" % toy)


@pytest.mark.parametrize("toy", sorted(TOYS))
def test_toys_fp16_storage(gpu, tmp_path, toy):
    """the engine's error against plain float64 held to 4x the error of the float64 emulation that rounds to fp16 wherever the engine stores
    a half tensor (the margin: one rounding that may land one ulp either way at each of those stores)"""
    b = TOYS[toy]()
    x = toy_input(b)
    (exact,), (emulated,) = cr.eval_graph(b, x), cr.eval_graph(b, x, rnd=cr.round_f16)
    eng, (got,) = run_engine(b, tmp_path, x, fp16=1)
    scale = np.abs(exact).max()
    err, emu = np.abs(got - exact).max() / scale, np.abs(emulated - exact).max() / scale
    record("toy %s fp16 storage: engine %.3e, emulation %.3e (max|d| / max|ref| against float64)" % (toy, err, emu))
    assert np.isfinite(got).all() and err <= 4.0 * emu, (err, emu)
    # the graph input stays fp32 under fp16 storage: the conv that reads it runs its fp32 kernel between casts, every other one the fp16 kernel
    kernels = [L["kernel"] for L in eng.profile() if L["type"] == "nn.Conv1d"]
    assert kernels[0].endswith("<float>") and all(k.endswith("<_Float16>") for k in kernels[1:]), kernels
    _, (cap,) = run_engine(b, tmp_path, x, forwards=3, graph=1, fp16=1)
    same_bits(cap, got, "toy %s fp16 captured" % toy)


@pytest.mark.parametrize("fp16", [0, 1])
@pytest.mark.parametrize("toy", sorted(TOYS))
def test_toys_rebatched(gpu, tmp_path, toy, fp16):
    """SetOption("batch", 5) on the file traced at batch 2 gives the bits of the file built at batch 5"""
    b2, b5 = (TOYS[toy](batch=n) for n in (2, 5))
    x = toy_input(b5)
    _, want = run_engine(b5, tmp_path, x, tag="b5", fp16=fp16)
    eng, got = run_engine(b2, tmp_path, x, tag="b2", batch=5, fp16=fp16)
    same_bits(got[0], want[0], "toy %s batch=5" % toy)
    first = [_parse(ln) for ln in b2.lines if ln.startswith("nn.Conv1d")][0][3][0]
    assert eng.operand_shape(first)[0] == 5


def test_quartznet_batch_split(gpu, tmp_path):
    """the quartznet toy (every operand carries the batch in dimension 0) re-batched to 8 and cut by host_slices and by streams: the bits of
    the unsplit run.  The conv_gru toy's output carries the batch in dimension 1: it is served unsplit"""
    b = mg.build_toy_quartznet(batch=2)
    x = toy_input(b, batch=8)
    eng, base = run_engine(b, tmp_path, x, batch=8, host_slices=1, streams=1)
    sched = eng.schedule()
    assert sched["batch_mixing"] == [] and sched["host_slices"] == 1 and sched["lanes"] == 1, sched
    for opts, slices, lanes in ((dict(host_slices=2), 2, 1), (dict(host_slices=4), 4, 1), (dict(streams=2), 1, 2)):
        eng, got = run_engine(b, tmp_path, x, batch=8, **opts)
        sched = eng.schedule()
        assert sched["batch_mixing"] == [] and sched["host_slices"] == slices and sched["lanes"] == lanes, (opts, sched)
        same_bits(got[0], base[0], "toy quartznet split %r" % (opts,))
    g = mg.build_toy_conv_gru(batch=2)
    eng, _ = run_engine(g, tmp_path, toy_input(g, batch=8), tag="gru", batch=8, host_slices=2)
    sched = eng.schedule()
    assert sched["host_slices"] == 1 and len(sched["batch_mixing"]) == 1 and "pnnx_output" in sched["batch_mixing"][0], sched


def test_fp16_engine_takes_the_fp32_fallback_for_a_layer_that_breaks_the_rule(gpu, tmp_path):
    """C / groups = 12 between two elementwise layers, so that the operator's operands are halves: the layer runs its fp32 kernel between
    casts, and the result is the fp32 engine's within the fp16 bar"""
    b = mg.PnnxBuilder(seed=3)
    b.output(b.relu(b.conv1d(b.relu(b.input((2, 12, 40))), 16, 3, 1, 1)))
    x = frames((2, 12, 40), seed=9)
    (want,) = cr.eval_graph(b, x)
    eng, (got,) = run_engine(b, tmp_path, x, fp16=1)
    (layer,) = [L for L in eng.profile() if L["type"] == "nn.Conv1d"]
    assert layer["kernel"] == "conv1d_dense_kernel<float>", layer
    util.assert_parity(got, want, F16_TOL, what="fp32 fallback under fp16 storage")
    # the same graph at C = 16 runs the fp16 kernel
    b = mg.PnnxBuilder(seed=3)
    b.output(b.relu(b.conv1d(b.relu(b.input((2, 16, 40))), 16, 3, 1, 1)))
    eng, _ = run_engine(b, tmp_path, frames((2, 16, 40)), tag="c16", fp16=1)
    (layer,) = [L for L in eng.profile() if L["type"] == "nn.Conv1d"]
    assert layer["kernel"] == "conv1d_dense_kernel<_Float16>", layer
    # ... and a dilation whose span (63 + 2 * 500 + 1 positions) the fp16 image cannot hold while the fp32 image can: fp32 between casts
    b = mg.PnnxBuilder(seed=3)
    b.output(b.relu(b.conv1d(b.relu(b.input((1, 16, 1100))), 16, 3, 1, "same", d=500)))
    x = frames((1, 16, 1100), seed=10)
    eng, (got,) = run_engine(b, tmp_path, x, tag="d500", fp16=1)
    (layer,) = [L for L in eng.profile() if L["type"] == "nn.Conv1d"]
    assert layer["kernel"] == "conv1d_dense_kernel<float>", layer
    util.assert_parity(got, cr.eval_graph(b, x)[0], F16_TOL, what="a span beyond the fp16 image under fp16 storage")


def test_refused_with_a_status(gpu, tmp_path):
    """each refusal at LoadModel with its status; the process goes on"""
    def one(shape=(2, 8, 30), **kw):
        b = mg.PnnxBuilder(seed=3)
        b.output(b.conv1d(b.input(shape), 8, 3, **kw))
        return b

    assert status_of_load(one(padding_mode="reflect"), tmp_path, "reflect") == Status.kUnsupport
    assert status_of_load(one(padding_mode="circular"), tmp_path, "circular") == Status.kUnsupport
    bad = one(p="same")
    bad.lines[-2] = bad.lines[-2].replace("stride=(1)", "stride=(2)")
    assert status_of_load(bad, tmp_path, "same_s2") == Status.kUnsupport
    assert status_of_load(one(shape=(8, 30)), tmp_path, "rank2") == Status.kUnsupport
    wrong = one()
    out = _parse(wrong.lines[-2])[3][0]
    wrong.lines[-2] = wrong.lines[-2].replace("#%s=(2,8,30)f32" % out, "#%s=(2,8,29)f32" % out)
    wrong.lines[-1] = wrong.lines[-1].replace("#%s=(2,8,30)f32" % out, "#%s=(2,8,29)f32" % out)
    assert status_of_load(wrong, tmp_path, "shape") == Status.kErrorShape
    for drop in ("kernel_size=", "padding_mode=", "@weight="):
        b = one()
        b.lines[-2] = " ".join(tok for tok in b.lines[-2].split() if not tok.startswith(drop))
        assert status_of_load(b, tmp_path, "missing") == Status.kFail, drop
    b = one()
    x = frames((2, 8, 30))
    _, (got,) = run_engine(b, tmp_path, x)
    util.assert_parity(got, cr.eval_graph(b, x)[0], what="after the refusals")
