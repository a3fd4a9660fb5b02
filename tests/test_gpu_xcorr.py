"""GPU: the cross-correlation kernels (include/si_xcorr.h) and F.conv2d with a tensor filter.  Kernels: fp32 against float64 at the project's
fp32 bar, fp16 storage against the rounding restatement of tests/xcorr_reference.py at the fp16 bar, the depthwise form in both addressings,
exact checks on integer-valued data and with a one-hot filter (bit for bit, both types), every fused activation, the bit-for-bit invariants
(a batch item alone, a subset of the filters, a filter in another tile position, two runs, per-sample against unfused addressing), the NaN
rule, views under guard bands.  Layer and engine: the five toys in fp32, under fp16 storage and captured, the layer against the op-level
call, the fused and unfused plans of the depthwise sandwich, the lowering of a constant filter to nn.Conv2d, the fp32 fallback of a layer
that breaks the fp16 rule, the batch modes, and the refusals at LoadModel.

Shapes are the case list of tests/xcorr_reference.py: the smallest at which each mechanism can fail."""
import numpy as np
import pytest

import containment as ct
import util
import xcorr_reference as xr
from ct_reference import _parse
from simpleinfer_amd import hipops, modelgen as mg
from simpleinfer_amd.engine import Engine, Status, StatusError
from test_gpu_f16 import F16_TOL

pytestmark = pytest.mark.gpu

F32, F16 = np.float32, np.float16
ACTS = ("relu", "silu", "sigmoid", "hardsigmoid", "hardswish", "leakyrelu")
KEY = "si_hip_xcorr"


def record(line):
    print("xcorr: " + line)


def same_bits(got, want, what):
    ct.assert_same_bits(np.ascontiguousarray(got), np.ascontiguousarray(want), what)


def run(case, x, w, b, **kw):
    """torch layouts in and out; the kernel sees NHWC and the filter as stored"""
    n, c, h, wd, oc, kh, kw_, s, p, d, g = case
    return xr.nchw(hipops.xcorr(xr.nhwc(x), xr.nhwc(w), b, s, p, d, g, **kw))


def run_per_sample(case, x, z, b, **kw):
    n, c, h, wd, oc, kh, kw_, s, p, d, g = case
    return xr.nchw(hipops.xcorr(xr.nhwc(x), xr.nhwc(z), b, s, p, d, per_sample=True, **kw))


def ref(case, x, w, b, **kw):
    n, c, h, wd, oc, kh, kw_, s, p, d, g = case
    return xr.conv2d_ref(x, w, b, s, p, d, g, **kw)


def ref_per_sample(case, x, z, b, **kw):
    n, c, h, wd, oc, kh, kw_, s, p, d, g = case
    return xr.per_sample_ref(x, z, b, s, p, d, **kw)


# ---- accuracy -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", xr.CASES, ids=[xr.case_id(c) for c in xr.CASES])
def test_fp32_against_float64(gpu, case):
    x, w, b = xr.operands(case)
    got = run(case, x, w, b)
    assert hipops.LAST_KERNEL_NAME[KEY] == xr.kname(case, F32)
    want = ref(case, x, w, b)
    assert got.shape == want.shape and got.dtype == F32
    record("fp32 %s: max|d| / max|ref| = %.3e" % (xr.case_id(case), util.rel_err(got, want)))
    util.assert_parity(got, want, util.REL_TOL, what="xcorr fp32 " + xr.case_id(case))
    util.assert_parity(run(case, x, w, None), ref(case, x, w, None), util.REL_TOL, what="xcorr fp32, no bias, " + xr.case_id(case))


@pytest.mark.parametrize("case", xr.F16_CASES, ids=[xr.case_id(c) for c in xr.F16_CASES])
def test_fp16_against_the_rounding_restatement(gpu, case):
    x, w, b = xr.operands(case, dtype=F16)
    got = run(case, x, w, b)
    assert got.dtype == F16 and hipops.LAST_KERNEL_NAME[KEY] == xr.kname(case, F16)
    want = ref(case, x, w, b, rnd=xr.round_f16)
    record("fp16 %s: max|d| / max|ref| = %.3e" % (xr.case_id(case), util.rel_err(got.astype(F32), want)))
    util.assert_parity(got.astype(F32), want, F16_TOL, what="xcorr fp16 " + xr.case_id(case))


@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("case", xr.DEPTHWISE_CASES, ids=[xr.case_id(c) for c in xr.DEPTHWISE_CASES])
def test_depthwise_per_sample_addressing(gpu, case, dtype):
    """filter n meets image n: against float64 (fp16: the rounding restatement), with and without the bias"""
    x, _, b = xr.operands(case, dtype=dtype)
    z = xr.templates(case, dtype=dtype)
    rnd, tol = (xr.round_f16, F16_TOL) if dtype == F16 else (None, util.REL_TOL)
    for bias in (b, None):
        got = run_per_sample(case, x, z, bias)
        assert got.dtype == dtype and hipops.LAST_KERNEL_NAME[KEY] == xr.kname(case, dtype, depthwise=True)
        want = ref_per_sample(case, x, z, bias, rnd=rnd)
        record("per-sample %s %s: max|d| / max|ref| = %.3e" % (np.dtype(dtype).name, xr.case_id(case), util.rel_err(got.astype(F32), want)))
        util.assert_parity(got.astype(F32), want, tol, what="xcorr per-sample " + xr.case_id(case))


# ---- exact checks -----------------------------------------------------------------------------------------------------------------
def integer_operands(case, seed):
    """operands that are small integers with every partial sum below 2^11 in magnitude: exact in fp32 and in fp16, whatever the order"""
    n, c, h, wd, oc, kh, kw, s, p, d, g = case
    r = np.random.Generator(np.random.Philox(seed))
    terms = (c // g) * kh * kw
    hi = 3 if terms * 9 + 8 < 2048 else 1
    assert terms * hi * hi + 8 < 2048
    x = r.integers(-hi, hi + 1, (n, c, h, wd)).astype(F32)
    w = r.integers(-hi, hi + 1, (oc, c // g, kh, kw)).astype(F32)
    z = r.integers(-hi, hi + 1, (n, c, kh, kw)).astype(F32)
    b = r.integers(-8, 9, oc).astype(F32)
    return x, w, z, b


EXACT_CASES = [xr.DENSE_CASES[i] for i in (1, 2, 3, 4, 6, 7, 8)] + xr.DEPTHWISE_CASES


@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("case", EXACT_CASES, ids=[xr.case_id(c) for c in EXACT_CASES])
def test_integer_data_is_exact(gpu, case, dtype):
    if dtype == F16 and not xr.is_depthwise(case) and case[1] % 8 != 0:
        case = (case[0], 8) + case[2:]     # the same mechanism at C = 8
    x, w, z, b = integer_operands(case, 5)
    got = run(case, x.astype(dtype), w.astype(dtype), b)
    want = ref(case, x, w, b)
    assert np.abs(want).max() < 2048
    same_bits(got, want.astype(dtype), "integer data, " + xr.case_id(case))
    if xr.is_depthwise(case):
        same_bits(run_per_sample(case, x.astype(dtype), z.astype(dtype), b), ref_per_sample(case, x, z, b).astype(dtype),
                  "integer data per-sample, " + xr.case_id(case))


@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
def test_one_hot_filter_is_a_shifted_copy(gpu, dtype):
    """filter o is 1 at (channel perm[o], tap (ky[o], kx[o])) and 0 elsewhere: y[n, o] is channel perm[o] of x shifted by that tap, bit for
    bit -- a swapped row / column, a wrong lane map or a wrong tap order cannot pass.  24 filters over 8 channels: one and a half tiles"""
    c, oc, h, wd, kh, kw = 8, 24, 9, 11, 3, 4
    r = np.random.Generator(np.random.Philox(3))
    perm, ky, kx = r.integers(0, c, oc), r.integers(0, kh, oc), r.integers(0, kw, oc)
    w = np.zeros((oc, c, kh, kw), F32)
    w[np.arange(oc), perm, ky, kx] = 1.0
    x = r.uniform(-1, 1, (2, c, h, wd)).astype(F32).astype(dtype)
    got = run((2, c, h, wd, oc, kh, kw, 1, 0, 1, 1), x, w.astype(dtype), None)
    ho, wo = h - kh + 1, wd - kw + 1
    want = np.stack([x[:, perm[o], ky[o]:ky[o] + ho, kx[o]:kx[o] + wo] for o in range(oc)], axis=1)
    same_bits(got, want, "one-hot filters")
    # depthwise, both addressings: one tap per channel
    wdw = np.zeros((c, 1, kh, kw), F32)
    wdw[np.arange(c), 0, ky[:c], kx[:c]] = 1.0
    want = np.stack([x[:, o, ky[o]:ky[o] + ho, kx[o]:kx[o] + wo] for o in range(c)], axis=1)
    case = (2, c, h, wd, c, kh, kw, 1, 0, 1, c)
    same_bits(run(case, x, wdw.astype(dtype), None), want, "one-hot depthwise filters")
    z = np.broadcast_to(wdw[:, 0][None], (2, c, kh, kw)).astype(dtype)
    same_bits(run_per_sample(case, x, z, None), want, "one-hot per-sample filters")


# ---- activations ------------------------------------------------------------------------------------------------------------------
ACT_CASES = [xr.DENSE_CASES[4], xr.DEPTHWISE_CASES[3]]


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("case", ACT_CASES, ids=[xr.case_id(c) for c in ACT_CASES])
def test_every_fused_activation_and_the_bias(gpu, case, act):
    x, w, b = xr.operands(case, seed=2)
    x = x * 4.0     # (both sides of every clamp)
    got = run(case, x, w, b, act=act, act_param=0.1)
    want = ref(case, x, w, b, act=act, act_param=0.1)
    util.assert_parity(got, want, util.REL_TOL, what="xcorr %s %s" % (act, xr.case_id(case)))
    got16 = run(case, x.astype(F16), w.astype(F16), b, act=act, act_param=0.1)
    want16 = ref(case, x.astype(F16), w.astype(F16), b, act=act, act_param=0.1, rnd=xr.round_f16)
    util.assert_parity(got16.astype(F32), want16, F16_TOL, what="xcorr fp16 %s %s" % (act, xr.case_id(case)))


# ---- bit-for-bit invariants -------------------------------------------------------------------------------------------------------
INVARIANT_CASES = [(3, 8, 7, 9, 70, 3, 3, 1, 1, 1, 1), (3, 16, 9, 11, 40, 1, 5, (2, 1), 0, 1, 1), (3, 8, 8, 8, 5, 4, 2, 1, "same", 1, 1)]


@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("case", INVARIANT_CASES, ids=[xr.case_id(c) for c in INVARIANT_CASES])
def test_dense_invariants_bit_for_bit(gpu, case, dtype):
    n, c, h, wd, oc, kh, kw, s, p, d, g = case
    x, w, b = xr.operands(case, seed=7, dtype=dtype)
    y = run(case, x, w, b, act="silu")
    same_bits(run(case, x, w, b, act="silu"), y, "two runs")
    for i in range(n):
        same_bits(run((1,) + case[1:], x[i:i + 1], w, b, act="silu"), y[i:i + 1], "batch item %d alone" % i)
    for keep in sorted({1, max(oc - 3, 1), oc // 2}):
        sub = run(case[:4] + (keep,) + case[5:], x, w[:keep], b[:keep], act="silu")
        same_bits(sub, y[:, :keep], "the first %d filters" % keep)
    # filters picked from the middle land in other lanes and other tiles; a reversed order moves every filter to another place
    for rows in (np.arange(min(5, oc - 1), oc, 3), np.arange(oc)[::-1]):
        sub = run(case[:4] + (len(rows),) + case[5:], x, w[rows], b[rows], act="silu")
        same_bits(sub, y[:, rows], "filters %s..." % rows[:4])


DW_INVARIANT_CASES = [(2, 12, 9, 9, 12, 3, 3, 1, 1, 2, 12), (2, 64, 31, 31, 64, 7, 7, 1, 0, 1, 64), (2, 7, 9, 9, 7, 4, 2, 1, "same", 1, 7)]


@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("case", DW_INVARIANT_CASES, ids=[xr.case_id(c) for c in DW_INVARIANT_CASES])
def test_depthwise_invariants_bit_for_bit(gpu, case, dtype):
    n, c, h, wd, oc, kh, kw, s, p, d, g = case
    x, w, b = xr.operands(case, seed=7, dtype=dtype)
    z = xr.templates(case, seed=7, dtype=dtype)
    y = run_per_sample(case, x, z, b, act="silu")
    same_bits(run_per_sample(case, x, z, b, act="silu"), y, "two runs")
    for i in range(n):
        one = (1,) + case[1:]
        same_bits(run_per_sample(one, x[i:i + 1], z[i:i + 1], b, act="silu"), y[i:i + 1], "batch item %d alone" % i)
        # per-sample addressing against the unfused addressing on the same data: x as [1, C, H, W] with filter n as [C, 1, kh, kw]
        same_bits(run(one, x[i:i + 1], z[i][:, None], b, act="silu"), y[i:i + 1], "image %d: unfused addressing" % i)
    # ... and the whole batch at once as the unfused sandwich sees it: x [1, N C, H, W], w [N C, 1, kh, kw]
    if n * c * kh * kw < 1 << 20:
        folded = (1, n * c, h, wd, n * c, kh, kw, s, p, d, n * c)
        yy = run(folded, x.reshape(1, n * c, h, wd), z.reshape(n * c, 1, kh, kw), np.tile(b, n), act="silu")
        same_bits(yy.reshape(y.shape), y, "the folded batch in the unfused addressing")
    rows = np.arange(1, c, 2)
    sub_case = case[:1] + (len(rows),) + case[2:4] + (len(rows),) + case[5:10] + (len(rows),)
    same_bits(run_per_sample(sub_case, x[:, rows], z[:, rows], b[rows], act="silu"), y[:, rows], "every second channel")


# ---- NaN rule ---------------------------------------------------------------------------------------------------------------------
NAN_CASES = [(3, 8, 7, 9, 20, 3, 3, 1, 1, 1, 1), (2, 8, 8, 8, 5, 4, 2, 1, "same", 1, 1), (2, 12, 9, 9, 12, 3, 3, 1, 1, 2, 12)]


@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("case", NAN_CASES, ids=[xr.case_id(c) for c in NAN_CASES])
def test_nan_rule(gpu, case, dtype):
    """one NaN in x[n, c, iy, ix] makes NaN exactly the outputs of its image (and, depthwise, its channel) whose window covers it, one NaN
    in filter o exactly channel o, as in the float64 reference; every other element keeps the bits of the clean run"""
    n, c, h, wd, oc, kh, kw, s, p, d, g = case
    x, w, b = xr.operands(case, seed=11, dtype=dtype)
    clean = run(case, x, w, b)

    def check(xn, wn, what):
        got = run(case, xn, wn, b)
        want = np.isnan(ref(case, xn.astype(np.float64), wn.astype(np.float64), b))
        assert want.any() and not want.all()
        assert np.array_equal(np.isnan(got), want), "%s: the NaN mask is not the reference's" % what
        same_bits(np.where(want, 0, got).astype(dtype), np.where(want, 0, clean).astype(dtype), "%s: the other elements" % what)

    for ni, ci, yi, xi in ((0, 0, 0, 0), (n - 1, c - 1, h - 1, wd - 1), (1, c // 2, h // 2, wd // 2)):
        xn = x.copy()
        xn[ni, ci, yi, xi] = np.nan
        check(xn, w, "NaN in x at (%d, %d, %d, %d)" % (ni, ci, yi, xi))
    for o in (0, oc - 1, oc // 2):
        wn = w.copy()
        wn[o, 0, kh // 2, kw // 2] = np.nan
        check(x, wn, "NaN in filter %d" % o)


@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("case", [xr.DENSE_CASES[7], xr.DENSE_CASES[8], xr.DEPTHWISE_CASES[5], xr.DEPTHWISE_CASES[3]], ids=xr.case_id)
def test_the_padding_region_is_never_read(gpu, case, dtype):
    """x is a column crop of a wider tensor whose other positions hold NaN: beside the image, where the zero padding lies, memory holds NaN,
    and the result is the dense run's, bit for bit"""
    if dtype == F16 and not xr.is_depthwise(case) and case[1] % 8 != 0:
        case = (case[0], 8) + case[2:]
    x, w, b = xr.operands(case, seed=13, dtype=dtype)
    dense = run(case, x, w, b)
    got = run(case, x, w, b, in_w_total=case[3] + 16, in_w_off=8, in_fill=hipops.ByteFill(0xFF))
    assert np.isfinite(got).all()
    same_bits(got, dense, "NaN around the crop")


# ---- views and containment ----------------------------------------------------------------------------------------------------
class ViewCase:
    def __init__(self, vid, case, half, per_sample=False, **views):
        self.id, self.case, self.half, self.per_sample, self.views = vid, case, half, per_sample, views
        self.entries = ("si_hip_xcorr_f16" if half else "si_hip_xcorr_f32",)
        self.dtype = F16 if half else F32

    def operands(self):
        x, w, b = xr.operands(self.case, seed=17, dtype=self.dtype)
        return x, (xr.templates(self.case, seed=17, dtype=self.dtype) if self.per_sample else w), b

    def run(self, fill=None, **more):
        x, w, b = self.operands()
        n, c, h, wd, oc, kh, kw, s, p, d, g = self.case
        kw_ = dict(act="relu")
        if fill is not None:
            kw_.update(in_fill=fill, w_fill=fill, out_fill=fill, full=True, **dict(self.views, **more))
        if self.per_sample:
            return hipops.xcorr(xr.nhwc(x), xr.nhwc(w), b, s, p, d, per_sample=True, **kw_)
        return hipops.xcorr(xr.nhwc(x), xr.nhwc(w), b, s, p, d, g, **kw_)


DENSE_V, DW_V = (2, 8, 7, 9, 20, 3, 3, 1, 1, 1, 1), (2, 8, 9, 9, 8, 3, 3, 1, 1, 1, 8)
VIEW_CASES = []
for _half, _sfx in ((False, "f32"), (True, "f16")):
    VIEW_CASES += [
        # x, w and y as channel slices of wider tensors with gapped rows; aligned windows: the 16-byte paths
        ViewCase("dense_" + _sfx, DENSE_V, _half, in_c_total=24, in_c_off=8, in_w_total=12, in_w_off=2, w_c_total=16, w_c_off=8, w_w_total=5,
                 w_w_off=1, out_c_total=32, out_c_off=8, out_w_total=11, out_w_off=1),
        # misaligned starts: the element paths
        ViewCase("dense_odd_" + _sfx, DENSE_V, _half, in_c_total=11, in_c_off=3, in_w_total=10, in_w_off=1, w_c_total=9, w_c_off=1, w_w_total=4,
                 w_w_off=1, out_c_total=23, out_c_off=1, out_w_total=10, out_w_off=1),
        ViewCase("depthwise_" + _sfx, DW_V, _half, in_c_total=24, in_c_off=8, in_w_total=12, in_w_off=2, w_c_total=1, w_c_off=0, w_w_total=5,
                 w_w_off=1, out_c_total=16, out_c_off=8, out_w_total=11, out_w_off=1),
        ViewCase("depthwise_odd_" + _sfx, DW_V, _half, in_c_total=11, in_c_off=3, in_w_total=10, in_w_off=1, w_c_total=3, w_c_off=1, w_w_total=4,
                 w_w_off=1, out_c_total=13, out_c_off=1, out_w_total=10, out_w_off=1),
        ViewCase("per_sample_" + _sfx, DW_V, _half, True, in_c_total=24, in_c_off=8, in_w_total=12, in_w_off=2, w_c_total=16, w_c_off=8,
                 w_w_total=5, w_w_off=1, out_c_total=16, out_c_off=8, out_w_total=11, out_w_off=1),
        ViewCase("per_sample_odd_" + _sfx, DW_V, _half, True, in_c_total=11, in_c_off=3, in_w_total=10, in_w_off=1, w_c_total=9, w_c_off=1,
                 w_w_total=4, w_w_off=1, out_c_total=13, out_c_off=1, out_w_total=10, out_w_off=1),
    ]


def outside_window(full, case, views, byte, what):
    """every byte of the wide NHWC destination outside the window [:, :, w_off : w_off + Wo, c_off : c_off + OC] equals the fill"""
    n, c, h, wd, oc, kh, kw, s, p, d, g = case
    ho, wo = xr.out_hw(h, wd, kh, kw, s, p, d)
    bad = (ct._bits(full) != np.uint8(byte)).any(axis=-1)
    co, wo_ = views["out_c_off"], views["out_w_off"]
    bad[:, :, wo_:wo_ + wo, co:co + oc] = False
    assert not bad.any(), "%s: %d elements outside the window differ from the fill 0x%02X, first at %s" % (
        what, int(bad.sum()), byte, tuple(int(i[0]) for i in np.nonzero(bad)))
    return np.ascontiguousarray(full[:, :, wo_:wo_ + wo, co:co + oc])


@pytest.mark.parametrize("case", VIEW_CASES, ids=[c.id for c in VIEW_CASES])
def test_views_and_containment(gpu, case):
    del hipops.LAST_ENTRIES[:]
    dense = case.run()
    name = hipops.LAST_KERNEL_NAME[KEY]
    assert name == xr.kname(case.case, case.dtype, depthwise=case.per_sample or xr.is_depthwise(case.case))
    plain = case.run(hipops.ByteFill(0x00))
    assert set(case.entries) <= set(hipops.LAST_ENTRIES), hipops.LAST_ENTRIES
    assert hipops.LAST_KERNEL_NAME[KEY] == name
    same_bits(outside_window(plain, case.case, case.views, 0x00, case.id + ", plain run"), dense, case.id + " against the dense run")
    for byte in ct.PATTERNS:
        with hipops.guard_bands(byte) as g:      # all bands and the inputs (x, w, bias) are compared when the block ends
            out = case.run(hipops.ByteFill(byte))
        what = "%s under 0x%02X" % (case.id, byte)
        assert g.checked == 4, "%s: the guard saw %d buffers" % (what, g.checked)
        same_bits(outside_window(out, case.case, case.views, byte, what), dense, what)


# ---- layer and engine ---------------------------------------------------------------------------------------------------------
def save(b, tmp_path, tag):
    pp, bp = str(tmp_path / (tag + ".pnnx.param")), str(tmp_path / (tag + ".pnnx.bin"))
    b.save(pp, bp)
    return pp, bp


def graph_inputs(b):
    return [_parse(ln)[3][0] for ln in b.lines if ln.startswith("pnnx.Input")]


def graph_outputs(b):
    return [_parse(ln)[2][0] for ln in b.lines if ln.startswith("pnnx.Output")]


def toy_inputs(b, seed=5, batch=None):
    """the graph inputs in file order, torch's layout"""
    r = np.random.Generator(np.random.Philox(seed))
    shapes = [b.shapes[i] for i in graph_inputs(b)]
    return [r.uniform(-1, 1, ((batch,) + s[1:]) if batch else s).astype(F32) for s in shapes]


def run_engine(b, tmp_path, xs, tag="m", forwards=1, **opts):
    """(engine, the graph outputs in file order in torch's layout)"""
    pp, bp = save(b, tmp_path, tag)
    e = Engine(**opts)
    e.load_model(pp, bp)
    for name, x in zip(graph_inputs(b), xs):
        e.input(name, xr.nhwc(x))
    for _ in range(forwards):
        e.forward()
    return e, [xr.nchw(e.extract(o)) for o in graph_outputs(b)]


def status_of_load(b, tmp_path, tag, **opts):
    pp, bp = save(b, tmp_path, tag)
    try:
        Engine(**opts).load_model(pp, bp)
    except StatusError as ex:
        return ex.status
    return Status.kSuccess


TOYS = {
    "siamfc": mg.build_toy_siamfc,
    "siamrpn": mg.build_toy_siamrpn,
    "siamrpnpp_n1": lambda **kw: mg.build_toy_siamrpnpp(batch=1, **kw),
    "siamrpnpp_n2": lambda **kw: mg.build_toy_siamrpnpp(batch=2, **kw),
    "dynamic_head": mg.build_toy_dynamic_head,
    "dynamic_head_const": lambda **kw: mg.build_toy_dynamic_head(batch=2, constant=True, **kw),
    "blurpool": mg.build_toy_blurpool,
}
XCORR_KERNEL = {"siamfc": "xcorr_dense_kernel", "siamrpn": "xcorr_dense_kernel", "siamrpnpp_n1": "xcorr_depthwise_kernel",
                "siamrpnpp_n2": "xcorr_depthwise_kernel", "dynamic_head": "xcorr_dense_kernel", "dynamic_head_const": "xcorr_dense_kernel"}


def xcorr_layers(eng):
    return [L for L in eng.profile() if L["type"] == "F.conv2d"]


@pytest.mark.parametrize("toy", sorted(TOYS))
def test_toys_fp32(gpu, tmp_path, toy):
    b = TOYS[toy]()
    xs = toy_inputs(b)
    (want,) = xr.eval_graph(b, xs)
    eng, (got,) = run_engine(b, tmp_path, xs)
    util.assert_parity(got, want, what="toy " + toy)
    layers = xcorr_layers(eng)
    if toy == "blurpool":
        assert layers == [] and len([L for L in eng.profile() if L["type"] == "nn.Conv2d"]) == 3, eng.profile()
    else:
        assert [L["kernel"] for L in layers] == [XCORR_KERNEL[toy] + "<float>"], layers
        assert layers[0]["flops"] > 0
    _, (cap,) = run_engine(b, tmp_path, xs, forwards=3, graph=1)
    same_bits(cap, got, "toy %s captured over three forwards" % toy)
    _, (plain,) = run_engine(b, tmp_path, xs, fuse=0)
    same_bits(plain, got, "toy %s, fuse=0" % toy)


@pytest.mark.parametrize("toy", sorted(TOYS))
def test_toys_fp16_storage(gpu, tmp_path, toy):
    """the engine's error against plain float64 held to 4x the error of the float64 emulation that rounds to fp16 wherever the engine stores
    a half tensor (the margin: one rounding that may land one ulp either way at each of those stores)"""
    b = TOYS[toy]()
    xs = toy_inputs(b)
    (exact,), (emulated,) = xr.eval_graph(b, xs), xr.eval_graph(b, xs, rnd=xr.round_f16)
    eng, (got,) = run_engine(b, tmp_path, xs, fp16=1)
    scale = np.abs(exact).max()
    err, emu = np.abs(got - exact).max() / scale, np.abs(emulated - exact).max() / scale
    record("toy %s fp16 storage: engine %.3e, emulation %.3e (max|d| / max|ref| against float64)" % (toy, err, emu))
    assert np.isfinite(got).all() and err <= 4.0 * emu, (err, emu)
    if toy != "blurpool":
        assert [L["kernel"] for L in xcorr_layers(eng)] == [XCORR_KERNEL[toy] + "<_Float16>"], xcorr_layers(eng)
    _, (cap,) = run_engine(b, tmp_path, xs, forwards=3, graph=1, fp16=1)
    same_bits(cap, got, "toy %s fp16 captured" % toy)


ONE_OP = [(2, 8, 7, 9, 20, 3, 3, 1, 1, 1, 1), (1, 5, 8, 8, 3, 4, 2, 1, "same", 1, 1), (2, 4, 9, 9, 6, 3, 3, (2, 1), "valid", 2, 1),
          (2, 12, 9, 9, 12, 3, 3, 2, 1, 1, 12)]


@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("case", ONE_OP, ids=[xr.case_id(c) for c in ONE_OP])
def test_layer_against_the_op_level_call(gpu, tmp_path, case, with_bias):
    """x and the filter are both graph inputs, the bias a constant: the layer against float64 and bit for bit against the op-level call"""
    n, c, h, wd, oc, kh, kw, s, p, d, g = case
    x, w, bias = xr.operands(case, seed=21)
    b = mg.PnnxBuilder(seed=3)
    xi, wi = b.input((n, c, h, wd)), b.input((oc, c // g, kh, kw))
    b.output(b.conv2d_functional(xi, wi, b.attribute(bias) if with_bias else None, s, p, d, g))
    eng, (got,) = run_engine(b, tmp_path, [x, w])
    bias = bias if with_bias else None
    util.assert_parity(got, ref(case, x, w, bias), util.REL_TOL, what="layer " + xr.case_id(case))
    same_bits(got, run(case, x, w, bias), "layer against the op-level call")
    (layer,) = xcorr_layers(eng)
    assert layer["kernel"] == xr.kname(case, F32)
    assert layer["flops"] == 2.0 * got.size * (c // g) * kh * kw


def layout_steps(eng):
    return [L for L in eng.profile() if L["type"] in ("Tensor.view", "Tensor.reshape", "Tensor.permute")]


@pytest.mark.parametrize("fp16", [0, 1])
@pytest.mark.parametrize("batch", [1, 2])
def test_depthwise_sandwich_fused_and_unfused(gpu, tmp_path, batch, fp16):
    """fuse_xcorr=1: one xcorr_depthwise launch on the operands in front of the views and no layout step; fuse_xcorr=0 and fuse=0: the three
    layout steps around the unfused addressing; the same bits"""
    b = mg.build_toy_siamrpnpp(batch=batch)
    xs = toy_inputs(b, seed=9)
    fused, (got,) = run_engine(b, tmp_path, xs, fp16=fp16)
    sfx = "<_Float16>" if fp16 else "<float>"
    assert layout_steps(fused) == [], layout_steps(fused)
    assert [L["kernel"] for L in xcorr_layers(fused)] == ["xcorr_depthwise_kernel" + sfx]
    views = [_parse(ln)[1] for ln in b.lines if ln.startswith("Tensor.view")]
    assert set(views) <= set(fused.schedule()["fused"]), fused.schedule()
    for opts in (dict(fuse_xcorr=0), dict(fuse=0)):
        eng, (plain,) = run_engine(b, tmp_path, xs, fp16=fp16, **opts)
        assert len(layout_steps(eng)) == 3, (opts, layout_steps(eng))
        assert [L["kernel"] for L in xcorr_layers(eng)] == ["xcorr_depthwise_kernel" + sfx]
        same_bits(plain, got, "the sandwich under %r" % (opts,))


def test_blurpool_is_the_same_network_written_with_conv2d(gpu, tmp_path):
    b = mg.build_toy_blurpool()
    xs = toy_inputs(b)
    eng, (got,) = run_engine(b, tmp_path, xs)
    assert xcorr_layers(eng) == []
    # the same network with the module: the builder's second conv gets the blur filter as its weight
    m = mg.PnnxBuilder(seed=0)
    x = m.relu(m.conv(m.input((2, 3, 16, 16)), 8, 3, 1, 1))
    blur = m.conv(x, 8, 3, 2, 1, groups=8, bias=False)
    m.output(m.conv(blur, 4, 1, 1, 0))
    names = [_parse(ln)[1] for ln in m.lines if ln.startswith("nn.Conv2d")]
    a = np.array([1.0, 2.0, 1.0], F32)
    m.attrs[names[1] + ".weight"] = np.ascontiguousarray(np.broadcast_to((a[:, None] * a[None, :] / 16.0)[None, None], (8, 1, 3, 3)), dtype=F32)
    fn = [_parse(ln)[1] for ln in b.lines if ln.startswith("nn.Conv2d")]
    for src, dst in zip(fn, (names[0], names[2])):      # the two real convs carry the toy's weights
        for k in ("weight", "bias"):
            m.attrs[dst + "." + k] = b.attrs[src + "." + k]
    eng2, (want,) = run_engine(m, tmp_path, xs, tag="module")
    same_bits(got, want, "F.conv2d with a constant filter against nn.Conv2d")
    k1 = [L["kernel"] for L in eng.profile() if L["type"] == "nn.Conv2d"]
    k2 = [L["kernel"] for L in eng2.profile() if L["type"] == "nn.Conv2d"]
    assert k1 == k2 and len(k1) == 3, (k1, k2)


def test_fp16_engine_takes_the_fp32_fallback_for_a_layer_that_breaks_the_rule(gpu, tmp_path):
    """C = 12 dense between elementwise layers, so that the operands are halves: the layer runs its fp32 kernel between casts, and says so"""
    def graph(c):
        b = mg.PnnxBuilder(seed=3)
        xi, wi = b.input((2, c, 9, 9)), b.input((5, c, 3, 3))
        b.output(b.relu(b.conv2d_functional(b.relu(xi), b.relu(wi), None, 1, 1)))
        return b

    r = np.random.Generator(np.random.Philox(4))
    for c, kernel in ((12, "xcorr_dense_kernel<float>"), (16, "xcorr_dense_kernel<_Float16>")):
        b = graph(c)
        xs = [r.uniform(-1, 1, (2, c, 9, 9)).astype(F32), r.uniform(-0.3, 0.3, (5, c, 3, 3)).astype(F32)]
        # against the emulation that rounds where the engine stores a half (the inputs behind their ReLU, the conv's output): what is left
        # is the accumulation order and a rounding that may land one half ulp either way, 2^-11 of the element
        (want,) = xr.eval_graph(b, xs, rnd=xr.round_f16)
        eng, (got,) = run_engine(b, tmp_path, xs, tag="c%d" % c, fp16=1)
        (layer,) = xcorr_layers(eng)
        assert layer["kernel"] == kernel, layer
        util.assert_parity(got, want, F16_TOL, what="C = %d under fp16 storage" % c)
        casts = [s for s in eng.schedule()["run"] if "F_conv2d_0." in s and ("in_to_f32" in s or "out_to_f16" in s)]
        assert len(casts) == (3 if c == 12 else 0), eng.schedule()["run"]


def test_batch_modes_leave_a_tensor_filter_uncut_or_refuse(gpu, tmp_path):
    """host_slices leaves the graph uncut and lists the rule's reason; streams=2 and a re-batch are refused at load"""
    reason = "its dimension 0 counts filters, not images"
    toys = {"siamfc": mg.build_toy_siamfc(batch=2), "siamrpn": mg.build_toy_siamrpn(batch=2), "siamrpnpp": mg.build_toy_siamrpnpp(batch=2)}
    for toy, b in sorted(toys.items()):
        xs = toy_inputs(b)
        eng, (base,) = run_engine(b, tmp_path, xs, tag=toy)
        assert any(reason in m for m in eng.schedule()["batch_mixing"]), eng.schedule()["batch_mixing"]
        util.assert_parity(base, xr.eval_graph(b, xs)[0], what="toy %s at batch 2" % toy)
        eng, (got,) = run_engine(b, tmp_path, xs, tag=toy, host_slices=2)
        sched = eng.schedule()
        assert sched["lanes"] == 1 and sched["host_slices"] == 1 and any(reason in m for m in sched["batch_mixing"]), (toy, sched)
        same_bits(got, base, "toy %s under host_slices=2" % toy)
        assert status_of_load(b, tmp_path, toy, streams=2) == Status.kUnsupport
        assert status_of_load(b, tmp_path, toy, batch=4) == Status.kUnsupport


def test_dynamic_head_with_constant_derived_filters_is_split(gpu, tmp_path):
    b = mg.build_toy_dynamic_head(batch=2, constant=True)
    xs = toy_inputs(b, batch=8)
    eng, (base,) = run_engine(b, tmp_path, xs, batch=8)
    assert eng.schedule()["batch_mixing"] == [], eng.schedule()
    (want,) = xr.eval_graph(mg.build_toy_dynamic_head(batch=8, constant=True), xs)
    util.assert_parity(base, want, what="dynamic head re-batched to 8")
    for opts, slices, lanes in ((dict(host_slices=2), 2, 1), (dict(streams=2), 1, 2)):
        eng, (got,) = run_engine(b, tmp_path, xs, batch=8, **opts)
        sched = eng.schedule()
        assert sched["batch_mixing"] == [] and sched["host_slices"] == slices and sched["lanes"] == lanes, (opts, sched)
        same_bits(got, base, "dynamic head split %r" % (opts,))


def test_refused_at_load_with_a_status(gpu, tmp_path):
    """each refusal at LoadModel with its status; the process goes on"""
    def graph(xs, ws, groups=1, bias=None):
        b = mg.PnnxBuilder(seed=3)
        xi, wi = b.input(xs), b.input(ws)
        bi = b.input(bias) if bias else None
        b.output(b.conv2d_functional(xi, wi, bi, 1, 0, 1, groups))
        return b

    assert status_of_load(graph((1, 8, 9, 9), (8, 4, 3, 3), groups=2), tmp_path, "groups2") == Status.kUnsupport
    assert status_of_load(graph((1, 8, 9, 9), (4, 8, 3, 3), bias=(4,)), tmp_path, "tensor_bias") == Status.kUnsupport
    # a rank-3 x: the builder wants four dimensions, so the line is rewritten
    bad = graph((1, 8, 9, 9), (4, 8, 3, 3))
    bad.lines = [ln.replace("#0=(1,8,9,9)f32", "#0=(8,9,9)f32") for ln in bad.lines]
    assert status_of_load(bad, tmp_path, "rank3") == Status.kUnsupport
    wrong = graph((1, 8, 9, 9), (4, 8, 3, 3))
    wrong.lines = [ln.replace("#1=(4,8,3,3)f32", "#1=(4,6,3,3)f32") for ln in wrong.lines]
    assert status_of_load(wrong, tmp_path, "channels") == Status.kErrorShape
    for drop in ("stride=", "groups=", "padding="):
        b = graph((1, 8, 9, 9), (4, 8, 3, 3))
        b.lines[-2] = " ".join(tok for tok in b.lines[-2].split() if not tok.startswith(drop))
        assert status_of_load(b, tmp_path, "missing") == Status.kFail, drop
    b = graph((1, 8, 9, 9), (4, 8, 3, 3))
    xs = toy_inputs(b)
    _, (got,) = run_engine(b, tmp_path, xs)
    util.assert_parity(got, xr.eval_graph(b, xs)[0], what="after the refusals")
