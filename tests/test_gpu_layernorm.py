"""GPU: F.layer_norm (include/si_layernorm.h) and F.gelu (include/si_act.h): the kernels against float64, exact rows, bit-for-bit invariants,
special values, views under guard bands, and the layers in the engine.  Every check prints its figures before it asserts (run with -s)."""
import functools

import numpy as np
import pytest
import torch

import act_reference as ar
import containment as ct
import elementwise_reference as er
import layernorm_reference as lnr
import util
from simpleinfer_amd import hipops, modelgen as mg
from simpleinfer_amd.engine import Engine, Status, StatusError

pytestmark = pytest.mark.gpu
DTYPES = {"f32": np.float32, "f16": np.float16}
WORST = {}


def run(x, gamma=None, beta=None, eps=1e-5, **views):
    return hipops.layernorm(x, gamma, beta, eps, **views), hipops.LAST_KERNEL_NAME["si_hip_layernorm"]


@functools.lru_cache(maxsize=None)
def data(rows, c, dt):
    """mean 3, standard deviation 0.5: E[x^2] - mean^2 would lose six bits here"""
    return (3.0 + 0.5 * np.random.RandomState(17 + c).standard_normal((rows, c))).astype(DTYPES[dt])


@functools.lru_cache(maxsize=None)
def params(c, affine):
    r = np.random.RandomState(c)
    g, b = r.uniform(0.5, 1.5, c).astype(np.float32), r.uniform(-0.5, 0.5, c).astype(np.float32)
    return (g if affine != "none" else None), (b if affine == "both" else None)


def bar_of(x, g, b, ref):
    """4x the error torch's CPU fp32 F.layer_norm makes on the same inputs against the same float64 (the margin: another order of additions);
    under fp16 storage plus, per element, half an fp16 ulp of the reference"""
    t = lambda a: None if a is None else torch.from_numpy(np.asarray(a, np.float32))
    cpu = torch.nn.functional.layer_norm(t(x), (x.shape[-1],), t(g), t(b), 1e-5).numpy()
    allow = 4.0 * float(np.abs(cpu.astype(np.float64) - ref).max())
    return allow if x.dtype == np.float32 else allow + 0.5 * np.spacing(np.abs(ref).astype(np.float16)).astype(np.float64)


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("c", (1, 3, 4, 5, 8, 255, 256, 260, 1024, 1028, 4096, 4100))
def test_kernel_against_float64(gpu, c, dt):
    for rows in (1, 3, 67):
        for affine in ("both", "none", "weight"):
            x, (g, b) = data(rows, c, dt), params(c, affine)
            got, kernel = run(x, g, b)
            assert got.dtype == x.dtype and kernel == lnr.expected_kernel(c, x.dtype, c % (4 if dt == "f32" else 8) == 0), kernel
            ref = lnr.layernorm_ref(x, g, b)
            err, bar = np.abs(got.astype(np.float64) - ref), bar_of(x, g, b, ref)
            ratio = float((err / np.maximum(bar, 1e-300)).max()) if err.max() > 0 else 0.0
            key = (kernel.split("<")[0], dt)
            WORST[key] = max(WORST.get(key, 0.0), ratio)
            print("layernorm c=%d rows=%d %s %s [%s]: max|d| %.3e, worst error / bar %.3f (per form so far %.3f)" % (c, rows, dt, affine, kernel, err.max(), ratio, WORST[key]))
            assert np.all(err <= bar), (c, rows, affine, float(err.max()))


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("c", (8, 260, 1028, 4100))
def test_exact_rows_and_invariants(gpu, c, dt):
    g, b = params(c, "both")
    # equal values whose sums are exact: every centred value is +0, the result is beta
    x = np.repeat(np.array([[3.0], [-0.5], [0.0]]), c, axis=1).astype(DTYPES[dt])
    ct.assert_same_bits(run(x, g, b)[0], np.broadcast_to(b, x.shape).astype(x.dtype), "equal rows give beta, c=%d" % c)
    # +-1 in equal numbers with eps = 0: mean 0, variance 1, rstd 1 -- (+-1 * gamma) + beta in fp32, rounded once at a half store
    s = np.where(np.random.RandomState(c).permutation(c) % 2 == 0, 1.0, -1.0).astype(np.float32)
    x = np.stack([s, -s]).astype(DTYPES[dt])
    ct.assert_same_bits(run(x, g, b, eps=0.0)[0], (x.astype(np.float32) * g + b).astype(x.dtype), "+-1 rows give +-gamma + beta, c=%d" % c)
    # two launches, a row alone, and a NaN / Inf row that poisons only itself
    x = data(5, c, dt)
    y, k = run(x, g, b)
    ct.assert_same_bits(y, run(x, g, b)[0], "two launches")
    ct.assert_same_bits(y[3:4], run(x[3:4], g, b)[0], "row 3 alone")
    for poison in (np.nan, np.inf, -np.inf):
        z = np.array(x)
        z[1, c // 2] = poison
        yz, _ = run(z, g, b)
        assert np.isnan(yz[1].astype(np.float64)).all(), poison
        ct.assert_same_bits(np.delete(yz, 1, 0), np.delete(y, 1, 0), "the other rows beside a %s row" % poison)


@pytest.mark.parametrize("form,rows,c,dt", [("row_group", 2 * 2048 * 256 + 5, 4, "f32"), ("row_block", 2 * 2048 + 5, 1032, "f16"),
                                            ("row_block_3pass", 2 * 2048 + 5, 4104, "f16")], ids=["row_group", "row_block", "row_block_3pass"])
def test_three_passes_of_the_grid_stride_loop(gpu, form, rows, c, dt):
    """the capped grid is 2048 workgroups: the last rows are computed in a third pass, with the bits they have in a launch of their own"""
    x = np.tile(data(64, c, dt), (rows // 64 + 1, 1))[:rows]
    x = np.ascontiguousarray(x + (np.arange(rows) % 7)[:, None].astype(x.dtype))
    g, b = params(c, "both")
    y, kernel = run(x, g, b)
    assert kernel == lnr.kname(form, x.dtype, True), kernel
    for lo, hi in ((0, 9), (rows // 2, rows // 2 + 9), (rows - 9, rows)):
        ct.assert_same_bits(y[lo:hi], run(x[lo:hi], g, b)[0], "%s rows %d .. %d of three passes" % (form, lo, hi))


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("c", (8, 264, 1032, 4104))
def test_views_under_guard_bands(gpu, c, dt):
    x, (g, b) = data(3, c, dt), params(c, "both")
    (dense, kd), nan, sentinel = run(x, g, b), float("nan"), 7.25
    with hipops.guard_bands(0xFF):
        # rows 8 apart with NaN in the gaps; the output a channel slice of a wider buffer that keeps its sentinel
        full, kernel = run(x, g, b, in_ld=c + 8, in_c_off=8, in_fill=nan, out_ld=c + 16, out_c_off=8, out_fill=sentinel, full=True)
        assert kernel == kd
        ct.assert_same_bits(full[:, 8:8 + c], dense, "the slice")
        assert (full[:, :8] == sentinel).all() and (full[:, 8 + c:] == sentinel).all()
        # a slice one element off the vector: the single-element instantiation
        odd, ko = run(x, g, b, in_ld=c + 8, in_c_off=1, in_fill=nan, out_ld=c + 8, out_c_off=3, out_fill=sentinel, full=True)
        assert ko == lnr.expected_kernel(c, x.dtype, False), ko
        assert (odd[:, :3] == sentinel).all() and (odd[:, 3 + c:] == sentinel).all()
    ref = lnr.layernorm_ref(x, g, b)
    assert np.all(np.abs(odd[:, 3:3 + c].astype(np.float64) - ref) <= bar_of(x, g, b, ref))


@pytest.mark.parametrize("approximate", ["none", "tanh"])
def test_gelu_within_4_fp32_ulp_and_1_fp16_ulp(gpu, approximate):
    x = ar.fp32_inputs()
    ref = lnr.gelu_ref(x.astype(np.float64), approximate)
    outs = []
    for c in (8, 7):       # the vector and the single-element arm
        t, n = er.as_rows(x, c, odd_pixels=True)
        outs.append(hipops.gelu(t, approximate).reshape(-1)[:n])
    er.assert_arms_agree(outs[0], outs[1], "gelu %s vector vs scalar" % approximate)
    e = er.ulp32(outs[0], ref)
    print("gelu %s fp32: worst %.3f ulp at x = %r on %d values" % (approximate, float(e.max()), x[int(np.argmax(e))], x.size))
    er.assert_ulp32(outs[0], ref, 4, "gelu " + approximate)
    tail = (x < -6) & (x > (-12 if approximate == "none" else -9))      # (the tanh formula underflows below x = -10.2)
    assert tail.any() and (outs[0][tail] != 0).all(), "the negative tail is there"
    h = er.all_halves()
    t, n = er.as_rows(h, 8, odd_pixels=True)
    got, ref = hipops.gelu(t, approximate).reshape(-1)[:n], lnr.gelu_ref(h.astype(np.float64), approximate)
    d = er.half_ulp(got, ref)
    print("gelu %s fp16: %d of 65536 inputs differ from the reference rounded once, worst %d fp16 ulp" % (approximate, int((d > 0).sum()), int(d.max())))
    er.assert_half(got, ref, 1, "gelu %s fp16" % approximate, max_share=er.H_MISMATCH_SHARE)


def run_engine(b, tmp_path, x, tag="m", forwards=1, **opts):
    pp, bp = str(tmp_path / (tag + ".pnnx.param")), str(tmp_path / (tag + ".pnnx.bin"))
    b.save(pp, bp)
    e = Engine(**opts)
    e.load_model(pp, bp)
    for _ in range(forwards):
        e.input(e.input_names()[0], x)
        e.forward()
    return e, e.extract(e.output_names()[0])


@pytest.mark.parametrize("op,shape,arg", [("ln", (5, 24), "both"), ("ln", (3, 7, 32), "both"), ("ln", (3, 7, 33), "weight"), ("ln", (2, 3, 1028), "none"),
                                          ("gelu", (3, 7, 32), "none"), ("gelu", (5, 24), "tanh")])
def test_engine_one_op_graph(gpu, tmp_path, op, shape, arg):
    b = mg.PnnxBuilder(seed=5)
    g, bt = params(shape[-1], arg) if op == "ln" else (None, None)
    x = b.input(shape)
    b.output(b.layer_norm(x, False if g is None else g, False if bt is None else bt) if op == "ln" else b.gelu(x, arg))
    xin = util.rng_uniform(9, shape, -2.0, 4.0)
    e, got = run_engine(b, tmp_path, xin)
    want = hipops.layernorm(xin, g, bt) if op == "ln" else hipops.gelu(xin, arg)
    ct.assert_same_bits(got, want.reshape(got.shape), "engine vs op level")
    (layer,) = [L for L in e.profile() if L["type"] in ("F.layer_norm", "F.gelu")]
    assert layer["kernel"] == (hipops.LAST_KERNEL_NAME["si_hip_layernorm"] if op == "ln" else "param_act"), layer     # (the activation layer reports its family)


def test_toy_vit_block_fp32_captured_and_fp16_storage(gpu, tmp_path):
    b = mg.build_toy_vit_block(2, 16, 32, 4, 2)
    x = mg.synth_input((2, 16, 16, 3))
    exact, emulated = lnr.eval_graph(b, x), lnr.eval_graph(b, x, rnd=lnr.round_f16)
    e, got = run_engine(b, tmp_path, x)
    print("toy vit block fp32: max-based %.3e, element-wise %.3e" % (util.rel_err(got, exact), util.mixed_err(got, exact)))
    util.assert_parity(got, exact, what="toy vit block")
    assert [L["kernel"] for L in e.profile() if L["type"] == "F.layer_norm"] == [lnr.kname("row_group", np.float32, True)] * 5
    assert [L["kernel"] for L in e.profile() if L["type"] == "F.gelu"] == ["param_act"] * 2
    ct.assert_same_bits(run_engine(b, tmp_path, x, forwards=3, graph=1)[1], got, "graph=1 replay")
    # fp16 storage: the error against float64 held to 4x the error of the float64 emulation that rounds to fp16 at every half store
    e, half = run_engine(b, tmp_path, x, fp16=1)
    scale = np.abs(exact).max()
    err, emu = np.abs(half - exact).max() / scale, np.abs(emulated - exact).max() / scale
    print("toy vit block fp16 storage: engine %.3e, emulation %.3e (max|d| / max|ref| against float64)" % (err, emu))
    assert [L["kernel"] for L in e.profile() if L["type"] == "F.layer_norm"] == [lnr.kname("row_group", np.float16, True)] * 5
    assert np.isfinite(half).all() and err <= 4.0 * emu, (err, emu)


def test_toy_vit_block_rebatched_and_split(gpu, tmp_path):
    b2, b5 = mg.build_toy_vit_block(2, 16, 32, 4, 2), mg.build_toy_vit_block(5, 16, 32, 4, 2)
    x = util.rng_uniform(21, (5, 16, 16, 3), 0.0, 1.0)
    ct.assert_same_bits(run_engine(b2, tmp_path, x, tag="b2", batch=5)[1], run_engine(b5, tmp_path, x, tag="b5")[1], "batch=5 vs the file built at batch 5")
    _, whole = run_engine(b2, tmp_path, x[:4], tag="b2", batch=4)
    for mode in ("streams", "host_slices"):
        e, split = run_engine(b2, tmp_path, x[:4], tag="b2", batch=4, **{mode: 2})
        assert not e.schedule()["batch_mixing"], e.schedule()
        ct.assert_same_bits(split, whole, "%s=2 vs unsplit" % mode)


def test_load_refusals_leave_the_process_usable(gpu, tmp_path):
    for case in ("rank 4", "normalized_shape of two dimensions", "an activation (a second graph input) as weight"):
        b = mg.PnnxBuilder(seed=1)
        x = b.input((2, 8, 5, 6) if case == "rank 4" else (2, 5, 6))
        b.output(b.layer_norm(x, weight=b.input((6,)), bias=False) if case.startswith("an activation") else b.layer_norm(x))
        if case.startswith("normalized_shape"):
            b.lines = [ln.replace("normalized_shape=(6)", "normalized_shape=(5,6)") for ln in b.lines]
            assert any("(5,6)" in ln for ln in b.lines)
        with pytest.raises(StatusError) as ei:
            run_engine(b, tmp_path, None, tag="refused", forwards=0)
        assert ei.value.status == Status.kUnsupport, case
    test_engine_one_op_graph(gpu, tmp_path, "ln", (5, 24), "both")                  # ... and the same process loads and runs afterwards
