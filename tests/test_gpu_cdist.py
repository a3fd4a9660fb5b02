"""GPU: torch.cdist (include/si_cdist.h) -- both kernels against float64 with derived bars, exact integer cases and the stated order of the
norms' additions bit for bit, NaN / infinity, bit-for-bit invariants, views under guard bands, and the layer in the engine.  Every check
prints its figures before it asserts (run with -s)."""
import functools

import numpy as np
import pytest
import torch

import cdist_reference as cr
import containment as ct
import util
from ct_reference import _parse
from simpleinfer_amd import hipops, modelgen as mg
from simpleinfer_amd.engine import Engine, Status, StatusError

pytestmark = pytest.mark.gpu
DTYPES = {"f32": np.float32, "f16": np.float16}
INF = float("inf")
MM, NO_MM = "use_mm_for_euclid_dist", "donot_use_mm_for_euclid_dist"
# (p, compute_mode, the kernel kind it must take whatever the shape)
FORMS = [(1.0, None, "direct"), (INF, None, "direct"), (2.0, MM, "mm"), (2.0, NO_MM, "direct")]


def run(x1, x2, p=2.0, mode=None, **views):
    return hipops.cdist(x1, x2, p, mode, **views), hipops.LAST_KERNEL_NAME["si_hip_cdist"]


@functools.lru_cache(maxsize=None)
def data(shape, dt, seed=0):
    return np.random.RandomState(seed + sum(shape)).standard_normal(shape).astype(DTYPES[dt])


def expected(kind, dt, p, m, vec_ok=True):
    return cr.kname("mm", DTYPES[dt], vec_ok and m % (4 if dt == "f32" else 8) == 0) if kind == "mm" else cr.kname("direct", DTYPES[dt], p)


# P, R around the mode threshold (25 / 26) and the tile (63 / 64 / 65 / 129), M around the vector (3 / 4), the K-tile (31 / 32 / 33) and
# several K-tiles (100); every broadcast form of the batch
SHAPES = [((1, 1), (26, 1)), ((25, 3), (25, 3)), ((26, 4), (1, 4)), ((3, 63, 31), (3, 65, 31)), ((64, 32), (64, 32)), ((1, 65, 33), (3, 129, 33)),
          ((3, 129, 100), (1, 63, 100)), ((3, 64, 8), (129, 8)), ((129, 64), (3, 26, 64))]


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("s1,s2", SHAPES, ids=["%sx%s" % ("_".join(map(str, a)), "_".join(map(str, b))) for a, b in SHAPES])
def test_kernels_against_float64(gpu, s1, s2, dt):
    x1, x2, m = data(s1, dt), data(s2, dt, 1), s1[-1]
    default_mm = s1[-2] > 25 or s2[-2] > 25
    for p, mode, kind in FORMS + [(2.0, None, "mm" if default_mm else "direct")]:
        got, kernel = run(x1, x2, p, mode)
        assert got.dtype == x1.dtype and kernel == expected(kind, dt, p, m), (kernel, p, mode)
        ratio, ok = cr.check(got, x1, x2, p, mm=kind == "mm")
        print("cdist %s x %s %s p=%s %s [%s]: worst error / bar %.3f" % (s1, s2, dt, p, mode, kernel, ratio))
        assert ok, (s1, s2, p, mode, ratio)


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_exact_integer_cases_and_the_order_of_the_norms(gpu, dt):
    r = np.random.RandomState(5)
    # small integers, Pythagorean rows among them: every fp32 product and sum is exact, so the result is the rounded root
    x1 = r.randint(-8, 9, (2, 70, 36)).astype(DTYPES[dt])
    x2 = r.randint(-8, 9, (2, 67, 36)).astype(DTYPES[dt])
    x1[0, 0], x2[0, :2] = 0, 0
    x1[0, 0, :2], x2[0, 0, 2:4], x2[0, 1, :2] = (3, 4), (5, 12), (3, 4)     # 5^2 + 13^2 = 194; and a distance of exactly 0
    for p, mode, kind in FORMS:
        got, kernel = run(x1, x2, p, mode)
        want = cr.cdist_ref(x1, x2, p).astype(np.float32).astype(x1.dtype)
        ct.assert_same_bits(got, want, "integer data, %s" % kernel)
        assert got[0, 0, 1] == 0 and (p != 2.0 or got[0, 0, 0] == np.sqrt(np.float32(194)).astype(x1.dtype))
        diag = run(x1, x1, p, mode)[0]
        assert (diag[:, np.arange(70), np.arange(70)] == 0).all(), "cdist(x, x) has a zero diagonal (%s)" % kernel
    # against a zero row the mm kernel returns sqrt(n): the numpy restatement of the norms' additions, bit for bit (m: vector and single-element)
    for m in (100, 33, 200):
        x, zero = data((70, m), dt, 9), np.zeros((1, m), DTYPES[dt])
        want = np.sqrt(cr.mm_sqnorm(x)).astype(x.dtype)
        ct.assert_same_bits(run(x, zero, 2.0, MM)[0][:, 0], want, "n1, m=%d" % m)
        ct.assert_same_bits(run(zero, x, 2.0, MM)[0][0], want, "n2, m=%d" % m)


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_nan_stays_in_its_row_and_infinity_is_torch_cpu(gpu, dt):
    x1, x2 = data((70, 20), dt), data((66, 20), dt, 1)
    for p, mode, kind in FORMS:
        clean, _ = run(x1, x2, p, mode)
        a, b = np.array(x1), np.array(x2)
        a[5, 3], b[64, 0] = np.nan, np.nan
        got, _ = run(a, b, p, mode)
        nan = np.isnan(got.astype(np.float64))
        assert nan[5].all() and nan[:, 64].all() and nan.sum() == 66 + 70 - 1, (p, mode, int(nan.sum()))
        ct.assert_same_bits(np.delete(np.delete(got, 5, 0), 64, 1), np.delete(np.delete(clean, 5, 0), 64, 1), "beside the NaN row and column")
        a, b = np.array(x1), np.array(x2)
        a[7, 2], b[3, 11], b[4, 2] = np.inf, -np.inf, np.inf
        got = run(a, b, p, mode)[0].astype(np.float32)
        t = torch.cdist(torch.from_numpy(a.astype(np.float32)), torch.from_numpy(b.astype(np.float32)), p=p, compute_mode=mode or MM).numpy()
        if p == INF:     # inf - inf at one k: the kernel's max keeps the NaN (the header's rule), torch's CPU max drops it
            assert np.isnan(got[7, 4]) and not np.isnan(t[7, 4])
            got[7, 4] = t[7, 4]
        assert np.array_equal(np.isnan(got), np.isnan(t)) and np.array_equal(np.isposinf(got), np.isposinf(t)), (p, mode)
        assert np.isposinf(t).any() and (p == INF or np.isnan(t).any())


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_invariants_bit_for_bit(gpu, dt):
    x1, x2 = data((3, 129, 40), dt), data((3, 70, 40), dt, 1)
    for p, mode, kind in FORMS:
        got, kernel = run(x1, x2, p, mode)
        ct.assert_same_bits(got, run(x1, x2, p, mode)[0], "two launches, %s" % kernel)
        for b in range(3):
            ct.assert_same_bits(got[b], run(x1[b], x2[b], p, mode)[0], "batch item %d alone, %s" % (b, kernel))
        ct.assert_same_bits(got[:, :64], run(x1[:, :64], x2, p, mode)[0], "the first 64 rows of P = 129 as P = 64, %s" % kernel)
        ct.assert_same_bits(got[:, :, :26], run(x1, x2[:, :26], p, mode)[0], "the first 26 columns of R = 70 as R = 26, %s" % kernel)


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("p,mode,kind", FORMS, ids=["p1", "pinf", "p2mm", "p2direct"])
def test_views_under_guard_bands(gpu, p, mode, kind, dt):
    x1, x2, nan, sentinel = data((2, 65, 24), dt), data((33, 24), dt, 1), float("nan"), 7.25
    dense, kd = run(x1, x2, p, mode)
    with hipops.guard_bands(0xFF):
        # rows 16 apart with NaN in the gaps; the output a column slice of a wider buffer that keeps its sentinel
        full, kernel = run(x1, x2, p, mode, x1_ld=40, x1_off=8, x1_fill=nan, x2_ld=32, x2_off=8, x2_fill=nan, out_ld=48, out_off=8, out_fill=sentinel, full=True)
        assert kernel == kd == expected(kind, dt, p, 24)
        ct.assert_same_bits(full[..., 8:41], dense, "the slice")
        assert (full[..., :8] == sentinel).all() and (full[..., 41:] == sentinel).all()
        # operands one element off the vector and strides no multiple of it: the single-element instantiation, the same bits
        odd, ko = run(x1, x2, p, mode, x1_ld=37, x1_off=1, x1_fill=nan, x2_ld=27, x2_off=3, x2_fill=nan, out_ld=35, out_off=1, out_fill=sentinel, full=True)
        assert ko == expected(kind, dt, p, 24, vec_ok=False), ko
        ct.assert_same_bits(odd[..., 1:34], dense, "the misaligned slice")
        assert (odd[..., :1] == sentinel).all() and (odd[..., 34:] == sentinel).all()


# ---- the layer in the engine
def run_engine(b, tmp_path, xs, tag="m", forwards=1, **opts):
    pp, bp = str(tmp_path / (tag + ".pnnx.param")), str(tmp_path / (tag + ".pnnx.bin"))
    b.save(pp, bp)
    e = Engine(**opts)
    e.load_model(pp, bp)
    for name, x in zip(e.input_names(), xs):
        e.input(name, x)
    for _ in range(forwards):
        e.forward()
    return e, e.extract(e.output_names()[0]) if forwards else None


def toy_inputs(b):
    shapes = [b.shapes[_parse(ln)[3][0]] for ln in b.lines if ln.startswith("pnnx.Input")]
    return [util.rng_uniform(31 + i, (n, h, w, c), 0.0, 1.0) for i, (n, c, h, w) in enumerate(shapes)]


# (vq_m12: rows of 12 elements, which the fp16 kernels do not take -- under fp16 storage the layer runs in fp32 between casts)
TOYS = {"matcher": mg.build_toy_descriptor_matcher, "vq": mg.build_toy_vq_encoder, "vq_m12": functools.partial(mg.build_toy_vq_encoder, d=12)}


@pytest.mark.parametrize("which", sorted(TOYS))
def test_toys_fp32_captured_fp16_storage_and_rebatched(gpu, tmp_path, which):
    b = TOYS[which](batch=2)
    xs = toy_inputs(b)
    exact, emulated = cr.eval_toy(b, xs), cr.eval_toy(b, xs, rnd=cr.round_f16)
    e, got = run_engine(b, tmp_path, xs)
    print("toy %s fp32: max-based %.3e, element-wise %.3e" % (which, util.rel_err(got, exact), util.mixed_err(got, exact)))
    util.assert_parity(got, exact, what="toy " + which)
    assert [L["kernel"] for L in e.profile() if L["type"] == "torch.cdist"] == [cr.kname("mm", np.float32, True)]
    ct.assert_same_bits(run_engine(b, tmp_path, xs, forwards=3, graph=1)[1], got, "graph=1 replay")
    # fp16 storage: the error against float64 held to 4x the error of the float64 emulation that rounds to fp16 at every half store
    e, half = run_engine(b, tmp_path, xs, fp16=1)
    scale = np.abs(exact).max()
    err, emu = np.abs(half - exact).max() / scale, np.abs(emulated - exact).max() / scale
    print("toy %s fp16 storage: engine %.3e, emulation %.3e (max|d| / max|ref| against float64)" % (which, err, emu))
    assert [L["kernel"] for L in e.profile() if L["type"] == "torch.cdist"] == [cr.kname("mm", np.float32 if which == "vq_m12" else np.float16, True)]
    assert np.isfinite(half).all() and err <= 4.0 * emu, (err, emu)
    # re-batched and split: dimension 0 is the batch
    b5 = TOYS[which](batch=5)
    x5 = toy_inputs(b5)
    ct.assert_same_bits(run_engine(b, tmp_path, x5, tag="b2", batch=5)[1], run_engine(b5, tmp_path, x5, tag="b5")[1], "batch=5 vs the file built at batch 5")
    x4 = [x[:4] for x in x5]
    _, whole = run_engine(b, tmp_path, x4, tag="b2", batch=4)
    for mode in ("streams", "host_slices"):
        e, split = run_engine(b, tmp_path, x4, tag="b2", batch=4, **{mode: 2})
        assert not e.schedule()["batch_mixing"], e.schedule()
        ct.assert_same_bits(split, whole, "%s=2 vs unsplit" % mode)


def one_op(s1, s2, p=2.0, mode=None, constant=None):
    b = mg.PnnxBuilder(seed=5)
    x1 = b.input(s1)
    b.output(b.cdist(x1, b.attribute(constant) if constant is not None else b.input(s2), p, mode))
    return b


@pytest.mark.parametrize("s1,s2,p,mode,const", [((2, 70, 24), (2, 30, 24), 2.0, None, False), ((2, 70, 24), (30, 24), 1.0, None, True),
                                                ((3, 20, 7), (1, 9, 7), INF, None, False), ((2, 70, 12), (70, 12), 2.0, NO_MM, True)])
def test_layer_is_the_op_level_call(gpu, tmp_path, s1, s2, p, mode, const):
    x1, x2 = util.rng_uniform(9, s1, -2.0, 2.0), util.rng_uniform(10, s2, -2.0, 2.0)
    e, got = run_engine(one_op(s1, s2, p, mode, x2 if const else None), tmp_path, [x1] if const else [x1, x2])
    (layer,) = [L for L in e.profile() if L["type"] == "torch.cdist"]
    want = hipops.cdist(x1, x2, p, mode)
    assert layer["kernel"] == hipops.LAST_KERNEL_NAME["si_hip_cdist"] and layer["flops"] > 0 and layer["bytes"] == 4 * (x1.size + x2.size + want.size), layer
    ct.assert_same_bits(got, want, "engine vs op level")


def test_point_sets_are_left_uncut_with_the_reason(gpu, tmp_path):
    """two rank-2 activations: dimension 0 counts points -- host_slices=2 serves the graph unsliced and names the layer; streams=2 and a
    re-batch are refused at load, also where the two point counts agree"""
    for r in (4, 9):
        b = one_op((4, 16), (r, 16))
        xs = [util.rng_uniform(3, (4, 16)), util.rng_uniform(4, (r, 16))]
        _, base = run_engine(b, tmp_path, xs)
        ct.assert_same_bits(base, hipops.cdist(xs[0], xs[1]), "unsplit")
        e, got = run_engine(b, tmp_path, xs, host_slices=2)
        sched = e.schedule()
        assert sched["host_slices"] == 1 and any("torch_cdist_0" in m and "counts points" in m for m in sched["batch_mixing"]), sched
        ct.assert_same_bits(got, base, "host_slices=2")
        for opts in (dict(streams=2), dict(batch=8), dict(batch=4)):
            with pytest.raises(StatusError) as ei:
                run_engine(b, tmp_path, xs, tag="refused", forwards=0, **opts)
            assert ei.value.status == Status.kUnsupport, opts


def test_load_refusals_leave_the_process_usable(gpu, tmp_path):
    cases = {"p = 3": (one_op((2, 5, 6), (2, 4, 6), 3.0), Status.kUnsupport), "p = 0.5": (one_op((2, 5, 6), (2, 4, 6), 0.5), Status.kUnsupport),
             "rank 4": (one_op((2, 3, 5, 6), (2, 3, 4, 6)), Status.kErrorShape), "unequal M": (one_op((2, 5, 6), (2, 4, 7)), Status.kErrorShape),
             "batches 2 and 3": (one_op((2, 5, 6), (3, 4, 6)), Status.kErrorShape)}
    for case, (b, status) in cases.items():
        with pytest.raises(StatusError) as ei:
            run_engine(b, tmp_path, [], tag="refused", forwards=0)
        assert ei.value.status == status, case
    test_layer_is_the_op_level_call(gpu, tmp_path, (2, 70, 24), (2, 30, 24), 2.0, None, False)      # ... and the same process loads and runs afterwards
