"""GPU: the fused nearest-row search (include/si_nearest.h) against the unfused composition -- si_hip_cdist_* in mm mode, then the order rule
in numpy -- without a tolerance; exact integer data with planted ties across tile and split boundaries; split invariance; NaN and equal
keys; views under guard bands."""
import functools

import numpy as np
import pytest

import cdist_reference as cr
import containment as ct
import nearest_reference as nref
import util
from simpleinfer_amd import hipops, modelgen as mg
from simpleinfer_amd.engine import Engine, Status, StatusError

pytestmark = pytest.mark.gpu
DTYPES = {"f32": np.float32, "f16": np.float16}
MM = "use_mm_for_euclid_dist"
OUTPUTS = ("idx", "dist", "rows")


@functools.lru_cache(maxsize=None)
def data(shape, dt, seed=0):
    return np.random.RandomState(seed + sum(shape)).standard_normal(shape).astype(DTYPES[dt])


def take_rows(x2, idx0):
    """x2[b, idx0[b, i]] for x2 [R, M] or [B, R, M] and idx0 [.., P]"""
    return x2[idx0] if x2.ndim == 2 else np.stack([x2[b][idx0[b]] for b in range(len(x2))])


def same(a, b, what):
    """bit for bit, a NaN equal to a NaN (the search returns one quiet NaN for every NaN distance)"""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, what
    a, b, nan = a.copy(), b.copy(), np.isnan(a) & np.isnan(b)
    a[nan], b[nan] = 0, 0
    ct.assert_same_bits(a, b, what)


def check_against_cdist(out, x1, x2, k):
    """the four statements of the header about one result and the matrix D of the unfused launch"""
    D = hipops.cdist(x1, x2, 2.0, MM)
    order = nref.topk(D, k)                                   # NaN-aware: the first NaN of a row, else the first minimum
    idx, dist = out["idx"], out["dist"]
    assert idx.dtype == np.int32 and dist.dtype == np.float32 and idx.shape == dist.shape == D.shape[:-1] + (k,)
    picked = np.take_along_axis(D, idx.astype(np.int64), -1)
    same(picked[..., 0], np.take_along_axis(D, order[..., :1].astype(np.int64), -1)[..., 0], "D[idx0] is the row's minimum")
    nan_rows = np.isnan(D.astype(np.float64)).any(-1)
    assert np.array_equal(idx[nan_rows, 0], order[nan_rows, 0]), "a row with a NaN: its first NaN"
    same(dist.astype(D.dtype), picked, "dist has the bits of D[idx]")
    if k == 2:
        rest = D.astype(np.float64)
        np.put_along_axis(rest, idx[..., :1].astype(np.int64), np.inf, -1)       # column idx0 removed
        second = np.take_along_axis(rest, nref.topk(rest, 1).astype(np.int64), -1)[..., 0]
        assert (idx[..., 0] != idx[..., 1]).all()
        same(picked[..., 1].astype(np.float64), second, "dist1 is the minimum of the rest")
    ct.assert_same_bits(out["rows"], take_rows(x2, idx[..., 0]), "rows == x2[idx0]")


PS, RS = (1, 63, 64, 65, 129), (1, 2, 63, 64, 65, 129, 257)
MS = {"f32": (1, 4, 31, 32, 33, 72), "f16": (8, 56, 64, 72)}


def case(dt, i):
    """case i of a covering set: P, R and M walk their lists at coprime periods; k, the batch and a shared x2 alternate at their own"""
    r = RS[i % 7]
    return (dt, PS[i % 5], r, MS[dt][i % len(MS[dt])], 1 if r == 1 else 1 + (i // 2) % 2, (1, 3)[(i // 3) % 2], i % 4 < 2)


CASES = [case("f32", i) for i in range(24)] + [case("f16", i) for i in range(16)]


@pytest.mark.parametrize("dt,p,r,m,k,b,shared", CASES, ids=["%s-P%d-R%d-M%d-k%d-B%d%s" % (c[:6] + ("s" if c[6] else "",)) for c in CASES])
def test_against_the_unfused_composition(gpu, dt, p, r, m, k, b, shared):
    x1 = data((b, p, m) if b > 1 else (p, m), dt)
    x2 = data((r, m) if shared or b == 1 else (b, r, m), dt, 1)
    out = hipops.nearest(x1, x2, k)
    assert hipops.LAST_KERNEL_NAME["si_hip_nearest"] == nref.kname(DTYPES[dt], m % 4 == 0, k)
    check_against_cdist(out, x1, x2, k)


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_exact_on_integer_data_with_planted_ties(gpu, dt):
    """small integers: every fp32 product and sum is exact, so idx is the order rule on the float64 distances -- and a planted copy of the
    nearest row in a later tile (and so in a later split) must lose to the lower column"""
    rs = np.random.RandomState(11)
    R = 200
    x1 = rs.randint(-8, 9, (70, 40)).astype(DTYPES[dt])
    x2 = rs.randint(-8, 9, (R, 40)).astype(DTYPES[dt])
    for row, (col, copies) in enumerate({0: (70, 199), 63: (65,), 64: (130,), R - 1: ()}.items()):
        for c in (col,) + copies:
            x2[c] = x1[3 + row]                # distance exactly 0, at `col` first
    want = nref.topk(cr.cdist_ref(x1, x2), 2)
    assert [tuple(want[3 + i]) for i in range(3)] == [(0, 70), (63, 65), (64, 130)] and want[6, 0] == R - 1
    for splits in (1, 3, 4):                   # 4 tiles: 3 splits as two of 2 tiles and an empty one, 4 of one tile each
        out = hipops.nearest(x1, x2, 2, splits=splits)
        assert np.array_equal(out["idx"], want), splits
        ct.assert_same_bits(out["dist"], np.take_along_axis(cr.cdist_ref(x1, x2), want.astype(np.int64), -1).astype(np.float32), "integer distances")
        assert (out["dist"][3:7, 0] == 0).all()


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("p,r", [(70, 200), (5, 65), (129, 1000)], ids=["P70-R200", "P5-R65", "P129-R1000"])
def test_split_invariance(gpu, dt, p, r):
    """R = 200 and 1000 are no multiple of 64 * splits; with R = 65 (2 tiles) and 16 splits fourteen splits get no column"""
    x1, x2 = data((3, p, 24), dt), data((3, r, 24), dt, 1)
    base = hipops.nearest(x1, x2, 2, splits=1)
    check_against_cdist(base, x1, x2, 2)
    for splits in (2, 3, 16, 0, 1):            # 0: the plan's choice (more than one split at these shapes); 1 again: two launches
        got = hipops.nearest(x1, x2, 2, splits=splits)
        for name in OUTPUTS:
            ct.assert_same_bits(got[name], base[name], "%s, splits=%d" % (name, splits))
    for b in range(3):
        for splits in (1, 3):
            alone = hipops.nearest(x1[b], x2[b], 2, splits=splits)
            for name in OUTPUTS:
                ct.assert_same_bits(alone[name], base[name][b], "%s, batch item %d alone, splits=%d" % (name, b, splits))
    first = hipops.nearest(x1, x2, 1, splits=3)                                  # k = 1 is the first column of k = 2
    ct.assert_same_bits(first["idx"], base["idx"][..., :1], "k = 1")
    ct.assert_same_bits(first["rows"], base["rows"], "k = 1 rows")


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("splits", [1, 3])
def test_nan_and_equal_keys(gpu, dt, splits):
    x1, x2 = data((66, 16), dt), data((140, 16), dt, 1)
    # NaN rows of x2 in the second and third tile: the first NaN wins, the second NaN is second
    b = np.array(x2)
    b[70, 3], b[130, 0] = np.nan, np.nan
    out = hipops.nearest(x1, b, 2, splits=splits)
    assert (out["idx"] == (70, 130)).all() and np.isnan(out["dist"]).all()
    check_against_cdist(out, x1, b, 2)
    # a NaN in a row of x1: every key of the row is NaN, index 0 (and 1); the other rows as without it
    a = np.array(x1)
    a[5, 7] = np.nan
    clean, out = hipops.nearest(x1, x2, 2, splits=splits), hipops.nearest(a, x2, 2, splits=splits)
    assert tuple(out["idx"][5]) == (0, 1) and np.isnan(out["dist"][5]).all()
    ct.assert_same_bits(out["rows"][5], x2[0], "the NaN row takes row 0")
    for name in OUTPUTS:
        ct.assert_same_bits(np.delete(out[name], 5, 0), np.delete(clean[name], 5, 0), name + " beside the NaN row")
    # an all-equal codebook: every key of a row ties, columns 0 and 1; and infinite rows (inf - inf: NaN keys) follow the composition
    out = hipops.nearest(x1, np.tile(x2[:1], (140, 1)), 2, splits=splits)
    assert (out["idx"] == (0, 1)).all() and (out["dist"][:, 0] == out["dist"][:, 1]).all()
    b = np.array(x2)
    b[3, 2], b[90, 5] = np.inf, -np.inf
    check_against_cdist(hipops.nearest(x1, b, 2, splits=splits), x1, b, 2)


# ---- the engine: torch.cdist -> torch.argmin -> F.embedding / nn.Embedding as one launch (pnnx/lower_nearest_rows.h)
def run_engine(b, tmp_path, x, tag="m", forwards=1, **opts):
    pp, bp = str(tmp_path / (tag + ".pnnx.param")), str(tmp_path / (tag + ".pnnx.bin"))
    b.save(pp, bp)
    e = Engine(**opts)
    e.load_model(pp, bp)
    e.input(e.input_names()[0], x)
    for _ in range(forwards):
        e.forward()
    return e, e.extract(e.output_names()[0]) if forwards else None


def vq_trunk(batch, d):
    """build_toy_vq up to z: the same names and seed, so the same weights"""
    b = mg.PnnxBuilder(0)
    b.output(b.view(b.permute(b.conv(b.input((batch, 3, 8, 8)), d, 3, 1), (0, 2, 3, 1)), (batch, -1, d)))
    return b


def check_quantised(got, z, table, what):
    """every row of got is a row of table bit for bit, and the row the float64 rule accepts.  The kernel's key of a pair is within
    bar = (M + 3) u (|z| + |c|)^2 + 2 u D^2 (half the mm bar of cdist_reference.check, which is stated for the squared result) of the true
    squared distance, so the chosen column's true key is above the row's minimum by at most its bar plus the minimum's; where the float64
    gap between best and second best exceeds that, the choice is the float64 argmin"""
    rows = {r.tobytes(): j for j, r in enumerate(table)}
    idx = np.array([rows.get(r.tobytes(), -1) for r in got.reshape(-1, got.shape[-1])])
    assert (idx >= 0).all(), "%s: %d rows are no row of the codebook" % (what, int((idx < 0).sum()))
    z = z.reshape(-1, z.shape[-1]).astype(np.float64)
    D2 = cr.cdist_ref(z, table) ** 2
    norms = np.sqrt((z * z).sum(-1))[:, None] + np.sqrt((table.astype(np.float64) ** 2).sum(-1))[None, :]
    bar = (z.shape[-1] + 3) * cr.U * norms ** 2 + 2.0 * cr.U * D2
    order = nref.topk(D2, 2).astype(np.int64)
    at = lambda a, j: np.take_along_axis(a, j[:, None], -1)[:, 0]
    clear = at(D2, order[:, 1]) - at(D2, order[:, 0]) > at(bar, order[:, 1]) + at(bar, order[:, 0])
    excess = at(D2, idx) - at(D2, order[:, 0])
    print("%s: %d rows, gap clear in %.1f %%, off the float64 argmin in %d, worst excess / bar %.3f" % (
        what, len(idx), 100 * clear.mean(), int((idx != order[:, 0]).sum()), float((excess / (at(bar, idx) + at(bar, order[:, 0]))).max())))
    assert clear.mean() >= 0.99, "the case must separate best and second best"
    assert (excess <= at(bar, idx) + at(bar, order[:, 0])).all() and (idx != order[:, 0]).mean() <= 0.01 and (idx[clear] == order[clear, 0]).all()


@pytest.mark.parametrize("module", [False, True], ids=["F.embedding", "nn.Embedding"])
def test_engine_runs_the_vq_lookup_as_one_launch(gpu, tmp_path, module):
    b, x = mg.build_toy_vq(batch=2, module=module), util.rng_uniform(31, (2, 8, 8, 3), 0.0, 1.0)
    table = b.attrs["pnnx_attr_0.data"]
    e, got = run_engine(b, tmp_path, x)
    kernels = [L["kernel"] for L in e.profile()]
    assert [L["kernel"] for L in e.profile() if L["type"] == "torch.cdist"] == [nref.kname(np.float32, True, 1)] and not any(k.startswith("cdist_") for k in kernels)
    check_quantised(got, run_engine(vq_trunk(2, 16), tmp_path, x, tag="z")[1], table, "fp32")
    ct.assert_same_bits(run_engine(b, tmp_path, x, forwards=3, graph=1)[1], got, "graph=1, three forwards")
    # fp16 storage: z and the codebook as stored halves, the half kernel (M = 16); M = 12 runs the fp32 kernel between casts
    e, half = run_engine(b, tmp_path, x, fp16=1)
    assert [L["kernel"] for L in e.profile() if L["type"] == "torch.cdist"] == [nref.kname(np.float16, True, 1)]
    check_quantised(half, run_engine(vq_trunk(2, 16), tmp_path, x, tag="z", fp16=1)[1], table.astype(np.float16).astype(np.float32), "fp16=1")
    b12 = mg.build_toy_vq(batch=2, d=12, module=module)
    e, half = run_engine(b12, tmp_path, x, tag="m12", fp16=1)
    assert [L["kernel"] for L in e.profile() if L["type"] == "torch.cdist"] == [nref.kname(np.float32, True, 1)]
    check_quantised(half, run_engine(vq_trunk(2, 12), tmp_path, x, tag="z12", fp16=1)[1], b12.attrs["pnnx_attr_0.data"].astype(np.float16).astype(np.float32), "fp16=1, M = 12")
    # re-batched and split: dimension 0 is the batch
    x5 = util.rng_uniform(32, (5, 8, 8, 3), 0.0, 1.0)
    ct.assert_same_bits(run_engine(b, tmp_path, x5, batch=5)[1], run_engine(mg.build_toy_vq(batch=5, module=module), tmp_path, x5, tag="b5")[1], "batch=5")
    whole = run_engine(b, tmp_path, x5[:4], batch=4)[1]
    for mode in ("streams", "host_slices"):
        e, split = run_engine(b, tmp_path, x5[:4], batch=4, **{mode: 2})
        assert not e.schedule()["batch_mixing"], e.schedule()
        ct.assert_same_bits(split, whole, "%s=2 vs unsplit" % mode)


def test_engine_refuses_other_chains_and_stays_usable(gpu, tmp_path):
    for name, b in nref.vq_refusals().items():
        with pytest.raises(StatusError) as ei:
            run_engine(b, tmp_path, None, tag="refused", forwards=0)
        assert ei.value.status == Status.kUnsupport, name
    b, x = mg.build_toy_vq(batch=2), util.rng_uniform(31, (2, 8, 8, 3), 0.0, 1.0)
    check_quantised(run_engine(b, tmp_path, x)[1], run_engine(vq_trunk(2, 16), tmp_path, x, tag="z")[1], b.attrs["pnnx_attr_0.data"], "after the refusals")


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_views_under_guard_bands(gpu, dt):
    x1, x2, nan, sentinel = data((2, 65, 24), dt), data((70, 24), dt, 1), float("nan"), 7.25
    dense = hipops.nearest(x1, x2, 2)
    # rows 16 apart with NaN in the gaps, the winning rows into a column slice of a wider buffer that keeps its sentinel; then one element off
    # the vector with strides no multiple of it: fp32 takes the single-element instantiation, the fp16 entry refuses
    wide, odd = dict(x1_ld=40, x1_off=8, x2_ld=32, x2_off=8, rows_ld=48, rows_off=8), dict(x1_ld=37, x1_off=1, x2_ld=27, x2_off=3, rows_ld=35, rows_off=1)
    if dt == "f16":
        assert hipops.nearest_kernel_name(x1.shape, x2.shape, 2, True, x1_ld=37, x2_ld=27, rows_ld=35) == "none"
    with hipops.guard_bands(0xFF):
        for views, vec, splits in [(wide, True, 1), (wide, True, 2)] + [(odd, False, 1)] * (dt == "f32"):
            got = hipops.nearest(x1, x2, 2, splits=splits, x1_fill=nan, x2_fill=nan, rows_fill=sentinel, full=True, **views)
            assert hipops.LAST_KERNEL_NAME["si_hip_nearest"] == nref.kname(DTYPES[dt], vec, 2)
            lo = views["rows_off"]
            ct.assert_same_bits(got["rows"][..., lo:lo + 24], dense["rows"], "the slice")
            assert (got["rows"][..., :lo] == sentinel).all() and (got["rows"][..., lo + 24:] == sentinel).all()
            ct.assert_same_bits(got["idx"], dense["idx"], "idx")
            ct.assert_same_bits(got["dist"], dense["dist"], "dist")
