"""GPU: torch.norm / F.normalize -- si_hip_lpnorm_f32 / _f16 (include/si_lpnorm.h).  Every form and instantiation BIT FOR BIT against the
numpy float32 restatement of the header's documented order of additions (tests/lpnorm_reference.py), and within the derived bars of
float64; results that are exact by construction; special values; the invariants (two runs, image i alone, set independence, three passes
of the grid-stride loop); strided views under guard bands; the refusals; and the layer inside the engine: one-op graphs against the
op-level call, the toy SuperPoint in both spellings (the planner pass fuse_norm against the unfused plan, the same bits in fp32) and the
toy embedding head, in fp32, captured, re-batched, batch-split and under fp16 storage.  Every engine test fails without the layer
(LoadModel rejects the types), every op-level test without the kernels (the symbols are missing).

Every check prints its figures before it asserts (run with -s)."""
import ctypes as C
import functools

import numpy as np
import pytest

import containment as ct
import lpnorm_reference as lr
import util
from ct_reference import _parse
from simpleinfer_amd import _native, hipops, modelgen as mg
from simpleinfer_amd.engine import Engine, Status, StatusError
from test_gpu_f16 import F16_TOL

pytestmark = pytest.mark.gpu

DTYPES = {"f32": np.float32, "f16": np.float16}
INF = float("inf")
G, B, REG = lr.header_enum("SI_LPNORM_GROUP_MAX_C"), lr.header_enum("SI_LPNORM_BLOCK_MAX_C"), lr.header_enum("SI_LPNORM_COL_REG_POSITIONS")
SINGLE = (1, 2, 4, 8)

ROW_C = (1, 3, 4, 5, 63, 64, 65, 257, 1024, 1025, 4096, 4097)
ROW_CASES = [((1 + i % 5, 1, 1, c), 8) for i, c in enumerate(ROW_C)]
COL_LENGTHS = (1, 7, 8, 9, 33)
COL_CS = (1, 4, 12, 13)


def col_shape(mask, a, c):
    return {1: (a, 2, 3, c), 2: (2, a, 3, c), 4: (2, 3, a, c), 6: (2, a, 3, c), 7: (a, 2, 3, c)}[mask]


COL_CASES = [(col_shape(m, a, c), m) for m in (1, 2, 4, 6, 7) for a in COL_LENGTHS for c in COL_CS]
ALL_CASES = ROW_CASES + COL_CASES
SEEN = set()
WORST = {}


def run(x, p, axes, normalize=False, eps=0.0, **views):
    y = hipops.lpnorm(x, p, axes, normalize, eps, **views)
    return y, hipops.LAST_KERNEL_NAME["si_hip_lpnorm"]


@functools.lru_cache(maxsize=None)
def data(shape, dt, seed=41):
    x = lr.ranged(shape, seed, DTYPES[dt])
    x.setflags(write=False)
    return x


def same_bits(got, want, what):
    """bit for bit where the expected value is a number, NaN where it is NaN (a NaN's payload is not part of the contract)"""
    assert got.shape == want.shape and got.dtype == want.dtype, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what + ": NaN masks differ"
    ct.assert_same_bits(np.where(nan, 0, got).astype(got.dtype), np.where(nan, 0, want).astype(want.dtype), what)


def check(x, p, axes, normalize, eps=1e-12, what=""):
    """the device against the float32 restatement, bit for bit, and against float64 within the derived bar"""
    dt = "f32" if x.dtype == np.float32 else "f16"
    got, kernel = run(x, p, axes, normalize, eps)
    SEEN.add(kernel)
    what = "%s p=%s %s mask %d normalize=%d %s [%s]" % (what, p, x.shape, axes, normalize, dt, kernel)
    assert got.dtype == x.dtype and got.shape == lr.out_shape(x.shape, axes, normalize), what
    assert kernel == lr.expected_kernel(x.shape, axes, x.dtype, normalize), what
    same_bits(got, lr.lpnorm_f32(x, p, axes, normalize, eps), what)
    want = lr.lpnorm_ref(x, p, axes, normalize, eps)
    keep = np.abs(want) <= 65504.0 if x.dtype == np.float16 else np.ones(want.shape, bool)
    rel, absolute = lr.bar(x.shape, axes, p, x.dtype, kernel.endswith(("4>", "8>")), normalize)
    w = lr.check_bar(got[keep], want[keep], rel, absolute)
    key = (kernel.split("<")[0], dt, p, normalize)
    WORST[key] = max(WORST.get(key, 0.0), w)
    return got


# ---- 1. bit for bit against the restatement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,axes", ROW_CASES, ids=["c%d_x%d" % (s[3], s[0]) for s, _ in ROW_CASES])
def test_row_forms_bit_for_bit(gpu, shape, axes):
    for dt in sorted(DTYPES):
        for p in lr.PS:
            for normalize in (False, True):
                check(data(shape, dt), p, axes, normalize)


@pytest.mark.parametrize("mask", (1, 2, 4, 6, 7))
@pytest.mark.parametrize("length", COL_LENGTHS)
def test_col_lane_bit_for_bit(gpu, mask, length):
    for c in COL_CS:
        shape = col_shape(mask, length, c)
        for dt in sorted(DTYPES):
            for p in lr.PS:
                for normalize in ((False, True) if mask in SINGLE else (False,)):
                    check(data(shape, dt), p, mask, normalize)


ALL_KERNELS = {lr.kname(f, d, v) for f in ("row_group", "row_block", "row_block_2pass", "col_lane", "col_lane_reg") for d in DTYPES.values()
               for v in (True, False)}


def test_every_kernel_ran_and_the_worst_errors(gpu):
    """(runs after the parametrised tests above, whose names it collects; alone it runs one case per kernel)"""
    if not ALL_KERNELS <= SEEN:
        for shape, axes in [((2, 1, 1, 64), 8), ((2, 1, 1, 65), 8), ((2, 1, 1, G + 8), 8), ((2, 1, 1, G + 1), 8), ((2, 1, 1, B + 8), 8),
                            ((2, 1, 1, B + 1), 8), ((2, 9, 3, 8), 2), ((2, 9, 3, 13), 2), ((2, 7, 3, 8), 2), ((2, 7, 3, 13), 2)]:
            for dt in sorted(DTYPES):
                for normalize in (False, True):
                    check(data(shape, dt), 2, axes, normalize)
    assert ALL_KERNELS <= SEEN, sorted(ALL_KERNELS - SEEN)
    for key in sorted(WORST, key=str):
        print("%s vs float64: worst relative error %.3e" % (key, WORST[key]))


# ---- 2. exact by construction ------------------------------------------------------------------------------------------------------------------
def pythagorean_rows(c):
    """integer rows of c elements built from a blocks (3, 4) and b blocks (8, 15): the sum of squares 25 a + 289 b is a perfect square below 2^24,
    so every partial sum is exact in float32 in any order and the norm is an integer; signs alternate, the blocks are spread over the row"""
    rows, norms = [], []
    for a, b, n in ((1, 0, 5), (0, 1, 17), (4, 0, 10), (9, 0, 15), (16, 0, 20), (0, 4, 34), (32, 1, 33)):
        v = [3, -4] * a + [-8, 15] * b
        if len(v) > c:
            continue
        row = np.zeros(c)
        row[np.linspace(0, c - 1, len(v)).astype(int)] = v
        assert (row * row).sum() == n * n
        rows.append(row)
        norms.append(n)
    return np.array(rows).reshape(len(rows), 1, 1, c), np.array(norms, np.float64).reshape(-1, 1, 1, 1)


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_exact_norms_of_pythagorean_rows(gpu, dt):
    for c in (2, 8, 65, 72, G + 8, B + 1):
        x, norms = pythagorean_rows(c)
        x = x.astype(DTYPES[dt])
        got, kernel = run(x, 2, 8)
        ct.assert_same_bits(got, norms.astype(x.dtype), "p=2 norm of 3-4-5 / 8-15-17 rows, c=%d [%s]" % (c, kernel))
        got1, _ = run(x, 1, 8)
        ct.assert_same_bits(got1, np.abs(x.astype(np.float64)).sum(axis=3, keepdims=True).astype(x.dtype), "p=1 of integers, c=%d" % c)
        # the same rows as columns: every channel a set over h
        xt = np.ascontiguousarray(x.reshape(1, x.shape[0], c, 1).transpose(0, 2, 3, 1))   # [1, c, 1, rows]
        gt, _ = run(xt, 2, 2)
        ct.assert_same_bits(gt.reshape(-1), norms.astype(x.dtype).reshape(-1), "p=2 norm over h, %d positions" % c)


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_normalize_exact_for_power_of_two_norms_and_for_p_inf(gpu, dt):
    dtype = DTYPES[dt]
    # rows whose sum of squares is 64: the norm is 8, the division exact, so the result is float64's rounded once (here: not rounded at all)
    pats = [[3] * 7 + [1], [5, 5, 3, 1, 1, 1, 1, 1], [7, 3, 2, 1, 1], [1] * 64, [4, 4, 4, 4], [8]]
    for c in (64, 65, G + 8):
        x = np.zeros((len(pats), 1, 1, c))
        for i, v in enumerate(pats):
            x[i, 0, 0, np.linspace(0, c - 1, len(v)).astype(int)] = np.array(v) * (-1.0) ** np.arange(len(v))
        x = x.astype(dtype)
        got, kernel = run(x, 2, 8, True, 1e-12)
        ct.assert_same_bits(got, (x.astype(np.float64) / 8.0).astype(dtype), "normalize by a norm of 8, c=%d [%s]" % (c, kernel))
    # p = inf: one IEEE division of two numbers of the type; through float64 it rounds to the same value (53 >= 2 * 24 + 2)
    for shape, axes in (((5, 1, 1, 64), 8), ((3, 1, 1, 13), 8), ((2, 1, 1, B + 8), 8), ((2, 7, 3, 8), 2), ((2, 3, 33, 13), 4)):
        x = data(shape, dt, seed=5)
        got, kernel = run(x, INF, axes, True, 0.0)
        x64 = x.astype(np.float64)
        want = x64 / np.abs(x64).max(axis=lr.mask_axes(axes), keepdims=True)
        ct.assert_same_bits(got, want.astype(dtype), "p=inf normalize vs float64 rounded once, %s [%s]" % (shape, kernel))
        assert np.abs(got.astype(np.float64)).max(axis=lr.mask_axes(axes)).min() == 1.0


# ---- 3. special values ---------------------------------------------------------------------------------------------------------------------
def special_rows(dtype):
    x = np.array(data((8, 1, 1, 8), "f32" if dtype == np.float32 else "f16", seed=3))
    x[0, 0, 0, 5] = np.nan                       # a NaN: its own set only
    x[1, 0, 0, 2] = np.inf                       # +inf
    x[2, 0, 0, 6] = -np.inf                      # -inf
    x[2, 0, 0, 1] = np.inf
    x[3] = 0.0                                   # a zero set, one element -0.0
    x[3, 0, 0, 4] = -0.0
    x[4] = np.array([1, -2, 3, -4, 1, 1, 1, 1]) * 2.0 ** -14   # a norm below eps = 1e-3
    if dtype == np.float32:
        x[5, 0, 0, 0], x[5, 0, 0, 3] = 3e19, -1e-30              # a square that overflows; a tiny one that underflows to 0
    return x


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_special_values(gpu, dt):
    x = special_rows(DTYPES[dt])
    cols = np.ascontiguousarray(x.reshape(1, 8, 8, 1).transpose(0, 2, 3, 1))   # [1, 8 positions, 1, 8 sets]
    for p in lr.PS:
        for eps in (1e-3, 0.0):
            got, kernel = run(x, p, 8, True, eps)
            same_bits(got, lr.lpnorm_f32(x, p, 8, True, eps), "special rows p=%s eps=%g [%s]" % (p, eps, kernel))
            g = got.astype(np.float64).reshape(8, 8)
            assert np.isnan(g[0]).all() and not np.isnan(g[6:]).any()                      # the NaN's set, and no other
            assert np.isnan(g[1, 2]) and (np.delete(g[1], 2) == 0).all()                  # inf / inf, finite / inf
            assert np.array_equal(np.signbit(np.delete(g[1], 2)), np.signbit(np.delete(x[1, 0, 0], 2)))
            assert np.isnan(g[2, [1, 6]]).all() and (np.delete(g[2], [1, 6]) == 0).all()
            if eps > 0:
                assert (g[3] == 0).all() and np.signbit(g[3, 4]) and not np.signbit(g[3, 0])   # 0 / eps, the sign kept
                assert np.array_equal(got[4], (x[4].astype(np.float32) / np.float32(eps)).astype(x.dtype))   # the clamp binds
            else:
                assert np.isnan(g[3]).all()                                                 # 0 / 0
            if dt == "f32" and p == 2:
                assert (g[5] == 0).all()                                                    # the norm is +inf
            n, _ = run(x, p, 8)
            same_bits(n, lr.lpnorm_f32(x, p, 8), "special rows, the norm, p=%s" % p)
            assert np.isnan(n[0, 0, 0, 0]) and np.isinf(n[1, 0, 0, 0]) and n[3, 0, 0, 0] == 0 and np.isfinite(n[6:].astype(np.float64)).all()
            if dt == "f32":
                assert np.isinf(n[5, 0, 0, 0]) == (p == 2)
            for normalize in (False, True):
                gc, kc = run(cols, p, 2, normalize, eps)
                same_bits(gc, lr.lpnorm_f32(cols, p, 2, normalize, eps), "special columns p=%s normalize=%d [%s]" % (p, normalize, kc))


def test_every_finite_half(gpu):
    bits = np.arange(1 << 16, dtype=np.uint16)
    h = bits.view(np.float16)
    x = h[np.isfinite(h)].reshape(-1, 1, 1, 8)
    assert x.shape[0] == 63488 // 8
    for p in lr.PS:
        for normalize in (False, True):
            got, kernel = run(x, p, 8, normalize, 1e-12)
            assert kernel == lr.kname("row_group", np.float16, True)
            same_bits(got, lr.lpnorm_f32(x, p, 8, normalize, 1e-12), "every finite half, p=%s normalize=%d" % (p, normalize))


# ---- 4. invariants ---------------------------------------------------------------------------------------------------------------------------
INVARIANT_CASES = [((3, 4, 5, 8), 8), ((3, 1, 1, G + 8), 8), ((3, 1, 1, B + 1), 8), ((3, 9, 5, 8), 2), ((3, 4, 7, 6), 4), ((3, 5, 5, 8), 6)]


@pytest.mark.parametrize("shape,axes", INVARIANT_CASES, ids=["%s_mask%d" % ("x".join(map(str, s)), a) for s, a in INVARIANT_CASES])
def test_same_bits_twice_per_image_and_per_set(gpu, shape, axes):
    for dt in sorted(DTYPES):
        x = data(shape, dt, seed=7)
        for normalize in ((False, True) if axes in SINGLE else (False,)):
            y3, k3 = run(x, 2, axes, normalize, 1e-12)
            ct.assert_same_bits(y3, run(x, 2, axes, normalize, 1e-12)[0], "two launches")
            y1, k1 = run(x[1:2], 2, axes, normalize, 1e-12)
            assert k1 == k3, (k1, k3)
            ct.assert_same_bits(y3[1:2], y1, "image 1 of 3")
            # set independence: image 0 changes (a NaN among the changes), the sets of images 1 and 2 keep their bits
            z = np.array(x)
            z[0] = -z[0] * 3
            z[0, 0, 0, 0] = np.nan
            yz, _ = run(z, 2, axes, normalize, 1e-12)
            ct.assert_same_bits(yz[1:], y3[1:], "other sets after image 0 changed")
            assert np.isnan(yz[0].astype(np.float64)).any() and not np.isnan(yz[1:].astype(np.float64)).any()


GRID_CASES = [
    # the capped grid is 2048 workgroups; each case needs a third pass for its last sets
    ("row_group", (2 * 2048 * 256 + 5, 1, 1, 4), 8, "f32"),      # one lane per row, 256 rows per workgroup
    ("row_block", (2 * 2048 + 5, 1, 1, G + 8), 8, "f16"),        # one workgroup per row
    ("row_block_2pass", (2 * 2048 + 5, 1, 1, B + 8), 8, "f16"),
    ("col_lane", (1, 2, 2 * 2048 * 256 + 5, 1), 2, "f32"),       # one lane per kept pixel
]


@pytest.mark.parametrize("form,shape,axes,dt", GRID_CASES, ids=[c[0] for c in GRID_CASES])
def test_three_passes_of_the_grid_stride_loop(gpu, form, shape, axes, dt):
    x = data(shape, dt, seed=13)
    for normalize in (False, True):
        got, kernel = run(x, 2, axes, normalize, 1e-12)
        assert kernel.startswith("lpnorm_" + form), kernel
        same_bits(got, lr.lpnorm_f32(x, 2, axes, normalize, 1e-12), "%s over three passes, normalize=%d [%s]" % (form, normalize, kernel))


# ---- 5. views and containment: checks (a) - (d) of tests/test_gpu_containment.py --------------------------------------------------------------
class ViewCase:
    def __init__(self, vid, half, shape, axes, p, normalize, form, vec, **views):
        self.id, self.half, self.shape, self.axes, self.p, self.normalize, self.form, self.vec, self.views = vid, half, shape, axes, p, normalize, form, vec, views
        self.entries = ("si_hip_lpnorm_f16" if half else "si_hip_lpnorm_f32",)
        self.dt = "f16" if half else "f32"
        self.dtype = DTYPES[self.dt]
        self.oc = shape[3] if normalize or not axes & 8 else 1

    def input(self):
        return data(self.shape, self.dt)

    def run(self, F):
        y, _ = run(self.input(), self.p, self.axes, self.normalize, 1e-12, in_fill=F, out_fill=F, full=True, **self.views)
        return ct.Out("y", y, self.views.get("out_c_off", 0), self.oc)


VIEW_CASES = []
for _half, _sfx, _v in ((False, "f32", 4), (True, "f16", 8)):
    VIEW_CASES += [
        # 16-byte aligned on both sides, ld > c on both sides
        ViewCase("row_group_norm_vector_" + _sfx, _half, (2, 5, 7, 8), 8, 2, False, "row_group", True, in_ld=24, in_c_off=8, out_ld=3, out_c_off=1),
        ViewCase("row_group_normalize_vector_" + _sfx, _half, (2, 5, 7, 8), 8, 2, True, "row_group", True, in_ld=24, in_c_off=8, out_ld=32, out_c_off=16),
        ViewCase("row_block_normalize_vector_" + _sfx, _half, (3, 1, 1, G + 8), 8, 1, True, "row_block", True, in_ld=G + 24, in_c_off=8, out_ld=G + 16, out_c_off=8),
        ViewCase("row_block_2pass_normalize_vector_" + _sfx, _half, (2, 1, 1, B + 8), 8, INF, True, "row_block_2pass", True, in_ld=B + 24, in_c_off=16, out_ld=B + 16, out_c_off=0),
        ViewCase("col_lane_norm_vector_hw_" + _sfx, _half, (2, 5, 6, 8), 6, 2, False, "col_lane", True, in_ld=24, in_c_off=8, out_ld=32, out_c_off=16),
        ViewCase("col_lane_normalize_vector_h_" + _sfx, _half, (2, 9, 3, 8), 2, 2, True, "col_lane", True, in_ld=16, in_c_off=8, out_ld=24, out_c_off=8),
        ViewCase("col_lane_reg_vector_w_" + _sfx, _half, (2, 3, 7, 8), 4, 1, True, "col_lane_reg", True, in_ld=24, in_c_off=16, out_ld=16, out_c_off=8),
        # odd offsets and strides
        ViewCase("row_group_normalize_scalar_" + _sfx, _half, (2, 5, 7, 6), 8, 2, True, "row_group", False, in_ld=9, in_c_off=2, out_ld=11, out_c_off=5),
        ViewCase("row_block_norm_scalar_" + _sfx, _half, (3, 1, 1, G + 1), 8, 2, False, "row_block", False, in_ld=G + 4, in_c_off=3, out_ld=3, out_c_off=0),
        ViewCase("row_block_2pass_norm_scalar_" + _sfx, _half, (2, 1, 1, B + 1), 8, 1, False, "row_block_2pass", False, in_ld=B + 4, in_c_off=3, out_ld=2, out_c_off=1),
        ViewCase("col_lane_normalize_scalar_n_" + _sfx, _half, (9, 2, 3, 6), 1, INF, True, "col_lane", False, in_ld=9, in_c_off=2, out_ld=7, out_c_off=1),
        ViewCase("col_lane_reg_scalar_h_" + _sfx, _half, (2, 5, 7, 6), 2, 2, True, "col_lane_reg", False, in_ld=8, in_c_off=1, out_ld=7, out_c_off=1),
        # vector-sized channels and strides behind a pointer that is 8 bytes off a 16-byte boundary: the scalar instantiation
        ViewCase("row_group_unaligned_in_" + _sfx, _half, (2, 5, 7, 8), 8, 2, True, "row_group", False, in_ld=16, in_c_off=_v // 2, out_ld=8, out_c_off=0),
        ViewCase("row_group_unaligned_out_" + _sfx, _half, (2, 5, 7, 8), 8, 2, True, "row_group", False, in_ld=16, in_c_off=0, out_ld=16, out_c_off=_v // 2),
        ViewCase("col_lane_unaligned_out_" + _sfx, _half, (2, 5, 6, 8), 6, 2, False, "col_lane", False, in_ld=16, in_c_off=0, out_ld=24, out_c_off=_v // 2),
        # the input slice ends where its buffer ends
        ViewCase("row_group_last_slice_" + _sfx, _half, (2, 5, 7, 6), 8, 2, False, "row_group", False, in_ld=14, in_c_off=8, out_ld=1, out_c_off=0),
    ]


def test_view_cases_cover_the_forms():
    assert {(c.form, c.vec, c.half) for c in VIEW_CASES} >= {(f, v, h) for f in ("row_group", "row_block", "row_block_2pass", "col_lane", "col_lane_reg")
                                                             for v in (True, False) for h in (True, False)}
    assert {c.p for c in VIEW_CASES} == set(lr.PS) and {c.normalize for c in VIEW_CASES} == {False, True}
    for c in VIEW_CASES:
        assert lr.expected_form(c.shape, c.axes, c.normalize) == c.form, c.id
        assert lr.vectorised(c.shape, c.axes, c.dtype, c.normalize, **c.views) == c.vec, c.id
        assert c.views["in_ld"] > c.shape[3], c.id
    assert any(c.shape[3] % (16 // np.dtype(c.dtype).itemsize) == 0 and not c.vec for c in VIEW_CASES)   # the misaligned base pointer


@pytest.mark.parametrize("case", VIEW_CASES, ids=[c.id for c in VIEW_CASES])
def test_views_and_containment(gpu, case):
    del hipops.LAST_ENTRIES[:]
    plain = case.run(hipops.ByteFill(0x00))
    plain_kernel = hipops.LAST_KERNEL_NAME["si_hip_lpnorm"]
    assert set(case.entries) <= set(hipops.LAST_ENTRIES), hipops.LAST_ENTRIES
    assert plain_kernel == lr.kname(case.form, case.dtype, case.vec), plain_kernel
    ct.assert_outside_fill(plain.full, plain.c_off, plain.c, 0x00, case.id + ", plain run")
    # the value too: nothing of the gaps between the input's pixels reached the output -- the restatement of the same instantiation
    want = lr.lpnorm_f32(case.input(), case.p, case.axes, case.normalize, 1e-12, vec=case.vec)
    same_bits(np.ascontiguousarray(plain.dest), want, case.id + " vs the restatement")
    for byte in ct.PATTERNS:
        with hipops.guard_bands(byte) as g:      # (a) all bands and (d) the input are compared when the block ends
            out = case.run(hipops.ByteFill(byte))
        what = "%s under 0x%02X" % (case.id, byte)
        assert g.checked == 2, "%s: the guard saw %d buffers" % (what, g.checked)   # x, y
        assert hipops.LAST_KERNEL_NAME["si_hip_lpnorm"] == plain_kernel, what
        ct.assert_outside_fill(out.full, out.c_off, out.c, byte, what)                              # (b)
        ct.assert_same_bits(out.dest, plain.dest, what + ": guarded + pattern-filled vs plain")    # (c)


# ---- engine helpers --------------------------------------------------------------------------------------------------------------------------
def save(b, tmp_path, tag="m"):
    pp, bp = str(tmp_path / (tag + ".pnnx.param")), str(tmp_path / (tag + ".pnnx.bin"))
    b.save(pp, bp)
    return pp, bp


def run_engine(pp, bp, x, **opts):
    """the engine and the list of its graph outputs, in the engine's layout"""
    e = Engine(**opts)
    e.load_model(pp, bp)
    e.input(e.input_names()[0], x)
    e.forward()
    return e, [e.extract(n) for n in e.output_names()]


def one_op_graph(typ, shape_file, dim, **kw):
    """input -> one operator -> output, for the file's (NCHW or [N, F]) shape"""
    b = mg.PnnxBuilder(seed=5)
    x = b.input(shape_file)
    b.output(b.normalize(x, dim, **kw) if typ == "F.normalize" else b.norm(x, dim, **kw))
    return b


def nhwc_of(a):
    """a file-order array (NCHW, [N, H, W], [N, F]) as the engine holds it"""
    return np.ascontiguousarray(a.transpose(0, 2, 3, 1)) if a.ndim == 4 else a


def lpnorm_layers(prof):
    return [L for L in prof if L["type"] in lr.LPNORM_TYPES]


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_leave_the_process_usable(gpu, tmp_path):
    x = np.array(data((2, 5, 7, 8), "f32"))
    H = _native.hip()
    fill = np.full(x.shape, 7.25, np.float32)
    src, dst = hipops.DeviceBuffer.from_numpy(x), hipops.DeviceBuffer.from_numpy(fill, out=True)
    desc = hipops.lpnorm_desc

    def entry(d, fn="si_hip_lpnorm_f32", a=None, b=None):
        return getattr(H, fn)(C.byref(d), src.ptr if a is None else a, dst.ptr if b is None else b, None)

    bad_p = desc(x.shape, 2, 8)
    bad_p.p = 3
    codes = [entry(bad_p), entry(desc(x.shape, 2, 16)), entry(desc(x.shape, 2, 8, in_ld=7)), entry(desc(x.shape, 2, 8, True, -1.0)),
             entry(desc(x.shape, 2, 6, True)), entry(desc(x.shape, 2, 8, True), b=src.ptr), entry(desc(x.shape, 2, 6), a=C.c_void_p(None)),
             entry(desc(x.shape, 2, 6), fn="si_hip_lpnorm_f16", b=C.c_void_p(None))]
    assert codes == [-1] * len(codes), codes
    codes = [entry(desc(x.shape, 2, m)) for m in (9, 10, 12, 15)] + [entry(desc((1, 16384, 16384, 8), 2, 8))]
    assert codes == [-2] * len(codes), codes
    ct.assert_same_bits(dst.to_numpy(x.shape, np.float32), fill, "the output buffer keeps its fill")
    with pytest.raises(hipops.HipError):
        hipops.lpnorm(x, 2, 9)

    def load(b, tag):
        pp, bp = save(b, tmp_path, tag)
        with pytest.raises(StatusError) as ei:
            Engine().load_model(pp, bp)
        return ei.value.status

    # refused at LoadModel, with the reason in the log, not at the first Forward
    assert load(one_op_graph("F.normalize", (2, 6, 5, 7), 1, p=3.0), "p3") == Status.kUnsupport
    assert load(one_op_graph("torch.norm", (2, 6, 5, 7), 1, p=0, keepdim=True), "p0") == Status.kUnsupport
    assert load(one_op_graph("torch.norm", (2, 6, 5, 7), 1, p="nuc", keepdim=True), "nuc") == Status.kUnsupport
    assert load(one_op_graph("torch.norm", (2, 6, 5, 7), 1, p=-INF, keepdim=True), "minus_inf") == Status.kUnsupport
    b = one_op_graph("torch.norm", (2, 6, 5, 7), (2, 3), keepdim=True)
    b.lines = [ln.replace(" dim=(2,3) ", " ") for ln in b.lines]
    assert " dim=" not in b.lines[1] and load(b, "no_dim") == Status.kUnsupport                  # the reduction to a scalar
    b = one_op_graph("torch.norm", (2, 6, 5, 7), 1, keepdim=True)
    b.lines = [ln.replace(" p=2 ", " p=2 dtype=torch.float ") for ln in b.lines]
    assert "dtype=torch.float" in b.lines[1] and load(b, "dtype") == Status.kUnsupport
    assert load(one_op_graph("F.normalize", (2, 6, 5), 1), "rank3") == Status.kUnsupport
    assert load(one_op_graph("torch.norm", (2, 6, 5), 2, keepdim=True), "rank3_norm") == Status.kUnsupport
    assert load(one_op_graph("torch.norm", (2, 6, 5, 7), 2, keepdim=False), "keepdim_false_dim2") == Status.kUnsupport
    assert load(one_op_graph("torch.norm", (3, 10), 1, keepdim=False), "rank1_result") == Status.kUnsupport
    assert load(one_op_graph("torch.norm", (2, 6, 5, 7), (1, 2), keepdim=True), "mixed_mask") == Status.kUnsupport
    assert load(one_op_graph("F.normalize", (2, 6, 5, 7), 4), "dim4") == Status.kUnsupport
    b = one_op_graph("torch.norm", (2, 6, 5, 7), (2, 3), keepdim=True)
    b.lines = [ln.replace("(2,6,1,1)f32", "(2,6,1,5)f32") for ln in b.lines]
    assert "(2,6,1,5)f32" in b.lines[1] and load(b, "wrong_shape") == Status.kErrorShape        # the file's output shape is not the rule's
    b = one_op_graph("F.normalize", (2, 6, 5, 7), 1)
    b.lines = [ln.replace(" dim=1 ", " dim=1.5 ") for ln in b.lines]
    assert "dim=1.5" in b.lines[1] and load(b, "float_dim") == Status.kFail                      # a mistyped key
    b = one_op_graph("torch.norm", (2, 6, 5, 7), 1, keepdim=True)
    b.lines = [ln.replace(" keepdim=True ", " keepdim=1 ") for ln in b.lines]
    assert "keepdim=1 " in b.lines[1] and load(b, "int_keepdim") == Status.kFail
    # ... and the same process launches, loads and runs afterwards
    same_bits(run(x, 2, 6)[0], lr.lpnorm_f32(x, 2, 6), "good launch after the refusals")
    pp, bp = save(one_op_graph("F.normalize", (2, 8, 5, 7), 1), tmp_path, "good")
    _, (out,) = run_engine(pp, bp, x)
    ct.assert_same_bits(out, hipops.lpnorm(x, 2, 8, True, 1e-12), "good model after the refusals")


# ---- 7. the layers against the op-level call ---------------------------------------------------------------------------------------------------
ONE_OP = [("F.normalize", (2, 8, 5, 7), dim, dict(p=p)) for dim in (1, -3, 2, 3, 0) for p in (2.0, 1.0, INF)]
ONE_OP += [("F.normalize", (2, 6, 5, 7), 1, dict(p=2.0, eps=0.5)), ("F.normalize", (3, 10), 1, dict()), ("F.normalize", (3, 24), -1, dict(p=1.0)),
           ("F.normalize", (9, 10), 0, dict(p=INF)), ("F.normalize", (3, G + 8), 1, dict()), ("F.normalize", (2, B + 8), 1, dict())]
ONE_OP += [("torch.norm", (2, 8, 5, 7), dim, dict(p=p, keepdim=True)) for dim in (1, (1,), 2, (2, 3), (0, 2, 3), 0, -1) for p in (2, 1.0, INF)]
ONE_OP += [("torch.norm", (2, 8, 5, 7), 1, dict(p=2, keepdim=False)), ("torch.norm", (2, 6, 5, 7), -3, dict(p=INF, keepdim=False)),
           ("torch.norm", (2, 8, 5, 7), (2, 3), dict(p="fro", keepdim=False)), ("torch.norm", (2, 8, 5, 7), (-1, -2), dict(p=1, keepdim=False)),
           ("torch.norm", (3, 10), 1, dict(p=2.0, keepdim=True)), ("torch.norm", (3, 10), 0, dict(p=1, keepdim=True))]


def _one_op_id(t, s, d, kw):
    return "%s_%s_dim%s_%s" % (t, "x".join(map(str, s)), "_".join(map(str, d)) if isinstance(d, tuple) else d,
                               "_".join("%s%s" % (k[0], v) for k, v in sorted(kw.items())))


@pytest.mark.parametrize("typ,shape_file,dim,kw", ONE_OP, ids=[_one_op_id(*c) for c in ONE_OP])
def test_engine_one_op_graph(gpu, tmp_path, typ, shape_file, dim, kw):
    """LoadModel -> Forward -> Extract reproduces the op-level result bit for bit, and the torch float64 evaluation of the file within the bar"""
    b = one_op_graph(typ, shape_file, dim, **kw)
    assert _parse(b.lines[1])[0] == typ
    pp, bp = save(b, tmp_path)
    rank = len(shape_file)
    x = lr.ranged((shape_file[0], shape_file[2], shape_file[3], shape_file[1]) if rank == 4 else shape_file, 9)
    e, (got,) = run_engine(pp, bp, x)
    axes = lr.nhwc_mask(dim, rank)
    x4 = x if rank == 4 else x.reshape(x.shape[0], 1, 1, x.shape[1])
    p = {"fro": 2}.get(kw.get("p", 2.0), kw.get("p", 2.0))
    normalize = typ == "F.normalize"
    op_level, kernel = run(x4, p, axes, normalize, kw.get("eps", 1e-12) if normalize else 0.0)
    ct.assert_same_bits(got, op_level.reshape(got.shape), "engine vs op level")
    (ref,) = lr.eval_graph(b, x)
    ref = nhwc_of(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    rel, _ = lr.bar(x4.shape, axes, p, np.float32, kernel.endswith("4>"), normalize)
    print("%s: worst relative error %.3e (bar %.3e)" % (_one_op_id(typ, shape_file, dim, kw), lr.check_bar(got, ref, rel), rel))
    layers = lpnorm_layers(e.profile())
    assert len(layers) == 1 and layers[0]["type"] == typ and layers[0]["kernel"] == kernel == lr.expected_kernel(x4.shape, axes, np.float32, normalize), layers


def test_norm_reads_a_channel_slice_and_normalize_writes_into_a_concat(gpu, tmp_path):
    """the kernels honour ld on both sides: F.normalize reads the second half of a chunk (a view at a pixel stride of 16) and writes channels
    0 .. 7 of a concat; torch.norm reads the first half"""
    b = mg.PnnxBuilder(seed=7)
    x = b.input((2, 4, 9, 11))
    f = b.relu(b.conv(x, 16, 3, 1, 1))
    lo, hi = b.chunk(f, 2, 1)
    u = b.normalize(hi, 1)
    n = b.norm(lo, 1, 2, True)
    y = b.conv(b.cat([u, b.relu(b.conv(f, 8, 1))]), 8, 1)
    b.output(b.conv(b.div(y, n), 4, 1))
    pp, bp = save(b, tmp_path)
    xin = util.rng_uniform(15, (2, 9, 11, 4), -1.0, 1.0)
    e, (got,) = run_engine(pp, bp, xin)
    alias = e.schedule()["alias"]
    assert all(any(o in ln.split() for ln in alias) for o in (lo, hi, u)), e.schedule()
    assert [L["kernel"] for L in lpnorm_layers(e.profile())] == [lr.kname("row_group", np.float32, True)] * 2
    # the same graph with nothing aliased computes the same bits
    _, (plain,) = run_engine(pp, bp, xin, alias_cat=0, alias_split=0)
    ct.assert_same_bits(got, plain, "views vs copies")
    _, (g,) = run_engine(pp, bp, xin, graph=1)
    ct.assert_same_bits(g, got, "graph=1 vs eager")


# ---- 8. the toys -----------------------------------------------------------------------------------------------------------------------------
TOYS = {
    "superpoint": (lambda: mg.build_toy_superpoint(), (2, 32, 32, 1)),
    "superpoint_functional": (lambda: mg.build_toy_superpoint(functional=True), (2, 32, 32, 1)),
    "embedding_head": (lambda: mg.build_toy_embedding_head(), (2, 32, 32, 3)),
}


def unit_rows(desc, dtype_bar):
    """| ||row|| - 1 | of a normalised [.., C] output (the channel axis last, as the engine holds it)"""
    n = np.sqrt((desc.astype(np.float64) ** 2).sum(axis=-1))
    worst = np.abs(n - 1.0).max()
    assert worst <= dtype_bar, (worst, dtype_bar)
    return worst


@pytest.mark.parametrize("toy", sorted(TOYS))
def test_toy_model_fp32(gpu, tmp_path, toy):
    build, s = TOYS[toy]
    b = build()
    pp, bp = save(b, tmp_path)
    x = mg.synth_input(s)
    e, got = run_engine(pp, bp, x)
    ref = [nhwc_of(r) for r in lr.eval_graph(b, x)]
    assert len(got) == len(ref) == (1 if toy == "embedding_head" else 2)
    for k, (g, r) in enumerate(zip(got, ref)):
        print("toy %s fp32, output %d: max-based %.3e, element-wise %.3e" % (toy, k, util.rel_err(g, r), util.mixed_err(g, r)))
        util.assert_parity(g, r, what="toy %s fp32, output %d" % (toy, k))
    # the normalised output has unit rows: the norm's own bound (A + 3) u, one rounding per element for the division, in float32
    c = got[-1].shape[-1]
    a = lr.chain_length((1, 1, 1, c), 8, np.float32, c % 4 == 0, True)
    print("toy %s fp32: | ||row|| - 1 | <= %.3e (bar %.3e)" % (toy, unit_rows(got[-1], (a + 5) * lr.U), (a + 5) * lr.U))
    layers = lpnorm_layers(e.profile())
    assert [L["kernel"] for L in layers] == [lr.kname("row_group", np.float32, True)], layers
    # a captured graph replays the same bits, three forwards
    eg = Engine(graph=1)
    eg.load_model(pp, bp)
    for _ in range(3):
        eg.input(eg.input_names()[0], x)
        eg.forward()
        for k, n in enumerate(eg.output_names()):
            ct.assert_same_bits(eg.extract(n), got[k], "graph=1 vs eager, output %d" % k)


def test_superpoint_written_out_norm_is_one_launch(gpu, tmp_path):
    """fuse_norm: torch.norm -> torch.unsqueeze -> BinaryOp div is ONE lpnorm launch with normalize = 1, eps = 0 that writes no norm; the
    unsqueeze and the division (the BinaryOp div_<k> the expression lowers to) are reported under `fused`.  fuse_norm = 0 runs the three steps; in fp32 both plans divide by the same
    float32 norm with the IEEE division, so the bits are the same.  The functional spelling (eps = 1e-12 does not bind) has them too."""
    b = mg.build_toy_superpoint()
    pp, bp = save(b, tmp_path, "written")
    x = mg.synth_input((2, 32, 32, 1))
    e1, fused = run_engine(pp, bp, x)
    e0, plain = run_engine(pp, bp, x, fuse_norm=0)
    for k in range(2):
        ct.assert_same_bits(fused[k], plain[k], "fuse_norm 1 vs 0, output %d" % k)
    s1, s0 = e1.schedule(), e0.schedule()
    in_list = lambda name, lines: any(name in ln.split() for ln in lines)
    assert in_list("torch_norm_0", s1["run"]) and not in_list("torch_unsqueeze_0", s1["run"]) and not any("div_" in ln for ln in s1["run"]), s1
    assert any("torch_unsqueeze_0" in ln for ln in s1["fused"]) and any("div_" in ln for ln in s1["fused"]), s1
    assert in_list("torch_norm_0", s0["run"]) and not any("torch_unsqueeze_0" in ln or "div_" in ln for ln in s0["fused"]), s0
    assert len(s1["run"]) + 2 == len(s0["run"]) or len(s1["run"]) + 1 == len(s0["run"]), (s1["run"], s0["run"])   # (the unsqueeze is a view: it may launch nothing)
    k1 = [L for L in e1.profile() if L["type"] == "torch.norm"]
    k0 = [L for L in e0.profile() if L["type"] == "torch.norm"]
    assert len(k1) == len(k0) == 1 and k1[0]["kernel"] == k0[0]["kernel"] == lr.kname("row_group", np.float32, True)
    assert k1[0]["bytes"] > 1.5 * k0[0]["bytes"]      # the fused launch writes the quotient, the unfused one the norm
    ppf, bpf = save(mg.build_toy_superpoint(functional=True), tmp_path, "functional")
    _, fn = run_engine(ppf, bpf, x)
    for k in range(2):
        ct.assert_same_bits(fn[k], fused[k], "F.normalize vs the written-out form, output %d" % k)
    # p = 1 and inf, and keepdim=True (no unsqueeze), fuse too
    for p, keep in ((1, False), (INF, True), (2, True)):
        g = mg.PnnxBuilder(seed=3)
        f = g.conv(g.input((2, 3, 6, 5)), 8, 3, 1, 1)
        n = g.norm(f, 1, p, keep)
        g.output(g.div(f, n if keep else g.unsqueeze(n, 1)))
        pq, bq = save(g, tmp_path, "p%s_%d" % (p, keep))
        xin = util.rng_uniform(4, (2, 6, 5, 3), -1.0, 1.0)
        ea, (ya,) = run_engine(pq, bq, xin)
        eb, (yb,) = run_engine(pq, bq, xin, fuse_norm=0)
        ct.assert_same_bits(ya, yb, "fuse_norm 1 vs 0, p=%s keepdim=%s" % (p, keep))
        assert len(ea.schedule()["fused"]) == len(eb.schedule()["fused"]) + (1 if keep else 2), (ea.schedule(), eb.schedule())


def test_a_norm_with_a_second_reader_is_not_fused(gpu, tmp_path):
    b = mg.PnnxBuilder(seed=3)
    f = b.conv(b.input((2, 3, 6, 5)), 8, 3, 1, 1)
    n = b.norm(f, 1, 2, True)
    b.output(b.div(f, n))
    b.output(n)                                  # the norm is a graph output as well
    pp, bp = save(b, tmp_path, "out")
    x = util.rng_uniform(4, (2, 6, 5, 3), -1.0, 1.0)
    e, outs = run_engine(pp, bp, x)
    q, nrm = sorted(outs, key=lambda a: -a.shape[-1])      # (the engine lists its outputs by name, not in file order)
    refs = [nhwc_of(r) for r in lr.eval_graph(b, x)]
    util.assert_parity(q, refs[0], what="quotient")
    util.assert_parity(nrm, refs[1], what="norm")
    assert not any("div_" in ln for ln in e.schedule()["fused"]), e.schedule()
    g = mg.PnnxBuilder(seed=3)
    f = g.conv(g.input((2, 3, 6, 5)), 8, 3, 1, 1)
    n = g.norm(f, 1, 2, True)
    g.output(g.conv(g.mul(g.div(f, n), n), 4, 1))   # two readers inside the graph
    pp, bp = save(g, tmp_path, "two")
    e, (y,) = run_engine(pp, bp, x)
    util.assert_parity(y, nhwc_of(lr.eval_graph(g, x)[0]), what="two readers")
    assert not any("div_" in ln for ln in e.schedule()["fused"]), e.schedule()
    # the divisor is the norm of ANOTHER tensor: not the pattern
    h = mg.PnnxBuilder(seed=3)
    f = h.conv(h.input((2, 3, 6, 5)), 8, 3, 1, 1)
    f2 = h.relu(f)
    h.output(h.div(f, h.norm(f2, 1, 2, True)))
    pp, bp = save(h, tmp_path, "other")
    e, (y,) = run_engine(pp, bp, x + 2.0)
    util.assert_parity(y, nhwc_of(lr.eval_graph(h, x + 2.0)[0]), what="norm of another tensor")
    assert not any("div_" in ln for ln in e.schedule()["fused"]), e.schedule()


@pytest.mark.parametrize("toy", sorted(TOYS))
def test_toy_model_rebatch_and_batch_split(gpu, tmp_path, toy):
    """SetOption("batch", 5) on the batch-2 file: per image the same bits as batch-2 runs of the same images; streams=2 cuts the batch in
    two lanes: the same bits as the unsplit run"""
    build, s = TOYS[toy]
    pp, bp = save(build(), tmp_path)
    x5 = util.rng_uniform(21, (5,) + s[1:], 0.0, 1.0)
    _, y5 = run_engine(pp, bp, x5, batch=5)
    xs = np.concatenate([x5, x5[:1]], 0)   # pairs (0, 1), (2, 3), (4, 0)
    for i in range(0, 6, 2):
        _, y2 = run_engine(pp, bp, xs[i:i + 2])
        for j in range(2):
            if i + j < 5:
                for k in range(len(y2)):
                    ct.assert_same_bits(y5[k][i + j], y2[k][j], "image %d, output %d" % (i + j, k))
    x4 = util.rng_uniform(22, (4,) + s[1:], 0.0, 1.0)
    e1, whole = run_engine(pp, bp, x4, batch=4)
    e2, split = run_engine(pp, bp, x4, batch=4, streams=2)
    assert not e2.schedule()["batch_mixing"], e2.schedule()
    for k in range(len(whole)):
        ct.assert_same_bits(split[k], whole[k], "streams=2 vs unsplit, output %d" % k)


@pytest.mark.parametrize("toy", sorted(TOYS))
def test_toy_model_fp16_storage(gpu, tmp_path, toy):
    """fp16=1: the result is within F16_TOL of the fp16-storage emulation; the unit rows hold within the norm's bound plus one half
    rounding.  (The half kernel inside the engine: test_cosine_head_runs_the_half_kernels_under_fp16_storage.)"""
    build, s = TOYS[toy]
    b = build()
    pp, bp = save(b, tmp_path)
    x = mg.synth_input(s)
    e, got = run_engine(pp, bp, x, fp16=1)
    ref = [nhwc_of(r) for r in lr.eval_graph(b, x)]
    emu = [nhwc_of(r) for r in lr.eval_graph(b, x, rnd=lr.round_f16, unstored=("torch.norm",))]   # (the fused plan stores no norm)
    for k in range(len(got)):
        print("toy %s fp16 storage, output %d: vs the emulation %.3e; vs fp64: engine %.3e, emulation %.3e" % (
            toy, k, util.rel_err(got[k], emu[k]), util.rel_err(got[k], ref[k]), util.rel_err(emu[k], ref[k])))
        assert np.isfinite(got[k]).all()
        util.assert_parity(got[k], emu[k], rel=F16_TOL, what="toy %s fp16 storage vs the emulation, output %d" % (toy, k))
    c = got[-1].shape[-1]
    a = lr.chain_length((1, 1, 1, c), 8, np.float16, c % 8 == 0, True)
    bar = (a + 5) * lr.U + 2.0 ** -11
    print("toy %s fp16 storage: | ||row|| - 1 | <= %.3e (bar %.3e)" % (toy, unit_rows(got[-1], bar), bar))
    # (the toys end in the normalisation: it writes halves, and the engine's output cast behind it makes the fp32 graph output)
    layers = lpnorm_layers(e.profile())
    assert len(layers) == 1 and layers[0]["kernel"] == lr.kname("row_group", np.float16, True), layers
    if toy == "superpoint":
        assert any("div_" in ln for ln in e.schedule()["fused"]), e.schedule()
        # the unfused plan rounds the norm to a half in between: only the float64 bar applies
        _, plain = run_engine(pp, bp, x, fp16=1, fuse_norm=0)
        stored = nhwc_of(lr.eval_graph(b, x, rnd=lr.round_f16)[-1])
        print("toy %s fp16 storage, fuse_norm=0: vs its emulation %.3e, vs fp64 %.3e" % (toy, util.rel_err(plain[-1], stored), util.rel_err(plain[-1], ref[-1])))
        util.assert_parity(plain[-1], stored, rel=F16_TOL, what="fuse_norm=0 under fp16 storage")


@pytest.mark.parametrize("spelling", ["written_out", "functional"])
def test_cosine_head_runs_the_half_kernels_under_fp16_storage(gpu, tmp_path, spelling):
    """conv -> normalise over the channels -> 1x1 conv: halves in and out of the normalisation, so fp16=1 runs the fp16 entry with no cast
    around it -- the fused launch, F.normalize, and with fuse_norm = 0 the norm kernel on its own"""
    b = mg.PnnxBuilder(seed=11)
    f = b.conv(b.relu(b.conv(b.input((2, 3, 12, 10)), 16, 3, 1, 1)), 32, 3, 1, 1)
    u = b.normalize(f, 1) if spelling == "functional" else b.div(f, b.unsqueeze(b.norm(f, 1, 2, False), 1))
    b.output(b.conv(u, 8, 1))
    pp, bp = save(b, tmp_path)
    x = mg.synth_input((2, 12, 10, 3))
    (ref,) = [nhwc_of(r) for r in lr.eval_graph(b, x)]
    for fuse in ((1, 0) if spelling == "written_out" else (1,)):
        e, (got,) = run_engine(pp, bp, x, fp16=1, fuse_norm=fuse)
        prof = e.profile()
        layers = lpnorm_layers(prof)
        assert len(layers) == 1 and layers[0]["kernel"] == lr.kname("row_group", np.float16, True), layers
        names = [L["name"] for L in prof]
        assert not any(n.startswith(layers[0]["name"] + ".in_to_f32") or n.startswith(layers[0]["name"] + ".out_to_f16") for n in names), names
        assert any("div_" in ln for ln in e.schedule()["fused"]) == (spelling == "written_out" and fuse == 1), e.schedule()
        (emu,) = [nhwc_of(r) for r in lr.eval_graph(b, x, rnd=lr.round_f16, unstored=("torch.norm",) if fuse else ())]
        print("cosine head %s fuse_norm=%d fp16 storage: vs the emulation %.3e; vs fp64: engine %.3e, emulation %.3e" % (
            spelling, fuse, util.rel_err(got, emu), util.rel_err(got, ref), util.rel_err(emu, ref)))
        util.assert_parity(got, emu, rel=F16_TOL, what="cosine head %s fuse_norm=%d" % (spelling, fuse))
