"""GPU: the sampler and the affine-grid kernel of include/si_grid.h, F.grid_sample and F.affine_grid.  Kernel: the case table of
tests/grid_reference.py against the float64 rule, nearest exactly (ties included), boundary and non-finite coordinates, bit-for-bit
independence of vector arm / grid strides / pixel strides, views under guard bands, three passes of the grid-stride loop, the theta source
against the two-launch path.  Layer and engine: one-operator graphs, both toys in fp32 (captured, re-batched, batch-split, the planner passes on
and off) and under fp16 storage, the pass conditions, refusals at load.  Every engine test fails without the layers (LoadModel rejects the
types with kEmpty), every op-level test without the kernels (the symbols are missing)."""
import numpy as np
import pytest

import containment as ct
import grid_reference as gr
import util
from ct_reference import _parse
from simpleinfer_amd import hipops, modelgen as mg
from simpleinfer_amd.engine import Engine, Status, StatusError

pytestmark = pytest.mark.gpu

FP16_EPS = 2.0 ** -11     # half an ulp of a round-to-nearest-even fp16 store, relative to the element


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype and got.dtype in (np.float32, np.float16), (what, got.shape, want.shape, got.dtype, want.dtype)
    u = np.uint32 if got.dtype == np.float32 else np.uint16
    bad = np.nonzero(got.view(u) != want.view(u))
    assert bad[0].size == 0, "%s: %d of %d elements differ in bits, first at %s" % (what, bad[0].size, got.size, tuple(int(b[0]) for b in bad))


def check(got, ref, what, exact=False):
    """the NaN and Inf positions equal the reference's; everything else exact (nearest: the kernel moves values) or at the fp32 bar of
    util.assert_parity -- for fp16 storage plus half an fp16 ulp of the element for the one rounding store.  Returns the max-based error."""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "%s: NaN masks differ (%d vs %d)" % (what, np.isnan(got).sum(), np.isnan(ref).sum())
    inf = np.isinf(ref)
    assert np.array_equal(got[inf].astype(np.float64), ref[inf]), what + ": Inf positions differ"
    ok = np.isfinite(ref)
    g, r = np.where(ok, got, 0.0).astype(np.float64), np.where(ok, ref, 0.0)
    if exact:
        assert np.array_equal(g, r), "%s: %d of %d elements differ" % (what, int((g != r).sum()), r.size)
        return 0.0
    if got.dtype == np.float32:
        return util.assert_parity(g, r, what=what)
    scale = max(float(np.abs(r).max()), 1e-30)
    worst = float((np.abs(g - r) / (FP16_EPS * np.abs(r) + util.REL_TOL * scale)).max())
    assert worst <= 1.0, "%s: %.3f of the fp16 bound" % (what, worst)
    return util.rel_err(g, r)


def run_op(x, grid, mode="bilinear", pad="zeros", ac=False, form="dense", grid_ld=None, grid_c_off=0, **views):
    """hipops.grid_sample on a logical grid [n, ho, wo, 2] handed over in one of its three memory images"""
    with np.errstate(over="ignore"):            # (1e30 is Inf in fp16 storage)
        grid = np.asarray(grid, x.dtype)
    if form == "dense":
        img, strides = gr.dense_grid(grid)
        off = 0
    elif form == "stored":
        img, strides = gr.stored_grid(grid, grid_ld)
        off = 0
    else:
        img, strides, off = gr.in_place_grid(grid, grid_ld, grid_c_off)
    return hipops.grid_sample(x, img, mode, pad, ac, out_hw=grid.shape[1:3], grid_strides=strides, grid_off=off, **views)


# ---- the kernel against float64 -----------------------------------------------------------------------------------------------
_REF = {}


def case_with_ref(i):
    """(row, x, grid, float64 reference), computed once and shared"""
    if i not in _REF:
        r = gr.CASES[i]
        x, grid = gr.case_operands(r)
        ref = gr.grid_sample_ref(x, grid, r["mode"], r["pad"], r["ac"])
        ref.setflags(write=False)
        _REF[i] = (r, x, grid, ref)
    return _REF[i]


@pytest.mark.parametrize("i", range(len(gr.CASES)), ids=[gr.case_id(r) for r in gr.CASES])
def test_cases_against_float64(gpu, i):
    r, x, grid, ref = case_with_ref(i)
    got = run_op(x, grid, r["mode"], r["pad"], r["ac"])
    assert got.dtype == x.dtype
    assert hipops.LAST_KERNEL_NAME["si_hip_grid_sample"] == gr.expected_kernel(r["c"], r["half"], "pair")
    e = check(got, ref, gr.case_id(r), exact=r["mode"] == "nearest")
    ok = np.isfinite(ref)
    print("grid_sample %s: max-based %.3e, element-wise %.3e" % (gr.case_id(r), e, util.mixed_err(np.where(ok, got, 0.0), np.where(ok, ref, 0.0))))


def _pixel_grid(py, px):
    """a logical grid [1, ho, wo, 2] whose PIXEL coordinates on a 5 x 5 image under align_corners=True are exactly (py, px): g = p / 2 - 1 is
    exact for multiples of 1/4 of moderate size, and ((g + 1) * 0.5) * 4 gives p back exactly"""
    return np.stack([np.asarray(px, np.float32) / 2 - 1, np.asarray(py, np.float32) / 2 - 1], -1)[None].astype(np.float32)


@pytest.mark.parametrize("pad", gr.PADDINGS)
@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
def test_nearest_is_exact_also_on_ties(gpu, half, pad):
    """every multiple of 1/4 px from -4 to 8 on both axes: the ties at .5 go to the even pixel, before and after border and reflection"""
    p = np.arange(-16, 33, dtype=np.float32) / 4
    py, px = np.meshgrid(p, p, indexing="ij")
    grid = _pixel_grid(py, px)
    x = util.rng_uniform(7, (1, 5, 5, 3), -1.0, 1.0).astype(np.float16 if half else np.float32)
    coords = gr.pixel_coords(grid.astype(x.dtype), 5, 5, "zeros", True)
    assert np.array_equal(coords[0][0], py) and np.array_equal(coords[1][0], px)         # the construction is exact, in fp16 storage too
    ref = gr.grid_sample_ref(x, grid.astype(x.dtype), "nearest", pad, True)
    got = run_op(x, grid, "nearest", pad, True)
    check(got, ref, "nearest ties, " + pad, exact=True)
    if pad == "zeros":       # spot checks of half-to-even that do not go through the reference: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, 3.5 -> 4, 4.5 -> 4, -0.5 -> 0
        col = {float(v): k for k, v in enumerate(p)}
        for v, want in ((0.5, 0), (1.5, 2), (2.5, 2), (3.5, 4), (4.5, 4), (-0.5, 0)):
            assert np.array_equal(got[0, col[v], col[2.0]], x[0, want, 2]) and np.array_equal(got[0, col[2.0], col[v]], x[0, 2, want]), v
        assert not got[0, col[4.75]].any() and not got[0, col[-0.75]].any() and not got[0, :, col[5.0]].any()


@pytest.mark.parametrize("mode", gr.MODES)
@pytest.mark.parametrize("c,half", [(4, False), (3, False), (8, True)], ids=["f32_vec4", "f32_scalar", "f16_vec8"])
def test_boundary_and_non_finite_coordinates(gpu, c, half, mode):
    """-1, size, size - 0.5 and -0.5 px, +-1e30, +-Inf and NaN on either axis, per padding mode; zeros padding gives exactly 0 out of range
    and NaN in every channel for a NaN coordinate"""
    vals = np.asarray([-1.0, 5.0, 4.5, -0.5, 0.0, 4.0, 2.25, 1e30, -1e30, np.inf, -np.inf, np.nan], np.float32)
    py, px = np.meshgrid(vals, vals, indexing="ij")
    with np.errstate(invalid="ignore", over="ignore"):
        grid = _pixel_grid(py, px)
    x = util.rng_uniform(9, (1, 5, 5, c), 0.5, 1.5).astype(np.float16 if half else np.float32)
    with np.errstate(over="ignore"):
        stored_values = grid.astype(x.dtype)            # (1e30 is Inf in fp16 storage)
    for pad in gr.PADDINGS:
        ref = gr.grid_sample_ref(x, stored_values, mode, pad, True)
        got = run_op(x, grid, mode, pad, True)
        assert hipops.LAST_KERNEL_NAME["si_hip_grid_sample"] == gr.expected_kernel(c, half)
        check(got, ref, "%s %s" % (mode, pad), exact=mode == "nearest")
        nan = np.isnan(vals)
        if pad == "zeros":
            assert np.isnan(got[0][nan]).all() and np.isnan(got[0][:, nan]).all()                # a NaN coordinate: every channel
            out = np.isin(np.arange(vals.size), [0, 1, 7, 8, 9, 10])                             # -1, size, +-1e30, +-Inf
            assert not got[0][out][:, ~nan].any() and not got[0][~nan][:, out].any()             # exactly 0
            if mode == "bilinear":
                assert np.array_equal(got[0, 3, 4].astype(np.float64), 0.5 * x[0, 0, 0].astype(np.float64))           # (-0.5, 0): half the edge
        else:
            assert np.isfinite(got).all(), pad


@pytest.mark.parametrize("c,half", [(4, False), (5, False), (8, True)], ids=["f32_vec4", "f32_scalar", "f16_vec8"])
def test_inf_in_x_under_a_weight_of_zero(gpu, c, half):
    """integer positions: the other three taps have weight 0 and are still multiplied where they are inside the image (0 * Inf is NaN, as in
    torch); a tap outside is not read"""
    p = np.arange(0, 5, dtype=np.float32)
    py, px = np.meshgrid(p, p, indexing="ij")
    grid = _pixel_grid(py, px)
    x = util.rng_uniform(11, (1, 5, 5, c), -1.0, 1.0).astype(np.float16 if half else np.float32)
    x[0, 2, 2, 1 % c] = np.inf
    x[0, 4, 4, 0] = -np.inf
    ref = gr.grid_sample_ref(x, grid.astype(x.dtype), "bilinear", "zeros", True)
    assert np.isnan(ref).sum() == 6 and np.isinf(ref).sum() == 2       # three pixels whose footprint holds each Inf under a weight of 0
    check(run_op(x, grid, "bilinear", "zeros", True), ref, "Inf in x")


@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
def test_independence_bit_for_bit(gpu, half):
    """one result whatever the vector arm, the grid's memory image and the pixel strides"""
    dt = np.float16 if half else np.float32
    x = util.rng_uniform(21, (3, 7, 6, 8), -1.0, 1.0).astype(dt)
    grid = gr.make_grid(22, 3, 5, 9).astype(dt)
    full = 8 if half else 4
    for mode, pad, ac in (("bilinear", "zeros", False), ("bilinear", "reflection", True), ("nearest", "border", False)):
        base = run_op(x, grid, mode, pad, ac)
        assert hipops.LAST_KERNEL_NAME["si_hip_grid_sample"] == gr.expected_kernel(8, half, "pair")
        what = "%s %s %d: " % (mode, pad, ac)
        same_bits(run_op(x, grid, mode, pad, ac), base, what + "two launches")
        arms = set()
        for in_ld, out_ld in ((16, 24), (12, 8), (10, 8), (8, 18), (9, 8), (8, 11)):                      # every vector width of the type, scalars
            same_bits(run_op(x, grid, mode, pad, ac, in_ld=in_ld, out_ld=out_ld, in_fill=np.nan), base, what + "in_ld %d out_ld %d" % (in_ld, out_ld))
            arms.add(hipops.LAST_KERNEL_NAME["si_hip_grid_sample"])
        assert arms == {gr.expected_kernel(v, half) for v in ((8, 4, 2, 1) if half else (4, 1))}, arms
        for form, kw, source in (("stored", {}, "strided"), ("stored", dict(grid_ld=8), "strided"), ("inplace", {}, "pair"),
                                 ("inplace", dict(grid_ld=6, grid_c_off=2), "pair"), ("inplace", dict(grid_ld=5, grid_c_off=1), "strided"),
                                 ("inplace", dict(grid_ld=4, grid_c_off=1), "strided")):
            same_bits(run_op(x, grid, mode, pad, ac, form=form, **kw), base, what + "%s %r" % (form, kw))
            assert hipops.LAST_KERNEL_NAME["si_hip_grid_sample"] == gr.expected_kernel(full, half, source), (form, kw)
        for i in range(3):
            same_bits(run_op(x[i:i + 1], grid[i:i + 1], mode, pad, ac), base[i:i + 1], what + "batch item %d alone" % i)


# ---- views and containment ----------------------------------------------------------------------------------------------------
def _wild_grid(seed, n, ho, wo):
    """a grid with +-Inf, NaN and +-1e30 (fp16: Inf) among ordinary values"""
    g = gr.make_grid(seed, n, ho, wo).reshape(-1)
    for k, v in enumerate((np.inf, -np.inf, np.nan, 1e30, -1e30)):
        g[3 + k::13] = v
    return g.reshape(n, ho, wo, 2)


class SampleView:
    def __init__(self, vid, half, c, mode, pad, ac, form="dense", grid_kw=None, **views):
        self.id, self.half, self.c, self.mode, self.pad, self.ac, self.form, self.grid_kw, self.views = vid, half, c, mode, pad, ac, form, grid_kw or {}, views
        self.entries = ("si_hip_grid_sample_f16" if half else "si_hip_grid_sample_f32",)
        self.buffers = 3

    def operands(self):
        dt = np.float16 if self.half else np.float32
        with np.errstate(over="ignore"):
            return util.rng_uniform(31, (2, 7, 6, self.c), -1.0, 1.0).astype(dt), _wild_grid(32, 2, 5, 9).astype(dt)

    def run(self, fill):
        x, grid = self.operands()
        full = run_op(x, grid, self.mode, self.pad, self.ac, form=self.form, full=True, in_fill=fill, out_fill=fill, **self.grid_kw, **self.views)
        return ct.Out("y", full, self.views.get("out_c_off", 0), self.c)

    def dense(self):
        x, grid = self.operands()
        return run_op(x, grid, self.mode, self.pad, self.ac), gr.grid_sample_ref(x, grid, self.mode, self.pad, self.ac)


class AffineView:
    def __init__(self, vid, half, out_ld):
        self.id, self.half, self.out_ld = vid, half, out_ld
        self.entries = ("si_hip_affine_grid_f16" if half else "si_hip_affine_grid_f32",)
        self.buffers = 2
        self.c = 5          # H: the innermost dimension of the stored [n][W][2][H] image

    def run(self, fill):
        theta = util.rng_uniform(33, (2, 2, 3), -1.5, 1.5)
        full = hipops.affine_grid(theta, (5, 7), True, self.half, out_ld=self.out_ld, out_fill=fill, full=True)
        return ct.Out("grid", full, 0, 5)

    def dense(self):
        theta = util.rng_uniform(33, (2, 2, 3), -1.5, 1.5)
        dt = np.float16 if self.half else np.float32
        got = hipops.affine_grid(theta, (5, 7), True, self.half)
        return got.transpose(0, 2, 3, 1), gr.affine_grid_ref(theta.astype(dt), (5, 7), True).astype(np.float64).transpose(0, 2, 3, 1)


VIEW_CASES = [
    SampleView("f32_vec4_slices", False, 8, "bilinear", "zeros", False, in_ld=20, in_c_off=4, out_ld=24, out_c_off=12),
    SampleView("f32_scalar_last_slice", False, 5, "bilinear", "reflection", True, in_ld=9, in_c_off=4, out_ld=7, out_c_off=2),
    SampleView("f32_nearest_in_place_grid", False, 4, "nearest", "border", False, "inplace", dict(grid_ld=6, grid_c_off=4), in_ld=8, in_c_off=4, out_ld=12, out_c_off=8),
    SampleView("f32_stored_grid", False, 3, "bilinear", "border", True, "stored", dict(grid_ld=7), in_ld=4, in_c_off=1, out_ld=3, out_c_off=0),
    SampleView("f16_vec8_slices", True, 8, "bilinear", "zeros", True, in_ld=16, in_c_off=8, out_ld=32, out_c_off=16),
    SampleView("f16_vec2_in_place_grid", True, 6, "nearest", "zeros", False, "inplace", dict(grid_ld=4, grid_c_off=2), in_ld=14, in_c_off=2, out_ld=22, out_c_off=4),
    SampleView("f16_scalar", True, 3, "bilinear", "reflection", False, "stored", {}, in_ld=11, in_c_off=5, out_ld=8, out_c_off=5),
    AffineView("affine_f32_rows", False, 9),
    AffineView("affine_f16_rows", True, 6),
]


@pytest.mark.parametrize("case", VIEW_CASES, ids=[c.id for c in VIEW_CASES])
def test_views_and_containment(gpu, case):
    del hipops.LAST_ENTRIES[:]
    dense, ref = case.dense()
    check(dense, ref, case.id + ", dense", exact=getattr(case, "mode", "") == "nearest")
    plain = case.run(hipops.ByteFill(0x00))
    assert set(case.entries) <= set(hipops.LAST_ENTRIES), hipops.LAST_ENTRIES
    ct.assert_outside_fill(plain.full, plain.c_off, plain.c, 0x00, case.id + ", plain run")
    same_bits(plain.full[..., plain.c_off:plain.c_off + plain.c], dense, case.id + " against the dense run")
    for byte in ct.PATTERNS:      # 0xFF: the gaps between the channels hold NaN; 0x7B: a large finite sentinel
        with hipops.guard_bands(byte) as g:      # all bands and the inputs are compared when the block ends
            out = case.run(hipops.ByteFill(byte))
        what = "%s under 0x%02X" % (case.id, byte)
        assert g.checked == case.buffers, "%s: the guard saw %d buffers" % (what, g.checked)
        ct.assert_outside_fill(out.full, out.c_off, out.c, byte, what)             # every byte outside the output view unchanged
        same_bits(out.full[..., out.c_off:out.c_off + out.c], plain.full[..., plain.c_off:plain.c_off + plain.c], what)


def test_three_passes_of_the_grid_stride_loop(gpu):
    """fp16, c = 8: one item per pixel, 2048 x 256 items per pass, 1030 x 1030 pixels = 2.02 passes' worth: every lane goes round up to three
    times"""
    ho = wo = 1030
    assert 2 * 2048 * 256 < ho * wo <= 3 * 2048 * 256
    x = util.rng_uniform(41, (1, 4, 5, 8), -1.0, 1.0).astype(np.float16)
    grid = util.rng_uniform(42, (1, ho, wo, 2), -1.2, 1.2).astype(np.float16)
    got = run_op(x, grid, "bilinear", "border", False)
    assert hipops.LAST_KERNEL_NAME["si_hip_grid_sample"] == gr.expected_kernel(8, True)
    check(got, gr.grid_sample_ref(x, grid, "bilinear", "border", False), "three passes")


# ---- affine grid and the theta source -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("ac", [False, True], ids=["noac", "ac"])
def test_affine_grid_against_the_rule(gpu, ac, half):
    dt = np.float16 if half else np.float32
    for k, (h, w) in enumerate([(1, 1), (1, 6), (7, 2), (13, 17)]):
        theta = util.rng_uniform(50 + k, (3, 2, 3), -1.5, 1.5).astype(dt)
        got = hipops.affine_grid(theta, (h, w), ac, half)
        assert got.shape == (3, h, w, 2) and got.dtype == dt
        assert hipops.LAST_KERNEL_NAME["si_hip_affine_grid"] == ("affine_grid_kernel<_Float16>" if half else "affine_grid_kernel<float>")
        ref = gr.affine_grid_ref(theta, (h, w), ac, coords64=True)
        # |g| <= 4.5 here: an fp32 result is within a few ulps of 4.5 (two fused multiply-adds on rounded base coordinates), an fp16 one
        # within half an fp16 ulp of the element more
        bound = 8 * 2.0 ** -24 * 4.5 + (FP16_EPS * np.abs(ref) if half else 0.0)
        assert (np.abs(got.astype(np.float64) - ref) <= bound).all(), (h, w, np.abs(got - ref).max())
        if not half:
            same_bits(got, gr.affine_grid_ref(theta, (h, w), ac), "fp32 affine grid against the fp32 rule %dx%d" % (h, w))


@pytest.mark.parametrize("mode", gr.MODES)
def test_theta_source_equals_the_two_launch_path(gpu, mode):
    """fp32, bit for bit: the sampler computing the coordinates from theta against si_hip_affine_grid followed by the sampler on that grid
    (stored and dense images).  nearest: translations and power-of-two scales that keep every coordinate 0.18 px from a tie by construction
    (W = H = 8, no align_corners: xb = odd / 8, g = odd / 16 + 1 / 64, px = 4 g + 3.5 = odd / 4 + 3.5625)"""
    x = util.rng_uniform(60, (2, 8, 8, 8), -1.0, 1.0)
    if mode == "nearest":
        thetas = [np.asarray([[[0.5, 0, 1 / 64], [0, 0.5, 1 / 64]], [[2.0, 0, -1 / 64], [0, 0.25, 3 / 64]]], np.float32)]
        settings = [("zeros", False), ("border", False), ("reflection", False)]
    else:
        thetas = [util.rng_uniform(61, (2, 2, 3), -1.3, 1.3), np.asarray([[[1, 0, 0], [0, 1, 0]]] * 2, np.float32)]
        settings = [("zeros", False), ("border", True), ("reflection", False), ("reflection", True)]
    for theta in thetas:
        for pad, ac in settings:
            grid = hipops.affine_grid(theta, (8, 8), ac)
            if mode == "nearest":
                py, px = gr.pixel_coords(grid, 8, 8, "zeros", ac)
                assert (np.abs(py - np.floor(py) - 0.5) >= 1e-3).all() and (np.abs(px - np.floor(px) - 0.5) >= 1e-3).all()
            two = run_op(x, grid, mode, pad, ac, form="stored")
            one = hipops.grid_sample(x, None, mode, pad, ac, theta=theta, out_hw=(8, 8))
            assert hipops.LAST_KERNEL_NAME["si_hip_grid_sample"] == gr.expected_kernel(8, False, "theta")
            same_bits(one, two, "theta source, %s %s %d" % (mode, pad, ac))
            same_bits(run_op(x, grid, mode, pad, ac), two, "dense grid")
            check(one, gr.grid_sample_ref(x, gr.affine_grid_ref(theta, (8, 8), ac), mode, pad, ac), "theta source against the rule", exact=mode == "nearest")


# ---- layer and engine ---------------------------------------------------------------------------------------------------------
def save(b, tmp_path, tag):
    pp, bp = str(tmp_path / (tag + ".pnnx.param")), str(tmp_path / (tag + ".pnnx.bin"))
    b.save(pp, bp)
    return pp, bp


def run_engine(b, tmp_path, xs, tag="m", forwards=1, outputs=None, **opts):
    """(engine, the graph output as the engine stores it -- or the list of the named outputs); xs: one array per graph input, in order"""
    pp, bp = save(b, tmp_path, tag)
    e = Engine(**opts)
    e.load_model(pp, bp)
    xs = xs if isinstance(xs, (list, tuple)) else [xs]
    for name, x in zip(e.input_names(), xs):
        e.input(name, x)
    for _ in range(forwards):
        e.forward()
    outs = [_parse(ln)[2][0] for ln in b.lines if ln.startswith("pnnx.Output")]
    if outputs is None:
        (out,) = outs
        return e, e.extract(out)
    return e, [e.extract(o) for o in outs]


def stored(grid):
    """a logical rank-4 [n, ho, wo, 2] array as the engine takes and returns that operand: dimensions (0, 2, 3, 1)"""
    return np.ascontiguousarray(np.asarray(grid).transpose(0, 2, 3, 1))


def logical(stored_grid):
    return np.ascontiguousarray(np.asarray(stored_grid).transpose(0, 3, 1, 2))


@pytest.mark.parametrize("mode,pad,ac", [("bilinear", "zeros", False), ("nearest", "reflection", True), ("bilinear", "border", None)])
def test_grid_sample_in_a_one_operator_graph(gpu, tmp_path, mode, pad, ac):
    x = util.rng_uniform(70, (2, 9, 11, 8), -1.0, 1.0)
    grid = gr.make_grid(71, 2, 13, 17)
    b = mg.PnnxBuilder(seed=1)
    b.output(b.grid_sample(b.input((2, 8, 9, 11)), b.input((2, 13, 17, 2)), mode, pad, ac))
    eng, got = run_engine(b, tmp_path, [x, stored(grid)])
    assert got.shape == (2, 13, 17, 8)
    check(got, gr.grid_sample_ref(x, grid, mode, pad, bool(ac)), "F.grid_sample layer", exact=mode == "nearest")
    same_bits(got, run_op(x, grid, mode, pad, bool(ac), form="stored"), "the layer against the op-level entry")
    (layer,) = [L for L in eng.profile() if L["type"] == gr.SAMPLE]
    assert layer["kernel"] == gr.expected_kernel(8, False, "strided"), layer          # the stored [N][Wo][2][Ho] image: the coordinates Ho apart
    assert layer["flops"] == (8.0 * got.size if mode == "bilinear" else 0.0)
    assert layer["bytes"] == 4.0 * (x.size + grid.size + got.size)


@pytest.mark.parametrize("ac", [False, True, None], ids=["noac", "ac", "none"])
def test_affine_grid_in_a_one_operator_graph(gpu, tmp_path, ac):
    theta = util.rng_uniform(72, (2, 2, 3), -1.5, 1.5)
    b = mg.PnnxBuilder(seed=1)
    b.output(b.affine_grid(b.input((2, 2, 3)), (2, 3, 6, 7), ac))
    eng, got = run_engine(b, tmp_path, [theta])
    assert got.shape == (2, 7, 2, 6)
    same_bits(logical(got), gr.affine_grid_ref(theta, (6, 7), bool(ac)), "F.affine_grid layer against the fp32 rule")
    (layer,) = [L for L in eng.profile() if L["type"] == gr.AFFINE]
    assert layer["kernel"] == "affine_grid_kernel<float>" and layer["flops"] == 4.0 * got.size, layer


def stn_input(b):
    n, c, h, w = b.shapes["0"]
    return mg.synth_input((n, h, w, c))


def flow_inputs(b):
    n, c, h, w = b.shapes["0"]
    return [mg.synth_input((n, h, w, c)), mg.flow_base_grid(n, h, w)]


TOYS = {"stn": (mg.build_toy_stn, stn_input), "flow": (mg.build_toy_flow_warp, flow_inputs)}


@pytest.mark.parametrize("which", sorted(TOYS))
def test_toys_fp32(gpu, tmp_path, which):
    build, inputs = TOYS[which]
    b = build()
    xs = inputs(b)
    want = gr.eval_graph(b, xs)
    eng, got = run_engine(b, tmp_path, xs)
    util.assert_parity(got, want, what="toy " + which)
    types = [L["type"] for L in eng.profile()]
    (layer,) = [L for L in eng.profile() if L["type"] == gr.SAMPLE]
    sched = eng.schedule()
    if which == "stn":
        # one launch: no affine step, the grid [2, 32, 32, 2] is never allocated
        assert gr.AFFINE not in types and "F_affine_grid_0" in sched["fused"] and layer["kernel"] == gr.expected_kernel(3, False, "theta"), (types, layer)
    else:
        # the grid is read in place: no permute launch, both coordinates in one load
        assert "Tensor.permute" not in types and "Tensor_permute_0" in sched["fused"] and layer["kernel"] == gr.expected_kernel(8, False, "pair"), (types, layer)
    _, cap = run_engine(b, tmp_path, xs, forwards=3, graph=1)
    same_bits(cap, got, which + ": graph=1 replay over three forwards")
    # the passes off (fuse_grid=0 alone, then every fusion): the same bits from the two-launch plans, whose grid has a step and a buffer
    grid_bytes = 4 * int(np.prod(b.shapes[[_parse(ln) for ln in b.lines if ln.startswith(gr.SAMPLE)][0][2][1]]))
    for opts in (dict(fuse_grid=0), dict(fuse=0)) + ((dict(fuse_layout=0),) if which == "flow" else ()):
        e0, plain = run_engine(b, tmp_path, xs, **opts)
        same_bits(plain, got, "%s: %r" % (which, opts))
        types0 = [L["type"] for L in e0.profile()]
        (layer0,) = [L for L in e0.profile() if L["type"] == gr.SAMPLE]
        assert layer0["kernel"].endswith("strided>") and ((gr.AFFINE if which == "stn" else "Tensor.permute") in types0), (opts, types0, layer0)
        assert not {"F_affine_grid_0", "Tensor_permute_0"} & set(e0.schedule()["fused"]), opts
        if "fuse_grid" in opts:
            assert e0.schedule()["per_operand_bytes"] - sched["per_operand_bytes"] == grid_bytes, (e0.schedule(), sched)


@pytest.mark.parametrize("which", sorted(TOYS))
def test_toys_rebatched(gpu, tmp_path, which):
    build, inputs = TOYS[which]
    b2, b4 = build(batch=2), build(batch=4)
    xs = inputs(b4)
    _, want = run_engine(b4, tmp_path, xs, tag="b4")
    util.assert_parity(want, gr.eval_graph(b4, xs), what="batch 4")
    eng, got = run_engine(b2, tmp_path, xs, tag="b2", batch=4)
    same_bits(got, want, "batch=4 on the batch-2 file")          # (F.affine_grid's size=(2, ..) follows the re-batch)
    smp = [_parse(ln) for ln in b2.lines if ln.startswith(gr.SAMPLE)][0]
    assert eng.operand_shape(smp[3][0])[0] == 4
    _, plain = run_engine(b2, tmp_path, xs, tag="b2", batch=4, fuse=0)
    same_bits(plain, want, "batch=4, fuse=0")


@pytest.mark.parametrize("mode", ["host_slices2", "streams2"])
@pytest.mark.parametrize("which", sorted(TOYS))
def test_toys_batch_split(gpu, tmp_path, which, mode):
    """as tests/test_gpu_batch_split.py for its toys: the split run has the bits of the unsplit one, and it really was split"""
    build, inputs = TOYS[which]
    b = build(batch=4)
    xs = inputs(b)
    e0, base = run_engine(b, tmp_path, xs, host_slices=1, streams=1)
    util.assert_parity(base, gr.eval_graph(b, xs), what="unsplit")
    opts, slices, lanes = {"host_slices2": (dict(host_slices=2), 2, 1), "streams2": (dict(streams=2), 1, 2)}[mode]
    e1, got = run_engine(b, tmp_path, xs, **opts)
    sched = e1.schedule()
    assert sched["batch_mixing"] == [] and sched["host_slices"] == slices and sched["lanes"] == lanes, sched
    same_bits(got, base, mode)


@pytest.mark.parametrize("which", sorted(TOYS))
def test_toys_fp16_storage(gpu, tmp_path, which):
    """fp16=1: native fp16 sampler launches; the error against float64 is at most 2x that of the fp16-storage emulation (weights, biases, the
    inputs and every operator's output rounded to fp16, float64 arithmetic between): the bar of test_toys_fp16_storage of the other toys"""
    build, inputs = TOYS[which]
    b = build()
    xs = inputs(b)
    eng, got = run_engine(b, tmp_path, xs, fp16=1)
    (layer,) = [L for L in eng.profile() if L["type"] == gr.SAMPLE]
    assert layer["kernel"].startswith("grid_sample_kernel<"), layer
    ref, emu = gr.eval_graph(b, xs), gr.eval_graph(b, xs, rnd=gr.round_f16)
    e_engine, e_emu = util.rel_err(got, ref), util.rel_err(emu, ref)
    print("toy %s fp16 storage vs float64: engine %.3e, fp16 emulation %.3e, sampler %s" % (which, e_engine, e_emu, layer["kernel"]))
    assert np.isfinite(got).all()
    assert e_engine <= 2.0 * e_emu, (e_engine, e_emu)


def test_pass_conditions_not_met(gpu, tmp_path):
    """a grid that is a graph output, or that has two readers, keeps its own step -- and the results still match"""
    img, base = mg.synth_input((2, 12, 10, 3)), mg.flow_base_grid(2, 12, 10)
    for tag, second in (("output", "output"), ("two_readers", "reader")):
        b = mg.PnnxBuilder(seed=3)
        x, g0 = b.input((2, 3, 12, 10)), b.input((2, 2, 12, 10))
        feat = b.conv(x, 8, 3, 1, 1)
        grid = b.permute(b.add(g0, b.tanh(b.conv(feat, 2, 3, 1, 1))), (0, 2, 3, 1))
        y = b.grid_sample(feat, grid, "bilinear", "border", True)
        if second == "reader":
            y2 = b.grid_sample(feat, grid, "bilinear", "zeros", True)
            b.output(y)
            b.output(y2)
        else:
            b.output(y)
            b.output(grid)
        eng, outs = run_engine(b, tmp_path, [img, base], tag=tag, outputs="all")
        types = [L["type"] for L in eng.profile()]
        assert "Tensor.permute" in types and all(L["kernel"].endswith("strided>") for L in eng.profile() if L["type"] == gr.SAMPLE), eng.profile()
        feat64 = gr.eval_graph(_prefix(b, 3), [img, base])           # features, NHWC
        flow_b = _prefix(b, 6)
        g64 = gr.eval_graph(flow_b, [img, base])                     # base + tanh(flow), NHWC storage of [N, 2, H, W] = the logical grid
        want = gr.grid_sample_ref(feat64, g64, "bilinear", "border", True, coords64=True)
        util.assert_parity(outs[0], want, what=tag)
        if second == "reader":
            util.assert_parity(outs[1], gr.grid_sample_ref(feat64, g64, "bilinear", "zeros", True, coords64=True), what="the second reader")
        else:
            util.assert_parity(logical(outs[1]), g64, what="the grid as a graph output")
    # F.affine_grid: the grid as a graph output keeps the affine step
    theta = util.rng_uniform(80, (2, 2, 3), -1.2, 1.2)
    xa = util.rng_uniform(81, (2, 6, 7, 4), -1.0, 1.0)
    b = mg.PnnxBuilder(seed=4)
    t, x = b.input((2, 2, 3)), b.input((2, 4, 6, 7))
    grid = b.affine_grid(t, (2, 4, 5, 9), False)
    b.output(b.grid_sample(x, grid, "bilinear", "zeros", False))
    b.output(grid)
    eng, outs = run_engine(b, tmp_path, [theta, xa], tag="affine_output", outputs="all")
    assert gr.AFFINE in [L["type"] for L in eng.profile()]
    g32 = gr.affine_grid_ref(theta, (5, 9), False)
    same_bits(logical(outs[1]), g32, "the affine grid as a graph output")
    check(outs[0], gr.grid_sample_ref(xa, g32, "bilinear", "zeros", False), "sampler behind an affine grid that is also an output")
    # different align_corners on the two operators: two launches
    b = mg.PnnxBuilder(seed=4)
    t, x = b.input((2, 2, 3)), b.input((2, 4, 6, 7))
    b.output(b.grid_sample(x, b.affine_grid(t, (2, 4, 5, 9), True), "bilinear", "zeros", False))
    eng, got = run_engine(b, tmp_path, [theta, xa], tag="affine_mixed")
    assert gr.AFFINE in [L["type"] for L in eng.profile()]
    check(got, gr.grid_sample_ref(xa, gr.affine_grid_ref(theta, (5, 9), True), "bilinear", "zeros", False), "mixed align_corners")


def _prefix(b, n_ops):
    """the first n_ops lines of a builder's graph with the last operand as the graph output"""
    p = mg.PnnxBuilder(seed=b.seed)
    p.lines, p.attrs, p.shapes = list(b.lines[:n_ops]), b.attrs, b.shapes
    p.lines.append("pnnx.Output out 1 0 %s" % _parse(b.lines[n_ops - 1])[3][0])
    return p


def test_refused_at_load(gpu, tmp_path):
    """bicubic and rank 5: kUnsupport; wrong shapes: kErrorShape -- with a logged reason at LoadModel; the process goes on"""
    def load(b, tag):
        pp, bp = save(b, tmp_path, tag)
        with pytest.raises(StatusError) as ei:
            Engine().load_model(pp, bp)
        return ei.value.status

    def sampler(x_shape, g_shape, out_shape=None, mode="bilinear"):
        b = mg.PnnxBuilder(seed=1)
        y = b.grid_sample(b.input(x_shape), b.input(g_shape), mode)
        if out_shape:
            b.shapes[y] = tuple(out_shape)
            b.lines[-1] = re_shape(b.lines[-1], y, out_shape)
        b.output(y)
        return b

    def re_shape(line, operand, shape):
        return " ".join("#%s=(%s)f32" % (operand, ",".join(str(s) for s in shape)) if t.startswith("#%s=" % operand) else t for t in line.split())

    assert load(sampler((2, 8, 9, 11), (2, 13, 17, 2), mode="bicubic"), "bicubic") == Status.kUnsupport
    b5 = mg.PnnxBuilder(seed=1)
    x5, g5 = b5.input((2, 4, 3, 9, 11)), b5.input((2, 2, 5, 6, 3))
    y5 = b5._new_operand((2, 4, 2, 5, 6))
    b5._emit(gr.SAMPLE, "F_grid_sample_0", [x5, g5], [y5], dict(align_corners=False, mode="bilinear", padding_mode="zeros"))
    b5.output(y5)
    assert load(b5, "rank5") == Status.kUnsupport
    assert load(sampler((2, 8, 9, 11), (2, 13, 17, 3)), "grid_k") == Status.kErrorShape            # the last dimension is not 2
    assert load(sampler((2, 8, 9, 11), (3, 13, 17, 2)), "grid_n") == Status.kErrorShape
    assert load(sampler((2, 8, 9, 11), (2, 13, 17, 2), (2, 8, 13, 16)), "out_w") == Status.kErrorShape
    assert load(sampler((2, 8, 9, 11), (2, 13, 17, 2), (2, 7, 13, 17)), "out_c") == Status.kErrorShape
    assert load(sampler((2, 8, 9), (2, 13, 17, 2), (2, 8, 13, 17)), "x_rank3") == Status.kErrorShape
    bad = sampler((2, 8, 9, 11), (2, 13, 17, 2))
    bad.lines = [ln.replace("padding_mode=zeros", "padding_mode=wrap") for ln in bad.lines]
    assert load(bad, "padding") == Status.kFail

    def affine(t_shape, size, out_shape=None):
        b = mg.PnnxBuilder(seed=1)
        y = b.affine_grid(b.input(t_shape), size)
        if out_shape:
            b.shapes[y] = tuple(out_shape)
            b.lines[-1] = re_shape(b.lines[-1], y, out_shape)
        b.output(y)
        return b

    assert load(affine((2, 3, 2), (2, 3, 6, 7)), "theta") == Status.kErrorShape
    assert load(affine((2, 2, 3), (2, 3, 6, 7), (2, 6, 8, 2)), "size_w") == Status.kErrorShape
    assert load(affine((2, 2, 3), (3, 3, 6, 7), (2, 6, 7, 2)), "size_n") == Status.kErrorShape
    assert load(affine((2, 3, 4), (2, 3, 4, 6, 7), (2, 4, 6, 7, 3)), "affine_3d") == Status.kUnsupport
    b = sampler((2, 8, 9, 11), (2, 13, 17, 2))
    x, grid = util.rng_uniform(70, (2, 9, 11, 8), -1.0, 1.0), gr.make_grid(71, 2, 13, 17)
    _, got = run_engine(b, tmp_path, [x, stored(grid)])
    check(got, gr.grid_sample_ref(x, grid), "after the refusals")
