"""GPU: si_hip_detect_image_masks_f32 (include/si_imgmask.h) against the numpy float32 restatement bit for bit, against detect_masks at the
identity, against the float64 rule outside its bound, on views under guard bands, and its invariants (tests/imgmask_reference.py)."""
import numpy as np
import pytest

import detect_reference as dr
import imgmask_reference as R

pytestmark = pytest.mark.gpu
SENT = 0x5A
GEOMS = list(R.geometries(20, 24))
PRODUCT = [(p, nm, crop, g, cnt) for p in R.PLANES for nm in R.NMS for crop in R.CROPS for g in GEOMS for cnt in R.COUNTS]
IDS = ["%dx%d-nm%d-%s-%s-c%d" % (p[0], p[1], nm, crop, g, cnt[0]) for p, nm, crop, g, cnt in PRODUCT]


@pytest.fixture(scope="module")
def hops(native_libs):
    from simpleinfer_amd import hipops
    return hipops


def run(hops, c, nm, **kw):
    return hops.detect_image_masks(c.protos, c.extras, c.boxes, c.counts, c.geom, c.out_hw, c.crop, c.coef_off, nm=nm, out_fill=SENT, full=True, **kw)


def check(planes, want, what):
    for b, w in enumerate(want):
        assert planes[b, :len(w)].tobytes() == w.tobytes(), "%s image %d: %d mask bytes differ" % (what, b, int((planes[b, :len(w)] != w).sum()))
        assert (planes[b, len(w):] == SENT).all(), "%s image %d: planes behind the %d detections were written" % (what, b, len(w))


@pytest.mark.parametrize("plane,nm,crop,gname,counts", PRODUCT, ids=IDS)
def test_bits_equal_the_float32_restatement(hops, plane, nm, crop, gname, counts):
    c = R.case(plane, nm, crop, gname, counts)
    d = hops.image_mask_desc(2, plane[0], plane[1], nm, R.MAX_DET, nm + c.coef_off, c.out_hw[0], c.out_hw[1], c.coef_off, crop=crop)
    name = hops.detect_image_masks_kernel_name(d)
    assert name == "detect_image_masks_kernel<%s>" % c.arm if c.arm else name in ("detect_image_masks_kernel<shared>", "detect_image_masks_kernel<direct>")
    want = R.expected(plane, nm, crop, gname, counts)
    check(run(hops, c, nm), want, IDS[PRODUCT.index((plane, nm, crop, gname, counts))])
    if counts[0] and gname != "down":
        assert 0 < sum(int(w.sum()) for w in want) < sum(w.size for w in want), "the case sets some pixels and clears some"


@pytest.mark.parametrize("cid", ["m20x24_nm32", "m20x24_nm33", "m5x7_nm64", "m160x160_nm32"])
def test_identity_crop_after_equals_detect_masks(hops, cid):
    """the whole plane as the window, the output of the plane's size, the boxes scaled by the ratio 0.25: a power of two, so that
    x * 0.25 + w * 0.25 here and (x + w) * 0.25 in detect_masks are the same number"""
    c = dr.mask_cases()[cid]
    n, mh, mw, nm = c.protos.shape
    assert c.ratio_w == c.ratio_h == 0.25
    geom = np.tile(np.asarray([0, 0, mw, mh, mw, mh], np.int32), (n, 1))
    got = hops.detect_image_masks(c.protos, c.extras, c.net_boxes * np.float32(0.25), c.counts, geom, (mh, mw), "after", c.coef_off, nm=nm,
                                  out_fill=SENT, full=True)
    want = hops.detect_masks(c.protos, c.extras, c.net_boxes, c.counts, c.ratio_w, c.ratio_h, c.coef_off, out_fill=SENT, full=True)
    assert got.tobytes() == want.tobytes() and 0 < int((want == 1).sum())


@pytest.mark.parametrize("plane,nm,crop,gname,counts", [p for p in PRODUCT if p[4][0] and p[3] in ("x4", "offset", "down")],
                         ids=[i for i, p in zip(IDS, PRODUCT) if p[4][0] and p[3] in ("x4", "offset", "down")])
def test_bytes_equal_the_float64_rule_outside_its_bound(hops, plane, nm, crop, gname, counts):
    c = R.case(plane, nm, crop, gname, counts)
    ref = R.expected_f64(plane, nm, crop, gname, counts)
    decided, excluded = R.decided(ref)
    print("excluded share %.5f" % excluded)
    assert excluded <= R.EXCLUDED_CAP
    got = run(hops, c, nm)
    for b, (want, _, _) in enumerate(ref):
        m = decided[b]
        assert np.array_equal(got[b, :len(want)][m], want[m]), (b, int((got[b, :len(want)][m] != want[m]).sum()))


@pytest.mark.parametrize("pattern", [0xFF, 0x7B])
@pytest.mark.parametrize("nm,crop,gname", [(32, "after", "border"), (33, "first", "border"), (64, "after", "x4"), (32, "first", "down")])
def test_views_under_guard_bands(hops, nm, crop, gname, pattern):
    """proto_ld > nm and box_ld > 4 with NaN (0xFF) or 1.3e36 (0x7B) in the gaps, prototypes off a 16-byte and masks off a 4-byte boundary (the
    border geometry of the 20 x 24 plane has OW = 75), the sentinel behind counts[b], bands on both sides of every buffer"""
    key = ((20, 24), nm, crop, gname, R.COUNTS[0])
    c = R.case(*key)
    with hops.guard_bands(pattern):
        got = run(hops, c, nm, proto_ld=nm + 3, protos_off=1, box_ld=7, masks_off=3, in_fill=hops.ByteFill(pattern))
    check(got, R.expected(*key), "view %s %s" % (gname, crop))


@pytest.mark.parametrize("crop", R.CROPS)
def test_invariants(hops, crop):
    key = ((20, 24), 32, crop, "x4", R.COUNTS[1])
    c = R.case(*key)
    first = run(hops, c, 32)
    assert first.tobytes() == run(hops, c, 32).tobytes(), "two runs"
    assert first.tobytes() == run(hops, c, 32, force_direct=True).tobytes(), "both arms"
    d = hops.image_mask_desc(2, 20, 24, 32, R.MAX_DET, 32 + c.coef_off, 80, 96, c.coef_off, crop=crop, force_direct=True)
    assert hops.detect_image_masks_kernel_name(d) == "detect_image_masks_kernel<direct>"
    # detection 5 of image 1 alone, as detection 0 of image 0 of a call with other neighbours
    other = R.case((20, 24), 32, crop, "x4", R.COUNTS[1], seed=1)
    protos, extras, boxes = (np.array(a) for a in (other.protos, other.extras, other.boxes))
    protos[0], extras[0, 0], boxes[0, 0] = c.protos[1], c.extras[1, 5], c.boxes[1, 5]
    alone = hops.detect_image_masks(protos, extras, boxes, (1, 9), c.geom, c.out_hw, crop, c.coef_off, nm=32)
    assert alone[0][0].tobytes() == first[1, 5].tobytes() and first[1, 5].any()


@pytest.mark.parametrize("bad", [(-1, 0, 24, 20, 96, 80), (0, 0, 25, 20, 96, 80), (0, 3, 24, 18, 96, 80), (0, 0, 24, 0, 96, 80),
                                 (0, 0, 24, 20, 0, 80), (0, 0, 24, 20, 97, 80), (2 ** 31 - 1, 0, 2 ** 31 - 1, 20, 96, 80)])
def test_a_window_that_leaves_the_plane_gives_zero_planes(hops, bad):
    """image 0 carries the bad record, image 1 a good one: zeros for the first, the rule for the second, nothing touched outside (bands)"""
    key = ((20, 24), 32, "after", "x4", R.COUNTS[1])
    c = R.case(*key)
    geom = np.array(c.geom)
    geom[0] = bad
    with hops.guard_bands(0x7B):
        got = hops.detect_image_masks(c.protos, c.extras, c.boxes, c.counts, geom, c.out_hw, c.crop, c.coef_off, nm=32, out_fill=SENT, full=True)
    assert not got[0].any() and got[1].tobytes() == R.expected(*key)[1].tobytes()
