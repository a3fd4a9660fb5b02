"""GPU: si_hip_detect_postprocess_f32 and si_hip_detect_masks_f32 (include/si_detect.h; simpleinfer_amd/csrc/hip/postprocess.hip and
detect_masks.hip) against the numpy rule of tests/detect_reference.py.  Every comparison is EXACT -- bytes, NaN payloads included where a
value is carried and not computed -- into sentinel-filled outputs whose elements behind min(counts, max_det) must still hold the sentinel;
there is no tolerance in this file.  Old entry against new on every case of tests/post_reference.py; the matrix of layouts, box formats,
box score, payload sizes and kernel sizes (MATRIX, whose coverage tests/test_detect_post_cpu.py asserts); CHANNELS against ROWS on transposed
data; views under guard bands (VIEW_CASES); special values; repeatability; masks; and two toys end to end through the engine with the
outputs left on the device."""
from typing import NamedTuple

import numpy as np
import pytest

import detect_reference as dr
import post_reference as pr

pytestmark = pytest.mark.gpu

F = np.float32
SENT = 0x7B
SENT32 = np.uint32(0x7B7B7B7B)
EXTRAS = (0, 1, 32, 51)


@pytest.fixture(scope="module")
def hops(gpu):
    from simpleinfer_amd import hipops
    return hipops


def logical(pred, layout):
    return pred if layout == "rows" else dr.to_channels(pred)


def run(hops, cid, layout="rows", agnostic=False, adjusted=False, extra=0, nan_payload=False, max_det=None, **kw):
    """one call into sentinel-filled outputs -> (DetectResult, the rule's answer)"""
    c = dr.cases()[cid]
    pred, outs, cnt = dr.expected(cid, agnostic, adjusted, extra, nan_payload)
    res = hops.detect_postprocess(logical(pred, layout), c.desc.classes, c.desc.objectness, extra, layout, c.desc.box_format, c.desc.prob_thr,
                                  c.desc.nms_thr, agnostic, c.adjust if adjusted else None, max_det=max_det, out_fill=hops.ByteFill(SENT), **kw)
    return res, (outs, cnt)


def check(res, ref, what):
    """the stored rows are the rule's, in every output the call asked for; everything behind them still holds the sentinel"""
    dr.assert_same_picks(res, ref, res.max_det, what)
    for name, a in res.full.items():
        if name == "counts":
            continue
        for b in range(res.n):
            k = min(int(res.counts[b]), res.max_det)
            behind = np.ascontiguousarray(a[b, k:]).view(np.uint32)
            assert (behind == SENT32).all(), "%s image %d: %d words of %s behind the %d stored rows were written" % (
                what, b, int((behind != SENT32).sum()), name, k)


# ---- 1. old against new -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", pr.CASE_IDS)
def test_yolov5_mode_writes_the_old_entrys_bytes(hops, cid):
    c = pr.cases()[cid]
    n, rows, ne = c.pred.shape
    for agnostic in (False, True):
        for adjusted in (False, True):
            dd = hops.DeviceBuffer(n * rows * 6 * 4)
            dd.fill(SENT)
            _, old_cnt = hops.yolo_postprocess(c.pred, c.prob_thr, c.nms_thr, agnostic, c.adjust if adjusted else None, max_det=rows, dets_dev=dd)
            old = dd.to_numpy((n, rows, 6))
            res, ref = run(hops, "v5/" + cid, "rows", agnostic, adjusted)
            what = "%s agnostic=%d adjust=%d" % (cid, agnostic, adjusted)
            assert res.full["dets"].tobytes() == old.tobytes() and res.counts.tobytes() == np.asarray(old_cnt, np.int32).tobytes(), what
            check(res, ref, what)                       # src_rows are the rule's element indices, the network boxes the rule's boxes
            pr.assert_same_result((res.dets, res.counts), pr.expected(cid, agnostic, adjusted), what)


# ---- 2. the matrix ----------------------------------------------------------------------------------------------------------------------------
class Cell(NamedTuple):
    cid: str
    layout: str
    extra: int
    agnostic: bool
    adjusted: bool


def _matrix():
    """every converted case once, every generated case and every class count (bins_*) in both layouts; layout, payload size, agnostic and
    adjust cycle with the index so that the product is thinned and every value still meets every kind of case (tests/test_detect_post_cpu.py
    asserts the coverage)"""
    cells = []
    ids = [cid for cid in dr.cases() if not cid.startswith("v5/")]
    for i, cid in enumerate(ids):
        c = dr.cases()[cid]
        for j in range(1 if c.origin and not c.origin.startswith("bins_") else 2):
            extra = EXTRAS[(i + j) % 4]
            layout = ("rows", "channels")[(i // 4 + j) % 2]
            if cid == "sized_lvis":
                extra, layout = 32, "channels"
            if cid == "sized_ne128":
                extra, layout = 32, ("rows", "channels")[j]
            if layout == "rows" and c.desc.ne + extra > 128:
                layout = "channels"
            cells.append(Cell(cid, layout, extra, bool((i // 2 + j) % 2), bool((i // 8) % 2)))
    cells.append(Cell("v5xy/bins_123", "rows", 0, False, True))             # ROWS at ne = 128 without a payload
    return cells


MATRIX = _matrix()


@pytest.mark.parametrize("cell", MATRIX, ids=["%s-%s-x%d-%s%s" % (m.cid, m.layout, m.extra, "agn" if m.agnostic else "cls", "-adj" if m.adjusted else "")
                                              for m in MATRIX])
def test_matrix_equals_the_rule(hops, cell):
    res, ref = run(hops, cell.cid, cell.layout, cell.agnostic, cell.adjusted, cell.extra)
    check(res, ref, str(cell))


# ---- 3. transposed data -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,extra", [("v8/counts_1025", 32), ("v5xy/geometry", 1), ("v8_classes", 51), ("v8xy/chain2_200", 0), ("sized_ne128", 32)])
def test_channels_on_transposed_data_writes_the_bytes_rows_writes(hops, cid, extra):
    for agnostic in (False, True):
        (r, ref), (c, _) = run(hops, cid, "rows", agnostic, True, extra), run(hops, cid, "channels", agnostic, True, extra)
        for name in r.full:
            assert r.full[name].tobytes() == c.full[name].tobytes(), (cid, agnostic, name)
        check(c, ref, cid)


# ---- 4. views ---------------------------------------------------------------------------------------------------------------------------------
class View(NamedTuple):
    id: str
    entries: tuple
    cid: str
    layout: str
    extra: int
    ld_pad: int
    image_pad: int
    off: int


VIEW_CASES = [
    View("rows_ld", ("si_hip_detect_postprocess_f32",), "v8/counts_129", "rows", 32, 5, 0, 0),
    View("rows_ld_image_ld_off1", ("si_hip_detect_postprocess_f32",), "v8xy/bins_65", "rows", 1, 3, 77, 1),
    View("rows_dense_scan_image_ld", ("si_hip_detect_postprocess_f32",), "v5/counts_257", "rows", 0, 0, 13, 1),
    View("channels_ld", ("si_hip_detect_postprocess_f32",), "v8/counts_129", "channels", 32, 7, 0, 0),
    View("channels_ld_image_ld_off1", ("si_hip_detect_postprocess_f32",), "v5xy/chain_130", "channels", 51, 1, 101, 1),
    View("masks_proto_ld_off1", ("si_hip_detect_masks_f32",), "m20x24_nm32", "", 0, 4, 0, 1),
    View("masks_proto_ld_aligned", ("si_hip_detect_masks_f32",), "m16x16_nm32", "", 0, 8, 0, 0),
    View("masks_generic_ld", ("si_hip_detect_masks_f32",), "m5x7_nm33", "", 0, 3, 0, 0),
]


def run_masks(hops, cid, proto_pad=0, off=0, fill=np.nan):
    c = dr.mask_cases()[cid]
    nm = c.protos.shape[3]
    return hops.detect_masks(c.protos, c.extras, c.net_boxes, c.counts, c.ratio_w, c.ratio_h, c.coef_off, proto_ld=nm + proto_pad, protos_off=off,
                             in_fill=fill, out_fill=SENT, full=True)


def check_masks(planes, cid, what=""):
    c = dr.mask_cases()[cid]
    ref = dr.mask_expected(cid)
    max_det = c.extras.shape[1]
    for b, want in enumerate(ref):
        k = min(int(c.counts[b]), max_det)
        assert planes[b, :k].tobytes() == want.tobytes(), "%s %s image %d: %d mask bytes differ" % (what, cid, b, int((planes[b, :k] != want).sum()))
        assert (planes[b, k:] == SENT).all(), "%s %s image %d: planes behind the %d detections were written" % (what, cid, b, k)


@pytest.mark.parametrize("pattern", [0xFF, 0x7B])
@pytest.mark.parametrize("view", VIEW_CASES, ids=[v.id for v in VIEW_CASES])
def test_views_under_guard_bands(hops, view, pattern):
    """gaps hold NaN (0xFF) or 1.3e36 (0x7B: it would win every class scan and every dot it reached); the bands around every buffer and the
    inputs themselves are compared when the block ends"""
    fill = hops.ByteFill(pattern)
    hops.LAST_ENTRIES.clear()
    with hops.guard_bands(pattern):
        if view.layout:
            c = dr.cases()[view.cid]
            n, rows, _ = c.pred.shape
            ne = c.desc.ne + view.extra
            inner, outer = (ne, rows) if view.layout == "rows" else (rows, ne)
            ld = inner + view.ld_pad
            image_ld = (outer - 1) * ld + inner + view.image_pad
            res, ref = run(hops, view.cid, view.layout, True, True, view.extra, ld=ld, image_ld=image_ld, pred_off=view.off, in_fill=fill)
            check(res, ref, view.id)
        else:
            check_masks(run_masks(hops, view.cid, view.ld_pad, view.off, fill), view.cid, view.id)
    assert set(view.entries) <= set(hops.LAST_ENTRIES)


@pytest.mark.parametrize("agnostic", [False, True], ids=["perclass", "agnostic"])
@pytest.mark.parametrize("delta", ["zero", "one", "picks-1", "picks", "picks+1"])
def test_max_det_around_the_number_of_picks(hops, delta, agnostic):
    _, outs, cnt = dr.expected("v8/counts_129", agnostic, True, 32)
    picks = int(cnt[2])
    assert 2 < picks < 129
    max_det = {"zero": 0, "one": 1, "picks-1": picks - 1, "picks": picks, "picks+1": picks + 1}[delta]
    for layout in ("rows", "channels"):
        res, ref = run(hops, "v8/counts_129", layout, agnostic, True, 32, max_det=max_det)
        check(res, ref, "max_det %d %s" % (max_det, layout))


@pytest.mark.parametrize("want", [(), ("src_rows",), ("net_boxes",), ("extras",), ("src_rows", "extras"), ("net_boxes", "extras")])
def test_each_optional_output_may_be_null(hops, want):
    for agnostic in (False, True):
        res, ref = run(hops, "v8xy/counts_65", "channels", agnostic, True, 51, want=want)
        assert sorted(res.full) == sorted(("dets", "counts") + want)
        check(res, ref, "want=%s" % (want,))


# ---- 5. special values ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["rows", "channels"])
@pytest.mark.parametrize("cid", ["v8_classes", "v8_minus_one", "v5/classes", "v5xy/classes", "v8/geometry", "v8xy/geometry_negthr", "v8/ties_zero"])
def test_special_scores_and_boxes(hops, cid, layout):
    for agnostic in (False, True):
        for adjusted in (False, True):
            res, ref = run(hops, cid, layout, agnostic, adjusted, 1)
            check(res, ref, "%s %s" % (cid, layout))
    if cid == "v8_minus_one":
        assert all((d[:, 5] == -1).sum() == 2 and (d[d[:, 5] == -1][:, 4] == -pr.FLT_MAX).all() for d in res.dets)


@pytest.mark.parametrize("layout", ["rows", "channels"])
def test_a_payload_of_nans_keeps_its_bits(hops, layout):
    res, ref = run(hops, "v8/counts_257", layout, False, True, 51, nan_payload=True)
    check(res, ref, layout)       # (assert_same_picks compares the payload as 32-bit words)
    words = np.concatenate([e.reshape(-1) for e in res.extras]).view(np.uint32)
    assert np.isnan(words.view(F)).all() and len(np.unique(words)) > words.size // 2, "distinct NaN bit patterns, quiet and signalling, both signs"
    assert ((words & np.uint32(0x00400000)) == 0).any() and (words >> 31).any() and not (words >> 31).all()


# ---- 6. repeatability -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["rows", "channels"])
def test_three_runs_and_a_dirty_workspace_give_the_same_bytes(hops, layout):
    cid, extra = "v8/counts_1025", 32
    c = dr.cases()[cid]
    n, rows, _ = c.pred.shape
    d = hops.detect_desc(n, rows, c.desc.classes, c.desc.objectness, extra, layout)
    ws = hops.DeviceBuffer(hops.detect_workspace_bytes(d))
    for agnostic in (False, True):
        first, ref = run(hops, cid, layout, agnostic, True, extra)
        check(first, ref, cid)
        fills = [None, None, 0xFF, np.uint32(0x7FC00000)]
        for f in fills:
            if isinstance(f, int):
                ws.fill(f)
            elif f is not None:
                hops._chk(hops._native.hip().si_hip_memcpy_h2d(ws.ptr, np.full(ws.nbytes // 4, f, np.uint32).ctypes.data, ws.nbytes // 4 * 4, None), "h2d")
            again, _ = run(hops, cid, layout, agnostic, True, extra, workspace=ws if f is not None else None)
            for name in first.full:
                assert first.full[name].tobytes() == again.full[name].tobytes(), (layout, agnostic, f, name)


# ---- 7. masks ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", sorted(dr.mask_cases()))
def test_masks_equal_the_rule(hops, cid):
    c = dr.mask_cases()[cid]
    nm = c.protos.shape[3]
    d = hops.detect_mask_desc(c.protos.shape[0], c.protos.shape[1], c.protos.shape[2], nm, c.extras.shape[1], c.extras.shape[2], c.coef_off)
    assert hops.detect_masks_kernel_name(d) == ("detect_masks_kernel<32>" if nm == 32 else "detect_masks_kernel<0>")
    dense = run_masks(hops, cid)
    check_masks(dense, cid, "dense")
    padded = run_masks(hops, cid, proto_pad=5)          # proto_ld > nm, and for nm == 32 the generic form: the same bytes
    assert padded.tobytes() == dense.tobytes()
    if nm == 32:
        d.proto_ld = nm + 5
        assert hops.detect_masks_kernel_name(d) == "detect_masks_kernel<0>"
        assert run_masks(hops, cid, proto_pad=4).tobytes() == dense.tobytes()       # the register form with gaps


# ---- 8. end to end ----------------------------------------------------------------------------------------------------------------------------
def _engine(b, tmp_path, x, tag, forwards=1, **opts):
    from simpleinfer_amd.engine import Engine
    pp, bp = str(tmp_path / (tag + ".pnnx.param")), str(tmp_path / (tag + ".pnnx.bin"))
    b.save(pp, bp)
    e = Engine(outputs_to_host=0, **opts)
    e.load_model(pp, bp)
    e.input(e.input_names()[0], x)
    for _ in range(forwards):
        e.forward()
    outs = []
    for name in e.output_names():
        ptr, on_dev = e.extract_ptr(name)
        assert on_dev, name
        outs.append((ptr, e.extract(name)))
    return e, outs


MODES = [("eager", dict()), ("graph", dict(graph=1)), ("fp16", dict(fp16=1))]


@pytest.mark.parametrize("mode", MODES, ids=[m[0] for m in MODES])
def test_anchorfree_head_end_to_end(hops, tmp_path, mode):
    """build_toy_anchorfree_head: [N, cells, 32] read as box | box score | 11 class scores | a payload of 16, on the engine's device pointer"""
    from simpleinfer_amd import modelgen as mg
    b = mg.build_toy_anchorfree_head()
    x = mg.synth_input((2, 64, 64, 3))
    e, ((ptr, pred),) = _engine(b, tmp_path, x, mode[0], forwards=3 if "graph" in mode[1] else 1, **mode[1])
    assert pred.shape == (2, 320, 32) and pred.dtype == F and np.isfinite(pred).all()
    if "fp16" in mode[1]:      # the graph output of an fp16 engine is fp32 storage: halves read as floats would be nowhere near the fp32 engine's
        _, ((_, ref32),) = _engine(b, tmp_path, x, "f32")
        assert np.abs(pred - ref32).max() < 2e-2 * np.abs(ref32).max()
    with np.errstate(all="ignore"):
        conf = pred[..., 4] * pred[..., 5:16].max(-1)
    thr = F(np.sort(conf.reshape(-1))[-120])
    for agnostic in (False, True):
        desc = dr.Desc(11, 1, 16, "cxcywh", thr, F(0.45), agnostic)
        ref = dr.postprocess(pred, desc, pr._adjust(2))
        assert 2 < ref[1].min() and 50 < ref[1].max() and ref[1].sum() <= 120, "more picks than max_det in one image"
        res = hops.detect_postprocess(None, 11, True, 16, "rows", "cxcywh", thr, 0.45, agnostic, pr._adjust(2), max_det=50,
                                      pred_dev=hops.DeviceBuffer.view(ptr, pred.nbytes), shape=(2, 320), out_fill=hops.ByteFill(SENT), stream=e.stream())
        check(res, ref, "anchorfree %s" % mode[0])


@pytest.mark.parametrize("mode", MODES, ids=[m[0] for m in MODES])
@pytest.mark.parametrize("channels_first", [True, False], ids=["channels", "rows"])
def test_yolov8_seg_end_to_end(hops, tmp_path, channels_first, mode):
    """build_toy_yolov8_seg: both graph outputs stay on the device; detect_postprocess reads the head where the engine left it, detect_masks
    the prototypes and what detect_postprocess wrote"""
    from simpleinfer_amd import modelgen as mg
    nc, nm, size = 5, 32, 64
    b = mg.build_toy_yolov8_seg(2, size, nc, nm, channels_first)
    x = mg.synth_input((2, size, size, 3))
    e, ((hptr, head), (pptr, protos)) = _engine(b, tmp_path, x, mode[0], forwards=3 if "graph" in mode[1] else 1, **mode[1])
    no = 4 + nc + nm
    assert head.shape == ((2, no, 320) if channels_first else (2, 320, no)) and protos.shape == (2, 16, 16, nm), (head.shape, protos.shape)
    if "fp16" in mode[1]:
        _, ((_, h32), (_, p32)) = _engine(b, tmp_path, x, "f32")
        assert np.abs(head - h32).max() < 2e-2 * np.abs(h32).max() and np.abs(protos - p32).max() < 2e-2 * np.abs(p32).max()
    rows_form = np.ascontiguousarray(np.transpose(head, (0, 2, 1))) if channels_first else head
    thr = F(np.sort(rows_form[..., 4:4 + nc].max(-1).reshape(-1))[-200])
    layout = "channels" if channels_first else "rows"
    ratio = F(16) / F(size)
    for agnostic in (False, True):
        ref = dr.postprocess(rows_form, dr.Desc(nc, 0, nm, "cxcywh", thr, F(0.45), agnostic))
        assert 2 < ref[1].min() and ref[1].sum() < 200, "the boxes overlap: real suppression"
        res = hops.detect_postprocess(None, nc, False, nm, layout, "cxcywh", thr, 0.45, agnostic, max_det=6,
                                      pred_dev=hops.DeviceBuffer.view(hptr, head.nbytes), shape=(2, 320), out_fill=hops.ByteFill(SENT), stream=e.stream())
        check(res, ref, "seg %s %s" % (layout, mode[0]))
        planes = hops.detect_masks(None, res, None, None, ratio, ratio, protos_dev=hops.DeviceBuffer.view(pptr, protos.nbytes),
                                   shape=protos.shape, out_fill=SENT, full=True, stream=e.stream())
        want = dr.masks_ref(protos, res.full["extras"], res.full["net_boxes"], res.counts, ratio, ratio)
        for i, w in enumerate(want):
            assert planes[i, :len(w)].tobytes() == w.tobytes() and (planes[i, len(w):] == SENT).all(), (layout, mode[0], agnostic, i)
        assert sum(int(w.sum()) for w in want) > 0, "some mask pixels are set"
