"""GPU: si_hip_detect_obb_postprocess_f32 (include/si_obb.h; simpleinfer_amd/csrc/hip/detect_obb.hip) against the float64 rule of
tests/obb_reference.py.  The kernel decides in fp32, so every input is first held to the margin on the host: no candidate pair has a float64
ProbIoU within M of nms_threshold, and the fp32 restatement of the kernel's arithmetic is within DEV of float64 on it (M = 8 * DEV; DESIGN.md
section 9y).  Inside that, the kept set, its order and every carried value are compared as bytes, into sentinel-filled outputs."""
import ctypes as C

import numpy as np
import pytest

import obb_reference as R

pytestmark = pytest.mark.gpu

F = np.float32
DEV = 1.77e-6            # 1.763e-6 rounded up: the largest |iou(fp32 bd) - iou(float64 bd)| over every candidate pair of every input of this file, measured on the CPU
M = 8 * DEV
SENT32 = np.uint32(0x7B7B7B7B)
PROB, NMS = 0.25, 0.45
COUNTS = (0, 1, 63, 64, 65, 255, 256, 257, 1023, 1025, 2100)
SEED = 11
MARGINS = {}             # an input's (deviation, gap), computed once however many launches it gets


@pytest.fixture(scope="module")
def hops(gpu):
    from simpleinfer_amd import hipops
    return hipops


def launch(hops, pred, classes, extra=1, angle_off=0, layout="rows", agnostic=False, max_det=None, adjust=None, nms=NMS, **kw):
    """the margin on the host, one call into sentinel-filled outputs, and the whole result against the rule; returns the result"""
    key = (pred.tobytes(), classes, extra, angle_off, nms)
    if key not in MARGINS:
        MARGINS[key] = R.deviation_and_gap(pred, classes, extra, angle_off, PROB, nms)
    dev, gap = MARGINS[key]
    assert dev <= DEV and gap > M, (dev, gap)
    res = hops.detect_obb_postprocess(pred if layout == "rows" else np.transpose(pred, (0, 2, 1)), classes, extra, angle_off, layout=layout,
                                      prob_threshold=PROB, nms_threshold=nms, agnostic=agnostic, adjust=adjust, max_det=max_det,
                                      out_fill=hops.ByteFill(0x7B), **kw)
    outs, counts = R.postprocess(pred, classes, extra, angle_off, PROB, nms, agnostic, res.max_det, adjust)
    assert list(res.counts) == list(counts)
    for b, (obbs, rows, extras) in enumerate(outs):
        assert list(res.src_rows[b]) == list(rows), b
        assert res.obbs[b].tobytes() == obbs.tobytes() and res.extras[b].tobytes() == np.ascontiguousarray(extras).tobytes(), b
        for name in ("obbs", "src_rows", "extras"):
            assert (np.ascontiguousarray(res.full[name][b, len(rows):]).view(np.uint32) == SENT32).all(), (name, b)
    return res


def rows_of(boxes, conf, label, classes=1, extra=1, angle_off=0):
    """prediction rows [1][k][ne] of boxes [k][5] with the given confidences and labels"""
    boxes = np.asarray(boxes, F).reshape(-1, 5)
    pred = np.zeros((1, len(boxes), 4 + classes + extra), F)
    pred[0, :, :4] = boxes[:, :4]
    pred[0, np.arange(len(boxes)), 4 + np.asarray(label)] = np.asarray(conf, F)
    pred[0, :, 4 + classes + angle_off] = boxes[:, 4]
    return pred


@pytest.mark.parametrize("layout", ["rows", "channels"])
@pytest.mark.parametrize("count", COUNTS)
def test_keep_decisions_and_order(hops, count, layout):
    """two images with different counts; the wave, the workgroup and one, two and three LDS tiles"""
    for classes in (1, 3):
        pred = R.case(SEED, (count, 2 * count // 3 + 1), classes)
        for agnostic in (False, True):
            launch(hops, pred, classes, layout=layout, agnostic=agnostic)


@pytest.mark.parametrize("layout", ["rows", "channels"])
def test_strided_views_payload_and_max_det(hops, layout):
    """NaN-filled gaps between rows / channels and images, the angle at payload element 2 of 4, max_det below the pick count"""
    pred = R.case(SEED, (257, 90), 3, 4, 2)
    n, rows, ne = pred.shape
    ld = ne + 3 if layout == "rows" else rows + 5
    image_ld = (rows if layout == "rows" else ne) * ld + 11
    res = launch(hops, pred, 3, 4, 2, layout=layout, max_det=40, ld=ld, image_ld=image_ld, pred_off=1)
    assert min(res.counts) > 40 and [len(o) for o in res.obbs] == [40, 40]


def test_crossing_pair_is_kept_where_the_axis_aligned_rule_drops_it(hops):
    pred = rows_of([[50, 50, 100, 10, 0.0], [50, 50, 100, 10, np.pi / 2]], [0.9, 0.8], [0, 0])
    res = launch(hops, pred, 1)
    assert list(res.counts) == [2] and list(res.src_rows[0]) == [0, 1]
    plain = hops.detect_postprocess(pred, 1, extra=1, prob_threshold=PROB, nms_threshold=NMS)
    assert list(plain.counts) == [1], "the same rows through the axis-aligned entry: one rectangle twice"


def test_half_turn_is_the_same_box(hops):
    pred = rows_of([[50, 50, 80, 30, 0.4], [50, 50, 80, 30, 0.4 + np.pi], [300, 50, 80, 30, 0.4 + np.pi]], [0.9, 0.8, 0.7], [0, 0, 0])
    assert list(launch(hops, pred, 1).src_rows[0]) == [0, 2]


def test_a_dropped_box_still_drops(hops):
    """the matrix rule: A drops B, B overlaps C, A does not -- C goes (a greedy chain would keep it); under another label it stays"""
    boxes = [[0, 0, 100, 20, 0], [40, 0, 100, 20, 0], [80, 0, 100, 20, 0]]
    assert list(launch(hops, rows_of(boxes, [0.9, 0.8, 0.7], [0, 0, 0]), 1).src_rows[0]) == [0]
    pred = rows_of(boxes, [0.9, 0.8, 0.7], [0, 0, 1], classes=2)
    assert list(launch(hops, pred, 2).src_rows[0]) == [0, 2] and list(launch(hops, pred, 2, agnostic=True).src_rows[0]) == [0]


def test_same_bytes_twice_and_alone(hops):
    pred = R.case(SEED, (257, 172), 3)
    a, b = (launch(hops, pred, 3) for _ in range(2))
    assert all(a.full[k].tobytes() == b.full[k].tobytes() for k in a.full)
    for i in range(2):
        alone = launch(hops, pred[i:i + 1], 3)
        assert all(alone.full[k][0].tobytes() == a.full[k][i].tobytes() for k in a.full), i


def test_degenerate_boxes_and_adjust(hops):
    """w = 0 at angle 0 (an exact zero covariance term): the later one on the same line goes, the one beside it stays; a NaN centre drops the
    later boxes of ITS label and only those, and is dropped itself unless first; adjust in fp32 with IEEE division, nothing clipped"""
    boxes = [[10, 10, 0, 40, 0], [10, 10, 0, 40, 0], [25, 10, 0, 40, 0], [200, 200, 60, 20, 0.3]]
    assert list(launch(hops, rows_of(boxes, [0.9, 0.8, 0.7, 0.6], [0] * 4), 1).src_rows[0]) == [0, 2, 3]
    boxes = [[100, 100, 60, 20, 0.3], [np.nan, 5, 60, 20, 0.1], [900, 900, 60, 20, 0.2], [500, 500, 60, 20, 0.2], [np.nan, 7, 60, 20, 0.1], [700, 7, 60, 20, 0.1]]
    pred = rows_of(boxes, [0.9, 0.85, 0.8, 0.7, 0.6, 0.5], [0, 1, 1, 0, 2, 2], classes=3)
    assert list(launch(hops, pred, 3).src_rows[0]) == [0, 1, 3, 4]
    assert list(launch(hops, pred, 3, agnostic=True).src_rows[0]) == [0]
    pred = R.case(SEED, (65, 44), 3)
    res = launch(hops, pred, 3, adjust=np.asarray([[13, 7.5, 0.618, 640, 480], [0, 40, 1.7, 64, 48]], F))
    assert (res.obbs[0][:, 0] < 0).any() or (res.obbs[0][:, 0] > 640).any(), "a centre outside the image stays where it is"


def test_refusals_without_a_launch(hops, native_libs):
    """every refusal happens before any device call: the addresses are made up"""
    H, _ = native_libs
    from simpleinfer_amd import _native
    P, A, D, N, W = (C.c_void_p((j + 1) << 24) for j in range(5))

    def call(d, pred=P, out=(D, N, None, None), ws=W, ws_bytes=1 << 40):
        o = _native.SiDetectObbOut(*[p.value if p is not None else None for p in out])
        return H.si_hip_detect_obb_postprocess_f32(C.byref(d), pred, A, C.byref(o), ws, ws_bytes, None)

    def desc(**kw):
        args = dict(n=2, rows=300, classes=15, extra=1, angle_off=0)
        args.update(kw)
        return hops.detect_obb_desc(**args)

    need = hops.detect_obb_workspace_bytes(desc())
    plain = hops.detect_workspace_bytes(hops.detect_desc(2, 300, 15, extra=1))
    assert need == plain + sum((2 * 300 * b + 255) // 256 * 256 for b in (32, 16, 4)), "the general layout, then record / raw / keep, each 256-byte aligned"
    assert call(desc(), ws_bytes=need - 1) == -1 and call(desc(), pred=None) == -1 and call(desc(), ws=None) == -1
    assert call(desc(), out=(D, None, None, None)) == -1 and call(desc(), out=(None, N, None, None)) == -1
    assert call(desc(), pred=C.c_void_p(P.value + 2)) == -1 and H.si_hip_detect_obb_postprocess_workspace_bytes(None) == 0
    bad = [dict(n=0), dict(rows=0), dict(classes=0), dict(extra=0), dict(angle_off=-1), dict(angle_off=1), dict(extra=4, angle_off=4), dict(max_det=-1),
           dict(nms_threshold=0.0), dict(nms_threshold=1.5), dict(nms_threshold=float("nan")), dict(layout=2), dict(ld=19), dict(image_ld=299 * 20 + 19)]
    for kw in bad:
        assert call(desc(**kw)) == -1 and hops.detect_obb_workspace_bytes(desc(**kw)) == 0, kw
    for kw in (dict(n=65536, rows=4), dict(classes=124), dict(rows=1 << 28, layout="channels"), dict(n=65535, rows=1 << 20, image_ld=1 << 31)):
        assert call(desc(**kw)) == -2 and hops.detect_obb_workspace_bytes(desc(**kw)) == 0, kw
    assert hops.detect_obb_workspace_bytes(desc(nms_threshold=1.0, max_det=0, extra=4, angle_off=3)) > 0
