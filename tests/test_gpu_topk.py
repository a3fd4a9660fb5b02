"""GPU: si_hip_detect_topk_postprocess_f32 (include/si_topk.h; simpleinfer_amd/csrc/hip/detect_topk.hip) against the rule restated here:
candidates with score > prob_threshold, ordered by np.lexsort((flat index, -score)) on the fp32 values, cut at max_det.  The box arithmetic is
tests/detect_reference.py's.  Selection is exact: every comparison is on bits, into sentinel-filled outputs, and pred's gaps hold NaN."""
import itertools

import numpy as np
import pytest

import detect_reference as dr

pytestmark = pytest.mark.gpu
F = np.float32
SENT32 = np.uint32(0x7B7B7B7B)
CHUNK = 256   # csrc/hip/detect_topk_plan.h kChunkRows


@pytest.fixture(scope="module")
def hops(gpu):
    from simpleinfer_amd import hipops
    return hipops


def topk_ref(pred, classes, extra, fmt, thr, multi_label, max_det, adjust):
    """pred [n][rows][ne] -> (Picks per image cut at max_det, uncapped counts)"""
    outs, counts = [], []
    for b, p in enumerate(pred):
        _, box, label, score = dr.filter_rows(p, dr.Desc(classes, 0, extra, fmt, prob_thr=F(-np.inf)))     # every row: box, first maximum
        row = np.arange(len(p))
        if multi_label:
            score = np.ascontiguousarray(p[:, 4:4 + classes]).reshape(-1)
            row, label = np.arange(score.size) // classes, (np.arange(score.size) % classes).astype(np.int32)
        with np.errstate(invalid="ignore"):
            f = np.nonzero(score > F(thr))[0]
        f = f[np.lexsort((f, -score[f]))]
        counts.append(len(f))
        f = f[:max_det]
        r = row[f].astype(np.int32)
        outs.append(dr.Picks(dr.finish(box[r], label[f], score[f], None if adjust is None else adjust[b]), r, np.ascontiguousarray(box[r]),
                             np.ascontiguousarray(p[r, 4 + classes:])))
    return outs, np.asarray(counts, np.int32)


def run(hops, pred, classes, extra=0, layout="rows", fmt="cxcywh", thr=0.25, multi_label=1, max_det=300, adjust=None, pad=(3, 5), **kw):
    """one launch on padded storage into sentinel-filled outputs, the whole result against the rule; returns the result"""
    n, rows, ne = pred.shape
    ld = (rows if layout == "channels" else ne) + pad[0]
    image_ld = (ne if layout == "channels" else rows) * ld + pad[1]
    res = hops.detect_topk_postprocess(pred if layout == "rows" else dr.to_channels(pred), classes, extra, layout, fmt, thr, multi_label, adjust,
                                       max_det, ld=ld, image_ld=image_ld, out_fill=hops.ByteFill(0x7B), **kw)
    ref = topk_ref(pred, classes, extra, fmt, thr, multi_label, max_det, adjust)
    dr.assert_same_picks(res, ref, max_det, "topk")
    for b in range(n):      # the confidence keeps the score's own bits, and nothing behind the last detection is written
        assert np.array_equal(res.dets[b][:, 4].view(np.uint32), ref[0][b].dets[:, 4].view(np.uint32))
        for name in ("dets", "src_rows", "net_boxes", "extras"):
            assert (np.ascontiguousarray(res.full[name][b, len(res.dets[b]):]).view(np.uint32) == SENT32).all(), (name, b)
    return res


def make_pred(n, rows, classes, extra, seed, fmt="cxcywh"):
    """scores on a grid of 1 / 64 (ties everywhere) with a fifth of them off it; boxes of positive size; a NaN in the payload"""
    r = np.random.Generator(np.random.Philox(seed))
    p = np.empty((n, rows, 4 + classes + extra), F)
    p[..., :2] = r.uniform(50, 500, (n, rows, 2))
    p[..., 2:4] = r.uniform(5, 90, (n, rows, 2)) + (p[..., :2] if fmt == "xyxy" else 0)
    s = r.integers(0, 64, (n, rows, classes)) / 64.0
    p[..., 4:4 + classes] = np.where(r.random(s.shape) < 0.2, r.random(s.shape), s)
    p[..., 4 + classes:] = r.standard_normal((n, rows, extra))
    if extra:
        p[0, 0, -1] = np.nan
    return p


def _cases():
    out = []
    for i, (rows, classes) in enumerate(itertools.product((1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 1500), (1, 3, 80))):
        layouts, fmts = ("rows", "channels"), ("cxcywh", "xyxy")
        out.append((rows, classes, (1, 7, 300)[i % 3], 1 + 2 * (i % 2), layouts[i % 2], fmts[(i // 2) % 2], 1, bool((i // 3) % 2)))
        if classes > 1:     # the other layout, one candidate per row
            out.append((rows, classes, (7, 300, 1)[i % 3], 3 - 2 * (i % 2), layouts[1 - i % 2], fmts[(i // 3) % 2], 0, bool(i % 2)))
    return out


@pytest.mark.parametrize("rows,classes,max_det,n,layout,fmt,multi_label,adjusted", _cases())
def test_sizes_layouts_and_modes(hops, rows, classes, max_det, n, layout, fmt, multi_label, adjusted):
    extra = 5 * (rows % 2)
    pred = make_pred(n, rows, classes, extra, rows * 100 + classes, fmt)
    adjust = np.asarray([[12.0, 8.0, 0.75 + 0.1 * b, 640.0, 480.0] for b in range(n)], F) if adjusted else None
    res = run(hops, pred, classes, extra, layout, fmt, 0.25, multi_label, max_det, adjust)
    assert hops.LAST_KERNEL_NAME["si_hip_detect_topk"] == "topk_hist_kernel<SI_DETECT_%s>" % layout.upper() and len(res.counts) == n


ROWS, CLASSES, K = 600, 3, 7      # three chunks; K = max_det of the hard sets
BITS = lambda u: np.asarray(u, np.uint32).view(F)


def _hard(name):
    """(scores [ROWS][CLASSES], threshold, expected count or None)"""
    r = np.random.Generator(np.random.Philox(5))
    s = np.full((ROWS, CLASSES), 0.125, F)
    spread = np.asarray([3, 100, 255, 256, 257, 400, 511, 512, 599, 10])      # rows in all three chunks
    if name == "all_equal":
        return np.full_like(s, 0.5), 0.25, ROWS * CLASSES
    if name.startswith("above"):
        k = K + int(name[5:])
        s[spread[:k], np.arange(k) % CLASSES] = 0.5 + np.arange(k) / 64.0
        return s, 0.25, k
    if name == "straddle":      # four keys above the group, six equal ones in three chunks: three of them are taken, the lowest flat indices
        s[spread[:4], 0] = [0.9, 0.8, 0.7, 0.6]
        s[[599, 300, 10, 580, 301, 550], [0, 2, 1, 1, 0, 2]] = 0.5
        return s, 0.25, 10
    if name == "low_bits":
        return BITS(0x3F000000 + r.integers(0, 1024, s.shape)), 0.25, s.size
    if name == "zeros":
        return np.where(r.random(s.shape) < 0.5, F(-0.0), F(0.0)).astype(F), -1.0, s.size
    if name == "negative":
        return -r.random(s.shape).astype(F), -0.5, None
    if name == "specials":
        s = r.standard_normal(s.shape).astype(F)
        s[r.random(s.shape) < 0.3] = np.nan
        s[spread[:3], 1], s[spread[3:6], 2] = np.inf, -np.inf
        return s, -np.inf, int((s > -np.inf).sum())
    assert name == "none"
    return s, 0.25, 0


@pytest.mark.parametrize("layout", ["rows", "channels"])
@pytest.mark.parametrize("name", ["all_equal", "above-1", "above+0", "above+1", "straddle", "low_bits", "zeros", "negative", "specials", "none"])
def test_hard_score_sets(hops, name, layout):
    scores, thr, count = _hard(name)
    pred = make_pred(1, ROWS, CLASSES, 0, 9)
    pred[0, :, 4:] = scores
    res = run(hops, pred, CLASSES, 0, layout, thr=thr, multi_label=1, max_det=K)
    assert count is None or res.counts[0] == count
    if name == "straddle":
        assert list(res.src_rows[0]) == [3, 100, 255, 256, 10, 300, 301]
    run(hops, pred, CLASSES, 0, layout, thr=thr, multi_label=0, max_det=K)


def test_repeatable_from_a_poisoned_workspace_and_alone_as_in_a_batch(hops):
    pred = make_pred(3, 700, 3, 2, 21)
    d = hops.detect_topk_desc(3, 700, 3, 2, "channels", max_det=40, ld=703, image_ld=9 * 703 + 5)
    ws = hops.DeviceBuffer(hops.detect_topk_workspace_bytes(d))
    ws.fill(0xFF)
    first = run(hops, pred, 3, 2, "channels", max_det=40, workspace=ws)
    again = run(hops, pred, 3, 2, "channels", max_det=40, workspace=ws)
    assert all(first.full[k].tobytes() == again.full[k].tobytes() for k in first.full)
    for b in range(3):
        alone = run(hops, pred[b:b + 1], 3, 2, "channels", max_det=40)
        assert all(alone.full[k][0].tobytes() == first.full[k][b].tobytes() for k in ("dets", "src_rows", "net_boxes", "extras"))


@pytest.mark.parametrize("layout", ["rows", "channels"])
def test_outputs_are_the_nms_entrys_where_both_rules_pick_the_same_rows(hops, layout):
    """multi_label = 0 against si_hip_detect_postprocess_f32 with nms_threshold = 1 (nothing suppressed), on distinct scores off the threshold"""
    n, rows, classes, extra = 2, 300, 4, 6
    pred = make_pred(n, rows, classes, extra, 33)
    r = np.random.Generator(np.random.Philox(34))
    pred[..., 4:4 + classes] = (r.permutation(n * rows * classes).reshape(n, rows, classes) + 0.5) / (n * rows * classes)
    adjust = np.asarray([[12.0, 8.0, 0.8, 640.0, 480.0]] * n, F)
    got = run(hops, pred, classes, extra, layout, multi_label=0, max_det=50, adjust=adjust)
    old = hops.detect_postprocess(pred if layout == "rows" else dr.to_channels(pred), classes, False, extra, layout, nms_threshold=1.0, adjust=adjust,
                                  max_det=50)
    assert list(got.counts) == list(old.counts) and min(got.counts) > 50
    for k in ("dets", "src_rows", "net_boxes", "extras"):
        assert got.full[k].tobytes() == old.full[k].tobytes(), k
